// sdrhip.cpp -- host side of libsdrhip.so (include/sdrhip.h): the context, its options, counters, timers and pinned allocator.
// C++11-style host code calling HIP; no torch, no oracle, no CPU fallback: without a
// usable GPU every compute entry point fails with SDRHIP_EDEVICE.
#include "sdrhip_host.h"
#include "gf256.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace sdrhip;

namespace {
thread_local std::string g_err;
}

namespace sdrhip {

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

} // namespace sdrhip

extern "C" const char *sdrhip_last_error(void) { return g_err.c_str(); }

extern "C" int sdrhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace sdrhip {
static void ctx_free(sdrhip_ctx *c);
static void drop_kernel_events(sdrhip_ctx *c)
{
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (int k = 0; k < SDRHIP_KCLASSES; ++k) {
        for (auto &pr : c->kev[k]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        c->kev[k].clear();
    }
}
}

extern "C" int sdrhip_ctx_create(int device, void *hip_stream, sdrhip_ctx **out)
{
    if (!out) return fail(SDRHIP_EINVAL, "ctx_create: out is NULL");
    *out = nullptr;
    int n = sdrhip_device_count();
    if (n <= 0) return fail(SDRHIP_EDEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(SDRHIP_EINVAL, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    sdrhip_ctx *c = new (std::nothrow) sdrhip_ctx();
    if (!c) return fail(SDRHIP_ENOMEM, "out of host memory");
    c->device = device;
    c->stream = static_cast<hipStream_t>(hip_stream);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        // the environment is read here, once (getenv is not safe against a concurrent setenv): later changes go through
        // sdrhip_ctx_set_option()
        static const char *const keys[][2] = {{"SDRHIP_DECIM_PATH", "decim_path"}, {"SDRHIP_MFMA_SPAN", "mfma_span"}, {"SDRHIP_MFMA_MIN", "mfma_min"},
                                              {"SDRHIP_INTERP_PATH", "interp_path"}, {"SDRHIP_INTERP_SPAN", "interp_span"}, {"SDRHIP_RX_FUSED", "rx_fused"}, {"SDRHIP_RX_DIRECT", "rx_direct"},
                                              {"SDRHIP_DEC_PATH", "dec_path"}, {"SDRHIP_ENC_PATH", "enc_path"}, {"SDRHIP_ENC_MIN_ROWS", "enc_min_rows"}, {"SDRHIP_MFMA_RING", "mfma_ring"}, {"SDRHIP_TX_OVERLAP", "tx_overlap"}, {"SDRHIP_RX_WINDOW", "rx_window"}, {"SDRHIP_FEC_STAGGER", "fec_stagger"}, {"SDRHIP_FEC_STAGGER_MOD", "fec_stagger_mod"}, {"SDRHIP_DEC_PLAN", "dec_plan"}, {"SDRHIP_TX_GATHER", "tx_gather"}, {"SDRHIP_ENC_UNITS", "enc_units"}, {"SDRHIP_ENC_FORM", "enc_form"}};
        for (size_t i = 0; i < sizeof(keys) / sizeof(keys[0]); ++i)
            if (const char *v = getenv(keys[i][0])) (void)sdrhip_ctx_set_option(c, keys[i][1], v);
    }
    std::vector<uint8_t> tab(256 * 32);
    gf_build_tables(tab.data());
    if (hipMalloc(reinterpret_cast<void **>(&c->gf_tab), tab.size()) != hipSuccess) { c->gf_tab = nullptr; ctx_free(c); return fail(SDRHIP_ENOMEM, "hipMalloc gf tables"); }
    if (hipMemcpy(c->gf_tab, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess) { ctx_free(c); return fail(SDRHIP_EDEVICE, "upload gf tables"); }
    std::vector<uint8_t> em(128 * 128);
    cm256_encode_matrix(128, 128, em.data());
    if (hipMalloc(reinterpret_cast<void **>(&c->enc_matrix), em.size()) != hipSuccess ||
        hipMemcpy(c->enc_matrix, em.data(), em.size(), hipMemcpyHostToDevice) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "upload encode matrix"); }
    std::vector<uint8_t> kl(8 * 81 * 32);
    cm256_karatsuba_leaf_tables(kl.data());
    if (hipMalloc(reinterpret_cast<void **>(&c->enc_leaves), kl.size()) != hipSuccess ||
        hipMemcpy(c->enc_leaves, kl.data(), kl.size(), hipMemcpyHostToDevice) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "upload encoder constants"); }
    {
        std::vector<uint8_t> ft((size_t)CM256_FFT_TABLES * 32);
        cm256_fft_tables(ft.data());
        if (hipMalloc(reinterpret_cast<void **>(&c->enc_fft), ft.size()) != hipSuccess ||
            hipMemcpy(c->enc_fft, ft.data(), ft.size(), hipMemcpyHostToDevice) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "upload encoder FFT constants"); }
    }
    {
        const GF256 &g = gf();
        uint8_t el[1024];
        memcpy(el, g.exp, 512);
        memcpy(el + 512, g.log, 512);
        if (hipMalloc(reinterpret_cast<void **>(&c->gf_explog), sizeof(el)) != hipSuccess ||
            hipMemcpy(c->gf_explog, el, sizeof(el), hipMemcpyHostToDevice) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "upload GF(256) exp/log tables"); }
    }
    if (hipMalloc(reinterpret_cast<void **>(&c->dec_stats), 64) != hipSuccess ||
        hipMemset(c->dec_stats, 0, 64) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "hipMalloc decoder counters"); }
    if (hipMalloc(reinterpret_cast<void **>(&c->decim_dump), 4096) != hipSuccess) { c->decim_dump = nullptr; ctx_free(c); return fail(SDRHIP_ENOMEM, "hipMalloc decimator scratch"); }
    if (hipMalloc(reinterpret_cast<void **>(&c->fused_roles), SDRHIP_FUSED_ROLE_WORDS * 4) != hipSuccess ||
        hipMemset(c->fused_roles, 0, SDRHIP_FUSED_ROLE_WORDS * 4) != hipSuccess) { ctx_free(c); return fail(SDRHIP_ENOMEM, "hipMalloc role table"); }
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) { ctx_free(c); return fail(SDRHIP_EDEVICE, "hipEventCreate"); }
    *out = c;
    return SDRHIP_OK;
}

namespace sdrhip {
int ctx_stream2(sdrhip_ctx *c, hipStream_t *out)
{
    if (!c->stream2) {
        // lowest priority: when both streams have workgroups to place, the first stream's (the long kernel) go first
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = 0;
        if (hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo) != hipSuccess) {
            c->stream2 = nullptr;
            return fail(SDRHIP_EDEVICE, "hipStreamCreate (second stream)");
        }
    }
    *out = c->stream2;
    return SDRHIP_OK;
}
void ctx_retain(sdrhip_ctx *c) { c->refs.fetch_add(1); }
void ctx_release(sdrhip_ctx *c)
{
    if (c->refs.fetch_sub(1) == 1 && c->dying) ctx_free(c);
}
} // namespace sdrhip

// Handles created on a context keep it alive: destroying the context first only marks it; the
// last handle to go frees it (destruction order is then irrelevant, e.g. under a garbage collector).
extern "C" void sdrhip_ctx_destroy(sdrhip_ctx *c)
{
    if (!c || c->dying.exchange(true)) return;
    if (c->refs.load() == 0) ctx_free(c);
}

// Kernel-path knobs (tests and tools; the defaults come from the environment at creation).  Unknown keys / values: EINVAL.
extern "C" int sdrhip_ctx_set_option(sdrhip_ctx *c, const char *key, const char *value)
{
    if (!c || !key || !value) return fail(SDRHIP_EINVAL, "ctx_set_option: NULL argument");
    sdrhip::CtxLock lock_(c);
    const std::string k(key), v(value);
    char *end = nullptr;
    const unsigned long long num = strtoull(value, &end, 10);
    const bool isnum = *value && end && !*end;
    if (k == "decim_path") {
        if (v == "auto") c->opt.decim_path = DECIM_PATH_AUTO;
        else if (v == "valu") c->opt.decim_path = DECIM_PATH_VALU;
        else if (v == "mfma") c->opt.decim_path = DECIM_PATH_MFMA;
        else return fail(SDRHIP_EINVAL, "ctx_set_option: decim_path must be auto, valu or mfma");
    } else if (k == "interp_path") {
        if (v == "auto") c->opt.interp_wave = CtxOptions().interp_wave;
        else if (v == "valu") c->opt.interp_wave = 0;
        else if (v == "wave") c->opt.interp_wave = 1;
        else return fail(SDRHIP_EINVAL, "ctx_set_option: interp_path must be auto, valu or wave");
    } else if (k == "mfma_span" && isnum) c->opt.mfma_span = (size_t)num;
    else if (k == "mfma_min" && isnum) c->opt.mfma_min = (size_t)num;
    else if (k == "interp_span" && isnum) c->opt.interp_span = (size_t)num;
    else if (k == "rx_fused" && isnum && num <= 3) c->opt.rx_fused = (int)num;
    else if (k == "rx_fused" && v == "overlap") c->opt.rx_fused = 3;
    else if (k == "rx_direct" && isnum && num <= 1) c->opt.rx_direct = (int)num;
    else if (k == "rx_window" && isnum && num <= 8) c->opt.rx_window = (int)num;
    else if (k == "mfma_ring" && isnum && num >= 2 && num <= 4) c->opt.mfma_ring = (int)num;
    else if (k == "tx_overlap" && isnum && num <= 1) c->opt.tx_overlap = (int)num;
    else if (k == "fec_stagger" && isnum && num <= 64) c->opt.fec_stagger = (int)num;
    else if (k == "fec_stagger_mod" && isnum && num <= 116) c->opt.fec_stagger_mod = (int)num;
    else if (k == "tx_gather" && isnum && num <= 1) c->opt.tx_gather = (int)num;
    else if (k == "dec_plan") {
        if (v == "fused") c->opt.dec_fused_plan = 1;
        else if (v == "kernel") c->opt.dec_fused_plan = 0;
        else return fail(SDRHIP_EINVAL, "ctx_set_option: dec_plan must be fused or kernel");
    }
    else if (k == "enc_min_rows" && isnum && num >= 1 && num <= 32) c->opt.enc_min_rows = (int)num;
    else if (k == "enc_units" && (v == "frame" || v == "half")) c->opt.enc_half = v == "half";
    else if (k == "enc_form" && (v == "bitslice" || v == "table")) c->opt.enc_bitslice = v == "bitslice";
    else if (k == "enc_path") {
        if (v == "fft") c->opt.enc_fft = 1;
        else if (v == "karatsuba") c->opt.enc_fft = 0;
        else return fail(SDRHIP_EINVAL, "ctx_set_option: enc_path must be fft or karatsuba");
    } else if (k == "dec_path") {
        if (v == "syndrome") c->opt.dec_syndrome = 1;
        else if (v == "dense") c->opt.dec_syndrome = 0;
        else return fail(SDRHIP_EINVAL, "ctx_set_option: dec_path must be syndrome or dense");
    } else if (k == "dec_max_rows" && isnum && num >= 1 && num <= 128) { c->opt.dec_max_rows = (int)num; c->opt.dec_auto = 0; }
    else if (k == "dec_max_rows" && v == "auto") { c->opt.dec_max_rows = 128; c->opt.dec_auto = 1; } // (whoever reads the number sees 128: auto is decided per frame, fec_decode_device)
    else if (k == "dec_strict" && isnum && num <= 1) c->opt.dec_strict = (int)num;
    else if (k == "ktime_stride" && isnum && num >= 1 && num <= 1024) { c->ktime_stride = (int)num; for (int i = 0; i < SDRHIP_KCLASSES; ++i) c->ktime_stride_cls[i] = 0; }
    else if (k == "ktime_stride_class") { // "<class>:<stride>": this kernel class only (e.g. the roofline kernel on every launch, the others on every 4th)
        int cls = -1, st = 0;
        if (sscanf(value, "%d:%d", &cls, &st) != 2 || cls < 0 || cls >= SDRHIP_KCLASSES || st < 1 || st > 1024) return fail(SDRHIP_EINVAL, "ctx_set_option: ktime_stride_class takes <class 0..4>:<stride 1..1024>");
        c->ktime_stride_cls[cls] = st;
    }
    else return fail(SDRHIP_EINVAL, "ctx_set_option: unknown key or malformed value: %s=%s", key, value);
    return SDRHIP_OK;
}

// Event counters: kept on the device (read = one stream synchronisation + a 4-byte copy), the host-link byte counts on the host.
extern "C" int sdrhip_ctx_get_counter(sdrhip_ctx *c, const char *key, uint64_t *value)
{
    if (!c || !key || !value) return fail(SDRHIP_EINVAL, "ctx_get_counter: NULL argument");
    sdrhip::CtxLock lock_(c);
    if (std::string(key) == "h2d_bytes") { *value = c->h2d_bytes; return SDRHIP_OK; }
    if (std::string(key) == "d2h_bytes") { *value = c->d2h_bytes; return SDRHIP_OK; }
    const bool shadow = std::string(key) == "fecbuf_shadow_mismatch"; // (streams whose classify pass disagreed with the host's shadow)
    const bool deferred = std::string(key) == "dec_deferred"; // (frames the one-launch decoder handed to the safe chain under dec_max_rows = auto)
    if (std::string(key) != "dec_rows_exceeded" && !shadow && !deferred) return fail(SDRHIP_EINVAL, "ctx_get_counter: unknown key: %s", key);
    HIP_TRY(hipSetDevice(c->device));
    unsigned v = 0;
    HIP_TRY(link_copy(c, &v, c->dec_stats + (shadow ? DEC_STATS_SHADOW_MISMATCH : deferred ? DEC_STATS_DEFERRED : 0), sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *value = v;
    return SDRHIP_OK;
}

int sdrhip::enc128_min_rows(const sdrhip_ctx *c) { return c->opt.enc_fft ? c->opt.enc_min_rows : ENC128_MIN_ROWS; }

static void sdrhip::ctx_free(sdrhip_ctx *c)
{
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    drop_kernel_events(c);
    c->in.release(); c->out.release(); c->aux.release(); c->aux3.release();
    if (c->gf_tab) (void)hipFree(c->gf_tab);
    if (c->enc_matrix) (void)hipFree(c->enc_matrix);
    if (c->enc_leaves) (void)hipFree(c->enc_leaves);
    if (c->enc_fft) (void)hipFree(c->enc_fft);
    if (c->decim_dump) (void)hipFree(c->decim_dump);
    if (c->fused_roles) (void)hipFree(c->fused_roles);
    if (c->gf_explog) (void)hipFree(c->gf_explog);
    if (c->dec_stats) (void)hipFree(c->dec_stats);
    c->dec_plan.release();
    c->pin.release();
    c->zin.release(); c->zout.release();
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
}

extern "C" int sdrhip_ctx_synchronize(sdrhip_ctx *c)
{
    if (!c) return fail(SDRHIP_EINVAL, "ctx is NULL");
    sdrhip::CtxLock lock_(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
    return SDRHIP_OK;
}

extern "C" int sdrhip_ctx_timing_begin(sdrhip_ctx *c)
{
    if (!c) return fail(SDRHIP_EINVAL, "ctx is NULL");
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return SDRHIP_OK;
}

extern "C" int sdrhip_ctx_timing_end(sdrhip_ctx *c, float *ms)
{
    if (!c || !ms) return fail(SDRHIP_EINVAL, "ctx/ms is NULL");
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return SDRHIP_OK;
}

extern "C" int sdrhip_ctx_kernel_timing(sdrhip_ctx *c, int enable)
{
    if (!c) return fail(SDRHIP_EINVAL, "ctx is NULL");
    sdrhip::CtxLock lock_(c);
    c->ktime_on = enable != 0;
    for (int i = 0; i < SDRHIP_KCLASSES; ++i) c->ktime_seen[i] = 0;
    if (!enable) drop_kernel_events(c); // pairs nobody read
    return SDRHIP_OK;
}

extern "C" int sdrhip_ctx_kernel_timing_read(sdrhip_ctx *c, int cls, double *total_ms, unsigned *launches)
{
    if (!c || cls < 0 || cls >= SDRHIP_KCLASSES || !total_ms || !launches) return fail(SDRHIP_EINVAL, "kernel_timing_read: bad argument");
    sdrhip::CtxLock lock_(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
    double sum = 0;
    unsigned n = 0;
    for (auto &pr : c->kev[cls]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { sum += ms; ++n; }
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    c->kev[cls].clear();
    *total_ms = sum;
    *launches = n;
    return SDRHIP_OK;
}

// ------------------------------------------------------------------------------ pinned host memory
namespace {
// memory handed out by sdrhip_host_alloc: pinned, usable in place
struct HostRange { const char *p; size_t n; };
std::mutex g_host_mtx;
std::vector<HostRange> g_host_ranges;
} // namespace
namespace sdrhip {
bool host_is_pinned(const void *p, size_t n)
{
    std::lock_guard<std::mutex> g(g_host_mtx);
    const char *c = static_cast<const char *>(p);
    for (const HostRange &r : g_host_ranges)
        if (c >= r.p && c + n <= r.p + r.n) return true;
    return false;
}
} // namespace sdrhip

extern "C" void *sdrhip_host_alloc(sdrhip_ctx *c, size_t bytes)
{
    if (!c || bytes == 0) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)fail(SDRHIP_ENOMEM, "hipHostMalloc(%zu) failed", bytes); return nullptr; }
    std::lock_guard<std::mutex> g(g_host_mtx);
    g_host_ranges.push_back(HostRange{static_cast<const char *>(p), bytes});
    return p;
}

extern "C" void sdrhip_host_free(sdrhip_ctx *c, void *p)
{
    if (!p) return;
    (void)c;
    {
        std::lock_guard<std::mutex> g(g_host_mtx);
        for (size_t i = 0; i < g_host_ranges.size(); ++i)
            if (g_host_ranges[i].p == p) { g_host_ranges.erase(g_host_ranges.begin() + (long)i); break; }
    }
    (void)hipHostFree(p);
}
