// sdrhip_interp.cpp -- the interpolator bank of include/sdrhip.h.
#include "sdrhip_host.h"

#include <cstring>
#include <new>
#include <vector>

using namespace sdrhip;

// --------------------------------------------------------------------------- interpolators
struct sdrhip_interpolators {
    sdrhip::CtxRef ctx; // (first: released last)
    int nstreams;
    sdrhip::DevBuf state[2]; // [nstreams][INT_STATE_WORDS]
    int cur;
    sdrhip::StreamMask reset_mask; // sdrhip_interpolators_reset_streams
    sdrhip_interp_plan last;       // what the last call launched (sdrhip_interpolators_last_plan)
    // ragged calls: the per-call table (rows and entries, interp_ragged_plan.h), the packed staging of host rows
    sdrhip::TableVersions map_tab;
    sdrhip::PinnedBuf stage_pin, out_pin;
    explicit sdrhip_interpolators(sdrhip_ctx *c) : ctx(c) { memset(&last, 0, sizeof(last)); }
};

namespace {
void set_last(sdrhip_interpolators *p, int path, size_t seg_len, int wpw, size_t entries, int compact)
{
    p->last.path = path; p->last.wpw = wpw; p->last.compact = compact; p->last.seg_len = seg_len; p->last.entries = entries;
}
int route_path(InterpRoute r) { return r == IR_WAVE ? SDRHIP_INTERP_WAVE : r == IR_VALU ? SDRHIP_INTERP_VALU : SDRHIP_INTERP_COPY; }
} // namespace

extern "C" int sdrhip_interpolators_last_plan(const sdrhip_interpolators *p, sdrhip_interp_plan *out)
{
    if (!p || !out) return fail(SDRHIP_EINVAL, "interpolators_last_plan: NULL argument");
    sdrhip::CtxLock lock_(p->ctx);
    *out = p->last;
    return SDRHIP_OK;
}

extern "C" int sdrhip_interpolators_create(sdrhip_ctx *ctx, int nstreams, sdrhip_interpolators **out)
{
    if (!ctx || !out || nstreams <= 0 || nstreams > 65535) return fail(SDRHIP_EINVAL, "interpolators_create: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    sdrhip_interpolators *p = new (std::nothrow) sdrhip_interpolators(ctx);
    if (!p) return fail(SDRHIP_ENOMEM, "out of host memory");
    p->nstreams = nstreams; p->cur = 0;
    size_t bytes = (size_t)nstreams * INT_STATE_WORDS * sizeof(int32_t);
    if (p->state[0].alloc_exact(bytes) || p->state[1].alloc_exact(bytes)) {
        delete p;
        return fail(SDRHIP_ENOMEM, "hipMalloc interpolator state");
    }
    *out = p;
    return sdrhip_interpolators_reset(p);
}

extern "C" void sdrhip_interpolators_destroy(sdrhip_interpolators *p)
{
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
}

extern "C" int sdrhip_interpolators_reset(sdrhip_interpolators *p)
{
    if (!p) return fail(SDRHIP_EINVAL, "interpolators is NULL");
    sdrhip::CtxLock lock_(p->ctx);
    size_t bytes = (size_t)p->nstreams * INT_STATE_WORDS * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(p->state[0].p, 0, bytes, p->ctx->stream));
    HIP_TRY(hipMemsetAsync(p->state[1].p, 0, bytes, p->ctx->stream));
    p->cur = 0;
    return SDRHIP_OK;
}

namespace sdrhip {
void interpolators_reset_part(sdrhip_interpolators *p, StreamResetArgs *a)
{
    a->rows[0] = p->state[0].as<int32_t>(); a->rows[1] = p->state[1].as<int32_t>();
    a->row_words = INT_STATE_WORDS;
}
int32_t *interpolators_row(sdrhip_interpolators *p, int s, int half) { return p->state[p->cur ^ (half & 1)].as<int32_t>() + (size_t)s * INT_STATE_WORDS; }
} // namespace sdrhip

extern "C" int sdrhip_interpolators_reset_streams(sdrhip_interpolators *p, const uint8_t *mask)
{
    if (!p) return fail(SDRHIP_EINVAL, "interpolators is NULL");
    sdrhip::CtxLock lock_(p->ctx);
    return stream_reset_bank(p->ctx, p->reset_mask, mask, p->nstreams,
                             [p](StreamResetArgs *a) { interpolators_reset_part(p, a); }, [](const uint8_t *) {});
}

namespace sdrhip {
bool interpolate_gather_ok(const sdrhip_ctx *c, int log2interp) { return interp_pick_wave(c->opt.interp_wave, log2interp); }

// x1, Upsampler::process m_interp == 0: samples_out = samples_in (Upsampler.cpp:54-57).  No filter, so no state: `cur` stays
static int interpolate1(sdrhip_interpolators *p, InterpRoute route, const int16_t *in, size_t n_in, size_t in_stride, int16_t *out, size_t out_stride,
                        const InterpCount *count, const int *fmt_dev)
{
    sdrhip_ctx *c = p->ctx;
    uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
    hipError_t e = hipErrorInvalidValue;
    const char *what = "copy";
    switch (route) {
    case IR_COPY: e = hipMemcpy2DAsync(out, out_stride * 4, in, in_stride * 4, n_in * 4, p->nstreams, hipMemcpyDeviceToDevice, c->stream); break;
    case IR_K6N: { // the copy, narrowed
        KTimer kt(c, SDRHIP_K_INTERPOLATE);
        e = launch_iq8_narrow(in, in_stride, out8, out_stride, n_in, p->nstreams, c->stream);
        what = "narrow launch";
        break;
    }
    case IR_K6X: { // the copy or its narrowing, stream by stream
        KTimer kt(c, SDRHIP_K_INTERPOLATE);
        e = launch_interpolate1_mixed(in, in_stride, out8, out_stride, n_in, p->nstreams, fmt_dev, count ? count->count : nullptr, count ? count->stride : 0,
                                      count ? count->unit : 0, c->stream);
        what = "mixed-format copy launch";
        break;
    }
    default: break;
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "interpolate1 %s: %s", what, hipGetErrorString(e));
    return SDRHIP_OK;
}

// validate and pick, plan, one timed launch, flip `cur`
int interpolate_device(sdrhip_interpolators *p, int log2interp, const int16_t *in, size_t n_in, size_t in_stride, int16_t *out,
                       size_t out_stride, size_t *n_out, const InterpGather *gather, const InterpCount *count, int out_fmt, const int *fmt_dev)
{
    sdrhip_ctx *c = p->ctx;
    if (n_out) *n_out = n_in << log2interp;
    set_last(p, 0, 0, 0, 0, 0); // (an empty or refused call reports no launch, not the previous call's)
    if (n_in == 0) return SDRHIP_OK;
    InterpPick pick = interp_pick(log2interp, c->opt.interp_wave, gather != nullptr, count != nullptr, out_fmt, fmt_dev != nullptr, 0);
    if (pick.route == IR_REFUSED) return fail(SDRHIP_EINVAL, "internal: %s", pick.why);
    if (log2interp == 0) {
        const int rc = interpolate1(p, pick.route, in, n_in, in_stride, out, out_stride, count, fmt_dev);
        if (rc == SDRHIP_OK) set_last(p, SDRHIP_INTERP_COPY, n_in, 1, (size_t)p->nstreams, 0);
        return rc;
    }
    InterpArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.out = out; a.in_stride = in_stride; a.out_stride = out_stride; a.n_in = n_in;
    a.state_cur = p->state[p->cur].as<int32_t>(); a.state_next = p->state[p->cur ^ 1].as<int32_t>();
    a.nstreams = p->nstreams;
    if (gather) { a.gmap = gather->map; a.grx = gather->rx; a.grest = gather->restored; a.gframes = gather->frames; }
    if (count) { a.count = count->count; a.count_stride = count->stride; a.count_unit = count->unit; }
    // SDRHIP_INTERP_PATH = wave (K5w, default) | valu (K5); SDRHIP_INTERP_SPAN = segment length in inputs (tests)
    if (pick.route == IR_WAVE) plan_interpolate_wave(log2interp, n_in, p->nstreams, c->n_cu, c->opt.interp_span, &a.nsub_per_seg, &a.nseg);
    else plan_interpolate(log2interp, n_in, p->nstreams, &a.nsub_per_seg, &a.nseg);
    pick.wpw = interp_pick_wpw(pick.route, (size_t)a.nseg * (size_t)a.nstreams);
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_INTERPOLATE);
        e = launch_interpolate(pick, log2interp, a, fmt_dev, c->stream);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "interpolate launch: %s", hipGetErrorString(e));
    p->cur ^= 1;
    set_last(p, route_path(pick.route), (size_t)a.nsub_per_seg * (pick.route == IR_WAVE ? (size_t)INTERP_WB : interp_macro_cycle(log2interp)), pick.wpw,
             (size_t)a.nseg * (size_t)a.nstreams, 0);
    return SDRHIP_OK;
}
} // namespace sdrhip

extern "C" int sdrhip_interpolate(sdrhip_interpolators *p, int log2interp, const int16_t *iq_in, size_t n_in, size_t in_stride,
                                  int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!p) return fail(SDRHIP_EINVAL, "interpolate: NULL handle");
    sdrhip::CtxLock lock_(p->ctx);
    if (log2interp < 0 || log2interp > 6) return fail(SDRHIP_EINVAL, "Invalid log2 interpolation factor"); // Upsampler.cpp:38-42
    if (n_in && (!iq_in || !iq_out)) return fail(SDRHIP_EINVAL, "interpolate: NULL buffer");
    sdrhip_ctx *c = p->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int S = p->nstreams;
    const size_t n_res = n_in << log2interp;
    if (S == 1) { in_stride = n_in; out_stride = n_res; }
    if (S > 1 && (in_stride < n_in || out_stride < n_res)) return fail(SDRHIP_EINVAL, "interpolate: stride smaller than the per-stream length");
    if (mem == SDRHIP_MEM_DEVICE) {
        if (n_in && (!aligned16(iq_in) || !aligned16(iq_out) || (S > 1 && ((in_stride & 3) || (out_stride & 3)))))
            return fail(SDRHIP_EALIGN, "interpolate: device pointers must be 16-byte aligned and strides multiples of 4 samples");
        return interpolate_device(p, log2interp, iq_in, n_in, in_stride, iq_out, out_stride, n_out);
    }
    if (int e = check_mem(mem)) return e;
    if (n_in == 0) { if (n_out) *n_out = 0; return SDRHIP_OK; }
    const size_t dis = (n_in + 3) & ~(size_t)3, dos = (n_res + 3) & ~(size_t)3;
    int rc;
    if ((rc = c->in.reserve((size_t)S * dis * 4 + 16))) return rc;
    if ((rc = c->out.reserve((size_t)S * dos * 4 + 16))) return rc;
    HIP_TRY(link_copy2d(c, c->in.p, dis * 4, iq_in, in_stride * 4, n_in * 4, S, hipMemcpyHostToDevice, c->stream));
    if ((rc = interpolate_device(p, log2interp, c->in.as<int16_t>(), n_in, dis, c->out.as<int16_t>(), dos, n_out))) return rc;
    HIP_TRY(link_copy2d(c, iq_out, out_stride * 4, c->out.p, dos * 4, n_res * 4, S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// ------------------------------------------------------------------------------ ragged interpolator calls (K5c)
namespace {
// the table up (a version no launch in flight reads: TableVersions), one timed launch over its entries, flip `cur`.  `table`: rows,
// then entries, as interp_ragged_build left them
int interpolate_ragged_device(sdrhip_interpolators *p, int log2interp, InterpPick pick, const InterpRaggedPlan &plan, const void *table,
                              const int16_t *in, int16_t *out)
{
    sdrhip_ctx *c = p->ctx;
    const int S = p->nstreams;
    const void *tab_dev = nullptr;
    if (int rc = p->map_tab.upload(c->stream, table, interp_ragged_table_bytes(S, plan), &tab_dev)) return rc;
    const InterpMapRow *rows = static_cast<const InterpMapRow *>(tab_dev);
    InterpArgs a;
    memset(&a, 0, sizeof(a)); // (strides 0: the rows carry the offsets; n_in / nseg come from the rows)
    a.in = in; a.out = out;
    a.state_cur = p->state[p->cur].as<int32_t>(); a.state_next = p->state[p->cur ^ 1].as<int32_t>();
    a.nstreams = S;
    a.nsub_per_seg = plan.nsub_per_seg;
    pick.wpw = plan.wpw;
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_INTERPOLATE);
        e = launch_interp_mapped(pick, log2interp, a, rows, reinterpret_cast<const InterpMapEntry *>(rows + S), plan.entries, c->stream);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "interpolate_ragged launch: %s", hipGetErrorString(e));
    if (log2interp) p->cur ^= 1; // (x1 has no filter and no state)
    set_last(p, route_path(plan.route), plan.seg_len, plan.wpw, plan.entries, 1);
    return SDRHIP_OK;
}
} // namespace

extern "C" int sdrhip_interpolate_ragged(sdrhip_interpolators *p, int log2interp, const int16_t *iq_in, const size_t *n_in, size_t in_stride,
                                         int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!p || !n_in || !n_out) return fail(SDRHIP_EINVAL, "interpolate_ragged: NULL handle or count array");
    sdrhip::CtxLock lock_(p->ctx);
    if (log2interp < 0 || log2interp > 6) return fail(SDRHIP_EINVAL, "Invalid log2 interpolation factor"); // Upsampler.cpp:38-42
    if (int e = check_mem(mem)) return e;
    sdrhip_ctx *c = p->ctx;
    const int S = p->nstreams;
    // everything that can refuse the call comes first: nothing is consumed, enqueued or flipped by a refused call
    const InterpPick pick = interp_pick_mapped(log2interp, c->opt.interp_wave);
    if (pick.route == IR_REFUSED) return fail(SDRHIP_EINVAL, "interpolate_ragged: %s", pick.why);
    InterpRaggedPlan plan;
    const char *why = "";
    const int sized = interp_ragged_size(n_in, S, log2interp, pick.route, c->opt.interp_span, &plan, &why);
    if (sized == INTERP_RAGGED_REFUSED) return fail(SDRHIP_EINVAL, "interpolate_ragged: %s", why);
    const size_t max_in = plan.max_n, max_res = max_in << log2interp;
    if (max_in && (!iq_in || !iq_out)) return fail(SDRHIP_EINVAL, "interpolate_ragged: NULL buffer");
    if (S == 1) { in_stride = max_in; out_stride = max_res; }
    if (S > 1 && (in_stride < max_in || out_stride < max_res)) return fail(SDRHIP_EINVAL, "interpolate_ragged: stride smaller than the largest count");
    if (mem == SDRHIP_MEM_DEVICE && max_in && (!aligned16(iq_in) || !aligned16(iq_out) || (S > 1 && ((in_stride & 3) || (out_stride & 3)))))
        return fail(SDRHIP_EALIGN, "interpolate_ragged: device pointers must be 16-byte aligned and strides multiples of 4 samples");
    HIP_TRY(hipSetDevice(c->device));
    for (int s = 0; s < S; ++s) n_out[s] = n_in[s] << log2interp;
    set_last(p, 0, 0, 0, 0, 0);
    if (sized == INTERP_RAGGED_EMPTY) return SDRHIP_OK; // nothing launched, `cur` stays

    std::vector<uint64_t> table((interp_ragged_table_bytes(S, plan) + 7) / 8);
    InterpMapRow *rows = reinterpret_cast<InterpMapRow *>(table.data());
    interp_ragged_fill(n_in, S, plan, in_stride, out_stride, rows, reinterpret_cast<InterpMapEntry *>(rows + S));
    if (mem == SDRHIP_MEM_DEVICE) return interpolate_ragged_device(p, log2interp, pick, plan, table.data(), iq_in, iq_out);

    // host rows: one packed upload of exactly the streams' samples and one packed download of exactly their results.  The rows lie
    // back to back on the device (the table's offsets say where).  x2 alone rounds every output row up to 4 samples, for K5's
    // 16-byte stores (from x4 on every n_out[s] is a multiple of 4; the x1 copy takes any alignment); an input row that does not
    // start on 16 bytes is read through K5w's guarded loads
    size_t total_in = 0, total_out = 0;
    for (int s = 0; s < S; ++s) {
        rows[s].in_off = total_in;
        rows[s].out_off = total_out;
        total_in += n_in[s];
        total_out += log2interp == 1 ? (n_out[s] + 3) & ~(size_t)3 : n_out[s];
    }
    int rc;
    if ((rc = p->stage_pin.reserve(total_in * 4))) return rc;
    if ((rc = p->out_pin.reserve(total_out * 4))) return rc;
    if ((rc = c->in.reserve(total_in * 4 + 16))) return rc;
    if ((rc = c->out.reserve(total_out * 4 + 16))) return rc;
    for (int s = 0; s < S; ++s)
        if (n_in[s]) memcpy(p->stage_pin.as<char>() + rows[s].in_off * 4, iq_in + (size_t)s * in_stride * 2, n_in[s] * 4);
    HIP_TRY(link_copy(c, c->in.p, p->stage_pin.p, total_in * 4, hipMemcpyHostToDevice, c->stream));
    p->stage_pin.mark(c->stream);
    if ((rc = interpolate_ragged_device(p, log2interp, pick, plan, table.data(), c->in.as<int16_t>(), c->out.as<int16_t>()))) return rc;
    HIP_TRY(link_copy(c, p->out_pin.p, c->out.p, total_out * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int s = 0; s < S; ++s)
        if (n_out[s]) memcpy(iq_out + (size_t)s * out_stride * 2, p->out_pin.as<char>() + rows[s].out_off * 4, n_out[s] * 4);
    return SDRHIP_OK;
}
