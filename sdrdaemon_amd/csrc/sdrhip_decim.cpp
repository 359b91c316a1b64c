// sdrhip_decim.cpp -- the decimator bank of include/sdrhip.h: the bank and its state, the uniform and the ragged device cores (shared
// with the Rx pipe), the host staging of both entries and the ragged table, and the taps entry (sdrhip_decimate_taps, K1t) on the
// ragged core's table and plan.  The launch geometry is decided in decim_plan.h.
#include "sdrhip_host.h"

#include <cstring>
#include <new>
#include <vector>

using namespace sdrhip;

// ------------------------------------------------------------------------------ decimators
struct sdrhip_decimators {
    sdrhip::CtxRef ctx; // (first: released last)
    int nstreams;
    int bias;
    sdrhip::DevBuf state[2]; // double buffered [nstreams][DEC_STATE_WORDS]
    int cur;
    bool stage0_int16; // history of m_decimator2 fits int16 (it last saw raw samples or nothing)
    sdrhip::DecimPlanInfo last; // what the last call launched
    // ragged calls: the per-call table (host staging, device copy), staging of host rows
    sdrhip::PinnedBuf rows_pin, stage_pin, out_pin;
    sdrhip::DevBuf rows_dev;
    sdrhip::StreamMask reset_mask; // sdrhip_decimators_reset_streams
    explicit sdrhip_decimators(sdrhip_ctx *c) : ctx(c) {}
};

extern "C" int sdrhip_decimators_last_plan(const sdrhip_decimators *d, sdrhip_decim_plan *out)
{
    if (!d || !out) return fail(SDRHIP_EINVAL, "decimators_last_plan: NULL argument");
    sdrhip::CtxLock lock_(d->ctx);
    out->path = d->last.path; out->wps = d->last.wps; out->npieces = d->last.npieces; out->nseg = d->last.nseg;
    out->span = d->last.span; out->head = d->last.head; out->tail_start = d->last.tail_start;
    return SDRHIP_OK;
}

extern "C" int sdrhip_decimators_create(sdrhip_ctx *ctx, int nstreams, int hb_variant, sdrhip_decimators **out)
{
    if (!ctx || !out || nstreams <= 0 || nstreams > 65535) return fail(SDRHIP_EINVAL, "decimators_create: bad argument");
    if (hb_variant != SDRHIP_HB_EO1 && hb_variant != SDRHIP_HB_DB) return fail(SDRHIP_EINVAL, "hb_variant must be SDRHIP_HB_EO1 or SDRHIP_HB_DB");
    HIP_TRY(hipSetDevice(ctx->device));
    sdrhip_decimators *d = new (std::nothrow) sdrhip_decimators(ctx);
    if (!d) return fail(SDRHIP_ENOMEM, "out of host memory");
    d->nstreams = nstreams; d->bias = hb_variant; d->cur = 0; d->stage0_int16 = true;
    size_t bytes = (size_t)nstreams * DEC_STATE_WORDS * sizeof(int32_t);
    if (d->state[0].alloc_exact(bytes) || d->state[1].alloc_exact(bytes)) {
        delete d;
        return fail(SDRHIP_ENOMEM, "hipMalloc decimator state");
    }
    *out = d;
    return sdrhip_decimators_reset(d);
}

extern "C" void sdrhip_decimators_destroy(sdrhip_decimators *d)
{
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    delete d;
}

extern "C" int sdrhip_decimators_reset(sdrhip_decimators *d)
{
    if (!d) return fail(SDRHIP_EINVAL, "decimators is NULL");
    sdrhip::CtxLock lock_(d->ctx);
    size_t bytes = (size_t)d->nstreams * DEC_STATE_WORDS * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(d->state[0].p, 0, bytes, d->ctx->stream)); // ctor zero fill, EO1.h:171-188
    HIP_TRY(hipMemsetAsync(d->state[1].p, 0, bytes, d->ctx->stream));
    d->cur = 0;
    d->stage0_int16 = true;
    return SDRHIP_OK;
}

namespace sdrhip {
void decimators_reset_part(sdrhip_decimators *d, StreamResetArgs *a)
{
    a->rows[0] = d->state[0].as<int32_t>(); a->rows[1] = d->state[1].as<int32_t>();
    a->row_words = DEC_STATE_WORDS;
}
void decimators_reset_done(sdrhip_decimators *d, bool all)
{
    // (bank-wide: the streams that were not reset may still hold rotate-sums in m_decimator2's history)
    if (all) d->stage0_int16 = true;
}
int32_t *decimators_row(sdrhip_decimators *d, int s, int half) { return d->state[d->cur ^ (half & 1)].as<int32_t>() + (size_t)s * DEC_STATE_WORDS; }
bool decimators_stage0_int16(const sdrhip_decimators *d) { return d->stage0_int16; }
void decimators_clear_stage0_int16(sdrhip_decimators *d) { d->stage0_int16 = false; }
} // namespace sdrhip

extern "C" int sdrhip_decimators_reset_streams(sdrhip_decimators *d, const uint8_t *mask)
{
    if (!d) return fail(SDRHIP_EINVAL, "decimators is NULL");
    sdrhip::CtxLock lock_(d->ctx);
    return stream_reset_bank(d->ctx, d->reset_mask, mask, d->nstreams,
                             [d](StreamResetArgs *a) { decimators_reset_part(d, a); },
                             [d](const uint8_t *m) { decimators_reset_done(d, m == nullptr); });
}

// ------------------------------------------------------------------------------ the device-pointer cores
namespace {
// DecimArgs::mf_* of a matrix-core launch from its plan
void set_mf_args(DecimArgs &a, const MfPlan &p)
{
    a.mf_head = p.head; a.mf_span = p.span; a.mf_tail_start = p.tail_start; a.mf_tail_seg = p.tail_seg;
    a.mf_wps = p.wps; a.mf_npieces = p.npieces;
    a.mf_piece_wgs = p.piece_wgs; a.mf_piece_early = p.piece_early; a.mf_piece_share = p.piece_share;
}

// a call as decimate_core sees it: the buffers, and the counts of its longest and its shortest stream (a uniform call: one count)
struct DecimCall {
    const int16_t *in;
    size_t in_stride;
    int16_t *out;
    size_t out_stride;
    int frame_mode, frame_blocks;
    size_t n_raw, n_dec; // the longest stream's samples, raw and decimated
    size_t min_used;     // raw samples the shortest stream's cascade consumes
};

// What decimate_device and decimate_ragged_device share: the calls that launch no cascade, the arguments every cascade launch
// takes, the record for last_plan and the bank's bookkeeping behind the launch.  The cores hand in what is their own:
//   simple()                  launches the filter-less kernel;
//   plan(a, &mfma)            fills the rest of the cascade's arguments and says which path the call takes (a result other than
//                             SDRHIP_OK refuses the call);
//   launch(a, pack16, mfma)   launches it.
template <class Simple, class Plan, class Launch>
int decimate_core(sdrhip_decimators *d, unsigned L, int fcpos, const DecimCall &k, Simple simple, Plan plan, Launch launch)
{
    sdrhip_ctx *c = d->ctx;
    d->last = DecimPlanInfo(); // (set below when a cascade kernel is launched; filter-less and empty calls report path 0, not the previous call's plan)
    // decimate1 copies (Downsampler::process m_decim == 0: Downsampler.cpp:76-80, Decimators.cpp:22-35); from decimate2 on a call
    // without a whole output sample launches nothing (the reference's unsigned loop bound would wrap there): nothing enters any history
    if ((L == 0 ? k.n_raw : k.n_dec) == 0) return SDRHIP_OK;
    const bool cen = fcpos == SDRHIP_FC_CEN;
    if (L == 0 || (!cen && L <= 2)) {
        if (k.frame_mode) return fail(SDRHIP_EINVAL, L == 0 ? "internal: frame mode needs log2decim >= 1" : "internal: frame mode unsupported for filter-less decimation");
        hipError_t e = simple();
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "decimate%u launch: %s", 1u << L, hipGetErrorString(e));
        return SDRHIP_OK;
    }

    DecimArgs a;
    memset(&a, 0, sizeof(a));
    a.in = k.in; a.out = k.out; a.in_stride = k.in_stride; a.out_stride = k.out_stride;
    a.state_cur = d->state[d->cur].as<int32_t>(); a.state_next = d->state[d->cur ^ 1].as<int32_t>();
    a.nstreams = d->nstreams;
    a.bias = d->bias;
    a.frame_mode = k.frame_mode; a.frame_blocks = k.frame_blocks;
    a.mf_dump = c->decim_dump;
    bool mfma = false;
    if (int rc = plan(a, &mfma)) return rc;
    const bool pack16 = cen && d->stage0_int16;
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_DECIMATE);
        e = launch(a, pack16, mfma);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "decimate launch: %s", hipGetErrorString(e));
    d->last.path = mfma ? DECIM_PATH_MFMA : DECIM_PATH_VALU;
    if (mfma) {
        d->last.span = a.mf_span; d->last.head = a.mf_head; d->last.tail_start = a.mf_tail_start;
        d->last.wps = a.mf_wps; d->last.npieces = a.mf_npieces;
    } else {
        d->last.nseg = a.nseg;
    }
    d->cur ^= 1;
    // m_decimator2's 64-entry history now holds raw int16 samples (cen) or rotate-sums (inf/sup); a centred call shorter than the
    // history leaves older rotate-sums in it, which the packed-int16 first stage cannot represent.  So every stream's first-stage
    // history holds raw int16 samples when every stream either saw a whole history of them now or held only such before (a stream
    // of a ragged call that got nothing keeps what it had)
    d->stage0_int16 = cen && (d->stage0_int16 || k.min_used >= (size_t)2 * DEC_HIST);
    return SDRHIP_OK;
}
} // namespace

namespace sdrhip {
// device-pointer core shared with the fused Rx pipe; frame_* = 0 for plain output
int decimate_device(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *in, size_t n_in,
                    size_t in_stride, int16_t *out, size_t out_stride, size_t *n_out, int frame_mode, int frame_blocks,
                    uint64_t frame_sample_base, const RxMeta *meta, const Enc128Args *fuse, bool *fused, bool coresident)
{
    if (fused) *fused = false;
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    const unsigned L = (unsigned)log2decim;
    const DecimShifts sh = decimated_shifts(L, *sampleSize); // Decimators.cpp:27-32, 43-44, 132-133, 222-223 ...
    const size_t n_dec = n_in >> L;                          // out.resize(len / N)
    const size_t n_used = n_dec << L;
    *sampleSize = decimated_sample_size(L, *sampleSize);
    if (n_out) *n_out = n_dec;
    const DecimCall k = {in, in_stride, out, out_stride, frame_mode, frame_blocks, n_in, n_dec, n_used};
    return decimate_core(
        d, L, fcpos, k,
        [&]() { return launch_decimate_simple(log2decim, fcpos, in, in_stride, out, out_stride, n_in, S, (int)sh.norm, (int)sh.trunk, c->stream); },
        [&](DecimArgs &a, bool *mfma) -> int {
            a.n_used = n_used;
            a.norm = (int)sh.norm; a.trunk = (int)sh.trunk;
            a.frame_sample_base = frame_sample_base;
            if (meta) set_meta_args(a, *meta);
            plan_decimate(log2decim, fcpos, n_used, S, &a.nsub_per_seg, &a.nseg);
            // matrix-core cascade for the centred modes when the call is long enough to fill the chip;
            // SDRHIP_DECIM_PATH = valu | mfma | auto (default), SDRHIP_MFMA_SPAN = span length in samples (tests)
            const CtxOptions &env = c->opt;
            // (frame mode on the matrix cores: the waves' store offsets are 32 bits with the top two reserved, decim_mfma.hip)
            const bool mfma_frames = env.rx_direct && out_stride * 4 < 0x3fffffffu;
            a.mf_ring = coresident ? 3 : env.mfma_ring; // (the planner reads it: ring 2 = two waves per SIMD)
            a.mf_prio = coresident ? 1 : 0;
            MfPlan p;
            *mfma = (!frame_mode || mfma_frames) && mfma_admitted(env.decim_path, env.mfma_min, log2decim, n_used * (size_t)S) &&
                    plan_decimate_mfma(log2decim, fcpos, n_used, S, env.mfma_span, c->n_cu, a.mf_ring, &p);
            if (*mfma) set_mf_args(a, p);
            return SDRHIP_OK;
        },
        [&](const DecimArgs &a, bool pack16, bool mfma) -> hipError_t {
            if (!(mfma && fuse && L <= 4)) // (decimate32 / 64: 180-220 VGPRs, no room for encoder waves beside them)
                return mfma ? launch_decimate_mfma(log2decim, pack16, a, c->stream) : launch_decimate(log2decim, fcpos, pack16, a, c->stream);
            hipError_t e;
            if (++c->fused_tag == 0xffffffffu) { // (the per-CU words hold the highest tag seen: start over before it wraps)
                (void)hipMemsetAsync(c->fused_roles, 0, SDRHIP_FUSED_ROLE_WORDS * 4, c->stream);
                c->fused_tag = 1;
            }
            if (c->opt.rx_fused == 2) { // (experiment: the fused kernel without encoder units, the encoder as its own launch)
                Enc128Args none = *fuse;
                none.nlist = 0;
                e = launch_rx_fused(log2decim, pack16, a, none, c->fused_roles, c->fused_tag, c->stream);
                if (e == hipSuccess) e = launch_gf_encode128(*fuse, c->stream);
            } else
                e = launch_rx_fused(log2decim, pack16, a, *fuse, c->fused_roles, c->fused_tag, c->stream);
            if (e != hipSuccess) {
                // a fused launch that never started has not cleared the NEXT launch's unit counters (block 0 of every launch
                // does that): start the role table over, or the next fused launch would find them exhausted and do nothing
                (void)hipMemsetAsync(c->fused_roles, 0, SDRHIP_FUSED_ROLE_WORDS * 4, c->stream);
                c->fused_tag = 0;
            }
            if (fused) *fused = true;
            return e;
        });
}

// would a plain (stream-order) decimate call of this size run on the matrix cores?  (The Rx pipe then decimates into
// a stream-order buffer and frames it with K2 instead of using the VALU kernel's fused frame epilogue.)
bool decimate_mfma_applies(const sdrhip_decimators *d, int log2decim, int fcpos, size_t n_in)
{
    const CtxOptions &env = d->ctx->opt;
    const size_t n_used = (n_in >> log2decim) << log2decim;
    MfPlan p;
    return mfma_admitted(env.decim_path, env.mfma_min, log2decim, n_used * (size_t)d->nstreams) &&
           plan_decimate_mfma(log2decim, fcpos, n_used, d->nstreams, env.mfma_span, d->ctx->n_cu, env.mfma_ring, &p);
}
} // namespace sdrhip

extern "C" int sdrhip_decimate(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                               size_t n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!d || !sampleSize) return fail(SDRHIP_EINVAL, "decimate: NULL handle or sampleSize");
    sdrhip::CtxLock lock_(d->ctx);
    if (log2decim < 0 || log2decim > 6) return fail(SDRHIP_EINVAL, "Invalid log2 decimation factor"); // Downsampler.cpp:39-43
    if (fcpos < SDRHIP_FC_INF || fcpos > SDRHIP_FC_CEN) return fail(SDRHIP_EINVAL, "Invalid Fc position index"); // :55-59
    if (*sampleSize < 1 || *sampleSize > 16) return fail(SDRHIP_EINVAL, "sampleSize must be 1..16");
    if (n_in && (!iq_in || (!iq_out && (n_in >> log2decim)))) return fail(SDRHIP_EINVAL, "decimate: NULL buffer"); // (no output, no buffer needed)
    sdrhip_ctx *c = d->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int S = d->nstreams;
    const size_t n_res = n_in >> log2decim;
    if (S == 1) { in_stride = n_in; out_stride = n_res; }
    if (S > 1 && (in_stride < n_in || out_stride < n_res)) return fail(SDRHIP_EINVAL, "decimate: stride smaller than the per-stream length");

    if (mem == SDRHIP_MEM_DEVICE) {
        if (n_in && (!aligned16(iq_in) || !aligned16(iq_out) || (S > 1 && ((in_stride & 3) || (out_stride & 3)))))
            return fail(SDRHIP_EALIGN, "decimate: device pointers must be 16-byte aligned and strides multiples of 4 samples");
        return decimate_device(d, log2decim, fcpos, sampleSize, iq_in, n_in, in_stride, iq_out, out_stride, n_out, 0, 0, 0);
    }
    if (int e = check_mem(mem)) return e;

    // host buffers: stage through device memory with padded (16-byte aligned) per-stream strides
    const size_t dis = (n_in + 3) & ~(size_t)3, dos = (n_res + 3) & ~(size_t)3;
    if (n_in == 0) // nothing to stage; sampleSize still advances like in the device path
        return decimate_device(d, log2decim, fcpos, sampleSize, nullptr, 0, 0, nullptr, 0, n_out, 0, 0, 0);
    int rc;
    if ((size_t)S * dis * 4 <= SDRHIP_ZEROCOPY_MAX) {
        // small call (one TestSource block ...): no copy engine, the kernel reads and writes pinned host memory itself
        if ((rc = c->zin.reserve((size_t)S * dis * 4 + 16))) return rc;
        if ((rc = c->zout.reserve((size_t)S * dos * 4 + 16))) return rc;
        for (int s = 0; s < S; ++s) memcpy(c->zin.as<int16_t>() + (size_t)s * dis * 2, iq_in + (size_t)s * in_stride * 2, n_in * 4);
        link_bytes(c, hipMemcpyHostToDevice, (size_t)S * n_in * 4);  // (read by the kernel over the link)
        link_bytes(c, hipMemcpyDeviceToHost, (size_t)S * n_res * 4); // (written by it)
        rc = decimate_device(d, log2decim, fcpos, sampleSize, c->zin.as<int16_t>(), n_in, dis, c->zout.as<int16_t>(), dos, n_out, 0, 0, 0);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int s = 0; s < S && n_res; ++s) memcpy(iq_out + (size_t)s * out_stride * 2, c->zout.as<int16_t>() + (size_t)s * dos * 2, n_res * 4);
        return SDRHIP_OK;
    }
    if ((rc = c->in.reserve((size_t)S * dis * 4 + 16))) return rc;
    if ((rc = c->out.reserve((size_t)S * dos * 4 + 16))) return rc;
    HIP_TRY(link_copy2d(c, c->in.p, dis * 4, iq_in, in_stride * 4, n_in * 4, S, hipMemcpyHostToDevice, c->stream));
    rc = decimate_device(d, log2decim, fcpos, sampleSize, static_cast<const int16_t *>(c->in.p), n_in, dis,
                         static_cast<int16_t *>(c->out.p), dos, n_out, 0, 0, 0);
    if (rc) return rc;
    if (n_res) HIP_TRY(link_copy2d(c, iq_out, out_stride * 4, c->out.p, dos * 4, n_res * 4, S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// ------------------------------------------------------------------------------ ragged decimator calls
namespace sdrhip {
int ragged_plan(const sdrhip_decimators *d, int log2decim, int fcpos, const size_t *n_in, RaggedRow *rows, RaggedPlan *plan)
{
    const sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    size_t total = 0;
    for (int s = 0; s < S; ++s) {
        rows[s].n_raw = n_in[s];
        rows[s].n_dec = n_in[s] >> log2decim;
        rows[s].n_used = (uint64_t)(n_in[s] >> log2decim) << log2decim;
        total += (size_t)rows[s].n_used;
    }
    // K1r's segments, then K1mr: the matrix-core launch with per-stream wave groups and pieces, under the rules of the uniform call
    // (decim_path, mfma_min of the call's total samples, a mean stream long enough for a span)
    if (!plan_decimate_ragged(log2decim, fcpos, rows, S, total, &plan->nsub, &plan->grid)) return fail(SDRHIP_EINVAL, "ragged call: too many segments");
    const CtxOptions &env = c->opt;
    plan->ring = env.mfma_ring == 3 ? 3 : 4;
    plan->mfma = mfma_admitted(env.decim_path, env.mfma_min, log2decim, total) &&
                 plan_decimate_mfma_ragged(log2decim, fcpos, rows, S, env.mfma_span, c->n_cu, plan->ring, &plan->mf);
    return SDRHIP_OK;
}

int ragged_prepare(sdrhip_decimators *d, int log2decim, int fcpos, const size_t *n_in, RaggedRow *rows, const RaggedRow **rows_dev,
                   RaggedPlan *plan, PinnedBuf *pin)
{
    sdrhip_ctx *c = d->ctx;
    int rc;
    if ((rc = ragged_plan(d, log2decim, fcpos, n_in, rows, plan))) return rc;
    const size_t bytes = (size_t)d->nstreams * sizeof(RaggedRow);
    PinnedBuf &tab = pin ? *pin : d->rows_pin;
    if ((rc = tab.reserve(bytes))) return rc; // (waits for the last upload from this staging: the previous table's, or the ring slot's)
    if ((rc = d->rows_dev.reserve(bytes))) return rc;
    memcpy(tab.p, rows, bytes);
    HIP_TRY(hipMemcpyAsync(d->rows_dev.p, tab.p, bytes, hipMemcpyHostToDevice, c->stream));
    tab.mark(c->stream);
    *rows_dev = d->rows_dev.as<RaggedRow>();
    return SDRHIP_OK;
}

int ragged_reserve(sdrhip_decimators *d, PinnedBuf *pin)
{
    const size_t bytes = (size_t)d->nstreams * sizeof(RaggedRow);
    if (int rc = (pin ? *pin : d->rows_pin).reserve(bytes)) return rc;
    return d->rows_dev.reserve(bytes);
}

int decimate_ragged_device(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *in, size_t in_stride,
                           int16_t *out, size_t out_stride, const RaggedRow *rows, const RaggedRow *rows_dev, const RaggedPlan &plan,
                           int frame_mode, int frame_blocks, const unsigned *meta_w, unsigned meta_rate)
{
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    const unsigned L = (unsigned)log2decim;
    size_t max_raw = 0, max_dec = 0, min_used = SIZE_MAX;
    for (int s = 0; s < S; ++s) {
        if (rows[s].n_raw > max_raw) max_raw = (size_t)rows[s].n_raw;
        if (rows[s].n_dec > max_dec) max_dec = (size_t)rows[s].n_dec;
        if (rows[s].n_used < min_used) min_used = (size_t)rows[s].n_used;
    }
    // (every stream's size advances as in sdrhip_decimate, whatever its count; the shifts went up with the rows: RaggedRow::shifts)
    for (int s = 0; s < S; ++s) sampleSize[s] = decimated_sample_size(L, sampleSize[s]);
    const DecimCall k = {in, in_stride, out, out_stride, frame_mode, frame_blocks, max_raw, max_dec, min_used};
    return decimate_core(
        d, L, fcpos, k,
        [&]() { return launch_decimate_simple_ragged(log2decim, fcpos, in, in_stride, out, out_stride, max_raw, S, 0, 0, rows_dev, c->stream); },
        [&](DecimArgs &a, bool *mfma) -> int {
            if (frame_mode && !plan.mfma) return fail(SDRHIP_EINVAL, "internal: ragged frame mode needs the matrix-core launch");
            // (a.n_used, a.norm and a.trunk stay 0: the ragged kernels take each stream's count and shift pair from its row)
            a.nsub_per_seg = plan.nsub; a.nseg = plan.grid;
            a.meta_rate = meta_rate;
            if (meta_w) memcpy(a.meta_w, meta_w, sizeof(a.meta_w));
            if (plan.mfma) {
                set_mf_args(a, plan.mf);
                a.mf_ring = plan.ring;
            }
            *mfma = plan.mfma;
            return SDRHIP_OK;
        },
        [&](const DecimArgs &a, bool pack16, bool mfma) {
            return mfma ? launch_decimate_mfma_ragged(log2decim, pack16, a, rows_dev, c->stream)
                        : launch_decimate_ragged(log2decim, fcpos, pack16, a, rows_dev, c->stream);
        });
}

int ragged_stage_in(sdrhip_ctx *c, PinnedBuf &pin, DevBuf &dev, const void *src, size_t in_stride, const size_t *n_in, int S, size_t esz,
                    size_t dstride, const void **out)
{
    int rc;
    size_t total = 0, max_n = 0;
    for (int s = 0; s < S; ++s) { total += n_in[s]; if (n_in[s] > max_n) max_n = n_in[s]; }
    const char *p = static_cast<const char *>(src);
    if ((size_t)S * dstride * esz <= SDRHIP_ZEROCOPY_MAX) { // (small call: the kernel reads the pinned rows itself)
        if ((rc = c->zin.reserve((size_t)S * dstride * esz + 16))) return rc;
        for (int s = 0; s < S; ++s)
            if (n_in[s]) memcpy(c->zin.as<char>() + (size_t)s * dstride * esz, p + (size_t)s * in_stride * esz, n_in[s] * esz);
        link_bytes(c, hipMemcpyHostToDevice, total * esz);
        *out = c->zin.p;
        return SDRHIP_OK;
    }
    if ((rc = pin.reserve((size_t)S * dstride * esz))) return rc;
    if ((rc = dev.reserve((size_t)S * dstride * esz + 16))) return rc;
    for (int s = 0; s < S; ++s)
        if (n_in[s]) memcpy(pin.as<char>() + (size_t)s * dstride * esz, p + (size_t)s * in_stride * esz, n_in[s] * esz);
    HIP_TRY(link_copy2d(c, dev.p, dstride * esz, pin.p, dstride * esz, max_n * esz, S, hipMemcpyHostToDevice, c->stream));
    pin.mark(c->stream);
    *out = dev.p;
    return SDRHIP_OK;
}
} // namespace sdrhip

// sampleSize: one entry per stream (sdrhip_decimate_ragged hands in nstreams copies of its one value)
static int decimate_ragged_sizes(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                                 const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (log2decim < 0 || log2decim > 6) return fail(SDRHIP_EINVAL, "Invalid log2 decimation factor");
    if (fcpos < SDRHIP_FC_INF || fcpos > SDRHIP_FC_CEN) return fail(SDRHIP_EINVAL, "Invalid Fc position index");
    for (int s = 0; s < d->nstreams; ++s)
        if (sampleSize[s] < 1 || sampleSize[s] > 16) return fail(SDRHIP_EINVAL, "sampleSize must be 1..16");
    if (int e = check_mem(mem)) return e;
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    size_t max_in = 0;
    for (int s = 0; s < S; ++s) if (n_in[s] > max_in) max_in = n_in[s];
    const size_t max_res = max_in >> log2decim;
    if (max_in && (!iq_in || (!iq_out && max_res))) return fail(SDRHIP_EINVAL, "decimate_ragged: NULL buffer");
    if (S == 1) { in_stride = max_in; out_stride = max_res; }
    if (S > 1 && (in_stride < max_in || out_stride < max_res)) return fail(SDRHIP_EINVAL, "decimate_ragged: stride smaller than the largest count");
    if (mem == SDRHIP_MEM_DEVICE && max_in && (!aligned16(iq_in) || !aligned16(iq_out) || (S > 1 && ((in_stride & 3) || (out_stride & 3)))))
        return fail(SDRHIP_EALIGN, "decimate_ragged: device pointers must be 16-byte aligned and strides multiples of 4 samples");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<RaggedRow> rows((size_t)S);
    memset(rows.data(), 0, rows.size() * sizeof(RaggedRow));
    for (int s = 0; s < S; ++s) n_out[s] = n_in[s] >> log2decim;
    if (max_in == 0) { // nothing to stage; sampleSize advances as in sdrhip_decimate
        d->last = DecimPlanInfo();
        for (int s = 0; s < S; ++s) sampleSize[s] = decimated_sample_size((unsigned)log2decim, sampleSize[s]);
        return SDRHIP_OK;
    }
    for (int s = 0; s < S; ++s) rows[(size_t)s].shifts = ragged_shift_word((unsigned)log2decim, sampleSize[s]);
    const RaggedRow *rdev = nullptr;
    RaggedPlan plan;
    int rc = ragged_prepare(d, log2decim, fcpos, n_in, rows.data(), &rdev, &plan);
    if (rc) return rc;
    if (mem == SDRHIP_MEM_DEVICE)
        return decimate_ragged_device(d, log2decim, fcpos, sampleSize, iq_in, in_stride, iq_out, out_stride, rows.data(), rdev, plan);
    const size_t dis = (max_in + 3) & ~(size_t)3, dos = (max_res + 3) & ~(size_t)3;
    const void *din = nullptr;
    if ((rc = ragged_stage_in(c, d->stage_pin, c->in, iq_in, in_stride, n_in, S, 4, dis, &din))) return rc;
    if ((rc = c->out.reserve((size_t)S * dos * 4 + 16))) return rc;
    if ((rc = decimate_ragged_device(d, log2decim, fcpos, sampleSize, static_cast<const int16_t *>(din), dis, c->out.as<int16_t>(), dos,
                                     rows.data(), rdev, plan)))
        return rc;
    if (max_res) {
        if ((rc = d->out_pin.reserve((size_t)S * dos * 4))) return rc;
        HIP_TRY(link_copy2d(c, d->out_pin.p, dos * 4, c->out.p, dos * 4, max_res * 4, S, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int s = 0; s < S; ++s)
        if (n_out[s]) memcpy(iq_out + (size_t)s * out_stride * 2, d->out_pin.as<char>() + (size_t)s * dos * 4, n_out[s] * 4);
    return SDRHIP_OK;
}

extern "C" int sdrhip_decimate_ragged(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                                      const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!d || !sampleSize || !n_in || !n_out) return fail(SDRHIP_EINVAL, "decimate_ragged: NULL handle, sampleSize or count array");
    sdrhip::CtxLock lock_(d->ctx);
    std::vector<unsigned> sizes((size_t)d->nstreams, *sampleSize);
    const int rc = decimate_ragged_sizes(d, log2decim, fcpos, sizes.data(), iq_in, n_in, in_stride, iq_out, out_stride, n_out, mem);
    *sampleSize = sizes[0];
    return rc;
}

// every sdrdaemonrx hands ITS source's get_sample_bits() to Downsampler::process (sdrdaemonrx.cpp:619-620, 639-640): a size per stream
extern "C" int sdrhip_decimate_ragged_bits(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                                           const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!d || !sampleSize || !n_in || !n_out) return fail(SDRHIP_EINVAL, "decimate_ragged_bits: NULL handle, sampleSize array or count array");
    sdrhip::CtxLock lock_(d->ctx);
    return decimate_ragged_sizes(d, log2decim, fcpos, sampleSize, iq_in, n_in, in_stride, iq_out, out_stride, n_out, mem);
}

// ------------------------------------------------------------------------------ taps of a centred cascade (K1t)
namespace {
// One launch for every stream and every tap of `t` (device pointers); L = the highest tap.  Two and more taps: K1t on K1r's grid and
// rows, through decimate_core like every cascade launch -- never the matrix cores.  One tap is the cascade alone: the launch
// sdrhip_decimate_ragged picks.
int decimate_taps_device(sdrhip_decimators *d, int L, unsigned sampleSize, const int16_t *in, size_t in_stride, const DecimTapArgs &t,
                         const RaggedRow *rows, const RaggedRow *rows_dev, const RaggedPlan &plan)
{
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    if ((t.mask & (t.mask - 1)) == 0) {
        std::vector<unsigned> sizes((size_t)S, sampleSize);
        return decimate_ragged_device(d, L, SDRHIP_FC_CEN, sizes.data(), in, in_stride, t.out[L], t.stride[L], rows, rows_dev, plan);
    }
    size_t max_raw = 0, max_dec = 0, min_used = SIZE_MAX;
    for (int s = 0; s < S; ++s) {
        if (rows[s].n_raw > max_raw) max_raw = (size_t)rows[s].n_raw;
        if (rows[s].n_dec > max_dec) max_dec = (size_t)rows[s].n_dec;
        if (rows[s].n_used < min_used) min_used = (size_t)rows[s].n_used;
    }
    const DecimCall k = {in, in_stride, t.out[L], t.stride[L], 0, 0, max_raw, max_dec, min_used};
    return decimate_core(
        d, (unsigned)L, SDRHIP_FC_CEN, k, [&]() { return hipErrorInvalidValue; }, // (centred, L >= 2: there is no filter-less call)
        [&](DecimArgs &a, bool *mfma) -> int {
            a.nsub_per_seg = plan.nsub; a.nseg = plan.grid;
            *mfma = false;
            return SDRHIP_OK;
        },
        [&](const DecimArgs &a, bool pack16, bool) { return launch_decimate_taps(L, pack16, a, t, rows_dev, c->stream); });
}

// ragged_stage_in with the link carrying exactly the counts: its copy of a call too big for the kernel to read pinned memory is one
// rectangle as wide as the largest count, so unequal rows of such a call go up one by one
int taps_stage_in(sdrhip_decimators *d, const int16_t *src, size_t in_stride, const size_t *n_in, size_t dstride, const void **out)
{
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    bool equal = true;
    for (int s = 1; s < S; ++s) equal = equal && n_in[s] == n_in[0];
    if (equal || (size_t)S * dstride * 4 <= SDRHIP_ZEROCOPY_MAX) return ragged_stage_in(c, d->stage_pin, c->in, src, in_stride, n_in, S, 4, dstride, out);
    int rc;
    if ((rc = d->stage_pin.reserve((size_t)S * dstride * 4))) return rc;
    if ((rc = c->in.reserve((size_t)S * dstride * 4 + 16))) return rc;
    for (int s = 0; s < S; ++s) {
        if (!n_in[s]) continue;
        char *row = d->stage_pin.as<char>() + (size_t)s * dstride * 4;
        memcpy(row, src + (size_t)s * in_stride * 2, n_in[s] * 4);
        HIP_TRY(link_copy(c, c->in.as<char>() + (size_t)s * dstride * 4, row, n_in[s] * 4, hipMemcpyHostToDevice, c->stream));
    }
    d->stage_pin.mark(c->stream);
    *out = c->in.p;
    return SDRHIP_OK;
}
} // namespace

extern "C" int sdrhip_decimate_taps(sdrhip_decimators *d, unsigned tap_mask, unsigned sampleSize, const int16_t *iq_in,
                                    const size_t *n_in, size_t in_stride, sdrhip_decim_taps *taps, size_t *n_used, int mem)
{
    if (!d || !taps || !n_in || !n_used) return fail(SDRHIP_EINVAL, "decimate_taps: NULL handle, taps or count array");
    sdrhip::CtxLock lock_(d->ctx);
    if (tap_mask == 0 || (tap_mask & ~0x7eu)) return fail(SDRHIP_EINVAL, "decimate_taps: tap_mask takes bits 1..6, at least one");
    if (sampleSize < 1 || sampleSize > 16) return fail(SDRHIP_EINVAL, "sampleSize must be 1..16");
    if (int e = check_mem(mem)) return e;
    sdrhip_ctx *c = d->ctx;
    const int S = d->nstreams;
    int L = 6;
    while (!((tap_mask >> L) & 1u)) --L;
    size_t max_in = 0;
    for (int s = 0; s < S; ++s) if (n_in[s] > max_in) max_in = n_in[s];
    const size_t max_used = (max_in >> L) << L;
    DecimTapArgs t;
    memset(&t, 0, sizeof(t));
    t.mask = tap_mask;
    for (int k = 1; k <= L; ++k) {
        if (!((tap_mask >> k) & 1u)) continue;
        const DecimShifts sh = decimated_shifts((unsigned)k, sampleSize); // the pair of decimate<2^k>_cen
        t.out[k] = taps->iq_out[k];
        t.stride[k] = S == 1 ? max_used >> k : taps->out_stride[k];
        t.norm[k] = (int)sh.norm; t.trunk[k] = (int)sh.trunk;
    }
    if (S == 1) in_stride = max_in;
    bool null_out = false, short_out = false, odd_out = false;
    for (int k = 1; k <= L; ++k) {
        if (!((tap_mask >> k) & 1u)) continue;
        null_out = null_out || !t.out[k];
        short_out = short_out || t.stride[k] < (max_used >> k);
        odd_out = odd_out || !aligned16(t.out[k]) || (S > 1 && (t.stride[k] & 3));
    }
    if (max_used && (!iq_in || null_out)) return fail(SDRHIP_EINVAL, "decimate_taps: NULL buffer");
    if (S > 1 && (in_stride < max_in || short_out)) return fail(SDRHIP_EINVAL, "decimate_taps: stride smaller than the largest count");
    if (mem == SDRHIP_MEM_DEVICE && max_used && (!aligned16(iq_in) || odd_out || (S > 1 && (in_stride & 3))))
        return fail(SDRHIP_EALIGN, "decimate_taps: device pointers must be 16-byte aligned and strides multiples of 4 samples");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<RaggedRow> rows((size_t)S);
    memset(rows.data(), 0, rows.size() * sizeof(RaggedRow));
    const RaggedRow *rdev = nullptr;
    RaggedPlan plan;
    int rc;
    if (max_used == 0) {
        d->last = DecimPlanInfo(); // no stream has a whole output sample of tap L: nothing enters any history, nothing is launched
    } else {
        for (int s = 0; s < S; ++s) rows[(size_t)s].shifts = ragged_shift_word((unsigned)L, sampleSize); // (the one-tap launch reads it)
        if ((rc = ragged_prepare(d, L, SDRHIP_FC_CEN, n_in, rows.data(), &rdev, &plan))) return rc;
        if (mem == SDRHIP_MEM_DEVICE) {
            if ((rc = decimate_taps_device(d, L, sampleSize, iq_in, in_stride, t, rows.data(), rdev, plan))) return rc;
        } else {
            // host rows: staged through device memory with padded (16-byte aligned) strides, the taps' banks one behind the other
            const size_t dis = (max_in + 3) & ~(size_t)3;
            size_t off[DECIM_TAP_SLOTS] = {0}, dos[DECIM_TAP_SLOTS] = {0}, total = 0;
            for (int k = 1; k <= L; ++k) {
                if (!((tap_mask >> k) & 1u)) continue;
                dos[k] = ((max_used >> k) + 3) & ~(size_t)3;
                off[k] = total;
                total += (size_t)S * dos[k] * 4;
            }
            const void *din = nullptr;
            if ((rc = taps_stage_in(d, iq_in, in_stride, n_in, dis, &din))) return rc;
            if ((rc = c->out.reserve(total + 16))) return rc;
            if ((rc = d->out_pin.reserve(total))) return rc;
            DecimTapArgs td = t;
            for (int k = 1; k <= L; ++k)
                if ((tap_mask >> k) & 1u) { td.out[k] = reinterpret_cast<int16_t *>(c->out.as<char>() + off[k]); td.stride[k] = dos[k]; }
            if ((rc = decimate_taps_device(d, L, sampleSize, static_cast<const int16_t *>(din), dis, td, rows.data(), rdev, plan))) return rc;
            // down: exactly the samples of the results -- one rectangle per tap when the counts agree, else row by row
            bool equal = true;
            for (int s = 1; s < S; ++s) equal = equal && rows[(size_t)s].n_used == rows[0].n_used;
            for (int k = 1; k <= L; ++k) {
                if (!((tap_mask >> k) & 1u)) continue;
                char *pin = d->out_pin.as<char>() + off[k];
                const char *dev = c->out.as<char>() + off[k];
                if (equal) {
                    HIP_TRY(link_copy2d(c, pin, dos[k] * 4, dev, dos[k] * 4, (max_used >> k) * 4, S, hipMemcpyDeviceToHost, c->stream));
                    continue;
                }
                for (int s = 0; s < S; ++s) {
                    const size_t n = (size_t)rows[(size_t)s].n_used >> k;
                    if (n) HIP_TRY(link_copy(c, pin + (size_t)s * dos[k] * 4, dev + (size_t)s * dos[k] * 4, n * 4, hipMemcpyDeviceToHost, c->stream));
                }
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (int k = 1; k <= L; ++k) {
                if (!((tap_mask >> k) & 1u)) continue;
                for (int s = 0; s < S; ++s) {
                    const size_t n = (size_t)rows[(size_t)s].n_used >> k;
                    if (n) memcpy(taps->iq_out[k] + (size_t)s * t.stride[k] * 2, d->out_pin.as<char>() + off[k] + (size_t)s * dos[k] * 4, n * 4);
                }
            }
        }
    }
    for (int s = 0; s < S; ++s) n_used[s] = (n_in[s] >> L) << L;
    for (int k = 1; k <= L; ++k)
        if ((tap_mask >> k) & 1u) taps->sample_size[k] = decimated_sample_size((unsigned)k, sampleSize);
    return SDRHIP_OK;
}
