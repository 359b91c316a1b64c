// sdrhip_pipes.cpp -- interpolator bank and the fused Rx / Tx pipes of include/sdrhip.h.
#include "gf256.h"
#include "sdrhip_host.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

using namespace sdrhip;

// --------------------------------------------------------------------------- interpolators
struct sdrhip_interpolators {
    sdrhip_ctx *ctx;
    int nstreams;
    int32_t *state[2]; // [nstreams][INT_STATE_WORDS]
    int cur;
};

extern "C" int sdrhip_interpolators_create(sdrhip_ctx *ctx, int nstreams, sdrhip_interpolators **out)
{
    if (!ctx || !out || nstreams <= 0 || nstreams > 65535) return fail(SDRHIP_EINVAL, "interpolators_create: bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    sdrhip_interpolators *p = new (std::nothrow) sdrhip_interpolators();
    if (!p) return fail(SDRHIP_ENOMEM, "out of host memory");
    p->ctx = ctx; p->nstreams = nstreams; p->cur = 0;
    size_t bytes = (size_t)nstreams * INT_STATE_WORDS * sizeof(int32_t);
    p->state[0] = p->state[1] = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&p->state[0]), bytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&p->state[1]), bytes) != hipSuccess) {
        if (p->state[0]) (void)hipFree(p->state[0]);
        delete p;
        return fail(SDRHIP_ENOMEM, "hipMalloc interpolator state");
    }
    ctx_retain(ctx);
    *out = p;
    return sdrhip_interpolators_reset(p);
}

extern "C" void sdrhip_interpolators_destroy(sdrhip_interpolators *p)
{
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    (void)hipFree(p->state[0]);
    (void)hipFree(p->state[1]);
    ctx_release(p->ctx);
    delete p;
}

extern "C" int sdrhip_interpolators_reset(sdrhip_interpolators *p)
{
    if (!p) return fail(SDRHIP_EINVAL, "interpolators is NULL");
    sdrhip::CtxLock lock_(p->ctx);
    size_t bytes = (size_t)p->nstreams * INT_STATE_WORDS * sizeof(int32_t);
    HIP_TRY(hipMemsetAsync(p->state[0], 0, bytes, p->ctx->stream));
    HIP_TRY(hipMemsetAsync(p->state[1], 0, bytes, p->ctx->stream));
    p->cur = 0;
    return SDRHIP_OK;
}

namespace sdrhip {
bool interpolate_gather_ok(const sdrhip_ctx *c, int log2interp) { return c->opt.interp_wave && log2interp >= 2; }

int interpolate_device(sdrhip_interpolators *p, int log2interp, const int16_t *in, size_t n_in, size_t in_stride, int16_t *out,
                       size_t out_stride, size_t *n_out, const InterpGather *gather, const InterpCount *count, int out_fmt)
{
    sdrhip_ctx *c = p->ctx;
    if (n_out) *n_out = n_in << log2interp;
    if (n_in == 0) return SDRHIP_OK;
    if (gather && !interpolate_gather_ok(p->ctx, log2interp)) return fail(SDRHIP_EINVAL, "internal: gathered input needs the wave interpolator");
    if (gather && count) return fail(SDRHIP_EINVAL, "internal: no ragged gather");
    if (gather && out_fmt != IQF_S16) return fail(SDRHIP_EINVAL, "internal: gathered input has int16 output only");
    if (log2interp == 0 && out_fmt == IQF_S8) { // the copy, narrowed (K6n)
        hipError_t e;
        {
            KTimer kt(c, SDRHIP_K_INTERPOLATE);
            e = launch_iq8_narrow(in, in_stride, reinterpret_cast<uint8_t *>(out), out_stride, n_in, p->nstreams, c->stream);
        }
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "narrow launch: %s", hipGetErrorString(e));
        return SDRHIP_OK;
    }
    if (log2interp == 0) { // Upsampler::process m_interp == 0: samples_out = samples_in (Upsampler.cpp:54-57)
        HIP_TRY(hipMemcpy2DAsync(out, out_stride * 4, in, in_stride * 4, n_in * 4, p->nstreams, hipMemcpyDeviceToDevice, c->stream));
        return SDRHIP_OK;
    }
    InterpArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.out = out; a.in_stride = in_stride; a.out_stride = out_stride; a.n_in = n_in;
    a.state_cur = p->state[p->cur]; a.state_next = p->state[p->cur ^ 1];
    a.nstreams = p->nstreams;
    if (gather) { a.gmap = gather->map; a.grx = gather->rx; a.grest = gather->restored; a.gframes = gather->frames; }
    if (count) { a.count = count->count; a.count_stride = count->stride; a.count_unit = count->unit; }
    // SDRHIP_INTERP_PATH = wave (K5w, default) | valu (K5); SDRHIP_INTERP_SPAN = segment length in inputs (tests)
    const bool use_wave = c->opt.interp_wave && log2interp >= 2;
    if (use_wave) plan_interpolate_wave(log2interp, n_in, p->nstreams, c->n_cu, c->opt.interp_span, &a.nsub_per_seg, &a.nseg);
    else plan_interpolate(log2interp, n_in, p->nstreams, &a.nsub_per_seg, &a.nseg);
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_INTERPOLATE);
        if (out_fmt == IQF_S8) {
            if (count) e = use_wave ? launch_interpolate_wave_ragged_s8(log2interp, a, c->stream) : launch_interpolate_ragged_s8(log2interp, a, c->stream);
            else e = use_wave ? launch_interpolate_wave_s8(log2interp, a, c->stream) : launch_interpolate_s8(log2interp, a, c->stream);
        } else if (count) e = use_wave ? launch_interpolate_wave_ragged(log2interp, a, c->stream) : launch_interpolate_ragged(log2interp, a, c->stream);
        else e = use_wave ? launch_interpolate_wave(log2interp, a, c->stream) : launch_interpolate(log2interp, a, c->stream);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "interpolate launch: %s", hipGetErrorString(e));
    p->cur ^= 1;
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
    if (mem != SDRHIP_MEM_HOST) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
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

// --------------------------------------------------------------------------- fused Rx pipe
struct sdrhip_rx {
    sdrhip_ctx *ctx;
    int nstreams;
    sdrhip_rx_config cfg;
    sdrhip_decimators *dec;
    // [nstreams][cap_frames][128 + nb_fec][512].  A call fills slots base_slot .. base_slot + done of
    // every stream; slot base_slot + done (the frame still being filled) is slot base_slot of the next
    // call, so the window slides and nothing is copied until it reaches the end of the area.
    DevBuf work;
    size_t cap_frames;        // frame slots per stream in `work`
    size_t base_slot;         // slot of the frame being filled
    uint64_t pending_samples; // decimated samples sitting in that slot (the partial frame)
    bool frame_open;          // it has its meta block (a frame was started)
    uint16_t frame_count;     // its m_frameCount
    // what sdrhip_rx_frames_view shows: the frames the last call DELIVERED
    const uint8_t *view_base = nullptr; // slot 0 of the delivered window of stream 0
    size_t view_stride = 0;             // bytes between streams
    size_t view_frames = 0;
    DevBuf lin[2];            // stream-order decimator output of a call that is framed by K2 (two: pipelined mode)
    int lin_sel = 0;
    DevBuf flist;             // frame list of the generic encode launch (device), relative to the window
    std::vector<int32_t> flist_host;
    size_t flist_done = 0, flist_cap = 0;
    // ---- pipelined mode (sdrhip_rx_set_pipelined): a call delivers the frames the PREVIOUS call completed; their
    // recovery blocks are computed by encoder workgroups inside this call's decimator launch (rx_fused_kernel)
    int pipelined = 0;
    struct Late {
        bool have = false;          // frames completed by the previous call wait for delivery
        bool encode = false;        // ... and still have to be encoded (k)
        Enc128Args k;
        const uint8_t *base = nullptr;
        size_t stride = 0, frames = 0, frame_bytes = 0;
        size_t slot0 = 0;           // window position inside `work` (overlap check of the sliding window), SIZE_MAX = other area
    } late;
    DevBuf old_work;          // the previous frame area after a re-allocation, kept while `late` points into it
    // overlap mode (option rx_fused = 3): the waiting encode runs on the context's second stream beside the next call's decimator.
    // ev_framed: recorded on the first stream when a call has written everything its deferred encode reads (decimator + K2);
    // ev_enc: recorded on the second stream behind the encode, the first stream waits for it before the frames are delivered
    hipEvent_t ev_framed = nullptr, ev_enc = nullptr;
    // ---- asynchronous host-pointer entry (sdrhip_rx_submit / sdrhip_rx_collect): a ring of batches
    struct Batch {
        PinnedBuf in;             // the submitted blocks, appended: [block][stream][n] (unless the caller's memory is pinned by us)
        DevBuf din;               // [stream][dstride] on the device
        PinnedBuf out;            // the batch's finished frames [stream][frames][128 + R][512]
        hipEvent_t done = nullptr;
        std::vector<std::pair<const int16_t *, size_t> > blocks; // source of each block (host address, samples per stream) and
        std::vector<size_t> strides;                             // its stream stride in samples
        size_t n_in = 0;          // samples per stream so far
        size_t in_cap = 0;        // row length of `in` in samples: staged blocks lie stream-major, [stream][in_cap], at their batch offset
        uint32_t tv_sec = 0, tv_usec = 0;
        size_t frames = 0, frame_bytes = 0;
        int state = 0;            // 0 free, 1 filling, 2 in flight
        // ---- a ragged batch (sdrhip_rx_submit_ragged; a batch holds one kind only): blocks of per-stream counts, packed
        bool ragged = false;
        struct Run { const char *p; size_t off, bytes; }; // packed bytes of one block: in place at p, or staged at `in` + off (p NULL)
        std::vector<Run> r_runs;
        std::vector<size_t> r_cnt;            // [block][stream] counts
        std::vector<size_t> r_tot;            // per-stream samples so far
        std::vector<uint32_t> r_sec, r_usec;  // the stamps of the batch's first block
        size_t r_used = 0;                    // staged bytes in `in`
        std::vector<size_t> r_frames;         // frames per stream of the launched batch, in stream order in `out`
        PinnedBuf r_tab;                      // K0p's table, then the frame list of the download
    };
    std::vector<Batch> abatch;
    DevBuf a_pk, a_din, a_tab, a_frames;      // ragged batches on the device: packed upload, K0p's rows, tables, compacted frames
    int a_blocks = 1;             // blocks per launch
    bool consumed = false;        // set by sdrhip_rx_process once the decimator launch of the call went out (the filter state advanced)
    size_t a_head = 0, a_tail = 0; // next batch to collect / batch being filled
    // ---- input format (sdrhip_rx_set_input_format): 8-bit input is widened by K0 into `wide`, the decimator's int16 input
    int in_fmt = IQF_S16;
    DevBuf wide;
    // ---- ragged calls (sdrhip_rx_process_ragged): per-stream framing state.  While `diverged` the vectors hold it (the scalars
    // above are stale) and every Rx call takes the ragged path; when a call leaves every stream at the same position the scalars
    // take over again
    bool diverged = false;
    std::vector<size_t> r_base;        // base_slot per stream
    std::vector<uint64_t> r_pending;   // pending_samples per stream
    std::vector<uint8_t> r_open;       // frame_open per stream
    std::vector<uint16_t> r_count;     // frame_count per stream
    std::vector<size_t> r_view_first, r_view_frames; // sdrhip_rx_frames_view_ragged: the frames the last call delivered
    bool view_ragged = false;          // the last call's windows differ between streams: sdrhip_rx_frames_view refuses
    PinnedBuf r_pin, r_flist_pin;      // host-row staging and the encoder's frame list
    DevBuf r_flist;
};

static int rx_check_config(const sdrhip_rx_config *cfg);

extern "C" int sdrhip_rx_create(sdrhip_ctx *ctx, int nstreams, const sdrhip_rx_config *cfg, sdrhip_rx **out)
{
    if (!ctx || !cfg || !out || nstreams <= 0) return fail(SDRHIP_EINVAL, "rx_create: bad argument");
    {
        const int rcc = rx_check_config(cfg);
        if (rcc) return rcc;
    }
    sdrhip_rx *rx = new (std::nothrow) sdrhip_rx();
    if (!rx) return fail(SDRHIP_ENOMEM, "out of host memory");
    rx->ctx = ctx; rx->nstreams = nstreams; rx->cfg = *cfg; rx->dec = nullptr;
    rx->cap_frames = 0; rx->base_slot = 0; rx->pending_samples = 0; rx->frame_open = false; rx->frame_count = 0;
    int rc = sdrhip_decimators_create(ctx, nstreams, cfg->hb_variant, &rx->dec);
    if (rc) { delete rx; return rc; }
    *out = rx;
    return SDRHIP_OK;
}

static int rx_check_config(const sdrhip_rx_config *cfg)
{
    if (cfg->log2decim < 0 || cfg->log2decim > 6) return fail(SDRHIP_EINVAL, "Invalid log2 decimation factor");
    if (cfg->fcpos < 0 || cfg->fcpos > 2) return fail(SDRHIP_EINVAL, "Invalid Fc position index");
    if (cfg->nb_fec < 0 || cfg->nb_fec > 128) return fail(SDRHIP_EINVAL, "nb_fec must be 0..128");
    if (cfg->sample_bits < 1 || cfg->sample_bits > 16) return fail(SDRHIP_EINVAL, "sample_bits must be 1..16");
    return SDRHIP_OK;
}

// the encode that a pipelined call left for the next launch, now (flush, reconfiguration, a call that cannot fuse it)
static int rx_settle(sdrhip_rx *rx)
{
    if (!rx->late.encode) return SDRHIP_OK;
    rx->late.encode = false;
    sdrhip_ctx *c = rx->ctx;
    if (c->opt.rx_fused != 3 || !rx->ev_framed) return fec_encode128_launch(c, rx->late.k);
    // overlap mode: the encode goes to the second stream -- behind everything the call that left it had enqueued (ev_framed), beside
    // whatever the first stream runs now (the decimator of the current call, enqueued just before) -- and the first stream picks
    // up behind it: the frames are delivered, and the buffers reused, in first-stream order
    hipStream_t s2 = nullptr;
    int rc = ctx_stream2(c, &s2);
    if (rc) return rc;
    if (!rx->ev_enc) HIP_TRY(hipEventCreateWithFlags(&rx->ev_enc, hipEventDisableTiming));
    HIP_TRY(hipStreamWaitEvent(s2, rx->ev_framed, 0));
    if ((rc = fec_encode128_launch(c, rx->late.k, s2))) return rc;
    HIP_TRY(hipEventRecord(rx->ev_enc, s2));
    HIP_TRY(hipStreamWaitEvent(c->stream, rx->ev_enc, 0));
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_set_pipelined(sdrhip_rx *rx, int on)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (!on && rx->late.have) return fail(SDRHIP_EINVAL, "rx_set_pipelined: sdrhip_rx_flush the waiting frames first");
    if (on && rx->diverged) return fail(SDRHIP_EINVAL, "rx_set_pipelined: ragged calls left the streams at different frame positions");
    rx->pipelined = on ? 1 : 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_set_input_format(sdrhip_rx *rx, int fmt)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (fmt != SDRHIP_IQ_S16 && fmt != SDRHIP_IQ_U8 && fmt != SDRHIP_IQ_S8) return fail(SDRHIP_EINVAL, "rx_set_input_format: unknown format %d", fmt);
    for (const auto &b : rx->abatch)
        if (b.state != 0) return fail(SDRHIP_EINVAL, "rx_set_input_format: asynchronous batches are being filled or in flight: collect them first");
    if (rx->late.have) return fail(SDRHIP_EINVAL, "rx_set_input_format: frames of the previous call wait for delivery (pipelined mode): sdrhip_rx_flush them first");
    rx->in_fmt = fmt;
    return SDRHIP_OK;
}

// K0: 8-bit rows (in_stride a multiple of 8 samples, or one stream) -> rx->wide [stream][dstride] int16, ahead of the decimator
static int rx_widen(sdrhip_rx *rx, const uint8_t *in, size_t in_stride, size_t n_in, size_t dstride, const int16_t **din)
{
    sdrhip_ctx *c = rx->ctx;
    int rc = rx->wide.reserve((size_t)rx->nstreams * dstride * 4 + 16);
    if (rc) return rc;
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_CONVERT);
        e = launch_iq8_widen(rx->in_fmt, in, in_stride, rx->wide.as<int16_t>(), dstride, n_in, rx->nstreams, c->stream);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "widen launch: %s", hipGetErrorString(e));
    *din = rx->wide.as<int16_t>();
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_reconfigure(sdrhip_rx *rx, const sdrhip_rx_config *cfg)
{
    if (!rx || !cfg) return fail(SDRHIP_EINVAL, "rx_reconfigure: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    int rc = rx_check_config(cfg);
    if (rc) return rc;
    if (cfg->hb_variant != rx->cfg.hb_variant) return fail(SDRHIP_EINVAL, "rx_reconfigure: hb_variant is fixed at creation");
    sdrhip_ctx *c = rx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (cfg->nb_fec != rx->cfg.nb_fec && rx->late.have)
        return fail(SDRHIP_EINVAL, "rx_reconfigure: frames of the previous call wait for delivery (pipelined mode): sdrhip_rx_flush them "
                                   "before changing fecblk (they carry the old frame size)");
    if (cfg->nb_fec != rx->cfg.nb_fec && rx->cap_frames) {
        // the slots change size: the frame being filled (its 128 original super blocks) moves to slot 0 of a new area
        if ((rc = rx_settle(rx))) return rc;
        const int S = rx->nstreams;
        const size_t old_fb = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
        const size_t new_fb = (size_t)(SDRHIP_NB_ORIGINAL + cfg->nb_fec) * SDRHIP_UDPSIZE;
        DevBuf fresh;
        if ((rc = fresh.reserve((size_t)S * rx->cap_frames * new_fb))) return rc;
        if (rx->diverged) { // (per-stream windows: each open frame moves to slot 0 of its stream)
            for (int s = 0; s < S; ++s) {
                if (rx->r_open[(size_t)s])
                    HIP_TRY(hipMemcpyAsync(fresh.as<uint8_t>() + (size_t)s * rx->cap_frames * new_fb,
                                           rx->work.as<uint8_t>() + (size_t)s * rx->cap_frames * old_fb + rx->r_base[(size_t)s] * old_fb,
                                           (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, hipMemcpyDeviceToDevice, c->stream));
                rx->r_base[(size_t)s] = 0;
            }
        } else if (rx->frame_open)
            HIP_TRY(hipMemcpy2DAsync(fresh.p, rx->cap_frames * new_fb, rx->work.as<uint8_t>() + rx->base_slot * old_fb,
                                     rx->cap_frames * old_fb, (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, S, hipMemcpyDeviceToDevice,
                                     c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // earlier launches may still use the old area
        // (no frames wait for delivery here: a fecblk change with late.have set was refused above)
        rx->old_work.release();
        rx->work.release();
        rx->work = fresh;
        rx->base_slot = 0;
        rx->view_base = nullptr;
        rx->view_frames = 0;
        rx->view_ragged = false;
    }
    rx->cfg = *cfg;
    return SDRHIP_OK;
}

extern "C" void sdrhip_rx_destroy(sdrhip_rx *rx)
{
    if (!rx) return;
    sdrhip_decimators_destroy(rx->dec);
    rx->work.release();
    rx->old_work.release();
    rx->lin[0].release();
    rx->lin[1].release();
    rx->flist.release();
    rx->wide.release();
    rx->r_pin.release(); rx->r_flist_pin.release(); rx->r_flist.release();
    if (rx->ev_framed) (void)hipEventDestroy(rx->ev_framed);
    if (rx->ev_enc) (void)hipEventDestroy(rx->ev_enc);
    for (auto &b : rx->abatch) {
        if (b.done) { (void)hipEventSynchronize(b.done); (void)hipEventDestroy(b.done); }
        b.in.release(); b.din.release(); b.out.release(); b.r_tab.release();
    }
    rx->a_pk.release(); rx->a_din.release(); rx->a_tab.release(); rx->a_frames.release();
    delete rx;
}

extern "C" int sdrhip_rx_frames_view(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes, size_t *n_frames)
{
    if (!rx || !base || !stream_stride_bytes || !n_frames) return fail(SDRHIP_EINVAL, "rx_frames_view: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    if (rx->view_ragged) return fail(SDRHIP_EINVAL, "rx_frames_view: the last call's windows differ between streams: use sdrhip_rx_frames_view_ragged");
    *base = rx->view_base;
    *stream_stride_bytes = rx->view_stride;
    *n_frames = rx->view_frames;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_frames_view_ragged(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes, size_t *first_slot,
                                            size_t *n_frames)
{
    if (!rx || !base || !stream_stride_bytes || !first_slot || !n_frames) return fail(SDRHIP_EINVAL, "rx_frames_view_ragged: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    const int S = rx->nstreams;
    const size_t fb = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
    if (rx->view_ragged) {
        *base = rx->work.as<uint8_t>();
        *stream_stride_bytes = rx->cap_frames * fb;
        for (int s = 0; s < S; ++s) { first_slot[s] = rx->r_view_first[(size_t)s]; n_frames[s] = rx->r_view_frames[(size_t)s]; }
        return SDRHIP_OK;
    }
    // (the last call delivered the same window of every stream: the uniform view, as slot offsets from the area)
    const size_t slot = rx->view_base && rx->work.p && rx->view_base >= rx->work.as<uint8_t>() && rx->view_stride == rx->cap_frames * fb
                            ? (size_t)(rx->view_base - rx->work.as<uint8_t>()) / fb : 0;
    *base = rx->view_base ? rx->view_base - slot * fb : nullptr;
    *stream_stride_bytes = rx->view_stride;
    for (int s = 0; s < S; ++s) { first_slot[s] = slot; n_frames[s] = rx->view_frames; }
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_last_plan(const sdrhip_rx *rx, sdrhip_decim_plan *out)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    return sdrhip_decimators_last_plan(rx->dec, out);
}

extern "C" size_t sdrhip_rx_max_frames(const sdrhip_rx *rx, size_t n_in)
{
    if (!rx) return 0;
    sdrhip::CtxLock lock_(rx->ctx);
    if (rx->diverged) { // (ragged calls left the streams at different positions: the stream that completes the most)
        size_t most = 0;
        for (size_t s = 0; s < rx->r_pending.size(); ++s) {
            const size_t f = (size_t)((rx->r_pending[s] + (n_in >> rx->cfg.log2decim)) / SDRHIP_SAMPLES_PER_FRAME);
            if (f > most) most = f;
        }
        return most;
    }
    const size_t now = (size_t)((rx->pending_samples + (n_in >> rx->cfg.log2decim)) / SDRHIP_SAMPLES_PER_FRAME);
    if (!rx->pipelined) return now;
    return rx->late.have && rx->late.frames > now ? rx->late.frames : now; // (a pipelined call delivers the previous call's frames)
}

// delivery of a finished window: optional copy to the caller's buffer, and the zero-copy view
static int rx_deliver(sdrhip_rx *rx, const uint8_t *base, size_t stride, size_t frames, size_t frame_bytes, uint8_t *frames_out,
                      size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    if (frames && frames_out) {
        if (S > 1 && frame_stride_bytes < frames * frame_bytes) return fail(SDRHIP_EINVAL, "rx_process: frame stride too small");
        HIP_TRY(link_copy2d(c, frames_out, S > 1 ? frame_stride_bytes : frames * frame_bytes, base, stride, frames * frame_bytes, S,
                            mem == SDRHIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    } else if (frames && mem != SDRHIP_MEM_DEVICE) {
        return fail(SDRHIP_EINVAL, "rx_process: NULL frames_out");
    }
    rx->view_base = base; rx->view_stride = stride; rx->view_frames = frames;
    rx->view_ragged = false;
    if (n_frames) *n_frames = frames;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_flush(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (n_frames) *n_frames = 0;
    if (mem != SDRHIP_MEM_HOST && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    if (!rx->late.have) { rx->view_frames = 0; return SDRHIP_OK; }
    HIP_TRY(hipSetDevice(rx->ctx->device));
    int rc;
    if ((rc = rx_settle(rx))) return rc;
    if ((rc = rx_deliver(rx, rx->late.base, rx->late.stride, rx->late.frames, rx->late.frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
    rx->late.have = false;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(rx->ctx->stream));
    return SDRHIP_OK;
}

static int rx_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                     const uint32_t *tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem, bool batch = false);

// batches of the ring that are being filled or in flight, of the ragged (or the uniform) kind
static bool rx_has_batches(const sdrhip_rx *rx, bool ragged)
{
    for (const auto &b : rx->abatch)
        if (b.state != 0 && b.ragged == ragged) return true;
    return false;
}

extern "C" int sdrhip_rx_process(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec, uint32_t tv_usec,
                                 uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (n_frames) *n_frames = 0;
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_process: ragged batches are being filled or in flight: collect them first");
    if (rx->diverged && n_in) {
        // ragged calls left the streams at different frame positions: a ragged call with equal counts and stamps; *n_frames = the
        // largest per-stream count (sdrhip_rx_frames_view_ragged has each)
        const size_t S = (size_t)rx->nstreams;
        std::vector<size_t> cnt(S, n_in), nf(S, 0);
        std::vector<uint32_t> sec(S, tv_sec), usec(S, tv_usec);
        const int rc = rx_ragged(rx, iq_in, cnt.data(), in_stride, sec.data(), usec.data(), frames_out, frame_stride_bytes, nf.data(), mem);
        if (rc) return rc;
        size_t most = 0;
        for (size_t s = 0; s < S; ++s) if (nf[s] > most) most = nf[s];
        if (n_frames) *n_frames = most;
        return SDRHIP_OK;
    }
    if (n_in == 0) {
        // an empty call completes nothing; in pipelined mode it still DELIVERS what the previous call completed (the header's
        // contract: every call delivers the frames of the one before it)
        if (rx->pipelined && rx->late.have) return sdrhip_rx_flush(rx, frames_out, frame_stride_bytes, n_frames, mem);
        rx->view_frames = 0;
        rx->view_ragged = false;
        return SDRHIP_OK;
    }
    if (!iq_in) return fail(SDRHIP_EINVAL, "rx_process: NULL input");
    sdrhip_ctx *c = rx->ctx;
    rx->consumed = false;
    HIP_TRY(hipSetDevice(c->device));
    const int S = rx->nstreams, L = rx->cfg.log2decim, R = rx->cfg.nb_fec;
    const int FB = SDRHIP_NB_ORIGINAL + R;
    const size_t frame_bytes = (size_t)FB * SDRHIP_UDPSIZE;
    const size_t n_dec = n_in >> L;
    const uint64_t total = rx->pending_samples + n_dec;
    const size_t done = (size_t)(total / SDRHIP_SAMPLES_PER_FRAME);
    const uint64_t rest = total - (uint64_t)done * SDRHIP_SAMPLES_PER_FRAME;
    if (S == 1) in_stride = n_in;
    const size_t deliver_now = rx->pipelined ? (rx->late.have ? rx->late.frames : 0) : done;
    const size_t deliver_fb = rx->pipelined && rx->late.have ? rx->late.frame_bytes : frame_bytes;
    if (deliver_now && !frames_out && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "rx_process: NULL frames_out");
    if (frames_out && S > 1 && deliver_now && frame_stride_bytes < deliver_now * deliver_fb) return fail(SDRHIP_EINVAL, "rx_process: frame stride too small");

    const int16_t *din = iq_in;
    size_t dstride = in_stride;
    int rc;
    if (rx->in_fmt != IQF_S16 && (mem == SDRHIP_MEM_HOST || mem == SDRHIP_MEM_DEVICE)) {
        // 8-bit input: 2 bytes per sample cross the link (rows of a multiple of 8 samples: K0's 16-byte loads), K0 widens them into
        // rx->wide, which the decimator reads as it reads int16 input
        const uint8_t *src = reinterpret_cast<const uint8_t *>(iq_in), *d8 = src;
        size_t sstride = in_stride;
        if (mem == SDRHIP_MEM_HOST) {
            sstride = (n_in + 7) & ~(size_t)7;
            if ((size_t)S * sstride * 2 <= SDRHIP_ZEROCOPY_MAX) { // (small call: K0 reads the pinned rows itself, as the decimator does for int16)
                if ((rc = c->zin.reserve((size_t)S * sstride * 2 + 16))) return rc;
                for (int s = 0; s < S; ++s) memcpy(c->zin.as<uint8_t>() + (size_t)s * sstride * 2, src + (size_t)s * in_stride * 2, n_in * 2);
                link_bytes(c, hipMemcpyHostToDevice, (size_t)S * n_in * 2);
                d8 = c->zin.as<uint8_t>();
            } else {
                if ((rc = c->in.reserve((size_t)S * sstride * 2 + 16))) return rc;
                HIP_TRY(link_copy2d(c, c->in.p, sstride * 2, src, in_stride * 2, n_in * 2, S, hipMemcpyHostToDevice, c->stream));
                d8 = c->in.as<uint8_t>();
            }
        } else if (!aligned16(iq_in) || (S > 1 && (in_stride & 7))) {
            return fail(SDRHIP_EALIGN, "rx_process: 8-bit device input must be 16-byte aligned, its stride a multiple of 8 samples");
        }
        dstride = (n_in + 3) & ~(size_t)3;
        if ((rc = rx_widen(rx, d8, sstride, n_in, dstride, &din))) return rc;
    } else if (mem == SDRHIP_MEM_HOST) {
        dstride = (n_in + 3) & ~(size_t)3;
        if ((size_t)S * dstride * 4 <= SDRHIP_ZEROCOPY_MAX) {
            // small call: the decimator reads pinned host memory itself (no copy engine in front of the launch); the buffer is
            // free again when this call returns (host-pointer calls end with a stream synchronisation)
            if ((rc = c->zin.reserve((size_t)S * dstride * 4 + 16))) return rc;
            for (int s = 0; s < S; ++s) memcpy(c->zin.as<int16_t>() + (size_t)s * dstride * 2, iq_in + (size_t)s * in_stride * 2, n_in * 4);
            link_bytes(c, hipMemcpyHostToDevice, (size_t)S * n_in * 4); // (read by the decimator over the link)
            din = c->zin.as<int16_t>();
        } else {
            if ((rc = c->in.reserve((size_t)S * dstride * 4 + 16))) return rc;
            HIP_TRY(link_copy2d(c, c->in.p, dstride * 4, iq_in, in_stride * 4, n_in * 4, S, hipMemcpyHostToDevice, c->stream));
            din = c->in.as<int16_t>();
        }
    } else if (mem == SDRHIP_MEM_DEVICE) {
        if (!aligned16(iq_in) || (S > 1 && (in_stride & 3))) return fail(SDRHIP_EALIGN, "rx_process: device input must be 16-byte aligned");
    } else {
        return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    }

    // ---- work area [stream][slot][128 + R][512]: this call fills slots base_slot .. base_slot + done.  The
    // finished frames stay readable in place until the next call (sdrhip_rx_frames_view); the frame still
    // being filled is the first slot of the next call.  At the end of the area the window wraps: the open
    // frame moves to slot 0 (one strided copy every few calls instead of a save + restore per call).  Frames that
    // wait for delivery (pipelined mode) are never overwritten: a window that would reach them gets a new area.
    const size_t need = done + 1;
    if (rx->old_work.p && !(rx->late.have && rx->late.slot0 == SIZE_MAX)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        rx->old_work.release();
    }
    if (rx->base_slot + need > rx->cap_frames) {
        const bool late_here = rx->late.have && rx->late.slot0 != SIZE_MAX;
        const bool wrap_hits_late = late_here && need > rx->late.slot0; // the wrapped window [0, need) against [slot0, slot0 + frames)
        if (need > rx->cap_frames || wrap_hits_late) {
            DevBuf bigger;
            // the window: TWO calls' frames (round 5; four until then).  The step rewrites what it wrote two calls ago: 2 x 84 MB per
            // 8-stream bank stay in the 256 MB of Infinity Cache, and on this memory system a write stream that stays there
            // costs the read stream beside it less (profiles/r05_rx_direct.txt: decimator launch 0.2435 -> 0.2335 ms, encoder
            // launch 0.052 -> 0.049 ms; a window of one call wraps -- a copy of the open frames -- on every call).  option rx_window (SDRHIP_RX_WINDOW at context creation, 1..8) = A / B
            // (pipelined pipes keep the previous call's frames until they are delivered: four calls, as before)
            const size_t wmul = c->opt.rx_window ? (size_t)c->opt.rx_window : rx->pipelined ? 4 : 2;
            const size_t ncap = need > rx->cap_frames ? wmul * need : rx->cap_frames;
            if ((rc = bigger.reserve((size_t)S * ncap * frame_bytes))) return rc;
            if (rx->frame_open)
                HIP_TRY(hipMemcpy2DAsync(bigger.p, ncap * frame_bytes, rx->work.as<uint8_t>() + rx->base_slot * frame_bytes,
                                         rx->cap_frames * frame_bytes, frame_bytes, S, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream)); // earlier launches may still use the old area
            if (late_here) { rx->old_work.release(); rx->old_work = rx->work; rx->late.slot0 = SIZE_MAX; }
            else rx->work.release();
            rx->work = bigger;
            rx->cap_frames = ncap;
        } else if (rx->frame_open) {
            uint8_t *w0 = rx->work.as<uint8_t>();
            HIP_TRY(hipMemcpy2DAsync(w0, rx->cap_frames * frame_bytes, w0 + rx->base_slot * frame_bytes, rx->cap_frames * frame_bytes,
                                     frame_bytes, S, hipMemcpyDeviceToDevice, c->stream));
        }
        rx->base_slot = 0;
    }
    const size_t stream_bytes = rx->cap_frames * frame_bytes;
    uint8_t *work = rx->work.as<uint8_t>() + rx->base_slot * frame_bytes; // slot 0 of the window

    // ---- meta record of the frames started by this call (UDPSinkFEC.cpp:87-132); the decimator kernel writes
    // their meta blocks and super block headers on its way
    unsigned ss = rx->cfg.sample_bits;
    const int first_new = rx->frame_open ? 1 : 0;
    const int started = (int)(done + (rest > 0 ? 1 : 0)) - first_new; // frames whose first sample arrives now
    RxMeta meta;
    memset(&meta, 0, sizeof(meta));
    if (started > 0) {
        const unsigned ssd = decimated_sample_size((unsigned)L, ss);
        uint8_t m[24];
        const uint32_t fc = rx->cfg.center_frequency_khz, sr = rx->cfg.sample_rate;
        memcpy(m + 0, &fc, 4); memcpy(m + 4, &sr, 4);
        m[8] = (uint8_t)((ssd - 1) / 8 + 1); // setSampleBytes((sampleSize - 1) / 8 + 1), sdrdaemonrx.cpp:643
        m[9] = (uint8_t)ssd;                 // setSampleBits(sampleSize), :642
        m[10] = SDRHIP_NB_ORIGINAL; m[11] = (uint8_t)R;
        // tv_sec / tv_usec = the stamp of the call's first sample; a frame's own stamp (the reference calls gettimeofday when it
        // opens the frame, UDPSinkFEC.cpp:90-104) is that plus its first sample's offset on the sample clock, and the
        // boost::crc_32_type over the first 20 bytes (:106-109) follows from it: both per frame on the device (frame_meta_words)
        // (m[20..23] = the CRC of the record with a ZERO stamp: the affine part of the per-frame CRC, see frame_meta_words)
        memset(m + 12, 0, 8);
        uint32_t crc = 0xFFFFFFFFu;
        for (int i = 0; i < 20; ++i) {
            crc ^= m[i];
            for (int k = 0; k < 8; ++k) crc = (crc & 1) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
        }
        crc ^= 0xFFFFFFFFu;
        memcpy(m + 12, &tv_sec, 4); memcpy(m + 16, &tv_usec, 4); memcpy(m + 20, &crc, 4);
        meta.first = first_new; meta.count = started; meta.frame_count0 = (unsigned)rx->frame_count + first_new;
        memcpy(meta.w, m, 24);
        meta.idx0 = first_new ? (uint64_t)SDRHIP_SAMPLES_PER_FRAME - rx->pending_samples : 0;
        meta.rate = sr;
    }

    size_t n_out = 0;
    EncodeLin elin;
    bool use_lin = false, pack_with_encoder = false;
    FrameArgs fa;
    memset(&fa, 0, sizeof(fa));
    const bool structured = R >= enc128_min_rows(c) && frame_bytes % 4 == 0; // gf_encode128_kernel serves this setting
    const bool filterless = L == 0 || (rx->cfg.fcpos != SDRHIP_FC_CEN && L <= 2); // Decimators.cpp:22-91,127-170: no cascade kernel
    const Enc128Args *fuse = rx->late.encode && (c->opt.rx_fused == 1 || c->opt.rx_fused == 2) ? &rx->late.k : nullptr;
    // overlap mode: the waiting encode will run on the second stream BESIDE this call's decimator (rx_settle below), which therefore
    // leaves room on its CUs (ring depth 3) and raises its waves' priority
    const bool coresident = rx->late.encode && c->opt.rx_fused == 3 && rx->ev_framed;
    bool fused = false;
    // (matrix-core decimator: stream order + K2 + the encoder's fused copy, unless its waves frame their output themselves)
    const bool direct = c->opt.rx_direct && !rx->pipelined && stream_bytes < 0x3fffffffu;
    if (filterless || (!direct && decimate_mfma_applies(rx->dec, L, rx->cfg.fcpos, n_in))) {
        // ---- decimate in stream order, then K2 lays the samples out as super blocks (+ meta blocks and headers)
        const size_t lstride = (n_dec + 3) & ~(size_t)3;
        if (rx->pipelined) rx->lin_sel ^= 1; // (the deferred encoder of the previous call still reads the other one)
        DevBuf &lin = rx->lin[rx->lin_sel];
        if (lin.cap < (size_t)S * lstride * 4 + 16 && rx->late.encode) { if ((rc = rx_settle(rx))) return rc; fuse = nullptr; HIP_TRY(hipStreamSynchronize(c->stream)); }
        if ((rc = lin.reserve((size_t)S * lstride * 4 + 16))) return rc;
        rc = decimate_device(rx->dec, L, rx->cfg.fcpos, &ss, din, n_in, dstride, lin.as<int16_t>(), lstride, &n_out, 0, 0, 0, nullptr, fuse, &fused, coresident);
        if (rc) return rc;
        rx->consumed = true;
        if (fused) rx->late.encode = false;
        // the frames that lie entirely inside this call's samples are laid out by the encoder (fused copy); K2 does
        // the frame that was open when the call began, the one left open at its end, meta blocks and headers
        if (fec_encode_fuses_framing(c, R)) {
            const size_t first = rx->pending_samples ? 1 : 0;
            if (done > first && frame_bytes % 4 == 0) {
                elin.lin = lin.as<unsigned>(); elin.stride = lstride; elin.cap = (int)rx->cap_frames;
                elin.first = (int)first; elin.pending = (int)rx->pending_samples;
                use_lin = true;
            }
        }
        if (use_lin) {
            fa.skip_from = (size_t)elin.first * SDRHIP_SAMPLES_PER_FRAME - (size_t)elin.pending;
            fa.skip_to = done * SDRHIP_SAMPLES_PER_FRAME - (size_t)elin.pending;
        }
        fa.in = lin.as<unsigned>(); fa.out = reinterpret_cast<unsigned *>(work);
        fa.in_stride = lstride; fa.out_stride = stream_bytes / 4;
        fa.n = n_dec; fa.frame_sample_base = rx->pending_samples; fa.frame_blocks = FB;
        fa.meta_first = meta.first; fa.meta_count = meta.count; fa.meta_frame_count0 = meta.frame_count0;
        memcpy(fa.meta_w, meta.w, sizeof(fa.meta_w));
        fa.meta_idx0 = meta.idx0; fa.meta_rate = meta.rate;
        // K2 rides in the encoder's launch when this call's frames are encoded right away by the structured encoder (one launch
        // less per step); otherwise it goes out now
        pack_with_encoder = !rx->pipelined && c->opt.rx_fused && structured && R > 0 && use_lin;
        if (!pack_with_encoder) {
            hipError_t e = launch_frame_pack(fa, S, c->stream);
            if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "frame pack launch: %s", hipGetErrorString(e));
        }
    } else {
        // ---- decimate straight into the frame layout (VALU cascade kernel with the framing epilogue, or the matrix-core kernel
        // with its frame-layout stores and the VALU pieces' epilogue for meta blocks and headers)
        rc = decimate_device(rx->dec, L, rx->cfg.fcpos, &ss, din, n_in, dstride, reinterpret_cast<int16_t *>(work), stream_bytes / 4, &n_out, 1,
                             FB, rx->pending_samples, &meta);
        if (rc) return rc;
        rx->consumed = true;
    }
    if ((rc = rx_settle(rx))) return rc; // (a waiting encode that this call's launch could not take along)

    // ---- FEC over the completed frames of every stream, recovery blocks land behind block 127
    bool encode_later = false;
    Enc128Args k;
    memset(&k, 0, sizeof(k));
    if (done && R > 0) {
        if (structured) {
            // structured encoder, one workgroup per (frame, half block); frame (s, f) of the window is frame s * cap_frames + f
            k.in = work; k.out = work + (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE; k.tab = c->gf_tab; k.leaf_tables = c->enc_leaves; k.fft_tables = c->enc_fft; k.use_fft = c->opt.enc_fft;
            k.bitslice = c->opt.enc_bitslice;
            k.in_frame_bytes = frame_bytes; k.out_frame_bytes = frame_bytes;
            k.rows = R; k.nframes = (int)((size_t)S * rx->cap_frames);
            k.nlist = (int)((size_t)S * done); k.gen_done = (int)done; k.gen_cap = (int)rx->cap_frames;
            if (use_lin) { k.lin = elin.lin; k.lin_stride = elin.stride; k.lin_cap = elin.cap; k.lin_first = elin.first; k.lin_pending = elin.pending; }
            if (rx->pipelined) {
                encode_later = true; // rides in the next call's decimator launch (or sdrhip_rx_flush)
            } else if (pack_with_encoder) {
                // encoder + K2 in one launch: the encoder derives the meta blocks of the frames this call starts itself and
                // completes the frame that was open (its tail comes from the stream-order buffer), K2 leaves both alone
                k.meta_first = meta.first; k.meta_count = meta.count; k.meta_frame_count0 = meta.frame_count0;
                memcpy(k.meta_w, meta.w, sizeof(k.meta_w));
                k.meta_idx0 = meta.idx0; k.meta_rate = meta.rate;
                if (elin.first == 1) { k.lin_straddle = 1; fa.skip_from = 0; }
                hipError_t e;
                {
                    KTimer kt(c, SDRHIP_K_FEC_ENCODE);
                    e = launch_gf_encode128_pack(k, fa, S, c->stream);
                }
                if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "encode + frame pack launch: %s", hipGetErrorString(e));
            } else if ((rc = fec_encode128_launch(c, k))) return rc;
        } else {
            // generic matrix kernel: one launch for every stream, frame list in groups of GF_FRAMES_PER_GROUP
            if (rx->flist_done != done || rx->flist_cap != rx->cap_frames) {
                HIP_TRY(hipStreamSynchronize(c->stream)); // a previous upload may still read flist_host
                rx->flist_host.clear();
                for (int s = 0; s < S; ++s)
                    for (size_t f = 0; f < done; ++f) rx->flist_host.push_back((int32_t)(s * rx->cap_frames + f));
                while (rx->flist_host.size() % GF_FRAMES_PER_GROUP) rx->flist_host.push_back(-1);
                if ((rc = rx->flist.reserve(rx->flist_host.size() * 4))) return rc;
                HIP_TRY(link_copy(c, rx->flist.p, rx->flist_host.data(), rx->flist_host.size() * 4, hipMemcpyHostToDevice, c->stream));
                rx->flist_done = done; rx->flist_cap = rx->cap_frames;
            }
            if ((rc = fec_encode_device(c, work, frame_bytes, (size_t)S * rx->cap_frames, R, work + (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE,
                                        frame_bytes, rx->flist.as<int32_t>(), (int)(rx->flist_host.size() / GF_FRAMES_PER_GROUP), nullptr)))
                return rc;
        }
    }
    // ---- delivery: this call's frames, or (pipelined) the previous call's, whose encode went out above
    if (rx->pipelined) {
        if (rx->late.have) {
            if ((rc = rx_deliver(rx, rx->late.base, rx->late.stride, rx->late.frames, rx->late.frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
        } else {
            rx->view_base = nullptr; rx->view_frames = 0; rx->view_ragged = false;
        }
        rx->late.have = done > 0;
        rx->late.encode = encode_later;
        if (encode_later && c->opt.rx_fused == 3) { // (everything the deferred encode reads has been enqueued on the first stream by now)
            if (!rx->ev_framed) HIP_TRY(hipEventCreateWithFlags(&rx->ev_framed, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(rx->ev_framed, c->stream));
        }
        rx->late.k = k;
        rx->late.base = work; rx->late.stride = stream_bytes; rx->late.frames = done; rx->late.frame_bytes = frame_bytes;
        rx->late.slot0 = rx->base_slot;
    } else {
        if ((rc = rx_deliver(rx, work, stream_bytes, done, frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
    }
    rx->base_slot += done; // the frame still being filled opens the next call's window
    rx->pending_samples = rest;
    rx->frame_open = rest > 0;
    rx->frame_count = (uint16_t)(rx->frame_count + done);
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- ragged Rx calls
// Every stream takes its own count: K0r (8-bit input) -> K1r / filter-less kernel into stream order -> K2r into each stream's
// own window -> one encoder launch over the list of every stream's completed frames.  The per-stream framing state lives in the
// r_* vectors while the streams differ, in the scalars otherwise.
static void rx_split(sdrhip_rx *rx)
{
    if (rx->diverged) return;
    const size_t S = (size_t)rx->nstreams;
    rx->r_base.assign(S, rx->base_slot);
    rx->r_pending.assign(S, rx->pending_samples);
    rx->r_open.assign(S, rx->frame_open ? 1 : 0);
    rx->r_count.assign(S, rx->frame_count);
}

static void rx_join(sdrhip_rx *rx)
{
    const size_t S = (size_t)rx->nstreams;
    for (size_t s = 1; s < S; ++s)
        if (rx->r_base[s] != rx->r_base[0] || rx->r_pending[s] != rx->r_pending[0] || rx->r_open[s] != rx->r_open[0] ||
            rx->r_count[s] != rx->r_count[0]) {
            rx->diverged = true;
            return;
        }
    rx->diverged = false;
    rx->base_slot = rx->r_base[0];
    rx->pending_samples = rx->r_pending[0];
    rx->frame_open = rx->r_open[0] != 0;
    rx->frame_count = rx->r_count[0];
}

// a HIP failure inside a ragged call: the per-stream state goes back to the scalars where the streams agree (the windows may have
// moved already), then the error
#define RX_TRY(expr)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) { rx_join(rx); return ::sdrhip::fail(SDRHIP_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } \
    } while (0)

// batch: a ragged asynchronous batch (rx_launch_ragged): int16 device rows that K0p laid out, whatever the input format
static int rx_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                     const uint32_t *tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem, bool batch)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams, L = rx->cfg.log2decim, R = rx->cfg.nb_fec;
    const size_t FB = (size_t)SDRHIP_NB_ORIGINAL + (size_t)R;
    const size_t frame_bytes = FB * SDRHIP_UDPSIZE;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    // ---- everything that can be refused is checked before anything is consumed
    if (mem != SDRHIP_MEM_HOST && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "rx_process_ragged: not available in pipelined mode");
    if (!batch)
        for (const auto &b : rx->abatch)
            if (b.state != 0) return fail(SDRHIP_EINVAL, "rx_process_ragged: asynchronous batches are being filled or in flight: collect them first");
    size_t max_in = 0;
    for (int s = 0; s < S; ++s) if (n_in[s] > max_in) max_in = n_in[s];
    if (S == 1) in_stride = max_in;
    if (S > 1 && in_stride < max_in) return fail(SDRHIP_EINVAL, "rx_process_ragged: in_stride smaller than the largest count");
    if (max_in && !iq_in) return fail(SDRHIP_EINVAL, "rx_process_ragged: NULL input");
    const bool wide8 = rx->in_fmt != IQF_S16 && !batch;
    if (max_in && mem == SDRHIP_MEM_DEVICE && (!aligned16(iq_in) || (S > 1 && (in_stride & (wide8 ? 7 : 3)))))
        return fail(SDRHIP_EALIGN, "rx_process_ragged: device input must be 16-byte aligned, its stride a multiple of %d samples", wide8 ? 8 : 4);
    rx_split(rx);
    std::vector<size_t> done((size_t)S);
    std::vector<uint64_t> rest((size_t)S);
    size_t max_done = 0, sum_done = 0, max_dec = 0;
    for (int s = 0; s < S; ++s) {
        const size_t n_dec = n_in[s] >> L;
        const uint64_t total = rx->r_pending[(size_t)s] + n_dec;
        done[(size_t)s] = (size_t)(total / SDRHIP_SAMPLES_PER_FRAME);
        rest[(size_t)s] = total - (uint64_t)done[(size_t)s] * SDRHIP_SAMPLES_PER_FRAME;
        if (done[(size_t)s] > max_done) max_done = done[(size_t)s];
        if (n_dec > max_dec) max_dec = n_dec;
        sum_done += done[(size_t)s];
    }
    if (max_done && !frames_out && mem != SDRHIP_MEM_DEVICE) { rx_join(rx); return fail(SDRHIP_EINVAL, "rx_process_ragged: NULL frames_out"); }
    if (frames_out && S > 1 && max_done && frame_stride_bytes < max_done * frame_bytes) {
        rx_join(rx);
        return fail(SDRHIP_EINVAL, "rx_process_ragged: frame stride too small for the stream with the most frames (%zu)", max_done);
    }
    RX_TRY(hipSetDevice(c->device));
    rx->consumed = false;
    if (max_in == 0) { // nothing arrives: nothing changes, nothing is delivered
        rx->view_frames = 0; rx->view_ragged = false;
        rx_join(rx);
        return SDRHIP_OK;
    }
    int rc;
    // ---- windows: stream s fills slots r_base[s] .. r_base[s] + done[s] of its area; a window that would pass the end of the area
    // moves that stream's open frame to slot 0 (the others stay where they are); a call that needs more slots than the area has
    // gets a new area, every open frame at slot 0
    size_t need_max = 0;
    for (int s = 0; s < S; ++s) if (done[(size_t)s] + 1 > need_max) need_max = done[(size_t)s] + 1;
    if (rx->old_work.p && !rx->late.have) {
        RX_TRY(hipStreamSynchronize(c->stream));
        rx->old_work.release();
    }
    if (need_max > rx->cap_frames) {
        const size_t wmul = c->opt.rx_window ? (size_t)c->opt.rx_window : 2;
        const size_t ncap = wmul * need_max;
        DevBuf bigger;
        if ((rc = bigger.reserve((size_t)S * ncap * frame_bytes))) { rx_join(rx); return rc; }
        // (the old area and every window stay as they were until the copies have completed: a failure leaves the handle untouched)
        hipError_t e = hipSuccess;
        for (int s = 0; s < S && e == hipSuccess; ++s)
            if (rx->r_open[(size_t)s])
                e = hipMemcpyAsync(bigger.as<uint8_t>() + (size_t)s * ncap * frame_bytes,
                                   rx->work.as<uint8_t>() + ((size_t)s * rx->cap_frames + rx->r_base[(size_t)s]) * frame_bytes, frame_bytes,
                                   hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // earlier launches may still use the old area
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            bigger.release();
            rx_join(rx);
            return fail(SDRHIP_EDEVICE, "rx_process_ragged: moving the open frames: %s", hipGetErrorString(e));
        }
        for (int s = 0; s < S; ++s) rx->r_base[(size_t)s] = 0;
        rx->work.release();
        rx->work = bigger;
        rx->cap_frames = ncap;
    } else {
        for (int s = 0; s < S; ++s) {
            if (rx->r_base[(size_t)s] + done[(size_t)s] + 1 <= rx->cap_frames) continue;
            uint8_t *a0 = rx->work.as<uint8_t>() + (size_t)s * rx->cap_frames * frame_bytes;
            if (rx->r_open[(size_t)s])
                RX_TRY(hipMemcpyAsync(a0, a0 + rx->r_base[(size_t)s] * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, c->stream));
            rx->r_base[(size_t)s] = 0;
        }
    }
    const size_t stream_bytes = rx->cap_frames * frame_bytes;
    uint8_t *area = rx->work.as<uint8_t>();

    // ---- the per-call table: counts (decimator), windows and meta records (K2r)
    unsigned ss = rx->cfg.sample_bits;
    const unsigned ssd = decimated_sample_size((unsigned)L, ss);
    unsigned mw[6];
    {
        uint8_t m[24];
        const uint32_t fc = rx->cfg.center_frequency_khz, sr = rx->cfg.sample_rate;
        memcpy(m + 0, &fc, 4); memcpy(m + 4, &sr, 4);
        m[8] = (uint8_t)((ssd - 1) / 8 + 1); m[9] = (uint8_t)ssd;
        m[10] = SDRHIP_NB_ORIGINAL; m[11] = (uint8_t)R;
        memset(m + 12, 0, 8);
        uint32_t crc = 0xFFFFFFFFu; // (the CRC of the record with a zero stamp: shared, the config is)
        for (int i = 0; i < 20; ++i) {
            crc ^= m[i];
            for (int k = 0; k < 8; ++k) crc = (crc & 1) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
        }
        crc ^= 0xFFFFFFFFu;
        memcpy(m + 20, &crc, 4);
        memcpy(mw, m, 24);
    }
    std::vector<RaggedRow> rows((size_t)S);
    memset(rows.data(), 0, rows.size() * sizeof(RaggedRow));
    for (int s = 0; s < S; ++s) {
        RaggedRow &r = rows[(size_t)s];
        const int first_new = rx->r_open[(size_t)s] ? 1 : 0;
        const int started = (int)(done[(size_t)s] + (rest[(size_t)s] > 0 ? 1 : 0)) - first_new;
        r.out_off = rx->r_base[(size_t)s] * frame_bytes / 4;
        r.frame_sample_base = rx->r_pending[(size_t)s];
        if (started > 0 && (n_in[s] >> L)) {
            r.meta_first = first_new; r.meta_count = started;
            r.frame_count0 = (unsigned)rx->r_count[(size_t)s] + (unsigned)first_new;
            r.meta_idx0 = first_new ? (uint64_t)SDRHIP_SAMPLES_PER_FRAME - rx->r_pending[(size_t)s] : 0;
            r.tv_sec = tv_sec[s]; r.tv_usec = tv_usec[s];
        }
    }
    const RaggedRow *rdev = nullptr;
    if ((rc = ragged_prepare(rx->dec, L, rx->cfg.fcpos, n_in, rows.data(), &rdev))) { rx_join(rx); return rc; }

    // ---- input: host rows staged stream by stream (n_in[s] samples each), 8-bit rows widened by K0r
    const int16_t *din = iq_in;
    size_t dstride = in_stride;
    if (wide8) {
        const uint8_t *d8 = reinterpret_cast<const uint8_t *>(iq_in);
        size_t sstride = in_stride;
        if (mem == SDRHIP_MEM_HOST) {
            sstride = (max_in + 7) & ~(size_t)7;
            const void *p = nullptr;
            if ((rc = ragged_stage_in(c, rx->r_pin, c->in, iq_in, in_stride, n_in, S, 2, sstride, &p))) { rx_join(rx); return rc; }
            d8 = static_cast<const uint8_t *>(p);
        }
        dstride = (max_in + 3) & ~(size_t)3;
        if ((rc = rx->wide.reserve((size_t)S * dstride * 4 + 16))) { rx_join(rx); return rc; }
        hipError_t e;
        {
            KTimer kt(c, SDRHIP_K_CONVERT);
            e = launch_iq8_widen_ragged(rx->in_fmt, d8, sstride, rx->wide.as<int16_t>(), dstride, max_in, S, rdev, c->stream);
        }
        if (e != hipSuccess) { rx_join(rx); return fail(SDRHIP_EDEVICE, "widen launch: %s", hipGetErrorString(e)); }
        din = rx->wide.as<int16_t>();
    } else if (mem == SDRHIP_MEM_HOST) {
        dstride = (max_in + 3) & ~(size_t)3;
        const void *p = nullptr;
        if ((rc = ragged_stage_in(c, rx->r_pin, c->in, iq_in, in_stride, n_in, S, 4, dstride, &p))) { rx_join(rx); return rc; }
        din = static_cast<const int16_t *>(p);
    }

    // ---- decimate: the matrix-core launch (K1mr) stores straight into each stream's window (context option rx_direct, the
    // default), its VALU pieces write the meta blocks; otherwise stream order, and K2r lays each stream's samples into its window
    const bool direct = ragged_mfma_planned(rx->dec) && c->opt.rx_direct && stream_bytes < 0x3fffffffu;
    const size_t lstride = (max_dec + 3) & ~(size_t)3;
    DevBuf &lin = rx->lin[0];
    if (direct) {
        rc = decimate_ragged_device(rx->dec, L, rx->cfg.fcpos, &ss, din, dstride, reinterpret_cast<int16_t *>(area), stream_bytes / 4,
                                    rows.data(), rdev, 1, (int)FB, mw, rx->cfg.sample_rate);
    } else {
        if ((rc = lin.reserve((size_t)S * lstride * 4 + 16))) { rx_join(rx); return rc; }
        rc = decimate_ragged_device(rx->dec, L, rx->cfg.fcpos, &ss, din, dstride, lin.as<int16_t>(), lstride, rows.data(), rdev);
    }
    if (rc) { rx_join(rx); return rc; }
    rx->consumed = true;
    if (max_dec && !direct) {
        FrameArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.in = lin.as<unsigned>(); fa.out = reinterpret_cast<unsigned *>(area);
        fa.in_stride = lstride; fa.out_stride = stream_bytes / 4;
        fa.n = max_dec; fa.frame_blocks = (int)FB;
        memcpy(fa.meta_w, mw, sizeof(fa.meta_w));
        fa.meta_rate = rx->cfg.sample_rate;
        hipError_t e = launch_frame_pack_ragged(fa, rdev, S, c->stream);
        if (e != hipSuccess) { rx_join(rx); return fail(SDRHIP_EDEVICE, "frame pack launch: %s", hipGetErrorString(e)); }
    }

    // ---- FEC: one launch over the completed frames of every stream (a dense list: frame f of stream s = area frame s * cap + slot)
    if (sum_done && R > 0) {
        const size_t nl = (sum_done + GF_FRAMES_PER_GROUP - 1) / GF_FRAMES_PER_GROUP * GF_FRAMES_PER_GROUP;
        if ((rc = rx->r_flist_pin.reserve(nl * 4))) { rx_join(rx); return rc; }
        if ((rc = rx->r_flist.reserve(nl * 4))) { rx_join(rx); return rc; }
        int32_t *fl = rx->r_flist_pin.as<int32_t>();
        size_t k = 0;
        for (int s = 0; s < S; ++s)
            for (size_t f = 0; f < done[(size_t)s]; ++f) fl[k++] = (int32_t)((size_t)s * rx->cap_frames + rx->r_base[(size_t)s] + f);
        while (k < nl) fl[k++] = -1;
        RX_TRY(hipMemcpyAsync(rx->r_flist.p, fl, nl * 4, hipMemcpyHostToDevice, c->stream));
        rx->r_flist_pin.mark(c->stream);
        if ((rc = fec_encode_device(c, area, frame_bytes, (size_t)S * rx->cap_frames, R, area + (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE,
                                    frame_bytes, rx->r_flist.as<int32_t>(), (int)(nl / GF_FRAMES_PER_GROUP))))
            { rx_join(rx); return rc; }
    }

    // ---- delivery: every stream's window (one 2-D copy when the windows line up, else a copy per stream)
    bool same_base = true;
    for (int s = 1; s < S; ++s) same_base = same_base && rx->r_base[(size_t)s] == rx->r_base[0];
    if (frames_out && max_done) {
        const hipMemcpyKind kind = mem == SDRHIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (same_base) {
            RX_TRY(link_copy2d(c, frames_out, S > 1 ? frame_stride_bytes : max_done * frame_bytes, area + rx->r_base[0] * frame_bytes, stream_bytes,
                                max_done * frame_bytes, S, kind, c->stream));
        } else {
            for (int s = 0; s < S; ++s)
                if (done[(size_t)s])
                    RX_TRY(link_copy(c, frames_out + (size_t)s * frame_stride_bytes, area + (size_t)s * stream_bytes + rx->r_base[(size_t)s] * frame_bytes,
                                      done[(size_t)s] * frame_bytes, kind, c->stream));
        }
    }
    rx->r_view_first.assign(rx->r_base.begin(), rx->r_base.end());
    rx->r_view_frames.assign(done.begin(), done.end());
    bool same_frames = true;
    for (int s = 1; s < S; ++s) same_frames = same_frames && done[(size_t)s] == done[0];
    rx->view_ragged = !(same_base && same_frames);
    if (!rx->view_ragged) { rx->view_base = area + rx->r_base[0] * frame_bytes; rx->view_stride = stream_bytes; rx->view_frames = done[0]; }
    for (int s = 0; s < S; ++s) {
        n_frames[s] = done[(size_t)s];
        rx->r_base[(size_t)s] += done[(size_t)s];
        rx->r_pending[(size_t)s] = rest[(size_t)s];
        rx->r_open[(size_t)s] = rest[(size_t)s] > 0 ? 1 : 0;
        rx->r_count[(size_t)s] = (uint16_t)(rx->r_count[(size_t)s] + done[(size_t)s]);
    }
    rx_join(rx);
    if (mem == SDRHIP_MEM_HOST) RX_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_process_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                                        const uint32_t *tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_in || !tv_sec || !tv_usec || !n_frames) return fail(SDRHIP_EINVAL, "rx_process_ragged: NULL count, stamp or n_frames array");
    sdrhip::CtxLock lock_(rx->ctx);
    return rx_ragged(rx, iq_in, n_in, in_stride, tv_sec, tv_usec, frames_out, frame_stride_bytes, n_frames, mem);
}

// --------------------------------------------------------------------------- asynchronous host-pointer Rx entry
// sdrdaemonrx's chain is asynchronous end to end (source thread -> source_buffer -> main loop -> output_buffer -> writer ->
// transmit thread, sdrdaemonrx.cpp:555-663): a block's frames leave the process long after Downsampler::process returned.
// sdrhip_rx_process on host pointers is one synchronous launch per block (38 us for a 65 536-sample TestSource block, of which
// the GPU works ~10); submit / collect give the host-pointer path the same asynchrony: blocks are appended to a pinned
// staging buffer (or taken in place from sdrhip_host_alloc memory), every `blocks` of them go out as ONE upload + launch +
// download on the context's stream, and the frames are collected later, batch by batch, in order.
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
namespace {
int rx_launch_batch(sdrhip_rx *rx, sdrhip_rx::Batch &b)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    // (8-bit input: the batch goes up as bytes, rows of a multiple of 8 samples; sdrhip_rx_process widens it on the device)
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2;
    const size_t dstride = esz == 4 ? (b.n_in + 3) & ~(size_t)3 : (b.n_in + 7) & ~(size_t)7;
    int rc;
    if ((rc = b.din.reserve((size_t)S * dstride * esz + 16))) return rc;
    // uploads: runs of blocks that are adjacent in host memory go out as ONE 2-D copy (a run of staged blocks -- stream-major in
    // the pinned arena -- or of in-place blocks cut from one buffer)
    size_t off = 0;
    for (size_t i = 0; i < b.blocks.size();) {
        const char *src = reinterpret_cast<const char *>(b.blocks[i].first);
        size_t sstride = b.strides[i], n = b.blocks[i].second, j = i + 1;
        if (!src) { // staged: [stream][in_cap] at sample offset `off` of every row (all staged blocks of a batch are one run)
            src = b.in.as<char>() + off * esz;
            sstride = b.in_cap;
            while (j < b.blocks.size() && !b.blocks[j].first) n += b.blocks[j++].second;
        } else {
            while (j < b.blocks.size() && reinterpret_cast<const char *>(b.blocks[j].first) == src + n * esz && b.strides[j] == sstride) n += b.blocks[j++].second;
        }
        if (S == 1) HIP_TRY(link_copy(c, b.din.as<char>() + off * esz, src, n * esz, hipMemcpyHostToDevice, c->stream)); // (no pitch limits)
        else HIP_TRY(link_copy2d(c, b.din.as<char>() + off * esz, dstride * esz, src, sstride * esz, n * esz, S, hipMemcpyHostToDevice, c->stream));
        off += n;
        i = j;
    }
    b.in.mark(c->stream);
    // everything that can fail for want of memory happens BEFORE the samples are consumed: a batch that failed here, or that
    // sdrhip_rx_process refused before its decimator launch went out, is launched again by the next submit / collect; one that fails
    // behind the decimator launch (rx->consumed) is dropped: its samples are in the filter state already, replaying them would
    // duplicate samples and shift every later stamp
    b.frame_bytes = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
    const size_t nf_max = sdrhip_rx_max_frames(rx, b.n_in);
    if (nf_max && (rc = b.out.reserve((size_t)S * nf_max * b.frame_bytes))) return rc;
    if (!b.done && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) { b.done = nullptr; return fail(SDRHIP_EDEVICE, "hipEventCreate"); }
    size_t nf = 0;
    rc = sdrhip_rx_process(rx, b.din.as<int16_t>(), b.n_in, dstride, b.tv_sec, b.tv_usec, nullptr, 0, &nf, SDRHIP_MEM_DEVICE);
    if (rc) {
        if (rx->consumed) b.state = 0; // consumed and lost: never replayed (the pipe's own error stands)
        return rc;
    }
    b.frames = nf;
    hipError_t e = hipSuccess;
    if (nf > nf_max) e = hipErrorInvalidValue; // (cannot happen: rx_max_frames is the pipe's own bound)
    else if (nf && S == 1) e = link_copy(c, b.out.p, rx->view_base, nf * b.frame_bytes, hipMemcpyDeviceToHost, c->stream);
    else if (nf) e = link_copy2d(c, b.out.p, nf * b.frame_bytes, rx->view_base, rx->view_stride, nf * b.frame_bytes, S, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) {
        b.state = 0; // consumed and lost: never replayed
        return fail(SDRHIP_EDEVICE, "rx batch download: %s (the batch's %zu frames per stream are lost)", hipGetErrorString(e), nf);
    }
    b.state = 2;
    return SDRHIP_OK;
}

// a ragged batch: ONE upload per run of adjacent packed memory -> K0p lays the rows out (and widens 8-bit input) -> per stream one
// sdrhip_rx_process_ragged step of the batch's summed counts with its first block's stamps -> the frames every stream delivered,
// compacted in stream order -> ONE download of exactly those frames.  Failure rules of rx_launch_batch: everything that can fail
// for want of memory happens before the decimator launch (the batch is launched again later); a failure behind it (rx->consumed)
// drops the batch.
int rx_launch_ragged(sdrhip_rx *rx, sdrhip_rx::Batch &b)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams, L = rx->cfg.log2decim;
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2;
    const size_t nblk = b.r_cnt.size() / (size_t)S;
    size_t max_t = 0, nseg = 0, packed = 0, sum_done = 0;
    for (size_t i = 0; i < b.r_cnt.size(); ++i) { packed += b.r_cnt[i]; nseg += b.r_cnt[i] ? 1 : 0; }
    for (int s = 0; s < S; ++s) if (b.r_tot[(size_t)s] > max_t) max_t = b.r_tot[(size_t)s];
    const size_t dstride = (max_t + 7) & ~(size_t)7;
    const size_t fb = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
    // (the frames every stream completes, counted as rx_ragged counts them: the buffers are sized before anything is consumed)
    for (int s = 0; s < S; ++s) {
        const uint64_t pend = rx->diverged ? rx->r_pending[(size_t)s] : rx->pending_samples;
        sum_done += (size_t)((pend + (b.r_tot[(size_t)s] >> L)) / SDRHIP_SAMPLES_PER_FRAME);
    }
    const size_t rows_bytes = (size_t)(S + 1) * sizeof(PackRow), segs_bytes = nseg * sizeof(PackSeg);
    const size_t list_off = (rows_bytes + segs_bytes + 15) & ~(size_t)15;
    int rc;
    if ((rc = b.r_tab.reserve(list_off + sum_done * 4 + 16))) return rc; // (waits for the table upload of this batch's last use)
    if (list_off + sum_done * 4 + 16 > rx->a_tab.cap || packed * esz + 64 > rx->a_pk.cap || (size_t)S * dstride * 4 + 16 > rx->a_din.cap ||
        sum_done * fb > rx->a_frames.cap)
        HIP_TRY(hipStreamSynchronize(c->stream)); // (a device buffer grows: batches in flight may still use the old one)
    if ((rc = rx->a_tab.reserve(list_off + sum_done * 4 + 16))) return rc;
    if ((rc = rx->a_pk.reserve(packed * esz + 64))) return rc;
    if ((rc = rx->a_din.reserve((size_t)S * dstride * 4 + 16))) return rc;
    if (sum_done && (rc = b.out.reserve(sum_done * fb))) return rc;
    if (sum_done && (rc = rx->a_frames.reserve(sum_done * fb))) return rc;
    if (!b.done && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) { b.done = nullptr; return fail(SDRHIP_EDEVICE, "hipEventCreate"); }

    // ---- K0p's table: segments stream by stream (block order inside), sources at their packed offsets (block-major, stream-minor)
    PackRow *rows = b.r_tab.as<PackRow>();
    PackSeg *segs = reinterpret_cast<PackSeg *>(b.r_tab.as<char>() + rows_bytes);
    std::vector<uint64_t> src(b.r_cnt.size());
    {
        uint64_t acc = 0;
        for (size_t i = 0; i < b.r_cnt.size(); ++i) { src[i] = acc; acc += b.r_cnt[i]; }
    }
    uint32_t k = 0;
    uint64_t wg = 0;
    for (int s = 0; s < S; ++s) {
        PackRow &r = rows[s];
        r.seg0 = k; r.wg0 = (uint32_t)wg; r.total = (uint32_t)b.r_tot[(size_t)s];
        uint32_t dst = 0;
        for (size_t blk = 0; blk < nblk; ++blk) {
            const size_t i = blk * (size_t)S + (size_t)s, n = b.r_cnt[i];
            if (!n) continue;
            segs[k].src = src[i]; segs[k].dst = dst; segs[k].n = (uint32_t)n;
            dst += (uint32_t)n;
            ++k;
        }
        r.nseg = k - r.seg0;
        wg += (b.r_tot[(size_t)s] + UNPACK_WG_SAMPLES - 1) / UNPACK_WG_SAMPLES;
    }
    rows[S].seg0 = k; rows[S].nseg = 0; rows[S].wg0 = (uint32_t)wg; rows[S].total = 0;
    if (wg > 0x7fffffffu) return fail(SDRHIP_EINVAL, "rx batch: too many samples for one launch");

    // ---- uploads: the packed samples, one copy per run of adjacent memory (staged runs are adjacent in the arena), then the table
    uint8_t *pk = rx->a_pk.as<uint8_t>();
    size_t off = 0;
    for (size_t i = 0; i < b.r_runs.size();) {
        const char *p0 = b.r_runs[i].p ? b.r_runs[i].p : b.in.as<char>() + b.r_runs[i].off;
        size_t n = b.r_runs[i].bytes, j = i + 1;
        for (; j < b.r_runs.size(); ++j) {
            const char *pj = b.r_runs[j].p ? b.r_runs[j].p : b.in.as<char>() + b.r_runs[j].off;
            if ((b.r_runs[j].p == nullptr) != (b.r_runs[i].p == nullptr) || pj != p0 + n) break;
            n += b.r_runs[j].bytes;
        }
        HIP_TRY(link_copy(c, pk + off, p0, n, hipMemcpyHostToDevice, c->stream));
        off += n;
        i = j;
    }
    b.in.mark(c->stream);
    HIP_TRY(hipMemcpyAsync(rx->a_tab.p, b.r_tab.p, rows_bytes + segs_bytes, hipMemcpyHostToDevice, c->stream)); // (not counted: a table)
    b.r_tab.mark(c->stream);
    const PackRow *rows_dev = rx->a_tab.as<PackRow>();
    const PackSeg *segs_dev = reinterpret_cast<const PackSeg *>(rx->a_tab.as<char>() + rows_bytes);
    {
        KTimer kt(c, SDRHIP_K_CONVERT);
        const hipError_t e = launch_unpack_packed(rx->in_fmt, pk, rx->a_din.as<int16_t>(), dstride, rows_dev, segs_dev, S, (unsigned)wg, c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "unpack launch: %s", hipGetErrorString(e));
    }

    // ---- the batch as one ragged step
    std::vector<size_t> nf((size_t)S, 0);
    rc = rx_ragged(rx, rx->a_din.as<int16_t>(), b.r_tot.data(), dstride, b.r_sec.data(), b.r_usec.data(), nullptr, 0, nf.data(),
                   SDRHIP_MEM_DEVICE, true);
    if (rc) {
        if (rx->consumed) b.state = 0; // consumed and lost: never replayed (the pipe's own error stands)
        return rc;
    }

    // ---- download: the delivered frames of every stream, compacted in stream order, in ONE copy
    int32_t *list = reinterpret_cast<int32_t *>(b.r_tab.as<char>() + list_off);
    size_t nl = 0;
    hipError_t e = hipSuccess;
    for (int s = 0; s < S && e == hipSuccess; ++s) {
        if (nl + nf[(size_t)s] > sum_done) { e = hipErrorInvalidValue; break; } // (cannot happen: the count above is the pipe's own)
        for (size_t f = 0; f < nf[(size_t)s]; ++f) list[nl++] = (int32_t)((size_t)s * rx->cap_frames + rx->r_view_first[(size_t)s] + f);
    }
    if (e == hipSuccess && nl) e = hipMemcpyAsync(rx->a_tab.as<char>() + list_off, list, nl * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nl) {
        b.r_tab.mark(c->stream);
        e = launch_frame_gather(rx->work.as<uint8_t>(), fb, reinterpret_cast<const int32_t *>(rx->a_tab.as<char>() + list_off), nl,
                                rx->a_frames.as<uint8_t>(), c->stream);
    }
    if (e == hipSuccess && nl) e = link_copy(c, b.out.p, rx->a_frames.p, nl * fb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) {
        b.state = 0; // consumed and lost: never replayed
        return fail(SDRHIP_EDEVICE, "rx ragged batch download: %s (the batch's %zu frames are lost)", hipGetErrorString(e), nl);
    }
    b.r_frames.assign(nf.begin(), nf.end());
    b.frame_bytes = fb;
    b.state = 2;
    return SDRHIP_OK;
}
} // namespace

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

extern "C" int sdrhip_rx_set_async(sdrhip_rx *rx, int depth, int blocks)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (depth < 1 || depth > 64 || blocks < 1 || blocks > 1024) return fail(SDRHIP_EINVAL, "rx_set_async: depth 1..64, blocks 1..1024");
    for (auto &b : rx->abatch)
        if (b.state != 0) return fail(SDRHIP_EINVAL, "rx_set_async: batches are in flight: collect them first");
    for (auto &b : rx->abatch) { if (b.done) (void)hipEventDestroy(b.done); b.in.release(); b.din.release(); b.out.release(); b.r_tab.release(); }
    rx->abatch.assign((size_t)depth, sdrhip_rx::Batch());
    rx->a_blocks = blocks; rx->a_head = rx->a_tail = 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_submit(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec, uint32_t tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (n_in == 0) return SDRHIP_OK;
    if (!iq_in) return fail(SDRHIP_EINVAL, "rx_submit: NULL input");
    if (rx->diverged) return fail(SDRHIP_EINVAL, "rx_submit: ragged calls left the streams at different frame positions");
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_submit: ragged batches are being filled or in flight: collect them first");
    if (rx->abatch.empty()) { rx->abatch.assign(4, sdrhip_rx::Batch()); rx->a_blocks = 1; }
    HIP_TRY(hipSetDevice(rx->ctx->device));
    const int S = rx->nstreams;
    if (S == 1) in_stride = n_in;
    sdrhip_rx::Batch &b = rx->abatch[rx->a_tail % rx->abatch.size()];
    if (b.state == 2) return fail(SDRHIP_EBUSY, "rx_submit: every batch of the ring is in flight: sdrhip_rx_collect first");
    if (b.state == 0) {
        b.blocks.clear(); b.strides.clear(); b.n_in = 0; b.tv_sec = tv_sec; b.tv_usec = tv_usec; b.state = 1; b.ragged = false;
        b.in_cap = 0; // no staged rows yet: the first pageable block of this batch (re)claims the arena
    }
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2; // bytes per sample (sdrhip_rx_set_input_format)
    const char *src = reinterpret_cast<const char *>(iq_in);
    if (host_is_pinned(iq_in, ((size_t)(S - 1) * in_stride + n_in) * esz)) {
        b.blocks.push_back(std::make_pair(iq_in, n_in)); // in place: the caller keeps it untouched until the batch is collected
        b.strides.push_back(in_stride);
    } else {
        // staged: row s of the pinned arena holds stream s, the block at the batch's current sample offset
        // (in-place blocks in front of it leave their part of the rows unused: a block always sits at its batch offset)
        const size_t need = b.n_in + n_in;
        if (b.in_cap == 0) { // first staged block of the batch, whatever came before it in place
            const size_t cap = (size_t)rx->a_blocks * n_in > need ? (size_t)rx->a_blocks * n_in : need;
            int rc = b.in.reserve((size_t)S * cap * esz); // (waits for the upload of the batch that used this buffer last)
            if (rc) return rc;
            b.in_cap = cap;
        } else if (need > b.in_cap) { // blocks longer than the first one: re-lay the rows out in a bigger arena
            PinnedBuf bigger;
            const size_t ncap = 2 * need;
            int rc = bigger.reserve((size_t)S * ncap * esz);
            if (rc) return rc;
            for (int s = 0; s < S; ++s) memcpy(bigger.as<char>() + (size_t)s * ncap * esz, b.in.as<char>() + (size_t)s * b.in_cap * esz, b.n_in * esz);
            b.in.release();
            b.in = bigger;
            b.in_cap = ncap;
        }
        for (int s = 0; s < S; ++s) memcpy(b.in.as<char>() + ((size_t)s * b.in_cap + b.n_in) * esz, src + (size_t)s * in_stride * esz, n_in * esz);
        b.blocks.push_back(std::make_pair((const int16_t *)nullptr, n_in));
        b.strides.push_back(n_in);
    }
    b.n_in += n_in;
    if ((int)b.blocks.size() >= rx->a_blocks) {
        int rc = rx_launch_batch(rx, b);
        if (rc) return rc;
        ++rx->a_tail;
    }
    return SDRHIP_OK;
}

// the oldest batch of the ring once it has finished (wait = 1: launches it when it is still being filled, then waits OUTSIDE the
// context lock: the submitting thread -- the reference's source / main thread -- keeps feeding the ring while the collecting thread
// -- its transmit thread -- sleeps on the oldest batch's event)
static int rx_wait_oldest(sdrhip_rx *rx, std::unique_lock<std::recursive_mutex> &lock_, int wait, const char *who, sdrhip_rx::Batch **bp)
{
    for (;;) {
        sdrhip_rx::Batch &h = rx->abatch[rx->a_head % rx->abatch.size()];
        if (h.state == 0) return fail(SDRHIP_EBUSY, "%s: nothing was submitted", who); // (SDRHIP_OK always means: one batch collected, *n_frames of it -- possibly 0)
        if (h.state == 1) {
            if (!wait) return fail(SDRHIP_EBUSY, "%s: the oldest batch is still being filled (wait = 1 launches it as it is)", who);
            int rc = h.ragged ? rx_launch_ragged(rx, h) : rx_launch_batch(rx, h); // a partly filled batch goes out as it is (end of stream)
            if (rc) return rc;
            ++rx->a_tail;
        }
        const hipError_t q = hipEventQuery(h.done);
        if (q == hipSuccess) { *bp = &h; break; }
        if (q != hipErrorNotReady) return fail(SDRHIP_EDEVICE, "hipEventQuery: %s", hipGetErrorString(q));
        if (!wait) return fail(SDRHIP_EBUSY, "%s: the oldest batch is still in flight", who);
        const size_t head = rx->a_head;
        hipEvent_t ev = h.done;
        lock_.unlock();
        const hipError_t w = hipEventSynchronize(ev);
        lock_.lock();
        if (w != hipSuccess) return fail(SDRHIP_EDEVICE, "hipEventSynchronize: %s", hipGetErrorString(w));
        if (rx->a_head == head) { *bp = &rx->abatch[head % rx->abatch.size()]; break; }
        // (another thread collected that batch meanwhile: look at the new head)
    }
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_collect(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames, int wait)
{
    if (!rx || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    *n_frames = 0;
    if (rx->abatch.empty()) return fail(SDRHIP_EBUSY, "rx_collect: nothing was submitted");
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_collect: ragged batches are being filled or in flight: use sdrhip_rx_collect_ragged");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    int rc = rx_wait_oldest(rx, lock_, wait, "rx_collect", &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    const int S = rx->nstreams;
    if (b.frames > max_frames) { // (the batch stays where it is: call again with room for *n_frames frames per stream)
        *n_frames = b.frames;
        return fail(SDRHIP_EINVAL, "rx_collect: the batch holds %zu frames per stream, frames_out has room for %zu", b.frames, max_frames);
    }
    if (b.frames) {
        if (!frames_out) return fail(SDRHIP_EINVAL, "rx_collect: NULL frames_out");
        const size_t row = b.frames * b.frame_bytes;
        if (S > 1 && frame_stride_bytes < row) return fail(SDRHIP_EINVAL, "rx_collect: frame stride too small");
        for (int s = 0; s < S; ++s) memcpy(frames_out + (size_t)s * (S > 1 ? frame_stride_bytes : row), b.out.as<char>() + (size_t)s * row, row);
    }
    *n_frames = b.frames;
    b.state = 0;
    ++rx->a_head;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_submit_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                                       const uint32_t *tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_in || !tv_sec || !tv_usec) return fail(SDRHIP_EINVAL, "rx_submit_ragged: NULL count or stamp array");
    sdrhip::CtxLock lock_(rx->ctx);
    // ---- everything that can be refused is checked before anything is consumed
    const int S = rx->nstreams;
    size_t max_in = 0, sum = 0;
    for (int s = 0; s < S; ++s) { sum += n_in[s]; if (n_in[s] > max_in) max_in = n_in[s]; }
    if (in_stride != SDRHIP_PACKED && in_stride < max_in)
        return fail(SDRHIP_EINVAL, "rx_submit_ragged: in_stride is neither SDRHIP_PACKED nor at least the largest count");
    if (sum && !iq_in) return fail(SDRHIP_EINVAL, "rx_submit_ragged: NULL input");
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "rx_submit_ragged: not available in pipelined mode");
    if (rx_has_batches(rx, false)) return fail(SDRHIP_EINVAL, "rx_submit_ragged: uniform batches are being filled or in flight: collect them first");
    if (rx->abatch.empty()) { rx->abatch.assign(4, sdrhip_rx::Batch()); rx->a_blocks = 1; }
    sdrhip_rx::Batch &b = rx->abatch[rx->a_tail % rx->abatch.size()];
    if (b.state == 2) return fail(SDRHIP_EBUSY, "rx_submit_ragged: every batch of the ring is in flight: sdrhip_rx_collect_ragged first");
    for (int s = 0; s < S; ++s) // (K0p's table holds 32-bit row positions)
        if ((b.state == 1 ? b.r_tot[(size_t)s] : 0) + n_in[s] > (size_t)0xffffffffu - UNPACK_WG_SAMPLES)
            return fail(SDRHIP_EINVAL, "rx_submit_ragged: a stream's batch would exceed 2^32 - 4096 samples");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2; // bytes per sample (sdrhip_rx_set_input_format)
    const char *src = reinterpret_cast<const char *>(iq_in);
    const bool inplace = in_stride == SDRHIP_PACKED && sum && host_is_pinned(iq_in, sum * esz);
    if (sum && !inplace) { // (the arena: the staged blocks of the batch back to back, packed)
        const size_t used = b.state == 1 ? b.r_used : 0, need = used + sum * esz;
        if (used == 0) {
            const size_t cap = (size_t)rx->a_blocks * sum * esz > need ? (size_t)rx->a_blocks * sum * esz : need;
            int rc = b.in.reserve(cap); // (waits for the upload of the batch that used this buffer last)
            if (rc) return rc;
        } else if (need > b.in.cap) {
            PinnedBuf bigger;
            int rc = bigger.reserve(2 * need);
            if (rc) return rc;
            memcpy(bigger.p, b.in.p, used);
            b.in.release();
            b.in = bigger;
        }
    }
    if (b.state == 0) { // the batch's first block: its stamps are the batch's
        b.ragged = true; b.state = 1;
        b.r_runs.clear(); b.r_cnt.clear(); b.r_used = 0;
        b.r_tot.assign((size_t)S, 0);
        b.r_sec.assign(tv_sec, tv_sec + S); b.r_usec.assign(tv_usec, tv_usec + S);
    }
    if (inplace) { // in place: the caller keeps it untouched until the batch is collected
        b.r_runs.push_back(sdrhip_rx::Batch::Run{src, 0, sum * esz});
    } else if (sum) { // staged packed: one memcpy per non-empty row, never the padding of a strided row
        char *dst = b.in.as<char>() + b.r_used;
        size_t soff = 0;
        for (int s = 0; s < S; ++s) {
            const size_t n = n_in[s];
            const char *row = in_stride == SDRHIP_PACKED ? src + soff : src + (size_t)s * in_stride * esz;
            if (n) memcpy(dst, row, n * esz);
            dst += n * esz;
            soff += n * esz;
        }
        b.r_runs.push_back(sdrhip_rx::Batch::Run{nullptr, b.r_used, sum * esz});
        b.r_used += sum * esz;
    }
    b.r_cnt.insert(b.r_cnt.end(), n_in, n_in + S);
    for (int s = 0; s < S; ++s) b.r_tot[(size_t)s] += n_in[s];
    if ((int)(b.r_cnt.size() / (size_t)S) >= rx->a_blocks) {
        int rc = rx_launch_ragged(rx, b);
        if (rc) return rc;
        ++rx->a_tail;
    }
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_collect_ragged(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames,
                                        int wait)
{
    if (!rx || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect_ragged: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    const int S = rx->nstreams;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    if (rx->abatch.empty()) return fail(SDRHIP_EBUSY, "rx_collect_ragged: nothing was submitted");
    if (rx_has_batches(rx, false)) return fail(SDRHIP_EINVAL, "rx_collect_ragged: uniform batches are being filled or in flight: use sdrhip_rx_collect");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    int rc = rx_wait_oldest(rx, lock_, wait, "rx_collect_ragged", &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    size_t most = 0;
    for (int s = 0; s < S; ++s) if (b.r_frames[(size_t)s] > most) most = b.r_frames[(size_t)s];
    if (most > max_frames) { // (the batch stays where it is: call again with room for the largest n_frames[s])
        for (int s = 0; s < S; ++s) n_frames[s] = b.r_frames[(size_t)s];
        return fail(SDRHIP_EINVAL, "rx_collect_ragged: a stream of the batch holds %zu frames, frames_out has room for %zu", most, max_frames);
    }
    if (most) {
        if (!frames_out) return fail(SDRHIP_EINVAL, "rx_collect_ragged: NULL frames_out");
        if (S > 1 && frame_stride_bytes < most * b.frame_bytes) return fail(SDRHIP_EINVAL, "rx_collect_ragged: frame stride too small");
        size_t off = 0;
        for (int s = 0; s < S; ++s) {
            const size_t row = b.r_frames[(size_t)s] * b.frame_bytes;
            if (row) memcpy(frames_out + (size_t)s * frame_stride_bytes, b.out.as<char>() + off, row);
            off += row;
        }
    }
    for (int s = 0; s < S; ++s) n_frames[s] = b.r_frames[(size_t)s];
    b.state = 0;
    ++rx->a_head;
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- fused Tx pipe
struct sdrhip_tx {
    sdrhip_ctx *ctx;
    int nstreams;
    int log2interp;
    sdrhip_interpolators *itp;
    DevBuf rxbuf, payload[2], outbuf;
    DevBuf srcmap, restored;  // no-copy mode (tx_gather): the decoder's position map and restored blocks, read by K5w's gather variant
    size_t restored_slots = 0; // slots `restored` was zero-terminated for (its last slot must read zero)
    // ---- pipelined mode (sdrhip_tx_set_pipelined): a call decodes ITS batch into payload[psel] -- on the context's second stream,
    // with work buffers of its own -- while the first stream interpolates the batch the PREVIOUS call decoded (payload[psel ^ 1]);
    // the samples are delivered one call late, like SDRdaemonFECBuffer delivers a frame when the next one begins (.cpp:133-139)
    int pipelined = 0;
    int psel = 0;
    struct Late {
        bool have = false;
        size_t n_payload = 0, pstride = 0;
        int log2interp = 0; // the factor in force when the batch was handed in
    } late;
    DevBuf plan_own, idx_own;
    PinnedBuf pin_own;
    hipEvent_t ev_in = nullptr;              // first stream: the caller's device rx buffer is ready
    hipEvent_t ev_up = nullptr;              // second stream: the upload of the caller's HOST rx buffer has read it (the call returns behind it)
    hipEvent_t ev_dec = nullptr;             // second stream: the waiting batch is decoded
    hipEvent_t ev_itp[2] = {nullptr, nullptr}; // first stream: the interpolator has read payload[i]
    bool itp_pending[2] = {false, false};
    // ---- asynchronous host-pointer entry (sdrhip_tx_submit / sdrhip_tx_collect): a ring of batches of received frames
    struct ABatch {
        PinnedBuf in;             // the batch's received super blocks [stream][frame][128][512] (staged; sdrhip_host_alloc memory is used in place)
        DevBuf din, dout, db0;    // ... on the device; its samples [stream][dos]; its meta blocks [stream * nframes][508]
        PinnedBuf out;            // samples, then meta blocks, downloaded
        hipEvent_t done = nullptr;
        size_t nframes = 0, n_res = 0, dos = 0;
        int state = 0;            // 0 free, 2 in flight
        // a batch of raw datagrams (sdrhip_tx_submit_datagrams): `in` holds them packed, `out` the gathered delivery (every
        // stream's samples, then the records, then the meta blocks); tab / seg = its collector tables and gather segments
        bool dg = false;
        PinnedBuf tab, seg;
        std::vector<size_t> frames; // released frames per stream
        int log2interp = 0;
        size_t esz = 4;
    };
    std::vector<ABatch> abatch;
    size_t a_head = 0, a_tail = 0;
    // device buffers of the datagram batches, shared by the ring (the context's stream orders the batches): the packed datagrams,
    // the collector's [stream][pitch] rows, the interpolator's output rows, the meta blocks, the gathered delivery, its segments
    DevBuf a_pk, a_pay, a_out, a_b0, a_gat, a_seg;
    // ---- datagram entry (sdrhip_tx_process_datagrams): one SDRdaemonFECBuffer per stream, created on first use; the frames it
    // releases go to payload[0] (or straight to the caller's device iq_out when log2interp = 0), the interpolator reads them there
    sdrhip_fecbuf *fb = nullptr;
    // ---- output format (sdrhip_tx_set_output_format): IQF_S8 = 2-byte samples from the interpolator's last stage (or K6n for x1)
    int out_fmt = IQF_S16;
};

namespace {
// bytes per output sample, and the row pitch (samples) of the library's own output buffers: 16-byte rows either way
inline size_t tx_esz(const sdrhip_tx *tx) { return tx->out_fmt == IQF_S8 ? 2 : 4; }
inline size_t tx_pitch(const sdrhip_tx *tx, size_t n) { return tx->out_fmt == IQF_S8 ? (n + 7) & ~(size_t)7 : (n + 3) & ~(size_t)3; }
// a device output the interpolator may store to with 16-byte stores: aligned, the stride a multiple of 4 (int16) / 8 (8-bit) samples
inline bool tx_out_aligned(const sdrhip_tx *tx, const void *p, size_t stride) { return aligned16(p) && (tx->nstreams == 1 || (stride & (tx->out_fmt == IQF_S8 ? 7 : 3)) == 0); }
// asynchronous batches of one kind in flight: raw datagrams (dg) or received frames
bool tx_in_flight(const sdrhip_tx *tx, bool dg)
{
    for (const auto &b : tx->abatch)
        if (b.state != 0 && b.dg == dg) return true;
    return false;
}
} // namespace

extern "C" int sdrhip_tx_create(sdrhip_ctx *ctx, int nstreams, int log2interp, sdrhip_tx **out)
{
    if (!ctx || !out || nstreams <= 0) return fail(SDRHIP_EINVAL, "tx_create: bad argument");
    if (log2interp < 0 || log2interp > 6) return fail(SDRHIP_EINVAL, "Invalid log2 interpolation factor");
    sdrhip_tx *tx = new (std::nothrow) sdrhip_tx();
    if (!tx) return fail(SDRHIP_ENOMEM, "out of host memory");
    tx->ctx = ctx; tx->nstreams = nstreams; tx->log2interp = log2interp; tx->itp = nullptr;
    int rc = sdrhip_interpolators_create(ctx, nstreams, &tx->itp);
    if (rc) { delete tx; return rc; }
    *out = tx;
    return SDRHIP_OK;
}

// Upsampler::configure (Upsampler.cpp:31-50), applied between two batches like sdrdaemontx does with a control message
// (sdrdaemontx.cpp:381): the six interpolator instances are shared by every interpolateN entry point
// (Interpolators.h:47-52), so their histories carry over.  (Pipelined mode: a batch that waits for delivery keeps the factor
// it was handed in with.)
extern "C" int sdrhip_tx_reconfigure(sdrhip_tx *tx, int log2interp)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (log2interp < 0 || log2interp > 6) return fail(SDRHIP_EINVAL, "Invalid log2 interpolation factor"); // Upsampler.cpp:38-42
    tx->log2interp = log2interp;
    return SDRHIP_OK;
}

extern "C" void sdrhip_tx_destroy(sdrhip_tx *tx)
{
    if (!tx) return;
    (void)hipSetDevice(tx->ctx->device);
    if (tx->ctx->stream2) (void)hipStreamSynchronize(tx->ctx->stream2); // (a decode of the pipelined mode may still run there)
    sdrhip_interpolators_destroy(tx->itp); // (synchronises the first stream)
    sdrhip_fecbuf_destroy(tx->fb);
    tx->rxbuf.release(); tx->payload[0].release(); tx->payload[1].release(); tx->outbuf.release();
    tx->srcmap.release(); tx->restored.release();
    tx->plan_own.release(); tx->idx_own.release(); tx->pin_own.release();
    for (auto &b : tx->abatch) {
        if (b.done) { (void)hipEventSynchronize(b.done); (void)hipEventDestroy(b.done); }
        b.in.release(); b.din.release(); b.dout.release(); b.db0.release(); b.out.release(); b.tab.release(); b.seg.release();
    }
    tx->a_pk.release(); tx->a_pay.release(); tx->a_out.release(); tx->a_b0.release(); tx->a_gat.release(); tx->a_seg.release();
    if (tx->ev_in) (void)hipEventDestroy(tx->ev_in);
    if (tx->ev_up) (void)hipEventDestroy(tx->ev_up);
    if (tx->ev_dec) (void)hipEventDestroy(tx->ev_dec);
    for (int i = 0; i < 2; ++i) if (tx->ev_itp[i]) (void)hipEventDestroy(tx->ev_itp[i]);
    delete tx;
}

extern "C" int sdrhip_tx_set_pipelined(sdrhip_tx *tx, int on)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (!on && tx->late.have) return fail(SDRHIP_EINVAL, "tx_set_pipelined: sdrhip_tx_flush the waiting batch first");
    if (on && tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_set_pipelined: asynchronous datagram batches are in flight: collect them first");
    if (on) {
        HIP_TRY(hipSetDevice(tx->ctx->device));
        if (!tx->ev_in) HIP_TRY(hipEventCreateWithFlags(&tx->ev_in, hipEventDisableTiming));
        if (!tx->ev_up) HIP_TRY(hipEventCreateWithFlags(&tx->ev_up, hipEventDisableTiming));
        if (!tx->ev_dec) HIP_TRY(hipEventCreateWithFlags(&tx->ev_dec, hipEventDisableTiming));
        for (int i = 0; i < 2; ++i) if (!tx->ev_itp[i]) HIP_TRY(hipEventCreateWithFlags(&tx->ev_itp[i], hipEventDisableTiming));
    }
    tx->pipelined = on ? 1 : 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_set_output_format(sdrhip_tx *tx, int fmt)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (fmt == SDRHIP_IQ_U8) return fail(SDRHIP_EINVAL, "tx_set_output_format: SDRHIP_IQ_U8 is an input format (RTL-SDR); the Tx side gives S16 or S8");
    if (fmt != SDRHIP_IQ_S16 && fmt != SDRHIP_IQ_S8) return fail(SDRHIP_EINVAL, "tx_set_output_format: unknown format %d", fmt);
    for (const auto &b : tx->abatch)
        if (b.state != 0) return fail(SDRHIP_EINVAL, "tx_set_output_format: asynchronous batches are in flight: collect them first");
    if (tx->late.have) return fail(SDRHIP_EINVAL, "tx_set_output_format: a pipelined batch waits: sdrhip_tx_flush it first");
    tx->out_fmt = fmt;
    return SDRHIP_OK;
}

namespace {
// decode S x nframes frames into `pay` ([S][pstride] samples): one batch, or one call per stream when the rows are padded
int tx_decode(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, DevBuf &pay, size_t pstride, const DecodeSide *side,
              uint8_t *block0 = nullptr) // block0 (optional, device): [stream * nframes][508], the frames' meta blocks
{
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams;
    const size_t fb = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, n_payload = nframes * SDRHIP_SAMPLES_PER_FRAME;
    int rc;
    if (pstride == n_payload)
        return fec_decode_device(c, drx, fb, indices, (size_t)S * nframes, pay.as<uint8_t>(), (size_t)127 * SDRHIP_BLOCK_BYTES, block0, side);
    for (int s = 0; s < S; ++s)
        if ((rc = fec_decode_device(c, drx + (size_t)s * nframes * fb, fb, indices ? indices + (size_t)s * nframes * SDRHIP_NB_ORIGINAL : nullptr, nframes,
                                    pay.as<uint8_t>() + (size_t)s * pstride * 4, (size_t)127 * SDRHIP_BLOCK_BYTES,
                                    block0 ? block0 + (size_t)s * nframes * SDRHIP_BLOCK_BYTES : nullptr, side)))
            return rc;
    return SDRHIP_OK;
}

// no-copy mode of a batch (round 6): the decoder leaves the received originals in drx and writes only the restored blocks + a map;
// the wave interpolator gathers through the map.  Applies to immediate calls and the asynchronous entry (the received frames must
// outlive the interpolator: a pipelined call interpolates one call LATE, when a device caller may have reused its buffer).
bool tx_gather_applies(const sdrhip_tx *tx, int log2interp)
{
    const sdrhip_ctx *c = tx->ctx;
    return c->opt.tx_gather && !tx->pipelined && tx->out_fmt == IQF_S16 && interpolate_gather_ok(c, log2interp) && fec_decode_gather_ok(c);
}
int tx_decode_gather(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, InterpGather *g, uint8_t *block0 = nullptr)
{
    sdrhip_ctx *c = tx->ctx;
    const size_t F = (size_t)tx->nstreams * nframes, rows = (size_t)c->opt.dec_max_rows, slots = F * rows + 1;
    if (F * 128 >= 0x7fffffffu || slots >= 0x7fffffffu) return fail(SDRHIP_EINVAL, "tx: too many frames in one call");
    int rc;
    if ((rc = tx->srcmap.reserve(F * 128 * sizeof(unsigned)))) return rc;
    if ((rc = tx->restored.reserve(slots * SDRHIP_BLOCK_BYTES))) return rc;
    if (tx->restored_slots != slots) { // (the all-zero slot behind the last frame's: wherever it lies for this batch size)
        HIP_TRY(hipMemsetAsync(tx->restored.as<uint8_t>() + (slots - 1) * SDRHIP_BLOCK_BYTES, 0, SDRHIP_BLOCK_BYTES, c->stream));
        tx->restored_slots = slots;
    }
    DecodeGather dg;
    dg.srcmap = tx->srcmap.as<unsigned>(); dg.restored = tx->restored.as<uint8_t>(); dg.rows = (int)rows;
    const size_t fb = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE;
    if ((rc = fec_decode_device(c, drx, fb, indices, F, nullptr, 0, block0, nullptr, &dg))) return rc;
    g->map = dg.srcmap; g->rx = drx; g->restored = dg.restored; g->frames = (int)nframes;
    return SDRHIP_OK;
}

// interpolate a decoded batch on the first stream into the caller's buffer (host: through outbuf + a download)
int tx_interpolate(sdrhip_tx *tx, int log2interp, const DevBuf &pay, size_t n_payload, size_t pstride, int16_t *iq_out, size_t out_stride, int mem,
                   const InterpGather *gather = nullptr)
{
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams;
    const size_t n_res = n_payload << log2interp;
    int16_t *dout = iq_out;
    size_t dos = out_stride;
    int rc;
    const size_t esz = tx_esz(tx);
    if (mem == SDRHIP_MEM_HOST) {
        dos = tx_pitch(tx, n_res);
        if ((rc = tx->outbuf.reserve((size_t)S * dos * esz + 16))) return rc;
        dout = tx->outbuf.as<int16_t>();
    }
    if ((rc = interpolate_device(tx->itp, log2interp, gather ? nullptr : pay.as<int16_t>(), n_payload, pstride, dout, dos, nullptr, gather, nullptr, tx->out_fmt))) return rc;
    if (mem == SDRHIP_MEM_HOST)
        HIP_TRY(link_copy2d(c, iq_out, out_stride * esz, dout, dos * esz, n_res * esz, S, hipMemcpyDeviceToHost, c->stream));
    return SDRHIP_OK;
}

// delivery half of a pipelined call (and of sdrhip_tx_flush): the waiting batch through the interpolator on the first stream
int tx_deliver_late(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams;
    const size_t n_res = tx->late.n_payload << tx->late.log2interp;
    if (S == 1) out_stride = n_res;
    if (!iq_out) return fail(SDRHIP_EINVAL, "tx: NULL output buffer for the waiting batch");
    if (out_stride < n_res) return fail(SDRHIP_EINVAL, "tx: out_stride smaller than the waiting batch (%zu samples per stream)", n_res);
    if (mem == SDRHIP_MEM_DEVICE && !tx_out_aligned(tx, iq_out, out_stride)) return fail(SDRHIP_EALIGN, "tx_process: device output must be 16-byte aligned, its stride a multiple of 4 (8-bit: 8) samples");
    const int sel = tx->psel ^ 1; // (psel already points at the buffer the NEXT decode fills)
    HIP_TRY(hipStreamWaitEvent(c->stream, tx->ev_dec, 0));
    int rc = tx_interpolate(tx, tx->late.log2interp, tx->payload[sel], tx->late.n_payload, tx->late.pstride, iq_out, out_stride, mem);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(tx->ev_itp[sel], c->stream));
    tx->itp_pending[sel] = true;
    tx->late.have = false;
    if (n_out) *n_out = n_res;
    return SDRHIP_OK;
}
} // namespace

extern "C" int sdrhip_tx_flush(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (n_out) *n_out = 0;
    if (mem != SDRHIP_MEM_HOST && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    if (!tx->late.have) return SDRHIP_OK;
    HIP_TRY(hipSetDevice(tx->ctx->device));
    int rc = tx_deliver_late(tx, iq_out, out_stride, n_out, mem);
    if (rc) return rc;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(tx->ctx->stream));
    return SDRHIP_OK;
}

extern "C" size_t sdrhip_tx_pending_samples(const sdrhip_tx *tx)
{
    if (!tx) return 0;
    sdrhip::CtxLock lock_(tx->ctx);
    return tx->late.have ? tx->late.n_payload << tx->late.log2interp : 0;
}

extern "C" int sdrhip_tx_process(sdrhip_tx *tx, const uint8_t *rx, const uint8_t *indices, size_t nframes, size_t rx_stride_bytes,
                                 int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    const size_t n_payload = nframes * SDRHIP_SAMPLES_PER_FRAME;
    const size_t n_res = n_payload << tx->log2interp;
    if (n_out) *n_out = tx->pipelined ? 0 : n_res;
    if (mem != SDRHIP_MEM_HOST && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    if (tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_process: asynchronous datagram batches are in flight: collect them first");
    if (nframes == 0) {
        // an empty call decodes nothing; in pipelined mode it still delivers the batch that waits
        if (tx->pipelined && tx->late.have) return sdrhip_tx_flush(tx, iq_out, out_stride, n_out, mem);
        return SDRHIP_OK;
    }
    if (!rx || (!iq_out && !tx->pipelined)) return fail(SDRHIP_EINVAL, "tx_process: NULL buffer");
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int S = tx->nstreams;
    const size_t fb = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE;
    if (S == 1) { rx_stride_bytes = nframes * fb; if (!tx->pipelined) out_stride = n_res; }
    if (rx_stride_bytes < nframes * fb || (!tx->pipelined && out_stride < n_res)) return fail(SDRHIP_EINVAL, "tx_process: stride too small");
    if (mem == SDRHIP_MEM_DEVICE && S > 1 && rx_stride_bytes != nframes * fb) return fail(SDRHIP_EINVAL, "tx_process: device rx must be contiguous per stream");
    const size_t pstride = (n_payload + 3) & ~(size_t)3; // samples
    int rc;

    if (tx->pipelined) {
        // ---- first stream: the batch that waits goes through the interpolator (enqueued FIRST: the long kernel takes the CUs, the
        // decoder's workgroups fill in as its waves retire); second stream: this call's batch is decoded beside it
        const bool overlap = c->opt.tx_overlap != 0;
        hipStream_t s2 = c->stream;
        if (overlap && (rc = ctx_stream2(c, &s2))) return rc;
        if (mem == SDRHIP_MEM_DEVICE && overlap) HIP_TRY(hipEventRecord(tx->ev_in, c->stream)); // (whatever produced rx on the caller's stream)
        if (tx->late.have) {
            if ((rc = tx_deliver_late(tx, iq_out, out_stride, n_out, mem))) return rc;
        }
        const int sel = tx->psel;
        DevBuf &pay = tx->payload[sel];
        if (pay.cap < (size_t)S * pstride * 4 + 16) {
            // (growing the buffer frees it: nothing may still read it)
            if (tx->itp_pending[sel]) { HIP_TRY(hipEventSynchronize(tx->ev_itp[sel])); tx->itp_pending[sel] = false; }
            if ((rc = pay.reserve((size_t)S * pstride * 4 + 16))) return rc;
        }
        const uint8_t *drx = rx;
        if (mem == SDRHIP_MEM_HOST) {
            if (overlap) HIP_TRY(hipStreamSynchronize(s2)); // (the previous decode may still read rxbuf; it ran beside the previous call's interpolator)
            if ((rc = tx->rxbuf.reserve((size_t)S * nframes * fb))) return rc;
            HIP_TRY(link_copy2d(c, tx->rxbuf.p, nframes * fb, rx, rx_stride_bytes, nframes * fb, S, hipMemcpyHostToDevice, s2));
            // (pinned caller memory makes this copy truly asynchronous, and it runs on the SECOND stream: the call must not return
            // before it has read `rx` -- the host-pointer contract is "the buffer is yours again when the call returns")
            if (overlap) HIP_TRY(hipEventRecord(tx->ev_up, s2));
            drx = tx->rxbuf.as<uint8_t>();
        } else if (overlap) {
            HIP_TRY(hipStreamWaitEvent(s2, tx->ev_in, 0));
        }
        if (overlap && tx->itp_pending[sel]) { HIP_TRY(hipStreamWaitEvent(s2, tx->ev_itp[sel], 0)); tx->itp_pending[sel] = false; }
        DecodeSide side;
        side.stream = s2; side.plan = &tx->plan_own; side.idx = &tx->idx_own; side.pin = &tx->pin_own;
        if ((rc = tx_decode(tx, drx, indices, nframes, pay, pstride, overlap ? &side : nullptr))) return rc;
        HIP_TRY(hipEventRecord(tx->ev_dec, s2));
        tx->late.have = true; tx->late.n_payload = n_payload; tx->late.pstride = pstride; tx->late.log2interp = tx->log2interp;
        tx->psel ^= 1;
        if (mem == SDRHIP_MEM_HOST) {
            HIP_TRY(hipStreamSynchronize(c->stream)); // (the delivered samples; the decode goes on)
            if (overlap) HIP_TRY(hipEventSynchronize(tx->ev_up)); // (... but the caller's rx has been read)
        }
        return SDRHIP_OK;
    }

    const uint8_t *drx = rx;
    if (mem == SDRHIP_MEM_HOST) {
        if ((rc = tx->rxbuf.reserve((size_t)S * nframes * fb))) return rc;
        HIP_TRY(link_copy2d(c, tx->rxbuf.p, nframes * fb, rx, rx_stride_bytes, nframes * fb, S, hipMemcpyHostToDevice, c->stream));
        drx = tx->rxbuf.as<uint8_t>();
    } else {
        if (!tx_out_aligned(tx, iq_out, out_stride)) return fail(SDRHIP_EALIGN, "tx_process: device output must be 16-byte aligned, its stride a multiple of 4 (8-bit: 8) samples");
    }
    if (tx_gather_applies(tx, tx->log2interp)) {
        // no-copy: decode (restored blocks + map only), then the interpolator reads the received frames through the map
        InterpGather g;
        if ((rc = tx_decode_gather(tx, drx, indices, nframes, &g))) return rc;
        if ((rc = tx_interpolate(tx, tx->log2interp, tx->payload[0], n_payload, pstride, iq_out, out_stride, mem, &g))) return rc;
        if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
        return SDRHIP_OK;
    }
    // decode all S * nframes frames in one batch: payload [S][nframes][127 * 508] = [S][n_payload] samples
    if ((rc = tx->payload[0].reserve((size_t)S * pstride * 4 + 16))) return rc;
    if ((rc = tx_decode(tx, drx, indices, nframes, tx->payload[0], pstride, nullptr))) return rc;
    if ((rc = tx_interpolate(tx, tx->log2interp, tx->payload[0], n_payload, pstride, iq_out, out_stride, mem))) return rc;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- asynchronous host-pointer Tx entry
// sdrdaemontx's chain is asynchronous as well: a reader thread keeps receiving super blocks while the main loop interpolates
// (sdrdaemontx.cpp:449-498), and SDRdaemonFECBuffer hands a frame out one frame late (SDRdaemonFECBuffer.cpp:133-139).
// sdrhip_tx_process on host pointers is upload + three launches + download + a synchronisation per call; submit / collect give
// the host-pointer path the reference's asynchrony: a batch of received frames goes out as ONE upload + decode + interpolate +
// download on the context's stream and the call returns; the samples (and the frames' meta blocks) are collected later, in order.
extern "C" int sdrhip_tx_set_async(sdrhip_tx *tx, int depth)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (depth < 1 || depth > 64) return fail(SDRHIP_EINVAL, "tx_set_async: depth 1..64");
    for (auto &b : tx->abatch)
        if (b.state != 0) return fail(SDRHIP_EINVAL, "tx_set_async: batches are in flight: collect them first");
    for (auto &b : tx->abatch) {
        if (b.done) (void)hipEventDestroy(b.done);
        b.in.release(); b.din.release(); b.dout.release(); b.db0.release(); b.out.release(); b.tab.release(); b.seg.release();
    }
    tx->abatch.assign((size_t)depth, sdrhip_tx::ABatch());
    tx->a_head = tx->a_tail = 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_submit(sdrhip_tx *tx, const uint8_t *rx, const uint8_t *indices, size_t nframes, size_t rx_stride_bytes)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (nframes == 0) return SDRHIP_OK;
    if (!rx) return fail(SDRHIP_EINVAL, "tx_submit: NULL input");
    if (tx->pipelined) return fail(SDRHIP_EINVAL, "tx_submit: the handle is in pipelined mode (sdrhip_tx_process delivers one call late there); use one or the other");
    if (tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_submit: asynchronous datagram batches are in flight: collect them first");
    if (tx->abatch.empty()) tx->abatch.assign(4, sdrhip_tx::ABatch());
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int S = tx->nstreams;
    const size_t fb = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, row = nframes * fb;
    if (S == 1) rx_stride_bytes = row;
    if (rx_stride_bytes < row) return fail(SDRHIP_EINVAL, "tx_submit: stride too small");
    sdrhip_tx::ABatch &b = tx->abatch[tx->a_tail % tx->abatch.size()];
    if (b.state == 2) return fail(SDRHIP_EBUSY, "tx_submit: every batch of the ring is in flight: sdrhip_tx_collect first");
    const size_t n_payload = nframes * SDRHIP_SAMPLES_PER_FRAME, n_res = n_payload << tx->log2interp;
    const size_t pstride = (n_payload + 3) & ~(size_t)3, dos = tx_pitch(tx, n_res), esz = tx_esz(tx);
    const size_t b0_bytes = (size_t)S * nframes * SDRHIP_BLOCK_BYTES;
    int rc;
    // everything that can fail for want of memory comes first
    if ((rc = b.din.reserve((size_t)S * row))) return rc;
    if ((rc = b.dout.reserve((size_t)S * dos * esz + 16))) return rc;
    if ((rc = b.db0.reserve(b0_bytes))) return rc;
    if ((rc = b.out.reserve((size_t)S * dos * esz + b0_bytes))) return rc;
    const bool gather = tx_gather_applies(tx, tx->log2interp);
    if (!gather && (rc = tx->payload[0].reserve((size_t)S * pstride * 4 + 16))) return rc;
    if (!b.done && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) { b.done = nullptr; return fail(SDRHIP_EDEVICE, "hipEventCreate"); }
    const uint8_t *src = rx;
    size_t sstride = rx_stride_bytes;
    if (!host_is_pinned(rx, (size_t)(S - 1) * rx_stride_bytes + row)) {
        if ((rc = b.in.reserve((size_t)S * row))) return rc; // (waits for the upload of the batch that used this buffer last)
        for (int s = 0; s < S; ++s) memcpy(b.in.as<char>() + (size_t)s * row, rx + (size_t)s * rx_stride_bytes, row);
        src = b.in.as<uint8_t>(); sstride = row;
    }
    if (S == 1) HIP_TRY(link_copy(c, b.din.p, src, row, hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(link_copy2d(c, b.din.p, row, src, sstride, row, S, hipMemcpyHostToDevice, c->stream));
    if (src != rx) b.in.mark(c->stream);
    if (gather) {
        // (the batch's received frames live in b.din until it is collected: the interpolator reads them in place)
        InterpGather g;
        if ((rc = tx_decode_gather(tx, b.din.as<uint8_t>(), indices, nframes, &g, b.db0.as<uint8_t>()))) return rc;
        if ((rc = interpolate_device(tx->itp, tx->log2interp, nullptr, n_payload, pstride, b.dout.as<int16_t>(), dos, nullptr, &g))) return rc;
    } else {
        if ((rc = tx_decode(tx, b.din.as<uint8_t>(), indices, nframes, tx->payload[0], pstride, nullptr, b.db0.as<uint8_t>()))) return rc;
        if ((rc = interpolate_device(tx->itp, tx->log2interp, tx->payload[0].as<int16_t>(), n_payload, pstride, b.dout.as<int16_t>(), dos, nullptr,
                                     nullptr, nullptr, tx->out_fmt)))
            return rc;
    }
    // (from here on the interpolator's state has advanced: a failure loses the batch, it is never replayed)
    hipError_t e = link_copy(c, b.out.p, b.dout.p, (size_t)S * dos * esz, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = link_copy(c, b.out.as<char>() + (size_t)S * dos * esz, b.db0.p, b0_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "tx batch download: %s (the batch's %zu frames per stream are lost)", hipGetErrorString(e), nframes);
    b.nframes = nframes; b.n_res = n_res; b.dos = dos;
    b.state = 2;
    ++tx->a_tail;
    return SDRHIP_OK;
}

// the oldest batch of the ring once it has finished (wait = 1: waits OUTSIDE the context lock -- the submitting thread, the
// reference's reader thread, keeps feeding the ring)
static int tx_wait_oldest(sdrhip_tx *tx, std::unique_lock<std::recursive_mutex> &lock_, int wait, const char *who, sdrhip_tx::ABatch **bp)
{
    for (;;) {
        sdrhip_tx::ABatch &h = tx->abatch[tx->a_head % tx->abatch.size()];
        if (h.state == 0) return fail(SDRHIP_EBUSY, "%s: nothing was submitted", who);
        const hipError_t q = hipEventQuery(h.done);
        if (q == hipSuccess) { *bp = &h; break; }
        if (q != hipErrorNotReady) return fail(SDRHIP_EDEVICE, "hipEventQuery: %s", hipGetErrorString(q));
        if (!wait) return fail(SDRHIP_EBUSY, "%s: the oldest batch is still in flight", who);
        const size_t head = tx->a_head;
        hipEvent_t ev = h.done;
        lock_.unlock();
        const hipError_t w = hipEventSynchronize(ev);
        lock_.lock();
        if (w != hipSuccess) return fail(SDRHIP_EDEVICE, "hipEventSynchronize: %s", hipGetErrorString(w));
        if (tx->a_head == head) { *bp = &tx->abatch[head % tx->abatch.size()]; break; }
        // (another thread collected that batch meanwhile: look at the new head)
    }
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_collect(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_samples, uint8_t *block0_out, size_t *n_out, size_t *n_frames, int wait)
{
    if (!tx || !n_out) return fail(SDRHIP_EINVAL, "tx_collect: NULL argument");
    // (the wait happens outside the context lock: the submitting thread -- the reference's reader thread -- keeps feeding the ring)
    std::unique_lock<std::recursive_mutex> lock_(tx->ctx->mtx);
    *n_out = 0;
    if (n_frames) *n_frames = 0;
    if (tx->abatch.empty()) return fail(SDRHIP_EBUSY, "tx_collect: nothing was submitted");
    if (tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_collect: asynchronous datagram batches are in flight: use sdrhip_tx_collect_datagrams");
    HIP_TRY(hipSetDevice(tx->ctx->device));
    sdrhip_tx::ABatch *bp = nullptr;
    int rc = tx_wait_oldest(tx, lock_, wait, "tx_collect", &bp);
    if (rc) return rc;
    sdrhip_tx::ABatch &b = *bp;
    const int S = tx->nstreams;
    const size_t esz = tx_esz(tx); // (the format cannot change while a batch is in flight)
    if (b.n_res > max_samples) { // (the batch stays where it is: call again with room for *n_out samples per stream)
        *n_out = b.n_res;
        if (n_frames) *n_frames = b.nframes;
        return fail(SDRHIP_EINVAL, "tx_collect: the batch holds %zu samples per stream, iq_out has room for %zu", b.n_res, max_samples);
    }
    if (b.n_res) {
        if (!iq_out) return fail(SDRHIP_EINVAL, "tx_collect: NULL iq_out");
        if (S == 1) out_stride = b.n_res;
        if (out_stride < b.n_res) return fail(SDRHIP_EINVAL, "tx_collect: out_stride too small");
        for (int s = 0; s < S; ++s) memcpy(reinterpret_cast<char *>(iq_out) + (size_t)s * out_stride * esz, b.out.as<char>() + (size_t)s * b.dos * esz, b.n_res * esz);
    }
    if (block0_out) memcpy(block0_out, b.out.as<char>() + (size_t)S * b.dos * esz, (size_t)S * b.nframes * SDRHIP_BLOCK_BYTES);
    *n_out = b.n_res;
    if (n_frames) *n_frames = b.nframes;
    b.state = 0;
    ++tx->a_head;
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- Tx pipe fed datagrams
// UDPSourceFEC::read -> SDRdaemonFECBuffer::writeAndRead -> Upsampler::process for every stream (sdrdaemontx.cpp:449-498,
// UDPSourceFEC.cpp:52-78): the FEC buffer bank collects and decodes into payload[0] ([stream][pitch] samples, every stream 16-byte
// aligned: one frame is 64 516 bytes = 4 mod 16, and K5w's paired loads want aligned streams), then ONE ragged interpolator launch
// takes each stream's own count from where the bank's classify pass left it.  The grid is planned from the largest count, which
// the host holds after the bank's one read-back.
namespace {
int tx_collector(sdrhip_tx *tx)
{
    return tx->fb ? SDRHIP_OK : sdrhip_fecbuf_create(tx->ctx, tx->nstreams, &tx->fb);
}
} // namespace

extern "C" int sdrhip_tx_collector(sdrhip_tx *tx, sdrhip_fecbuf **out)
{
    if (!tx || !out) return fail(SDRHIP_EINVAL, "tx_collector: NULL argument");
    sdrhip::CtxLock lock_(tx->ctx);
    int rc = tx_collector(tx);
    if (rc) return rc;
    *out = tx->fb;
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_process_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                           int16_t *iq_out, size_t out_stride, size_t max_frames, uint8_t *block0_out,
                                           sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (!n_dgrams || !n_frames) return fail(SDRHIP_EINVAL, "tx_process_datagrams: NULL n_dgrams / n_frames");
    if (mem != SDRHIP_MEM_HOST && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
    if (tx->pipelined) return fail(SDRHIP_EINVAL, "tx_process_datagrams: the handle is in pipelined mode");
    for (const auto &b : tx->abatch)
        if (b.state != 0) return fail(SDRHIP_EINVAL, "tx_process_datagrams: asynchronous batches are in flight: collect them first");
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams, L = tx->log2interp;
    if (max_frames > 0x3fffffffu) return fail(SDRHIP_EINVAL, "tx_process_datagrams: max_frames too large");
    if (max_frames > 0 && (!iq_out || !info_out)) return fail(SDRHIP_EINVAL, "tx_process_datagrams: NULL iq_out / info_out");
    const size_t per = max_frames * SDRHIP_SAMPLES_PER_FRAME, n_res_max = per << L;
    const bool s8 = tx->out_fmt == IQF_S8;
    const size_t esz = tx_esz(tx);
    if (S == 1) out_stride = tx_pitch(tx, n_res_max);
    if (out_stride < n_res_max) return fail(SDRHIP_EINVAL, "tx_process_datagrams: out_stride below max_frames x 16129 << log2interp");
    if (mem == SDRHIP_MEM_DEVICE && max_frames > 0 && (!aligned16(iq_out) || (out_stride & (s8 ? 7 : 3)) || (reinterpret_cast<uintptr_t>(block0_out) & 3u)))
        return fail(SDRHIP_EALIGN, "tx_process_datagrams: device iq_out must be 16-byte aligned, out_stride a multiple of 4 (8-bit: 8) samples, block0_out 4-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = tx_collector(tx))) return rc;
    if ((rc = fecbuf_check_dgrams(tx->fb, dgrams, n_dgrams, dgram_stride_bytes, mem, "tx_process_datagrams"))) return rc;
    // where the collector writes getSlotData: the caller's device iq_out (Upsampler's m_interp == 0 pass-through, Upsampler.cpp:54-57)
    // or payload[0]; host memory: outbuf / payload[0], downloaded below
    // (8-bit output with x1: the collector writes int16 to payload[0] as for the other ratios, K6n narrows it into dout)
    const size_t pitch = (per + 3) & ~(size_t)3, n_res_pitch = tx_pitch(tx, n_res_max);
    const bool direct = L == 0 && !s8;
    int16_t *dout = iq_out;
    size_t dos = out_stride;
    if (max_frames > 0 && mem == SDRHIP_MEM_HOST) {
        if ((rc = tx->outbuf.reserve((size_t)S * n_res_pitch * esz + 16))) return rc;
        dout = tx->outbuf.as<int16_t>(); dos = n_res_pitch;
    }
    if (max_frames > 0 && !direct && (rc = tx->payload[0].reserve((size_t)S * pitch * 4 + 16))) return rc;
    uint8_t *data = direct ? reinterpret_cast<uint8_t *>(dout) : tx->payload[0].as<uint8_t>();
    const size_t data_stride = direct ? dos * 4 : pitch * 4;
    const int *counts = nullptr;
    if ((rc = fecbuf_collect(tx->fb, dgrams, n_dgrams, dgram_stride_bytes, mem, max_frames ? data : nullptr, data_stride, block0_out, max_frames,
                             info_out, n_frames, &counts)))
        return rc; // (SDRHIP_EINVAL for want of room: nothing consumed, the interpolator has not run)
    size_t kmax = 0;
    for (int s = 0; s < S; ++s) kmax = n_frames[s] > kmax ? n_frames[s] : kmax;
    const size_t n_max = kmax * SDRHIP_SAMPLES_PER_FRAME;
    if (L == 0 && s8 && kmax > 0) {
        // (x1 has no count-aware kernel: K6n narrows the largest stream's length; past a stream's own count the samples are unspecified)
        if ((rc = interpolate_device(tx->itp, 0, tx->payload[0].as<int16_t>(), n_max, pitch, dout, dos, nullptr, nullptr, nullptr, IQF_S8))) return rc;
    } else if (L > 0 && kmax > 0) {
        // (the collector's state has moved on: from here a failure loses the call's frames, it is never replayed)
        const InterpCount cnt = {counts + FB_K, FB_COUNTS, (int)SDRHIP_SAMPLES_PER_FRAME};
        if ((rc = interpolate_device(tx->itp, L, tx->payload[0].as<int16_t>(), n_max, pitch, dout, dos, nullptr, nullptr, &cnt, tx->out_fmt))) return rc;
    }
    if (mem == SDRHIP_MEM_HOST) {
        if (kmax > 0)
            HIP_TRY(link_copy2d(c, iq_out, out_stride * esz, dout, dos * esz, (n_max << L) * esz, (size_t)S, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- asynchronous Tx batches of raw datagrams
// sdrdaemontx's reader thread receives datagrams while its main loop interpolates (sdrdaemontx.cpp:449-498).  A batch goes out with
// no synchronisation: its datagrams up packed (one memcpy per stream into the batch's pinned arena, or in place from
// sdrhip_host_alloc memory), the collector's passes with grids from the host's shadow of the classification (fecbuf_packed: no
// read-back), the decoder, the interpolator at the factor in force, the delivery gather, ONE download of exactly the delivered
// bytes.  The collector and the histories are the ones sdrhip_tx_process_datagrams and sdrhip_tx_process use.
namespace {
constexpr size_t DG_REC = sizeof(sdrhip_fecbuf_frame);
static_assert(sizeof(sdrhip_fecbuf_frame) == sizeof(FecBufPub), "public record layout");
// a failure behind the collector's scatter launch: the batch is consumed and lost, never replayed
int tx_batch_lost(int rc)
{
    const std::string m = sdrhip_last_error();
    return fail(rc, "tx_submit_datagrams: %s (the batch is lost)", m.c_str());
}
} // namespace

extern "C" int sdrhip_tx_submit_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    if (!n_dgrams) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: NULL n_dgrams");
    sdrhip::CtxLock lock_(tx->ctx);
    // ---- everything that can be refused is checked before anything is consumed
    const int S = tx->nstreams;
    size_t sum = 0, nmax = 0;
    for (int s = 0; s < S; ++s) {
        if (n_dgrams[s] > 0x3fffffffu) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: too many datagrams in one batch");
        sum += n_dgrams[s];
        nmax = n_dgrams[s] > nmax ? n_dgrams[s] : nmax;
    }
    const bool packed = dgram_stride_bytes == SDRHIP_PACKED || S == 1;
    if (sum && !dgrams) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: NULL dgrams");
    if (!packed && dgram_stride_bytes < nmax * SDRHIP_UDPSIZE)
        return fail(SDRHIP_EINVAL, "tx_submit_datagrams: dgram_stride_bytes is neither SDRHIP_PACKED nor at least the largest count x 512");
    if (tx->pipelined) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: the handle is in pipelined mode");
    if (tx->late.have) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: a pipelined batch waits: sdrhip_tx_flush it first");
    if (tx_in_flight(tx, false)) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: batches of received frames are in flight: sdrhip_tx_collect them first");
    if (tx->abatch.empty()) tx->abatch.assign(4, sdrhip_tx::ABatch());
    sdrhip_tx::ABatch &b = tx->abatch[tx->a_tail % tx->abatch.size()];
    if (b.state == 2) return fail(SDRHIP_EBUSY, "tx_submit_datagrams: every batch of the ring is in flight: sdrhip_tx_collect_datagrams first");
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = tx_collector(tx))) return rc;
    std::vector<FecBufShadow> sh;
    if ((rc = fecbuf_shadow(tx->fb, &sh))) return rc;

    // ---- staging: packed, one memcpy per non-empty stream (in place: the caller's pinned memory); the shadow runs over the headers
    const size_t bytes_in = sum * SDRHIP_UDPSIZE;
    auto row_of = [&](int s, size_t off) { return packed ? dgrams + off : dgrams + (size_t)s * dgram_stride_bytes; };
    const bool inplace = sum && (packed ? host_is_pinned(dgrams, bytes_in) : host_is_pinned(dgrams, (size_t)(S - 1) * dgram_stride_bytes + nmax * SDRHIP_UDPSIZE));
    if (sum && !inplace && (rc = b.in.reserve(bytes_in))) return rc; // (waits for the upload of this slot's last batch)
    std::vector<int> res((size_t)S * 4);
    {
        size_t off = 0;
        for (int s = 0; s < S; ++s) {
            const size_t nb = n_dgrams[s] * SDRHIP_UDPSIZE;
            const uint8_t *src = row_of(s, off);
            if (nb && !inplace) {
                memcpy(b.in.as<uint8_t>() + off, src, nb);
                src = b.in.as<uint8_t>() + off;
            }
            fecbuf_shadow_run(sh[(size_t)s], src, n_dgrams[s], &res[(size_t)s * 4]);
            off += nb;
        }
    }
    size_t kmax = 0, kall = 0;
    for (int s = 0; s < S; ++s) {
        kmax = (size_t)res[(size_t)s * 4] > kmax ? (size_t)res[(size_t)s * 4] : kmax;
        kall += (size_t)res[(size_t)s * 4];
    }
    const int L = tx->log2interp;
    const bool s8 = tx->out_fmt == IQF_S8, direct = L == 0 && !s8;
    const size_t esz = tx_esz(tx), per = kmax * SDRHIP_SAMPLES_PER_FRAME, pitch = (per + 3) & ~(size_t)3;
    const size_t dos = tx_pitch(tx, per << L), n_one = (size_t)SDRHIP_SAMPLES_PER_FRAME << L;
    const size_t b_samples = kall * n_one * esz, b_total = b_samples + kall * (DG_REC + SDRHIP_BLOCK_BYTES);
    // everything that can fail for want of memory comes before the collector moves (a device buffer that grows waits for the
    // batches in flight)
    if (sum && (rc = reserve_settled(c, tx->a_pk, bytes_in + 16))) return rc;
    if (kmax && !direct && (rc = reserve_settled(c, tx->a_pay, (size_t)S * pitch * 4 + 16))) return rc;
    if (kmax && (rc = reserve_settled(c, tx->a_out, (size_t)S * dos * esz + 16))) return rc;
    if (kmax && (rc = reserve_settled(c, tx->a_b0, (size_t)S * kmax * SDRHIP_BLOCK_BYTES + 16))) return rc;
    if (b_total && (rc = reserve_settled(c, tx->a_gat, b_total + 16))) return rc;
    if ((rc = reserve_settled(c, tx->a_seg, (size_t)3 * S * sizeof(GatherSeg)))) return rc;
    if (b_total && (rc = b.out.reserve(b_total))) return rc;
    if ((rc = b.seg.reserve((size_t)3 * S * sizeof(GatherSeg)))) return rc;
    if (!b.done && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) { b.done = nullptr; return fail(SDRHIP_EDEVICE, "hipEventCreate"); }

    // ---- upload: exactly the datagrams (staged: one copy; in place: one per run of adjacent rows)
    uint8_t *pk = tx->a_pk.as<uint8_t>();
    if (sum && !inplace) {
        HIP_TRY(link_copy(c, pk, b.in.p, bytes_in, hipMemcpyHostToDevice, c->stream));
        b.in.mark(c->stream);
    } else if (sum) {
        size_t off = 0;
        for (int s = 0; s < S;) {
            const uint8_t *p0 = row_of(s, off);
            size_t n = n_dgrams[s] * SDRHIP_UDPSIZE;
            int j = s + 1;
            // (packed input is one run; a strided row joins the next one when it fills its stride)
            for (; j < S && p0 + n == row_of(j, off + n); ++j) n += n_dgrams[j] * SDRHIP_UDPSIZE;
            if (n) HIP_TRY(link_copy(c, pk + off, p0, n, hipMemcpyHostToDevice, c->stream));
            off += n;
            s = j;
        }
    }

    // ---- the collector's passes, no read-back (from the scatter launch on, the batch is consumed: a failure loses it)
    uint8_t *data = direct ? tx->a_out.as<uint8_t>() : tx->a_pay.as<uint8_t>();
    const size_t data_stride = direct ? dos * 4 : pitch * 4;
    bool committed = false;
    const int *counts = nullptr;
    const FecBufPub *pub = nullptr;
    rc = fecbuf_packed(tx->fb, pk, n_dgrams, res.data(), sh, b.tab, kmax ? data : nullptr, data_stride, kmax ? tx->a_b0.as<uint8_t>() : nullptr, kmax,
                       c->dec_stats + DEC_STATS_SHADOW_MISMATCH, &committed, &counts, &pub);
    if (rc && !committed) return rc; // (nothing consumed)
    if (rc) return tx_batch_lost(rc);
    // ---- the interpolator (x1: the collector wrote the samples where the gather reads them; 8-bit x1: K6n narrows them)
    if (L == 0 && s8 && kmax) {
        rc = interpolate_device(tx->itp, 0, tx->a_pay.as<int16_t>(), per, pitch, tx->a_out.as<int16_t>(), dos, nullptr, nullptr, nullptr, IQF_S8);
    } else if (L > 0 && kmax) {
        const InterpCount cnt = {counts + FB_K, FB_COUNTS, (int)SDRHIP_SAMPLES_PER_FRAME};
        rc = interpolate_device(tx->itp, L, tx->a_pay.as<int16_t>(), per, pitch, tx->a_out.as<int16_t>(), dos, nullptr, nullptr, &cnt, tx->out_fmt);
    }
    if (rc) return tx_batch_lost(rc);
    // ---- the delivery: every stream's samples, then the records, then the meta blocks, gathered and downloaded in ONE copy
    GatherSeg *seg = b.seg.as<GatherSeg>();
    int nseg = 0;
    uint64_t dst = 0;
    for (int part = 0; part < 3; ++part)
        for (int s = 0; s < S; ++s) {
            const size_t k = (size_t)res[(size_t)s * 4];
            if (!k) continue;
            GatherSeg &g = seg[nseg++];
            if (part == 0) { g.src = tx->a_out.as<uint8_t>() + (size_t)s * dos * esz; g.bytes = k * n_one * esz; }
            else if (part == 1) { g.src = reinterpret_cast<const uint8_t *>(pub + (size_t)s * kmax); g.bytes = k * DG_REC; }
            else { g.src = tx->a_b0.as<uint8_t>() + (size_t)s * kmax * SDRHIP_BLOCK_BYTES; g.bytes = k * SDRHIP_BLOCK_BYTES; }
            g.dst = dst; g.pad = 0;
            dst += g.bytes;
        }
    const uint32_t grid = gather_plan(seg, nseg);
    hipError_t e = nseg && !grid ? hipErrorInvalidValue : hipSuccess;
    if (e == hipSuccess && nseg) e = hipMemcpyAsync(tx->a_seg.p, seg, (size_t)nseg * sizeof(GatherSeg), hipMemcpyHostToDevice, c->stream); // (not counted: a table)
    if (e == hipSuccess && nseg) {
        b.seg.mark(c->stream);
        KTimer kt(c, SDRHIP_K_CONVERT);
        e = launch_delivery_gather(tx->a_seg.as<GatherSeg>(), nseg, grid, tx->a_gat.as<uint8_t>(), c->stream);
    }
    if (e == hipSuccess && b_total) e = link_copy(c, b.out.p, tx->a_gat.p, b_total, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "tx datagram batch delivery: %s (the batch is lost)", hipGetErrorString(e));
    b.frames.resize((size_t)S);
    for (int s = 0; s < S; ++s) b.frames[(size_t)s] = (size_t)res[(size_t)s * 4];
    b.dg = true; b.log2interp = L; b.esz = esz;
    b.nframes = kmax; b.n_res = kmax * n_one; b.dos = 0;
    b.state = 2;
    ++tx->a_tail;
    fecbuf_set_async_busy(tx->fb, true);
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_collect_datagrams(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_frames, uint8_t *block0_out,
                                           sdrhip_fecbuf_frame *info_out, size_t *n_frames, int wait)
{
    if (!tx || !n_frames) return fail(SDRHIP_EINVAL, "tx_collect_datagrams: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(tx->ctx->mtx);
    const int S = tx->nstreams;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    if (tx->abatch.empty()) return fail(SDRHIP_EBUSY, "tx_collect_datagrams: nothing was submitted");
    if (tx_in_flight(tx, false)) return fail(SDRHIP_EINVAL, "tx_collect_datagrams: batches of received frames are in flight: use sdrhip_tx_collect");
    HIP_TRY(hipSetDevice(tx->ctx->device));
    sdrhip_tx::ABatch *bp = nullptr;
    int rc = tx_wait_oldest(tx, lock_, wait, "tx_collect_datagrams", &bp);
    if (rc) return rc;
    sdrhip_tx::ABatch &b = *bp;
    // (the batch stays where it is while the caller lacks room: n_frames says how much it needs)
    const size_t kmax = b.nframes, n_one = (size_t)SDRHIP_SAMPLES_PER_FRAME << b.log2interp;
    if (kmax > max_frames) {
        for (int s = 0; s < S; ++s) n_frames[s] = b.frames[(size_t)s];
        return fail(SDRHIP_EINVAL, "tx_collect_datagrams: a stream of the batch released %zu frames, the outputs have room for %zu", kmax, max_frames);
    }
    if (kmax) {
        if (S > 1 && out_stride < kmax * n_one) {
            for (int s = 0; s < S; ++s) n_frames[s] = b.frames[(size_t)s];
            return fail(SDRHIP_EINVAL, "tx_collect_datagrams: out_stride below the batch's %zu samples per stream", kmax * n_one);
        }
        if (!iq_out || !info_out) return fail(SDRHIP_EINVAL, "tx_collect_datagrams: NULL iq_out / info_out");
        size_t kall = 0;
        for (int s = 0; s < S; ++s) kall += b.frames[(size_t)s];
        const uint8_t *src = b.out.as<uint8_t>(), *rec = src + kall * n_one * b.esz, *meta = rec + kall * DG_REC;
        for (int s = 0; s < S; ++s) {
            const size_t k = b.frames[(size_t)s];
            if (!k) continue;
            memcpy(reinterpret_cast<uint8_t *>(iq_out) + (size_t)s * out_stride * b.esz, src, k * n_one * b.esz);
            memcpy(info_out + (size_t)s * max_frames, rec, k * DG_REC);
            if (block0_out) memcpy(block0_out + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES, meta, k * SDRHIP_BLOCK_BYTES);
            src += k * n_one * b.esz; rec += k * DG_REC; meta += k * SDRHIP_BLOCK_BYTES;
        }
    }
    for (int s = 0; s < S; ++s) n_frames[s] = b.frames[(size_t)s];
    b.state = 0;
    b.dg = false;
    ++tx->a_head;
    fecbuf_set_async_busy(tx->fb, tx_in_flight(tx, true));
    return SDRHIP_OK;
}
