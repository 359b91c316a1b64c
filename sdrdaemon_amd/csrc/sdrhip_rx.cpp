// sdrhip_rx.cpp -- the fused Rx pipe of include/sdrhip.h: life cycle, configuration, the uniform and the ragged step (the
// datagram-fed call in front of it: sdrhip_rx_datagrams.cpp).  The per-stream settings' values and records and the counts of a
// ragged step are rx_stream_settings.h's, what a step launches is rx_step_plan.h's; here they meet the device.
#include "sdrhip_pipes.h"

using namespace sdrhip;

static int rx_check_config(const sdrhip_rx_config *cfg);

extern "C" int sdrhip_rx_create(sdrhip_ctx *ctx, int nstreams, const sdrhip_rx_config *cfg, sdrhip_rx **out)
{
    if (!ctx || !cfg || !out || nstreams <= 0) return fail(SDRHIP_EINVAL, "rx_create: bad argument");
    {
        const int rcc = rx_check_config(cfg);
        if (rcc) return rcc;
    }
    sdrhip_rx *rx = new (std::nothrow) sdrhip_rx(ctx);
    if (!rx) return fail(SDRHIP_ENOMEM, "out of host memory");
    rx->nstreams = nstreams; rx->cfg = *cfg;
    rx->area.init((size_t)nstreams);
    rx->view.init((size_t)nstreams);
    rx->streams.init((size_t)nstreams);
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

// the planner's inputs that the handle and the context hold: the ONE place that reads the arrangement options
static RxStepIn rx_step_inputs(const sdrhip_rx *rx)
{
    const sdrhip_ctx *c = rx->ctx;
    RxStepIn in = RxStepIn();
    in.L = rx->cfg.log2decim; in.fcpos = rx->cfg.fcpos; in.R = rx->cfg.nb_fec; in.pipelined = rx->pipelined != 0;
    in.late_have = rx->late.have; in.late_encode = rx->late.encode; in.late_frames = rx->late.frames; in.late_frame_bytes = rx->late.frame_bytes;
    in.ev_framed = (hipEvent_t)rx->ev_framed != nullptr;
    in.rx_fused = c->opt.rx_fused; in.rx_direct = c->opt.rx_direct; in.enc_min_rows = enc128_min_rows(c);
    return in;
}
// the ragged step's: K1mr stores straight into the windows of the area as it stands
static bool rx_stores_direct(const sdrhip_rx *rx, bool plan_mfma) { return rx_ragged_direct(plan_mfma, rx->ctx->opt.rx_direct, rx->area.cap() * rx_frame_bytes(rx)); }

// the encode that a pipelined call left for the next launch, now (flush, reconfiguration, a call that cannot fuse it)
static int rx_settle(sdrhip_rx *rx)
{
    if (!rx->late.encode) return SDRHIP_OK;
    rx->late.encode = false;
    sdrhip_ctx *c = rx->ctx;
    if (!rx_late_overlaps(rx_step_inputs(rx))) return fec_encode128_launch(c, rx->late.k);
    // overlap mode: the encode goes to the second stream -- behind everything the call that left it had enqueued (ev_framed), beside
    // whatever the first stream runs now (the decimator of the current call, enqueued just before) -- and the first stream picks
    // up behind it: the frames are delivered, and the buffers reused, in first-stream order
    hipStream_t s2 = nullptr;
    int rc = ctx_stream2(c, &s2);
    if (rc) return rc;
    if ((rc = rx->ev_enc.ensure())) return rc;
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
    if (on && rx_refuse_uniform("rx_set_pipelined", nullptr, rx->streams.forces_ragged())) return SDRHIP_EINVAL;
    if (on && rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_set_pipelined: asynchronous datagram batches are in flight: collect them first");
    if (on && !rx->area.aligned()) return fail(SDRHIP_EINVAL, "rx_set_pipelined: ragged calls left the streams at different frame positions");
    rx->pipelined = on ? 1 : 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_set_input_format(sdrhip_rx *rx, int fmt)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (fmt != SDRHIP_IQ_S16 && fmt != SDRHIP_IQ_U8 && fmt != SDRHIP_IQ_S8) return fail(SDRHIP_EINVAL, "rx_set_input_format: unknown format %d", fmt);
    if (rx->ring.busy()) return fail(SDRHIP_EINVAL, "rx_set_input_format: asynchronous batches are being filled or in flight: collect them first");
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

// the old frame area of a pipelined pipe, kept while frames wait for delivery in it
static int rx_release_old(sdrhip_rx *rx)
{
    if (rx->old_work.p && !(rx->late.have && rx->late.in_old)) {
        HIP_TRY(hipStreamSynchronize(rx->ctx->stream));
        rx->old_work.release();
    }
    return SDRHIP_OK;
}

// Carries a plan out: `bytes` of every open frame whose window moves go to slot 0 of its stream -- of `fresh` (slots of dst_pitch
// bytes; it becomes the area behind a synchronisation: earlier launches may still use the old one) or, fresh = NULL, in place.
// One strided copy when every stream moves from the same slot, else one copy per stream.  A failure releases `fresh` and leaves
// the handle as it was.
static int rx_run_plan(sdrhip_rx *rx, const RxAreaPlan &p, DevBuf *fresh, size_t src_pitch, size_t dst_pitch, size_t bytes, const char *who)
{
    sdrhip_ctx *c = rx->ctx;
    const RxFrameArea &A = rx->area;
    const size_t S = A.streams(), dcap = fresh ? p.new_cap : A.cap();
    const uint8_t *src = rx->work.as<uint8_t>();
    uint8_t *dst = fresh ? fresh->as<uint8_t>() : rx->work.as<uint8_t>();
    bool together = true;
    for (size_t s = 0; s < S; ++s) together = together && p.to_slot0[s] && A.open(s) && A.slot(s) == A.slot(0);
    hipError_t e = hipSuccess;
    if (together)
        e = hipMemcpy2DAsync(dst, dcap * dst_pitch, src + A.slot(0) * src_pitch, A.cap() * src_pitch, bytes, S, hipMemcpyDeviceToDevice, c->stream);
    else
        for (size_t s = 0; s < S && e == hipSuccess; ++s)
            if (p.to_slot0[s] && A.open(s))
                e = hipMemcpyAsync(dst + s * dcap * dst_pitch, src + A.index(s) * src_pitch, bytes, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && fresh) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (fresh) { (void)hipStreamSynchronize(c->stream); fresh->release(); }
        return fail(SDRHIP_EDEVICE, "%s: moving the open frames: %s", who, hipGetErrorString(e));
    }
    if (fresh) {
        if (p.keep_old) { rx->old_work = std::move(rx->work); rx->late.in_old = true; } // (frees what old_work held)
        rx->work = std::move(*fresh); // (frees the area the windows leave, unless old_work took it)
        rx->view.clear(); // (the view of the last call's frames does not outlive the area it points into)
    }
    rx->area.moved(p);
    return SDRHIP_OK;
}

// the windows where a call that completes done[s] frames of stream s can write: plan, new area if the plan asks for one, moves
// (grow_only: ahead of the call, nothing moves in place yet)
static int rx_make_room(sdrhip_rx *rx, const size_t *done, bool pipelined, const char *who, bool grow_only = false)
{
    sdrhip_ctx *c = rx->ctx;
    // the window: TWO calls' frames (round 5; four until then).  The step rewrites what it wrote two calls ago: 2 x 84 MB per
    // 8-stream bank stay in the 256 MB of Infinity Cache, and on this memory system a write stream that stays there
    // costs the read stream beside it less (profiles/r05_rx_direct.txt: decimator launch 0.2435 -> 0.2335 ms, encoder
    // launch 0.052 -> 0.049 ms; a window of one call wraps -- a copy of the open frames -- on every call).  option rx_window (SDRHIP_RX_WINDOW at context creation, 1..8) = A / B
    // (pipelined pipes keep the previous call's frames until they are delivered: four calls, as before)
    const size_t wmul = c->opt.rx_window ? (size_t)c->opt.rx_window : pipelined ? 4 : 2;
    const RxAreaPlan p = rx->area.plan(done, rx->late.have && !rx->late.in_old ? rx->late.first : RX_NO_LATE, wmul);
    if (!p.new_cap && (grow_only || !p.moves())) return SDRHIP_OK;
    const size_t fb = rx_frame_bytes(rx);
    DevBuf fresh;
    if (p.new_cap)
        if (int rc = fresh.reserve(rx->area.streams() * p.new_cap * fb)) return rc;
    return rx_run_plan(rx, p, p.new_cap ? &fresh : nullptr, fb, fb, fb, who);
}

// the slots change size (a fecblk change): the frame being filled (its 128 original super blocks) moves to slot 0 of a new area
static int rx_repitch(sdrhip_rx *rx, size_t new_fb, const char *who)
{
    if (!rx->area.cap() || new_fb == rx_frame_bytes(rx)) return SDRHIP_OK;
    int rc;
    if ((rc = rx_settle(rx))) return rc;
    DevBuf fresh;
    if ((rc = fresh.reserve(rx->area.streams() * rx->area.cap() * new_fb))) return rc;
    if ((rc = rx_run_plan(rx, rx->area.replan(), &fresh, rx_frame_bytes(rx), new_fb, (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, who))) return rc;
    // (no frames wait for delivery here: a fecblk change with late.have set is refused by the callers)
    rx->old_work.release();
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
    // (per-stream fecblk: cfg.nb_fec is unused while the array is set, the slots keep their pitch)
    const bool fec_changes = rx->streams.forces_ragged() != RX_SET_FEC && cfg->nb_fec != rx->cfg.nb_fec;
    if (fec_changes && rx->late.have)
        return fail(SDRHIP_EINVAL, "rx_reconfigure: frames of the previous call wait for delivery (pipelined mode): sdrhip_rx_flush them "
                                   "before changing fecblk (they carry the old frame size)");
    if (fec_changes && (rc = rx_repitch(rx, (size_t)(SDRHIP_NB_ORIGINAL + cfg->nb_fec) * SDRHIP_UDPSIZE, "rx_reconfigure"))) return rc;
    rx->cfg = *cfg;
    return SDRHIP_OK;
}

extern "C" void sdrhip_rx_destroy(sdrhip_rx *rx)
{
    if (!rx) return;
    sdrhip_ctx *c = rx->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2); // (an encode of the overlap mode may still run there)
    rx->ring.wait_all();
    sdrhip_decimators_destroy(rx->dec);
    sdrhip_fecbuf_destroy(rx->fb);
    delete rx; // (no lock held: the last reference frees the context, its mutex included)
}

extern "C" int sdrhip_rx_frames_view(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes, size_t *n_frames)
{
    if (!rx || !base || !stream_stride_bytes || !n_frames) return fail(SDRHIP_EINVAL, "rx_frames_view: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    if (!rx->view.uniform()) return fail(SDRHIP_EINVAL, "rx_frames_view: the last call's windows differ between streams: use sdrhip_rx_frames_view_ragged");
    *base = rx->view.window(0, rx_frame_bytes(rx));
    *stream_stride_bytes = rx->view.stride();
    *n_frames = rx->view.frames(0);
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_frames_view_ragged(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes, size_t *first_slot,
                                            size_t *n_frames)
{
    if (!rx || !base || !stream_stride_bytes || !first_slot || !n_frames) return fail(SDRHIP_EINVAL, "rx_frames_view_ragged: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    *base = rx->view.base();
    *stream_stride_bytes = rx->view.stride();
    for (size_t s = 0; s < (size_t)rx->nstreams; ++s) { first_slot[s] = rx->view.first(s); n_frames[s] = rx->view.frames(s); }
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
    size_t now = 0; // (the stream that completes the most: every stream, while they stand at the same position)
    for (size_t s = 0; s < (size_t)rx->nstreams; ++s) {
        const size_t f = rx->area.advance(s, n_in >> rx->cfg.log2decim).done;
        if (f > now) now = f;
    }
    if (!rx->pipelined) return now;
    return rx->late.have && rx->late.frames > now ? rx->late.frames : now; // (a pipelined call delivers the previous call's frames)
}

// delivery of a finished window: optional copy to the caller's buffer, and the zero-copy view
static int rx_deliver(sdrhip_rx *rx, const uint8_t *area, size_t first, size_t stride, size_t frames, size_t frame_bytes, uint8_t *frames_out,
                      size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    const uint8_t *base = area + first * frame_bytes; // the window of stream 0
    if (frames && frames_out) {
        if (S > 1 && frame_stride_bytes < frames * frame_bytes) return fail(SDRHIP_EINVAL, "rx_process: frame stride too small");
        HIP_TRY(link_copy2d(c, frames_out, S > 1 ? frame_stride_bytes : frames * frame_bytes, base, stride, frames * frame_bytes, S,
                            mem == SDRHIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    } else if (frames && mem != SDRHIP_MEM_DEVICE) {
        return fail(SDRHIP_EINVAL, "rx_process: NULL frames_out");
    }
    rx->view.set(area, stride, (size_t)S, first, frames);
    if (n_frames) *n_frames = frames;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_flush(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (n_frames) *n_frames = 0;
    if (int e = check_mem(mem)) return e;
    if (!rx->late.have) { rx->view.clear(); return SDRHIP_OK; }
    HIP_TRY(hipSetDevice(rx->ctx->device));
    int rc;
    if ((rc = rx_settle(rx))) return rc;
    if ((rc = rx_deliver(rx, rx->late.area, rx->late.first, rx->late.stride, rx->late.frames, rx->late.frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
    rx->late.have = false;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(rx->ctx->stream));
    return SDRHIP_OK;
}

// the shared record of the bank-wide values (rx_meta_record: rx_stream_settings.h), with the bank-wide decimated sample size
static void rx_meta_base(const sdrhip_rx_config &cfg, unsigned w[6])
{
    rx_meta_record(cfg.center_frequency_khz, cfg.sample_rate, cfg.nb_fec, decimated_sample_size((unsigned)cfg.log2decim, cfg.sample_bits), w);
}

// ---- the per-stream setters and getters (rx->streams: rx_stream_settings.h).  A setter: the lock, its own refusals, then the
// type -- range, room, values, version; whatever fails, the old values stand.  A getter: the lock, the stream, then the type
static int rx_set_done(const RxSetResult &r, const char *who, const char *what, const char *range)
{
    if (r.kind == RxSetResult::RANGE) return fail(SDRHIP_EINVAL, "%s: %s[%zu] = %ld, must be %s", who, what, r.index, r.value, range);
    return r.kind == RxSetResult::NO_MEMORY ? fail(SDRHIP_ENOMEM, "out of host memory") : SDRHIP_OK;
}
static int rx_check_stream(const sdrhip_rx *rx, int stream, const char *who)
{
    return stream < 0 || stream >= rx->nstreams ? fail(SDRHIP_EINVAL, "%s: stream %d of %d", who, stream, rx->nstreams) : SDRHIP_OK;
}

// per-stream centre frequency / sample rate (UDPSink.h:93-96: every sdrdaemonrx sets them on its own sink)
extern "C" int sdrhip_rx_set_stream_meta(sdrhip_rx *rx, const uint32_t *center_frequency_khz, const uint32_t *sample_rate)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    // (host arrays alone: the next launch takes them, nothing is enqueued and nothing waited for here)
    return rx_set_done(rx->streams.set_meta(center_frequency_khz, sample_rate), "rx_set_stream_meta", "", "");
}

// ---- outgoing meta from the incoming meta blocks: the flag alone (the datagram entries read it per call / per submit)
extern "C" int sdrhip_rx_set_follow_meta(sdrhip_rx *rx, int on)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    rx->follow_meta = on ? 1 : 0;
    return SDRHIP_OK;
}

// ---- the sample size from the incoming meta blocks: the flag alone, the twin of the one above and independent of it
extern "C" int sdrhip_rx_set_follow_bits(sdrhip_rx *rx, int on)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    rx->follow_bits = on ? 1 : 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_get_stream_meta(const sdrhip_rx *rx, int stream, uint32_t *center_frequency_khz, uint32_t *sample_rate)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (int e = rx_check_stream(rx, stream, "rx_get_stream_meta")) return e;
    if (center_frequency_khz) *center_frequency_khz = rx->streams.fc(rx_bank(rx), (size_t)stream);
    if (sample_rate) *sample_rate = rx->streams.rate(rx_bank(rx), (size_t)stream);
    return SDRHIP_OK;
}

// per-stream fecblk (sdrdaemonrx.cpp:599-605: every sdrdaemonrx sets UDPSink::setNbBlocksFEC on its own sink)
extern "C" int sdrhip_rx_set_stream_fec(sdrhip_rx *rx, const int *nb_fec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    // ---- everything that can be refused, before anything changes
    if (rx->pipelined || rx->late.have) return fail(SDRHIP_EINVAL, "rx_set_stream_fec: not available in pipelined mode");
    if (rx_batches_active(rx)) return fail(SDRHIP_EINVAL, "rx_set_stream_fec: asynchronous batches are being filled or in flight: collect them first");
    if (rx->ring.busy()) return fail(SDRHIP_EINVAL, "rx_set_stream_fec: a batch is lent (sdrhip_rx_collect_egress): sdrhip_rx_release_egress it first");
    if (int rc = rx_set_done(rx->streams.admit_fec(nb_fec), "rx_set_stream_fec", "nb_fec", "0..128")) return rc;
    HIP_TRY(hipSetDevice(rx->ctx->device));
    // the slot pitch follows the largest count: a change moves the open frames like a fecblk change of sdrhip_rx_reconfigure
    if (int rc = rx_repitch(rx, rx->streams.slot_blocks_of(nb_fec, rx_bank(rx)) * SDRHIP_UDPSIZE, "rx_set_stream_fec")) return rc;
    return rx_set_done(rx->streams.set_fec(nb_fec), "rx_set_stream_fec", "nb_fec", "0..128"); // (behind admit_fec: cannot fail)
}

extern "C" int sdrhip_rx_get_stream_fec(const sdrhip_rx *rx, int stream, int *nb_fec, int *slot_blocks)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (int e = rx_check_stream(rx, stream, "rx_get_stream_fec")) return e;
    if (nb_fec) *nb_fec = rx_fec_of(rx, (size_t)stream);
    if (slot_blocks) *slot_blocks = (int)(rx_frame_bytes(rx) / SDRHIP_UDPSIZE);
    return SDRHIP_OK;
}

// per-stream sample size (sdrdaemonrx.cpp:619-623, 639-643: every sdrdaemonrx hands its own source's get_sample_bits() to its
// Downsampler and, decimated, to UDPSink::setSampleBits / setSampleBytes).  Host arrays alone, like sdrhip_rx_set_stream_meta
extern "C" int sdrhip_rx_set_stream_bits(sdrhip_rx *rx, const unsigned *sample_bits)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (rx->pipelined || rx->late.have) return fail(SDRHIP_EINVAL, "rx_set_stream_bits: not available in pipelined mode");
    return rx_set_done(rx->streams.set_bits(sample_bits), "rx_set_stream_bits", "sample_bits", "1..16");
}

extern "C" int sdrhip_rx_get_stream_bits(const sdrhip_rx *rx, int stream, unsigned *sample_bits, unsigned *frame_bits)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (int e = rx_check_stream(rx, stream, "rx_get_stream_bits")) return e;
    const unsigned b = rx_bits_of(rx, (size_t)stream);
    if (sample_bits) *sample_bits = b;
    if (frame_bits) *frame_bits = decimated_sample_size((unsigned)rx->cfg.log2decim, b);
    return SDRHIP_OK;
}

// per-stream input format (RtlSdrSource.cpp:542-553, HackRFSource.cpp:661-674: the format is the source object's, and
// sdrdaemonrx.cpp:264-374 picks one source per process).  Host array alone; a batch has ONE set of formats: the rule of
// sdrhip_rx_set_input_format
extern "C" int sdrhip_rx_set_stream_format(sdrhip_rx *rx, const int *fmt)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (rx->pipelined || rx->late.have) return fail(SDRHIP_EINVAL, "rx_set_stream_format: not available in pipelined mode");
    if (rx->ring.busy()) return fail(SDRHIP_EINVAL, "rx_set_stream_format: asynchronous batches are being filled or in flight: collect them first");
    return rx_set_done(rx->streams.set_format(fmt), "rx_set_stream_format", "fmt", "SDRHIP_IQ_S16, SDRHIP_IQ_U8 or SDRHIP_IQ_S8");
}

extern "C" int sdrhip_rx_get_stream_format(const sdrhip_rx *rx, int stream, int *fmt)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (int e = rx_check_stream(rx, stream, "rx_get_stream_format")) return e;
    if (fmt) *fmt = rx->streams.format(rx->in_fmt, (size_t)stream);
    return SDRHIP_OK;
}

// the streams' records on the device, for a uniform launch (*dev = NULL: no array is set, the shared record serves every stream).
// A new version is copied in front of the launch on the context's stream: from a pinned buffer of its own (four rotate; reuse
// waits for that buffer's own upload, four versions back) into the device table that the previous version does not occupy, so
// that a deferred encode keeps reading the one it was given
static int rx_stream_table(sdrhip_rx *rx, const unsigned **dev)
{
    *dev = nullptr;
    const RxStreamRecords *r = rx->streams.records(rx_bank(rx));
    if (!r) return SDRHIP_OK;
    if (rx->streams.changed()) {
        const void *tab = nullptr;
        if (int rc = rx->sm_tab.upload(rx->ctx->stream, r->words.data(), r->words.size() * sizeof(unsigned), &tab)) return rc;
        rx->streams.taken();
    }
    *dev = static_cast<const unsigned *>(rx->sm_tab.current());
    return SDRHIP_OK;
}

// host input of the uniform step: S rows of n_in samples of esz bytes -> [S][dstride] rows the first kernel reads.  A small call
// skips the copy engine: the kernel reads pinned host memory over the link itself, and the buffer is free again when the call
// returns (host-pointer calls end with a stream synchronisation); a large one goes to c->in in one 2-D copy
static int rx_stage_in(sdrhip_ctx *c, const void *src, size_t in_stride, size_t n_in, int S, size_t esz, size_t dstride, const void **out)
{
    int rc;
    if ((size_t)S * dstride * esz <= SDRHIP_ZEROCOPY_MAX) {
        if ((rc = c->zin.reserve((size_t)S * dstride * esz + 16))) return rc;
        for (int s = 0; s < S; ++s) memcpy(c->zin.as<char>() + (size_t)s * dstride * esz, static_cast<const char *>(src) + (size_t)s * in_stride * esz, n_in * esz);
        link_bytes(c, hipMemcpyHostToDevice, (size_t)S * n_in * esz); // (read by the kernel over the link)
        *out = c->zin.p;
    } else {
        if ((rc = c->in.reserve((size_t)S * dstride * esz + 16))) return rc;
        HIP_TRY(link_copy2d(c, c->in.p, dstride * esz, src, in_stride * esz, n_in * esz, S, hipMemcpyHostToDevice, c->stream));
        *out = c->in.p;
    }
    return SDRHIP_OK;
}

// ---- the uniform step: refuse, input, window and table, decimate and frame, encode, deliver and commit.  What the call launches is
// rx_step_plan.h's answer (asked once, behind rx_make_room); RxStep / RxRagged hold what the phases of a step share
namespace {
struct RxStep {
    sdrhip_rx *rx; sdrhip_ctx *c; int S;
    size_t n_in, n_dec, frame_bytes; RxAdvance adv;
    std::vector<size_t> dones;                      // every stream completes adv.done frames
    RxStepIn in; RxStepPlan plan;
    const int16_t *din; size_t dstride;             // the decimator's input rows
    size_t cap, slot0, stream_bytes; uint8_t *work; // the area, and slot 0 of the window
    RxMeta meta;                                    // meta record of the frames started by this call (UDPSinkFEC.cpp:87-132)
    const unsigned *lin; size_t lstride;            // stream-order rows (plan.use_lin: the encoder lays frames out from them)
    FrameArgs fa;                                   // K2's arguments (plan.k2_in_encoder: they ride in the encoder's launch)
    Enc128Args k;                                   // the structured encode of this call's frames, now or deferred
    int input(const int16_t *iq_in, size_t in_stride, int mem), window(uint32_t tv_sec, uint32_t tv_usec), decimate(), encode();
    int deliver(uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem);
};
struct RxRagged {
    sdrhip_rx *rx; sdrhip_ctx *c; int S, L;
    const RxRaggedCounts &n; const RxRaggedCall &call;
    RxRaggedInput route;                  // what stands between the caller's rows and the decimator
    size_t FB, frame_bytes, stream_bytes; uint8_t *area; // (per-stream fecblk: FB = the slot pitch, 128 + the largest count)
    std::vector<unsigned> ss;             // each stream's own sample size: sdrhip_rx_set_stream_bits, else the bank's
    unsigned mw[6];                       // the shared record with a zero stamp (stamps, fc, rate and CRC go per row)
    const RxStreamRecords *sw;            // NULL: no array is set, mw serves every stream
    std::vector<RaggedRow> rows; const RaggedRow *rdev; RaggedPlan plan; // the per-call table, its upload, the decimator's plan for it
    const int16_t *din; size_t dstride;   // the decimator's input rows
    int table(const uint32_t *tv_sec, const uint32_t *tv_usec), input(const int16_t *iq_in, size_t in_stride), decimate(), encode();
    int deliver(const RxFramesOut &out);
};
} // namespace

// input: host rows are staged; 8-bit input crosses the link as 2 bytes per sample (rows of a multiple of 8 samples: K0's 16-byte
// loads) and K0 widens it into rx->wide, which the decimator reads as it reads int16 input
int RxStep::input(const int16_t *iq_in, size_t in_stride, int mem)
{
    const bool wide8 = rx->in_fmt != IQF_S16;
    const void *src = iq_in;
    size_t sstride = in_stride;
    int rc;
    if ((rc = check_mem(mem))) return rc;
    if (mem == SDRHIP_MEM_HOST) {
        sstride = wide8 ? (n_in + 7) & ~(size_t)7 : (n_in + 3) & ~(size_t)3;
        if ((rc = rx_stage_in(c, iq_in, in_stride, n_in, S, wide8 ? 2 : 4, sstride, &src))) return rc;
    } else if (!aligned16(iq_in) || (S > 1 && (in_stride & (wide8 ? 7 : 3)))) {
        return wide8 ? fail(SDRHIP_EALIGN, "rx_process: 8-bit device input must be 16-byte aligned, its stride a multiple of 8 samples")
                     : fail(SDRHIP_EALIGN, "rx_process: device input must be 16-byte aligned");
    }
    din = static_cast<const int16_t *>(src);
    dstride = wide8 ? (n_in + 3) & ~(size_t)3 : sstride;
    return wide8 ? rx_widen(rx, static_cast<const uint8_t *>(src), sstride, n_in, dstride, &din) : SDRHIP_OK;
}

// window, plan and table.  Work area [stream][slot][128 + R][512]: this call fills slots slot .. slot + done.  The finished frames
// stay readable in place until the next call (sdrhip_rx_frames_view); the frame still being filled is the first slot of the next
// call.  At the end of the area the window wraps: the open frame moves to slot 0 (one strided copy every few calls instead of a
// save + restore per call).  Frames that wait for delivery (pipelined mode) are never overwritten: a window that would reach them
// gets a new area.  The decimator kernel writes the meta blocks and super block headers of the frames it starts on its way
int RxStep::window(uint32_t tv_sec, uint32_t tv_usec)
{
    int rc;
    if ((rc = rx_release_old(rx))) return rc;
    if ((rc = rx_make_room(rx, dones.data(), in.pipelined, "rx_process"))) return rc;
    cap = rx->area.cap(); slot0 = rx->area.slot(0); stream_bytes = in.stream_bytes = cap * frame_bytes;
    work = rx->work.as<uint8_t>() + slot0 * frame_bytes;
    in.mfma_applies = decimate_mfma_applies(rx->dec, in.L, in.fcpos, n_in);
    plan = rx_step_plan(in, frame_bytes);
    memset(&meta, 0, sizeof(meta));
    if (adv.started <= 0) return SDRHIP_OK;
    rx_meta_base(rx->cfg, meta.w);
    if ((rc = rx_stream_table(rx, &meta.tab))) return rc;
    meta.w[3] = tv_sec; meta.w[4] = tv_usec; // (the stamp of the call's first sample)
    meta.first = adv.first_new; meta.count = adv.started; meta.frame_count0 = adv.frame_count0;
    meta.idx0 = adv.idx0; meta.rate = rx->cfg.sample_rate;
    return SDRHIP_OK;
}

// decimate and frame, by the plan's route: straight into the frame layout, or in stream order, and K2 lays the samples out as super
// blocks (+ meta blocks and headers) -- now, unless it rides in the encoder's launch
int RxStep::decimate()
{
    const RxStepPlan &p = plan;
    const int L = in.L, FB = SDRHIP_NB_ORIGINAL + in.R;
    unsigned ss = rx->cfg.sample_bits;
    size_t n_out = 0;
    int rc;
    if (!p.stream_order()) {
        if ((rc = decimate_device(rx->dec, L, in.fcpos, &ss, din, n_in, dstride, reinterpret_cast<int16_t *>(work), stream_bytes / 4, &n_out, 1, FB, in.pending, &meta))) return rc;
        rx->consumed = true;
        return rx_settle(rx); // (a waiting encode: this launch takes none along)
    }
    lstride = (n_dec + 3) & ~(size_t)3;
    const size_t bytes = (size_t)S * lstride * 4 + 16;
    if (p.flip_lin) rx->lin_sel ^= 1;
    DevBuf &rows = rx->lin[rx->lin_sel];
    const Enc128Args *fuse = p.fuse ? &rx->late.k : nullptr;
    bool fused = false;
    // (rows that grow: the waiting encode goes out first, on its own, and the stream drains before the old rows are freed)
    if (rows.cap < bytes && rx->late.encode) { if ((rc = rx_settle(rx))) return rc; fuse = nullptr; HIP_TRY(hipStreamSynchronize(c->stream)); }
    if ((rc = rows.reserve(bytes))) return rc;
    if ((rc = decimate_device(rx->dec, L, in.fcpos, &ss, din, n_in, dstride, rows.as<int16_t>(), lstride, &n_out, 0, 0, 0, nullptr, fuse, &fused, p.coresident))) return rc;
    rx->consumed = true;
    if (fused) rx->late.encode = false;
    lin = rows.as<unsigned>();
    fa.skip_from = p.skip_from; fa.skip_to = p.skip_to;
    fa.in = lin; fa.out = reinterpret_cast<unsigned *>(work); fa.in_stride = lstride; fa.out_stride = stream_bytes / 4;
    fa.n = n_dec; fa.frame_sample_base = in.pending; fa.frame_blocks = FB;
    set_meta_args(fa, meta);
    if (!p.k2_in_encoder) {
        hipError_t e = launch_frame_pack(fa, S, c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "frame pack launch: %s", hipGetErrorString(e));
    }
    return rx_settle(rx); // (a waiting encode that this call's launch could not take along)
}

// FEC over the completed frames of every stream, recovery blocks land behind block 127.  The structured encoder (one workgroup per
// (frame, half block); frame (s, f) of the window is frame s * cap + f) reads and writes whole dwords:
static_assert(SDRHIP_UDPSIZE % 4 == 0, "gf_encode128_kernel: a frame of (128 + R) super blocks is a whole number of dwords");
int RxStep::encode()
{
    const RxStepPlan &p = plan;
    const size_t done = in.done, frames = (size_t)S * cap;
    uint8_t *rec = work + (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE;
    int rc;
    if (p.encoder == RX_ENC_NONE) return SDRHIP_OK;
    if (p.encoder == RX_ENC_GENERIC) {
        // generic matrix kernel: one launch for every stream, frame list in groups of GF_FRAMES_PER_GROUP
        if (rx->flist_done != done || rx->flist_cap != cap) {
            HIP_TRY(hipStreamSynchronize(c->stream)); // a previous upload may still read flist_host
            rx->flist_host.clear();
            for (int s = 0; s < S; ++s)
                for (size_t f = 0; f < done; ++f) rx->flist_host.push_back((int32_t)(s * cap + f));
            while (rx->flist_host.size() % GF_FRAMES_PER_GROUP) rx->flist_host.push_back(-1);
            if ((rc = rx->flist.reserve(rx->flist_host.size() * 4))) return rc;
            HIP_TRY(link_copy(c, rx->flist.p, rx->flist_host.data(), rx->flist_host.size() * 4, hipMemcpyHostToDevice, c->stream));
            rx->flist_done = done; rx->flist_cap = cap;
        }
        return fec_encode_device(c, work, frame_bytes, frames, in.R, rec, frame_bytes, rx->flist.as<int32_t>(), (int)(rx->flist_host.size() / GF_FRAMES_PER_GROUP), nullptr);
    }
    k.in = work; k.out = rec; k.tab = c->gf_tab; k.leaf_tables = c->enc_leaves; k.fft_tables = c->enc_fft; k.use_fft = c->opt.enc_fft;
    k.bitslice = c->opt.enc_bitslice; k.in_frame_bytes = frame_bytes; k.out_frame_bytes = frame_bytes;
    k.rows = in.R; k.nframes = (int)frames;
    k.nlist = (int)((size_t)S * done); k.gen_done = (int)done; k.gen_cap = (int)cap;
    if (p.use_lin) { k.lin = lin; k.lin_stride = lstride; k.lin_cap = (int)cap; k.lin_first = p.lin_first; k.lin_pending = (int)p.lin_pending; }
    if (p.encoder == RX_ENC_DEFERRED) return SDRHIP_OK; // rides in the next call's decimator launch (or sdrhip_rx_flush)
    if (!p.k2_in_encoder) return fec_encode128_launch(c, k);
    set_meta_args(k, meta); // (encoder + K2 in one launch: the encoder derives the meta blocks of the frames this call starts itself)
    k.lin_straddle = p.lin_straddle ? 1 : 0;
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_FEC_ENCODE);
        e = launch_gf_encode128_pack(k, fa, S, c->stream);
    }
    return e == hipSuccess ? SDRHIP_OK : fail(SDRHIP_EDEVICE, "encode + frame pack launch: %s", hipGetErrorString(e));
}

// delivery: this call's frames, or (pipelined) the previous call's, whose encode went out above; then every stream moves on
// together, and the frame still being filled opens the next call's window
int RxStep::deliver(uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    sdrhip_rx::Late &late = rx->late;
    const size_t done = in.done;
    int rc;
    if (!in.pipelined) {
        if ((rc = rx_deliver(rx, rx->work.as<uint8_t>(), slot0, stream_bytes, done, frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
    } else {
        if (!late.have) rx->view.clear();
        else if ((rc = rx_deliver(rx, late.area, late.first, late.stride, late.frames, late.frame_bytes, frames_out, frame_stride_bytes, n_frames, mem))) return rc;
        late.have = done > 0; late.encode = plan.encoder == RX_ENC_DEFERRED;
        if (plan.record_framed) { // (everything the deferred encode reads has been enqueued on the first stream by now)
            if ((rc = rx->ev_framed.ensure())) return rc;
            HIP_TRY(hipEventRecord(rx->ev_framed, c->stream));
        }
        late.k = k;
        late.area = rx->work.as<uint8_t>(); late.first = slot0; late.in_old = false;
        late.stride = stream_bytes; late.frames = done; late.frame_bytes = frame_bytes;
    }
    rx->area.commit(dones.data(), std::vector<uint64_t>(dones.size(), adv.rest).data());
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_process(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec, uint32_t tv_usec,
                                 uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (n_frames) *n_frames = 0;
    if (int e = rx_refuse_uniform("rx_process", "sdrhip_rx_process_ragged", rx->streams.forces_ragged())) return e;
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_process: ragged batches are being filled or in flight: collect them first");
    if (rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_process: asynchronous datagram batches are in flight: collect them first");
    if (n_in && !rx->area.aligned()) {
        // ragged calls left the streams at different frame positions: a ragged call with equal counts and stamps; *n_frames = the
        // largest per-stream count (sdrhip_rx_frames_view_ragged has each)
        const size_t S = (size_t)rx->nstreams;
        std::vector<size_t> cnt(S, n_in), nf(S, 0);
        std::vector<uint32_t> sec(S, tv_sec), usec(S, tv_usec);
        const RxFramesOut out = {frames_out, frame_stride_bytes, nf.data(), mem};
        const int rc = rx_ragged(rx, iq_in, rx_counts(rx, cnt.data()), in_stride, sec.data(), usec.data(), out);
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
        rx->view.clear(); return SDRHIP_OK;
    }
    if (!iq_in) return fail(SDRHIP_EINVAL, "rx_process: NULL input");
    rx->consumed = false;
    HIP_TRY(hipSetDevice(rx->ctx->device));
    const int S = rx->nstreams;
    RxStep st;
    st.rx = rx; st.c = rx->ctx; st.S = S;
    st.n_in = n_in; st.n_dec = n_in >> rx->cfg.log2decim; st.frame_bytes = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
    st.adv = rx->area.advance(0, st.n_dec); st.in = rx_step_inputs(rx);
    st.in.pending = rx->area.pending(0); st.in.done = st.adv.done; // (every stream stands here: aligned)
    st.lin = nullptr; st.lstride = 0;
    memset(&st.fa, 0, sizeof(st.fa)); memset(&st.k, 0, sizeof(st.k));
    if (S == 1) in_stride = n_in;
    // ---- everything that can be refused is refused before anything is consumed
    const RxStepDelivery d = rx_step_delivery(st.in, st.frame_bytes);
    if (d.frames && !frames_out && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "rx_process: NULL frames_out");
    if (frames_out && S > 1 && d.frames && frame_stride_bytes < d.frames * d.frame_bytes) return fail(SDRHIP_EINVAL, "rx_process: frame stride too small");
    int rc;
    if ((rc = st.input(iq_in, in_stride, mem))) return rc;
    st.dones.assign((size_t)S, st.adv.done);
    if ((rc = st.window(tv_sec, tv_usec))) return rc;
    if ((rc = st.decimate())) return rc;
    if ((rc = st.encode())) return rc;
    return st.deliver(frames_out, frame_stride_bytes, n_frames, mem);
}

// --------------------------------------------------------------------------- ragged Rx calls
int sdrhip::rx_area_room(sdrhip_rx *rx, const size_t *done)
{
    return rx_make_room(rx, done ? done : std::vector<size_t>(rx->area.streams(), 0).data(), false, "rx_process_ragged", true);
}

int sdrhip::rx_ragged_room(sdrhip_rx *rx, const RxRaggedCounts &n, RxTabs *tabs)
{
    const int S = rx->nstreams, L = rx->cfg.log2decim;
    int rc;
    if ((rc = rx_area_room(rx, n.done.data()))) return rc;
    if ((rc = ragged_reserve(rx->dec, tabs ? &tabs->rows : nullptr))) return rc;
    // (the stream-order rows, unless the decimator's plan for these counts stores straight into the windows: the step's own rule)
    std::vector<RaggedRow> rows((size_t)S);
    RaggedPlan plan;
    if ((rc = ragged_plan(rx->dec, L, rx->cfg.fcpos, n.n_in, rows.data(), &plan))) return rc;
    if (!rx_stores_direct(rx, plan.mfma) && (rc = rx->lin[0].reserve((size_t)S * ((n.max_dec + 3) & ~(size_t)3) * 4 + 16))) return rc;
    if (n.sum_done && rx_fec_max(rx) > 0) {
        const size_t nl = rx_flist_entries(n.sum_done);
        if ((rc = (tabs ? tabs->flist : rx->r_flist_pin).reserve(nl * 4))) return rc;
        if ((rc = rx->r_flist.reserve(nl * 4))) return rc;
    }
    return SDRHIP_OK;
}

void sdrhip::rx_pack_rows(char *dst, const void *src, size_t pitch, const size_t *n_in, const int *fmts, int bank_fmt, size_t S)
{
    const char *rows = static_cast<const char *>(src), *packed = rows;
    for (size_t s = 0; s < S; ++s) {
        const size_t bytes = n_in[s] * unpackx_sample_bytes(fmts ? fmts[s] : bank_fmt);
        if (bytes) memcpy(dst, pitch ? rows + s * pitch : packed, bytes);
        dst += bytes;
        packed += bytes;
    }
}

int sdrhip::rx_unpack_launch(sdrhip_rx *rx, PinnedBuf &pin, DevBuf &dev, size_t tab_bytes, const int *fmts, const void *src, int16_t *out,
                             size_t dstride, unsigned grid)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    HIP_TRY(hipMemcpyAsync(dev.p, pin.p, tab_bytes, hipMemcpyHostToDevice, c->stream)); // (not counted: a table)
    pin.mark(c->stream);
    const UnpackXRow *rows = dev.as<UnpackXRow>();
    const UnpackXSeg *segs = reinterpret_cast<const UnpackXSeg *>(rows + S + 1);
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_CONVERT);
        e = fmts ? launch_unpack_mixed(src, out, dstride, rows, segs, S, grid, c->stream)
                 : launch_unpack_packed(rx->in_fmt, static_cast<const uint8_t *>(src), out, dstride, rows, segs, S, grid, c->stream);
    }
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "unpack launch: %s", hipGetErrorString(e));
    return SDRHIP_OK;
}

// per-stream input format, the synchronous call: ONE K0x launch with one segment per stream lays the rows out as [S][*dstride] int16
// in rx->wide.  Host rows are staged packed -- n_in[s] * bytes(fmt[s]) per row, back to back -- and go up in one copy of exactly
// those bytes; device rows are read in place (row s at byte 4 * s * in_stride), nothing outside a row's own bytes
static int rx_unpack_rows(sdrhip_rx *rx, const int16_t *iq_in, size_t in_stride, const size_t *n_in, const int *fmts, bool in_dev,
                          const int16_t **din, size_t *dstride)
{
    sdrhip_ctx *c = rx->ctx;
    const size_t S = (size_t)rx->nstreams;
    const UnpackXPlan m = unpackx_measure(n_in, 1, S, fmts);
    size_t max_in = 0;
    for (size_t s = 0; s < S; ++s) if (n_in[s] > max_in) max_in = n_in[s];
    const size_t rows_bytes = (S + 1) * sizeof(UnpackXRow), tab_bytes = rows_bytes + (size_t)m.nseg * sizeof(UnpackXSeg);
    const size_t ds = (max_in + 7) & ~(size_t)7;
    int rc;
    if ((rc = rx->f_tab_pin.reserve(tab_bytes))) return rc; // (waits for the upload of the previous call's table)
    if ((rc = reserve_settled(c, rx->f_tab, tab_bytes))) return rc;
    if ((rc = rx->wide.reserve(S * ds * 4 + 16))) return rc;
    const void *src = iq_in;
    if (!in_dev) {
        if ((rc = rx->f_pin.reserve((size_t)m.bytes))) return rc; // (waits for the previous call's upload)
        if ((rc = reserve_settled(c, rx->f_pk, (size_t)m.bytes + 64))) return rc;
        rx_pack_rows(rx->f_pin.as<char>(), iq_in, in_stride * 4, n_in, fmts, 0, S);
        HIP_TRY(link_copy(c, rx->f_pk.p, rx->f_pin.p, (size_t)m.bytes, hipMemcpyHostToDevice, c->stream));
        rx->f_pin.mark(c->stream);
        src = rx->f_pk.p;
    }
    if (!unpackx_fill(n_in, 1, S, fmts, in_dev ? 2 * (uint64_t)in_stride : 0, rx->f_tab_pin.as<UnpackXRow>(),
                      reinterpret_cast<UnpackXSeg *>(rx->f_tab_pin.as<char>() + rows_bytes)).fits)
        return fail(SDRHIP_EINVAL, "rx_process_ragged: too many samples for one launch");
    if ((rc = rx_unpack_launch(rx, rx->f_tab_pin, rx->f_tab, tab_bytes, fmts, src, rx->wide.as<int16_t>(), ds, (unsigned)m.grid))) return rc;
    *din = rx->wide.as<int16_t>();
    *dstride = ds;
    return SDRHIP_OK;
}

// ---- the ragged step: every stream takes its own count.  K0x / K0r (input) -> K1mr straight into each stream's window, or K1r /
// the filter-less kernel into stream order and K2r into the windows -> the encoder over the list of every stream's completed
// frames; which of these run is rx_step_plan.h's answer.  The per-call table first: counts (decimator), windows and meta records
// (K2r); then the kernels that rewrite rows of it on the device
int RxRagged::table(const uint32_t *tv_sec, const uint32_t *tv_usec)
{
    const RxFrameArea &A = rx->area;
    memset(rows.data(), 0, rows.size() * sizeof(RaggedRow));
    for (size_t s = 0; s < (size_t)S; ++s) {
        RaggedRow &r = rows[s];
        const RxAdvance &a = n.adv[s];
        ss[s] = rx_bits_of(rx, s);
        r.out_off = A.slot(s) * frame_bytes / 4; r.frame_sample_base = A.pending(s);
        const unsigned *t = sw ? &sw->words[s * STREAM_META_WORDS] : nullptr;
        r.fc = t ? t[0] : mw[0]; r.rate = t ? t[1] : mw[1]; r.crc0 = t ? t[2] : mw[5];
        r.w2 = sw ? sw->w2[s] : mw[2];
        r.shifts = sw ? sw->shifts[s] : ragged_shift_word((unsigned)L, ss[s]);
        if (a.started > 0 && (n.n_in[s] >> L)) {
            r.meta_first = a.first_new; r.meta_count = a.started; r.frame_count0 = a.frame_count0; r.meta_idx0 = a.idx0;
            r.tv_sec = tv_sec[s]; r.tv_usec = tv_usec[s];
        }
    }
    if (int rc = ragged_prepare(rx->dec, L, rx->cfg.fcpos, n.n_in, rows.data(), &rdev, &plan, call.tabs ? &call.tabs->rows : nullptr)) return rc;
    hipError_t e = hipSuccess;
    // KFb, in front of KF (which runs its CRC over the row's third word): the streams that have an incoming sample size get the
    // shift pair, sampleBytes / sampleBits and the CRC from the collector's committed m_outputMeta, in the device table, behind its
    // upload and in front of every kernel that reads a row.  (The host's rows, `ss` and `mw` stay the host's values: every ragged
    // decimator launch takes the pair from the device row, and K2r the third word)
    if (call.follow_bits) e = launch_rx_follow_bits(call.follow_bits, const_cast<RaggedRow *>(rdev), L, S, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "follow bits launch: %s", hipGetErrorString(e));
    // KF: the streams that have incoming meta get {fc, rate >> L, CRC} from the collector's committed m_outputMeta, in the device
    // table (over the row's own third word), behind its upload and in front of K2r, the one kernel that reads a row's words (the
    // host's rows, `mw` and the rate handed to the decimator launch stay the configuration's)
    if (call.follow) e = launch_rx_follow_meta(call.follow, const_cast<RaggedRow *>(rdev), L, S, c->stream);
    return e == hipSuccess ? SDRHIP_OK : fail(SDRHIP_EDEVICE, "follow meta launch: %s", hipGetErrorString(e));
}

// input: per-stream formats through K0x, host rows staged stream by stream (n_in[s] samples each), 8-bit rows widened by K0r
int RxRagged::input(const int16_t *iq_in, size_t in_stride)
{
    const size_t max_in = n.max_in;
    const bool wide8 = route.widen;
    const void *src = iq_in;
    int rc;
    din = iq_in; dstride = in_stride;
    if (route.unpack) return rx_unpack_rows(rx, iq_in, in_stride, n.n_in, rx->streams.formats(), route.in_dev, &din, &dstride);
    if (route.stage) {
        dstride = wide8 ? (max_in + 7) & ~(size_t)7 : (max_in + 3) & ~(size_t)3;
        if ((rc = ragged_stage_in(c, rx->r_pin, c->in, iq_in, in_stride, n.n_in, S, wide8 ? 2 : 4, dstride, &src))) return rc;
        din = static_cast<const int16_t *>(src);
    }
    if (!wide8) return SDRHIP_OK;
    const size_t sstride = dstride;
    dstride = (max_in + 3) & ~(size_t)3;
    if ((rc = rx->wide.reserve((size_t)S * dstride * 4 + 16))) return rc;
    hipError_t e;
    {
        KTimer kt(c, SDRHIP_K_CONVERT);
        e = launch_iq8_widen_ragged(rx->in_fmt, static_cast<const uint8_t *>(src), sstride, rx->wide.as<int16_t>(), dstride, max_in, S, rdev, c->stream);
    }
    din = rx->wide.as<int16_t>();
    return e == hipSuccess ? SDRHIP_OK : fail(SDRHIP_EDEVICE, "widen launch: %s", hipGetErrorString(e));
}

// decimate and frame: K1mr straight into each stream's window, its VALU pieces write the meta blocks; otherwise stream order + K2r
int RxRagged::decimate()
{
    const bool direct = rx_stores_direct(rx, plan.mfma);
    const size_t lstride = (n.max_dec + 3) & ~(size_t)3;
    DevBuf &lin = rx->lin[0];
    int rc;
    if (direct) {
        rc = decimate_ragged_device(rx->dec, L, rx->cfg.fcpos, ss.data(), din, dstride, reinterpret_cast<int16_t *>(area), stream_bytes / 4, rows.data(), rdev, plan, 1,
                                    (int)FB, mw, rx->cfg.sample_rate);
    } else {
        if ((rc = lin.reserve((size_t)S * lstride * 4 + 16))) return rc;
        rc = decimate_ragged_device(rx->dec, L, rx->cfg.fcpos, ss.data(), din, dstride, lin.as<int16_t>(), lstride, rows.data(), rdev, plan);
    }
    if (rc) return rc;
    rx->consumed = true;
    const RxK2rJob job = rx_ragged_k2r(n.max_dec != 0, direct, sw != nullptr, call.follow != nullptr, call.follow_bits != nullptr);
    if (job == RX_K2R_NONE) return SDRHIP_OK;
    FrameArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.in = lin.as<unsigned>(); fa.out = reinterpret_cast<unsigned *>(area); fa.in_stride = lstride; fa.out_stride = stream_bytes / 4;
    fa.n = n.max_dec; fa.frame_blocks = (int)FB;
    memcpy(fa.meta_w, mw, sizeof(fa.meta_w)); fa.meta_rate = rx->cfg.sample_rate;
    hipError_t e = hipSuccess;
    if (job == RX_K2R_PACK) e = launch_frame_pack_ragged(fa, rdev, S, c->stream);
    else { // (without samples: as many frames per stream as the busiest one starts)
        int max_started = 0;
        for (int s = 0; s < S; ++s) if (rows[(size_t)s].meta_count > max_started) max_started = rows[(size_t)s].meta_count;
        if (max_started) e = launch_frame_meta_ragged(fa, rdev, max_started, S, c->stream);
    }
    return e == hipSuccess ? SDRHIP_OK : fail(SDRHIP_EDEVICE, "frame pack launch: %s", hipGetErrorString(e));
}

// FEC: the completed frames of every stream as a dense list (frame f of stream s = area frame s * cap + slot), one launch per
// encoder form present (rx_encode_groups; the surplus rows of a group's largest count land in the unspecified rest of the slot)
int RxRagged::encode()
{
    const RxFrameArea &A = rx->area;
    int rc;
    if (!(n.sum_done && FB > (size_t)SDRHIP_NB_ORIGINAL)) return SDRHIP_OK;
    const size_t nl = rx_flist_entries(n.sum_done);
    PinnedBuf &fpin = call.tabs ? call.tabs->flist : rx->r_flist_pin;
    if ((rc = fpin.reserve(nl * 4))) return rc;
    if ((rc = rx->r_flist.reserve(nl * 4))) return rc;
    int32_t *fl = fpin.as<int32_t>();
    const RxEncGroups g = rx_encode_groups((size_t)S, [&](size_t s) { const RxEncStream e = {rx_fec_of(rx, s), n.done[s], A.index(s)}; return e; }, enc128_min_rows(c), fl);
    if (g.k > nl) return fail(SDRHIP_EINVAL, "rx_process_ragged: frame list"); // (cannot happen: rx_flist_entries counts three paddings)
    if (g.k) {
        HIP_TRY(hipMemcpyAsync(rx->r_flist.p, fl, g.k * 4, hipMemcpyHostToDevice, c->stream));
        fpin.mark(c->stream);
    }
    for (int form = 0; form < 3; ++form)
        if (g.count[form] && (rc = fec_encode_device(c, area, frame_bytes, (size_t)S * A.cap(), g.rows[form], area + (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, frame_bytes,
                                                     rx->r_flist.as<int32_t>() + g.first[form], (int)(g.count[form] / GF_FRAMES_PER_GROUP))))
            return rc;
    return SDRHIP_OK;
}

// delivery: every stream's window in the shape rx_ragged_delivery names, the view, and the windows move on
int RxRagged::deliver(const RxFramesOut &out)
{
    const RxFrameArea &A = rx->area;
    const size_t nS = (size_t)S, max_done = n.max_done;
    const std::vector<size_t> &done = n.done;
    if (out.frames && max_done) {
        const hipMemcpyKind kind = out.mem == SDRHIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        bool same_base = true, same_done = true;
        for (size_t s = 1; s < nS; ++s) { same_base = same_base && A.slot(s) == A.slot(0); same_done = same_done && done[s] == done[0]; }
        const RxRaggedDelivery shape = rx_ragged_delivery(rx_fec_mixed(rx), same_base, same_done, call.dev_rows, out.mem == SDRHIP_MEM_HOST);
        if (shape == RX_DELIVER_RECTANGLE)
            HIP_TRY(link_copy2d(c, out.frames, S > 1 ? out.stride_bytes : max_done * frame_bytes, area + A.slot(0) * frame_bytes, stream_bytes, max_done * frame_bytes, nS,
                                kind, c->stream));
        for (size_t s = 0; s < nS && shape != RX_DELIVER_RECTANGLE; ++s) {
            uint8_t *to = out.frames + s * out.stride_bytes;
            const uint8_t *from = area + A.index(s) * frame_bytes;
            if (!done[s]) continue;
            if (shape == RX_DELIVER_PITCHED) // (each stream's frames dense, 128 + nb_fec[s] super blocks each)
                HIP_TRY(link_copy2d(c, to, rx_stream_bytes(rx, s), from, frame_bytes, rx_stream_bytes(rx, s), done[s], kind, c->stream));
            else
                HIP_TRY(link_copy(c, to, from, done[s] * frame_bytes, kind, c->stream));
        }
    }
    rx->view.set_each(area, stream_bytes, nS, A.slots(), done.data());
    for (size_t s = 0; s < nS; ++s) out.n_frames[s] = done[s];
    rx->area.commit(done.data(), n.rest.data());
    if (out.mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// A call that fails after it moved windows leaves the windows moved (the open frames lie there now) and the rest of the framing
// state untouched.
int sdrhip::rx_ragged(sdrhip_rx *rx, const int16_t *iq_in, const RxRaggedCounts &n, size_t in_stride, const uint32_t *tv_sec, const uint32_t *tv_usec,
                      const RxFramesOut &out, const RxRaggedCall &call)
{
    const int S = rx->nstreams;
    const size_t max_in = n.max_in;
    for (int s = 0; s < S; ++s) out.n_frames[s] = 0;
    // ---- everything that can be refused is checked before anything is consumed
    if (int e = check_mem(out.mem)) return e;
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "rx_process_ragged: not available in pipelined mode");
    if (!call.batch && rx_batches_active(rx)) return fail(SDRHIP_EINVAL, "rx_process_ragged: asynchronous batches are being filled or in flight: collect them first");
    if (S == 1) in_stride = max_in;
    if (S > 1 && in_stride < max_in) return fail(SDRHIP_EINVAL, "rx_process_ragged: in_stride smaller than the largest count");
    if (max_in && !iq_in) return fail(SDRHIP_EINVAL, "rx_process_ragged: NULL input");
    // (per-stream input format: the caller's rows are K0x's source, 4-byte units of stride whatever a row holds)
    const RxRaggedInput input = rx_ragged_input(call.batch, call.dev_rows, rx->streams.formats() != nullptr, rx->in_fmt == IQF_S16, out.mem == SDRHIP_MEM_DEVICE);
    if (input.unpack && !unpackx_measure(n.n_in, 1, (size_t)S, rx->streams.formats()).fits) return fail(SDRHIP_EINVAL, "rx_process_ragged: too many samples for one launch");
    if (max_in && input.in_dev && (!aligned16(iq_in) || (S > 1 && (in_stride & (input.widen ? 7 : 3)))))
        return fail(SDRHIP_EALIGN, "rx_process_ragged: device input must be 16-byte aligned, its stride a multiple of %d samples", input.widen ? 8 : 4);
    if (int e = rx_refuse_delivery("rx_process_ragged", n, out.frames, out.stride_bytes, out.mem, false)) return e;
    HIP_TRY(hipSetDevice(rx->ctx->device));
    rx->consumed = false;
    if (max_in == 0) { rx->view.clear(); return SDRHIP_OK; } // nothing arrives: nothing changes, nothing is delivered
    int rc;
    // ---- windows: stream s fills slots slot(s) .. slot(s) + done[s] of its area (what moves when: RxFrameArea::plan)
    if ((rc = rx_release_old(rx))) return rc;
    if ((rc = rx_make_room(rx, n.done.data(), false, "rx_process_ragged"))) return rc;
    const size_t fb = rx_frame_bytes(rx);
    RxRagged rg = {rx, rx->ctx, S, rx->cfg.log2decim, n, call, input, fb / SDRHIP_UDPSIZE, fb, rx->area.cap() * fb, rx->work.as<uint8_t>(), std::vector<unsigned>((size_t)S),
                   {0}, rx->streams.records(rx_bank(rx)), std::vector<RaggedRow>((size_t)S), nullptr, RaggedPlan(), nullptr, 0};
    rx_meta_base(rx->cfg, rg.mw);
    if ((rc = rg.table(tv_sec, tv_usec))) return rc;
    if ((rc = rg.input(iq_in, in_stride))) return rc;
    if ((rc = rg.decimate())) return rc;
    if ((rc = rg.encode())) return rc;
    return rg.deliver(out);
}

extern "C" int sdrhip_rx_process_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                                        const uint32_t *tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_in || !tv_sec || !tv_usec || !n_frames) return fail(SDRHIP_EINVAL, "rx_process_ragged: NULL count, stamp or n_frames array");
    sdrhip::CtxLock lock_(rx->ctx);
    const RxFramesOut out = {frames_out, frame_stride_bytes, n_frames, mem};
    return rx_ragged(rx, iq_in, rx_counts(rx, n_in), in_stride, tv_sec, tv_usec, out);
}
