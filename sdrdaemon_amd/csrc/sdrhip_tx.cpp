// sdrhip_tx.cpp -- the fused Tx pipe of include/sdrhip.h: life cycle, sdrhip_tx_process, flush, the datagram-fed call.
#include "sdrhip_pipes.h"

using namespace sdrhip;

namespace {
// waits for an event when its scope ends, whichever way: a copy on another stream that reads memory the caller gets back
struct EventWait {
    hipEvent_t ev = nullptr;
    ~EventWait() { if (ev) (void)hipEventSynchronize(ev); }
};
} // namespace

extern "C" int sdrhip_tx_create(sdrhip_ctx *ctx, int nstreams, int log2interp, sdrhip_tx **out)
{
    if (!ctx || !out || nstreams <= 0) return fail(SDRHIP_EINVAL, "tx_create: bad argument");
    if (log2interp < 0 || log2interp > 6) return fail(SDRHIP_EINVAL, "Invalid log2 interpolation factor");
    sdrhip_tx *tx = new (std::nothrow) sdrhip_tx(ctx);
    if (!tx) return fail(SDRHIP_ENOMEM, "out of host memory");
    tx->nstreams = nstreams; tx->log2interp = log2interp;
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
    sdrhip_ctx *c = tx->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2); // (a decode of the pipelined mode may still run there)
    tx->ring.wait_all();
    sdrhip_interpolators_destroy(tx->itp);
    sdrhip_fecbuf_destroy(tx->fb);
    delete tx; // (no lock held: the last reference frees the context, its mutex included)
}

extern "C" int sdrhip_tx_set_pipelined(sdrhip_tx *tx, int on)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (!on && tx->late.have) return fail(SDRHIP_EINVAL, "tx_set_pipelined: sdrhip_tx_flush the waiting batch first");
    if (on && tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_set_pipelined: asynchronous datagram batches are in flight: collect them first");
    if (on) {
        HIP_TRY(hipSetDevice(tx->ctx->device));
        for (DevEvent *e : {&tx->ev_in, &tx->ev_up, &tx->ev_dec, &tx->ev_itp[0], &tx->ev_itp[1]})
            if (int rc = e->ensure()) return rc;
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
    if (tx->ring.busy()) return fail(SDRHIP_EINVAL, "tx_set_output_format: asynchronous batches are in flight: collect them first");
    if (tx->late.have) return fail(SDRHIP_EINVAL, "tx_set_output_format: a pipelined batch waits: sdrhip_tx_flush it first");
    tx->out_fmt = fmt;
    return SDRHIP_OK;
}

// the sink object is per process and so per stream (sdrdaemontx.cpp:195-255): host state only, the table goes up with the next launch
extern "C" int sdrhip_tx_set_stream_format(sdrhip_tx *tx, const int *fmt)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    for (int s = 0; fmt && s < tx->nstreams; ++s) {
        if (fmt[s] == SDRHIP_IQ_U8) return fail(SDRHIP_EINVAL, "tx_set_stream_format: stream %d: SDRHIP_IQ_U8 is an input format (RTL-SDR); the Tx side gives S16 or S8", s);
        if (fmt[s] != SDRHIP_IQ_S16 && fmt[s] != SDRHIP_IQ_S8) return fail(SDRHIP_EINVAL, "tx_set_stream_format: stream %d: unknown format %d", s, fmt[s]);
    }
    if (tx->ring.busy()) return fail(SDRHIP_EINVAL, "tx_set_stream_format: asynchronous batches are in flight: collect them first");
    if (tx->late.have) return fail(SDRHIP_EINVAL, "tx_set_stream_format: a pipelined batch waits: sdrhip_tx_flush it first");
    if (fmt) tx->s_fmt.assign(fmt, fmt + tx->nstreams);
    else tx->s_fmt.clear();
    ++tx->s_fmt_ver;
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_get_stream_format(const sdrhip_tx *tx, int stream, int *fmt)
{
    if (!tx || !fmt) return fail(SDRHIP_EINVAL, "tx_get_stream_format: NULL argument");
    sdrhip::CtxLock lock_(tx->ctx);
    if (stream < 0 || stream >= tx->nstreams) return fail(SDRHIP_EINVAL, "tx_get_stream_format: stream %d of %d", stream, tx->nstreams);
    *fmt = tx_formats(tx) ? tx->s_fmt[(size_t)stream] : tx->out_fmt;
    return SDRHIP_OK;
}

namespace sdrhip {
int tx_format_table(sdrhip_tx *tx, const int **fmt_dev)
{
    *fmt_dev = nullptr;
    if (!tx_formats(tx)) return SDRHIP_OK;
    if (tx->s_fmt_up != tx->s_fmt_ver) {
        const void *dev = nullptr;
        if (int rc = tx->s_fmt_tab.upload(tx->ctx->stream, tx->s_fmt.data(), tx->s_fmt.size() * sizeof(int), &dev)) return rc;
        tx->s_fmt_up = tx->s_fmt_ver;
    }
    *fmt_dev = static_cast<const int *>(tx->s_fmt_tab.current());
    return SDRHIP_OK;
}

hipError_t tx_download_rows(sdrhip_tx *tx, void *iq_out, size_t out_stride, const void *dout, size_t dos, const size_t *n, size_t n_all)
{
    sdrhip_ctx *c = tx->ctx;
    const size_t S = (size_t)tx->nstreams, unit = tx_unit(tx);
    for (size_t s = 0; s < S;) {
        const size_t len = n ? n[s] : n_all, esz = tx_esz(tx, s);
        size_t e = s + 1;
        while (e < S && (n ? n[e] : n_all) == len && tx_esz(tx, e) == esz) ++e;
        if (len) {
            const hipError_t err = link_copy2d(c, static_cast<char *>(iq_out) + s * out_stride * unit, out_stride * unit,
                                               static_cast<const char *>(dout) + s * dos * unit, dos * unit, len * esz, e - s, hipMemcpyDeviceToHost, c->stream);
            if (err != hipSuccess) return err;
        }
        s = e;
    }
    return hipSuccess;
}

int tx_decode(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, DevBuf &pay, size_t pstride, const DecodeSide *side,
              uint8_t *block0)
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
    return c->opt.tx_gather && !tx->pipelined && tx->out_fmt == IQF_S16 && !tx_formats(tx) && interpolate_gather_ok(c, log2interp) && fec_decode_gather_ok(c);
}
int tx_decode_gather(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, InterpGather *g, uint8_t *block0)
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
static int tx_interpolate(sdrhip_tx *tx, int log2interp, const DevBuf &pay, size_t n_payload, size_t pstride, int16_t *iq_out, size_t out_stride, int mem,
                   const InterpGather *gather = nullptr)
{
    const int S = tx->nstreams;
    const size_t n_res = n_payload << log2interp;
    int16_t *dout = iq_out;
    size_t dos = out_stride;
    int rc;
    const int *fmt_dev = nullptr; // (set: the array of sdrhip_tx_set_stream_format; strides then count 4-byte units)
    if ((rc = tx_format_table(tx, &fmt_dev))) return rc;
    if (mem == SDRHIP_MEM_HOST) {
        dos = tx_own_pitch(tx, n_res);
        if ((rc = tx->outbuf.reserve((size_t)S * dos * tx_unit(tx) + 16))) return rc;
        dout = tx->outbuf.as<int16_t>();
    }
    if ((rc = interpolate_device(tx->itp, log2interp, gather ? nullptr : pay.as<int16_t>(), n_payload, pstride, dout, dos, nullptr, gather, nullptr, tx->out_fmt, fmt_dev))) return rc;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(tx_download_rows(tx, iq_out, out_stride, dout, dos, nullptr, n_res));
    return SDRHIP_OK;
}

// delivery half of a pipelined call (and of sdrhip_tx_flush): the waiting batch through the interpolator on the first stream
static int tx_deliver_late(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams;
    const size_t n_res = tx->late.n_payload << tx->late.log2interp;
    if (S == 1) out_stride = n_res;
    if (!iq_out) return fail(SDRHIP_EINVAL, "tx: NULL output buffer for the waiting batch");
    if (out_stride < n_res) return fail(SDRHIP_EINVAL, "tx: out_stride smaller than the waiting batch (%zu samples per stream)", n_res);
    if (mem == SDRHIP_MEM_DEVICE && !tx_out_aligned(tx, iq_out, out_stride)) return fail(SDRHIP_EALIGN, "tx_process: device output must be 16-byte aligned, its stride a multiple of 4 (8-bit: 8) samples (per-stream formats: of 4 4-byte units)");
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

int tx_interpolate_counts(sdrhip_tx *tx, const int16_t *pay, size_t n_max, size_t pitch, int16_t *dout, size_t dos, const int *counts)
{
    const int L = tx->log2interp;
    const int *fmt_dev = nullptr;
    if (int rc = tx_format_table(tx, &fmt_dev)) return rc;
    if (n_max == 0 || (L == 0 && tx->out_fmt != IQF_S8 && !fmt_dev)) return SDRHIP_OK;
    // (x1 has no count-aware kernel: K6n narrows the largest stream's length; past a stream's own count the samples are unspecified)
    const InterpCount cnt = {counts + FB_K, FB_COUNTS, (int)SDRHIP_SAMPLES_PER_FRAME};
    // (per-stream formats: K6x at x1 and K5x know each stream's own count; nothing is written past it)
    if (fmt_dev) return interpolate_device(tx->itp, L, pay, n_max, pitch, dout, dos, nullptr, nullptr, &cnt, tx->out_fmt, fmt_dev);
    if (L == 0) return interpolate_device(tx->itp, 0, pay, n_max, pitch, dout, dos, nullptr, nullptr, nullptr, IQF_S8);
    return interpolate_device(tx->itp, L, pay, n_max, pitch, dout, dos, nullptr, nullptr, &cnt, tx->out_fmt);
}

int tx_collector(sdrhip_tx *tx)
{
    return tx->fb ? SDRHIP_OK : sdrhip_fecbuf_create(tx->ctx, tx->nstreams, &tx->fb);
}
} // namespace sdrhip

extern "C" int sdrhip_tx_flush(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (n_out) *n_out = 0;
    if (int e = check_mem(mem)) return e;
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
    if (int e = check_mem(mem)) return e;
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
        EventWait up; // (armed below: no exit of this call leaves the upload reading the caller's rx)
        if (mem == SDRHIP_MEM_HOST) {
            if (overlap) HIP_TRY(hipStreamSynchronize(s2)); // (the previous decode may still read rxbuf; it ran beside the previous call's interpolator)
            if ((rc = tx->rxbuf.reserve((size_t)S * nframes * fb))) return rc;
            HIP_TRY(link_copy2d(c, tx->rxbuf.p, nframes * fb, rx, rx_stride_bytes, nframes * fb, S, hipMemcpyHostToDevice, s2));
            // (pinned caller memory makes this copy truly asynchronous, and it runs on the SECOND stream: the call must not return
            // before it has read `rx` -- the host-pointer contract is "the buffer is yours again when the call returns")
            if (overlap) { HIP_TRY(hipEventRecord(tx->ev_up, s2)); up.ev = tx->ev_up; }
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
            if (overlap) { up.ev = nullptr; HIP_TRY(hipEventSynchronize(tx->ev_up)); } // (... but the caller's rx has been read)
        }
        return SDRHIP_OK;
    }

    const uint8_t *drx = rx;
    if (mem == SDRHIP_MEM_HOST) {
        if ((rc = tx->rxbuf.reserve((size_t)S * nframes * fb))) return rc;
        HIP_TRY(link_copy2d(c, tx->rxbuf.p, nframes * fb, rx, rx_stride_bytes, nframes * fb, S, hipMemcpyHostToDevice, c->stream));
        drx = tx->rxbuf.as<uint8_t>();
    } else {
        if (!tx_out_aligned(tx, iq_out, out_stride)) return fail(SDRHIP_EALIGN, "tx_process: device output must be 16-byte aligned, its stride a multiple of 4 (8-bit: 8) samples (per-stream formats: of 4 4-byte units)");
    }
    // no-copy: decode (restored blocks + map only), then the interpolator reads the received frames through the map; otherwise
    // decode all S * nframes frames in one batch: payload [S][nframes][127 * 508] = [S][n_payload] samples
    InterpGather g;
    const bool gather = tx_gather_applies(tx, tx->log2interp);
    if (gather) rc = tx_decode_gather(tx, drx, indices, nframes, &g);
    else if (!(rc = tx->payload[0].reserve((size_t)S * pstride * 4 + 16))) rc = tx_decode(tx, drx, indices, nframes, tx->payload[0], pstride, nullptr);
    if (rc) return rc;
    if ((rc = tx_interpolate(tx, tx->log2interp, tx->payload[0], n_payload, pstride, iq_out, out_stride, mem, gather ? &g : nullptr))) return rc;
    if (mem == SDRHIP_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- Tx pipe fed datagrams
// UDPSourceFEC::read -> SDRdaemonFECBuffer::writeAndRead -> Upsampler::process for every stream (sdrdaemontx.cpp:449-498,
// UDPSourceFEC.cpp:52-78): the FEC buffer bank collects and decodes into payload[0] ([stream][pitch] samples, every stream 16-byte
// aligned: one frame is 64 516 bytes = 4 mod 16, and K5w's paired loads want aligned streams), then ONE ragged interpolator launch
// takes each stream's own count from where the bank's classify pass left it.  The grid is planned from the largest count, which
// the host holds after the bank's one read-back.
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
    if (int e = check_mem(mem)) return e;
    if (tx->pipelined) return fail(SDRHIP_EINVAL, "tx_process_datagrams: the handle is in pipelined mode");
    if (tx->ring.busy()) return fail(SDRHIP_EINVAL, "tx_process_datagrams: asynchronous batches are in flight: collect them first");
    sdrhip_ctx *c = tx->ctx;
    const int S = tx->nstreams, L = tx->log2interp;
    if (max_frames > 0x3fffffffu) return fail(SDRHIP_EINVAL, "tx_process_datagrams: max_frames too large");
    if (max_frames > 0 && (!iq_out || !info_out)) return fail(SDRHIP_EINVAL, "tx_process_datagrams: NULL iq_out / info_out");
    const size_t per = max_frames * SDRHIP_SAMPLES_PER_FRAME, n_res_max = per << L;
    const bool mixed = tx_formats(tx), s8 = !mixed && tx->out_fmt == IQF_S8; // (mixed: strides count 4-byte units, every x1 is K6x)
    const size_t unit = tx_unit(tx);
    if (S == 1) out_stride = tx_own_pitch(tx, n_res_max);
    if (out_stride < n_res_max) return fail(SDRHIP_EINVAL, "tx_process_datagrams: out_stride below max_frames x 16129 << log2interp");
    if (mem == SDRHIP_MEM_DEVICE && max_frames > 0 && (!aligned16(iq_out) || (out_stride & (s8 ? 7 : 3)) || (reinterpret_cast<uintptr_t>(block0_out) & 3u)))
        return fail(SDRHIP_EALIGN, "tx_process_datagrams: device iq_out must be 16-byte aligned, out_stride a multiple of 4 (8-bit: 8) samples (per-stream formats: of 4 4-byte units), block0_out 4-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = tx_collector(tx))) return rc;
    if ((rc = fecbuf_check_dgrams(tx->fb, dgrams, n_dgrams, dgram_stride_bytes, mem, "tx_process_datagrams"))) return rc;
    // where the collector writes getSlotData: the caller's device iq_out (Upsampler's m_interp == 0 pass-through, Upsampler.cpp:54-57)
    // or payload[0]; host memory: outbuf / payload[0], downloaded below
    // (8-bit output with x1: the collector writes int16 to payload[0] as for the other ratios, K6n narrows it into dout)
    const size_t pitch = (per + 3) & ~(size_t)3, n_res_pitch = tx_own_pitch(tx, n_res_max);
    const bool direct = L == 0 && !s8 && !mixed;
    int16_t *dout = iq_out;
    size_t dos = out_stride;
    if (max_frames > 0 && mem == SDRHIP_MEM_HOST) {
        if ((rc = tx->outbuf.reserve((size_t)S * n_res_pitch * unit + 16))) return rc;
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
    // (the collector's state has moved on: from here a failure loses the call's frames, it is never replayed)
    if ((rc = tx_interpolate_counts(tx, tx->payload[0].as<int16_t>(), n_max, pitch, dout, dos, counts))) return rc;
    if (mem == SDRHIP_MEM_HOST) {
        // (bank-wide: every row up to the largest count, as one copy; per-stream formats: each stream's own samples)
        std::vector<size_t> own;
        for (int s = 0; mixed && s < S; ++s) own.push_back((n_frames[s] * SDRHIP_SAMPLES_PER_FRAME) << L);
        if (kmax > 0) HIP_TRY(tx_download_rows(tx, iq_out, out_stride, dout, dos, mixed ? own.data() : nullptr, n_max << L));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SDRHIP_OK;
}
