// sdrhip_tx_async.cpp -- the asynchronous host-pointer entries of the Tx pipe (submit / collect of frames and of raw datagrams).
#include "sdrhip_pipes.h"

using namespace sdrhip;

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
    if (tx->ring.busy()) return fail(SDRHIP_EINVAL, "tx_set_async: batches are in flight: collect them first");
    tx->ring.reset((size_t)depth);
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
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int S = tx->nstreams;
    const size_t fb = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE, row = nframes * fb;
    if (S == 1) rx_stride_bytes = row;
    if (rx_stride_bytes < row) return fail(SDRHIP_EINVAL, "tx_submit: stride too small");
    sdrhip_tx::ABatch &b = tx->ring.tail_batch();
    if (b.state == 2) return fail(SDRHIP_EBUSY, "tx_submit: every batch of the ring is in flight: sdrhip_tx_collect first");
    const size_t n_payload = nframes * SDRHIP_SAMPLES_PER_FRAME, n_res = n_payload << tx->log2interp;
    const bool mixed = tx_formats(tx); // (per-stream formats: rows of 4-byte units, gathered into a download of exactly the delivered bytes)
    const size_t pstride = (n_payload + 3) & ~(size_t)3, dos = tx_own_pitch(tx, n_res), unit = tx_unit(tx);
    const size_t b0_bytes = (size_t)S * nframes * SDRHIP_BLOCK_BYTES;
    size_t s_bytes = (size_t)S * dos * unit; // sample bytes of the download
    if (mixed) {
        s_bytes = 0;
        for (int s = 0; s < S; ++s) s_bytes += n_res * tx_esz(tx, (size_t)s);
    }
    int rc;
    const int *fmt_dev = nullptr;
    // everything that can fail for want of memory comes first
    if ((rc = b.din.reserve((size_t)S * row))) return rc;
    if ((rc = b.dout.reserve((size_t)S * dos * unit + 16))) return rc;
    if ((rc = b.db0.reserve(b0_bytes))) return rc;
    if ((rc = b.out.reserve(s_bytes + b0_bytes))) return rc;
    if (mixed) {
        if ((rc = reserve_settled(c, tx->a_gat, s_bytes + 16))) return rc;
        if ((rc = reserve_settled(c, tx->a_seg, (size_t)3 * S * sizeof(GatherSeg)))) return rc;
        if ((rc = b.seg.reserve((size_t)3 * S * sizeof(GatherSeg)))) return rc;
        if ((rc = tx_format_table(tx, &fmt_dev))) return rc;
    }
    const bool gather = tx_gather_applies(tx, tx->log2interp);
    if (!gather && (rc = tx->payload[0].reserve((size_t)S * pstride * 4 + 16))) return rc;
    if ((rc = b.done.ensure())) return rc;
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
                                     nullptr, nullptr, tx->out_fmt, fmt_dev)))
            return rc;
    }
    // (from here on the interpolator's state has advanced: a failure loses the batch, it is never replayed)
    hipError_t e = hipSuccess;
    const void *samples = b.dout.p;
    if (mixed) { // each row's n_res * bytes(fmt[s]) bytes, back to back
        GatherSeg *seg = b.seg.as<GatherSeg>();
        uint64_t dst = 0;
        for (int s = 0; s < S; ++s) {
            GatherSeg &g = seg[s];
            g.src = b.dout.as<uint8_t>() + (size_t)s * dos * 4; g.bytes = n_res * tx_esz(tx, (size_t)s);
            g.dst = dst; g.pad = 0;
            dst += g.bytes;
        }
        const uint32_t grid = gather_plan(seg, S);
        if (!grid) e = hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMemcpyAsync(tx->a_seg.p, seg, (size_t)S * sizeof(GatherSeg), hipMemcpyHostToDevice, c->stream); // (not counted: a table)
        if (e == hipSuccess) {
            b.seg.mark(c->stream);
            KTimer kt(c, SDRHIP_K_CONVERT);
            e = launch_delivery_gather(tx->a_seg.as<GatherSeg>(), S, grid, tx->a_gat.as<uint8_t>(), c->stream);
        }
        samples = tx->a_gat.p;
    }
    if (e == hipSuccess) e = link_copy(c, b.out.p, samples, s_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = link_copy(c, b.out.as<char>() + s_bytes, b.db0.p, b0_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "tx batch download: %s (the batch's %zu frames per stream are lost)", hipGetErrorString(e), nframes);
    b.nframes = nframes; b.n_res = n_res; b.dos = dos;
    b.rows4 = mixed;
    b.esz.resize((size_t)S);
    for (int s = 0; s < S; ++s) b.esz[(size_t)s] = (uint8_t)tx_esz(tx, (size_t)s);
    b.state = 2;
    ++tx->ring.tail;
    return SDRHIP_OK;
}

// the oldest batch of the ring once it has finished (a Tx batch goes out when it is submitted: none is ever being filled)
static int tx_oldest(sdrhip_tx *tx, std::unique_lock<std::recursive_mutex> &lock_, int wait, const char *who, sdrhip_tx::ABatch **bp)
{
    return tx->ring.wait_oldest(lock_, wait, who, [](sdrhip_tx::ABatch &) { return SDRHIP_OK; }, bp);
}

extern "C" int sdrhip_tx_collect(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_samples, uint8_t *block0_out, size_t *n_out, size_t *n_frames, int wait)
{
    if (!tx || !n_out) return fail(SDRHIP_EINVAL, "tx_collect: NULL argument");
    // (the wait happens outside the context lock: the submitting thread -- the reference's reader thread -- keeps feeding the ring)
    std::unique_lock<std::recursive_mutex> lock_(tx->ctx->mtx);
    *n_out = 0;
    if (n_frames) *n_frames = 0;
    if (tx_in_flight(tx, true)) return fail(SDRHIP_EINVAL, "tx_collect: asynchronous datagram batches are in flight: use sdrhip_tx_collect_datagrams");
    HIP_TRY(hipSetDevice(tx->ctx->device));
    sdrhip_tx::ABatch *bp = nullptr;
    int rc = tx_oldest(tx, lock_, wait, "tx_collect", &bp);
    if (rc) return rc;
    sdrhip_tx::ABatch &b = *bp;
    const int S = tx->nstreams;
    // (the formats cannot change while a batch is in flight; the batch holds its own all the same)
    size_t s_bytes = 0;
    for (int s = 0; s < S; ++s) s_bytes += (b.rows4 ? b.n_res : b.dos) * b.esz[(size_t)s];
    if (b.n_res > max_samples) { // (the batch stays where it is: call again with room for *n_out samples per stream)
        *n_out = b.n_res;
        if (n_frames) *n_frames = b.nframes;
        return fail(SDRHIP_EINVAL, "tx_collect: the batch holds %zu samples per stream, iq_out has room for %zu", b.n_res, max_samples);
    }
    if (b.n_res) {
        if (!iq_out) return fail(SDRHIP_EINVAL, "tx_collect: NULL iq_out");
        if (S == 1) out_stride = b.n_res;
        if (out_stride < b.n_res) return fail(SDRHIP_EINVAL, "tx_collect: out_stride too small");
        const char *src = b.out.as<char>();
        for (int s = 0; s < S; ++s) { // (per-stream formats: packed rows in, rows of 4-byte units out)
            const size_t esz = b.esz[(size_t)s];
            memcpy(reinterpret_cast<char *>(iq_out) + (size_t)s * out_stride * (b.rows4 ? 4 : esz), src, b.n_res * esz);
            src += (b.rows4 ? b.n_res : b.dos) * esz;
        }
    }
    if (block0_out) memcpy(block0_out, b.out.as<char>() + s_bytes, (size_t)S * b.nframes * SDRHIP_BLOCK_BYTES);
    *n_out = b.n_res;
    if (n_frames) *n_frames = b.nframes;
    b.state = 0;
    ++tx->ring.head;
    return SDRHIP_OK;
}

// --------------------------------------------------------------------------- asynchronous Tx batches of raw datagrams
// sdrdaemontx's reader thread receives datagrams while its main loop interpolates (sdrdaemontx.cpp:449-498).  A batch goes out with
// no synchronisation: its datagrams up packed (one memcpy per stream into the batch's pinned arena, or in place from
// sdrhip_host_alloc memory), the collector's passes with grids from the host's shadow of the classification (fecbuf_packed: no
// read-back), the decoder, the interpolator at the factor in force, the delivery gather, ONE download of exactly the delivered
// bytes.  The collector and the histories are the ones sdrhip_tx_process_datagrams and sdrhip_tx_process use.
// one batch behind fecbuf_batch_check[_tagged] (`in`; the context lock is held): the rest of the refusals, then the submit
static int tx_submit_batch(sdrhip_tx *tx, FecBufBatch &in, const char *who)
{
    const int S = tx->nstreams;
    const size_t *n_dgrams = in.n_dgrams;
    if (tx->pipelined) return fail(SDRHIP_EINVAL, "%s: the handle is in pipelined mode", who);
    if (tx->late.have) return fail(SDRHIP_EINVAL, "%s: a pipelined batch waits: sdrhip_tx_flush it first", who);
    if (tx_in_flight(tx, false)) return fail(SDRHIP_EINVAL, "%s: batches of received frames are in flight: sdrhip_tx_collect them first", who);
    sdrhip_tx::ABatch &b = tx->ring.tail_batch();
    if (b.state == 2) return fail(SDRHIP_EBUSY, "%s: every batch of the ring is in flight: sdrhip_tx_collect_datagrams first", who);
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = tx_collector(tx))) return rc;
    std::vector<FecBufShadow> sh;
    if ((rc = fecbuf_shadow(tx->fb, &sh))) return rc;

    // ---- staging: packed, one memcpy per non-empty stream (in place: the caller's pinned memory); the shadow runs over the headers
    std::vector<int> res((size_t)S * 4);
    if ((rc = fecbuf_batch_stage(&in, b.in, b.tab, sh, res.data()))) return rc;
    size_t kmax = 0, kall = 0;
    for (int s = 0; s < S; ++s) {
        kmax = (size_t)res[(size_t)s * 4] > kmax ? (size_t)res[(size_t)s * 4] : kmax;
        kall += (size_t)res[(size_t)s * 4];
    }
    const int L = tx->log2interp;
    const bool mixed = tx_formats(tx), s8 = !mixed && tx->out_fmt == IQF_S8, direct = L == 0 && !s8 && !mixed;
    const size_t unit = tx_unit(tx), per = kmax * SDRHIP_SAMPLES_PER_FRAME, pitch = (per + 3) & ~(size_t)3;
    const size_t dos = tx_own_pitch(tx, per << L), n_one = (size_t)SDRHIP_SAMPLES_PER_FRAME << L;
    size_t b_samples = 0; // (each stream's frames at its own sample size)
    for (int s = 0; s < S; ++s) b_samples += (size_t)res[(size_t)s * 4] * n_one * tx_esz(tx, (size_t)s);
    const size_t b_total = b_samples + kall * (DG_REC + SDRHIP_BLOCK_BYTES);
    // everything that can fail for want of memory comes before the collector moves (a device buffer that grows waits for the
    // batches in flight)
    if (in.dev_bytes && (rc = reserve_settled(c, tx->a_pk, in.dev_bytes + 16))) return rc;
    if (kmax && !direct && (rc = reserve_settled(c, tx->a_pay, (size_t)S * pitch * 4 + 16))) return rc;
    if (kmax && (rc = reserve_settled(c, tx->a_out, (size_t)S * dos * unit + 16))) return rc;
    if (kmax && (rc = reserve_settled(c, tx->a_b0, (size_t)S * kmax * SDRHIP_BLOCK_BYTES + 16))) return rc;
    if (b_total && (rc = reserve_settled(c, tx->a_gat, b_total + 16))) return rc;
    if ((rc = reserve_settled(c, tx->a_seg, (size_t)3 * S * sizeof(GatherSeg)))) return rc;
    if (b_total && (rc = b.out.reserve(b_total))) return rc;
    if ((rc = b.seg.reserve((size_t)3 * S * sizeof(GatherSeg)))) return rc;
    if ((rc = b.done.ensure())) return rc;

    // ---- upload: exactly the datagrams (staged: one copy; in place: one per run of adjacent rows)
    uint8_t *pk = tx->a_pk.as<uint8_t>();
    if ((rc = fecbuf_batch_upload(c, in, b.in, pk))) return rc;

    // ---- the collector's passes, no read-back (from the scatter launch on, the batch is consumed: a failure loses it)
    uint8_t *data = direct ? tx->a_out.as<uint8_t>() : tx->a_pay.as<uint8_t>();
    const size_t data_stride = direct ? dos * 4 : pitch * 4;
    bool committed = false;
    const int *counts = nullptr;
    const FecBufPub *pub = nullptr;
    rc = fecbuf_packed(tx->fb, pk, n_dgrams, res.data(), sh, b.tab, kmax ? data : nullptr, data_stride, kmax ? tx->a_b0.as<uint8_t>() : nullptr, kmax,
                       c->dec_stats + DEC_STATS_SHADOW_MISMATCH, &committed, &counts, &pub);
    if (rc && !committed) { // (nothing consumed)
        if (in.n_total) b.tab.mark(c->stream); // (the places of a tagged batch went up from it)
        return rc;
    }
    if (rc) return fecbuf_batch_lost(who, rc);
    // ---- the interpolator (x1: the collector wrote the samples where the gather reads them; 8-bit x1: K6n narrows them)
    if ((rc = tx_interpolate_counts(tx, tx->a_pay.as<int16_t>(), per, pitch, tx->a_out.as<int16_t>(), dos, counts))) return fecbuf_batch_lost(who, rc);
    // ---- the delivery: every stream's samples, then the records, then the meta blocks, gathered and downloaded in ONE copy
    GatherSeg *seg = b.seg.as<GatherSeg>();
    int nseg = 0;
    uint64_t dst = 0;
    for (int part = 0; part < 3; ++part)
        for (int s = 0; s < S; ++s) {
            const size_t k = (size_t)res[(size_t)s * 4];
            if (!k) continue;
            GatherSeg &g = seg[nseg++];
            if (part == 0) { g.src = tx->a_out.as<uint8_t>() + (size_t)s * dos * unit; g.bytes = k * n_one * tx_esz(tx, (size_t)s); }
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
    b.dg = true; b.log2interp = L; b.rows4 = mixed;
    b.esz.resize((size_t)S);
    for (int s = 0; s < S; ++s) b.esz[(size_t)s] = (uint8_t)tx_esz(tx, (size_t)s);
    b.nframes = kmax; b.n_res = kmax * n_one; b.dos = 0;
    b.state = 2;
    ++tx->ring.tail;
    fecbuf_set_async_busy(tx->fb, true);
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_submit_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    if (!n_dgrams) return fail(SDRHIP_EINVAL, "tx_submit_datagrams: NULL n_dgrams");
    sdrhip::CtxLock lock_(tx->ctx);
    // ---- everything that can be refused is checked before anything is consumed
    const char *who = "tx_submit_datagrams";
    FecBufBatch in;
    if (int e = fecbuf_batch_check(&in, tx->nstreams, dgrams, n_dgrams, dgram_stride_bytes, who)) return e;
    return tx_submit_batch(tx, in, who);
}

// the same batch from an arrival-order array: the tags are walked (and refused) first, KX sorts the upload on the device
extern "C" int sdrhip_tx_submit_datagrams_tagged(sdrhip_tx *tx, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    const char *who = "tx_submit_datagrams_tagged";
    FecBufBatch in;
    if (int e = fecbuf_batch_check_tagged(&in, tx->nstreams, dgrams, stream_of, n_total, who)) return e;
    return tx_submit_batch(tx, in, who);
}

extern "C" int sdrhip_tx_collect_datagrams(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_frames, uint8_t *block0_out,
                                           sdrhip_fecbuf_frame *info_out, size_t *n_frames, int wait)
{
    if (!tx || !n_frames) return fail(SDRHIP_EINVAL, "tx_collect_datagrams: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(tx->ctx->mtx);
    const int S = tx->nstreams;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    if (tx_in_flight(tx, false)) return fail(SDRHIP_EINVAL, "tx_collect_datagrams: batches of received frames are in flight: use sdrhip_tx_collect");
    HIP_TRY(hipSetDevice(tx->ctx->device));
    sdrhip_tx::ABatch *bp = nullptr;
    int rc = tx_oldest(tx, lock_, wait, "tx_collect_datagrams", &bp);
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
        size_t kall = 0, b_samples = 0;
        for (int s = 0; s < S; ++s) { kall += b.frames[(size_t)s]; b_samples += b.frames[(size_t)s] * n_one * b.esz[(size_t)s]; }
        const uint8_t *src = b.out.as<uint8_t>(), *rec = src + b_samples, *meta = rec + kall * DG_REC;
        for (int s = 0; s < S; ++s) {
            const size_t k = b.frames[(size_t)s], esz = b.esz[(size_t)s];
            if (!k) continue;
            memcpy(reinterpret_cast<uint8_t *>(iq_out) + (size_t)s * out_stride * (b.rows4 ? 4 : esz), src, k * n_one * esz);
            memcpy(info_out + (size_t)s * max_frames, rec, k * DG_REC);
            if (block0_out) memcpy(block0_out + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES, meta, k * SDRHIP_BLOCK_BYTES);
            src += k * n_one * esz; rec += k * DG_REC; meta += k * SDRHIP_BLOCK_BYTES;
        }
    }
    for (int s = 0; s < S; ++s) n_frames[s] = b.frames[(size_t)s];
    b.state = 0;
    b.dg = false;
    ++tx->ring.head;
    fecbuf_set_async_busy(tx->fb, tx_in_flight(tx, true));
    return SDRHIP_OK;
}
