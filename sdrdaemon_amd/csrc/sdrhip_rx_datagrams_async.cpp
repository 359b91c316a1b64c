// sdrhip_rx_datagrams_async.cpp -- asynchronous batches of the Rx pipe fed raw FEC datagrams (sdrhip_rx_submit_datagrams /
// sdrhip_rx_collect_datagrams).  A hub's reader thread receives while its main loop works (sdrdaemontx.cpp:449-498) and
// UDPSinkFEC::write returns at once (UDPSinkFEC.cpp:193-211); sdrhip_rx_process_datagrams synchronises for the collector's
// read-back and again at its end.  A batch goes out with no synchronisation: its datagrams up packed (one memcpy per stream into
// the batch's pinned arena, or in place from sdrhip_host_alloc memory), the collector's passes with grids from the host's shadow
// of the classification (fecbuf_packed with the join: packed datagrams in, payloads behind each row's carry), the decoder, ONE
// ragged decimate / frame / encode step (rx_ragged) with counts the host derives from the shadow's release counts and its copy of
// the carry, KJ, the delivery KD (frames, then records: one launch), ONE download of exactly the delivered bytes.  The collector, the
// rows, the carry, the histories and the framing state are the ones sdrhip_rx_process_datagrams uses.
// sdrhip_rx_submit_datagrams_tagged is the same submit on an arrival-order array with a stream tag per datagram: the staging path
// (fecbuf_batch_*) walks the tags, uploads the array unsorted and has KX put it in packed order; nothing behind it differs.
#include "sdrhip_pipes.h"

using namespace sdrhip;

// one batch behind fecbuf_batch_check[_tagged] (`in`; the context lock is held): the rest of the refusals, then the submit
static int rx_submit_batch(sdrhip_rx *rx, FecBufBatch &in, const uint32_t *tv_sec, const uint32_t *tv_usec, const char *who)
{
    const int S = rx->nstreams;
    const size_t *n_dgrams = in.n_dgrams;
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "%s: not available in pipelined mode", who);
    if (rx_fec_mixed(rx) && !rx->egress)
        return fail(SDRHIP_EINVAL, "%s: the streams' fecblk differ (sdrhip_rx_set_stream_fec): such a batch is delivered in departure order only, sdrhip_rx_set_egress first", who);
    if (rx_has_batches(rx, false) || rx_has_batches(rx, true))
        return fail(SDRHIP_EINVAL, "%s: uniform or ragged batches are being filled or in flight: collect them first", who);
    sdrhip_rx::Batch &b = rx->ring.tail_batch();
    if (b.state >= 2) return fail(SDRHIP_EBUSY, "%s: every batch of the ring is in flight or lent: collect or release one first", who);
    sdrhip_ctx *c = rx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = rx_collector(rx))) return rc;
    unsigned *carry_dev = nullptr;
    std::vector<size_t> *carry = nullptr;
    if ((rc = fecbuf_join_carry(rx->fb, &carry_dev, &carry))) return rc;
    std::vector<FecBufShadow> sh;
    if ((rc = fecbuf_shadow(rx->fb, &sh))) return rc;

    // ---- staging: packed, one memcpy per non-empty stream (in place: the caller's pinned memory); the shadow runs over the headers
    std::vector<int> res((size_t)S * 4);
    if ((rc = fecbuf_batch_stage(&in, b.in, b.r_tab, sh, res.data()))) return rc;
    // ---- every count of the batch, from the shadow's release counts and the host's copy of the carry: what each stream feeds its
    // decimator, what it holds back (fed), the frames the ragged step completes and the bytes it delivers (n)
    const size_t U = rx_join_unit(rx->cfg), fb = rx_frame_bytes(rx); // (per-stream fecblk: the slot pitch)
    std::vector<size_t> rel((size_t)S), nf((size_t)S, 0);
    size_t kmax = 0, kall = 0;
    for (int s = 0; s < S; ++s) {
        const size_t k = rel[(size_t)s] = (size_t)res[(size_t)s * 4];
        kmax = k > kmax ? k : kmax;
        kall += k;
    }
    const RxJoinCounts fed = rx_join_counts(U, *carry, rel.data());
    const RxRaggedCounts n = rx_counts(rx, fed.fed.data());
    const bool any = fed.any;
    const size_t sum_done = n.sum_done, b_frames = n.bytes, b_total = b_frames + kall * DG_REC;
    const size_t seg_bytes = (size_t)2 * S * sizeof(RxDeliverSeg);
    // everything that can fail for want of memory comes before the collector moves (a device buffer that grows waits for the
    // batches in flight; the rows keep their heads): the batch's own buffers, then what the ragged step takes for these counts
    // (rx_ragged_room: frame area, tables, frame list, stream-order rows).  The pinned tables are the ring slot's own, so that what a submit waits
    // for is this slot's previous batch -- which the caller has collected -- and never the batch before it
    if (in.dev_bytes && (rc = reserve_settled(c, rx->a_pk, in.dev_bytes + 16))) return rc;
    if (kmax && (rc = rx_join_rows(rx, kmax, who))) return rc;
    if (b_total && (rc = reserve_settled(c, rx->a_frames, b_total + 16))) return rc;
    if ((rc = reserve_settled(c, rx->a_tab, seg_bytes))) return rc;
    if (b_total && (rc = b.out.reserve(b_total))) return rc;
    if ((rc = b.d_seg.reserve(seg_bytes))) return rc;
    if ((rc = b.done.ensure())) return rc;
    b.egress = rx->egress; // (departure order: the table and the tags, like everything else, before the collector moves)
    if (b.egress && (rc = rx_egress_room(rx, b, sum_done, fb / SDRHIP_UDPSIZE))) return rc;
    if (any && (rc = rx_ragged_room(rx, n, &b.d_tabs))) return rc;

    // ---- upload: exactly the datagrams (staged: one copy; in place: one per run of adjacent rows)
    uint8_t *pk = rx->a_pk.as<uint8_t>();
    if ((rc = fecbuf_batch_upload(c, in, b.in, pk))) return rc;

    // ---- the collector's passes, no read-back, the payloads behind each row's carry (from the scatter launch on, the batch is
    // consumed: a failure loses it)
    bool committed = false;
    const int *counts = nullptr;
    const FecBufPub *pub = nullptr;
    const FecBufJoin join = {carry_dev, nullptr, nullptr};
    rc = fecbuf_packed(rx->fb, pk, n_dgrams, res.data(), sh, b.r_tab, kmax ? rx->j_rows.as<uint8_t>() : nullptr, rx->j_row_len * 4, nullptr, kmax,
                       c->dec_stats + DEC_STATS_SHADOW_MISMATCH, &committed, &counts, &pub, &join);
    if (rc && !committed) { // (nothing consumed)
        if (in.n_total) b.r_tab.mark(c->stream); // (the places of a tagged batch went up from it)
        return rc;
    }
    if (rc) return fecbuf_batch_lost(who, rc);
    // ---- decimate, frame, encode: one ragged step; KJ moves every row's remainder to its head (the device's own counts)
    if (any) {
        const RxFramesOut view_only = {nullptr, 0, nf.data(), SDRHIP_MEM_DEVICE};
        const RxRaggedCall batch = {true, true, &b.d_tabs, rx->follow_meta ? fecbuf_committed_state(rx->fb) : nullptr, // (the flags as they stand at this submit)
                                    rx->follow_bits ? fecbuf_committed_state(rx->fb) : nullptr};
        if ((rc = rx_ragged(rx, rx->j_rows.as<int16_t>(), n, rx->j_row_len, tv_sec, tv_usec, view_only, batch))) return fecbuf_batch_lost(who, rc);
        hipError_t e = launch_rx_join_carry(rx->j_rows.as<int16_t>(), rx->j_row_len, carry_dev, counts, (unsigned)U, S, c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "rx join launch: %s (the batch is lost)", hipGetErrorString(e));
        *carry = fed.left;
    } else { // (nothing released, and no row holds a whole unit: rows and remainders stay)
        rx->view.clear();
    }
    // ---- the delivery: every stream's frames (its sliding window in `work`), then the records, gathered and downloaded in ONE copy
    RxDeliverSeg *seg = b.d_seg.as<RxDeliverSeg>();
    int nseg = 0;
    uint64_t dst = 0;
    for (int s = 0; s < S; ++s) {
        if (!nf[(size_t)s]) continue;
        RxDeliverSeg &g = seg[nseg++];
        g.src = rx->view.offset((size_t)s, fb);
        g.bytes = nf[(size_t)s] * rx_stream_bytes(rx, (size_t)s); g.dst = dst; g.from_records = 0; // (= fb unless the counts differ: departure order only)
        dst += g.bytes;
    }
    hipError_t e = dst == b_frames ? hipSuccess : hipErrorInvalidValue; // (this walk sums what was delivered on its own; the buffers hold what was counted)
    for (int s = 0; s < S; ++s) {
        const size_t k = (size_t)res[(size_t)s * 4];
        if (!k) continue;
        RxDeliverSeg &g = seg[nseg++];
        g.src = (size_t)s * kmax * DG_REC;
        g.bytes = k * DG_REC; g.dst = dst; g.from_records = 1;
        dst += g.bytes;
    }
    if (b.egress) { // departure order: KR / KP in KD's place writes the same buffer (sdrhip_rx_egress.cpp); KD's table stays unused
        nseg = 0;
        if (e == hipSuccess) e = rx_egress_launch(rx, b, nf.data(), fb, res.data(), kmax, reinterpret_cast<const uint8_t *>(pub));
    }
    const uint32_t grid = rx_deliver_plan(seg, nseg);
    if (e == hipSuccess && nseg && (!grid || !aligned16(pub))) e = hipErrorInvalidValue;
    if (e == hipSuccess && nseg) e = hipMemcpyAsync(rx->a_tab.p, seg, (size_t)nseg * sizeof(RxDeliverSeg), hipMemcpyHostToDevice, c->stream); // (not counted: a table)
    if (e == hipSuccess && nseg) {
        b.d_seg.mark(c->stream);
        KTimer kt(c, SDRHIP_K_CONVERT);
        e = launch_rx_deliver(rx->a_tab.as<RxDeliverSeg>(), nseg, grid, rx->work.as<uint8_t>(), reinterpret_cast<const uint8_t *>(pub),
                              rx->a_frames.as<uint8_t>(), c->stream);
    }
    if (e == hipSuccess && b_total) e = link_copy(c, b.out.p, rx->a_frames.p, b_total, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "rx datagram batch delivery: %s (the batch is lost)", hipGetErrorString(e));
    b.r_frames.assign(nf.begin(), nf.end());
    b.d_rel.assign(rel.begin(), rel.end());
    b.frame_bytes = fb;
    b.dg = true; b.ragged = false;
    b.state = 2;
    ++rx->ring.tail;
    fecbuf_set_async_busy(rx->fb, true);
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_submit_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                          const uint32_t *tv_sec, const uint32_t *tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_dgrams || !tv_sec || !tv_usec) return fail(SDRHIP_EINVAL, "rx_submit_datagrams: NULL count or stamp array");
    sdrhip::CtxLock lock_(rx->ctx);
    // ---- everything that can be refused is checked before anything is consumed
    const char *who = "rx_submit_datagrams";
    FecBufBatch in;
    if (int e = fecbuf_batch_check(&in, rx->nstreams, dgrams, n_dgrams, dgram_stride_bytes, who)) return e;
    return rx_submit_batch(rx, in, tv_sec, tv_usec, who);
}

// the same batch from an arrival-order array: the tags are walked (and refused) first, KX sorts the upload on the device
extern "C" int sdrhip_rx_submit_datagrams_tagged(sdrhip_rx *rx, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total,
                                                 const uint32_t *tv_sec, const uint32_t *tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!tv_sec || !tv_usec) return fail(SDRHIP_EINVAL, "rx_submit_datagrams_tagged: NULL stamp array");
    sdrhip::CtxLock lock_(rx->ctx);
    const char *who = "rx_submit_datagrams_tagged";
    FecBufBatch in;
    if (int e = fecbuf_batch_check_tagged(&in, rx->nstreams, dgrams, stream_of, n_total, who)) return e;
    return rx_submit_batch(rx, in, tv_sec, tv_usec, who);
}

extern "C" int sdrhip_rx_collect_datagrams(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames,
                                           size_t max_released, sdrhip_fecbuf_frame *info_out, size_t *n_released, size_t *n_frames, int wait)
{
    if (!rx || !n_released || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect_datagrams: NULL argument");
    // (the wait happens outside the context lock: the submitting thread -- the hub's reader thread -- keeps feeding the ring)
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    const int S = rx->nstreams;
    for (int s = 0; s < S; ++s) n_released[s] = n_frames[s] = 0;
    if (rx_has_batches(rx, false) || rx_has_batches(rx, true))
        return fail(SDRHIP_EINVAL, "rx_collect_datagrams: uniform or ragged batches are being filled or in flight: use sdrhip_rx_collect[_ragged]");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    // (a datagram batch goes out when it is submitted: none is ever being filled)
    int rc = rx->ring.wait_oldest(lock_, wait, "rx_collect_datagrams", [](sdrhip_rx::Batch &) { return SDRHIP_OK; }, &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    if (b.egress) return fail(SDRHIP_EINVAL, "rx_collect_datagrams: the batch was launched in departure order: use sdrhip_rx_collect_egress (the batch stays)");
    size_t most = 0, most_rel = 0, all = 0;
    for (int s = 0; s < S; ++s) {
        most = b.r_frames[(size_t)s] > most ? b.r_frames[(size_t)s] : most;
        most_rel = b.d_rel[(size_t)s] > most_rel ? b.d_rel[(size_t)s] : most_rel;
        all += b.r_frames[(size_t)s];
    }
    // (the batch stays where it is while the caller lacks room: the counts say how much it needs)
    const char *why = nullptr;
    if (most > max_frames) why = "a stream of the batch holds more frames than max_frames";
    else if (most_rel > max_released) why = "a stream of the batch released more frames than max_released";
    else if (most && S > 1 && frame_stride_bytes < most * b.frame_bytes) why = "frame stride too small for the stream with the most frames";
    else if (most && !frames_out) why = "NULL frames_out";
    else if (most_rel && !info_out) why = "NULL info_out";
    if (why) {
        for (int s = 0; s < S; ++s) { n_released[s] = b.d_rel[(size_t)s]; n_frames[s] = b.r_frames[(size_t)s]; }
        return fail(SDRHIP_EINVAL, "rx_collect_datagrams: %s (most frames %zu, most records %zu; the batch stays)", why, most, most_rel);
    }
    const uint8_t *src = b.out.as<uint8_t>(), *rec = src + all * b.frame_bytes;
    for (int s = 0; s < S; ++s) {
        const size_t row = b.r_frames[(size_t)s] * b.frame_bytes, k = b.d_rel[(size_t)s];
        if (row) memcpy(frames_out + (size_t)s * frame_stride_bytes, src, row);
        if (k) memcpy(info_out + (size_t)s * max_released, rec, k * DG_REC);
        src += row; rec += k * DG_REC;
        n_released[s] = k; n_frames[s] = b.r_frames[(size_t)s];
    }
    b.state = 0;
    b.dg = false;
    ++rx->ring.head;
    fecbuf_set_async_busy(rx->fb, rx_dgrams_in_flight(rx));
    return SDRHIP_OK;
}
