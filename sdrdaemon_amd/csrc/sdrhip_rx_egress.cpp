// sdrhip_rx_egress.cpp -- departure-order egress of the Rx pipe's asynchronous batches (sdrhip_rx_set_egress /
// sdrhip_rx_collect_egress / sdrhip_rx_release_egress).  A hub that sends what the stream-order collects hand it puts a burst per
// stream on the wire; the reference never does that to a receiver (UDPSinkFEC::transmitUDP sleeps txDelay between two datagrams of
// a stream, UDPSinkFEC.cpp:259-282).  With the order on, a batch's delivery is ONE array: datagram j of every stream before
// datagram j + 1 of any (rx_depart_order.h), with a stream tag per datagram -- the mirror of the tagged submit.  KR
// (rx_runs_kernels.hip) writes the batch's one download buffer in that order in KD's / the frame gather's place, run by run: one
// run per frame, or the pieces of the frames that another stream's end cuts (per-stream fecblk); the collect lends the ring
// slot's pinned download buffer and its tags instead of copying frames out of it.  The two launch paths
// (rx_submit_batch, rx_launch_ragged) call rx_egress_room ahead of everything that consumes input and rx_egress_launch where their
// stream-order delivery would go; nothing else of them differs.
// SDRHIP_EGRESS_PACED: the array in ascending departure key (2 j + 1) / (2 D_s) instead (rx_paced_order.h) -- what N senders that
// each space their own datagrams evenly put on the wire together; streams with unequal counts never burst.  Its destinations are
// no constant-stride runs, so KP (rx_paced_kernels.hip) gathers by destination through a table of one dword per datagram.
#include "sdrhip_pipes.h"

using namespace sdrhip;

namespace {
// KR's table: the record places (16 bytes each) in front, so that they are 16-byte aligned whatever the number of runs behind them
size_t runs_table_bytes(size_t runs, size_t S) { return S * sizeof(RxEgressRecPlace) + runs * sizeof(RxDepartRun); }
// the runs of a batch whose streams' frames differ in length (per-stream fecblk) at most: a frame each, and every stream's end cuts
// at most one frame of each other stream -- of the streams that deliver at all, min(S, frames) of them (quadratic in that number:
// 24 bytes a run, pinned per ring slot and on the device).  Equal frames: a run each
size_t depart_runs_bound(size_t frames, size_t S)
{
    const size_t live = frames < S ? frames : S;
    return frames + (live ? live * (live - 1) : 0);
}

// ... KP's, for a paced batch of either kind: a source per datagram
size_t paced_table_bytes(size_t dgrams, size_t S) { return S * sizeof(RxEgressRecPlace) + dgrams * sizeof(uint32_t); }

// the record places of a datagram batch, in front of every table; returns the records of the batch
uint32_t record_places(RxEgressRecPlace *place, size_t S, const int *released, size_t kmax)
{
    uint32_t pre = 0;
    for (size_t s = 0; s < S; ++s) {
        place[s].pre = pre;
        place[s].cnt = released && kmax ? (uint32_t)released[s * 4] : 0;
        place[s].pad[0] = place[s].pad[1] = 0;
        pre += place[s].cnt;
    }
    return pre;
}

// the batch the caller holds (state 3) is free again
void release_lent(sdrhip_rx *rx)
{
    for (auto &b : rx->ring.v)
        if (b.state == 3) b.state = 0;
}
} // namespace

int sdrhip::rx_egress_room(sdrhip_rx *rx, sdrhip_rx::Batch &b, size_t frames, size_t blocks_per_frame)
{
    // (per-stream fecblk with differing counts: the table of cut frames; blocks_per_frame = the slot pitch bounds the tags)
    const size_t S = (size_t)rx->nstreams;
    const bool mixed = rx_fec_mixed(rx);
    // (paced: the slot pitch bounds every frame's datagrams, so frames x blocks_per_frame bounds the table as it does the tags)
    const size_t bytes = (b.egress == SDRHIP_EGRESS_PACED ? paced_table_bytes(frames * blocks_per_frame, S)
                          : mixed                         ? runs_table_bytes(depart_runs_bound(frames, S), S)
                                                          : runs_table_bytes(frames, S)) + 16;
    int rc;
    if ((rc = b.e_tab.reserve(bytes))) return rc; // (waits for the table upload of this slot's last use)
    if ((rc = reserve_settled(rx->ctx, rx->e_tab, bytes))) return rc;
    try {
        b.e_tags.resize(frames * blocks_per_frame);
        // what the slot's previous batch left goes here, where the batch is launched: a batch that completes no frame never reaches
        // rx_egress_launch.  The batch keeps the counts it is launched with
        b.e_dgrams = 0;
        b.e_blocks.resize(mixed ? S : 0);
        for (size_t s = 0; s < b.e_blocks.size(); ++s) b.e_blocks[s] = rx_stream_blocks(rx, s);
    } catch (const std::bad_alloc &) {
        return fail(SDRHIP_ENOMEM, "rx egress: %zu tags", frames * blocks_per_frame);
    }
    return SDRHIP_OK;
}

hipError_t sdrhip::rx_egress_launch(sdrhip_rx *rx, sdrhip_rx::Batch &b, const size_t *n_frames, size_t frame_bytes, const int *released,
                                    size_t kmax, const uint8_t *records)
{
    sdrhip_ctx *c = rx->ctx;
    const size_t S = (size_t)rx->nstreams, B = frame_bytes / SDRHIP_UDPSIZE;
    // the order: round robin (the runs of rx_depart_order.h, moved by KR) or paced (one merge over the streams gives the tags and
    // KP's table).  each: rx_egress_room saw the streams' counts differ, and frame_bytes is the area's slot pitch
    const bool paced = b.egress == SDRHIP_EGRESS_PACED;
    const size_t *each = b.e_blocks.empty() ? nullptr : b.e_blocks.data();
    RxDepartOrder &d = rx->e_depart;
    RxPacedOrder &p = rx->e_paced;
    RxEgressRecPlace *place = b.e_tab.as<RxEgressRecPlace>();
    size_t n, bytes;
    try {
        std::vector<uint64_t> src0(S, 0);
        for (size_t s = 0; s < S; ++s)
            if (n_frames[s]) src0[s] = rx->view.offset(s, frame_bytes);
        // (a batch the order's index types cannot hold: refused, never truncated)
        if (!(paced ? (each ? p.plan(n_frames, each, S) : p.plan(n_frames, B, S)) : (each ? d.plan(n_frames, each, S) : d.plan(n_frames, B, S))))
            return hipErrorInvalidValue;
        n = (size_t)(paced ? p.dgrams() : d.dgrams());
        bytes = paced ? paced_table_bytes(n, S) : runs_table_bytes(d.nruns(), S);
        // (cannot differ: rx_egress_room was given the pipe's own count of these frames, and reserved the bound on their runs)
        if (bytes > b.e_tab.cap || n > b.e_tags.size()) return hipErrorInvalidValue;
        b.e_tags.resize(n); // (never grows)
        if (paced) {
            if (!p.fill(src0.data(), frame_bytes, b.e_tags.data(), reinterpret_cast<uint32_t *>(place + S))) return hipErrorInvalidValue;
        } else {
            if (!d.runs(src0.data(), frame_bytes, reinterpret_cast<RxDepartRun *>(place + S))) return hipErrorInvalidValue;
            d.tags(b.e_tags.data());
        }
    } catch (const std::bad_alloc &) {
        return hipErrorOutOfMemory;
    }
    b.e_dgrams = n;
    const uint32_t pre = record_places(place, S, released, kmax);
    if (!n && !pre) return hipSuccess;
    if (kmax > 0xffffffffu / S) return hipErrorInvalidValue;
    hipError_t e = hipMemcpyAsync(rx->e_tab.p, b.e_tab.p, bytes, hipMemcpyHostToDevice, c->stream); // (not counted: a table)
    if (e != hipSuccess) return e;
    b.e_tab.mark(c->stream);
    RxEgressRecords rec;
    rec.place = rx->e_tab.as<RxEgressRecPlace>();
    rec.records = records;
    rec.dst = (uint64_t)n * SDRHIP_UDPSIZE;
    rec.kmax = (uint32_t)kmax;
    rec.nslots = pre ? (uint32_t)(S * kmax) : 0;
    KTimer kt(c, SDRHIP_K_CONVERT);
    if (paced) return launch_rx_paced(reinterpret_cast<const uint32_t *>(rec.place + S), n, rx->work.as<uint8_t>(), rx->a_frames.as<uint8_t>(), rec, c->stream);
    return launch_rx_runs(reinterpret_cast<const RxDepartRun *>(rec.place + S), d.nruns(), d.wg_per_run(), rx->work.as<uint8_t>(),
                          rx->a_frames.as<uint8_t>(), rec, c->stream);
}

extern "C" int sdrhip_rx_set_egress(sdrhip_rx *rx, int order)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (order != SDRHIP_EGRESS_OFF && order != SDRHIP_EGRESS_ROUND_ROBIN && order != SDRHIP_EGRESS_PACED)
        return fail(SDRHIP_EINVAL, "rx_set_egress: unknown order %d", order);
    if ((size_t)rx->nstreams > RX_EGRESS_MAX_STREAMS) return fail(SDRHIP_EINVAL, "rx_set_egress: a tag names at most 65535 streams");
    if (rx->ring.any([](const sdrhip_rx::Batch &b) { return b.state == 1; }))
        return fail(SDRHIP_EINVAL, "rx_set_egress: a batch is being filled: collect it first");
    rx->egress = order;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_collect_egress(sdrhip_rx *rx, sdrhip_rx_egress *out, size_t *n_frames, size_t max_released,
                                        sdrhip_fecbuf_frame *info_out, size_t *n_released, int wait)
{
    if (!rx || !out || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect_egress: NULL argument");
    // (the wait happens outside the context lock: the submitting thread keeps feeding the ring)
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    const int S = rx->nstreams;
    for (int s = 0; s < S; ++s) {
        n_frames[s] = 0;
        if (n_released) n_released[s] = 0;
    }
    if (rx_has_batches(rx, false)) return fail(SDRHIP_EINVAL, "rx_collect_egress: uniform batches are being filled or in flight: use sdrhip_rx_collect");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    int rc = rx->ring.wait_oldest(lock_, wait, "rx_collect_egress", [rx](sdrhip_rx::Batch &f) { return rx_launch_filling(rx, f); }, &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    if (!b.egress)
        return fail(SDRHIP_EINVAL, "rx_collect_egress: the batch was launched in stream order: use sdrhip_rx_collect_%s (the batch stays)",
                    b.dg ? "datagrams" : "ragged");
    size_t all = 0, most_rel = 0;
    for (int s = 0; s < S; ++s) {
        all += b.r_frames[(size_t)s];
        if (b.dg && b.d_rel[(size_t)s] > most_rel) most_rel = b.d_rel[(size_t)s];
    }
    const char *why = nullptr;
    if (b.dg && !n_released) why = "NULL n_released for a datagram batch";
    else if (most_rel > max_released) why = "a stream of the batch released more frames than max_released";
    else if (most_rel && !info_out) why = "NULL info_out";
    if (why) { // (the batch stays where it is: the counts say how much room it needs)
        for (int s = 0; s < S; ++s) {
            n_frames[s] = b.r_frames[(size_t)s];
            if (n_released) n_released[s] = b.dg ? b.d_rel[(size_t)s] : 0;
        }
        return fail(SDRHIP_EINVAL, "rx_collect_egress: %s (most records %zu; the batch stays)", why, most_rel);
    }
    // (per-stream fecblk with differing counts: blocks_per_frame = 0, sdrhip_rx_egress_stream_blocks has each stream's)
    const bool each = !b.e_blocks.empty();
    const size_t B = each ? 0 : b.frame_bytes / SDRHIP_UDPSIZE, n = each ? b.e_dgrams : all * B;
    // the records alone are copied (16 bytes per released frame); the datagrams and the tags are lent where they lie
    const uint8_t *rec = b.out.as<uint8_t>() + n * SDRHIP_UDPSIZE;
    for (int s = 0; s < S; ++s) {
        const size_t k = b.dg ? b.d_rel[(size_t)s] : 0;
        if (k) memcpy(info_out + (size_t)s * max_released, rec, k * DG_REC);
        rec += k * DG_REC;
        n_frames[s] = b.r_frames[(size_t)s];
        if (n_released) n_released[s] = k;
    }
    release_lent(rx); // (a successful collect releases what the previous one lent)
    out->dgrams = n ? b.out.as<uint8_t>() : nullptr;
    out->stream_of = n ? b.e_tags.data() : nullptr;
    out->n_dgrams = n;
    out->blocks_per_frame = B;
    const bool was_dg = b.dg;
    b.state = 3;
    b.dg = false;
    ++rx->ring.head;
    if (was_dg) fecbuf_set_async_busy(rx->fb, rx_dgrams_in_flight(rx));
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_egress_stream_blocks(const sdrhip_rx *rx, size_t *blocks)
{
    if (!rx || !blocks) return fail(SDRHIP_EINVAL, "rx_egress_stream_blocks: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    for (const auto &b : rx->ring.v) {
        if (b.state != 3) continue;
        for (size_t s = 0; s < (size_t)rx->nstreams; ++s) blocks[s] = b.e_blocks.empty() ? b.frame_bytes / SDRHIP_UDPSIZE : b.e_blocks[s];
        return SDRHIP_OK;
    }
    return fail(SDRHIP_EINVAL, "rx_egress_stream_blocks: no batch is lent (sdrhip_rx_collect_egress)");
}

extern "C" int sdrhip_rx_release_egress(sdrhip_rx *rx)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    release_lent(rx);
    return SDRHIP_OK;
}
