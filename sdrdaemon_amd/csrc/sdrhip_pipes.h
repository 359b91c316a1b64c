// sdrhip_pipes.h -- the fused Rx / Tx pipes of include/sdrhip.h: their handles (every buffer, event and ring a member that owns
// what it holds: dev_buffers.h, the ring of asynchronous batches among them) and what the units sdrhip_rx.cpp, sdrhip_rx_async.cpp,
// sdrhip_rx_datagrams.cpp, sdrhip_rx_datagrams_async.cpp, sdrhip_tx.cpp and
// sdrhip_tx_async.cpp share.  The Rx pipe's host decisions live in headers of their own: rx_frame_area.h (windows),
// rx_stream_settings.h (per-stream settings, the counts of a ragged step and of a join), rx_depart_order.h and rx_paced_order.h
// (departure orders), rx_step_plan.h (what a step launches)
#pragma once
#include "rx_depart_order.h"
#include "rx_frame_area.h"
#include "rx_paced_order.h"
#include "rx_step_plan.h"
#include "rx_stream_settings.h"
#include "sdrhip_host.h"

#include <cstring>
#include <new>

// --------------------------------------------------------------------------- fused Rx pipe
namespace sdrhip {
// pinned staging of the ragged step's two host tables (the decimator's rows, the encoder's frame list).  The handle owns one pair,
// whose reuse waits for the previous call's upload; a datagram batch brings its ring slot's pair (rx_ragged's `tabs`)
struct RxTabs { PinnedBuf rows, flist; };
// the kind of a ragged step.  batch: a ragged asynchronous batch (rx_launch_ragged): int16 device rows that K0p laid out, whatever
// the input format.  dev_rows: iq_in is int16 device rows whatever `mem` and the input format are (the datagram entries' rows); `mem`
// then speaks of frames_out alone.  tabs: the ring slot's staging instead of the handle's.  follow (the datagram entries with
// sdrhip_rx_set_follow_meta on): the collector's committed state on the device; KF forms the meta words of the streams that have
// incoming meta from it, behind the table's upload.  follow_bits (sdrhip_rx_set_follow_bits on): the same state; KFb, in front of
// KF, forms the shift pair, the third meta word and the CRC of the streams that have an incoming sample size
struct RxRaggedCall {
    bool batch, dev_rows;
    RxTabs *tabs;
    const FecBufState *follow, *follow_bits;
};
// where a step delivers: the caller's buffer (`mem` memory; NULL: the view alone) and the per-stream frame counts
struct RxFramesOut {
    uint8_t *frames;
    size_t stride_bytes;
    size_t *n_frames;
    int mem;
};
} // namespace sdrhip
struct sdrhip_rx {
    sdrhip::CtxRef ctx; // (first: released last -- the pipe's own reference, whatever its banks hold)
    int nstreams;
    sdrhip_rx_config cfg;
    sdrhip_decimators *dec = nullptr;
    explicit sdrhip_rx(sdrhip_ctx *c) : ctx(c) {}
    // [nstreams][area.cap()][128 + nb_fec][512] (per-stream fecblk: 128 + the largest count, rx_frame_bytes).  A call fills slots area.slot(s) .. area.slot(s) + done of stream s; the frame
    // still being filled is the first slot of the next call, so the window slides and nothing is copied until it reaches the end
    // of the area.  `area` decides where the windows go (rx_frame_area.h), rx_run_plan moves the open frames there
    sdrhip::DevBuf work;
    sdrhip::RxFrameArea area;
    sdrhip::RxView view;      // what sdrhip_rx_frames_view / _ragged show: the frames the last call DELIVERED
    sdrhip::DevBuf lin[2];    // stream-order decimator output of a call that is framed by K2 (two: pipelined mode)
    int lin_sel = 0;
    sdrhip::DevBuf flist;     // frame list of the generic encode launch (device), relative to the window
    std::vector<int32_t> flist_host;
    size_t flist_done = 0, flist_cap = 0;
    // ---- pipelined mode (sdrhip_rx_set_pipelined): a call delivers the frames the PREVIOUS call completed; their
    // recovery blocks are computed by encoder workgroups inside this call's decimator launch (rx_fused_kernel)
    int pipelined = 0;
    struct Late {
        bool have = false;          // frames completed by the previous call wait for delivery
        bool encode = false;        // ... and still have to be encoded (k)
        sdrhip::Enc128Args k;
        const uint8_t *area = nullptr; // the area they lie in, from slot `first` of every stream on
        size_t first = 0, stride = 0, frames = 0, frame_bytes = 0;
        bool in_old = false;        // that area is old_work (the windows got a new one meanwhile)
    } late;
    sdrhip::DevBuf old_work;  // the previous frame area after a re-allocation, kept while `late` points into it
    // overlap mode (option rx_fused = 3): the waiting encode runs on the context's second stream beside the next call's decimator.
    // ev_framed: recorded on the first stream when a call has written everything its deferred encode reads (decimator + K2);
    // ev_enc: recorded on the second stream behind the encode, the first stream waits for it before the frames are delivered
    sdrhip::DevEvent ev_framed, ev_enc;
    // ---- asynchronous host-pointer entry (sdrhip_rx_submit / sdrhip_rx_collect): a ring of batches
    struct Batch {
        sdrhip::PinnedBuf in;     // the submitted blocks, appended: [block][stream][n] (unless the caller's memory is pinned by us)
        sdrhip::DevBuf din;       // [stream][dstride] on the device
        sdrhip::PinnedBuf out;    // the batch's finished frames [stream][frames][128 + R][512]
        sdrhip::DevEvent done;
        std::vector<std::pair<const int16_t *, size_t> > blocks; // source of each block (host address, samples per stream) and
        std::vector<size_t> strides;                             // its stream stride in samples
        size_t n_in = 0;          // samples per stream so far
        size_t in_cap = 0;        // row length of `in` in samples: staged blocks lie stream-major, [stream][in_cap], at their batch offset
        uint32_t tv_sec = 0, tv_usec = 0;
        size_t frames = 0, frame_bytes = 0;
        int state = 0;            // 0 free, 1 filling, 2 in flight, 3 lent (collected by sdrhip_rx_collect_egress, not yet released)
        // ---- a ragged batch (sdrhip_rx_submit_ragged; a batch holds one kind only): blocks of per-stream counts, packed
        bool ragged = false;
        struct Run { const char *p; size_t off, bytes; }; // packed bytes of one block: in place at p, or staged at `in` + off (p NULL)
        std::vector<Run> r_runs;
        std::vector<size_t> r_cnt;            // [block][stream] counts
        std::vector<size_t> r_tot;            // per-stream samples so far
        std::vector<uint32_t> r_sec, r_usec;  // the stamps of the batch's first block
        size_t r_used = 0;                    // staged bytes in `in`
        std::vector<size_t> r_frames;         // frames per stream of the launched batch, in stream order in `out`
        sdrhip::PinnedBuf r_tab;              // K0p's table, then the frame list of the download
        // ---- a batch of raw datagrams (sdrhip_rx_submit_datagrams; the third kind, never being filled: one submit is one batch):
        // `in` holds them packed, r_tab the collector's tables, d_seg the delivery's segments, `out` the gathered delivery (every
        // stream's r_frames[s] frames, then every stream's d_rel[s] records)
        // d_tabs = the ragged step's row table and frame list, per slot: a submit waits for its own slot's last use, never for
        // the previous batch
        bool dg = false;
        sdrhip::PinnedBuf d_seg;
        sdrhip::RxTabs d_tabs;
        std::vector<size_t> d_rel;            // released frames (records) per stream
        // ---- departure-order egress (sdrhip_rx_set_egress; a ragged or a datagram batch): the order the batch was launched with,
        // KR's table (the record places, then the runs; SDRHIP_EGRESS_PACED: KP's, a dword per datagram), and the
        // tags the collect lends beside `out`
        int egress = 0;
        sdrhip::PinnedBuf e_tab;
        std::vector<uint16_t> e_tags;
        // (per-stream fecblk, sdrhip_rx_set_stream_fec with differing counts: the super blocks per frame of every stream the batch
        // was launched with, and the datagrams of its array; empty: every frame holds frame_bytes / 512)
        std::vector<size_t> e_blocks;
        size_t e_dgrams = 0;
    };
    sdrhip::BatchRing<Batch> ring;
    // ragged batches on the device: packed upload, K0p's rows, tables, compacted frames (datagram batches: the packed datagrams in
    // a_pk, the delivery's segments in a_tab, the gathered delivery in a_frames)
    sdrhip::DevBuf a_pk, a_din, a_tab, a_frames;
    int a_blocks = 1;             // blocks per launch
    // ---- departure-order egress (sdrhip_rx_set_egress): the order later launches get, and the order's table on the device
    int egress = 0;
    sdrhip::DevBuf e_tab;
    sdrhip::RxDepartOrder e_depart; // (SDRHIP_EGRESS_ROUND_ROBIN, equal frames or not: rx_depart_order.h)
    sdrhip::RxPacedOrder e_paced;   // (SDRHIP_EGRESS_PACED, either kind of batch: rx_paced_order.h)
    bool consumed = false;        // set by sdrhip_rx_process once the decimator launch of the call went out (the filter state advanced)
    // ---- input format (sdrhip_rx_set_input_format): 8-bit input is widened by K0 into `wide`, the decimator's int16 input
    int in_fmt = sdrhip::IQF_S16;
    sdrhip::DevBuf wide;
    // ---- per-stream input format (sdrhip_rx_set_stream_format; the array itself is `streams`'): K0x's table of a synchronous ragged
    // call on its way up, and the staged host rows (packed, each n * bytes(fmt) long) with their upload; K0x writes `wide`
    sdrhip::PinnedBuf f_tab_pin, f_pin;
    sdrhip::DevBuf f_tab, f_pk;
    // ---- ragged calls (sdrhip_rx_process_ragged)
    sdrhip::PinnedBuf r_pin, r_flist_pin; // host-row staging and the encoder's frame list
    sdrhip::DevBuf r_flist;
    // ---- per-stream centre frequency / sample rate, fecblk and sample size (sdrhip_rx_set_stream_meta / _fec / _bits): the arrays,
    // what they force and the streams' records are rx_stream_settings.h's; a setter touches the host arrays alone, the next launch
    // forms the records.  Ragged launches carry them in their row table.  Uniform launches read a device table: a change goes up in
    // front of the launch, on the context's stream, from the next of four pinned versions into the device table the previous version
    // does NOT occupy -- launches in flight keep the table they were enqueued with, a deferred encode (late.k) keeps its pointer.
    // Per-stream fecblk: the frame area keeps ONE slot pitch, 128 + the largest count (rx_frame_bytes), a frame of stream s holds
    // rx_stream_blocks(rx, s) valid super blocks at the head of its slot
    sdrhip::RxStreamSettings streams;
    sdrhip::TableVersions sm_tab;
    // ---- datagram entry (sdrhip_rx_process_datagrams): one SDRdaemonFECBuffer per stream, created on first use; it delivers into
    // j_rows ([nstreams][j_row_len] samples, the ragged step's input), behind the samples each row holds back from earlier calls
    // (their counts live with the collector: fecbuf_join_carry)
    sdrhip_fecbuf *fb = nullptr;
    sdrhip::DevBuf j_rows;
    size_t j_row_len = 0;
    // ---- outgoing meta from the incoming meta blocks (sdrhip_rx_set_follow_meta): a host flag, read by the datagram entries per call
    // and per batch at its submit; KF (rx_follow_kernels.hip) then rewrites the rows of the streams that have incoming meta
    int follow_meta = 0;
    // ---- the sample size from the incoming meta blocks (sdrhip_rx_set_follow_bits): its twin, independent of it; KFb
    // (rx_follow_bits_kernels.hip) rewrites the shift pair, the third meta word and the CRC of the streams that have an incoming size
    int follow_bits = 0;
    // ---- per-stream lifecycle (sdrhip_rx_reset_streams): the mask's versions on their way up; sdrhip_rx_export_stream /
    // _import_stream: the contiguous device blob KG packs / KS unpacks, and the pinned staging of an import's upload
    sdrhip::StreamMask reset_mask;
    sdrhip::DevBuf x_blob;
    sdrhip::PinnedVersions x_pin; // (four versions: an import waits for the upload four imports back, not for the previous one)
};

// --------------------------------------------------------------------------- fused Tx pipe
struct sdrhip_tx {
    sdrhip::CtxRef ctx; // (first: released last -- the pipe's own reference, whatever its banks hold)
    int nstreams;
    int log2interp;
    sdrhip_interpolators *itp = nullptr;
    explicit sdrhip_tx(sdrhip_ctx *c) : ctx(c) {}
    sdrhip::DevBuf rxbuf, payload[2], outbuf;
    sdrhip::DevBuf srcmap, restored; // no-copy mode (tx_gather): the decoder's position map and restored blocks, read by K5w's gather variant
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
    sdrhip::DevBuf plan_own, idx_own;
    sdrhip::PinnedBuf pin_own;
    sdrhip::DevEvent ev_in;                  // first stream: the caller's device rx buffer is ready
    sdrhip::DevEvent ev_up;                  // second stream: the upload of the caller's HOST rx buffer has read it (the call returns behind it)
    sdrhip::DevEvent ev_dec;                 // second stream: the waiting batch is decoded
    sdrhip::DevEvent ev_itp[2];              // first stream: the interpolator has read payload[i]
    bool itp_pending[2] = {false, false};
    // ---- asynchronous host-pointer entry (sdrhip_tx_submit / sdrhip_tx_collect): a ring of batches of received frames
    struct ABatch {
        sdrhip::PinnedBuf in;        // the batch's received super blocks [stream][frame][128][512] (staged; sdrhip_host_alloc memory is used in place)
        sdrhip::DevBuf din, dout, db0; // ... on the device; its samples [stream][dos]; its meta blocks [stream * nframes][508]
        sdrhip::PinnedBuf out;       // samples, then meta blocks, downloaded
        sdrhip::DevEvent done;
        size_t nframes = 0, n_res = 0, dos = 0;
        int state = 0;            // 0 free, 2 in flight
        // a batch of raw datagrams (sdrhip_tx_submit_datagrams): `in` holds them packed, `out` the gathered delivery (every
        // stream's samples, then the records, then the meta blocks); tab / seg = its collector tables and gather segments
        bool dg = false;
        sdrhip::PinnedBuf tab, seg;
        std::vector<size_t> frames; // released frames per stream
        int log2interp = 0;
        // bytes per output sample of every stream, as the batch was handed in.  rows4 (sdrhip_tx_set_stream_format's array was set):
        // the caller's row s starts 4 * s * out_stride bytes into iq_out, and a batch of received frames lies packed in `out` too
        std::vector<uint8_t> esz;
        bool rows4 = false;
    };
    sdrhip::BatchRing<ABatch> ring;
    // device buffers of the datagram batches, shared by the ring (the context's stream orders the batches): the packed datagrams,
    // the collector's [stream][pitch] rows, the interpolator's output rows, the meta blocks, the gathered delivery, its segments
    sdrhip::DevBuf a_pk, a_pay, a_out, a_b0, a_gat, a_seg;
    // ---- datagram entry (sdrhip_tx_process_datagrams): one SDRdaemonFECBuffer per stream, created on first use; the frames it
    // releases go to payload[0] (or straight to the caller's device iq_out when log2interp = 0), the interpolator reads them there
    sdrhip_fecbuf *fb = nullptr;
    // ---- output format (sdrhip_tx_set_output_format): IQF_S8 = 2-byte samples from the interpolator's last stage (or K6n for x1)
    int out_fmt = sdrhip::IQF_S16;
    // ---- per-stream output format (sdrhip_tx_set_stream_format): the host array (empty: bank-wide, out_fmt) and its version; K5x /
    // K6x read one int per stream from a device table, which goes up on the context's stream in front of the first launch that
    // finds its version changed (tx_format_table).  The setter touches s_fmt / s_fmt_ver alone
    std::vector<int> s_fmt;
    uint64_t s_fmt_ver = 0, s_fmt_up = 0; // versions of the array: as set / as uploaded (0: none yet)
    sdrhip::TableVersions s_fmt_tab;
    // ---- per-stream lifecycle (sdrhip_tx_reset_streams): the mask's versions on their way up; sdrhip_tx_export_stream /
    // _import_stream: the contiguous device blob KG packs / KS unpacks, and the pinned staging of an import's upload
    sdrhip::StreamMask reset_mask;
    sdrhip::DevBuf x_blob;
    sdrhip::PinnedVersions x_pin; // (four versions: an import waits for the upload four imports back, not for the previous one)
};

namespace sdrhip {
static_assert(RX_FRAME_SAMPLES == SDRHIP_SAMPLES_PER_FRAME, "rx_frame_area.h frames the header's frame");
static_assert(RX_STEP_FRAME_SAMPLES == SDRHIP_SAMPLES_PER_FRAME && RX_STEP_FC_CEN == SDRHIP_FC_CEN && RX_STEP_GROUP == GF_FRAMES_PER_GROUP, "rx_step_plan.h");
static_assert(RX_NB_ORIGINAL == SDRHIP_NB_ORIGINAL && RX_UDPSIZE == SDRHIP_UDPSIZE && RX_STREAM_WORDS == STREAM_META_WORDS, "rx_stream_settings.h");
// the bank-wide values rx_stream_settings.h resolves against, and its answers for this pipe: the count and the sample size of
// stream s (as its source delivers it: the decimator's input), the largest count, whether two differ; bytes of a slot of the frame
// area (the ONE pitch) and of the valid super blocks of a frame of stream s
inline RxBankValues rx_bank(const sdrhip_rx *rx)
{
    const RxBankValues b = {rx->cfg.center_frequency_khz, rx->cfg.sample_rate, rx->cfg.nb_fec, (unsigned)rx->cfg.sample_bits, rx->cfg.log2decim};
    return b;
}
inline int rx_fec_of(const sdrhip_rx *rx, size_t s) { return rx->streams.fec(rx_bank(rx), s); }
inline int rx_fec_max(const sdrhip_rx *rx) { return rx->streams.fec_max(rx_bank(rx)); }
inline bool rx_fec_mixed(const sdrhip_rx *rx) { return rx->streams.fec_mixed(); }
inline unsigned rx_bits_of(const sdrhip_rx *rx, size_t s) { return rx->streams.bits(rx_bank(rx), s); }
inline size_t rx_frame_bytes(const sdrhip_rx *rx) { return rx->streams.slot_blocks(rx_bank(rx)) * SDRHIP_UDPSIZE; }
inline size_t rx_stream_blocks(const sdrhip_rx *rx, size_t s) { return rx->streams.stream_blocks(rx_bank(rx), s); }
inline size_t rx_stream_bytes(const sdrhip_rx *rx, size_t s) { return rx_stream_blocks(rx, s) * SDRHIP_UDPSIZE; }
// what a ragged step will complete and deliver for the counts n_in[s], as the pipe stands
inline RxRaggedCounts rx_counts(const sdrhip_rx *rx, const size_t *n_in) { return rx_ragged_counts(rx->area, rx->streams, rx_bank(rx), n_in); }
// the uniform entries (`who`) while an array forces the ragged step: `instead` = the entry to use (NULL: there is none, pipelined mode)
inline int rx_refuse_uniform(const char *who, const char *instead, RxSetting forced)
{
    if (forced == RX_SET_NONE) return SDRHIP_OK;
    const char *what = forced == RX_SET_FEC    ? "per-stream fecblk is set (sdrhip_rx_set_stream_fec)"
                       : forced == RX_SET_BITS ? "per-stream sample bits are set (sdrhip_rx_set_stream_bits)"
                                               : "per-stream input formats are set (sdrhip_rx_set_stream_format)";
    return instead ? fail(SDRHIP_EINVAL, "%s: %s: use %s", who, what, instead) : fail(SDRHIP_EINVAL, "%s: %s: every step is the ragged step", who, what);
}
// a delivery of these counts that the caller's frames_out cannot take (`unconsumed`: the entry says that nothing was consumed)
inline int rx_refuse_delivery(const char *who, const RxRaggedCounts &n, const uint8_t *frames_out, size_t frame_stride_bytes, int mem, bool unconsumed)
{
    if (n.max_done && !frames_out && mem != SDRHIP_MEM_DEVICE) return fail(SDRHIP_EINVAL, "%s: NULL frames_out", who);
    if (frames_out && n.done.size() > 1 && n.max_done && frame_stride_bytes < n.max_row)
        return fail(SDRHIP_EINVAL, "%s: frame stride too small: the longest stream's frames take %zu bytes (%zu frames at most%s)", who, n.max_row, n.max_done,
                    unconsumed ? "; nothing was consumed" : "");
    return SDRHIP_OK;
}
// batches of the ring that are being filled or in flight, of the ragged (or the uniform) kind.  (A lent batch -- state 3 -- is
// neither: it was collected, and only its slot is still taken.)
inline bool rx_has_batches(const sdrhip_rx *rx, bool ragged)
{
    return rx->ring.any([ragged](const sdrhip_rx::Batch &b) { return b.state != 3 && !b.dg && b.ragged == ragged; });
}
// ... of the datagram kind (sdrhip_rx_submit_datagrams): every other entry that moves the pipe is refused meanwhile
inline bool rx_dgrams_in_flight(const sdrhip_rx *rx)
{
    return rx->ring.any([](const sdrhip_rx::Batch &b) { return b.state != 3 && b.dg; });
}
// ... of any kind: what the synchronous entries wait for (ring.busy() counts lent batches as well: the slots are taken)
inline bool rx_batches_active(const sdrhip_rx *rx)
{
    return rx->ring.any([](const sdrhip_rx::Batch &b) { return b.state != 3; });
}
// samples a datagram call feeds the decimator in one piece: 2^log2decim, but 4 for decimate2_inf / _sup, which walk their input in
// fours (Decimators.cpp:48,76) -- the datagram entries never hand them a tail of 2
inline size_t rx_join_unit(const sdrhip_rx_config &cfg)
{
    return cfg.log2decim == 1 && cfg.fcpos != SDRHIP_FC_CEN ? 4 : (size_t)1 << cfg.log2decim;
}
// the datagram entries' rows (j_rows): room for 63 samples held back and max_released payloads behind them.  Rows that grow keep
// their heads and grow behind a synchronisation (earlier launches may still use the old rows)
int rx_join_rows(sdrhip_rx *rx, size_t max_released, const char *who);
// the ragged step (sdrhip_rx_process_ragged), of the kind `call` names (none: the caller's own rows, in the pipe's input format).
// n = rx_counts() of the call's counts, taken while the pipe stands where this call finds it
int rx_ragged(sdrhip_rx *rx, const int16_t *iq_in, const RxRaggedCounts &n, size_t in_stride, const uint32_t *tv_sec, const uint32_t *tv_usec,
              const RxFramesOut &out, const RxRaggedCall &call = RxRaggedCall());
// everything the ragged step allocates for these counts, ahead of it (a caller that must not fail between two launches): the frame
// area (grown behind a synchronisation), the tables, the frame list, and the stream-order rows when the decimator's plan for these
// counts does not store straight into the windows (the step's own decision: rx_step_plan.h).  rx_ragged itself then allocates nothing
int rx_ragged_room(sdrhip_rx *rx, const RxRaggedCounts &n, RxTabs *tabs);
// ---- the unpack pass (K0p / K0x) of the two sample-fed entries that have one: a ragged batch and the synchronous per-stream-format call
// rx_pack_rows: S rows of n_in[s] * bytes(fmt) bytes back to back at dst, fmt = fmts[s] or (fmts NULL) bank_fmt.  Row s is read at
// src + s * pitch, or (pitch 0) where the row before it ended: an empty row is skipped, a strided row's padding never read
void rx_pack_rows(char *dst, const void *src, size_t pitch, const size_t *n_in, const int *fmts, int bank_fmt, size_t S);
// rx_unpack_launch: the table of rx_unpack_plan.h that stands in `pin` (S + 1 rows, then the segments: tab_bytes in all) goes up into
// `dev`, then K0x (fmts set) or K0p (NULL: the bank's format) lays `src` out as out[S][dstride] with `grid` workgroups
int rx_unpack_launch(sdrhip_rx *rx, PinnedBuf &pin, DevBuf &dev, size_t tab_bytes, const int *fmts, const void *src, int16_t *out, size_t dstride,
                     unsigned grid);
int rx_collector(sdrhip_rx *rx); // the datagram collector, created on first use
// a uniform or ragged batch that is still being filled goes out as it is (wait_oldest's launch_filling; sdrhip_rx_async.cpp)
int rx_launch_filling(sdrhip_rx *rx, sdrhip_rx::Batch &b);
// ---- departure-order egress (sdrhip_rx_egress.cpp), for a launch path whose batch has an order (b.egress).  rx_egress_room:
// everything the launch needs for a batch of at most `frames` delivered frames of blocks_per_frame datagrams -- the slot's pinned
// table and tags, the device table -- ahead of anything that consumes input (a device table that grows synchronises once).
// rx_egress_launch: the runs, the record places and the tags from the delivered counts n_frames[s] (each stream's frames contiguous
// in `work` from view.offset(s, frame_bytes)), the table's upload, and KR into a_frames: the datagrams in departure order, then --
// a datagram batch: released = the collector's [S][4] results, records = its public records [S][kmax] -- the records as KD lays
// them out.  The table, the tags and the device table are rx_egress_room's; the order's own vectors (one entry per run) are the
// handle's and keep their capacity.  The runs are rx_depart_order.h's: one per frame, or -- per-stream fecblk with differing counts
// (rx_fec_mixed): frame_bytes / blocks_per_frame are the slot pitch -- at most frames + S (S - 1); b.e_blocks / b.e_dgrams say so.
// SDRHIP_EGRESS_PACED (b.egress, either kind of batch): the table is rx_paced_order.h's -- the record places, then 4 bytes per
// datagram -- and KP moves the datagrams
int rx_egress_room(sdrhip_rx *rx, sdrhip_rx::Batch &b, size_t frames, size_t blocks_per_frame);
hipError_t rx_egress_launch(sdrhip_rx *rx, sdrhip_rx::Batch &b, const size_t *n_frames, size_t frame_bytes, const int *released, size_t kmax,
                            const uint8_t *records);
// the frame area made ready for a ragged step that completes done[s] frames of stream s (NULL: none -- a slot per stream for
// sdrhip_rx_import_stream into a bank that never ran): plan, new area or in-place moves
int rx_area_room(sdrhip_rx *rx, const size_t *done);

// ---- Tx: bytes per output sample, and the row pitch (samples) of the library's own output buffers: 16-byte rows either way
inline size_t tx_esz(const sdrhip_tx *tx) { return tx->out_fmt == IQF_S8 ? 2 : 4; }
inline size_t tx_pitch(const sdrhip_tx *tx, size_t n) { return tx->out_fmt == IQF_S8 ? (n + 7) & ~(size_t)7 : (n + 3) & ~(size_t)3; }
// ---- per-stream output format (sdrhip_tx_set_stream_format).  tx_formats: the array is set.  Then: tx_esz(tx, s) = bytes per sample
// of stream s, and every row -- the caller's and the library's own -- starts 4 * s * stride bytes into its buffer, the stride in
// 4-byte units; tx_pitch4 = the stride of the library's own rows, a multiple of 4 (16-byte rows).  Unset, tx_esz(tx, s) is tx_esz(tx)
inline bool tx_formats(const sdrhip_tx *tx) { return !tx->s_fmt.empty(); }
inline size_t tx_esz(const sdrhip_tx *tx, size_t s) { return tx_formats(tx) ? (tx->s_fmt[s] == IQF_S8 ? 2 : 4) : tx_esz(tx); }
inline size_t tx_pitch4(size_t n) { return (n + 3) & ~(size_t)3; }
// row pitch and bytes per pitch unit of the library's own output rows, whichever mode the handle is in
inline size_t tx_own_pitch(const sdrhip_tx *tx, size_t n) { return tx_formats(tx) ? tx_pitch4(n) : tx_pitch(tx, n); }
inline size_t tx_unit(const sdrhip_tx *tx) { return tx_formats(tx) ? 4 : tx_esz(tx); }
// a device output the interpolator may store to with 16-byte stores: aligned, the stride a multiple of 4 (int16) / 8 (8-bit)
// samples; with the array set, a multiple of 4 of its 4-byte units
inline bool tx_out_aligned(const sdrhip_tx *tx, const void *p, size_t stride)
{
    return aligned16(p) && (tx->nstreams == 1 || (stride & (!tx_formats(tx) && tx->out_fmt == IQF_S8 ? 7 : 3)) == 0);
}
// the device table of the array (NULL while it is unset): uploaded on the context's stream when its version changed
int tx_format_table(sdrhip_tx *tx, const int **fmt_dev);
// rows of the library's own device buffer `dout` (pitch `dos` units of tx_unit) to the caller's host rows (out_stride units), n[s]
// samples of stream s (n NULL: n_all each): one link copy per run of adjacent rows of equal format and length -- exactly
// sum n[s] * tx_esz(tx, s) bytes cross the link
hipError_t tx_download_rows(sdrhip_tx *tx, void *iq_out, size_t out_stride, const void *dout, size_t dos, const size_t *n, size_t n_all);
// asynchronous batches of one kind in flight: raw datagrams (dg) or received frames
inline bool tx_in_flight(const sdrhip_tx *tx, bool dg)
{
    return tx->ring.any([dg](const sdrhip_tx::ABatch &b) { return b.dg == dg; });
}
// decode S x nframes frames into `pay` ([S][pstride] samples): one batch, or one call per stream when the rows are padded
int tx_decode(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, DevBuf &pay, size_t pstride, const DecodeSide *side,
              uint8_t *block0 = nullptr); // block0 (optional, device): [stream * nframes][508], the frames' meta blocks
bool tx_gather_applies(const sdrhip_tx *tx, int log2interp);
int tx_decode_gather(sdrhip_tx *tx, const uint8_t *drx, const uint8_t *indices, size_t nframes, InterpGather *g, uint8_t *block0 = nullptr);
int tx_collector(sdrhip_tx *tx); // the datagram collector, created on first use
// the interpolator behind the collector of a datagram call, each stream's own count (device, the classify pass's) of n_max at most:
// x1 to 8-bit = K6n narrows; x2 .. x64 = one ragged launch; x1 int16 = nothing, the collector wrote the samples where they go.
// (Per-stream formats: dos counts 4-byte units; x1 is K6x, x2 .. x64 K5x, both up to each stream's own count)
int tx_interpolate_counts(sdrhip_tx *tx, const int16_t *pay, size_t n_max, size_t pitch, int16_t *dout, size_t dos, const int *counts);
} // namespace sdrhip
