// rx_step_plan.h -- what one step of the Rx pipe launches: the arrangement of the uniform step (sdrhip_rx_process) and of the
// ragged step (rx_ragged), decided from plain values in one place.  sdrhip_rx.cpp fills the inputs, asks once and runs the answer
// phase by phase; rx_ragged_room asks the same questions ahead of a step.  Pure host arithmetic (C++11, standard headers and
// decim_plan.h, no HIP, no handle): tests/cxx/rx_step_plan_test.cpp replays every rule on a CPU against the code it replaced.
#pragma once
#include "decim_plan.h"

#include <cstddef>
#include <cstdint>

namespace sdrhip {
constexpr uint64_t RX_STEP_FRAME_SAMPLES = 127 * 127; // samples of one frame (SDRHIP_SAMPLES_PER_FRAME)
constexpr int RX_STEP_FC_CEN = 2;                     // SDRHIP_FC_CEN
constexpr int RX_STEP_GROUP = 2;                     // frames per group of the encoder's frame list (GF_FRAMES_PER_GROUP)
// the matrix-core waves' frame-layout store offsets are 32 bits with the top two reserved (decim_mfma.hip): a stream's area fits
inline bool rx_direct_fits(size_t stream_bytes) { return stream_bytes < 0x3fffffffu; }
// the form fec_encode_device chooses for `rows` recovery blocks: 0 the generic kernel, 1 the FFT / bit-sliced kernel, 2 the walk
inline int rx_encode_form(int rows, int enc_min_rows) { return rows < enc_min_rows ? 0 : rows <= 32 ? 1 : 2; }

// ------------------------------------------------------------------------------------------------ the uniform step
struct RxStepIn {
    int L, fcpos, R;             // log2 decimation, Fc position, recovery blocks per frame
    bool pipelined;              // the pipe delivers a call's frames with the next call
    bool late_have, late_encode; // frames of the previous call wait for delivery / for their encode
    size_t late_frames, late_frame_bytes;
    bool ev_framed;              // the event behind everything the waiting encode reads exists
    int rx_fused, rx_direct;     // context options
    int enc_min_rows;            // fewest recovery blocks the structured encoder serves (enc128_min_rows)
    uint64_t pending;            // samples in the frame that is open when the call begins
    size_t done;                 // frames the call completes
    size_t stream_bytes;         // bytes of one stream's frame area (known once the windows have room)
    bool mfma_applies;           // the decimator's planner puts a stream-order call of this size on the matrix cores
};

enum RxRoute {
    RX_ROUTE_LIN_FILTERLESS, // stream order + K2: the mode has no cascade kernel (Decimators.cpp:22-91,127-170)
    RX_ROUTE_LIN_MFMA,       // stream order + K2: the matrix cores apply and their frame-layout stores do not
    RX_ROUTE_FRAMES          // decimate into the frame layout (VALU framing epilogue, or K1m's frame-layout stores)
};
enum RxEncoder {
    RX_ENC_NONE,       // nothing completed, or no recovery blocks
    RX_ENC_STRUCTURED, // gf_encode128 now (K2 inside its launch: k2_in_encoder)
    RX_ENC_DEFERRED,   // gf_encode128 with the next call's decimator launch, or sdrhip_rx_flush (pipelined)
    RX_ENC_GENERIC     // the generic matrix kernel over a frame list (R < enc_min_rows)
};

// what the call hands to the caller: its own frames, or (pipelined) the previous call's.  Needed for the refusals, before the
// windows have room; the plan carries the same two values
struct RxStepDelivery { size_t frames, frame_bytes; };
inline RxStepDelivery rx_step_delivery(const RxStepIn &in, size_t frame_bytes)
{
    const RxStepDelivery d = {in.pipelined ? (in.late_have ? in.late_frames : 0) : in.done,
                              in.pipelined && in.late_have ? in.late_frame_bytes : frame_bytes};
    return d;
}

// overlap mode: a waiting encode goes to the second stream, behind everything the call that left it had enqueued (ev_framed)
inline bool rx_late_overlaps(const RxStepIn &in) { return in.rx_fused == 3 && in.ev_framed; }

struct RxStepPlan {
    size_t deliver_now, deliver_fb;
    RxRoute route;
    bool stream_order() const { return route != RX_ROUTE_FRAMES; }
    bool flip_lin;         // the other stream-order buffer (the deferred encoder of the previous call still reads this one)
    // ---- stream order: the frames that lie entirely inside the call's samples are laid out by the encoder (EncodeLin), K2 does
    // the frame that was open, the one left open, meta blocks and headers
    bool use_lin;
    int lin_first;         // 1: slot 0 of the window holds the frame that was open
    uint64_t lin_pending;
    size_t skip_from, skip_to; // K2 leaves these decimated samples to the encoder
    bool k2_in_encoder;    // K2 rides in the structured encoder's launch (one launch less per step)
    bool lin_straddle;     // ... and the encoder completes the frame that was open from the stream-order rows
    RxEncoder encoder;
    // ---- the encode that waits from the previous call
    bool fuse;             // it rides in this call's decimator launch (rx_fused 1 | 2)
    bool coresident;       // it runs on the second stream beside this call's decimator (rx_fused 3)
    bool record_framed;    // this call's own deferred encode will run there: ev_framed is recorded behind what it reads
};

// (structured: the encoder also wants frames of whole dwords; (128 + R) super blocks are, sdrhip_rx.cpp asserts it)
inline RxStepPlan rx_step_plan(const RxStepIn &in, size_t frame_bytes)
{
    RxStepPlan p = RxStepPlan();
    const RxStepDelivery d = rx_step_delivery(in, frame_bytes);
    p.deliver_now = d.frames; p.deliver_fb = d.frame_bytes;
    const bool structured = in.R >= in.enc_min_rows; // gf_encode128_kernel serves this setting, and lays frames out on its way
    const bool filterless = in.L == 0 || (in.fcpos != RX_STEP_FC_CEN && in.L <= 2);
    const bool direct = in.rx_direct && !in.pipelined && rx_direct_fits(in.stream_bytes);
    p.route = filterless ? RX_ROUTE_LIN_FILTERLESS : !direct && in.mfma_applies ? RX_ROUTE_LIN_MFMA : RX_ROUTE_FRAMES;
    p.fuse = in.late_encode && (in.rx_fused == 1 || in.rx_fused == 2);
    p.coresident = in.late_encode && rx_late_overlaps(in);
    if (p.stream_order()) {
        p.flip_lin = in.pipelined;
        const size_t first = in.pending ? 1 : 0;
        if (structured && in.done > first) {
            p.use_lin = true;
            p.lin_first = (int)first; p.lin_pending = in.pending;
            p.skip_from = first * (size_t)RX_STEP_FRAME_SAMPLES - (size_t)in.pending;
            p.skip_to = in.done * (size_t)RX_STEP_FRAME_SAMPLES - (size_t)in.pending;
        }
        p.k2_in_encoder = !in.pipelined && in.rx_fused && in.R > 0 && p.use_lin;
        if (p.k2_in_encoder && first == 1) { p.lin_straddle = true; p.skip_from = 0; }
    }
    p.encoder = !(in.done && in.R > 0) ? RX_ENC_NONE : !structured ? RX_ENC_GENERIC : in.pipelined ? RX_ENC_DEFERRED : RX_ENC_STRUCTURED;
    p.record_framed = p.encoder == RX_ENC_DEFERRED && in.rx_fused == 3;
    return p;
}

// ------------------------------------------------------------------------------------------------ the ragged step
// ---- input: what stands between the caller's rows and the decimator
struct RxRaggedInput {
    bool in_dev; // the rows are device memory, read in place
    bool unpack; // per-stream formats: K0x lays every row out as int16 (host rows staged packed)
    bool stage;  // host rows of one format: staged row by row
    bool widen;  // 8-bit rows: K0r widens them behind that
};
// batch: int16 device rows K0p laid out; dev_rows: int16 device rows whatever `mem` and the formats are (the datagram entries)
inline RxRaggedInput rx_ragged_input(bool batch, bool dev_rows, bool stream_formats, bool bank_s16, bool mem_device)
{
    const bool own = !batch && !dev_rows; // the caller's rows, in the pipe's input format
    RxRaggedInput r;
    r.in_dev = mem_device || dev_rows;
    r.unpack = own && stream_formats;
    r.stage = !r.unpack && !r.in_dev;
    r.widen = own && !bank_s16 && !stream_formats;
    return r;
}

// ---- K1mr stores straight into each stream's window (else: stream-order rows, and K2r lays them out)
inline bool rx_ragged_direct(bool plan_mfma, int rx_direct, size_t stream_bytes) { return plan_mfma && rx_direct && rx_direct_fits(stream_bytes); }

// ---- K2r's job.  Behind direct stores K1mr's pieces wrote the meta blocks with the shared record: K2r, without samples, writes them
// again where a stream has values of its own (the host's arrays, KFb's or KF's)
enum RxK2rJob { RX_K2R_NONE, RX_K2R_PACK, RX_K2R_META };
// (sw: the streams have records of their own; follow / follow_bits: KF / KFb rewrite rows of the device table)
inline RxK2rJob rx_ragged_k2r(bool any_dec, bool direct, bool sw, bool follow, bool follow_bits)
{
    if (!(any_dec && (!direct || sw || follow || follow_bits))) return RX_K2R_NONE;
    return direct ? RX_K2R_META : RX_K2R_PACK;
}

// ---- the encoder's frame list.  Recovery row r of CM256 is Cauchy row 128 + r whatever the count, so a frame encoded with R' >= its
// own count carries its own encoding in its first rows: the frames are grouped by the form fec_encode_device chooses for their own
// count, each group present is ONE launch with the group's largest count; streams without recovery blocks are left out.
// Entries of the list: up to three sublists, each padded to a whole group
inline size_t rx_flist_entries(size_t sum_done) { return (sum_done / RX_STEP_GROUP + 3) * RX_STEP_GROUP; }
struct RxEncStream { int fec; size_t done, first; }; // recovery blocks, completed frames, area index of the first of them
struct RxEncGroups {
    size_t k;                  // entries written
    size_t first[3], count[3]; // each form's sublist: where it starts, its entries (a multiple of RX_STEP_GROUP; 0: no launch)
    int rows[3];               // ... and the recovery blocks of its launch
};
// stream(s) -> RxEncStream; fl has room for rx_flist_entries(sum of done)
template <class StreamOf> inline RxEncGroups rx_encode_groups(size_t S, StreamOf stream, int enc_min_rows, int32_t *fl)
{
    RxEncGroups g = RxEncGroups();
    for (int form = 0; form < 3; ++form) {
        g.first[form] = g.k;
        for (size_t s = 0; s < S; ++s) {
            const RxEncStream e = stream(s);
            if (e.fec <= 0 || !e.done || rx_encode_form(e.fec, enc_min_rows) != form) continue;
            g.rows[form] = e.fec > g.rows[form] ? e.fec : g.rows[form];
            for (size_t f = 0; f < e.done; ++f) fl[g.k++] = (int32_t)(e.first + f);
        }
        while (g.k % RX_STEP_GROUP) fl[g.k++] = -1;
        g.count[form] = g.k - g.first[form];
    }
    return g;
}

// ---- delivery to the caller's frames_out
enum RxRaggedDelivery {
    RX_DELIVER_PITCHED,   // per-stream fecblk: each stream's frames dense -- a 2-D copy per stream from the pitched area
    RX_DELIVER_RECTANGLE, // the windows line up: one 2-D copy
    RX_DELIVER_LINEAR     // one linear copy per stream
};
// (dev_rows to host memory -- the datagram entry's host callers -- get each stream's own frames and no more: its link traffic is
// datagrams up, frames down)
inline RxRaggedDelivery rx_ragged_delivery(bool mixed, bool same_base, bool same_done, bool dev_rows, bool mem_host)
{
    if (mixed) return RX_DELIVER_PITCHED;
    return same_base && (same_done || !(dev_rows && mem_host)) ? RX_DELIVER_RECTANGLE : RX_DELIVER_LINEAR;
}
} // namespace sdrhip
