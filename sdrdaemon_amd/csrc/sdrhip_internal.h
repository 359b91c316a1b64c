// sdrhip_internal.h -- shared between the host side (sdrhip*.cpp) and the gfx950 kernels: the kernels' argument structs and launch_*
// functions.  (What a decimator launch's geometry is decided by lives in decim_plan.h, host-only.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "decim_plan.h"
#include "interp_pick.h"
#include "interp_ragged_plan.h"
#include "rx_depart_order.h"
#include "rx_unpack_plan.h"

// loads of data that is streamed through once (IQ input, frames): non-temporal.  tools/dma_probe.hip on MI355X: 7.1 TB/s with
// `nt` against 6.2 TB/s with the default cache policy, register loads and LDS-DMA alike (stores: no difference).
#ifndef SDRHIP_NT
#define SDRHIP_NT 1
#endif
#if SDRHIP_NT
#define SDRHIP_STREAM_LOAD(ptr) __builtin_nontemporal_load(ptr)
#else
#define SDRHIP_STREAM_LOAD(ptr) (*(ptr))
#endif

namespace sdrhip {

// Per-stream half-band decimator state: for each of the six filter instances
// (m_decimator2..64, Decimators.h:56-70) the last 64 inputs, split the way the kernels
// consume them: plane p = comp * 2 + parity (comp 0 = I, 1 = Q; parity 0 = even input
// = first sample of a myDecimate pair, 1 = odd), 32 int32 entries each, oldest first.
constexpr int DEC_STAGES = 6;
constexpr int DEC_HIST = 32;
constexpr int DEC_STATE_WORDS = DEC_STAGES * 4 * DEC_HIST; // int32 words per stream

// Per-stream interpolator state: for each of the six instances (m_interpolator2..64,
// Interpolators.h:47-52) the last 32 inputs per component (ring of order/2 <= 32), oldest first.
constexpr int INT_STAGES = 6;
constexpr int INT_HIST = 32;
constexpr int INT_STATE_WORDS = INT_STAGES * 2 * INT_HIST;

struct DecimArgs {
    const int16_t *in;   // stream s at in + 2 * s * in_stride
    int16_t *out;        // stream s at out + 2 * s * out_stride (or frame layout, see frame_*)
    size_t in_stride;    // samples
    size_t out_stride;   // samples
    size_t n_used;       // raw samples consumed per stream (multiple of 2^log2decim)
    const int32_t *state_cur; // [nstreams][DEC_STATE_WORDS]
    int32_t *state_next;
    int nstreams;
    int nsub_per_seg;    // sub-chunks per segment
    int nseg;            // grid.x
    int bias;            // 0 EO1, 1 DB
    int norm, trunk;     // final `<< norm >> trunk`
    // frame-layout epilogue (fused Rx pipe): when frame_mode != 0 the decimated sample with
    // per-stream running index g = out_index + frame_sample_base goes to the payload of super
    // block 1 + (g % 16129) / 127 of frame g / 16129 (UDPSinkFEC.cpp:134-155); `out` then is a
    // byte pointer to the stream's first frame slot and out_stride its stride in BYTES / 4.
    int frame_mode;
    int frame_blocks;        // super blocks per frame slot (128 + nb_fec)
    uint64_t frame_sample_base; // samples already sitting in the first (partial) frame slot
    // meta blocks of the frames this call starts (UDPSinkFEC.cpp:87-132, 150-152): frame slots meta_first ..
    // meta_first + meta_count - 1 of every stream get block 0 = {header, 24-byte MetaDataFEC, zero fill} and
    // the {frameIndex, blockIndex, 0} headers of blocks 1..127; frameIndex = meta_frame_count0 + i (mod 2^16)
    int meta_first, meta_count;
    unsigned meta_frame_count0;
    unsigned meta_w[6];
    uint64_t meta_idx0;  // decimated-sample index (counted from the call's first sample) at which frame meta_first starts
    unsigned meta_rate;  // sample rate of the frame stream in Hz (0: every frame carries the call's time stamp), see frame_meta_words()
    // matrix-core launch (decim_mfma.hip): per stream the VALU code runs the head [0, mf_head) and the tail
    // [mf_tail_start, n_used) in pieces of mf_tail_seg samples (mf_npieces = 1 + tail pieces workgroups), the
    // matrix-core waves run mf_wps groups of 8 spans of mf_span raw samples from mf_head on
    size_t mf_head, mf_span, mf_tail_start, mf_tail_seg;
    int mf_wps, mf_npieces;
    // the nstreams x mf_npieces VALU pieces go to mf_piece_wgs workgroups: the first mf_piece_early of them take mf_piece_share
    // pieces each (they start with the launch, on the CUs the matrix-core workgroups leave free), every other one a single piece
    int mf_piece_wgs, mf_piece_early, mf_piece_share;
    unsigned *mf_dump;   // >= 1 KiB of device memory that swallows the stores of the warm-up period
    int mf_ring;         // LDS-DMA ring depth of the decimate16 kernel in groups: 4 (147 KiB per workgroup), 3 (108 KiB: room for another kernel)
    int mf_prio;         // 1: the matrix-core waves raise their issue priority (they share their SIMDs with another kernel's waves)
    // (behind everything else: the kernels' argument offsets are part of their register allocation, decim_mfma.hip sits on the edge)
    const unsigned *meta_tab; // per-stream {fc, rate, zero-stamp CRC}, STREAM_META_WORDS each (stream_meta_base()); NULL: meta_w / meta_rate
                              // serve every stream.  (Ragged launches leave it NULL: each stream's three words come with its RaggedRow, for K2r)
};
// host: the meta_* fields of DecimArgs, FrameArgs or Enc128Args from the call's record (RxMeta, sdrhip_host.h)
template <class Args, class Meta> inline void set_meta_args(Args &a, const Meta &m)
{
    a.meta_first = m.first; a.meta_count = m.count; a.meta_frame_count0 = m.frame_count0;
    for (int i = 0; i < 6; ++i) a.meta_w[i] = m.w[i];
    a.meta_idx0 = m.idx0; a.meta_rate = m.rate; a.meta_tab = m.tab;
}

// MetaDataFEC of the fi-th frame a call starts (UDPSinkFEC.cpp:90-115: the reference takes gettimeofday() when it opens a
// frame and CRCs the first 20 bytes).  A batched call opens all its frames "at once", so the stamp of a frame is the
// call's stamp (base[3] = tv_sec, base[4] = tv_usec: the time of the call's first sample) advanced by the sample clock:
// frame fi starts idx0 + fi * 16129 samples into the call, i.e. floor(idx * 10^6 / rate) microseconds later.
// CRC-32 (boost::crc_32_type = reflected 0xEDB88320) of the stamped record: the CRC is affine over GF(2), so
// crc(record) = crc(record with a zero stamp) ^ XOR over the set stamp bits k of CRC_BIT[k]; the first term comes from the host
// (base[5]), CRC_BIT[k] = the zero-init CRC of the 20-byte message that has only stamp bit k set (compile-time table).  Lane k
// of a wave looks at bit k, six DPP / swizzle steps XOR-reduce: ~25 instructions per frame instead of a 160-step bit-serial
// loop (which doubled the framing kernel's time).  Must be called by whole waves.  (The test-side framer applies the same
// rule: DESIGN.md K2.)
constexpr int STREAM_META_WORDS = 3; // words per stream of DecimArgs::meta_tab (stream_meta_base)
#if defined(__HIPCC__) && __cplusplus >= 201703L // (the kernels' translation units: C++17; the host files are C++11)
struct CrcBitTable { unsigned c[64]; };
constexpr CrcBitTable make_crc_bit_table()
{
    CrcBitTable T{};
    for (int k = 0; k < 64; ++k) {
        unsigned crc = 0u;
        for (int byte = 0; byte < 20; ++byte) {
            unsigned v = 0u;
            if (byte >= 12 && byte == 12 + k / 8) v = 1u << (k % 8);
            crc ^= v;
            for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
        }
        T.c[k] = crc;
    }
    return T;
}
__device__ const CrcBitTable CRC_BIT = make_crc_bit_table();

__device__ __forceinline__ void frame_meta_words(const unsigned (&base)[6], uint64_t idx0, unsigned rate, int fi, unsigned (&w)[6])
{
    unsigned sec = base[3], usec = base[4];
    if (rate) {
        const uint64_t idx = idx0 + (uint64_t)fi * 16129u;
        const uint64_t dus = idx * 1000000ull / rate;
        const uint64_t ds = dus / 1000000ull;
        usec += (unsigned)(dus - ds * 1000000ull);
        sec += (unsigned)ds;
        if (usec >= 1000000u) { usec -= 1000000u; sec += 1u; }
    }
    w[0] = base[0]; w[1] = base[1]; w[2] = base[2]; w[3] = sec; w[4] = usec;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned word = lane < 32 ? sec : usec;
    unsigned x = ((word >> (lane & 31)) & 1u) ? CRC_BIT.c[lane] : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x ^= (unsigned)__shfl_xor((int)x, m, 64);
    w[5] = base[5] ^ x;
}
// the same record by ONE thread (no cross-lane step: every lane of a wave can form the record of a different frame at once)
__device__ __forceinline__ void frame_meta_words_thread(const unsigned (&base)[6], uint64_t idx0, unsigned rate, int fi, unsigned (&w)[6])
{
    unsigned sec = base[3], usec = base[4];
    if (rate) {
        const uint64_t idx = idx0 + (uint64_t)fi * 16129u;
        const uint64_t dus = idx * 1000000ull / rate;
        const uint64_t ds = dus / 1000000ull;
        usec += (unsigned)(dus - ds * 1000000ull);
        sec += (unsigned)ds;
        if (usec >= 1000000u) { usec -= 1000000u; sec += 1u; }
    }
    w[0] = base[0]; w[1] = base[1]; w[2] = base[2]; w[3] = sec; w[4] = usec;
    unsigned x = 0u;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
        x ^= (0u - ((sec >> k) & 1u)) & CRC_BIT.c[k];
        x ^= (0u - ((usec >> k) & 1u)) & CRC_BIT.c[32 + k];
    }
    w[5] = base[5] ^ x;
}
// Per-stream UDPSink::setCenterFrequency / setSampleRate (sdrhip_rx_set_stream_meta): of the six words of a launch's zero-stamp record
// three differ between the streams of a bank: w[0] = centre frequency, w[1] = sample rate (also the clock of the stamps) and
// w[5] = the record's CRC (host-computed: the affine part, see above).  ROW = false (uniform launches): `p` is the Rx handle's
// table, stream s at p + s * STREAM_META_WORDS, NULL: the shared record serves every stream.  ROW = true (ragged launches): `p` is
// the stream's own words, RaggedRow::fc ... w2 (the fourth, w[2], carries the stream's nbFECBlocks: sdrhip_rx_set_stream_fec).
// `stream` and `p` are wave-uniform: scalar loads where a workgroup starts on a stream's frames.
template <bool ROW = false>
__device__ __forceinline__ void stream_meta_base(const unsigned (&shared)[6], unsigned shared_rate, const unsigned *p, int stream,
                                                 unsigned (&base)[6], unsigned &rate)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) base[k] = shared[k];
    rate = shared_rate;
    if (ROW || p) {
        const unsigned *t = ROW ? p : p + (size_t)STREAM_META_WORDS * (size_t)__builtin_amdgcn_readfirstlane(stream);
        base[0] = t[0]; base[1] = t[1]; base[5] = t[2];
        if (ROW) base[2] = t[3]; // (RaggedRow::w2, behind the three: the stream's own nbFECBlocks byte)
        rate = t[1];
    }
}
#endif

// returns hipSuccess or the launch error
hipError_t launch_decimate(int log2decim, int fcpos, bool pack16, const DecimArgs &a, hipStream_t stream);
// matrix-core variant of the centred cascades, a.mf_* from plan_decimate_mfma (decim_plan.h)
hipError_t launch_decimate_mfma(int log2decim, bool pack16, const DecimArgs &a, hipStream_t stream);
struct Enc128Args;
// the same decimator launch (register-ring variant) with encoder workgroups for `e` behind it in the grid (fused Rx step)
// roles: SDRHIP_FUSED_ROLE_WORDS zero-initialised device words owned by the context, tag: 1, 2, 3 ... per launch on them
constexpr int SDRHIP_FUSED_ROLE_WORDS = 4096 + 8;
hipError_t launch_rx_fused(int log2decim, bool pack16, const DecimArgs &a, const Enc128Args &e, unsigned *roles, unsigned tag, hipStream_t stream);

// filter-less paths: log2decim 0 (decimate1) and inf/sup 2, 4 (Decimators.cpp:22-91,127-170)
hipError_t launch_decimate_simple(int log2decim, int fcpos, const int16_t *in, size_t in_stride, int16_t *out,
                                  size_t out_stride, size_t n_in, int nstreams, int norm, int trunk,
                                  hipStream_t stream);

// Ragged calls (sdrhip_decimate_ragged, sdrhip_rx_process_ragged): one row per stream, uploaded per call.  K1r reads
// n_used / seg0, K0r and the filter-less kernel n_raw, K2r the framing fields.
struct RaggedRow {
    uint64_t n_raw;             // samples of the stream in this call (K0r, filter-less kernel: the count itself)
    uint64_t n_used;            // raw samples the cascade consumes (multiple of 2^log2decim)
    uint64_t n_dec;             // decimated samples (K2r)
    uint64_t out_off;           // K2r: dwords from the stream's frame area to slot 0 of its window
    uint64_t frame_sample_base; // K2r: samples already in that slot
    uint64_t meta_idx0;         // K2r: decimated-sample index (from the stream's first sample of the call) of frame meta_first
    int seg0;                   // K1r: first workgroup of the stream (prefix sum of the per-stream segment counts)
    int meta_first, meta_count; // K2r: as FrameArgs::meta_*, per stream
    unsigned frame_count0;
    unsigned tv_sec, tv_usec;   // K2r: the stamp of the stream's first sample (meta_w[3..4])
    // K1mr (the matrix-core launch of ragged calls): the stream's matrix-core waves mf_w0 .. mf_w0 + mf_wps - 1 (mf_wps groups of 8
    // spans from the shared head on), its VALU pieces mf_p0 .. mf_p0 + mf_np - 1: piece 0 = [0, mf_head) from the state, pieces
    // 1.. = mf_tail_seg-long pieces from mf_tail_start, the last one storing the state.  A stream too short for a span
    // (mf_wps = 0) runs on pieces alone (mf_head = min(n_used, mf_tail_seg)).
    int mf_w0, mf_wps, mf_p0, mf_np;
    uint64_t mf_head, mf_tail_start;
    unsigned fc, rate, crc0;    // K2r: the stream's centre frequency, sample rate and zero-stamp CRC (stream_meta_base<true>)
    unsigned w2;                // K2r, KF: word 2 of the stream's record -- sampleBytes, sampleBits, 128, nbFECBlocks (per-stream fecblk)
    // K1r, K1mr, the filter-less kernel: the stream's final `<< norm >> trunk` (Decimators.cpp:27-32, 43-44), norm | trunk << 8
    // (ragged_shift_word, sdrhip_host.h).  Every ragged launch reads the pair here, not in DecimArgs: the bank-wide pair in every row
    // unless the streams' sample sizes differ (sdrhip_rx_set_stream_bits, sdrhip_decimate_ragged_bits).  One word: the row stays 128 bytes
    unsigned shifts;
};
static_assert(sizeof(RaggedRow) == 128, "RaggedRow: one 128-byte row per stream");
// K1mr: the matrix-core launch of a ragged call (plan_decimate_mfma_ragged, decim_plan.h: per-stream fields in the rows, shared span /
// grid in `a`: a.mf_wps = the launch's matrix-core waves, a.mf_npieces = its VALU pieces)
hipError_t launch_decimate_mfma_ragged(int log2decim, bool pack16, const DecimArgs &a, const RaggedRow *rows, hipStream_t stream);
// K1r: the VALU cascade with a 1-D grid of sum_s max(1, ceil(n_used_s / segment)) workgroups; workgroup b serves the stream
// whose seg0 range holds it (binary search over `rows`).  A stream with n_used = 0 copies its state.  a.nsub_per_seg is the
// segment length; a.n_used / a.nseg are ignored, a.nseg carries the grid size.
hipError_t launch_decimate_ragged(int log2decim, int fcpos, bool pack16, const DecimArgs &a, const RaggedRow *rows, hipStream_t stream);
// K1t (decim_taps_kernels.hip): the taps of a centred cascade, the second argument of its kernels.  Index k = log2 of a tap's
// decimation (slot 0 is not used): tap k is the output of half-band stage k - 1 behind its own `<< norm >> trunk`
// (decimated_shifts(k, sampleSize)), stream s at out[k] + 2 * s * stride[k].  mask: bit k set = tap k is stored; the highest set bit
// is the cascade's length L, whose slot serves the last stage (DecimArgs::out / out_stride / norm / trunk are not read).
// (DecimArgs itself stays as it is: see the note on its last field.)
constexpr int DECIM_TAP_SLOTS = 7;
struct DecimTapArgs {
    int16_t *out[DECIM_TAP_SLOTS];
    size_t stride[DECIM_TAP_SLOTS]; // samples
    int norm[DECIM_TAP_SLOTS], trunk[DECIM_TAP_SLOTS]; // (whole words: scalar loads, scalar shift operands)
    unsigned mask;
};
// K1r's grid and rows (a.nsub_per_seg, a.nseg = the grid, rows[s].n_used / seg0); log2decim = the highest tap, 2..6
hipError_t launch_decimate_taps(int log2decim, bool pack16, const DecimArgs &a, const DecimTapArgs &t, const RaggedRow *rows, hipStream_t stream);
// filter-less kernel with per-stream counts n_raw (grid planned for the largest, n_in); norm / trunk are kept for the signature and
// not read: like K1r and K1mr it shifts each stream by its row's pair (RaggedRow::shifts)
hipError_t launch_decimate_simple_ragged(int log2decim, int fcpos, const int16_t *in, size_t in_stride, int16_t *out,
                                         size_t out_stride, size_t n_in, int nstreams, int norm, int trunk, const RaggedRow *rows,
                                         hipStream_t stream);

// TestSource bank (testsource_kernels.hip): one record per stream and call
struct TestSourceParams {
    unsigned phase0; // NCO phase of the call's first sample (2^32 = one turn)
    unsigned inc;    // phase increment per sample
    int amp;         // peak amplitude, Q15
};
hipError_t launch_testsource(const int *table, const TestSourceParams *par, int16_t *out, size_t out_stride, size_t n, int nstreams,
                             hipStream_t stream);

// K2 (frame_kernels.hip): stream-order samples -> super blocks of the frame area
struct FrameArgs {
    const unsigned *in;   // [nstreams][in_stride] IQ dwords
    unsigned *out;        // frame area: stream s at out + s * out_stride dwords, slot 0 = the frame being filled
    size_t in_stride, out_stride;
    size_t n;             // samples per stream in this call
    size_t skip_from, skip_to;  // samples [skip_from, skip_to) are not copied (the encoder moves them, Enc128Args::lin)
    uint64_t frame_sample_base; // samples already in slot 0
    int frame_blocks;     // super blocks per frame slot (128 + nb_fec)
    int meta_first, meta_count; // as DecimArgs::meta_*
    unsigned meta_frame_count0;
    unsigned meta_w[6];
    uint64_t meta_idx0;
    unsigned meta_rate;
    const unsigned *meta_tab; // as DecimArgs::meta_tab
};
hipError_t launch_frame_pack(const FrameArgs &a, int nstreams, hipStream_t stream);
// K2r: the same with per-stream n / window / frame base / meta record from `rows` (a.n = the largest count: the grid;
// a.meta_w[3..4] are replaced by each row's stamp, {fc, rate, crc0} come from the row too; skip_* unused)
hipError_t launch_frame_pack_ragged(const FrameArgs &a, const RaggedRow *rows, int nstreams, hipStream_t stream);
// K2r without samples: block 0 (header, meta record, zero fill) and the headers of blocks 1..127 of the frames every stream starts,
// rewritten behind a K1mr launch whose pieces wrote them with the shared record; max_started = the largest meta_count of the rows
hipError_t launch_frame_meta_ragged(const FrameArgs &a, const RaggedRow *rows, int max_started, int nstreams, hipStream_t stream);

struct InterpArgs {
    const int16_t *in;
    int16_t *out;
    size_t in_stride, out_stride; // samples
    size_t n_in;                  // input samples per stream
    const int32_t *state_cur;     // [nstreams][INT_STATE_WORDS]
    int32_t *state_next;
    int nstreams;
    int nsub_per_seg, nseg;
    // (the Tx pipe's decoded payload -- 127 x 508 bytes per frame, contiguous -- is already the linear sample layout: `in`.)
    // Gather mode (round 6, K5w only; gmap != NULL): the Tx pipe's decoder does NOT copy the received originals; stream s is
    // gframes frames of 127 blocks of 127 samples, block b (1..127) of frame f lies where gmap[(s * gframes + f) * 128 + b] says:
    // bit 31 clear: super block slot (payload at +4) of the received frames grx, 512 bytes apart; bit 31 set: 508-byte slot of the
    // restored blocks grest (the decoder's output; its last slot is all zeros: blocks that never came and cannot be restored)
    const unsigned *gmap;
    const uint8_t *grx, *grest;
    int gframes;
    // Ragged launches (the Tx pipe fed datagrams; the IV_COUNT variants): stream s takes count[s * count_stride] *
    // count_unit inputs, read on the device where the FEC buffer bank's classify pass left the count; n_in / nseg are the
    // largest stream's (the grid).  NULL: every stream takes n_in.
    const int *count;
    int count_stride, count_unit;
};
// IQ sample formats of the pipes' edges (= SDRHIP_IQ_* of include/sdrhip.h)
enum { IQF_S16 = 0, IQF_U8 = 1, IQF_S8 = 2 };
// K0 (convert_kernels.hip): 8-bit IQ rows (stream s at in + 2 * s * in_stride bytes, in_stride a multiple of 8 samples) -> int16 rows
// (stream s at out + 2 * s * out_stride, out_stride a multiple of 4); fmt IQF_U8 / IQF_S8
hipError_t launch_iq8_widen(int fmt, const uint8_t *in, size_t in_stride, int16_t *out, size_t out_stride, size_t n, int nstreams,
                            hipStream_t stream);
// K0r: the same, stream s widening rows[s].n_raw samples (n = the largest: the grid)
hipError_t launch_iq8_widen_ragged(int fmt, const uint8_t *in, size_t in_stride, int16_t *out, size_t out_stride, size_t n, int nstreams,
                                   const struct RaggedRow *rows, hipStream_t stream);
// the grid's x of the row passes K0, K6n (8 samples per lane and step: steps = n >> 3) and K6x (sized for its int16 copy: n >> 2):
// enough workgroups of 256 lanes for the whole chip (256 CUs x 8 per row set), then each lane loops
inline unsigned cvt_blocks(size_t steps, int nstreams)
{
    size_t blocks = (steps + 255) / 256;
    const size_t cap = (size_t)2048 / (size_t)(nstreams > 0 ? nstreams : 1) + 1;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}
// K6n: int16 rows -> int8 rows of byte 1 of every component (interpolate1 with IQF_S8 output)
hipError_t launch_iq8_narrow(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n, int nstreams, hipStream_t stream);

// Asynchronous ragged Rx batches (sdrhip_rx_submit_ragged, rx_async_kernels.hip).  A batch's samples go up packed, block-major and
// stream-minor; K0p lays them out as [stream][out_stride] int16 rows (widening 8-bit input on the way).  The table of rows and
// segments is rx_unpack_plan.h's, filled for the bank's format (unpackx_fill with fmt == NULL).
// K0p: grid = rows[nstreams].wg0 workgroups; fmt IQF_S16 / IQF_U8 / IQF_S8 (rows[s].fmt is not read); out 16-byte aligned,
// out_stride a multiple of 8 samples; `packed` dword-aligned and readable 64 bytes past its last sample (the 8-bit loads of an odd
// segment start read 2 bytes ahead)
hipError_t launch_unpack_packed(int fmt, const uint8_t *packed, int16_t *out, size_t out_stride, const UnpackXRow *rows, const UnpackXSeg *segs,
                                int nstreams, unsigned grid, hipStream_t stream);
// K0x (rx_unpack_mixed_kernels.hip): the same walk over the same table with the format per stream (rows[s].fmt); grid =
// rows[nstreams].wg0 workgroups; src dword-aligned, out 16-byte aligned, out_stride a multiple of 8 samples.  A packed source is
// readable 64 bytes past its last sample (a realigned chunk reads 2 bytes ahead); strided rows that start on 16 bytes are read
// inside their own n * bytes(fmt) bytes alone
hipError_t launch_unpack_mixed(const void *src, int16_t *out, size_t out_stride, const UnpackXRow *rows, const UnpackXSeg *segs, int nstreams,
                               unsigned grid, hipStream_t stream);
// frame compaction for the download: frame k of `out` = frame list[k] of `area` (frames of frame_bytes, a multiple of 16)
hipError_t launch_frame_gather(const uint8_t *area, size_t frame_bytes, const int32_t *list, size_t nframes, uint8_t *out, hipStream_t stream);

// K5 (interp_body.h; log2interp 1..6) / K5w (interp_wave.h: wave-private pipelines in workgroups of one or four independent waves,
// blocks of 128 inputs; log2interp 2..6): each plans its own grid, the largest stream's where a.count is given
void plan_interpolate(int log2interp, size_t n_in, int nstreams, int *nsub_per_seg, int *nseg);
void plan_interpolate_wave(int log2interp, size_t n_in, int nstreams, int n_cu, size_t seg_override, int *nsub_per_seg, int *nseg);
// The bank's one launch: pick = interp_pick's IR_VALU / IR_WAVE answer for this call, `a` planned for pick.route, a.gmap / a.count set
// exactly where pick.variant says IV_GATHER / IV_COUNT (else hipErrorInvalidValue, as for a ratio the route does not serve).
// What `out` holds, by variant:
//  * plain, IV_GATHER, IV_COUNT: int16 IQ, stream s at a.out + 2 * s * a.out_stride, a.out_stride in samples;
//  * IV_S8 (bank-wide 8-bit output): a.out points at 2-byte samples {int8 re, int8 im} and a.out_stride counts THEM; the last stage
//    stores (int8)(v >> 8) of each component;
//  * IV_TABLE (K5x): fmt[s] = IQF_S16 | IQF_S8 on the device decides per stream, and a.out_stride counts 4-BYTE UNITS: row s starts at
//    byte 4 * s * a.out_stride whatever its format, an 8-bit row takes the first 2 * n bytes of it.  fmt is not read without IV_TABLE.
hipError_t launch_interpolate(const InterpPick &pick, int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream);
// (behind it: the IV_TABLE variants, instantiated in interp_mixed_kernels.hip alone)
hipError_t launch_interpolate_table(const InterpPick &pick, int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream);
// K5c (interp_ragged_kernels.hip), the sample-fed ragged entry: a 1-D grid over the `nentries` entries of a per-call table (device;
// interp_ragged_plan.h), pick = interp_pick_mapped's answer with wpw settled on nentries.  The rows carry every stream's offsets,
// count and segments: a.in_stride / a.out_stride are 0, a.n_in / a.nseg / a.nstreams are not read; x1 (IR_COPY) moves rows[s].n_in
// samples per row.  Int16 output
hipError_t launch_interp_mapped(const InterpPick &pick, int log2interp, const InterpArgs &a, const InterpMapRow *rows, const InterpMapEntry *entries,
                                unsigned nentries, hipStream_t stream);
// K6x (interp_mixed_kernels.hip) is x1 with a format table, rows as for IV_TABLE: the copy (int16 rows) or the narrowing (8-bit
// rows) of n samples per stream, or of count[s * count_stride] * count_unit <= n where count is given
hipError_t launch_interpolate1_mixed(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n, int nstreams, const int *fmt,
                                     const int *count, int count_stride, int count_unit, hipStream_t stream);

// frames are processed in groups that share one coefficient matrix (one frame per half-wave)
constexpr int GF_FRAMES_PER_GROUP = 2;

// GF(256) matrix apply: out[f][r][:] = XOR_j coef[f or 0][r][j] * in[f][src(j)][:]
struct GfArgs {
    const uint8_t *in;       // frames: [nframes][in_blocks][in_pitch] bytes
    uint8_t *out;            // [nframes][rows][out_pitch]
    const uint8_t *coef;     // [ngroups or 1][rows][cols]
    const uint8_t *tab;      // 256 x 32 byte multiplier tables (device)
    size_t in_frame_bytes, out_frame_bytes;
    int in_pitch, out_pitch; // bytes between consecutive blocks
    int in_off, out_off;     // byte offset of the 508 protected bytes inside a block slot
    int rows, cols;
    int coef_per_frame;      // 1: coef indexed by frame, 0: shared
    const int16_t *row_dst;  // optional [ngroups or 1][rows] destination block index, -1 = skip (else r)
    const int16_t *col_src;  // optional [ngroups or 1][cols] source block index (else j)
    int nframes;
    // frames are processed in groups of GF_FRAMES_PER_GROUP that share one coefficient matrix (index =
    // group when coef_per_frame, else 0): frame_list[group * GF_FRAMES_PER_GROUP + slot] (or -1), NULL = identity
    const int32_t *frame_list;
    int ngroups;
    // optional indirection: matrix slot of each group (pattern cache); matrices / row_dst tables are then
    // matrix_rows rows apart (0 = tightly packed, `rows` apart)
    const int32_t *group_cm;
    int matrix_rows;
};
hipError_t launch_gf_apply(const GfArgs &a, hipStream_t stream);

// structured (Karatsuba) encoder for OriginalCount = 128: frames of 128 super blocks (pitch 512,
// payload at +4) -> `rows` recovery super blocks (pitch 512, payload at +4)
struct Enc128Args {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *tab;             // 256 x 32 byte multiplier tables (device)
    const uint8_t *leaf_tables;     // [8][81][32] multiplier tables of the Karatsuba leaves of G_0..G_7 (device)
    const uint8_t *fft_tables;      // [192][32] butterfly / fold / row constants of the additive-FFT encoder (gf_encode128_fft.h, device)
    int use_fft;                    // 1: rows <= 32 run the additive-FFT encoder (context option enc_path), 0: the Karatsuba walk
    size_t in_frame_bytes, out_frame_bytes;
    int rows;                       // recovery blocks, 1..128
    int nframes;                    // frames addressable through in/out
    const int32_t *frame_list;      // optional list of frame indices (-1 = skip), nlist entries; NULL = 0..nlist-1
    int nlist;
    int gen_done, gen_cap;          // gen_done > 0: entry i of the list IS (i / gen_done) * gen_cap + i % gen_done (the Rx pipe's
                                    // frames: `gen_done` finished slots of each stream, streams gen_cap slots apart), no array
    // Rx pipe behind a stream-order decimator: the payload of super blocks 1..127 of frame slot f >= lin_first of stream s
    // (frame index s * lin_cap + f) is taken from lin[s][f * 16129 - lin_pending ...] instead of the frame area, and
    // written into the frame area on the way (UDPSinkFEC::write's copy, UDPSinkFEC.cpp:134-155, fused into the encoder);
    // block 0 and the headers are in place already.  lin == NULL: plain encode.
    const unsigned *lin;
    size_t lin_stride;              // dwords between streams
    int lin_cap, lin_first, lin_pending;
    int lin_straddle;               // 1: frame slot 0 (open when the call began, lin_pending samples in it) is completed from
                                    // lin[0 ..] by the encoder itself, K2 leaves it alone (launch_gf_encode128_pack)
    // Rx pipe with K2 in the SAME launch (launch_gf_encode128_pack): the meta blocks and frame indices of the frame slots
    // meta_first .. meta_first + meta_count - 1 of every stream (gen_* addressing) are not in memory yet when the encoder reads
    // block 0: it derives them itself, exactly as K2 writes them (frame_meta_words).  meta_count = 0: everything is in memory.
    int meta_first, meta_count;
    unsigned meta_frame_count0;
    unsigned meta_w[6];
    uint64_t meta_idx0;
    unsigned meta_rate;
    const unsigned *meta_tab;       // as DecimArgs::meta_tab : the frame's stream is fr / gen_cap
    // staggered start (round 6): the launch is ONE round of resident workgroups that all load first and compute afterwards -- the
    // memory phase and the VALU phase do not overlap.  Workgroup i sleeps (i / stagger_div) * stagger units of 1024 clocks before
    // its loads (stagger_div = the number of CUs: the i-th workgroup a CU receives), so that the co-resident workgroups of a CU are
    // in different phases.  0 = off.
    int stagger, stagger_div;
    int half_units;                 // 1: the FFT encoder runs in half-frame workgroups (gf_encode128_fft_half_kernel; context option enc_units)
    int bitslice;                   // 1: the FFT encoder's middle stages as bit-sliced XOR trees (gf_encode128_bs.h; context option
                                    // enc_form); whole-frame workgroups only: half_units = 1 runs the table form
};
// the sleep in front of a workgroup's loads (Enc128Args::stagger, DecodeBuffers::stagger)
#if defined(__HIPCC__)
// arrival counters per CU (key = XCC_ID, SE / SH / CU of HW_ID), never reset: the workgroups a CU receives one after the other get
// consecutive ranks whatever the dispatcher's dealing is (stagger_div <= -100)
static __device__ unsigned g_fec_cu_rank[4096];
__device__ __forceinline__ int fec_stagger_phase(int unit, int stagger_div)
{
    if (stagger_div <= -100) {
        __shared__ int s_phase;
        if (threadIdx.x == 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            const unsigned key = ((xcc & 0xfu) << 8) | ((hw >> 8) & 0xffu);
            s_phase = (int)(atomicAdd(&g_fec_cu_rank[key], 1u) % (unsigned)(-stagger_div - 100));
        }
        __syncthreads();
        return __builtin_amdgcn_readfirstlane(s_phase);
    }
    // stagger_div > 0: phase = the resident round (unit / CUs); < 0: phase = unit mod -stagger_div (consecutive workgroups on one CU)
    return stagger_div > 0 ? unit / stagger_div : unit % -stagger_div;
}
__device__ __forceinline__ int fec_stagger_sleep(int unit, int stagger, int stagger_div)
{
    if (stagger <= 0 || stagger_div == 0) return 0;
    const int ph = fec_stagger_phase(unit, stagger_div); // (workgroup-uniform)
    const int n = ph * stagger;
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(16);
    return ph;
}
#endif
// smallest number of recovery blocks the structured 128-original encoder is used for (below: the generic matrix kernel)
constexpr int ENC128_MIN_ROWS = 13;
hipError_t launch_gf_encode128(const Enc128Args &a, hipStream_t stream);
// encoder + K2 (framing residue: open frames, meta blocks, headers) of the same call in one launch
hipError_t launch_gf_encode128_pack(const Enc128Args &a, const FrameArgs &f, int nstreams, hipStream_t stream);
hipError_t launch_block_scatter(const uint8_t *src, size_t src_frame_bytes, int src_pitch, int src_off, uint8_t *dst,
                                size_t dst_frame_bytes, int dst_pitch, int dst_off, const int16_t *map, int nblocks, int nframes,
                                hipStream_t stream);
hipError_t launch_fec_headers(const uint8_t *frames, size_t in_frame_bytes, uint8_t *rec, size_t out_frame_bytes, int nb_fec,
                              int first_index, int nframes, const int32_t *frame_list, int nlist, hipStream_t stream);


// device-side decode planning (gf_kernels.hip): work buffers of a batch of nframes
constexpr size_t DECODE_PLAN2_BYTES = 1488; // sizeof(Dec128Plan), gf_kernels.hip
struct DecodeBuffers {
    uint8_t *coef;            // [nframes][128][128]
    int16_t *pmap, *zmap;     // [nframes][128]
    int16_t *pdst, *zdst;     // [nframes][128]
    int32_t *nrec;            // [nframes][2]
    uint8_t *plan2;           // [nframes][DECODE_PLAN2_BYTES] records of the syndrome decoder, NULL = dense path only
    const uint8_t *leaf_tables; // Karatsuba leaf tables of the 128-original encoder (the syndrome decoder walks the same tree)
    const uint8_t *fft_tables;  // constants of the additive-FFT encoder (gf_decode128_fft.h); NULL or use_fft = 0: the Karatsuba walk
    int use_fft;
    int stagger, stagger_div;   // staggered start of the FFT decoder's workgroups (see Enc128Args::stagger)
    int fused_plan;             // 1: frames that can carry at most DEC128_MAXN recovery blocks are planned by the decoder's own workgroups (one launch)
    // no-copy mode (only honoured by the fused-plan launch: the caller checks fec_decode_gather_ok()): see Dec128Args::srcmap
    unsigned *srcmap;
    uint8_t *restored;
    int restored_rows;
    // dec_max_rows = auto (NULL otherwise): the frames the one-launch decoder hands to the chain behind it -- a counter the launch
    // clears on its stream and [nframes] frame numbers, part of THIS plan buffer (a pipelined Tx call's second stream has its own)
    int *defer_count, *defer_list;
    static size_t bytes(size_t nframes, bool defer = false)
    {
        return nframes * (128 * 128 + 4 * 128 * sizeof(int16_t) + 2 * sizeof(int32_t) + DECODE_PLAN2_BYTES) + 64 + (defer ? 16 + nframes * sizeof(int) : 0);
    }
};
// words of sdrhip_ctx::dec_stats the decoder's kernels count in: [0] frames that broke the dec_max_rows promise, [2] frames the
// one-launch decoder handed to the safe chain under dec_max_rows = auto ([1]: DEC_STATS_SHADOW_MISMATCH, sdrhip_host.h)
constexpr int DEC_STATS_DEFERRED = 2;
// plan + scatter + apply, all on the stream, no host synchronisation; max_rows = upper bound of the recovery blocks a
// frame can have used (128 when unknown); a frame that carries more is left as received and counted in stats[0].
// d.defer_count != NULL (dec_max_rows = auto): max_rows is not read -- 32 for the one-launch decoder, 128 for the listed frames
hipError_t launch_fec_decode_device_plan(const DecodeBuffers &d, const uint8_t *rx, size_t rx_frame_bytes, const uint8_t *indices_dev,
                                         const uint8_t *explog, const uint8_t *tab, int nframes, uint8_t *payload_out,
                                         size_t payload_frame_bytes, uint8_t *block0_out, int max_rows, int strict, unsigned *stats, hipStream_t stream);


// SDRdaemonFECBuffer bank (fecbuf_kernels.hip, sdrhip_fecbuf.cpp): nstreams independent collectors fed raw datagrams
// per-stream collector state, double-buffered (a call reads [cur], writes [cur ^ 1]; the host flips cur when the call commits)
struct FecBufState {
    int head;              // m_frameHead: frame index of the open slot, -1 = the constructor's
    int count;             // m_blockCount of the open slot (every arrival)
    int recov;             // m_recoveryCount (among the first 128)
    int maxrow;            // highest recovery row (blockIndex - 128) among the first 128, -1 = none
    unsigned pres[4];      // originals present among the first 128 (bit b = blockIndex b)
    int dup;               // an original arrived twice among the first 128
    int cbuf;              // carry buffer (0 / 1) that holds the open slot's first 128 super blocks
    int cur_blocks, cur_recov, min_blocks, max_recov; // getCurNbBlocks, getCurNbRecovery, m_minNbBlocks, m_maxNbRecovery
    unsigned cur_meta[6], out_meta[6];                // m_currentMeta, m_outputMeta (MetaDataFEC: 20 bytes, then zero)
    int b0;                // rank of the last block 0 among the open slot's first 128, -1 = none (m_metaRetrieved)
    int pad;
};
// a frame of the call, internal form: rank r of its first 128 arrivals is datagram start + r of the call, or (start + r < 0) super
// block r of the carry buffer st_cur.cbuf
struct FecBufRec {
    int start, count, dslot, flags; // dslot: index among the stream's frames that go to the decoder (-1: written straight)
};
// public record (sdrhip_fecbuf_frame)
struct FecBufPub {
    int frame_index, block_count, recovery_count;
    unsigned flags;
};
// per-stream results of the classify pass read back by the host
enum { FB_K = 0, FB_D, FB_MAXROW, FB_MAXREC, FB_COUNTS = 8 };
struct FecBufArgs {
    const uint8_t *dg;           // stream s: datagram i at dg + s * dg_stride + i * 512
    size_t dg_stride;
    const int *ndg;              // [S] datagrams per stream in this call
    const long long *rec_base;   // [S] first internal record of the stream (prefix of ndg + 1)
    FecBufRec *rec;
    FecBufPub *pub;              // [S][max_frames] public records (released frames only, k < max_frames)
    int *counts;                 // [S][FB_COUNTS]
    int max_frames;
    const FecBufState *st_cur;
    FecBufState *st_next;
    const uint8_t *carry_cur_base; // carry buffers: [2][S][128][512]
    uint8_t *carry_base;
    int nstreams;
    // scatter pass
    const int *job_off;          // [S + 1] prefix of K_s + 1 (the released frames and the open slot of every stream)
    const int *dbase;            // [S] first staging slot of the stream's frames that go to the decoder
    uint8_t *stage;              // [D][128][512] arrival-order super blocks for the decoder
    int *dmap;                   // [D][2] stream, frame of every staging slot
    uint8_t *data_out;           // stream s, frame k: data_out + s * data_stride + k * 127 * 508
    size_t data_stride;
    uint8_t *block0_out;         // stream s, frame k: block0_out + (s * max_frames + k) * 508 (may be NULL)
    const uint8_t *dec_out, *dec_b0; // the decoder's output of staging slot j: dec_out + j * 127 * 508, dec_b0 + j * 508
};
enum { FB_DECODED = 1, FB_META = 2, FB_REPAIRED = 4, FB_DECODE_ERROR = 8 };
hipError_t launch_fecbuf_classify(const FecBufArgs &a, hipStream_t stream);
hipError_t launch_fecbuf_scatter(const FecBufArgs &a, int njobs, hipStream_t stream);
hipError_t launch_fecbuf_copy(const FecBufArgs &a, int nslots, hipStream_t stream);
// the Rx pipe fed datagrams (sdrhip_rx_process_datagrams, rx_join_kernels.hip): the scatter and copy passes with stream s's
// payloads row_off[s] samples (device) behind a.data_out + s * a.data_stride, and KJ, which moves what the decimator left of
// every stream's row (carry[s] + 16129 x counts[s][FB_K] samples, less their largest multiple of `unit` <= 64) to the row's head
// and writes the new carry[s]; rows = [nstreams][row_len] samples
hipError_t launch_fecbuf_scatter_rows(const FecBufArgs &a, const unsigned *row_off, int njobs, hipStream_t stream);
hipError_t launch_fecbuf_copy_rows(const FecBufArgs &a, const unsigned *row_off, int nslots, hipStream_t stream);
hipError_t launch_rx_join_carry(int16_t *rows, size_t row_len, unsigned *carry, const int *counts, unsigned unit, int nstreams,
                                hipStream_t stream);
// KF (rx_follow_kernels.hip, sdrhip_rx_set_follow_meta): one lane per stream; a stream whose committed m_outputMeta (state[s].out_meta)
// carries a sample rate other than 0 gets {fc, rate >> log2decim, CRC of the zero-stamp record with third word w2} in rows[s]
// (device: the per-call table, behind its upload); the others keep their row
hipError_t launch_rx_follow_meta(const FecBufState *state, RaggedRow *rows, int log2decim, int nstreams, hipStream_t stream);
// KFb (rx_follow_bits_kernels.hip, sdrhip_rx_set_follow_bits): one lane per stream, in front of KF; a stream whose committed
// m_outputMeta says a sample size b of 1..16 (byte 1 of state[s].out_meta[2]) gets in rows[s] the shift pair of (log2decim, b), w2 with
// sampleBytes / sampleBits of the decimated size (bytes 2 and 3 kept) and the CRC of {fc, rate, that w2, 0, 0}; the others keep their row
hipError_t launch_rx_follow_bits(const FecBufState *state, RaggedRow *rows, int log2decim, int nstreams, hipStream_t stream);
// asynchronous Tx batches (sdrhip_tx_submit_datagrams): stream s's datagrams back to back at a.dg + dg_off[s] (device); njobs /
// nslots come from the host's shadow of the classification; the scatter pass skips what lies past the classify pass's own counts,
// max_frames or nslots, the guarded copy a slot whose dmap entry is still -1 (preset by the caller)
hipError_t launch_fecbuf_classify_packed(const FecBufArgs &a, const long long *dg_off, hipStream_t stream);
hipError_t launch_fecbuf_scatter_packed(const FecBufArgs &a, const long long *dg_off, int njobs, int nslots, hipStream_t stream);
hipError_t launch_fecbuf_copy_guarded(const FecBufArgs &a, int nslots, hipStream_t stream);
// asynchronous Rx batches (sdrhip_rx_submit_datagrams, rx_dgram_async_kernels.hip): the packed scatter and guarded copy passes with
// stream s's payloads row_off[s] samples (device) behind a.data_out + s * a.data_stride; on top of the packed guards they skip a
// frame whose payload would end past the stream's row (a.data_stride bytes)
hipError_t launch_fecbuf_scatter_packed_rows(const FecBufArgs &a, const long long *dg_off, const unsigned *row_off, int njobs, int nslots,
                                             hipStream_t stream);
hipError_t launch_fecbuf_copy_guarded_rows(const FecBufArgs &a, const unsigned *row_off, int nslots, hipStream_t stream);
// their delivery, KD: segment i = bytes from (from_records ? records : frames) + src to out + dst; src, dst and bytes are multiples
// of 16, the three bases 16-byte aligned
struct RxDeliverSeg {
    uint64_t src, dst, bytes;
    uint32_t wg0, from_records; // first workgroup (rx_deliver_plan)
};
constexpr uint64_t RX_DELIVER_WG_BYTES = 16384; // bytes per workgroup (256 lanes x 4 chunks of 16 bytes)
// fills every segment's wg0, returns the grid (0: an empty or misaligned segment, one of 32 GiB or more, or more than 2^31 workgroups)
uint32_t rx_deliver_plan(RxDeliverSeg *segs, int nseg);
hipError_t launch_rx_deliver(const RxDeliverSeg *segs, int nseg, uint32_t grid, const uint8_t *frames, const uint8_t *records, uint8_t *out,
                             hipStream_t stream);
// counts [S][FB_COUNTS] against the shadow's expect [S][4] = {K, D, maxrow, maxrec}: +1 on *mismatch per
// stream that differs
hipError_t launch_fecbuf_shadow_check(const int *counts, const int *expect, int nstreams, unsigned *mismatch, hipStream_t stream);
// the records of a datagram batch behind a departure-order array (sdrhip_rx_set_egress; KR and KP move them alike,
// rx_records_body.h): record k < place[s].cnt of stream s from records + 16 (s kmax + k) to out + dst + 16 (place[s].pre + k);
// nslots = streams x kmax (0: no records), records readable for all of them.  Bases and offsets 16-byte aligned; the host that made
// the tables vouches for every piece lying inside `out`
struct RxEgressRecPlace {
    uint32_t pre, cnt, pad[2]; // records of the streams before this one, and its own (16 bytes: read with one dwordx4)
};
struct RxEgressRecords {
    const RxEgressRecPlace *place; // [streams] (device)
    const uint8_t *records;
    uint64_t dst;
    uint32_t kmax, nslots;
};
// KR (rx_runs_kernels.hip), round-robin departure-order batches, equal frames (one run per frame) or not (sdrhip_rx_set_stream_fec):
// run k = `count` datagrams from frames + src to out + dst + i * stride (rx_depart_order.h; wg_per_run = its wg_per_run()), then
// the records
hipError_t launch_rx_runs(const RxDepartRun *runs, uint64_t nruns, uint32_t wg_per_run, const uint8_t *frames, uint8_t *out,
                          const RxEgressRecords &rec, hipStream_t stream);
// KP (rx_paced_kernels.hip), paced departure-order batches (SDRHIP_EGRESS_PACED), equal frames or not: datagram i of the array
// comes from frames + 16 * table[i] (device table, n_dgrams entries, rx_paced_order.h) and goes to out + 512 * i, then the records
// as KR moves them.  The host that made the table vouches for every entry lying inside `frames`
hipError_t launch_rx_paced(const uint32_t *table, uint64_t n_dgrams, const uint8_t *frames, uint8_t *out, const RxEgressRecords &rec,
                           hipStream_t stream);
// KX (dgram_demux_kernels.hip), tagged datagram batches: datagram i of the arrival-order array src goes to dst + 512 * dest[i]
// (device table, n_total entries; 0xffffffff: the datagram is moved nowhere).  src and dst 16-byte aligned, n_total below 2^30;
// the host that made dest vouches for every entry lying inside dst
hipError_t launch_dgram_demux(const uint8_t *src, const uint32_t *dest, size_t n_total, uint8_t *dst, hipStream_t stream);
// delivery gather: segment i = bytes (a multiple of 2) from src (dword-aligned, readable 2 bytes past the end) to out + dst
struct GatherSeg {
    const uint8_t *src;
    uint64_t dst, bytes;
    uint32_t wg0, pad; // first workgroup (gather_plan)
};
constexpr uint64_t GATHER_WG_BYTES = 16384; // 16-byte-aligned output bytes per workgroup (256 lanes x 4 chunks of 16 bytes)
// fills every segment's wg0, returns the grid (0: more than 2^31 workgroups)
uint32_t gather_plan(GatherSeg *segs, int nseg);
hipError_t launch_delivery_gather(const GatherSeg *segs, int nseg, uint32_t grid, uint8_t *out, hipStream_t stream);

// KR (stream_state_kernels.hip, sdrhip_*_reset_streams): the streams whose mask byte is set go back to constructor state, in one
// launch over (stream, piece of state).  Every part is optional: a bank's handle fills in its own, a pipe's handle those of its
// filter bank and of its collector
struct StreamResetArgs {
    const uint8_t *mask;   // [nstreams] on the device; NULL: every stream
    int nstreams;
    int row_words;         // int32 words per stream of a history row (DEC_STATE_WORDS / INT_STATE_WORDS), a multiple of 4
    int32_t *rows[2];      // both halves of the double-buffered filter histories (zero filled); NULL: none
    FecBufState *fb[2];    // both halves of the collector state (set to fb_init); NULL: none
    unsigned *carry;       // the samples every stream holds back in front of its decimator (zeroed); NULL: none
    union { FecBufState st; unsigned w[sizeof(FecBufState) / sizeof(unsigned)]; } fb_init; // the constructor's state (fecbuf_fresh_state)
};
hipError_t launch_stream_reset(const StreamResetArgs &a, hipStream_t stream);
// KG / KS (sdrhip_*_export_stream / _import_stream): the scattered pieces of one stream's state <-> one contiguous device blob, as KD
// packs a delivery: segment i = `bytes` (a multiple of 16) from src to dst, both 16-byte aligned; the segments travel in the
// kernel's arguments (no table to upload).  Workgroup w serves the segment whose wg0 range holds it (stream_copy_plan)
constexpr int STREAM_COPY_MAX_SEGS = 8;
constexpr uint32_t STREAM_COPY_WG_BYTES = 16384; // bytes per workgroup (256 lanes x 4 chunks of 16 bytes)
struct StreamCopySeg {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t bytes, wg0;
};
struct StreamCopyArgs {
    StreamCopySeg seg[STREAM_COPY_MAX_SEGS];
    int nseg;
    // KG: which of the two carry buffers holds the collector's open slot stands in the stream's state on the device:
    // seg[carry_seg].src += cbuf_from->cbuf * carry_half bytes (carry_seg = -1: no such segment)
    int carry_seg;
    const FecBufState *cbuf_from;
    size_t carry_half;
    // KS: the stream's count of held-back samples, one word beside the segments (NULL: none)
    unsigned *word_dst;
    unsigned word_val;
};
// fills every segment's wg0, returns the grid (0: no segment, a misaligned or empty one)
uint32_t stream_copy_plan(StreamCopyArgs *a);
hipError_t launch_stream_gather(const StreamCopyArgs &a, uint32_t grid, hipStream_t stream);
hipError_t launch_stream_scatter(const StreamCopyArgs &a, uint32_t grid, hipStream_t stream);

} // namespace sdrhip
