// sdrhip_host.h -- host-side internals shared by the .cpp files of libsdrhip.so
#pragma once
#include "../../include/sdrhip.h"
#include "dev_buffers.h" // (fail, DevBuf, PinnedBuf, DevEvent, TableVersions, CtxRef, BatchRing: who owns what)
#include "rx_stream_settings.h" // (the sample-size arithmetic of the decimators lives there: decimated_sample_size, decimated_shifts, ragged_shift_word)
#include "sdrhip_internal.h"

#include <cstdint>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace sdrhip {

#define HIP_TRY(expr)                                                                                           \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return ::sdrhip::fail(SDRHIP_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// host-pointer calls up to this many input bytes skip the copy engine: the input is memcpy'd into pinned host memory that the
// kernel reads over PCIe itself, small outputs are written the same way (one launch + one sync instead of H2D + launch + D2H + sync:
// 42 -> ~28 us for one 65 536-sample TestSource block, tools/bench_host_block.py)
constexpr size_t SDRHIP_ZEROCOPY_MAX = (size_t)384 << 10; // (measured: 256 KiB calls 42 -> 29 us, 1 MiB calls 59 -> 77 us: the copy engine wins from there)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// the `mem` argument of an entry point
inline int check_mem(int mem)
{
    return mem == SDRHIP_MEM_HOST || mem == SDRHIP_MEM_DEVICE ? SDRHIP_OK : fail(SDRHIP_EINVAL, "mem must be SDRHIP_MEM_HOST or SDRHIP_MEM_DEVICE");
}

// meta blocks the decimator kernel writes for the fused Rx pipe (DecimArgs::meta_*)
struct RxMeta {
    int first, count;
    unsigned frame_count0;
    unsigned w[6]; // MetaDataFEC, 24 bytes: w[3], w[4] = time stamp of the call's first sample; the kernels advance it per frame and add the CRC
    uint64_t idx0; // call-relative decimated-sample index of the first started frame's first sample
    unsigned rate; // sample rate the stamps advance with (Hz, 0 = none)
    const unsigned *tab; // per-stream {fc, rate, zero-stamp CRC} on the device (DecimArgs::meta_tab), NULL: w / rate serve every stream
};

// ---- the decimator bank (sdrhip_decim.cpp)
// device-pointer cores (no argument validation, no staging)
int decimate_device(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *in, size_t n_in,
                    size_t in_stride, int16_t *out, size_t out_stride, size_t *n_out, int frame_mode, int frame_blocks,
                    uint64_t frame_sample_base, const RxMeta *meta = nullptr, const Enc128Args *fuse = nullptr, bool *fused = nullptr,
                    bool coresident = false); // coresident: another kernel's workgroups share the CUs (ring depth 3, raised wave priority)
// ragged calls (sdrhip_decimate_ragged, sdrhip_rx_process_ragged): ragged_prepare fills the decimator fields of rows[0..S) (the
// caller's framing fields are kept), plans the launch into *plan (K1r's geometry, and K1mr's when the call goes to the matrix cores:
// plan->mfma) and uploads the table (the decimators' own device copy, valid until the next ragged call on them);
// decimate_ragged_device then runs the cascade with the table and that plan
// pin (optional): the caller's own pinned staging for the table instead of the handle's one -- an asynchronous batch passes its
// ring slot's, so that the call waits for that slot's last upload, not for the previous call's
int ragged_prepare(sdrhip_decimators *d, int log2decim, int fcpos, const size_t *n_in, RaggedRow *rows, const RaggedRow **rows_dev,
                   RaggedPlan *plan, PinnedBuf *pin = nullptr);
// its planning half alone (no upload, nothing changes): what a step with these counts will launch, for a caller that sizes buffers ahead
int ragged_plan(const sdrhip_decimators *d, int log2decim, int fcpos, const size_t *n_in, RaggedRow *rows, RaggedPlan *plan);
int ragged_reserve(sdrhip_decimators *d, PinnedBuf *pin); // the table's storage alone: nothing left to allocate in ragged_prepare
// frame_mode != 0 (only when plan.mfma): the matrix-core launch stores straight into the frame layout, `out` = the frame
// area (stream s at out + s * out_stride dwords, its window at RaggedRow out_off), meta_w / meta_rate = the shared meta words
int decimate_ragged_device(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *in, size_t in_stride,
                           int16_t *out, size_t out_stride, const RaggedRow *rows, const RaggedRow *rows_dev, const RaggedPlan &plan,
                           int frame_mode = 0, int frame_blocks = 0, const unsigned *meta_w = nullptr, unsigned meta_rate = 0);
// host rows of n_in[s] samples of esz bytes -> [S][dstride] rows the kernels read (pinned zero-copy memory for small calls, else
// `dev` through the pinned `pin`); only n_in[s] samples of row s are read
int ragged_stage_in(sdrhip_ctx *c, PinnedBuf &pin, DevBuf &dev, const void *src, size_t in_stride, const size_t *n_in, int S, size_t esz,
                    size_t dstride, const void **out);
// the context's second stream (created on first use; non-blocking, so that it never synchronises with a NULL caller stream)
int ctx_stream2(sdrhip_ctx *c, hipStream_t *out);
bool decimate_mfma_applies(const sdrhip_decimators *d, int log2decim, int fcpos, size_t n_in);
struct InterpGather { // InterpArgs::gmap / grx / grest / gframes
    const unsigned *map;
    const uint8_t *rx, *restored;
    int frames;
};
bool interpolate_gather_ok(const sdrhip_ctx *c, int log2interp); // K5w serves this ratio (interpolate4 .. 64, interp_path != valu)
struct InterpCount { // InterpArgs::count / count_stride / count_unit: per-stream input counts on the device (ragged launch)
    const int *count;
    int stride, unit;
};
// count (optional): stream s takes count[s * stride] * unit inputs, at most n_in (the grid is planned for n_in, the largest)
int interpolate_device(sdrhip_interpolators *p, int log2interp, const int16_t *in, size_t n_in, size_t in_stride, int16_t *out,
                       size_t out_stride, size_t *n_out, const InterpGather *gather = nullptr, const InterpCount *count = nullptr,
                       int out_fmt = IQF_S16, // IQF_S8: `out` holds 2-byte samples, out_stride counts them (multiple of 8 for streams > 1)
                       const int *fmt_dev = nullptr); // the format per stream (device, IQF_S16 | IQF_S8; K5x / K6x): out_fmt is unused, row s
                                                      // starts at byte 4 * s * out_stride (a multiple of 4 for streams > 1); NULL: the paths above
// FEC buffer bank (sdrhip_fecbuf.cpp) for the Tx pipe fed datagrams: the datagram arguments of sdrhip_fecbuf_write_and_read, then
// the bank's call with data_out on the device and dgrams / block0_out in `mem` memory (host: staged; block0_out downloaded on the
// context's stream, not synchronised); *counts (device) = the per-stream counts [S][FB_COUNTS] the classify pass left (FB_K: frames)
int fecbuf_check_dgrams(const sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, const char *who);
// join (the Rx pipe fed datagrams): stream s's payloads go row_off[s] samples (device) behind its data_out row; admit is called
// with the call's release counts behind the read-back, while nothing is committed: what it returns other than SDRHIP_OK refuses
// the call (nothing consumed)
struct FecBufJoin {
    const unsigned *row_off;
    int (*admit)(void *arg, const size_t *n_frames);
    void *arg;
};
int fecbuf_collect(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, uint8_t *data_out,
                   size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames,
                   const int **counts, const FecBufJoin *join = nullptr, const uint8_t *staged = nullptr);
// (staged, host memory: the datagrams are already on the device, stream s's row at staged + s * nmax * 512 -- the tagged bank call)
// the samples every stream of the collector's owner (an Rx handle) holds back between datagram calls: [nstreams] on the device
// (KJ keeps it) and the host's copy; created zero on first use, zeroed by sdrhip_fecbuf_reset
int fecbuf_join_carry(sdrhip_fecbuf *b, unsigned **dev, std::vector<size_t> **host);
// the committed half of the collector's double-buffered state, [nstreams] on the device: what launches enqueued behind the
// collector's passes of a call read (KF: m_outputMeta); the next call writes the other half
const FecBufState *fecbuf_committed_state(const sdrhip_fecbuf *b);
// asynchronous Tx / Rx batches (sdrhip_tx_submit_datagrams, sdrhip_rx_submit_datagrams): the host's shadow of the classification part
// of a stream's FecBufState
struct FecBufShadow {
    int head, count, recov, maxrow, dup;
    unsigned pres[4];
};
// the shadow of the committed state (refreshed from the device -- one copy + one synchronisation -- when something else moved the
// collector since the last asynchronous batch)
int fecbuf_shadow(sdrhip_fecbuf *b, std::vector<FecBufShadow> *out);
// the classify pass's rule over n datagrams of one stream (datagram i at dg + 512 i, host): advances h; res = what the pass reports
// for the stream, {FB_K, FB_D, FB_MAXROW, FB_MAXREC}
void fecbuf_shadow_run(FecBufShadow &h, const uint8_t *dg, size_t n, int res[4]);
// one datagram of that rule: header word hd (frameIndex | blockIndex << 16 | filler << 24) advances h and adds to res, which the
// caller starts at {0, 0, -1, 0}.  fecbuf_shadow_run is this step over a row; the walk of a tagged batch calls it in arrival order
void fecbuf_shadow_step(FecBufShadow &h, uint32_t hd, int res[4]);
// one batch on the device without a read-back: stream s's datagrams back to back at dg + sum_{t<s} n_dgrams[t] * 512 (device),
// grids and decoder bound from res ([S][4], fecbuf_shadow_run); tab = the batch's pinned table buffer; data_out / block0_out on
// the device, max_frames >= every res[s][0]; +1 on *mismatch (device) per stream whose classify pass disagrees with res.
// *committed: the state has moved on (to `next`; a failure after it loses the batch); *counts / *pub = the pass's counts
// [S][FB_COUNTS] and public records [S][max_frames] on the device (valid until the next batch).  join (asynchronous Rx batches):
// stream s's payloads go join->row_off[s] samples (device) behind its data_out row, never past the row's data_stride bytes (admit
// is not used: nothing is read back)
int fecbuf_packed(sdrhip_fecbuf *b, const uint8_t *dg, const size_t *n_dgrams, const int *res, const std::vector<FecBufShadow> &next,
                  PinnedBuf &tab, uint8_t *data_out, size_t data_stride, uint8_t *block0_out, size_t max_frames, unsigned *mismatch,
                  bool *committed, const int **counts, const FecBufPub **pub, const FecBufJoin *join = nullptr);
// a batch of an asynchronous datagram-fed pipe on its way up (sdrhip_tx_submit_datagrams, sdrhip_rx_submit_datagrams; `who` in the
// messages).  fecbuf_batch_check: the count limit, NULL dgrams and the SDRHIP_PACKED / stride rule; it fills `in` (nothing consumed).
// fecbuf_batch_stage: one memcpy per non-empty stream into the batch's pinned `arena`, packed (not at all where the caller's memory
// is pinned: in->inplace), and the shadow `sh` run over every stream's headers: res [S][4].  fecbuf_batch_upload: exactly the
// datagrams to pk (device), packed -- staged: one copy; in place: one per run of adjacent rows
// The tagged form (sdrhip_*_submit_datagrams_tagged; tags != NULL): n_total datagrams in arrival order, tags[i] = the stream of
// datagram i or SDRHIP_DGRAM_SKIP.  fecbuf_batch_check_tagged walks the tags once (a tag that names no stream refuses the batch;
// the per-stream counts, which n_dgrams then points at).  fecbuf_batch_stage: ONE memcpy of the whole array (none in place), then
// one walk in arrival order over the tags and the headers: the shadow's step for the datagram's stream and its place
// dest[i] = first datagram of its stream in packed order + its rank within the stream (0xffffffff: skipped), written into `tab`,
// the batch's pinned table buffer, behind the table fecbuf_packed fills.  fecbuf_batch_upload: the arrival array (bytes_in,
// skipped datagrams included) and dest (4 n_total bytes) go up behind the packed area of pk, and KX (launch_dgram_demux) moves
// every datagram to its place at pk: from there on the batch is an SDRHIP_PACKED one.  (`tab` is not marked: fecbuf_packed, which
// uploads its own part of it behind, does that; a caller that returns before it marks the buffer itself.)
struct FecBufBatch {
    int S;
    const uint8_t *dgrams;
    const size_t *n_dgrams;
    size_t stride;
    bool packed, inplace;       // packed: the rows lie back to back (SDRHIP_PACKED, or one stream), else row s at dgrams + s * stride
    size_t sum, nmax, bytes_in; // the streams' datagrams, the most of a stream, the bytes that go up (sum x 512; tagged: n_total x 512)
    size_t dev_bytes;           // what the device arena pk holds: bytes_in; tagged: sum x 512 packed + n_total x (512 + 4)
    // ---- the tagged form
    const uint16_t *tags = nullptr;
    size_t n_total = 0;
    std::vector<size_t> counts; // [S]
    uint32_t *dest = nullptr;   // [n_total] in the batch's pinned table buffer (fecbuf_batch_stage)
};
int fecbuf_batch_check(FecBufBatch *in, int S, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, const char *who);
int fecbuf_batch_check_tagged(FecBufBatch *in, int S, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total, const char *who);
int fecbuf_batch_stage(FecBufBatch *in, PinnedBuf &arena, PinnedBuf &tab, std::vector<FecBufShadow> &sh, int *res);
int fecbuf_batch_upload(sdrhip_ctx *c, const FecBufBatch &in, PinnedBuf &arena, uint8_t *pk);
// the per-stream counts of a tagged array into counts [S] (zeroed here); SDRHIP_EINVAL for a tag that is neither a stream of the
// bank nor SDRHIP_DGRAM_SKIP, for NULL tags or datagrams with n_total > 0, for more than 65535 streams; *sum / *nmax as count_dgrams
int fecbuf_tag_counts(int S, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total, const char *who, size_t *counts, size_t *sum,
                      size_t *nmax);
// a failure behind the collector's scatter launch: the batch is consumed and lost, never replayed
int fecbuf_batch_lost(const char *who, int rc);
// a public record as a batch delivers it
constexpr size_t DG_REC = sizeof(sdrhip_fecbuf_frame);
static_assert(sizeof(sdrhip_fecbuf_frame) == sizeof(FecBufPub), "public record layout");
// DevBuf::reserve behind a synchronisation of the context's stream when the buffer grows (it frees the old one, which batches in
// flight may still use)
inline int reserve_settled(sdrhip_ctx *c, DevBuf &b, size_t n);
// the word of sdrhip_ctx::dec_stats the shadow check counts in (sdrhip_ctx_get_counter "fecbuf_shadow_mismatch")
constexpr int DEC_STATS_SHADOW_MISMATCH = 1;
// while set, sdrhip_fecbuf_reset / sdrhip_fecbuf_write_and_read on the collector are refused (SDRHIP_EINVAL)
void fecbuf_set_async_busy(sdrhip_fecbuf *b, bool busy);
// frames/recovery on the device; recovery slots may be interleaved with the frames
// (rec_frame_bytes = stride between the recovery areas of consecutive frames)
// frame_list_dev (optional, device): groups of GF_FRAMES_PER_GROUP frame indices (-1 = none), ngroups of them
// lin (optional, Rx pipe): the payload of the frame slots >= first of every stream is taken from the stream-order output
// of the decimator and copied into the frame area by the encoder itself (Enc128Args::lin); only honoured when the
// structured encoder runs (nb_fec >= ENC128_MIN_ROWS): the caller checks fec_encode_fuses_framing()
struct EncodeLin {
    const unsigned *lin;
    size_t stride;
    int cap, first, pending;
};
// smallest number of recovery blocks the structured encoder serves: 13 for the Karatsuba walk (ENC128_MIN_ROWS: below, the generic
// matrix kernel's rows x 128 products are fewer than one 32-row tile's), enc_min_rows (default 1) for the additive FFT, whose 592
// products do not depend on the row count (profiles/r05_enc_rows.txt)
int enc128_min_rows(const sdrhip_ctx *c);
inline bool fec_encode_fuses_framing(const sdrhip_ctx *c, int nb_fec) { return nb_fec >= enc128_min_rows(c); }
int fec_encode_device(sdrhip_ctx *ctx, const uint8_t *frames, size_t frame_bytes, size_t nframes, int nb_fec, uint8_t *rec,
                      size_t rec_frame_bytes, const int32_t *frame_list_dev = nullptr, int ngroups = 0, const EncodeLin *lin = nullptr);
// the structured 128-original encoder on prepared arguments (the Rx pipe's deferred encode)
int fec_encode128_launch(sdrhip_ctx *ctx, const Enc128Args &k, hipStream_t on = nullptr); // on: another stream than the context's
// rx on the device, indices on the host; payload_out / block0_out on the device
struct DecodeSide { // decode on another stream than the context's, with the caller's own work buffers
    hipStream_t stream;
    DevBuf *plan, *idx;
    PinnedBuf *pin;
};
// no-copy decode (round 6, the Tx pipe in front of K5w): the received originals stay in rx, the restored blocks go to `restored`
// (nframes * rows + 1 slots of 508 bytes, the last one all zeros), `srcmap` ([nframes][128]) tells the interpolator where every block
// lies (InterpArgs::gmap).  Only when fec_decode_gather_ok(): the fused-plan FFT decoder is the one kernel that writes the map.
struct DecodeGather {
    unsigned *srcmap;
    uint8_t *restored;
    int rows;
};
bool fec_decode_gather_ok(const sdrhip_ctx *c);
// max_rows > 0: the promise for this batch instead of the context option dec_max_rows (the FEC buffer bank knows the rows it collected)
int fec_decode_device(sdrhip_ctx *ctx, const uint8_t *rx, size_t rx_frame_bytes, const uint8_t *indices, size_t nframes,
                      uint8_t *payload_out, size_t payload_frame_bytes, uint8_t *block0_out, const DecodeSide *side = nullptr,
                      const DecodeGather *gather = nullptr, int max_rows = 0);
// sdrhip_host_alloc memory: pinned, usable in place
bool host_is_pinned(const void *p, size_t n);

// ---- per-stream lifecycle (sdrhip_*_reset_streams, sdrhip_stream_state.cpp).  The mask of a call goes up like the Rx pipe's
// stream-meta table, as the next of its TableVersions -- a launch in flight never sees a later call's mask
typedef TableVersions StreamMask;
// counts the streams `mask` names (NULL: all S) into *n_set.  *dev = NULL when it names none or all of them (nothing is enqueued),
// else the device copy, enqueued on the context's stream
int stream_mask_upload(sdrhip_ctx *c, StreamMask &m, const uint8_t *mask, int S, const uint8_t **dev, int *n_set);
// the handles' parts of KR's arguments (*_reset_part: they change nothing), and the host side of the reset, once the launch is out
// (*_reset_done; all: every stream was reset, else `mask` names them): decimators: stage0_int16 becomes true only when every
// stream was reset; collector: a valid shadow gets the constructor's values for the streams reset (it stays valid: the next
// asynchronous batch reads nothing back), and so does the host's copy of the carry
void decimators_reset_part(sdrhip_decimators *d, StreamResetArgs *a);
void decimators_reset_done(sdrhip_decimators *d, bool all);
void interpolators_reset_part(sdrhip_interpolators *p, StreamResetArgs *a);
void fecbuf_reset_part(sdrhip_fecbuf *b, StreamResetArgs *a);
void fecbuf_reset_done(sdrhip_fecbuf *b, const uint8_t *mask); // mask NULL: every stream
void fecbuf_fresh_state(FecBufState *x); // what SDRdaemonFECBuffer's constructor leaves
int stream_reset_launch(sdrhip_ctx *c, const StreamResetArgs &a);
// ---- export / import of one stream (sdrhip_*_export_stream / _import_stream): where the handles keep stream s
// the stream's history row in the current half (half = 0: what the next call reads) or the other one
int32_t *decimators_row(sdrhip_decimators *d, int s, int half);
int32_t *interpolators_row(sdrhip_interpolators *p, int s, int half);
bool decimators_stage0_int16(const sdrhip_decimators *d);
void decimators_clear_stage0_int16(sdrhip_decimators *d); // an imported history may hold rotate-sums
struct FecBufStreamRef {
    FecBufState *st[2];   // [0]: the committed half
    uint8_t *carry;       // the stream's 128 super blocks in carry buffer 0; buffer 1 lies carry_half bytes behind
    size_t carry_half;
};
void fecbuf_stream_ref(sdrhip_fecbuf *b, int s, FecBufStreamRef *out);
// the host side of an import: a valid shadow takes the stream's classification part of `st` (it stays valid), the host's copy of
// the carry takes `carry`
void fecbuf_import_host(sdrhip_fecbuf *b, int s, const FecBufState &st, size_t carry);

} // namespace sdrhip

#define SDRHIP_KCLASSES 5 // SDRHIP_K_DECIMATE .. SDRHIP_K_CONVERT
namespace sdrhip {
// Kernel-path knobs of a context.  Read ONCE from the environment when the context is created (SDRHIP_DECIM_PATH =
// valu | mfma | auto, SDRHIP_MFMA_SPAN, SDRHIP_MFMA_MIN, SDRHIP_INTERP_PATH = valu | wave, SDRHIP_INTERP_SPAN); afterwards
// only sdrhip_ctx_set_option() changes them (tests, tools), under the context's lock.
struct CtxOptions {
    int decim_path = DECIM_PATH_AUTO;      // DECIM_PATH_*, decim_plan.h
    size_t mfma_span = 0;                  // forced span length of the matrix-core decimator (0 = planner's choice)
    size_t mfma_min = (size_t)1 << 22;     // smallest call (samples over all streams, decimate4 / 8) the matrix cores take in auto mode
    int interp_wave = 1;                   // interpolate4 .. 64: K5w, the barrier-free wave-private pipeline (interp_wave.h); 0 = K5
    size_t interp_span = 0;
    int mfma_ring = 4;                     // LDS-DMA ring depth of the decimate16 matrix-core kernel (3 or 4 groups; overlap mode always runs 3)
    // pipelined Rx pipe, where the encoder of the previous call's frames runs: 0 = its own launch behind the decimator, 1 = inside the
    // decimator's launch (rx_fused_kernel), 3 = its own launch on the context's SECOND stream, beside the decimator ("overlap")
    int rx_fused = 1;
    // Rx pipe on the matrix-core decimator: 1 = its waves store straight into the frame layout (round 5: no stream-order buffer, no
    // framing copy in the encoder, no K2 launch), 0 = stream order + K2 + the encoder's fused copy (the round-3 arrangement)
    int rx_direct = 1;
    int rx_window = 0;                     // frame window of the Rx pipe in calls (1..8); 0 = the default: 2, pipelined pipes 4 (sdrhip_rx_process)
    int tx_overlap = 1;                    // pipelined Tx pipe: 1 = decode of this batch on the second stream beside the interpolator of the previous one, 0 = one stream
    int enc_fft = 1;                       // structured 128-original encoder, rows <= 32: additive FFT (1) or the Karatsuba XOR-convolution walk (0)
    int enc_half = 0;                      // FFT encoder in half-frame workgroups (enc_units = half): finer units for the CUs, 128 threads each
    int enc_bitslice = 1;                  // FFT encoder's middle stages as bit-sliced XOR trees (enc_form = bitslice) or all in the table form (table)
    int enc_min_rows = 1;                  // ... the FFT from this many recovery blocks on (the generic matrix kernel below)
    int fec_stagger_mod = 0;               // 0: phase = resident round (workgroup / CUs); 1..16: phase = workgroup mod m; 100 + m: arrival rank on the CU mod m (experiment)
    int fec_stagger = 0;                   // staggered start of the FFT encoder's / decoder's workgroups, units of 1024 clocks per resident round (0 = off)
    // Tx pipe without the decoder's copy (built in round 6): immediate mode on K5w with the fused-plan decoder, the
    // interpolator gathers the received originals through the decoder's position map.  OFF by default: the decoder gets 11 us
    // faster per 1024 frames (0.0822 -> 0.0710 ms), the interpolator 62 us SLOWER (0.2354 -> 0.2974 ms: 48 load instructions per
    // wave instead of 8 in front of its store stream, profiles/r06_tx_gather_ab.txt)
    int tx_gather = 0;
    int dec_fused_plan = 1;                // batched decode with dec_max_rows <= 32 on the FFT decoder: the plan is made inside the decoder's launch (0: gf_decode_plan_kernel in front)
    int dec_syndrome = 1;                  // batched CM256 decode: syndrome kernel (1) or the dense matrix kernel alone (0)
    int dec_strict = 0;                    // batched decode delivers only what the reference's copy-back loop delivers (SDRdaemonFECBuffer.cpp:204-211)
    int dec_max_rows = 128;                // upper bound of the recovery blocks a received frame can have used (the sender's fecblk)
    int dec_auto = 0;                      // dec_max_rows = auto: no promise, the one-launch decoder defers per frame (fec_decode_device); dec_max_rows holds 128 meanwhile
};
// what the last decimate / rx call of a bank actually launched (sdrhip_decimators_last_plan)
struct DecimPlanInfo {
    int path = 0;       // 0 none yet, DECIM_PATH_VALU, DECIM_PATH_MFMA
    size_t span = 0, head = 0, tail_start = 0;
    int wps = 0, npieces = 0, nseg = 0;
};
} // namespace sdrhip

struct sdrhip_ctx {
    // Every public entry point that works on this context (directly or through one of its handles) holds this lock
    // for its duration: the staging buffers, the decode-plan cache and the timing log are per context.  Calls on
    // one context therefore serialise; threads that want to overlap use one context each.
    std::recursive_mutex mtx;
    int device = 0;
    int n_cu = 256;                          // hipDeviceProp_t::multiProcessorCount (the planners size their grids from it)
    sdrhip::CtxOptions opt;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;           // the library's own second stream (created on first use: overlap modes of the pipes)
    std::atomic<int> refs{0}; // handles created on this context (they keep it alive)
    std::atomic<bool> dying{false}; // sdrhip_ctx_destroy was called while handles were still alive
    sdrhip::DevBuf in, out, aux, aux3;       // staging for SDRHIP_MEM_HOST calls and FEC work areas
    uint8_t *gf_tab = nullptr;               // 256 x 32 B multiplier tables (device)
    uint8_t *enc_matrix = nullptr;           // 128 x 128 encode matrix, rows 128..255 (device)
    uint8_t *enc_leaves = nullptr;           // Karatsuba leaf tables of the structured k = 128 encoder (device)
    uint8_t *enc_fft = nullptr;              // constants of the additive-FFT form of the same encoder (device)
    unsigned *decim_dump = nullptr;          // sink of the matrix-core decimator's warm-up stores (DecimArgs::mf_dump)
    unsigned *fused_roles = nullptr;         // role table of the fused Rx launch (rx_fused_kernel), fused_tag = its launch counter
    unsigned fused_tag = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t *gf_explog = nullptr;             // exp[512] + log[256] (uint16) of GF(256) for the decode planner (device)
    sdrhip::DevBuf dec_plan;                  // per-frame decode plans of the current batch (DecodeBuffers)
    unsigned *dec_stats = nullptr;            // device counters of the batched decoder: [0] frames that broke the dec_max_rows promise, [1] DEC_STATS_SHADOW_MISMATCH, [2] DEC_STATS_DEFERRED
    sdrhip::PinnedBuf pin;                       // per-call upload staging (maps, frame lists)
    sdrhip::PinnedBuf zin, zout;                 // zero-copy staging of small host-pointer calls (the kernels read / write pinned host memory)
    // per-kernel-class timing with hipEvents on `stream` (sdrhip_ctx_kernel_timing)
    bool ktime_on = false;
    int ktime_stride = 1;                     // kernel-class timers bracket every ktime_stride-th launch of a class (option "ktime_stride")
    int ktime_stride_cls[SDRHIP_KCLASSES] = {0, 0, 0, 0, 0}; // ... per class when > 0 (option "ktime_stride_class" = "<class>:<stride>"; "ktime_stride" resets them)
    unsigned ktime_seen[SDRHIP_KCLASSES] = {0, 0, 0, 0, 0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kev[SDRHIP_KCLASSES];
    // bytes the entry points copied across the host link (sdrhip_ctx_get_counter "h2d_bytes" / "d2h_bytes"), counted when enqueued
    uint64_t h2d_bytes = 0, d2h_bytes = 0;
};

namespace sdrhip {
struct CtxLock {
    std::lock_guard<std::recursive_mutex> g;
    explicit CtxLock(sdrhip_ctx *c) : g(c->mtx) {}
};
// RAII: brackets the launches of one kernel class with events when timing is enabled
struct KTimer {
    sdrhip_ctx *c;
    int cls;
    hipEvent_t e1 = nullptr;
    hipStream_t st;
    KTimer(sdrhip_ctx *ctx, int kernel_class, hipStream_t on = nullptr) : c(ctx), cls(kernel_class), st(on ? on : ctx->stream)
    {
        if (!c->ktime_on) return;
        // (an event pair around a launch costs the stream ~2.5 us: timing every launch of a two-launch step took 3 % off the step)
        if (cls >= 0 && cls < SDRHIP_KCLASSES) {
            const int stride = c->ktime_stride_cls[cls] > 0 ? c->ktime_stride_cls[cls] : c->ktime_stride;
            if (stride > 1 && (c->ktime_seen[cls]++ % (unsigned)stride) != 0) return;
        }
        hipEvent_t e0 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess) return;
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); e1 = nullptr; return; }
        (void)hipEventRecord(e0, st);
        c->kev[cls].push_back(std::make_pair(e0, e1));
    }
    ~KTimer()
    {
        if (e1) (void)hipEventRecord(e1, st);
    }
};
inline int reserve_settled(sdrhip_ctx *c, DevBuf &b, size_t n)
{
    if (n > b.cap && b.p && hipStreamSynchronize(c->stream) != hipSuccess) return fail(SDRHIP_EDEVICE, "hipStreamSynchronize");
    return b.reserve(n);
}
// a copy across the host link of `bytes` (hipMemcpyHostToDevice / DeviceToHost; anything else is not counted)
inline void link_bytes(sdrhip_ctx *c, hipMemcpyKind kind, size_t bytes)
{
    if (kind == hipMemcpyHostToDevice) c->h2d_bytes += bytes;
    else if (kind == hipMemcpyDeviceToHost) c->d2h_bytes += bytes;
}
// hipMemcpyAsync / hipMemcpy2DAsync on the context's behalf: the bytes of a copy across the host link are counted (link_bytes)
// when it was enqueued
inline hipError_t link_copy(sdrhip_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    if (e == hipSuccess) link_bytes(c, kind, bytes);
    return e;
}
inline hipError_t link_copy2d(sdrhip_ctx *c, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                              hipMemcpyKind kind, hipStream_t stream)
{
    const hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, stream);
    if (e == hipSuccess) link_bytes(c, kind, width * height);
    return e;
}
// the whole call of every reset entry, banks and pipes alike: mask up, `fill` the handle's parts of the arguments, KR, and only
// behind a launch that went out `done(mask)`, the host's bookkeeping (mask NULL: every stream was reset)
template <class F, class D> int stream_reset_bank(sdrhip_ctx *c, StreamMask &m, const uint8_t *mask, int S, F fill, D done)
{
    HIP_TRY(hipSetDevice(c->device));
    StreamResetArgs a;
    memset(&a, 0, sizeof(a));
    int n_set = 0;
    if (int rc = stream_mask_upload(c, m, mask, S, &a.mask, &n_set)) return rc;
    if (n_set == 0) return SDRHIP_OK; // (an all-zero mask launches nothing)
    a.nstreams = S;
    fill(&a);
    if (int rc = stream_reset_launch(c, a)) return rc;
    done(n_set == S ? nullptr : mask);
    return SDRHIP_OK;
}
} // namespace sdrhip
