// stream_state_kernels.hip -- per-stream lifecycle (sdrhip_*_reset_streams): one stream of a bank back to what the reference's
// constructors leave (Decimators.h:56-70 / Interpolators.h:47-52: zero histories, EO1.h:171-188; SDRdaemonFECBuffer.cpp:28-52),
// while the other streams of the bank run on.
//
// KR: ONE launch per call, grid = (stream, piece of state).  Piece 0 / 1 = the stream's filter-history row in the first / second
// half of the double buffer -- both, because a ragged call that feeds the stream nothing copies "its history as it was" from
// whichever half is current --; the last piece (handles with a collector) = the stream's FecBufState in both halves and the
// samples it holds back.  Every workgroup reads the device copy of the call's mask and leaves an unmasked stream untouched.
// Stores are 16-byte (rows) or 4-byte (state words) vector stores.
//
// KG / KS (sdrhip_*_export_stream / _import_stream): one stream's scattered state -- its history row, its open frame, its
// FecBufState, the carry buffer of its open collector slot, the samples it holds back -- gathered into one contiguous device blob
// (one copy to the host instead of a dozen), and scattered back from one uploaded blob.  The segments come in the kernel's
// arguments; KG picks the carry buffer from the state on the device (the host never reads cbuf back), KS also stores the stream's
// held-back count.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {
constexpr int SR_NT = 256;
constexpr int FB_STATE_WORDS = (int)(sizeof(FecBufState) / sizeof(unsigned));
static_assert(sizeof(FecBufState) % sizeof(unsigned) == 0 && FB_STATE_WORDS <= SR_NT - 1, "one lane per state word, one for the carry");
static_assert(DEC_STATE_WORDS % 4 == 0 && INT_STATE_WORDS % 4 == 0, "history rows are stored in 16-byte pieces");

__global__ __launch_bounds__(SR_NT) void stream_reset_kernel(StreamResetArgs a)
{
    const int s = (int)blockIdx.x, piece = (int)blockIdx.y, t = (int)threadIdx.x;
    if (s >= a.nstreams) return;
    if (a.mask && a.mask[s] == 0) return; // (workgroup-uniform)
    const int row_pieces = a.rows[0] ? 2 : 0;
    if (piece < row_pieces) {
        uint4 *row = reinterpret_cast<uint4 *>(a.rows[piece] + (size_t)s * (size_t)a.row_words);
        const int n16 = a.row_words >> 2;
        for (int i = t; i < n16; i += SR_NT) row[i] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    if (piece == row_pieces && a.fb[0]) {
        if (t < FB_STATE_WORDS) {
            // (a by-value kernel argument indexed with the lane id: the 28 words lie in the kernarg segment, each lane loads its own
            // word from there -- one dword load per lane, no private copy; fecbuf_fresh_state() on the host stays the one
            // definition of the constructor's values)
            const unsigned v = a.fb_init.w[t];
            reinterpret_cast<unsigned *>(a.fb[0] + s)[t] = v;
            reinterpret_cast<unsigned *>(a.fb[1] + s)[t] = v;
        } else if (t == FB_STATE_WORDS && a.carry) {
            a.carry[s] = 0u;
        }
    }
}

// KG (GATHER) / KS: the 16-byte chunks of the segment that holds workgroup blockIdx.x.  (One body on the kernel's own argument
// block: handing the block to a helper by reference makes the compiler keep a private copy of it in scratch.)
template <bool GATHER> __global__ __launch_bounds__(SR_NT) void stream_copy_kernel(StreamCopyArgs a)
{
    const uint32_t w = blockIdx.x;
    int i = 0;
#pragma unroll
    for (int k = 1; k < STREAM_COPY_MAX_SEGS; ++k)
        if (k < a.nseg && a.seg[k].wg0 <= w) i = k;
    // (the segment's fields picked with compares, not a dynamic index into the argument block)
    const uint8_t *src = a.seg[0].src;
    uint8_t *dst = a.seg[0].dst;
    uint32_t bytes = a.seg[0].bytes, wg0 = a.seg[0].wg0;
#pragma unroll
    for (int k = 1; k < STREAM_COPY_MAX_SEGS; ++k)
        if (i == k) { src = a.seg[k].src; dst = a.seg[k].dst; bytes = a.seg[k].bytes; wg0 = a.seg[k].wg0; }
    // KG: the carry buffer that holds the open slot, from the state on the device (scalar load; 0 / 1 are the only buffers there are)
    if (GATHER && a.carry_seg >= 0 && i == a.carry_seg && (a.cbuf_from->cbuf & 1)) src += a.carry_half;
    const uint32_t n16 = bytes >> 4, first = (w - wg0) * (STREAM_COPY_WG_BYTES >> 4);
    const uint4 *s16 = reinterpret_cast<const uint4 *>(src);
    uint4 *d16 = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int k = 0; k < (int)(STREAM_COPY_WG_BYTES >> 4) / SR_NT; ++k) {
        const uint32_t c = first + (uint32_t)k * SR_NT + threadIdx.x;
        if (c < n16) d16[c] = s16[c];
    }
    // KS: the stream's count of held-back samples
    if (!GATHER && a.word_dst && blockIdx.x == 0 && threadIdx.x == 0) *a.word_dst = a.word_val;
}
} // namespace

uint32_t stream_copy_plan(StreamCopyArgs *a)
{
    if (a->nseg <= 0 || a->nseg > STREAM_COPY_MAX_SEGS) return 0;
    uint32_t grid = 0;
    for (int i = 0; i < a->nseg; ++i) {
        StreamCopySeg &g = a->seg[i];
        if (!g.src || !g.dst || g.bytes == 0 || (g.bytes & 15u) || (reinterpret_cast<uintptr_t>(g.src) & 15u) || (reinterpret_cast<uintptr_t>(g.dst) & 15u)) return 0;
        g.wg0 = grid;
        grid += (g.bytes + STREAM_COPY_WG_BYTES - 1) / STREAM_COPY_WG_BYTES;
    }
    return grid;
}

hipError_t launch_stream_gather(const StreamCopyArgs &a, uint32_t grid, hipStream_t stream)
{
    if (!grid || (a.carry_seg >= 0 && (a.carry_seg >= a.nseg || !a.cbuf_from || (a.carry_half & 15u)))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_copy_kernel<true>, dim3(grid), dim3(SR_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stream_scatter(const StreamCopyArgs &a, uint32_t grid, hipStream_t stream)
{
    if (!grid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_copy_kernel<false>, dim3(grid), dim3(SR_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_stream_reset(const StreamResetArgs &a, hipStream_t stream)
{
    const int pieces = (a.rows[0] ? 2 : 0) + (a.fb[0] ? 1 : 0);
    if (a.nstreams <= 0 || pieces == 0) return hipSuccess;
    if (a.rows[0] && (!a.rows[1] || a.row_words <= 0 || (a.row_words & 3))) return hipErrorInvalidValue;
    if (a.fb[0] && !a.fb[1]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_reset_kernel, dim3((unsigned)a.nstreams, (unsigned)pieces), dim3(SR_NT), 0, stream, a);
    return hipGetLastError();
}
} // namespace sdrhip
