// tx_async_kernels.hip -- the kernels of asynchronous datagram-fed Tx batches (sdrhip_tx_submit_datagrams /
// sdrhip_tx_collect_datagrams).
//
//  * the collector's passes: the packed instantiations of fecbuf_passes.h (classify, scatter, a guarded copy), the same text as the
//    FEC buffer bank's kernels (fecbuf_kernels.hip) with a stream's datagrams back to back at a per-stream offset.
//  * shadow check: the host plans a batch's grids from its own run of the classify rule over the headers (the shadow, no
//    read-back); one thread per stream compares the classify pass's counts with the host's and raises the context counter
//    "fecbuf_shadow_mismatch" when they differ.
//  * delivery gather: the samples each stream delivered (in its [stream][pitch] row), the frames' records and meta blocks ->
//    one contiguous buffer, so that ONE download carries exactly the delivered bytes.  A segment table lists the pieces; a
//    segment gets ceil(16-byte-aligned interior / 16 KiB) workgroups (found by binary search, as K0p finds its stream), every
//    lane stores whole 16-byte chunks of the output, four in flight.  A chunk's source is dword-aligned (one 16-byte load) or, with
//    8-bit samples at x1, 2 bytes off (five dwords realigned); the unaligned head and tail of a segment (< 16 bytes each) go by
//    2-byte units.  Every segment is a multiple of 2 bytes and starts on a dword.
// No kernel here uses scratch.  The gather reads at most 2 bytes past a segment (the realigned path), inside the source buffer's pad.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned tg_uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned tg_uint4a4_t __attribute__((ext_vector_type(4), aligned(4))); // 16-byte load from a dword-aligned address

#define FB_PACKED 1
#include "fecbuf_passes.h"
#undef FB_PACKED

constexpr int GA_NT = 256;
constexpr int GA_PER_LANE = 4; // 16-byte chunks per lane and workgroup

__global__ __launch_bounds__(64) void fecbuf_shadow_check_kernel(const int *counts, const int *expect, int nstreams, unsigned *mismatch)
{
    const int s = (int)(blockIdx.x * 64 + threadIdx.x);
    if (s >= nstreams) return;
    const int *c = counts + (size_t)s * FB_COUNTS, *e = expect + (size_t)s * 4;
    if (c[FB_K] != e[0] || c[FB_D] != e[1] || c[FB_MAXROW] != e[2] || c[FB_MAXREC] != e[3]) atomicAdd(mismatch, 1u);
}

// the last segment of [0, nseg) whose first workgroup is at or before b
__device__ __forceinline__ int ga_find(const GatherSeg *segs, int nseg, uint32_t b)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].wg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ tg_uint4_t ga_load16(const uint8_t *p)
{
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        const tg_uint4a4_t v = *reinterpret_cast<const tg_uint4a4_t *>(p);
        return (tg_uint4_t){v.x, v.y, v.z, v.w};
    }
    const uint8_t *q = p - 2; // (2 bytes off: the dwords around the chunk, realigned)
    const tg_uint4a4_t v = *reinterpret_cast<const tg_uint4a4_t *>(q);
    const unsigned e = reinterpret_cast<const unsigned *>(q)[4];
    return (tg_uint4_t){__builtin_amdgcn_alignbit(v.y, v.x, 16), __builtin_amdgcn_alignbit(v.z, v.y, 16),
                        __builtin_amdgcn_alignbit(v.w, v.z, 16), __builtin_amdgcn_alignbit(e, v.w, 16)};
}

__global__ __launch_bounds__(GA_NT) void delivery_gather_kernel(const GatherSeg *segs, int nseg, uint8_t *out)
{
    const uint32_t b = blockIdx.x;
    const GatherSeg g = segs[ga_find(segs, nseg, b)];
    const uint64_t D = g.dst, E = g.dst + g.bytes;
    uint64_t A0 = (D + 15) & ~(uint64_t)15, A1 = E & ~(uint64_t)15;
    if (A0 > A1) A0 = A1 = E; // (the segment lies inside one 16-byte chunk: all of it is head)
    const int t = (int)threadIdx.x;
    if (b == g.wg0) { // head [D, A0) and tail [A1, E), 2 bytes at a time
        for (uint64_t x = D + 2 * (uint64_t)t; x < A0; x += 2 * GA_NT)
            *reinterpret_cast<uint16_t *>(out + x) = *reinterpret_cast<const uint16_t *>(g.src + (x - D));
        for (uint64_t x = A1 + 2 * (uint64_t)t; x < E; x += 2 * GA_NT)
            *reinterpret_cast<uint16_t *>(out + x) = *reinterpret_cast<const uint16_t *>(g.src + (x - D));
    }
    const uint64_t c0 = A0 + (uint64_t)(b - g.wg0) * GATHER_WG_BYTES;
    tg_uint4_t v[GA_PER_LANE];
#pragma unroll
    for (int j = 0; j < GA_PER_LANE; ++j) {
        const uint64_t c = c0 + 16 * (uint64_t)(t + j * GA_NT);
        if (c < A1) v[j] = ga_load16(g.src + (c - D));
    }
#pragma unroll
    for (int j = 0; j < GA_PER_LANE; ++j) {
        const uint64_t c = c0 + 16 * (uint64_t)(t + j * GA_NT);
        if (c < A1) *reinterpret_cast<tg_uint4_t *>(out + c) = v[j];
    }
}

} // namespace

hipError_t launch_fecbuf_classify_packed(const FecBufArgs &a, const long long *dg_off, hipStream_t stream)
{
    hipLaunchKernelGGL(fecbuf_classify_packed_kernel, dim3(a.nstreams), dim3(CL_NT), 0, stream, a, dg_off);
    return hipGetLastError();
}

hipError_t launch_fecbuf_scatter_packed(const FecBufArgs &a, const long long *dg_off, int njobs, int nslots, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_scatter_packed_kernel, dim3(njobs), dim3(SC_NT), 0, stream, a, dg_off, nslots);
    return hipGetLastError();
}

hipError_t launch_fecbuf_copy_guarded(const FecBufArgs &a, int nslots, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_copy_guarded_kernel, dim3(nslots), dim3(SC_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fecbuf_shadow_check(const int *counts, const int *expect, int nstreams, unsigned *mismatch, hipStream_t stream)
{
    if (nstreams <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_shadow_check_kernel, dim3((unsigned)(nstreams + 63) / 64), dim3(64), 0, stream, counts, expect, nstreams, mismatch);
    return hipGetLastError();
}

uint32_t gather_plan(GatherSeg *segs, int nseg)
{
    uint64_t wg = 0;
    for (int i = 0; i < nseg; ++i) {
        segs[i].wg0 = (uint32_t)wg;
        const uint64_t D = segs[i].dst, E = D + segs[i].bytes;
        const uint64_t A0 = (D + 15) & ~(uint64_t)15, A1 = E & ~(uint64_t)15;
        const uint64_t body = A1 > A0 ? A1 - A0 : 0;
        wg += body ? (body + GATHER_WG_BYTES - 1) / GATHER_WG_BYTES : 1;
        if (wg > 0x7fffffffu) return 0;
    }
    return (uint32_t)wg;
}

hipError_t launch_delivery_gather(const GatherSeg *segs, int nseg, uint32_t grid, uint8_t *out, hipStream_t stream)
{
    if (nseg <= 0 || grid == 0) return hipSuccess;
    hipLaunchKernelGGL(delivery_gather_kernel, dim3(grid), dim3(GA_NT), 0, stream, segs, nseg, out);
    return hipGetLastError();
}

} // namespace sdrhip
