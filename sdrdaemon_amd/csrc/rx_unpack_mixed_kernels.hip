// rx_unpack_mixed_kernels.hip -- K0x: the unpack pass of sample-fed blocks whose rows differ in format (sdrhip_rx_set_stream_format).
//
// K0x is K0p (rx_async_kernels.hip) with the format taken from the stream's row of the per-call table (rx_unpack_plan.h) instead of
// a template argument, and with segment sources counted in 2-byte units instead of samples: rows of int16 and of 8-bit samples share
// one source -- a batch's packed upload, the staged rows of a synchronous host call, or a caller's strided device rows -- and come
// out as the [stream][dstride] int16 rows that K1mr / K1r / the filter-less kernel read.  The split of the work is K0p's: a 1-D grid,
// each stream's ceil(total / UNPACKX_WG_SAMPLES) workgroups found by a binary search over the rows' prefix; a workgroup serves ONE
// stream, so its format is uniform: one branch per workgroup into one of three bodies, none per sample.  Every lane writes
// 16-byte-aligned chunks of its row (4 int16 samples, or 8 widened 8-bit samples as two 16-byte stores); a chunk that lies wholly in
// one segment is read with one 16-byte load, one that straddles segments or the row's end is assembled per sample.
// New against K0p: an int16 segment may start at an odd 2-byte unit (behind an odd number of 8-bit samples of a packed batch); its
// chunks are then read as the dwords around them and realigned by 2 bytes, the way K0p realigns an odd 8-bit start.
// Reads: a chunk's own 16 bytes; a realigned chunk the 2 bytes in front of it (inside the source: its unit is odd, so at least 1)
// and 2 behind it (inside the upload's 64-byte pad at the very end).  Strided device rows start on 16 bytes, so no chunk of theirs is
// realigned, and the per-sample path reads a sample's own bytes alone: nothing outside a row's n * bytes(fmt) bytes.  No scratch, no LDS.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned ux_uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned ux_uint4a4_t __attribute__((ext_vector_type(4), aligned(4))); // 16-byte load from a dword-aligned address

// convert_kernels.hip's rule: two samples {re, im, re, im} of one dword -> two IQSample dwords (U8 = S8 behind one XOR)
template <int FMT> __device__ __forceinline__ void ux_widen2(unsigned x, unsigned &lo, unsigned &hi)
{
    if (FMT == IQF_U8) x ^= 0x80808080u;
    const int b0 = (int)(x << 24) >> 24, b1 = (int)(x << 16) >> 24, b2 = (int)(x << 8) >> 24, b3 = (int)x >> 24;
    lo = ((unsigned)b0 & 0xffffu) | ((unsigned)b1 << 16);
    hi = ((unsigned)b2 & 0xffffu) | ((unsigned)b3 << 16);
}

// the sample at 2-byte unit u as an int16 IQ dword (an int16 sample may sit 2 bytes off a dword: two 2-byte loads)
template <int FMT> __device__ __forceinline__ unsigned ux_sample(const uint16_t *src, uint64_t u)
{
    if (FMT == IQF_S16) return (unsigned)src[u] | ((unsigned)src[u + 1] << 16);
    unsigned lo, hi;
    ux_widen2<FMT>((unsigned)src[u], lo, hi);
    return lo;
}

// the last segment of [lo, hi] that starts at or before row sample x
__device__ __forceinline__ int ux_find(const UnpackXSeg *segs, int lo, int hi, uint32_t x)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].dst <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// one workgroup's part [d0, d1) of a row of format FMT
template <int FMT> __device__ __forceinline__ void ux_body(const uint16_t *src, unsigned *orow, const UnpackXSeg *sg, int nseg, uint32_t total,
                                                           uint32_t d0, uint32_t d1)
{
    constexpr uint32_t SPC = FMT == IQF_S16 ? 4 : 8; // row samples per lane and chunk
    constexpr uint32_t UPS = FMT == IQF_S16 ? 2 : 1; // 2-byte units per sample
    const int k0 = ux_find(sg, 0, nseg - 1, d0), k1 = ux_find(sg, k0, nseg - 1, d1 - 1);
    for (uint32_t c = d0 + threadIdx.x * SPC; c < d1; c += 256 * SPC) {
        int k = ux_find(sg, k0, k1, c);
        const UnpackXSeg g = sg[k];
        unsigned w[SPC];
        if (c + SPC <= g.dst + g.n) { // the chunk lies in one segment: one 16-byte load
            const uint64_t u = g.src + (uint64_t)(c - g.dst) * UPS;
            unsigned x[4];
            if ((u & 1) == 0) {
                const ux_uint4a4_t v = *reinterpret_cast<const ux_uint4a4_t *>(src + u);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else { // (odd unit: the dwords around the chunk, realigned by 2 bytes)
                const uint16_t *p = src + u - 1;
                const ux_uint4a4_t v = *reinterpret_cast<const ux_uint4a4_t *>(p);
                const unsigned e = reinterpret_cast<const unsigned *>(p)[4];
                x[0] = __builtin_amdgcn_alignbit(v.y, v.x, 16);
                x[1] = __builtin_amdgcn_alignbit(v.z, v.y, 16);
                x[2] = __builtin_amdgcn_alignbit(v.w, v.z, 16);
                x[3] = __builtin_amdgcn_alignbit(e, v.w, 16);
            }
            if constexpr (FMT == IQF_S16) {
                w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) ux_widen2<FMT>(x[j], w[2 * j], w[2 * j + 1]);
            }
        } else { // the chunk straddles segments or the row's end: sample by sample
#pragma unroll
            for (uint32_t j = 0; j < SPC; ++j) {
                const uint32_t i = c + j;
                w[j] = 0;
                if (i >= total) continue;
                while (sg[k].dst + sg[k].n <= i) ++k;
                w[j] = ux_sample<FMT>(src, sg[k].src + (uint64_t)(i - sg[k].dst) * UPS);
            }
        }
        ux_uint4_t *o = reinterpret_cast<ux_uint4_t *>(orow + c);
        o[0] = (ux_uint4_t){w[0], w[1], w[2], w[3]};
        if constexpr (SPC == 8) o[1] = (ux_uint4_t){w[4], w[5], w[6], w[7]};
    }
}

__global__ __launch_bounds__(256) void unpack_mixed_kernel(const uint16_t *src, unsigned *out, size_t out_stride, const UnpackXRow *rows,
                                                           const UnpackXSeg *segs, int nstreams)
{
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].wg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int s = lo;
    const UnpackXRow r = rows[s];
    const UnpackXSeg *sg = segs + r.seg0;
    const uint32_t d0 = (b - r.wg0) * UNPACKX_WG_SAMPLES;
    if (d0 >= r.total) return; // (cannot happen with rx_unpack_plan.h's grid: an empty row has no workgroup)
    const uint32_t d1 = d0 + UNPACKX_WG_SAMPLES < r.total ? d0 + UNPACKX_WG_SAMPLES : r.total;
    unsigned *orow = out + (size_t)s * out_stride;
    // (blockIdx alone decides the row: the format is the same for every lane of the workgroup)
    if (r.fmt == IQF_S16) ux_body<IQF_S16>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
    else if (r.fmt == IQF_U8) ux_body<IQF_U8>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
    else ux_body<IQF_S8>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
}

} // namespace

hipError_t launch_unpack_mixed(const void *src, int16_t *out, size_t out_stride, const UnpackXRow *rows, const UnpackXSeg *segs, int nstreams,
                               unsigned grid, hipStream_t stream)
{
    if (grid == 0) return hipSuccess;
    if (nstreams <= 0 || (out_stride & 7) || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(src) & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(unpack_mixed_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const uint16_t *>(src), reinterpret_cast<unsigned *>(out),
                       out_stride, rows, segs, nstreams);
    return hipGetLastError();
}

} // namespace sdrhip
