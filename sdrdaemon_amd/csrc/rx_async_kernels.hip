// rx_async_kernels.hip -- the kernels of asynchronous ragged Rx batches (sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged).
//
//  * K0p: the batch's packed upload (block-major, stream-minor segments) -> the [stream][dstride] int16 rows that K1mr / K1r read,
//    8-bit input widened on the way (one pass, not two).  1-D grid: each stream gets ceil(total / UNPACK_WG_SAMPLES) workgroups,
//    found by a binary search over the per-stream prefix (as K1r finds its stream); a workgroup finds the segments that hold its
//    first and last sample by binary search over the stream's segment starts.  Every lane writes 16-byte-aligned chunks of its
//    row (4 int16 samples, or 8 widened 8-bit samples as two 16-byte stores), so no two lanes share a chunk; a chunk that lies
//    wholly in one segment is read with one 16-byte load, one that straddles segments or the row's end is assembled per sample.
//  * frame gather: the frames each stream delivered (in its own window of the frame area) -> one contiguous buffer in stream
//    order, so that ONE download carries exactly the frames.  16-byte copies, one workgroup row per frame.
// No kernel reads a packed sample outside the batch (K0p's odd-start 8-bit loads read at most 2 bytes past a segment, inside the
// upload's 64-byte pad) and neither uses scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned pk_uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned pk_uint4a4_t __attribute__((ext_vector_type(4), aligned(4))); // 16-byte load from a dword-aligned address

// convert_kernels.hip's rule: two samples {re, im, re, im} of one dword -> two IQSample dwords (U8 = S8 behind one XOR)
template <int FMT> __device__ __forceinline__ void pk_widen2(unsigned x, unsigned &lo, unsigned &hi)
{
    if (FMT == IQF_U8) x ^= 0x80808080u;
    const int b0 = (int)(x << 24) >> 24, b1 = (int)(x << 16) >> 24, b2 = (int)(x << 8) >> 24, b3 = (int)x >> 24;
    lo = ((unsigned)b0 & 0xffffu) | ((unsigned)b1 << 16);
    hi = ((unsigned)b2 & 0xffffu) | ((unsigned)b3 << 16);
}

// one packed sample as an int16 IQ dword
template <int FMT> __device__ __forceinline__ unsigned pk_sample(const uint8_t *packed, uint64_t i)
{
    if (FMT == IQF_S16) return reinterpret_cast<const unsigned *>(packed)[i];
    const unsigned x = (unsigned)reinterpret_cast<const uint16_t *>(packed)[i];
    unsigned lo, hi;
    pk_widen2<FMT>(x, lo, hi);
    return lo;
}

// the last segment of [lo, hi] that starts at or before row sample x
__device__ __forceinline__ int pk_find(const PackSeg *segs, int lo, int hi, uint32_t x)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].dst <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <int FMT> __global__ __launch_bounds__(256) void unpack_packed_kernel(const uint8_t *packed, unsigned *out, size_t out_stride,
                                                                                const PackRow *rows, const PackSeg *segs, int nstreams)
{
    constexpr uint32_t SPC = FMT == IQF_S16 ? 4 : 8; // row samples per lane and chunk
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].wg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int s = lo;
    const PackRow r = rows[s];
    const PackSeg *sg = segs + r.seg0;
    const uint32_t d0 = (b - r.wg0) * UNPACK_WG_SAMPLES;
    const uint32_t d1 = d0 + UNPACK_WG_SAMPLES < r.total ? d0 + UNPACK_WG_SAMPLES : r.total;
    const int k0 = pk_find(sg, 0, (int)r.nseg - 1, d0), k1 = pk_find(sg, k0, (int)r.nseg - 1, d1 - 1);
    unsigned *orow = out + (size_t)s * out_stride;
    for (uint32_t c = d0 + threadIdx.x * SPC; c < d1; c += 256 * SPC) {
        int k = pk_find(sg, k0, k1, c);
        const PackSeg g = sg[k];
        unsigned w[SPC];
        if (c + SPC <= g.dst + g.n) { // the chunk lies in one segment: one 16-byte load
            const uint64_t si = g.src + (c - g.dst);
            if constexpr (FMT == IQF_S16) {
                const pk_uint4a4_t v = *reinterpret_cast<const pk_uint4a4_t *>(packed + 4 * si);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                unsigned x[4];
                if ((si & 1) == 0) {
                    const pk_uint4a4_t v = *reinterpret_cast<const pk_uint4a4_t *>(packed + 2 * si);
                    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                } else { // (odd start: the dwords around it, realigned by 2 bytes)
                    const uint8_t *p = packed + 2 * si - 2;
                    const pk_uint4a4_t v = *reinterpret_cast<const pk_uint4a4_t *>(p);
                    const unsigned e = reinterpret_cast<const unsigned *>(p)[4];
                    x[0] = __builtin_amdgcn_alignbit(v.y, v.x, 16);
                    x[1] = __builtin_amdgcn_alignbit(v.z, v.y, 16);
                    x[2] = __builtin_amdgcn_alignbit(v.w, v.z, 16);
                    x[3] = __builtin_amdgcn_alignbit(e, v.w, 16);
                }
                for (int j = 0; j < 4; ++j) pk_widen2<FMT>(x[j], w[2 * j], w[2 * j + 1]);
            }
        } else { // the chunk straddles segments or the row's end: sample by sample
            for (uint32_t j = 0; j < SPC; ++j) {
                const uint32_t i = c + j;
                w[j] = 0;
                if (i >= r.total) continue;
                while (sg[k].dst + sg[k].n <= i) ++k;
                w[j] = pk_sample<FMT>(packed, sg[k].src + (i - sg[k].dst));
            }
        }
        pk_uint4_t *o = reinterpret_cast<pk_uint4_t *>(orow + c);
        o[0] = (pk_uint4_t){w[0], w[1], w[2], w[3]};
        if constexpr (SPC == 8) o[1] = (pk_uint4_t){w[4], w[5], w[6], w[7]};
    }
}

__global__ __launch_bounds__(256) void frame_gather_kernel(const uint8_t *area, size_t frame_bytes, const int32_t *list, uint8_t *out)
{
    const size_t f = blockIdx.x;
    const pk_uint4_t *src = reinterpret_cast<const pk_uint4_t *>(area + (size_t)list[f] * frame_bytes);
    pk_uint4_t *dst = reinterpret_cast<pk_uint4_t *>(out + f * frame_bytes);
    const size_t n16 = frame_bytes / 16;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.y * 256) dst[i] = SDRHIP_STREAM_LOAD(src + i);
}

} // namespace

hipError_t launch_unpack_packed(int fmt, const uint8_t *packed, int16_t *out, size_t out_stride, const PackRow *rows, const PackSeg *segs,
                                int nstreams, unsigned grid, hipStream_t stream)
{
    if (grid == 0) return hipSuccess;
    unsigned *o = reinterpret_cast<unsigned *>(out);
    if (fmt == IQF_S16) hipLaunchKernelGGL((unpack_packed_kernel<IQF_S16>), dim3(grid), dim3(256), 0, stream, packed, o, out_stride, rows, segs, nstreams);
    else if (fmt == IQF_U8) hipLaunchKernelGGL((unpack_packed_kernel<IQF_U8>), dim3(grid), dim3(256), 0, stream, packed, o, out_stride, rows, segs, nstreams);
    else if (fmt == IQF_S8) hipLaunchKernelGGL((unpack_packed_kernel<IQF_S8>), dim3(grid), dim3(256), 0, stream, packed, o, out_stride, rows, segs, nstreams);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_frame_gather(const uint8_t *area, size_t frame_bytes, const int32_t *list, size_t nframes, uint8_t *out, hipStream_t stream)
{
    if (nframes == 0) return hipSuccess;
    if (nframes > 0x7fffffffu || (frame_bytes & 15)) return hipErrorInvalidValue;
    // (a frame is 64..128 KiB: four workgroups of 256 lanes per frame copy 16..32 KiB each)
    hipLaunchKernelGGL(frame_gather_kernel, dim3((unsigned)nframes, 4), dim3(256), 0, stream, area, frame_bytes, list, out);
    return hipGetLastError();
}

} // namespace sdrhip
