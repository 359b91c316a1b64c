// rx_async_kernels.hip -- the kernels of asynchronous ragged Rx batches (sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged).
//
//  * K0p: the batch's packed upload (block-major, stream-minor segments) -> the [stream][dstride] int16 rows that K1mr / K1r read,
//    8-bit input widened on the way (one pass, not two).  1-D grid: each stream gets ceil(total / UNPACKX_WG_SAMPLES) workgroups,
//    found by a binary search over the per-stream prefix (as K1r finds its stream); the workgroup's part of the row is
//    rx_unpack_body.h's walk over the table of rx_unpack_plan.h, with the bank's format as a template argument.  An 8-bit batch may
//    have a segment at an odd 2-byte unit (behind an odd count): the ODD body.  An int16 batch has every segment at an even one.
//  * frame gather: the frames each stream delivered (in its own window of the frame area) -> one contiguous buffer in stream
//    order, so that ONE download carries exactly the frames.  16-byte copies, one workgroup row per frame.
// No kernel reads a packed sample outside the batch (K0p's odd-start 8-bit loads read at most 2 bytes past a segment, inside the
// upload's 64-byte pad) and neither uses scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

#include "rx_unpack_body.h"

template <int FMT> __global__ __launch_bounds__(256) void unpack_packed_kernel(const uint8_t *packed, unsigned *out, size_t out_stride,
                                                                                const UnpackXRow *rows, const UnpackXSeg *segs, int nstreams)
{
    const uint32_t b = blockIdx.x;
    const int s = unpack_find_row(rows, nstreams, b);
    const UnpackXRow r = rows[s]; // (r.fmt is the template argument's value and is not read)
    const uint32_t d0 = (b - r.wg0) * UNPACKX_WG_SAMPLES;
    const uint32_t d1 = d0 + UNPACKX_WG_SAMPLES < r.total ? d0 + UNPACKX_WG_SAMPLES : r.total;
    unpack_body<FMT, FMT != IQF_S16>(reinterpret_cast<const uint16_t *>(packed), out + (size_t)s * out_stride, segs + r.seg0, (int)r.nseg, r.total, d0, d1);
}

__global__ __launch_bounds__(256) void frame_gather_kernel(const uint8_t *area, size_t frame_bytes, const int32_t *list, uint8_t *out)
{
    const size_t f = blockIdx.x;
    const rxu_uint4_t *src = reinterpret_cast<const rxu_uint4_t *>(area + (size_t)list[f] * frame_bytes);
    rxu_uint4_t *dst = reinterpret_cast<rxu_uint4_t *>(out + f * frame_bytes);
    const size_t n16 = frame_bytes / 16;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.y * 256) dst[i] = SDRHIP_STREAM_LOAD(src + i);
}

} // namespace

hipError_t launch_unpack_packed(int fmt, const uint8_t *packed, int16_t *out, size_t out_stride, const UnpackXRow *rows, const UnpackXSeg *segs,
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
