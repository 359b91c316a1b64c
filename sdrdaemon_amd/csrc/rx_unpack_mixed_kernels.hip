// rx_unpack_mixed_kernels.hip -- K0x: the unpack pass of sample-fed blocks whose rows differ in format (sdrhip_rx_set_stream_format).
//
// Rows of int16 and of 8-bit samples share one source -- a batch's packed upload, the staged rows of a synchronous host call, or a
// caller's strided device rows -- and come out as the [stream][dstride] int16 rows that K1mr / K1r / the filter-less kernel read.
// The walk is rx_unpack_body.h's, the one K0p (rx_async_kernels.hip) runs, over the same table (rx_unpack_plan.h): a 1-D grid, each
// stream's ceil(total / UNPACKX_WG_SAMPLES) workgroups found by a binary search over the rows' prefix.  What K0x adds: the format
// comes from the stream's row of the table instead of a template argument -- a workgroup serves ONE stream, so its format is
// uniform: one branch per workgroup into one of three bodies, none per sample -- and every body is the ODD one: an int16 segment may
// start at an odd 2-byte unit (behind an odd number of 8-bit samples of a packed batch).  Reads are the body's: nothing outside a
// strided row's n * bytes(fmt) bytes, at most 2 bytes past a packed source's last sample.  No scratch, no LDS.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

#include "rx_unpack_body.h"

__global__ __launch_bounds__(256) void unpack_mixed_kernel(const uint16_t *src, unsigned *out, size_t out_stride, const UnpackXRow *rows,
                                                           const UnpackXSeg *segs, int nstreams)
{
    const uint32_t b = blockIdx.x;
    const int s = unpack_find_row(rows, nstreams, b);
    const UnpackXRow r = rows[s];
    const UnpackXSeg *sg = segs + r.seg0;
    const uint32_t d0 = (b - r.wg0) * UNPACKX_WG_SAMPLES;
    if (d0 >= r.total) return; // (cannot happen with rx_unpack_plan.h's grid: an empty row has no workgroup)
    const uint32_t d1 = d0 + UNPACKX_WG_SAMPLES < r.total ? d0 + UNPACKX_WG_SAMPLES : r.total;
    unsigned *orow = out + (size_t)s * out_stride;
    // (blockIdx alone decides the row: the format is the same for every lane of the workgroup)
    if (r.fmt == IQF_S16) unpack_body<IQF_S16, true>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
    else if (r.fmt == IQF_U8) unpack_body<IQF_U8, true>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
    else unpack_body<IQF_S8, true>(src, orow, sg, (int)r.nseg, r.total, d0, d1);
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
