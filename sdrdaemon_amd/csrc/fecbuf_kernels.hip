// fecbuf_kernels.hip -- a bank of SDRdaemonFECBuffer collectors (SDRdaemonFECBuffer.cpp:112-250) fed raw datagrams.
//
// A call hands in n_s datagrams of 512 bytes per stream, in arrival order.  Three passes (sdrhip_fecbuf.cpp drives them):
//   classify  one workgroup per stream reads the 4-byte headers only.  A datagram whose frameIndex differs from the one before
//             it (datagram 0: from the open slot carried over from the last call) starts a frame and releases the one before;
//             a workgroup-wide scan numbers the frames (ordinal 0 = the carried open slot) and gives each datagram its rank in
//             its frame.  Per frame: block count, recovery blocks / highest recovery row / originals present among the first 128
//             (LDS atomics keyed by the frame's ordinal within the chunk), whether it goes to the decoder (>= 128 blocks,
//             recovery blocks, no repeated original: the frames cm256_decode repairs), the stream's statistics.
//   scatter   one workgroup per released frame and per open slot.  Frames that need no decoder are written straight to the
//             output (originals in place, the LAST of repeated arrivals wins as in m_frame, holes zero); frames that do are
//             staged as 128 arrival-order super blocks for launch_fec_decode_device_plan; the open slot's new arrivals go to
//             the stream's carry buffer.
//   copy      the decoder's output of each staged frame to its place in the output.
// The passes themselves are in fecbuf_passes.h: tx_async_kernels.hip instantiates them once more for the asynchronous Tx batches
// (sdrhip_tx_submit_datagrams: a stream's datagrams back to back at a per-stream offset, grids sized by the host's shadow of the
// classification).
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

#define FB_PACKED 0
#include "fecbuf_passes.h"
#undef FB_PACKED

} // namespace

hipError_t launch_fecbuf_classify(const FecBufArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(fecbuf_classify_kernel, dim3(a.nstreams), dim3(CL_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fecbuf_scatter(const FecBufArgs &a, int njobs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_scatter_kernel, dim3(njobs), dim3(SC_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_fecbuf_copy(const FecBufArgs &a, int nslots, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_copy_kernel, dim3(nslots), dim3(SC_NT), 0, stream, a);
    return hipGetLastError();
}

} // namespace sdrhip
