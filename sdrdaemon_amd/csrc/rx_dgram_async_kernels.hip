// rx_dgram_async_kernels.hip -- the kernels of asynchronous datagram-fed Rx batches (sdrhip_rx_submit_datagrams /
// sdrhip_rx_collect_datagrams): the collector's delivery passes (fecbuf_passes.h) instantiated a fourth time, packed datagrams in
// (stream s's datagrams back to back at a per-stream offset, as the asynchronous Tx batches upload them) and payloads out behind a
// per-stream row offset (the samples the stream's row holds back, as the Rx pipe fed datagrams keeps them).  The grids are the
// host's shadow of the classification: both passes carry the packed guards (a job past the classify pass's own count, a frame at or
// past max_frames, a staging slot at or past nslots, a slot whose dmap entry is still -1) and skip a frame whose payload would end
// past the stream's row, so that counts that disagree with the shadow never write outside the rows.
// The classify pass and the shadow check of a batch are tx_async_kernels.hip's, the remainder kernel KJ is rx_join_kernels.hip's.
//
// The delivery, KD: the frames every stream completed (its sliding window in the frame area) and the records of the frames its
// collector released -> one contiguous buffer, frames first in stream order, then the records, so that ONE download carries
// exactly the delivered bytes.  Every piece starts on a 16-byte boundary on both sides and is a multiple of 16 bytes long (a frame
// is (128 + nb_fec) x 512 bytes, a record 16), so there are no heads or tails: a segment gets ceil(bytes / 16 KiB) workgroups
// (found by binary search, as the Tx delivery gather finds its segment), every lane moves whole 16-byte chunks, four loads in
// flight before their stores.  The table comes from the host's own counts alone.
// No kernel here uses scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

#define FB_PACKED 1
#define FB_ROWS 1
#include "fecbuf_passes.h"
#undef FB_PACKED

constexpr int KD_NT = 256;
constexpr int KD_PER_LANE = 4; // 16-byte chunks per lane and workgroup (RX_DELIVER_WG_BYTES = 16 * KD_NT * KD_PER_LANE)
static_assert(RX_DELIVER_WG_BYTES == 16u * KD_NT * KD_PER_LANE, "workgroup share");

__global__ __launch_bounds__(KD_NT) void rx_deliver_kernel(const RxDeliverSeg *segs, int nseg, const uint8_t *frames, const uint8_t *records,
                                                           uint8_t *out)
{
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = nseg - 1; // the last segment whose first workgroup is at or before b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].wg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const RxDeliverSeg g = segs[lo];
    // (32-bit chunk positions: rx_deliver_plan refuses a segment of 2^32 chunks or more)
    const uint32_t n = (uint32_t)(g.bytes / 16), c0 = (b - g.wg0) * (uint32_t)(RX_DELIVER_WG_BYTES / 16) + threadIdx.x;
    const uint4_t *src = reinterpret_cast<const uint4_t *>((g.from_records ? records : frames) + g.src) + c0;
    uint4_t *dst = reinterpret_cast<uint4_t *>(out + g.dst) + c0;
    uint4_t v[KD_PER_LANE];
#pragma unroll
    for (int j = 0; j < KD_PER_LANE; ++j)
        if (c0 + (uint32_t)j * KD_NT < n) v[j] = __builtin_nontemporal_load(src + j * KD_NT);
#pragma unroll
    for (int j = 0; j < KD_PER_LANE; ++j)
        if (c0 + (uint32_t)j * KD_NT < n) dst[j * KD_NT] = v[j];
}

} // namespace

uint32_t rx_deliver_plan(RxDeliverSeg *segs, int nseg)
{
    uint64_t wg = 0;
    for (int i = 0; i < nseg; ++i) {
        segs[i].wg0 = (uint32_t)wg;
        wg += (segs[i].bytes + RX_DELIVER_WG_BYTES - 1) / RX_DELIVER_WG_BYTES;
        if ((segs[i].bytes | segs[i].src | segs[i].dst) & 15u || !segs[i].bytes || segs[i].bytes >> 35 || wg > 0x7fffffffu) return 0;
    }
    return (uint32_t)wg;
}

hipError_t launch_rx_deliver(const RxDeliverSeg *segs, int nseg, uint32_t grid, const uint8_t *frames, const uint8_t *records, uint8_t *out,
                             hipStream_t stream)
{
    if (nseg <= 0 || grid == 0) return hipSuccess;
    hipLaunchKernelGGL(rx_deliver_kernel, dim3(grid), dim3(KD_NT), 0, stream, segs, nseg, frames, records, out);
    return hipGetLastError();
}

hipError_t launch_fecbuf_scatter_packed_rows(const FecBufArgs &a, const long long *dg_off, const unsigned *row_off, int njobs, int nslots,
                                             hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_scatter_packed_rows_kernel, dim3(njobs), dim3(SC_NT), 0, stream, a, dg_off, nslots, row_off);
    return hipGetLastError();
}

hipError_t launch_fecbuf_copy_guarded_rows(const FecBufArgs &a, const unsigned *row_off, int nslots, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_copy_guarded_rows_kernel, dim3(nslots), dim3(SC_NT), 0, stream, a, row_off);
    return hipGetLastError();
}

} // namespace sdrhip
