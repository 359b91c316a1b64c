// rx_join_kernels.hip -- the join of the Rx pipe fed datagrams (sdrhip_rx_process_datagrams): collector -> decimator on the device.
//
// The handle owns rows [stream][row_len] of int16 IQ samples (16-byte aligned starts, row_len a multiple of 4), the ragged
// decimator's input.  Row s begins with the carry[s] samples the stream held back from earlier calls; the collector's delivery
// passes -- fecbuf_passes.h instantiated once more, with a per-stream output offset -- put the payloads the call releases right
// behind them.  The decimator takes the largest multiple of U (the decimation unit) from the row's head, and KJ, below, moves what
// is left (fewer than U <= 64 samples) to the row's head and writes the new carry[s]: one launch for the whole bank, no copies or
// launches per stream.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

#define FB_PACKED 0
#define FB_ROWS 1
#include "fecbuf_passes.h"
#undef FB_PACKED

constexpr int KJ_WAVES = 4; // streams per workgroup: one wave each

// KJ: stream s holds carry[s] + 16129 K_s samples at its row's head (K_s = counts[s][FB_K], the frames the collector released);
// the decimator has read `used`, the largest multiple of `unit` among them.  Lane i moves sample used + i to sample i -- the two
// ranges cannot overlap: the remainder is shorter than `unit`, and `used` is at least `unit` whenever something moves.
__global__ __launch_bounds__(64 * KJ_WAVES) void rx_join_carry_kernel(unsigned *rows, size_t row_len, unsigned *carry, const int *counts,
                                                                     unsigned unit, int nstreams)
{
    const int s = (int)blockIdx.x * KJ_WAVES + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    if (s >= nstreams) return;
    const size_t total = (size_t)carry[s] + (size_t)counts[(size_t)s * FB_COUNTS + FB_K] * 16129u;
    if (total > row_len) return; // (the host sized the rows for the call's max_released: never taken)
    const size_t used = total / unit * unit;
    const unsigned rem = (unsigned)(total - used);
    unsigned *row = rows + (size_t)s * row_len;
    if (used != 0 && (unsigned)lane < rem) row[lane] = row[used + (size_t)lane];
    if (lane == 0) carry[s] = rem;
}

} // namespace

hipError_t launch_fecbuf_scatter_rows(const FecBufArgs &a, const unsigned *row_off, int njobs, hipStream_t stream)
{
    if (njobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_scatter_rows_kernel, dim3(njobs), dim3(SC_NT), 0, stream, a, row_off);
    return hipGetLastError();
}

hipError_t launch_fecbuf_copy_rows(const FecBufArgs &a, const unsigned *row_off, int nslots, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fecbuf_copy_rows_kernel, dim3(nslots), dim3(SC_NT), 0, stream, a, row_off);
    return hipGetLastError();
}

hipError_t launch_rx_join_carry(int16_t *rows, size_t row_len, unsigned *carry, const int *counts, unsigned unit, int nstreams,
                                hipStream_t stream)
{
    if (nstreams <= 0 || unit == 0 || unit > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_join_carry_kernel, dim3((nstreams + KJ_WAVES - 1) / KJ_WAVES), dim3(64 * KJ_WAVES), 0, stream,
                       reinterpret_cast<unsigned *>(rows), row_len, carry, counts, unit, nstreams);
    return hipGetLastError();
}

} // namespace sdrhip
