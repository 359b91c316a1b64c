// rx_follow_bits_kernels.hip -- KFb, the pass in front of KF (the follow-meta pass) in the ragged step of the Rx pipe fed datagrams
// when the sample size follows the incoming meta blocks (sdrhip_rx_set_follow_bits): sdrdaemonrx hands its own source's
// get_sample_bits() to its Downsampler and, decimated, to UDPSink::setSampleBits / setSampleBytes (sdrdaemonrx.cpp:619-623, 639-643);
// the hub's source is the radio head, whose size arrives in byte 9 of the meta block of its frames, which SDRdaemonFECBuffer keeps
// as m_outputMeta (SDRdaemonFECBuffer.cpp:72-85).
//
// One launch per call or batch for the whole bank, one lane per stream: the lane reads the third word of m_outputMeta from the
// collector state the call committed; a size b of 1..16 in its byte 1 gives the stream's row of the per-call table the shift pair of
// (log2decim, b) -- where the filter-less kernel, K1r and K1mr take it -- the third word of its record with sampleBytes / sampleBits
// of the decimated size b' and the row's own bytes 2 and 3, and the CRC of the zero-stamp record with that word -- where K2r, and
// KF behind this launch, take them.  Any other byte (no frame released with its block 0 yet, a sender that says 0 or more than 16)
// leaves the row as the host put it.  The arithmetic is the host's own text (rx_stream_settings.h: followed_size_words).  The
// launch sits behind the table's upload and in front of every kernel that reads a row, on the context's stream: nothing is read back.
#include "sdrhip_internal.h"

#include "rx_stream_settings.h"

namespace sdrhip {
namespace {

constexpr int KFB_LANES = 64; // streams per workgroup: one wave

__global__ __launch_bounds__(KFB_LANES) void rx_follow_bits_kernel(const FecBufState *state, RaggedRow *rows, unsigned log2decim, int nstreams)
{
    const int s = (int)blockIdx.x * KFB_LANES + (int)threadIdx.x;
    if (s >= nstreams) return;
    RaggedRow &r = rows[s];
    FollowedSize f;
    if (!followed_size_words(state[s].out_meta[2], log2decim, r.fc, r.rate, r.w2, &f)) return; // (no incoming size: the host's values stay)
    r.shifts = f.shifts;
    r.w2 = f.w2;
    r.crc0 = f.crc0;
}

} // namespace

hipError_t launch_rx_follow_bits(const FecBufState *state, RaggedRow *rows, int log2decim, int nstreams, hipStream_t stream)
{
    if (!state || !rows || nstreams <= 0 || log2decim < 0 || log2decim > 6) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_follow_bits_kernel, dim3((unsigned)((nstreams + KFB_LANES - 1) / KFB_LANES)), dim3(KFB_LANES), 0, stream, state, rows,
                       (unsigned)log2decim, nstreams);
    return hipGetLastError();
}

} // namespace sdrhip
