// rx_follow_kernels.hip -- KF, the pass between the collector and the ragged step of the Rx pipe fed datagrams when the outgoing
// meta blocks follow the incoming ones (sdrhip_rx_set_follow_meta): sdrdaemonrx's loop takes the centre frequency and the sample
// rate it announces from its own source (sdrdaemonrx.cpp:622-631,644); the hub's source is the radio head's meta block, which
// SDRdaemonFECBuffer keeps as m_outputMeta (SDRdaemonFECBuffer.cpp:72-85).
//
// One launch per call or batch for the whole bank, one lane per stream: the lane reads m_outputMeta's frequency and rate from the
// collector state the call committed, forms the zero-stamp MetaDataFEC record the stream's next frames carry -- frequency unchanged,
// rate >> log2decim, the third word the host put into the stream's row (its own nbFECBlocks) -- with its CRC, and writes {fc, rate, crc0} into the stream's row of the per-call
// table, where K2r takes them (stream_meta_base<true>).  A stream whose incoming rate is 0 (none of its frames released with a
// block 0 yet, or a sender that says 0) keeps what the host put there.  The launch sits behind the table's upload and in front of
// the first kernel that reads a row's three words, on the context's stream: nothing is read back.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

constexpr int KF_LANES = 64; // streams per workgroup: one wave

// boost::crc_32_type over the little-endian bytes of `w`, 32 bit steps (UDPSinkFEC.cpp:106-109; the host's restatement:
// rx_meta_record)
__device__ __forceinline__ unsigned kf_crc_word(unsigned crc, unsigned w)
{
    crc ^= w;
#pragma unroll
    for (int k = 0; k < 32; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    return crc;
}

__global__ __launch_bounds__(KF_LANES) void rx_follow_meta_kernel(const FecBufState *state, RaggedRow *rows, unsigned log2decim, int nstreams)
{
    const int s = (int)blockIdx.x * KF_LANES + (int)threadIdx.x;
    if (s >= nstreams) return;
    const unsigned fc = state[s].out_meta[0], in_rate = state[s].out_meta[1];
    if (in_rate == 0) return; // (no incoming meta: the host's values stay)
    const unsigned rate = in_rate >> log2decim;
    unsigned crc = 0xFFFFFFFFu;
    crc = kf_crc_word(crc, fc);
    crc = kf_crc_word(crc, rate);
    RaggedRow &r = rows[s];
    crc = kf_crc_word(crc, r.w2);
    crc = kf_crc_word(crc, 0u); // tv_sec
    crc = kf_crc_word(crc, 0u); // tv_usec
    r.fc = fc;
    r.rate = rate;
    r.crc0 = crc ^ 0xFFFFFFFFu;
}

} // namespace

hipError_t launch_rx_follow_meta(const FecBufState *state, RaggedRow *rows, int log2decim, int nstreams, hipStream_t stream)
{
    if (!state || !rows || nstreams <= 0 || log2decim < 0 || log2decim > 31) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_follow_meta_kernel, dim3((unsigned)((nstreams + KF_LANES - 1) / KF_LANES)), dim3(KF_LANES), 0, stream, state, rows,
                       (unsigned)log2decim, nstreams);
    return hipGetLastError();
}

} // namespace sdrhip
