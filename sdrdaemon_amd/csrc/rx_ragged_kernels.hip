// rx_ragged_kernels.hip -- the kernels of ragged calls (sdrhip_decimate_ragged, sdrhip_rx_process_ragged): every stream of a bank takes
// its own number of samples in one launch per step.  They are separate instantiations of the uniform kernels' bodies with the
// per-stream counts read from a per-call table (RaggedRow, sdrhip_internal.h); the uniform kernels keep their instructions.
//
//  * K0r: the 8-bit widening pass, stream s widens n_raw[s] samples.
//  * K1r: the VALU cascade (decim_body.h) over a 1-D grid whose workgroups are dealt to the streams by a prefix table: the launch
//    has sum_s max(1, ceil(n_used_s / segment)) workgroups, so its work follows the total count, not streams x the largest.
//  * the filter-less kernel (decimate1, 2 / 4 inf / sup) with per-stream counts.
//  * K2r: UDPSinkFEC::write framing (frame_pack_body.h) with each stream's own window, frame base, meta record and stamp.
// No kernel reads a sample of stream s past its count: the cascade's last pass and the widening pass bound every load by it.
#include "sdrhip_internal.h"

#include "decim_body.h"

namespace sdrhip {
namespace {

#include "frame_pack_body.h"
#include "rx_unpack_body.h"

// K1r: ragged calls.  1-D grid: workgroup b serves stream s with rows[s].seg0 <= b < rows[s + 1].seg0 (binary search over
// the per-call table), segment b - seg0 of that stream; a stream gets max(1, ceil(n_used / segment)) segments, so one with
// nothing to do still has the workgroup that copies its state
template <int L, int FC, bool PACK16> __global__ __launch_bounds__(NT) void decim_ragged_kernel(DecimArgs a, const RaggedRow *rows)
{
    constexpr int PRAW = P0 << (FC == 2 ? 0 : 2);
    __shared__ __attribute__((aligned(16))) int lds[DecimLds<L, FC, PACK16>::dwords];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].seg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int s = lo, seg = b - rows[s].seg0;
    const size_t n_used = (size_t)rows[s].n_used;
    // the stream's own output shift (RaggedRow::shifts; workgroup-uniform like the row's other fields: scalar registers)
    const unsigned sh = rows[s].shifts;
    a.norm = (int)(sh & 0xffu); a.trunk = (int)(sh >> 8);
    const size_t seg_raw = (size_t)a.nsub_per_seg * PRAW;
    const int nseg = n_used ? (int)((n_used + seg_raw - 1) / seg_raw) : 1;
    const size_t seg_start = (size_t)seg * seg_raw;
    size_t seg_end = seg_start + seg_raw;
    if (seg_end > n_used) seg_end = n_used;
    decim_piece<L, FC, PACK16, false>(a, lds, s, seg_start, seg_end, seg == 0, seg == nseg - 1, seg, nseg);
}

template <int L, int FC, bool PACK16> hipError_t launch_ragged_variant(const DecimArgs &a, const RaggedRow *rows, hipStream_t stream)
{
    hipLaunchKernelGGL((decim_ragged_kernel<L, FC, PACK16>), dim3(a.nseg), dim3(NT), 0, stream, a, rows);
    return hipGetLastError();
}

// ragged calls: stream s takes rows[s].n_raw samples and shifts its output by its own pair (RaggedRow::shifts; the two shift
// arguments are kept for the signature and not read)
__global__ void decim_simple_ragged_kernel(int log2decim, int fcpos, const int16_t *in, size_t in_stride, int16_t *out,
                                           size_t out_stride, int, int, const RaggedRow *rows)
{
    const int s = (int)blockIdx.y;
    const unsigned sh = rows[s].shifts;
    decim_simple_row(log2decim, fcpos, in, in_stride, out, out_stride, (size_t)rows[s].n_raw, (int)(sh & 0xffu), (int)(sh >> 8), s);
}

// K2r: the stream's own count, window, frame base and meta record from its row of the per-call table
__global__ __launch_bounds__(256) void frame_pack_ragged_kernel(FrameArgs a, const RaggedRow *rows)
{
    const int s = (int)blockIdx.y;
    const RaggedRow &r = rows[s];
    a.n = a.in ? (size_t)r.n_dec : 0; // (a.in == NULL: no samples, the meta blocks alone -- launch_frame_meta_ragged)
    a.out += r.out_off;
    a.frame_sample_base = r.frame_sample_base;
    a.meta_first = r.meta_first; a.meta_count = r.meta_count; a.meta_frame_count0 = r.frame_count0;
    a.meta_w[3] = r.tv_sec; a.meta_w[4] = r.tv_usec;
    a.meta_idx0 = r.meta_idx0;
    frame_pack_wg<true>(a, s, blockIdx.x, gridDim.x, &r.fc);
}

// K0r: K0's row pass (rx_unpack_body.h), stream s widening its own count
template <int FMT> __global__ __launch_bounds__(256) void iq8_widen_ragged_kernel(const uint8_t *in, size_t in_stride, int16_t *out,
                                                                                   size_t out_stride, const RaggedRow *rows)
{
    const int s = (int)blockIdx.y;
    iq8_widen_row<FMT>(in + (size_t)s * in_stride * 2, reinterpret_cast<unsigned *>(out) + (size_t)s * out_stride, (size_t)rows[s].n_raw);
}

} // namespace

hipError_t launch_decimate_ragged(int log2decim, int fcpos, bool pack16, const DecimArgs &a, const RaggedRow *rows, hipStream_t stream)
{
#define SDRHIP_CEN(L_)                                                                                          \
    case L_:                                                                                                    \
        return pack16 ? launch_ragged_variant<L_, 2, true>(a, rows, stream) : launch_ragged_variant<L_, 2, false>(a, rows, stream);
#define SDRHIP_ROT(L_, FC_)                                                                                     \
    case L_:                                                                                                    \
        return launch_ragged_variant<L_, FC_, false>(a, rows, stream);
    if (fcpos == 2) {
        switch (log2decim) {
            SDRHIP_CEN(1) SDRHIP_CEN(2) SDRHIP_CEN(3) SDRHIP_CEN(4) SDRHIP_CEN(5) SDRHIP_CEN(6)
        }
    } else if (fcpos == 0) {
        switch (log2decim) { SDRHIP_ROT(3, 0) SDRHIP_ROT(4, 0) SDRHIP_ROT(5, 0) SDRHIP_ROT(6, 0) }
    } else {
        switch (log2decim) { SDRHIP_ROT(3, 1) SDRHIP_ROT(4, 1) SDRHIP_ROT(5, 1) SDRHIP_ROT(6, 1) }
    }
#undef SDRHIP_CEN
#undef SDRHIP_ROT
    return hipErrorInvalidValue;
}

hipError_t launch_decimate_simple_ragged(int log2decim, int fcpos, const int16_t *in, size_t in_stride, int16_t *out,
                                         size_t out_stride, size_t n_in, int nstreams, int norm, int trunk, const RaggedRow *rows,
                                         hipStream_t stream)
{
    size_t work = log2decim == 0 ? n_in : (n_in + 3) / 4;
    size_t blocks = (work + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(decim_simple_ragged_kernel, dim3((unsigned)blocks, nstreams), dim3(256), 0, stream, log2decim, fcpos, in,
                       in_stride, out, out_stride, norm, trunk, rows);
    return hipGetLastError();
}

hipError_t launch_frame_pack_ragged(const FrameArgs &a, const RaggedRow *rows, int nstreams, hipStream_t stream)
{
    size_t blocks = (a.n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(frame_pack_ragged_kernel, dim3((unsigned)blocks, nstreams), dim3(256), 0, stream, a, rows);
    return hipGetLastError();
}

hipError_t launch_frame_meta_ragged(const FrameArgs &a0, const RaggedRow *rows, int max_started, int nstreams, hipStream_t stream)
{
    FrameArgs a = a0;
    a.in = nullptr;
    const int blocks = max_started < 1 ? 1 : max_started > 2048 ? 2048 : max_started; // (frame fi of a stream by workgroup fi mod blocks)
    hipLaunchKernelGGL(frame_pack_ragged_kernel, dim3((unsigned)blocks, nstreams), dim3(256), 0, stream, a, rows);
    return hipGetLastError();
}

hipError_t launch_iq8_widen_ragged(int fmt, const uint8_t *in, size_t in_stride, int16_t *out, size_t out_stride, size_t n, int nstreams,
                                   const RaggedRow *rows, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    size_t blocks = ((n >> 3) + 255) / 256;
    const size_t cap = (size_t)2048 / (size_t)(nstreams > 0 ? nstreams : 1) + 1; // (as K0: enough for the chip, then each lane loops)
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks, (unsigned)nstreams);
    if (fmt == IQF_U8) hipLaunchKernelGGL((iq8_widen_ragged_kernel<IQF_U8>), grid, dim3(256), 0, stream, in, in_stride, out, out_stride, rows);
    else if (fmt == IQF_S8) hipLaunchKernelGGL((iq8_widen_ragged_kernel<IQF_S8>), grid, dim3(256), 0, stream, in, in_stride, out, out_stride, rows);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace sdrhip
