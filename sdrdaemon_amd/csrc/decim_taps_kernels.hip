// decim_taps_kernels.hip -- K1t: every rate of a centred cascade in one launch (sdrhip_decimate_taps).  The reference's centred
// cascades nest: decimate4_cen is m_decimator2 -> m_decimator4 (Decimators.cpp:173-213), decimate16_cen runs the same two stages and
// two more (:403-516), decimate64_cen those four and two more (:902-1305); every stage is the same HB64 filter, the stages hand each
// other unshifted int32, and the sample size enters once, in the final `x << norm_shift >> trunk_shift`.  So the output of stage
// k - 1 of a /2^L cascade, shifted by the pair of decimate<2^k>_cen, IS that cascade's output: a tap costs a pack and a store.
//
// The kernel has the shape of K1r (decim_ragged_kernel, rx_ragged_kernels.hip): a 1-D compact grid, workgroup b serves the stream
// whose RaggedRow::seg0 range holds it, the stream's count comes from its row, decim_piece (decim_body.h) runs the segment -- with a
// warm-up for every segment but the first --, the stream's last segment stores the state.  L is the highest tap; which of the stages
// in front of it are stored is the mask of DecimTapArgs, read as a workgroup-uniform value: one scalar branch per stage and ten
// kernels (L = 2..6, packed int16 first stage or not), not one per mask.  Centred modes, plain output rows.
#include "sdrhip_internal.h"

#include "decim_body.h"

namespace sdrhip {
namespace {

template <int L, bool PACK16> __global__ __launch_bounds__(NT) void decim_taps_kernel(DecimArgs a, DecimTapArgs t, const RaggedRow *rows)
{
    __shared__ __attribute__((aligned(16))) int lds[DecimLds<L, 2, PACK16>::dwords];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].seg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int s = lo, seg = b - rows[s].seg0;
    const size_t n_used = (size_t)rows[s].n_used;
    // the last stage is tap L: its row and shift pair from the tap's slot
    a.out = t.out[L]; a.out_stride = t.stride[L];
    a.norm = t.norm[L]; a.trunk = t.trunk[L];
    a.frame_mode = 0; // (plain rows only: a constant here, so none of decim_piece's framing code is compiled into these kernels)
    const size_t seg_raw = (size_t)a.nsub_per_seg * P0;
    const int nseg = n_used ? (int)((n_used + seg_raw - 1) / seg_raw) : 1;
    const size_t seg_start = (size_t)seg * seg_raw;
    size_t seg_end = seg_start + seg_raw;
    if (seg_end > n_used) seg_end = n_used;
    StageTaps taps = {t, s, {0, 0, 0, 0, 0, 0}};
    decim_piece<L, 2, PACK16, false, StageTaps>(a, lds, s, seg_start, seg_end, seg == 0, seg == nseg - 1, seg, nseg, &taps);
}

template <int L> hipError_t launch_taps_variant(bool pack16, const DecimArgs &a, const DecimTapArgs &t, const RaggedRow *rows, hipStream_t stream)
{
    if (pack16) hipLaunchKernelGGL((decim_taps_kernel<L, true>), dim3(a.nseg), dim3(NT), 0, stream, a, t, rows);
    else hipLaunchKernelGGL((decim_taps_kernel<L, false>), dim3(a.nseg), dim3(NT), 0, stream, a, t, rows);
    return hipGetLastError();
}

} // namespace

hipError_t launch_decimate_taps(int log2decim, bool pack16, const DecimArgs &a, const DecimTapArgs &t, const RaggedRow *rows, hipStream_t stream)
{
    if (a.frame_mode || a.nseg < 1) return hipErrorInvalidValue;
    switch (log2decim) {
    case 2: return launch_taps_variant<2>(pack16, a, t, rows, stream);
    case 3: return launch_taps_variant<3>(pack16, a, t, rows, stream);
    case 4: return launch_taps_variant<4>(pack16, a, t, rows, stream);
    case 5: return launch_taps_variant<5>(pack16, a, t, rows, stream);
    case 6: return launch_taps_variant<6>(pack16, a, t, rows, stream);
    }
    return hipErrorInvalidValue;
}

} // namespace sdrhip
