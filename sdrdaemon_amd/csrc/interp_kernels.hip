// interp_kernels.hip -- cascaded integer half-band interpolators for gfx950 (MI355X).
//
// Replaces Interpolators::interpolate{2..64}_cen (Interpolators.cpp:23-606) over
// IntHalfbandFilterEO1/DB<64|32|16>::myInterpolate (IntHalfbandFilterEO1.h:44-65,149-168;
// DB twin IntHalfbandFilterDB.h:51-72,109-128 -- identical arithmetic):
//     v[2m]   = u[m - O/4]
//     v[2m+1] = (sum_{i < O/4} c[i] * (u[m - (O/2 - 1) + i] + u[m - i])) >> 13
// stage orders 64, 32, 16, 16, 16 (Interpolators.h:31-33); int32 between stages, int16
// truncation at the end.  interpolate64_cen is reproduced as the reference has it: five
// stages and 32 zero samples after every 32 outputs (Interpolators.cpp:363-606).
//
// Design (DESIGN.md "K5"), the mirror image of the decimator kernel:
//  * grid = (segments, streams); a 256-thread workgroup walks its segment in macro-cycles of
//    512 inputs.  The inputs of every stage sit in LDS (I and Q planes, int32, plane stride
//    8 mod 16 slots) behind 32 entries of history.
//  * the cascade is an expanding tree, walked depth first: one invocation of stage s
//    (512 inputs) feeds two invocations of stage s+1, so every invocation keeps all 256
//    threads busy: lanes 2j / 2j+1 compute the 8 outputs of 4 consecutive inputs of I / Q;
//    the last stage takes 1024 inputs per invocation and handles both components per thread
//    so that it can pack int16 I/Q and store 2 x 16 bytes per thread without a lane exchange.
//  * segment 0 takes the histories from the bank state, other segments rebuild them from the
//    64 preceding inputs (the cascade's memory is 43 inputs) with stores suppressed.
//
// The kernels and their launchers are interp_variant.h's; this unit instantiates the plain ones and the bank-wide variants (gathered
// input, per-stream counts, 8-bit output, 8-bit output with counts), plans the grids and holds the bank's one launch entry.
#include "interp_variant.h"

namespace sdrhip {

// the segments of a uniform call: interp_ragged_plan.h holds the rules (the ragged entry plans with the same ones)
void plan_interpolate(int log2interp, size_t n_in, int nstreams, int *nsub_per_seg, int *nseg)
{
    static_assert(INTERP_MC == MC, "interp_ragged_plan.h plans with the body's macro-cycle");
    interp_plan_valu(log2interp, n_in, nstreams, nsub_per_seg, nseg);
}

void plan_interpolate_wave(int log2interp, size_t n_in, int nstreams, int n_cu, size_t seg_override, int *nsub_per_seg, int *nseg)
{
    static_assert(INTERP_WB == WB && INTERP_WPAIRS == WPAIRS, "interp_ragged_plan.h plans with K5w's block and pair count");
    (void)log2interp; (void)nstreams; (void)n_cu;
    interp_plan_wave(n_in, seg_override, nsub_per_seg, nseg);
}

// the bank-wide variants live here, the table variants behind launch_interpolate_table
hipError_t launch_interpolate(const InterpPick &pick, int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    switch (pick.variant) {
    case 0: return launch_variant<0>(pick, log2interp, a, fmt, stream);
    case IV_GATHER: return launch_variant<IV_GATHER>(pick, log2interp, a, fmt, stream);
    case IV_COUNT: return launch_variant<IV_COUNT>(pick, log2interp, a, fmt, stream);
    case IV_S8: return launch_variant<IV_S8>(pick, log2interp, a, fmt, stream);
    case IV_S8 | IV_COUNT: return launch_variant<IV_S8 | IV_COUNT>(pick, log2interp, a, fmt, stream);
    case IV_TABLE:
    case IV_TABLE | IV_COUNT: return launch_interpolate_table(pick, log2interp, a, fmt, stream);
    }
    return hipErrorInvalidValue;
}

} // namespace sdrhip
