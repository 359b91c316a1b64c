// interp_count.h -- the per-stream count of a ragged interpolator launch: what the IV_COUNT variants of interp_variant.h do in front
// of their segment (InterpArgs::count).
#pragma once
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

// Ragged launches (InterpArgs::count): the grid is planned for the largest stream, every (stream, segment) finds its stream's
// own end.  The count is wave-uniform (one stream per workgroup row): a scalar load.  A segment past its stream's last returns at
// once; the last one (segment 0 of a stream without input: it copies state_cur through) writes state_next, as seg == nseg - 1
// does in a uniform launch.  -> false: nothing to do; else `a` holds the stream's n_in and an nseg whose last segment is its own.
__device__ __forceinline__ bool ragged_args(InterpArgs &a, int seg, int stream, size_t seg_len)
{
    const int k = __builtin_amdgcn_readfirstlane(a.count[(size_t)stream * (size_t)a.count_stride]);
    size_t n = (size_t)(unsigned)k * (size_t)(unsigned)a.count_unit;
    if (n > a.n_in) n = a.n_in; // (never beyond what the grid and the buffers were planned for)
    const size_t start = (size_t)seg * seg_len;
    if (seg != 0 && start >= n) return false;
    if (start + seg_len >= n) a.nseg = seg + 1;
    a.n_in = n;
    return true;
}

} // namespace
} // namespace sdrhip
