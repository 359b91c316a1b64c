// interp_ragged_kernels.hip -- K5c, the kernels of the sample-fed ragged interpolator entry (sdrhip_interpolate_ragged) for gfx950.
//
// The arithmetic is Interpolators::interpolate{2..64}_cen (Interpolators.cpp:23-606) as interp_body.h (K5) and interp_wave.h (K5w)
// have it: the bodies are included and run as they are.  What is new is the grid.  K5r (the IV_COUNT variants of interp_variant.h)
// launches `largest count x streams` workgroups and lets those of the shorter streams return; here the grid is 1-D over a per-call
// table of (stream, segment) entries (interp_ragged_plan.h), sum_s max(1, ceil(n_s / segment)) of them, so that the cost follows
// the samples.  A workgroup (K5) or a wave (K5w) reads its entry and its stream's row with scalar loads -- both are wave-uniform --,
// sets n_in / nseg / the row pointers of its copy of the arguments and runs the body.  The rows carry their own offsets, so the
// launch serves strided rows (device-memory calls) and packed ones (the staging of host-memory calls) alike: in_stride and
// out_stride of the arguments are 0 and the body's `stream * stride` adds nothing.
//
// The kernel templates are this file's own (interp_variant.h is not included: its kernels stay the 74 of interp_kernels.hip and
// the table variants of interp_mixed_kernels.hip).  K5 runs the RAGGED instantiation of its body, whose geometry type is apart from
// the uniform one's (IGeoRagged).  Int16 output only.
#include "interp_body.h"
#include "interp_wave.h"

namespace sdrhip {
namespace {

static_assert(INTERP_MC == MC && INTERP_WB == WB && INTERP_WPAIRS == WPAIRS, "interp_ragged_plan.h plans with the bodies' constants");
static_assert(INTERP_COPY_SEG % 4 == 0, "a copy segment keeps its row's 16-byte alignment");

struct InterpMapArgs {
    const InterpMapRow *rows;
    const InterpMapEntry *entries;
    unsigned nentries;
};

__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// entry `idx` (wave-uniform, below m.nentries) -> the stream and the segment; the stream's row -> n_in, nseg and the row pointers
// of `a` (whose strides the host left 0)
__device__ __forceinline__ void mapped_args(InterpArgs &a, const InterpMapArgs &m, unsigned idx, int &stream, int &seg)
{
    const InterpMapEntry e = m.entries[idx];
    stream = __builtin_amdgcn_readfirstlane((int)e.stream);
    seg = __builtin_amdgcn_readfirstlane((int)e.seg);
    const InterpMapRow r = m.rows[stream];
    a.n_in = (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)r.n_in);
    a.nseg = __builtin_amdgcn_readfirstlane(r.nseg);
    a.in += 2 * uniform64(r.in_off);
    a.out += 2 * uniform64(r.out_off);
}

// K5 mapped: one workgroup per entry
template <int L> __global__ __launch_bounds__(NT) void interp_mapped_kernel(InterpArgs a, InterpMapArgs m)
{
    __shared__ __attribute__((aligned(16))) int lds[IGeo<(L == 6) ? 5 : L>::ldsDw];
    int stream, seg;
    mapped_args(a, m, blockIdx.x, stream, seg);
    interp_segment<L, true, IQF_S16>(a, seg, stream, lds);
}

// K5w mapped: wave w of a workgroup takes entry blockIdx.x * WPW + w.  The waves of a workgroup may belong to different streams;
// they share nothing (no barrier, an LDS slice each), as in interp_wave_kernel
template <int L, int WPW> __global__ __launch_bounds__(WNT * WPW) void interp_wave_mapped_kernel(InterpArgs a, InterpMapArgs m)
{
    __shared__ __attribute__((aligned(16))) int lds[WPW][WGeo<(L == 6) ? 5 : L>::ldsDw];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned idx = blockIdx.x * (unsigned)WPW + (unsigned)w;
    if (idx >= m.nentries) return;
    int stream, seg;
    mapped_args(a, m, idx, stream, seg);
    interp_wave_segment<L, false, IQF_S16>(a, seg, stream, lds[w]);
}

// x1 (Upsampler::process m_interp == 0: samples_out = samples_in, Upsampler.cpp:54-57) over the same table: entry (s, g) moves the
// samples [g * seg_len, min((g + 1) * seg_len, n_in[s])) of row s, 16 bytes per lane where both rows allow it, else sample by sample
__global__ __launch_bounds__(NT) void interp1_mapped_kernel(const unsigned *in, unsigned *out, InterpMapArgs m, unsigned seg_len)
{
    const InterpMapEntry e = m.entries[blockIdx.x];
    const int stream = __builtin_amdgcn_readfirstlane((int)e.stream);
    const InterpMapRow r = m.rows[stream];
    const size_t n = (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)r.n_in);
    const size_t start = (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)e.seg) * seg_len;
    if (start >= n) return;
    const size_t len = n - start < (size_t)seg_len ? n - start : (size_t)seg_len;
    const unsigned *src = in + uniform64(r.in_off) + start;
    unsigned *dst = out + uniform64(r.out_off) + start;
    size_t done = 0;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        const size_t n4 = len / 4;
        for (size_t i = threadIdx.x; i < n4; i += NT)
            reinterpret_cast<uint4_t *>(dst)[i] = SDRHIP_STREAM_LOAD(reinterpret_cast<const uint4_t *>(src) + i);
        done = n4 * 4;
    }
    for (size_t i = done + threadIdx.x; i < len; i += NT) dst[i] = SDRHIP_STREAM_LOAD(src + i);
}

template <int L> hipError_t launch_valu_mapped(const InterpArgs &a, const InterpMapArgs &m, hipStream_t stream)
{
    hipLaunchKernelGGL((interp_mapped_kernel<L>), dim3(m.nentries), dim3(NT), 0, stream, a, m);
    return hipGetLastError();
}

template <int L, int WPW = 4> hipError_t launch_wave_mapped(int wpw, const InterpArgs &a, const InterpMapArgs &m, hipStream_t stream)
{
    if (WPW != 1 && wpw == 1) return launch_wave_mapped<L, 1>(1, a, m, stream);
    hipLaunchKernelGGL((interp_wave_mapped_kernel<L, WPW>), dim3((m.nentries + WPW - 1) / WPW), dim3(WNT * WPW), 0, stream, a, m);
    return hipGetLastError();
}

} // namespace

hipError_t launch_interp_mapped(const InterpPick &pick, int log2interp, const InterpArgs &a, const InterpMapRow *rows, const InterpMapEntry *entries,
                                unsigned nentries, hipStream_t stream)
{
    if (pick.variant != (log2interp ? IV_MAPPED : 0u) || !rows || !entries || nentries == 0 || nentries > INTERP_RAGGED_MAX_ENTRIES) return hipErrorInvalidValue;
    if (a.in_stride || a.out_stride || a.count || a.gmap) return hipErrorInvalidValue; // (the rows carry their own offsets)
    const InterpMapArgs m = {rows, entries, nentries};
    if (pick.route == IR_COPY && log2interp == 0) {
        hipLaunchKernelGGL(interp1_mapped_kernel, dim3(nentries), dim3(NT), 0, stream, reinterpret_cast<const unsigned *>(a.in),
                           reinterpret_cast<unsigned *>(a.out), m, (unsigned)INTERP_COPY_SEG);
        return hipGetLastError();
    }
    if (pick.route == IR_WAVE) {
        switch (log2interp) {
        case 2: return launch_wave_mapped<2>(pick.wpw, a, m, stream);
        case 3: return launch_wave_mapped<3>(pick.wpw, a, m, stream);
        case 4: return launch_wave_mapped<4>(pick.wpw, a, m, stream);
        case 5: return launch_wave_mapped<5>(pick.wpw, a, m, stream);
        case 6: return launch_wave_mapped<6>(pick.wpw, a, m, stream);
        }
    } else if (pick.route == IR_VALU) {
        switch (log2interp) {
        case 1: return launch_valu_mapped<1>(a, m, stream);
        case 2: return launch_valu_mapped<2>(a, m, stream);
        case 3: return launch_valu_mapped<3>(a, m, stream);
        case 4: return launch_valu_mapped<4>(a, m, stream);
        case 5: return launch_valu_mapped<5>(a, m, stream);
        case 6: return launch_valu_mapped<6>(a, m, stream);
        }
    }
    return hipErrorInvalidValue;
}

} // namespace sdrhip
