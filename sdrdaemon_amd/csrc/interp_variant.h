// interp_variant.h -- the kernels of the interpolator bank and their launchers, shared by interp_kernels.hip (the bank-wide variants)
// and interp_mixed_kernels.hip (the IV_TABLE variants, K5x).  Four kernel templates: the plain K5 / K5w, interp_kernel<L> and
// interp_wave_kernel<L, WPW>, and one variant template for each, interp_variant_kernel<L, V> and interp_wave_variant_kernel<L, WPW, V>,
// where V is an OR of the IV_* flags of interp_pick.h: what a variant does beside the plain kernel is selected at compile time, the
// bodies (interp_body.h, interp_wave.h) are the plain kernel's.  Every variant takes the format table as a second argument (read with
// IV_TABLE alone); InterpArgs is the same for all.
//
// IV_TABLE (K5x): in the reference the format belongs to the sink object, one per process and so per stream: HackRFSink.cpp:671-672
// sends real() >> 8, imag() >> 8, FileSink.cpp:216-277 writes int16 IQ.  Here the stream is blockIdx.y, so the format is uniform over a
// workgroup: one int per stream (`fmt`, IQF_S16 | IQF_S8) is read with a scalar load and the kernel branches to the int16 or the 8-bit
// body.  out_stride then counts 4-byte units and row s starts at byte 4 * s * out_stride whatever its format.  The 8-bit bodies
// address 2-byte samples, so their branch hands them a copy of the arguments with out_stride doubled: both land on the same byte.
// An 8-bit row is written in its first 2 * n bytes alone.
#pragma once
#include "interp_body.h"
#include "interp_count.h"
#include "interp_wave.h"

namespace sdrhip {
namespace {

static_assert(INTERP_S16 == IQF_S16 && INTERP_S8 == IQF_S8, "interp_pick.h names the formats of sdrhip_internal.h");

__device__ __forceinline__ int stream_fmt(const int *fmt) { return __builtin_amdgcn_readfirstlane(fmt[blockIdx.y]); }
// the stream index as a value of the branch's own: what either body derives from it is computed inside that body, not once in front
// of the branch and kept in registers through both (K5w x4 allocated 104 registers per lane with it shared, 96 like its twins without)
__device__ __forceinline__ int own_stream()
{
    int s = (int)blockIdx.y;
    asm volatile("" : "+s"(s));
    return s;
}
// ... and an end of its own for either branch: a comment in the assembly, no instruction.  The two bodies end alike (the last segment
// stores the histories), and with one shared tail the values live into it hold the same registers through both branches: K5 x64
// allocated 74 registers per lane with the tail shared (its twins 68 and 70), 70 with the ends told apart
#define END_OF_BRANCH(which) asm volatile("; K5x " which " row done")

// K5.  L = log2 interpolation (6 = the reference's 5-stage + zero stuffing variant)
template <int L> __global__ __launch_bounds__(NT) void interp_kernel(InterpArgs a)
{
    __shared__ __attribute__((aligned(16))) int lds[IGeo<(L == 6) ? 5 : L>::ldsDw];
    interp_segment<L>(a, blockIdx.x, blockIdx.y, lds);
}

// IV_COUNT: ragged_args of interp_count.h finds each (stream, segment)'s own end; the body is instantiated apart (RAGGED).  The
// table variant without counts runs the plain instantiation of either body
template <int L, unsigned V> __global__ __launch_bounds__(NT) void interp_variant_kernel(InterpArgs a, const int *fmt)
{
    static_assert(V != 0 && !(V & IV_GATHER) && (V & (IV_S8 | IV_TABLE)) != (IV_S8 | IV_TABLE), "no such variant of K5");
    constexpr bool COUNT = (V & IV_COUNT) != 0;
    __shared__ __attribute__((aligned(16))) int lds[IGeo<(L == 6) ? 5 : L>::ldsDw];
    if constexpr (COUNT)
        if (!ragged_args(a, (int)blockIdx.x, (int)blockIdx.y, (size_t)a.nsub_per_seg * IGeo<(L == 6) ? 5 : L>::mc)) return;
    if constexpr (V & IV_TABLE) {
        if (stream_fmt(fmt) == IQF_S8) {
            a.out_stride *= 2;
            interp_segment<L, COUNT, IQF_S8>(a, blockIdx.x, own_stream(), lds);
            END_OF_BRANCH("s8");
        } else {
            interp_segment<L, COUNT, IQF_S16>(a, blockIdx.x, own_stream(), lds);
            END_OF_BRANCH("s16");
        }
    } else
        interp_segment<L, COUNT, (V & IV_S8) ? IQF_S8 : IQF_S16>(a, blockIdx.x, blockIdx.y, lds);
}

// K5w: one time slice of one stream per wave, no barrier (interp_wave.h).
// WPW waves per workgroup, each on a segment of its own (no barrier, no shared data: a workgroup is only a way of starting WPW
// waves at the same moment, which puts their clusters of input loads at the same moment -- see interp_wave_segment; measured
// 6 % on interpolate32, 0..1 % on the others, tools/experiments_r04 batch 20).  Launches too small to fill the chip with
// workgroups of four keep one wave per workgroup.
template <int L, int WPW> __global__ __launch_bounds__(WNT * WPW) void interp_wave_kernel(InterpArgs a)
{
    __shared__ __attribute__((aligned(16))) int lds[WPW][WGeo<(L == 6) ? 5 : L>::ldsDw];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int seg = (int)blockIdx.x * WPW + w;
    if (seg >= a.nseg) return;
    interp_wave_segment<L>(a, seg, blockIdx.y, lds[w]);
}

// IV_GATHER: the input through the Tx decoder's position map (InterpArgs::gmap)
template <int L, int WPW, unsigned V> __global__ __launch_bounds__(WNT * WPW) void interp_wave_variant_kernel(InterpArgs a, const int *fmt)
{
    static_assert(V != 0 && (!(V & IV_GATHER) || V == IV_GATHER) && (V & (IV_S8 | IV_TABLE)) != (IV_S8 | IV_TABLE), "no such variant of K5w");
    __shared__ __attribute__((aligned(16))) int lds[WPW][WGeo<(L == 6) ? 5 : L>::ldsDw];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int seg = (int)blockIdx.x * WPW + w;
    if (seg >= a.nseg) return;
    if constexpr (V & IV_COUNT)
        if (!ragged_args(a, seg, (int)blockIdx.y, (size_t)a.nsub_per_seg * WB)) return;
    if constexpr (V & IV_TABLE) {
        if (stream_fmt(fmt) == IQF_S8) {
            a.out_stride *= 2;
            interp_wave_segment<L, false, IQF_S8>(a, seg, own_stream(), lds[w]);
            END_OF_BRANCH("s8");
        } else {
            interp_wave_segment<L, false, IQF_S16>(a, seg, own_stream(), lds[w]);
            END_OF_BRANCH("s16");
        }
    } else
        interp_wave_segment<L, (V & IV_GATHER) != 0, (V & IV_S8) ? IQF_S8 : IQF_S16>(a, seg, blockIdx.y, lds[w]);
}

// One launcher per path; variant 0 is the plain kernel.  K5: grid = (segments, streams)
template <int L, unsigned V> hipError_t launch_valu(const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    const dim3 grid(a.nseg, a.nstreams);
    if constexpr (V == 0) hipLaunchKernelGGL((interp_kernel<L>), grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((interp_variant_kernel<L, V>), grid, dim3(NT), 0, stream, a, fmt);
    return hipGetLastError();
}

// K5w: grid = (workgroups of wpw segments, streams), wpw as interp_pick_wpw decided it on the planned -- largest -- grid
template <int L, unsigned V, int WPW = 4> hipError_t launch_wave(int wpw, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    if (WPW != 1 && wpw == 1) return launch_wave<L, V, 1>(1, a, fmt, stream);
    const dim3 grid((a.nseg + WPW - 1) / WPW, a.nstreams);
    if constexpr (V == 0) hipLaunchKernelGGL((interp_wave_kernel<L, WPW>), grid, dim3(WNT * WPW), 0, stream, a);
    else hipLaunchKernelGGL((interp_wave_variant_kernel<L, WPW, V>), grid, dim3(WNT * WPW), 0, stream, a, fmt);
    return hipGetLastError();
}

// ... and the ratio: the kernels of variant V that exist are the ones named here
template <unsigned V> hipError_t launch_variant(const InterpPick &pick, int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    if ((V & IV_TABLE) && !fmt) return hipErrorInvalidValue;
    if (((V & IV_COUNT) != 0) != (a.count != nullptr) || ((V & IV_GATHER) != 0) != (a.gmap != nullptr)) return hipErrorInvalidValue;
    if (pick.route == IR_WAVE) {
        switch (log2interp) {
        case 2: return launch_wave<2, V>(pick.wpw, a, fmt, stream);
        case 3: return launch_wave<3, V>(pick.wpw, a, fmt, stream);
        case 4: return launch_wave<4, V>(pick.wpw, a, fmt, stream);
        case 5: return launch_wave<5, V>(pick.wpw, a, fmt, stream);
        case 6: return launch_wave<6, V>(pick.wpw, a, fmt, stream);
        }
    } else if constexpr (!(V & IV_GATHER)) { // (K5 has no gathered input)
        if (pick.route != IR_VALU) return hipErrorInvalidValue;
        switch (log2interp) {
        case 1: return launch_valu<1, V>(a, fmt, stream);
        case 2: return launch_valu<2, V>(a, fmt, stream);
        case 3: return launch_valu<3, V>(a, fmt, stream);
        case 4: return launch_valu<4, V>(a, fmt, stream);
        case 5: return launch_valu<5, V>(a, fmt, stream);
        case 6: return launch_valu<6, V>(a, fmt, stream);
        }
    }
    return hipErrorInvalidValue;
}

} // namespace
} // namespace sdrhip
