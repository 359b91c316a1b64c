// interp_mixed_kernels.hip -- K5x / K6x: the Tx bank's last stage with the output format per stream (sdrhip_tx_set_stream_format).
//
// In the reference the format belongs to the sink object, one per process and so per stream: HackRFSink.cpp:671-672 sends
// real() >> 8, imag() >> 8, FileSink.cpp:216-277 writes int16 IQ.  Here the stream is blockIdx.y, so the format is uniform over a
// workgroup: one int per stream (`fmt`, IQF_S16 | IQF_S8) is read with a scalar load and the kernel branches to the int16 or the
// 8-bit body of interp_wave.h / interp_body.h, which stay as they are.
//
// Addressing: out_stride counts 4-byte units and row s starts at byte 4 * s * out_stride whatever its format.  The 8-bit bodies
// address 2-byte samples, so their branch hands them a copy of the arguments with out_stride doubled: both land on the same byte.
// An 8-bit row is written in its first 2 * n bytes alone.
//
// K5x: interp_wave_mixed_kernel<L, WPW> (x4 .. x64) and interp_mixed_kernel<L> (x2, and interp_path = valu), each with a count
// variant (InterpArgs::count, interp_count.h); grids and workgroup shapes are those of the bank-wide launches (interp_kernels.hip).
// InterpArgs is unchanged: the table is a second kernel argument.
// K6x: x1 (Upsampler.cpp:54-57, samples_out = samples_in) over (chunks, streams): an int16 row is copied, 16 bytes per lane and step,
// an 8-bit row is narrowed to byte 1 of every component (the rule of K6n, convert_kernels.hip), up to the stream's own count where a
// count table is given.  Rows are 16-byte aligned on both sides; a row's last samples go one by one, nothing past them is touched.
// No kernel here uses scratch.
#include "interp_body.h"
#include "interp_count.h"
#include "interp_wave.h"

namespace sdrhip {
namespace {

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

template <int L, int WPW> __global__ __launch_bounds__(WNT * WPW) void interp_wave_mixed_kernel(InterpArgs a, const int *fmt)
{
    __shared__ __attribute__((aligned(16))) int lds[WPW][WGeo<(L == 6) ? 5 : L>::ldsDw];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int seg = (int)blockIdx.x * WPW + w;
    if (seg >= a.nseg) return;
    if (stream_fmt(fmt) == IQF_S8) {
        a.out_stride *= 2;
        interp_wave_segment<L, false, IQF_S8>(a, seg, own_stream(), lds[w]);
        END_OF_BRANCH("s8");
    } else {
        interp_wave_segment<L, false, IQF_S16>(a, seg, own_stream(), lds[w]);
        END_OF_BRANCH("s16");
    }
}
template <int L, int WPW> __global__ __launch_bounds__(WNT * WPW) void interp_wave_mixed_count_kernel(InterpArgs a, const int *fmt)
{
    __shared__ __attribute__((aligned(16))) int lds[WPW][WGeo<(L == 6) ? 5 : L>::ldsDw];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int seg = (int)blockIdx.x * WPW + w;
    if (seg >= a.nseg) return;
    if (!ragged_args(a, seg, (int)blockIdx.y, (size_t)a.nsub_per_seg * WB)) return;
    if (stream_fmt(fmt) == IQF_S8) {
        a.out_stride *= 2;
        interp_wave_segment<L, false, IQF_S8>(a, seg, own_stream(), lds[w]);
        END_OF_BRANCH("s8");
    } else {
        interp_wave_segment<L, false, IQF_S16>(a, seg, own_stream(), lds[w]);
        END_OF_BRANCH("s16");
    }
}
template <int L> __global__ __launch_bounds__(NT) void interp_mixed_kernel(InterpArgs a, const int *fmt)
{
    __shared__ __attribute__((aligned(16))) int lds[IGeo<(L == 6) ? 5 : L>::ldsDw];
    if (stream_fmt(fmt) == IQF_S8) {
        a.out_stride *= 2;
        interp_segment<L, false, IQF_S8>(a, blockIdx.x, own_stream(), lds);
        END_OF_BRANCH("s8");
    } else {
        interp_segment<L, false, IQF_S16>(a, blockIdx.x, own_stream(), lds);
        END_OF_BRANCH("s16");
    }
}
template <int L> __global__ __launch_bounds__(NT) void interp_mixed_count_kernel(InterpArgs a, const int *fmt)
{
    __shared__ __attribute__((aligned(16))) int lds[IGeo<(L == 6) ? 5 : L>::ldsDw];
    if (!ragged_args(a, (int)blockIdx.x, (int)blockIdx.y, (size_t)a.nsub_per_seg * IGeo<(L == 6) ? 5 : L>::mc)) return;
    if (stream_fmt(fmt) == IQF_S8) {
        a.out_stride *= 2;
        interp_segment<L, true, IQF_S8>(a, blockIdx.x, own_stream(), lds);
        END_OF_BRANCH("s8");
    } else {
        interp_segment<L, true, IQF_S16>(a, blockIdx.x, own_stream(), lds);
        END_OF_BRANCH("s16");
    }
}

// K6x.  in: int16 rows, in_stride samples apart; out: rows 4 * out_stride bytes apart
constexpr int X1_NT = 256;
__global__ __launch_bounds__(X1_NT) void interp1_mixed_kernel(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n_max,
                                                              const int *fmt, const int *count, int count_stride, int count_unit)
{
    const int s = (int)blockIdx.y;
    size_t n = n_max;
    if (count) {
        const int k = __builtin_amdgcn_readfirstlane(count[(size_t)s * (size_t)count_stride]);
        n = (size_t)(unsigned)k * (size_t)(unsigned)count_unit;
        if (n > n_max) n = n_max; // (never beyond what the grid and the buffers were planned for)
    }
    const unsigned *row = reinterpret_cast<const unsigned *>(in) + (size_t)s * in_stride;
    uint8_t *orow = out + (size_t)s * out_stride * 4;
    const size_t t0 = (size_t)blockIdx.x * X1_NT + threadIdx.x, step = (size_t)gridDim.x * X1_NT;
    if (stream_fmt(fmt) == IQF_S8) {
        const size_t groups = n >> 3; // 8 samples: two 16-byte loads, one 16-byte store
        for (size_t g = t0; g < groups; g += step) {
            const uint4_t *p = reinterpret_cast<const uint4_t *>(row + 8 * g);
            const uint4_t a = SDRHIP_STREAM_LOAD(p), b = SDRHIP_STREAM_LOAD(p + 1);
            uint4_t o;
            o.x = __builtin_amdgcn_perm(a.y, a.x, 0x07050301u); // (re hi8, im hi8) of two samples
            o.y = __builtin_amdgcn_perm(a.w, a.z, 0x07050301u);
            o.z = __builtin_amdgcn_perm(b.y, b.x, 0x07050301u);
            o.w = __builtin_amdgcn_perm(b.w, b.z, 0x07050301u);
            reinterpret_cast<uint4_t *>(orow)[g] = o;
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
            const size_t i = (groups << 3) + threadIdx.x;
            const unsigned x = row[i];
            orow[2 * i] = (uint8_t)(x >> 8);
            orow[2 * i + 1] = (uint8_t)(x >> 24);
        }
    } else {
        const size_t groups = n >> 2; // 4 samples: one 16-byte load, one 16-byte store
        for (size_t g = t0; g < groups; g += step)
            reinterpret_cast<uint4_t *>(orow)[g] = SDRHIP_STREAM_LOAD(reinterpret_cast<const uint4_t *>(row) + g);
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const size_t i = (groups << 2) + threadIdx.x;
            reinterpret_cast<unsigned *>(orow)[i] = row[i];
        }
    }
}

// (the workgroup shapes of launch_w / launch_l and their ragged twins, decided on the planned -- largest -- grid)
template <int L> hipError_t launch_w_mixed(const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    constexpr int WPW = 4;
    const bool four = (size_t)a.nseg * (size_t)a.nstreams >= 4096;
    if (a.count) {
        if (four) hipLaunchKernelGGL((interp_wave_mixed_count_kernel<L, WPW>), dim3((a.nseg + WPW - 1) / WPW, a.nstreams), dim3(WNT * WPW), 0, stream, a, fmt);
        else hipLaunchKernelGGL((interp_wave_mixed_count_kernel<L, 1>), dim3(a.nseg, a.nstreams), dim3(WNT), 0, stream, a, fmt);
    } else if (four)
        hipLaunchKernelGGL((interp_wave_mixed_kernel<L, WPW>), dim3((a.nseg + WPW - 1) / WPW, a.nstreams), dim3(WNT * WPW), 0, stream, a, fmt);
    else
        hipLaunchKernelGGL((interp_wave_mixed_kernel<L, 1>), dim3(a.nseg, a.nstreams), dim3(WNT), 0, stream, a, fmt);
    return hipGetLastError();
}

template <int L> hipError_t launch_l_mixed(const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    if (a.count) hipLaunchKernelGGL((interp_mixed_count_kernel<L>), dim3(a.nseg, a.nstreams), dim3(NT), 0, stream, a, fmt);
    else hipLaunchKernelGGL((interp_mixed_kernel<L>), dim3(a.nseg, a.nstreams), dim3(NT), 0, stream, a, fmt);
    return hipGetLastError();
}

} // namespace

hipError_t launch_interpolate_wave_mixed(int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    if (!fmt || a.gmap) return hipErrorInvalidValue;
    switch (log2interp) {
    case 2: return launch_w_mixed<2>(a, fmt, stream);
    case 3: return launch_w_mixed<3>(a, fmt, stream);
    case 4: return launch_w_mixed<4>(a, fmt, stream);
    case 5: return launch_w_mixed<5>(a, fmt, stream);
    case 6: return launch_w_mixed<6>(a, fmt, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_interpolate_mixed(int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    if (!fmt || a.gmap) return hipErrorInvalidValue;
    switch (log2interp) {
    case 1: return launch_l_mixed<1>(a, fmt, stream);
    case 2: return launch_l_mixed<2>(a, fmt, stream);
    case 3: return launch_l_mixed<3>(a, fmt, stream);
    case 4: return launch_l_mixed<4>(a, fmt, stream);
    case 5: return launch_l_mixed<5>(a, fmt, stream);
    case 6: return launch_l_mixed<6>(a, fmt, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_interpolate1_mixed(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n, int nstreams, const int *fmt,
                                     const int *count, int count_stride, int count_unit, hipStream_t stream)
{
    if (!fmt) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    // enough workgroups for the whole chip (256 CUs x 8 per row set), then each lane loops: K6n's grid, sized for the int16 copy
    size_t blocks = ((n >> 2) + X1_NT - 1) / X1_NT;
    const size_t cap = (size_t)2048 / (size_t)(nstreams > 0 ? nstreams : 1) + 1;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(interp1_mixed_kernel, dim3((unsigned)blocks, (unsigned)nstreams), dim3(X1_NT), 0, stream, in, in_stride, out, out_stride, n, fmt, count,
                       count_stride, count_unit);
    return hipGetLastError();
}

} // namespace sdrhip
