// interp_mixed_kernels.hip -- K5x / K6x: the Tx bank's last stage with the output format per stream (sdrhip_tx_set_stream_format).
//
// K5x: the IV_TABLE variants of interp_variant.h, interp_wave_variant_kernel<L, WPW, V> (x4 .. x64) and interp_variant_kernel<L, V>
// (x2, and interp_path = valu) with V = IV_TABLE and IV_TABLE | IV_COUNT, instantiated here and nowhere else; grids and workgroup
// shapes are those of the bank-wide launches (one launcher serves both).  InterpArgs is unchanged: the table is a second kernel
// argument.
// K6x: x1 (Upsampler.cpp:54-57, samples_out = samples_in) over (chunks, streams): an int16 row is copied, 16 bytes per lane and step,
// an 8-bit row is narrowed to byte 1 of every component (the rule of K6n, convert_kernels.hip), up to the stream's own count where a
// count table is given.  Rows are 16-byte aligned on both sides; a row's last samples go one by one, nothing past them is touched.
// No kernel here uses scratch.
#include "interp_variant.h"

namespace sdrhip {
namespace {

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

} // namespace

hipError_t launch_interpolate_table(const InterpPick &pick, int log2interp, const InterpArgs &a, const int *fmt, hipStream_t stream)
{
    switch (pick.variant) {
    case IV_TABLE: return launch_variant<IV_TABLE>(pick, log2interp, a, fmt, stream);
    case IV_TABLE | IV_COUNT: return launch_variant<IV_TABLE | IV_COUNT>(pick, log2interp, a, fmt, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_interpolate1_mixed(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n, int nstreams, const int *fmt,
                                     const int *count, int count_stride, int count_unit, hipStream_t stream)
{
    if (!fmt) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    // K6n's grid, sized for the int16 copy: 4 samples per lane and step
    hipLaunchKernelGGL(interp1_mixed_kernel, dim3(cvt_blocks(n >> 2, nstreams), (unsigned)nstreams), dim3(X1_NT), 0, stream, in, in_stride, out, out_stride,
                       n, fmt, count, count_stride, count_unit);
    return hipGetLastError();
}

} // namespace sdrhip
