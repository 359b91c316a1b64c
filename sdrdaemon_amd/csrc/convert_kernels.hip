// convert_kernels.hip -- 8-bit IQ at the edges of the pipes (include/sdrhip.h "IQ sample formats").
//
// K0 (widen): the Rx pipe's 8-bit input -> the int16 IQSample rows the decimator reads.  RtlSdrSource's callback does it on a host
// core, IQSample(buf[2i] - 128, buf[2i + 1] - 128) (RtlSdrSource.cpp:542-553), HackRFSource's IQSample(buf[2i], buf[2i + 1])
// (HackRFSource.cpp:661-674); here the bytes cross the host link as they are and one pass on the device widens them: the row
// pass of rx_unpack_body.h (a lane takes 8 samples: one 16-byte load, two 16-byte stores), which K0r runs with per-stream counts.
//
// K6n (narrow): the Tx pipe's interpolate1 (a copy, Upsampler.cpp:54-57) with 8-bit output, HackRFSink's buf[2i] = real() >> 8,
// buf[2i + 1] = imag() >> 8 (HackRFSink.cpp:671-672): byte 1 of every int16 component.  A lane takes 8 samples: two 16-byte loads,
// one 16-byte store.  (Interpolating ratios narrow in the interpolator's last stage instead, interp_wave.h / interp_body.h.)
//
// Rows are 16-byte aligned (8-bit strides are multiples of 8 samples, int16 strides multiples of 4); a row's last n % 8 samples go
// sample by sample, so no lane reads or writes past a row's n samples.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned cvt_uint4_t __attribute__((ext_vector_type(4)));
constexpr int CVT_NT = 256;

#include "rx_unpack_body.h"

template <int FMT> __global__ __launch_bounds__(CVT_NT) void iq8_widen_kernel(const uint8_t *in, size_t in_stride, int16_t *out, size_t out_stride,
                                                                               size_t n)
{
    const int s = (int)blockIdx.y;
    iq8_widen_row<FMT>(in + (size_t)s * in_stride * 2, reinterpret_cast<unsigned *>(out) + (size_t)s * out_stride, n);
}

__global__ __launch_bounds__(CVT_NT) void iq8_narrow_kernel(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n)
{
    const int s = (int)blockIdx.y;
    const unsigned *row = reinterpret_cast<const unsigned *>(in) + (size_t)s * in_stride;
    uint8_t *orow = out + (size_t)s * out_stride * 2;
    const size_t groups = n >> 3;
    for (size_t g = (size_t)blockIdx.x * CVT_NT + threadIdx.x; g < groups; g += (size_t)gridDim.x * CVT_NT) {
        const cvt_uint4_t *p = reinterpret_cast<const cvt_uint4_t *>(row + 8 * g);
        const cvt_uint4_t a = SDRHIP_STREAM_LOAD(p), b = SDRHIP_STREAM_LOAD(p + 1);
        cvt_uint4_t o;
        o.x = __builtin_amdgcn_perm(a.y, a.x, 0x07050301u); // (re hi8, im hi8) of two samples
        o.y = __builtin_amdgcn_perm(a.w, a.z, 0x07050301u);
        o.z = __builtin_amdgcn_perm(b.y, b.x, 0x07050301u);
        o.w = __builtin_amdgcn_perm(b.w, b.z, 0x07050301u);
        reinterpret_cast<cvt_uint4_t *>(orow)[g] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const size_t i = (groups << 3) + threadIdx.x;
        const unsigned x = row[i];
        orow[2 * i] = (uint8_t)(x >> 8);
        orow[2 * i + 1] = (uint8_t)(x >> 24);
    }
}

} // namespace

hipError_t launch_iq8_widen(int fmt, const uint8_t *in, size_t in_stride, int16_t *out, size_t out_stride, size_t n, int nstreams,
                            hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const dim3 grid(cvt_blocks(n >> 3, nstreams), (unsigned)nstreams);
    if (fmt == IQF_U8) hipLaunchKernelGGL((iq8_widen_kernel<IQF_U8>), grid, dim3(CVT_NT), 0, stream, in, in_stride, out, out_stride, n);
    else if (fmt == IQF_S8) hipLaunchKernelGGL((iq8_widen_kernel<IQF_S8>), grid, dim3(CVT_NT), 0, stream, in, in_stride, out, out_stride, n);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_iq8_narrow(const int16_t *in, size_t in_stride, uint8_t *out, size_t out_stride, size_t n, int nstreams, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(iq8_narrow_kernel, dim3(cvt_blocks(n >> 3, nstreams), (unsigned)nstreams), dim3(CVT_NT), 0, stream, in, in_stride, out, out_stride, n);
    return hipGetLastError();
}

} // namespace sdrhip
