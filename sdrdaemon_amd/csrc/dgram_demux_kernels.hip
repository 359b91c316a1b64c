// dgram_demux_kernels.hip -- KX, the demultiplexer of tagged datagram batches (sdrhip_fecbuf_write_and_read_tagged,
// sdrhip_tx_submit_datagrams_tagged, sdrhip_rx_submit_datagrams_tagged).  A hub's one socket hands it the datagrams of all its
// streams interleaved in arrival order; the collector's passes (fecbuf_passes.h, not included here) expect every stream's
// datagrams back to back.  The host walks the tags once and gives datagram i its place dest[i] in that order (0xffffffff: the
// datagram belongs to no stream); KX moves datagram i from src + 512 i to dst + 512 dest[i].
// Half a wave takes a datagram: 32 lanes x 16 bytes, one non-temporal dwordx4 load and one dwordx4 store per lane, so that a wave
// instruction reads and writes two whole datagrams (1 KiB, both 512-byte runs contiguous).  A half-wave takes KX_PER consecutive
// datagrams: it reads their dest entries (every lane the same address: one request per entry and half-wave), then has all their
// loads in flight before the first store, as the collector's copy_dwords does.  The tail (n_total no multiple of KX_PER, the last
// partial workgroup) is guarded by index; there is no barrier, no LDS and no scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

constexpr int KX_NT = 256;
constexpr int KX_PER = 4;                  // datagrams per half-wave
constexpr unsigned KX_CHUNKS = 512 / 16;   // 16-byte chunks of a datagram = lanes of a half-wave
constexpr unsigned KX_WG_DGRAMS = KX_NT / KX_CHUNKS * KX_PER;
constexpr unsigned KX_NONE = 0xffffffffu;

__global__ __launch_bounds__(KX_NT) void dgram_demux_kernel(const uint4_t *src, const unsigned *dest, unsigned n_total, uint4_t *dst)
{
    const unsigned half = (blockIdx.x * (unsigned)KX_NT + threadIdx.x) / KX_CHUNKS, lane = threadIdx.x % KX_CHUNKS;
    const unsigned i0 = half * KX_PER; // (the host keeps n_total below 2^30)
    unsigned d[KX_PER];
    uint4_t v[KX_PER];
    // the loads are unconditional, so that none waits for another: a datagram past the end reads the last one instead (n_total > 0:
    // the launcher's), a skipped one is read like any other; only the stores are guarded
#pragma unroll
    for (int j = 0; j < KX_PER; ++j) {
        const unsigned i = i0 + j < n_total ? i0 + j : n_total - 1;
        d[j] = dest[i];
        v[j] = __builtin_nontemporal_load(src + (size_t)i * KX_CHUNKS + lane);
    }
    // (keeps the compiler from sinking a load into its store's branch, behind the waits of the others)
#pragma unroll
    for (int j = 0; j < KX_PER; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
    for (int j = 0; j < KX_PER; ++j)
        if (i0 + j >= n_total) d[j] = KX_NONE;
#pragma unroll
    for (int j = 0; j < KX_PER; ++j)
        if (d[j] != KX_NONE) dst[(size_t)d[j] * KX_CHUNKS + lane] = v[j];
}

} // namespace

hipError_t launch_dgram_demux(const uint8_t *src, const uint32_t *dest, size_t n_total, uint8_t *dst, hipStream_t stream)
{
    if (n_total == 0) return hipSuccess;
    if (n_total > 0x3fffffffu || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n_total + KX_WG_DGRAMS - 1) / KX_WG_DGRAMS);
    hipLaunchKernelGGL(dgram_demux_kernel, dim3(grid), dim3(KX_NT), 0, stream, reinterpret_cast<const uint4_t *>(src), dest, (unsigned)n_total,
                       reinterpret_cast<uint4_t *>(dst));
    return hipGetLastError();
}

} // namespace sdrhip
