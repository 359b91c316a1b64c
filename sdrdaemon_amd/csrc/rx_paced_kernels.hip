// rx_paced_kernels.hip -- KP, the paced departure-order delivery of the Rx pipe's asynchronous batches (SDRHIP_EGRESS_PACED; the
// order is rx_paced_order.h's, the host side lives beside that of the other orders).  It takes KE's / KR's place and writes the
// same contiguous buffer that ONE download brings to the host: the datagrams of every delivered frame, then the records as KD lays
// them out.  Only the order of the datagrams differs: ascending departure key (2 j + 1) / (2 D_s), and a stream's destinations are
// no constant-stride runs any more.  So KP is a gather keyed by destination: table entry i = the source of the array's datagram i,
// in 16-byte units into the frame area (one dword per datagram, made by the host in its one merge over the streams).  One kernel
// serves batches of equal frames and of per-stream fecblk: the table absorbs the difference.
// Workgroup w (256 lanes) writes the datagrams 32 w .. 32 w + 31: 16 KiB of contiguous stores.  Half a wave takes a datagram --
// 32 lanes x 16 bytes -- and a lane moves four chunks (datagrams 8 apart inside the workgroup's 32): the four table entries first,
// then all four non-temporal loads in flight before the first store.  The loads are unconditional: a datagram past the array's
// last (n no multiple of 32: the last workgroup) reads the last entry again, only the stores are guarded.
// The records of a datagram batch are handled as in KE: slot i = record i % kmax of stream i / kmax goes to
// out + rec.dst + 16 (pre + k), by the workgroups behind the datagrams', 1024 slots each (rx_records_body.h).
// Every piece is 16-byte aligned on both sides (a table entry counts 16-byte units), byte offsets are 64-bit on both sides.  No
// LDS, no barrier, no scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

#include "rx_records_body.h"

constexpr int KP_NT = 256;
constexpr int KP_PER = 4;                  // 16-byte chunks per lane
constexpr unsigned KP_CHUNKS = 512 / 16;   // chunks of a datagram = lanes of a half-wave
constexpr unsigned KP_HALVES = KP_NT / KP_CHUNKS; // datagrams a workgroup moves per step
constexpr unsigned KP_WG_DGRAMS = KP_HALVES * KP_PER;
static_assert(KP_WG_DGRAMS == 32, "workgroup share");

__global__ __launch_bounds__(KP_NT) void rx_paced_kernel(const uint32_t *__restrict__ table, uint64_t n, unsigned dgram_wgs,
                                                         const uint8_t *__restrict__ frames, uint8_t *__restrict__ out, RxEgressRecords rec)
{
    const unsigned wg = blockIdx.x;
    if (wg < dgram_wgs) {
        const unsigned lane = threadIdx.x % KP_CHUNKS;
        const uint64_t d0 = (uint64_t)wg * KP_WG_DGRAMS + threadIdx.x / KP_CHUNKS;
        uint32_t at[KP_PER];
        uint4_t v[KP_PER];
#pragma unroll
        for (int j = 0; j < KP_PER; ++j) {
            const uint64_t d = d0 + j * KP_HALVES < n ? d0 + j * KP_HALVES : n - 1;
            at[j] = table[d];
        }
#pragma unroll
        for (int j = 0; j < KP_PER; ++j)
            v[j] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(frames + (uint64_t)at[j] * 16) + lane);
        // (keeps the compiler from sinking a load into its store's branch, behind the waits of the others)
#pragma unroll
        for (int j = 0; j < KP_PER; ++j) asm volatile("" : "+v"(v[j]));
        uint8_t *dst = out + lane * 16;
#pragma unroll
        for (int j = 0; j < KP_PER; ++j) {
            const uint64_t d = d0 + j * KP_HALVES;
            if (d < n) *reinterpret_cast<uint4_t *>(dst + d * 512) = v[j];
        }
        return;
    }
    deliver_records_wg<KP_NT, KP_PER>(wg - dgram_wgs, rec, out); // ---- the records (rx_records_body.h)
}

} // namespace

hipError_t launch_rx_paced(const uint32_t *table, uint64_t n_dgrams, const uint8_t *frames, uint8_t *out, const RxEgressRecords &rec,
                           hipStream_t stream)
{
    const uint64_t dgram_wgs = (n_dgrams + KP_WG_DGRAMS - 1) / KP_WG_DGRAMS;
    const uint64_t rec_wgs = ((uint64_t)rec.nslots + KP_NT * KP_PER - 1) / (KP_NT * KP_PER), grid = dgram_wgs + rec_wgs;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffu || (n_dgrams && (!table || !frames || !out)) ||
        (rec.nslots && (!rec.kmax || !rec.place || !rec.records || (rec.dst & 15u))) ||
        ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(rec.records)) & 15u) ||
        (reinterpret_cast<uintptr_t>(table) & 3u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_paced_kernel, dim3((unsigned)grid), dim3(KP_NT), 0, stream, table, n_dgrams, (unsigned)dgram_wgs, frames, out, rec);
    return hipGetLastError();
}

} // namespace sdrhip
