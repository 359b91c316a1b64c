// rx_egress_kernels.hip -- KE, the departure-order delivery of the Rx pipe's asynchronous batches (sdrhip_rx_set_egress,
// SDRHIP_EGRESS_ROUND_ROBIN; the host side is sdrhip_rx_egress.cpp, the order rx_egress_order.h).  It takes the place of KD (a
// datagram batch, rx_dgram_async_kernels.hip) or of the frame gather (a ragged batch) and writes the same contiguous buffer that ONE
// download brings to the host: the datagrams of every delivered frame, then the records as KD lays them out.  Only the order of the
// datagrams differs: datagram j of every stream before datagram j + 1 of any.
// One run per delivered frame (RxEgressRun): the frame's B datagrams lie back to back at frames + src and go to out + dst + b stride.
// B is the batch's, so a frame gets wgpf = ceil(B / 32) workgroups and workgroup -> frame is a division.  Half a wave takes a
// datagram -- 32 lanes x 16 bytes, as in KX -- so a wave instruction reads 1 KiB in one piece and writes two 512-byte pieces; a
// lane moves four chunks (datagrams 8 apart inside the workgroup's 32), all four non-temporal loads in flight before the first
// store.  The loads are unconditional: a datagram past the frame's last (B no multiple of 32: the last workgroup of a frame, down to
// one half-filled wave for B = 129) reads the last one instead, only the stores are guarded.
// The records (a datagram batch): the collector's public records lie [stream][kmax], stream s released cnt of them; record k of
// stream s goes to out + rec_dst + 16 (pre + k), {pre, cnt} per stream (one 16-byte entry) from the host's own counts.  The workgroups behind the
// frames' take 1024 record slots each; slot -> stream is a division by kmax.
// Every piece is 16-byte aligned on both sides (rx_egress_order.h refuses anything else), destination offsets are 64-bit.  No LDS,
// no barrier, no scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

#include "rx_records_body.h"

constexpr int KE_NT = 256;
constexpr int KE_PER = 4;                  // 16-byte chunks per lane
constexpr unsigned KE_CHUNKS = 512 / 16;   // chunks of a datagram = lanes of a half-wave
constexpr unsigned KE_HALVES = KE_NT / KE_CHUNKS; // datagrams a workgroup moves per step
static_assert(KE_HALVES * KE_PER == RX_EGRESS_WG_DGRAMS, "workgroup share");
static_assert(sizeof(RxEgressRun) == 24, "run layout");

__global__ __launch_bounds__(KE_NT) void rx_egress_kernel(const RxEgressRun *__restrict__ runs, unsigned frame_wgs, unsigned wgpf,
                                                          unsigned B, const uint8_t *__restrict__ frames, uint8_t *__restrict__ out,
                                                          RxEgressRecords rec)
{
    const unsigned wg = blockIdx.x;
    uint4_t v[KE_PER];
    if (wg < frame_wgs) {
        // (the quotient is the same in every lane; saying so keeps the run in scalar registers: one s_load, no per-lane table read)
        const unsigned k = __builtin_amdgcn_readfirstlane(wg / wgpf), w = wg - k * wgpf;
        const RxEgressRun r = runs[k];
        const unsigned lane = threadIdx.x % KE_CHUNKS, d0 = w * RX_EGRESS_WG_DGRAMS + threadIdx.x / KE_CHUNKS;
        const uint4_t *src = reinterpret_cast<const uint4_t *>(frames + r.src) + lane;
#pragma unroll
        for (int j = 0; j < KE_PER; ++j) {
            const unsigned d = d0 + j * KE_HALVES < B ? d0 + j * KE_HALVES : B - 1;
            v[j] = __builtin_nontemporal_load(src + (size_t)d * KE_CHUNKS);
        }
        // (keeps the compiler from sinking a load into its store's branch, behind the waits of the others)
#pragma unroll
        for (int j = 0; j < KE_PER; ++j) asm volatile("" : "+v"(v[j]));
        uint8_t *dst = out + r.dst + lane * 16;
#pragma unroll
        for (int j = 0; j < KE_PER; ++j) {
            const unsigned d = d0 + j * KE_HALVES;
            if (d < B) *reinterpret_cast<uint4_t *>(dst + (uint64_t)d * r.stride) = v[j];
        }
        return;
    }
    deliver_records_wg<KE_NT, KE_PER>(wg - frame_wgs, rec, out); // ---- the records (rx_records_body.h)
}

} // namespace

hipError_t launch_rx_egress(const RxEgressRun *runs, uint64_t nruns, uint32_t wg_per_frame, uint32_t blocks_per_frame, const uint8_t *frames,
                            uint8_t *out, const RxEgressRecords &rec, hipStream_t stream)
{
    const uint64_t frame_wgs = nruns * wg_per_frame;
    const uint64_t rec_wgs = ((uint64_t)rec.nslots + KE_NT * KE_PER - 1) / (KE_NT * KE_PER), grid = frame_wgs + rec_wgs;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffu || (nruns && (!blocks_per_frame || wg_per_frame != (blocks_per_frame + RX_EGRESS_WG_DGRAMS - 1) / RX_EGRESS_WG_DGRAMS)) ||
        (rec.nslots && (!rec.kmax || !rec.place || !rec.records || (rec.dst & 15u))) ||
        ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(rec.records)) & 15u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_egress_kernel, dim3((unsigned)grid), dim3(KE_NT), 0, stream, runs, (unsigned)frame_wgs, wg_per_frame, blocks_per_frame,
                       frames, out, rec);
    return hipGetLastError();
}

} // namespace sdrhip
