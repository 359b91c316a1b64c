// rx_runs_kernels.hip -- KR, the departure-order delivery of an asynchronous Rx batch whose streams' frames differ in length
// (per-stream fecblk, sdrhip_rx_set_stream_fec; the order: rx_depart_order.h).  KE delivers a batch of equal frames with one run
// per frame; here a stream's last datagram can fall inside another stream's frame, the destination stride changes there, and a
// frame splits into runs (RxDepartRun): `count` <= 256 datagrams back to back at frames + src go to out + dst + i stride.
// KE's access shape: half a wave takes a datagram -- 32 lanes x 16 bytes -- a lane moves four chunks (datagrams 8 apart inside the
// workgroup's 32), all four non-temporal loads in flight before the first store.  The loads are unconditional: a datagram past the
// run's last reads the last one instead, only the stores are guarded.
// Workgroups to runs: every run gets wgpr = ceil(longest run of the batch / 32) workgroups, workgroup -> run is a division, and a
// workgroup whose 32 datagrams lie behind its run's end leaves before it loads anything (short runs -- the pieces a stream's end
// cuts off another stream's frame -- cost an idle workgroup each, not a search in every workgroup).
// The records of a datagram batch are handled as in KE: slot i = record i % kmax of stream i / kmax goes to
// out + rec.dst + 16 (pre + k), by the workgroups behind the runs', 1024 slots each.
// Every piece is 16-byte aligned on both sides (rx_depart_order.h refuses anything else), destination offsets are 64-bit.  No LDS,
// no barrier, no scratch.
#include "sdrhip_internal.h"

namespace sdrhip {
namespace {

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

#include "rx_records_body.h"

constexpr int KR_NT = 256;
constexpr int KR_PER = 4;                  // 16-byte chunks per lane
constexpr unsigned KR_CHUNKS = 512 / 16;   // chunks of a datagram = lanes of a half-wave
constexpr unsigned KR_HALVES = KR_NT / KR_CHUNKS; // datagrams a workgroup moves per step
static_assert(KR_HALVES * KR_PER == RX_DEPART_WG_DGRAMS, "workgroup share");
static_assert(sizeof(RxDepartRun) == 24, "run layout");

__global__ __launch_bounds__(KR_NT) void rx_runs_kernel(const RxDepartRun *__restrict__ runs, unsigned run_wgs, unsigned wgpr,
                                                        const uint8_t *__restrict__ frames, uint8_t *__restrict__ out, RxEgressRecords rec)
{
    const unsigned wg = blockIdx.x;
    uint4_t v[KR_PER];
    if (wg < run_wgs) {
        // (the quotient is the same in every lane; saying so keeps the run in scalar registers: scalar loads, no per-lane table read)
        const unsigned k = __builtin_amdgcn_readfirstlane(wg / wgpr), w = wg - k * wgpr;
        const RxDepartRun r = runs[k];
        if (w * RX_DEPART_WG_DGRAMS >= r.count) return; // (a run shorter than the batch's longest: nothing left for this workgroup)
        const unsigned lane = threadIdx.x % KR_CHUNKS, d0 = w * RX_DEPART_WG_DGRAMS + threadIdx.x / KR_CHUNKS;
        const uint4_t *src = reinterpret_cast<const uint4_t *>(frames + r.src) + lane;
#pragma unroll
        for (int j = 0; j < KR_PER; ++j) {
            const unsigned d = d0 + j * KR_HALVES < r.count ? d0 + j * KR_HALVES : r.count - 1;
            v[j] = __builtin_nontemporal_load(src + (size_t)d * KR_CHUNKS);
        }
        // (keeps the compiler from sinking a load into its store's branch, behind the waits of the others)
#pragma unroll
        for (int j = 0; j < KR_PER; ++j) asm volatile("" : "+v"(v[j]));
        uint8_t *dst = out + r.dst + lane * 16;
#pragma unroll
        for (int j = 0; j < KR_PER; ++j) {
            const unsigned d = d0 + j * KR_HALVES;
            if (d < r.count) *reinterpret_cast<uint4_t *>(dst + (uint64_t)d * r.stride) = v[j];
        }
        return;
    }
    deliver_records_wg<KR_NT, KR_PER>(wg - run_wgs, rec, out); // ---- the records (rx_records_body.h)
}

} // namespace

hipError_t launch_rx_runs(const RxDepartRun *runs, uint64_t nruns, uint32_t wg_per_run, const uint8_t *frames, uint8_t *out,
                          const RxEgressRecords &rec, hipStream_t stream)
{
    const uint64_t run_wgs = nruns * wg_per_run;
    const uint64_t rec_wgs = ((uint64_t)rec.nslots + KR_NT * KR_PER - 1) / (KR_NT * KR_PER), grid = run_wgs + rec_wgs;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffu || (nruns && (!wg_per_run || wg_per_run > RX_DEPART_MAX_COUNT / RX_DEPART_WG_DGRAMS || !runs)) ||
        (rec.nslots && (!rec.kmax || !rec.place || !rec.records || (rec.dst & 15u))) ||
        ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(rec.records)) & 15u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rx_runs_kernel, dim3((unsigned)grid), dim3(KR_NT), 0, stream, runs, (unsigned)run_wgs, wg_per_run, frames, out, rec);
    return hipGetLastError();
}

} // namespace sdrhip
