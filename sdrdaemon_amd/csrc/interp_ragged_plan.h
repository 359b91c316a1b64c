// interp_ragged_plan.h -- the launch geometry of the interpolator kernels: how a call is cut into segments (K5: whole macro-cycles,
// K5w: blocks of 128 inputs), and the per-call table of the sample-fed ragged entry (sdrhip_interpolate_ragged, K5c): one segment
// length for the launch, each stream's own number of segments, one table entry per (stream, segment).  Pure integer arithmetic on
// plain types: C++11, standard headers only (and interp_pick.h, which is as plain), so that tests/cxx/interp_ragged_plan_test.cpp runs
// every rule on a CPU under sanitizers.  Every rule here is a bound a kernel relies on without checking (interp_body.h, interp_wave.h,
// interp_ragged_kernels.hip): a wrong one is an out-of-bounds access or a dropped sample there.
#pragma once
#include <cstddef>
#include <cstdint>

#include "interp_pick.h"

namespace sdrhip {

// ---- what the planners share with the kernels (interp_ragged_kernels.hip asserts that the bodies' own constants agree)
constexpr int INTERP_MC = 512;         // K5: inputs per macro-cycle (interp_body.h: MC; 1024 where the cascade has a single stage)
constexpr int INTERP_WB = 128;         // K5w: inputs per block (interp_wave.h: WB)
constexpr int INTERP_WPAIRS = 8;       // K5w: pairs of blocks a wave parks in registers: a segment is at most 2 x 8 blocks
constexpr size_t INTERP_COPY_SEG = 8192; // x1 of the ragged entry: samples per workgroup of the copy kernel (a multiple of 4)
constexpr size_t interp_macro_cycle(int log2interp) { return log2interp == 1 ? 1024 : (size_t)INTERP_MC; }

// ---- K5: macro-cycles per segment and segments per stream of a call of n_in inputs per stream
inline void interp_plan_valu(int log2interp, size_t n_in, int nstreams, int *nsub_per_seg, int *nseg)
{
    const size_t ci = interp_macro_cycle(log2interp);
    size_t nsub = (n_in + ci - 1) / ci;
    if (nsub == 0) nsub = 1;
    size_t per = 16; // warm-up is 64 inputs: 16 macro-cycles per segment keep its cost below 1 %
    while (per > 1 && ((nsub + per - 1) / per) * (size_t)nstreams < 2048) per >>= 1;
    *nsub_per_seg = (int)per;
    *nseg = (int)((nsub + per - 1) / per);
}

// ---- K5w: blocks of 128 inputs, segments of at most 2 x WPAIRS = 16 blocks (the wave parks its whole segment's input in registers at
// its start), an even number of them (the input comes back a PAIR of blocks at a time; an odd rest runs the guarded path), or one.
// seg_override != 0: the segment length in inputs (context option interp_span; tests)
inline void interp_plan_wave(size_t n_in, size_t seg_override, int *nsub_per_seg, int *nseg)
{
    const size_t maxper = 2 * (size_t)INTERP_WPAIRS;
    size_t nsub = (n_in + INTERP_WB - 1) / INTERP_WB;
    if (nsub == 0) nsub = 1;
    size_t per = seg_override ? (seg_override + INTERP_WB - 1) / INTERP_WB : maxper;
    if (per > maxper) per = maxper;
    if (per > 1) per &= ~(size_t)1;
    if (per < 1) per = 1;
    *nsub_per_seg = (int)per;
    *nseg = (int)((nsub + per - 1) / per);
}

// ---- K5c: the table of a ragged launch, as the kernels read it (scalar loads: an entry and a row are wave-uniform)
struct InterpMapEntry {
    uint32_t stream, seg; // segment `seg` of stream `stream`: inputs [seg * seg_len, min((seg + 1) * seg_len, n_in))
};
struct InterpMapRow {
    uint64_t in_off, out_off; // samples from the call's input / output base to the stream's row
    uint32_t n_in;            // the stream's inputs in this call
    int32_t nseg;             // its segments, max(1, ceil(n_in / seg_len)): segment nseg - 1 writes the stream's state
};
static_assert(sizeof(InterpMapEntry) == 8 && sizeof(InterpMapRow) == 24, "the table's layout: rows, then entries, 8-byte aligned");

struct InterpRaggedPlan {
    InterpRoute route;  // IR_COPY (x1), IR_VALU (K5), IR_WAVE (K5w)
    int wpw;            // waves per workgroup (K5w), by interp_pick_wpw on `entries`
    int nsub_per_seg;   // macro-cycles (K5) or blocks (K5w) per segment; 0 for the copy
    size_t seg_len;     // inputs per segment
    size_t max_n;       // the largest count
    uint32_t entries;   // sum over the streams of max(1, ceil(n_s / seg_len))
    uint32_t grid;      // workgroups: entries, or ceil(entries / wpw) on K5w
};
enum { INTERP_RAGGED_OK = 0, INTERP_RAGGED_EMPTY = 1, INTERP_RAGGED_REFUSED = -1 };
constexpr size_t INTERP_RAGGED_MAX_COUNT = 0x7fffffffu; // InterpMapRow::n_in, and the bodies' int counters
constexpr size_t INTERP_RAGGED_MAX_ENTRIES = 0x7fffffffu; // the 1-D grid, InterpMapRow::nseg and the kernels' int indices

inline size_t interp_ragged_nseg(size_t n, size_t seg_len) { return n ? (n + seg_len - 1) / seg_len : 1; }

// Sizes a ragged launch and touches no table.  route: interp_pick_mapped's answer; span: the interp_span override (K5w alone, as in
// the uniform call).  The segment length comes from the largest count, the way the uniform planners take it from n_in, so equal
// counts get the uniform launch's segments.  INTERP_RAGGED_EMPTY: every count is 0, nothing to launch.  INTERP_RAGGED_REFUSED with
// *why: a count, the number of entries or the grid does not fit the 32-bit fields above
inline int interp_ragged_size(const size_t *n_in, int nstreams, int log2interp, InterpRoute route, size_t span, InterpRaggedPlan *p, const char **why)
{
    *p = InterpRaggedPlan();
    p->route = route; p->wpw = 1;
    if (nstreams <= 0 || !n_in) { *why = "no streams"; return INTERP_RAGGED_REFUSED; }
    if (route != IR_COPY && route != IR_VALU && route != IR_WAVE) { *why = "no ragged kernel serves the route"; return INTERP_RAGGED_REFUSED; }
    const int lo = route == IR_COPY ? 0 : route == IR_WAVE ? 2 : 1, hi = route == IR_COPY ? 0 : 6;
    if (log2interp < lo || log2interp > hi) {
        *why = "the route does not serve the ratio";
        return INTERP_RAGGED_REFUSED;
    }
    size_t max_n = 0;
    for (int s = 0; s < nstreams; ++s) {
        if (n_in[s] > INTERP_RAGGED_MAX_COUNT) { *why = "a count of 2^31 samples or more"; return INTERP_RAGGED_REFUSED; }
        if (n_in[s] > max_n) max_n = n_in[s];
    }
    p->max_n = max_n;
    if (max_n == 0) return INTERP_RAGGED_EMPTY;
    int per = 0, nseg = 0;
    if (route == IR_WAVE) {
        interp_plan_wave(max_n, span, &per, &nseg);
        p->seg_len = (size_t)per * INTERP_WB;
    } else if (route == IR_VALU) {
        interp_plan_valu(log2interp, max_n, nstreams, &per, &nseg);
        p->seg_len = (size_t)per * interp_macro_cycle(log2interp);
    } else
        p->seg_len = INTERP_COPY_SEG;
    p->nsub_per_seg = per;
    size_t entries = 0;
    for (int s = 0; s < nstreams; ++s) {
        entries += interp_ragged_nseg(n_in[s], p->seg_len);
        if (entries > INTERP_RAGGED_MAX_ENTRIES) { *why = "more than 2^31 - 1 segments"; return INTERP_RAGGED_REFUSED; }
    }
    p->entries = (uint32_t)entries;
    p->wpw = interp_pick_wpw(route, entries);
    p->grid = (uint32_t)((entries + (size_t)p->wpw - 1) / (size_t)p->wpw);
    return INTERP_RAGGED_OK;
}

// bytes of the table of a sized launch: nstreams rows, then the entries
inline size_t interp_ragged_table_bytes(int nstreams, const InterpRaggedPlan &p)
{
    return (size_t)nstreams * sizeof(InterpMapRow) + (size_t)p.entries * sizeof(InterpMapEntry);
}

// Fills the table of a sized launch: rows[s] = {s * in_stride, s * out_stride, n_in[s], the stream's segments}, and the entries
// stream-major, segments ascending -- the four waves of a K5w workgroup read neighbouring input.  entries: p.entries of them
inline void interp_ragged_fill(const size_t *n_in, int nstreams, const InterpRaggedPlan &p, size_t in_stride, size_t out_stride, InterpMapRow *rows,
                               InterpMapEntry *entries)
{
    size_t k = 0;
    for (int s = 0; s < nstreams; ++s) {
        const size_t nseg = interp_ragged_nseg(n_in[s], p.seg_len);
        rows[s].in_off = (uint64_t)s * in_stride;
        rows[s].out_off = (uint64_t)s * out_stride;
        rows[s].n_in = (uint32_t)n_in[s];
        rows[s].nseg = (int32_t)nseg;
        for (size_t g = 0; g < nseg; ++g, ++k) {
            entries[k].stream = (uint32_t)s;
            entries[k].seg = (uint32_t)g;
        }
    }
}

// size, then fill a table of `cap` bytes (rows at its start, the entries behind them); a launch that is refused, is empty or does
// not fit `cap` (INTERP_RAGGED_REFUSED) leaves the table as it was
inline int interp_ragged_build(const size_t *n_in, int nstreams, int log2interp, InterpRoute route, size_t span, size_t in_stride, size_t out_stride,
                               void *table, size_t cap, InterpRaggedPlan *p, const char **why)
{
    const int rc = interp_ragged_size(n_in, nstreams, log2interp, route, span, p, why);
    if (rc != INTERP_RAGGED_OK) return rc;
    if (!table || interp_ragged_table_bytes(nstreams, *p) > cap) { *why = "the table does not fit its buffer"; return INTERP_RAGGED_REFUSED; }
    InterpMapRow *rows = static_cast<InterpMapRow *>(table);
    interp_ragged_fill(n_in, nstreams, *p, in_stride, out_stride, rows, reinterpret_cast<InterpMapEntry *>(rows + nstreams));
    return INTERP_RAGGED_OK;
}

// what a kernel makes of an entry: the inputs [*start, *end) of the entry's stream, and whether it writes the stream's state
inline void interp_ragged_segment(const InterpMapRow &row, const InterpMapEntry &e, size_t seg_len, size_t *start, size_t *end, bool *last)
{
    *start = (size_t)e.seg * seg_len;
    *end = *start + seg_len < (size_t)row.n_in ? *start + seg_len : (size_t)row.n_in;
    if (*end < *start) *end = *start;
    *last = (int32_t)e.seg == row.nseg - 1;
}

} // namespace sdrhip
