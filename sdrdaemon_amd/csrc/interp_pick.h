// interp_pick.h -- which kernel a call of the interpolator bank runs: the x1 copy, K6n or K6x, or one variant of K5 (valu) / K5w (wave)
// in workgroups of one or four waves.  Pure host arithmetic on plain types (C++11, standard headers only): interpolate_device asks it,
// the launchers of interp_variant.h follow it, tests/cxx/interp_pick_test.cpp walks every combination on a CPU.
#pragma once
#include <cstddef>

namespace sdrhip {
constexpr int INTERP_S16 = 0, INTERP_S8 = 2; // (= SDRHIP_IQ_* of include/sdrhip.h)

// what a variant kernel does beside the plain one (interp_variant.h); a variant is an OR of these
constexpr unsigned IV_GATHER = 1; // input through the Tx decoder's position map (InterpArgs::gmap): K5w only, alone
constexpr unsigned IV_COUNT = 2;  // per-stream input counts (InterpArgs::count)
constexpr unsigned IV_S8 = 4;     // 8-bit output, bank-wide
constexpr unsigned IV_TABLE = 8;  // the output format per stream, from a table on the device (never with IV_S8: the table decides)

enum InterpRoute {
    IR_REFUSED, // no kernel serves the combination: `why`
    IR_COPY,    // x1, int16: a strided copy
    IR_K6N,     // x1, 8-bit: the copy, narrowed
    IR_K6X,     // x1 with a format table
    IR_VALU,    // K5
    IR_WAVE,    // K5w
};

struct InterpPick {
    InterpRoute route;
    unsigned variant; // IV_*, of IR_VALU / IR_WAVE
    int wpw;          // waves per workgroup, of IR_WAVE: 1 or 4
    const char *why;  // of IR_REFUSED
};

// K5w serves interpolate4 .. 64 unless the context says interp_path = valu
inline bool interp_pick_wave(bool interp_wave, int log2interp) { return interp_wave && log2interp >= 2; }

// Workgroups of four waves where the grid fills the chip with them, else one wave per workgroup (interp_wave_kernel);
// segments = nseg * nstreams of the planned -- largest -- grid
inline int interp_pick_wpw(InterpRoute route, size_t segments) { return route == IR_WAVE && segments >= 4096 ? 4 : 1; }

// interp_wave: the context's option; gather / count / table: whether the call has a position map, a count table, a format table;
// out_fmt: the bank-wide format, not looked at where a table is given; segments: as above (a caller that plans by the route picks
// with 0 and settles wpw behind its plan).  The x1 routes take every stream's n_in except K6x, which reads the counts itself
inline InterpPick interp_pick(int log2interp, bool interp_wave, bool gather, bool count, int out_fmt, bool table, size_t segments)
{
    InterpPick p = {IR_REFUSED, 0, 1, nullptr};
    const bool wave = interp_pick_wave(interp_wave, log2interp);
    if (log2interp < 0 || log2interp > 6) p.why = "log2interp out of range";
    else if (gather && !wave) p.why = "gathered input needs the wave interpolator";
    else if (gather && count) p.why = "no ragged gather";
    else if (gather && (out_fmt != INTERP_S16 || table)) p.why = "gathered input has int16 output only";
    else if (log2interp == 0) p.route = table ? IR_K6X : out_fmt == INTERP_S8 ? IR_K6N : IR_COPY;
    else {
        p.route = wave ? IR_WAVE : IR_VALU;
        p.variant = (gather ? IV_GATHER : 0u) | (count ? IV_COUNT : 0u) | (table ? IV_TABLE : out_fmt == INTERP_S8 ? IV_S8 : 0u);
        p.wpw = interp_pick_wpw(p.route, segments);
    }
    return p;
}

// The sample-fed ragged entry (sdrhip_interpolate_ragged, K5c): per-stream counts from the host, a 1-D grid over a per-call table of
// (stream, segment) entries (interp_ragged_plan.h) and kernels of their own (interp_ragged_kernels.hip).  A flag of its own, never
// combined with the others and never an answer of interp_pick: int16 output, contiguous input, no format
constexpr unsigned IV_MAPPED = 16;
// x1: IR_COPY (a ragged copy kernel, not the strided copy); wpw is settled behind the plan, on the table's real number of entries
inline InterpPick interp_pick_mapped(int log2interp, bool interp_wave)
{
    InterpPick p = {IR_REFUSED, 0, 1, nullptr};
    if (log2interp < 0 || log2interp > 6) p.why = "log2interp out of range";
    else if (log2interp == 0) p.route = IR_COPY;
    else {
        p.route = interp_pick_wave(interp_wave, log2interp) ? IR_WAVE : IR_VALU;
        p.variant = IV_MAPPED;
    }
    return p;
}
} // namespace sdrhip
