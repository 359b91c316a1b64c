// The interpolator bank's choice of kernel (sdrdaemon_amd/csrc/interp_pick.h) against a hand transcription of what the bank did before
// the choice was one function: the if-chain of interpolate_device and the guards and dispatch of its twelve launch_interpolate*
// functions, each written out below as it stood, kernels by the names they had.  Every combination of log2interp 0..6, interp_wave,
// gather, count, out_fmt {S16, S8}, table and a grid below, at and above 4096 segments: a refused one must be refused, an accepted one
// must name the kernel the chain launched.  Stand-alone (no GPU, no library); built with the address and undefined-behaviour
// sanitizers by tests/test_interp_pick.py.
#include "interp_pick.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace sdrhip;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- the transcription
enum Outcome { W_EINVAL, W_LAUNCH_REFUSED /* hipErrorInvalidValue from a launch_* */, W_COPY, W_K6N, W_K6X, W_KERNEL };
struct Was {
    Outcome outcome;
    std::string kernel; // template name
    int L, wpw;         // wpw 0: a K5 kernel (one template argument)
};
struct Args { // what the launch_* functions looked at in InterpArgs
    bool count, gmap;
    size_t segments; // nseg * nstreams
};
static Was refused() { Was w = {W_LAUNCH_REFUSED, "", 0, 0}; return w; }
static Was kernel(const char *name, int L, int wpw) { Was w = {W_KERNEL, name, L, wpw}; return w; }

// launch_w / launch_w_ragged / launch_w_s8 / launch_w_mixed: workgroups of four where the grid has 4096 segments
static Was was_launch_w(int L, const Args &a) { return kernel(a.gmap ? "interp_wave_gather_kernel" : "interp_wave_kernel", L, a.segments >= 4096 ? 4 : 1); }
static Was was_launch_w_ragged(int L, const Args &a) { return kernel("interp_wave_ragged_kernel", L, a.segments >= 4096 ? 4 : 1); }
static Was was_launch_w_s8(int L, const Args &a) { return kernel(a.count ? "interp_wave_s8_count_kernel" : "interp_wave_s8_kernel", L, a.segments >= 4096 ? 4 : 1); }
static Was was_launch_w_mixed(int L, const Args &a) { return kernel(a.count ? "interp_wave_mixed_count_kernel" : "interp_wave_mixed_kernel", L, a.segments >= 4096 ? 4 : 1); }
static Was was_launch_l(int L, const Args &) { return kernel("interp_kernel", L, 0); }
static Was was_launch_l_ragged(int L, const Args &) { return kernel("interp_ragged_kernel", L, 0); }
static Was was_launch_l_s8(int L, const Args &a) { return kernel(a.count ? "interp_s8_count_kernel" : "interp_s8_kernel", L, 0); }
static Was was_launch_l_mixed(int L, const Args &a) { return kernel(a.count ? "interp_mixed_count_kernel" : "interp_mixed_kernel", L, 0); }

// the twelve exported functions: a guard, then `switch (log2interp)` over 2..6 (wave) or 1..6
static Was was_launch_interpolate_wave(int L, const Args &a) { return L >= 2 && L <= 6 ? was_launch_w(L, a) : refused(); }
static Was was_launch_interpolate(int L, const Args &a) { return L >= 1 && L <= 6 ? was_launch_l(L, a) : refused(); }
static Was was_launch_interpolate_wave_ragged(int L, const Args &a)
{
    if (!a.count || a.gmap) return refused();
    return L >= 2 && L <= 6 ? was_launch_w_ragged(L, a) : refused();
}
static Was was_launch_interpolate_ragged(int L, const Args &a)
{
    if (!a.count) return refused();
    return L >= 1 && L <= 6 ? was_launch_l_ragged(L, a) : refused();
}
static Was was_launch_interpolate_wave_s8(int L, const Args &a)
{
    if (a.gmap || a.count) return refused();
    return L >= 2 && L <= 6 ? was_launch_w_s8(L, a) : refused();
}
static Was was_launch_interpolate_wave_ragged_s8(int L, const Args &a)
{
    if (!a.count || a.gmap) return refused();
    return L >= 2 && L <= 6 ? was_launch_w_s8(L, a) : refused();
}
static Was was_launch_interpolate_s8(int L, const Args &a)
{
    if (a.gmap || a.count) return refused();
    return L >= 1 && L <= 6 ? was_launch_l_s8(L, a) : refused();
}
static Was was_launch_interpolate_ragged_s8(int L, const Args &a)
{
    if (!a.count || a.gmap) return refused();
    return L >= 1 && L <= 6 ? was_launch_l_s8(L, a) : refused();
}
static Was was_launch_interpolate_wave_mixed(int L, const Args &a, bool fmt)
{
    if (!fmt || a.gmap) return refused();
    return L >= 2 && L <= 6 ? was_launch_w_mixed(L, a) : refused();
}
static Was was_launch_interpolate_mixed(int L, const Args &a, bool fmt)
{
    if (!fmt || a.gmap) return refused();
    return L >= 1 && L <= 6 ? was_launch_l_mixed(L, a) : refused();
}

// interpolate_device behind its n_in == 0 exit; IQF_S16 = 0, IQF_S8 = 2
static Was was_interpolate_device(int log2interp, bool opt_interp_wave, bool gather, bool count, int out_fmt, bool fmt_dev, size_t segments)
{
    const Was einval = {W_EINVAL, "", 0, 0};
    if (gather && !(opt_interp_wave && log2interp >= 2)) return einval; // interpolate_gather_ok
    if (gather && count) return einval;
    if (gather && (out_fmt != 0 || fmt_dev)) return einval;
    if (log2interp == 0 && fmt_dev) { Was w = {W_K6X, "", 0, 0}; return w; }
    if (log2interp == 0 && out_fmt == 2) { Was w = {W_K6N, "", 0, 0}; return w; }
    if (log2interp == 0) { Was w = {W_COPY, "", 0, 0}; return w; }
    const Args a = {count, gather, segments};
    const bool use_wave = opt_interp_wave && log2interp >= 2;
    const int L = log2interp;
    if (fmt_dev) return use_wave ? was_launch_interpolate_wave_mixed(L, a, fmt_dev) : was_launch_interpolate_mixed(L, a, fmt_dev);
    else if (out_fmt == 2) {
        if (count) return use_wave ? was_launch_interpolate_wave_ragged_s8(L, a) : was_launch_interpolate_ragged_s8(L, a);
        else return use_wave ? was_launch_interpolate_wave_s8(L, a) : was_launch_interpolate_s8(L, a);
    } else if (count) return use_wave ? was_launch_interpolate_wave_ragged(L, a) : was_launch_interpolate_ragged(L, a);
    else return use_wave ? was_launch_interpolate_wave(L, a) : was_launch_interpolate(L, a);
}

// ---- the kernel a pick names, by the name it had: the plain kernels keep theirs
static std::string named(const InterpPick &p)
{
    const bool w = p.route == IR_WAVE;
    switch (p.variant) {
    case 0: return w ? "interp_wave_kernel" : "interp_kernel";
    case IV_GATHER: return w ? "interp_wave_gather_kernel" : "(no gathered K5)";
    case IV_COUNT: return w ? "interp_wave_ragged_kernel" : "interp_ragged_kernel";
    case IV_S8: return w ? "interp_wave_s8_kernel" : "interp_s8_kernel";
    case IV_S8 | IV_COUNT: return w ? "interp_wave_s8_count_kernel" : "interp_s8_count_kernel";
    case IV_TABLE: return w ? "interp_wave_mixed_kernel" : "interp_mixed_kernel";
    case IV_TABLE | IV_COUNT: return w ? "interp_wave_mixed_count_kernel" : "interp_mixed_count_kernel";
    }
    return "(no such variant)";
}

int main()
{
    static_assert(INTERP_S16 == 0 && INTERP_S8 == 2, "SDRHIP_IQ_S16 / SDRHIP_IQ_S8");
    const size_t grids[3] = {4095, 4096, 4097};
    const int fmts[2] = {INTERP_S16, INTERP_S8};
    int cases = 0, accepted = 0, kernels = 0;
    for (int L = 0; L <= 6; ++L)
        for (int wave = 0; wave < 2; ++wave)
            for (int gather = 0; gather < 2; ++gather)
                for (int count = 0; count < 2; ++count)
                    for (int f = 0; f < 2; ++f)
                        for (int table = 0; table < 2; ++table)
                            for (int g = 0; g < 3; ++g) {
                                const Was w = was_interpolate_device(L, wave, gather, count, fmts[f], table, grids[g]);
                                const InterpPick p = interp_pick(L, wave, gather, count, fmts[f], table, grids[g]);
                                char what[128];
                                std::snprintf(what, sizeof what, "L %d wave %d gather %d count %d fmt %d table %d grid %zu", L, wave, gather, count, fmts[f], table,
                                              grids[g]);
                                ++cases;
                                // (no accepted call reached a launch_* guard: the chain's own refusals come first)
                                CHECK(w.outcome != W_LAUNCH_REFUSED, "%s", what);
                                if (w.outcome == W_EINVAL) {
                                    CHECK(p.route == IR_REFUSED && p.why && std::strlen(p.why) > 0, "%s: route %d", what, (int)p.route);
                                    continue;
                                }
                                ++accepted;
                                CHECK(p.why == nullptr, "%s", what);
                                if (w.outcome == W_COPY) CHECK(p.route == IR_COPY, "%s: route %d", what, (int)p.route);
                                else if (w.outcome == W_K6N) CHECK(p.route == IR_K6N, "%s: route %d", what, (int)p.route);
                                else if (w.outcome == W_K6X) CHECK(p.route == IR_K6X, "%s: route %d", what, (int)p.route);
                                else {
                                    ++kernels;
                                    CHECK(p.route == (w.wpw ? IR_WAVE : IR_VALU), "%s: route %d, was %s", what, (int)p.route, w.kernel.c_str());
                                    CHECK(named(p) == w.kernel, "%s: %s, was %s", what, named(p).c_str(), w.kernel.c_str());
                                    CHECK(w.L == L && (p.route == IR_WAVE ? L >= 2 : L >= 1), "%s", what);
                                    CHECK(p.wpw == (w.wpw ? w.wpw : 1), "%s: wpw %d, was %d", what, p.wpw, w.wpw);
                                    // the planner's path and the later settling of wpw agree with the one-call form
                                    const InterpPick q = interp_pick(L, wave, gather, count, fmts[f], table, 0);
                                    CHECK(q.route == p.route && q.variant == p.variant && q.wpw == 1, "%s", what);
                                    CHECK(interp_pick_wpw(q.route, grids[g]) == p.wpw, "%s", what);
                                    CHECK(interp_pick_wave(wave, L) == (p.route == IR_WAVE), "%s", what);
                                }
                            }
    CHECK(cases == 7 * 2 * 2 * 2 * 2 * 2 * 3, "%d", cases);
    // out of range: never a kernel
    CHECK(interp_pick(-1, true, false, false, INTERP_S16, false, 1).route == IR_REFUSED, "L -1");
    CHECK(interp_pick(7, true, false, false, INTERP_S16, false, 1).route == IR_REFUSED, "L 7");
    std::printf("%d cases, %d accepted, %d of them kernels, %d failures\n", cases, accepted, kernels, failures);
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
