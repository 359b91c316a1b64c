// decim_plan.h -- the launch geometry of the decimator kernels: which path a call takes (K1 / K1r on the VALU, K1m / K1mr on the
// matrix cores) and how it is cut into segments, spans, wave groups and pieces.  Pure integer arithmetic on plain types: C++11,
// standard headers only, so that tests/cxx/decim_plan_test.cpp runs every rule on a CPU under sanitizers.  Every rule here is a bound
// a kernel relies on without checking (decim_kernels.hip, decim_mfma.hip, rx_ragged_kernels.hip): a wrong one is an out-of-bounds
// read or a dropped sample there.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdrhip {

// ---- what the planners share with the kernels (decim_body.h and decim_mfma.hip assert that their own constants agree)
constexpr int DECIM_PASS = 2048;           // first-stage inputs per pass of the VALU cascade (decim_body.h: P0)
constexpr size_t MF_HEAD_MIN = 2048;       // K1m: shortest VALU head piece (whole passes)
constexpr size_t MF_TAIL_SEG = 16384;      // K1m: raw samples per tail piece, 8 passes of the VALU code
constexpr size_t MF_READ_AHEAD = 256;      // K1m: the register ring reads 8 steps of 32 samples past a wave's last span
constexpr bool mf_dma_applies(int ns) { return ns == 4; } // the LDS-DMA kernel is decimate16 (period of 32 steps; one workgroup per CU)
// raw samples per pass: the rotating modes (inf / sup) sum four raw samples in front of the first stage
constexpr size_t decim_pass_raw(bool cen) { return cen ? (size_t)DECIM_PASS : (size_t)DECIM_PASS * 4; }

// ---- the path rule: context option decim_path, then mfma_min of the call's total samples; then the planner has to agree
enum { DECIM_PATH_AUTO = 0, DECIM_PATH_VALU = 1, DECIM_PATH_MFMA = 2 };
// A launch of the matrix-core kernel lasts at least one warm-up + the shortest span, i.e. ~20 us at decimate16 and
// twice as long per further stage, however small the call; below these sizes the VALU kernel is faster
// (tools/bench_small.py): 2^22 samples over all streams up to decimate8, 2^23 for decimate16, 2^24, 2^25.
inline size_t mfma_min_samples(size_t mfma_min, int log2decim) { return mfma_min << (log2decim > 3 ? log2decim - 3 : 0); }
// total = the raw samples the call consumes over all streams
inline bool mfma_admitted(int decim_path, size_t mfma_min, int log2decim, size_t total)
{
    return decim_path != DECIM_PATH_VALU && (decim_path == DECIM_PATH_MFMA || total >= mfma_min_samples(mfma_min, log2decim));
}

// ---- K1: picks nsub_per_seg / nseg for a call
inline void plan_decimate(int log2decim, int fcpos, size_t n_used, int nstreams, int *nsub_per_seg, int *nseg)
{
    const bool cen = (fcpos == 2);
    const size_t praw = decim_pass_raw(cen);
    size_t npass = (n_used + praw - 1) / praw;
    if (npass == 0) npass = 1;
    // a segment is a whole number of schedule periods (2^(NS-2) passes) so that full-rate
    // stages never flush early; >= 16 passes keep the warm-up (64 * 2^L samples) below ~3 %.
    const int ns = cen ? log2decim : log2decim - 2;
    size_t period = (size_t)1 << (ns > 2 ? ns - 2 : 0);
    size_t per = period < 32 ? 32 : period; // warm-up = 64 * 2^L of 32 * 2048 samples: 1.6 % at L = 4
    // fewer passes per segment when the call is too short to fill 256 CUs x 4 workgroups
    while (per > period && ((npass + per - 1) / per) * (size_t)nstreams < 2048) per >>= 1;
    while (per > 1 && ((npass + per - 1) / per) * (size_t)nstreams < 256) per >>= 1;
    // the warm-up region must not reach before the stream start
    const size_t wraw = (size_t)64 << log2decim;
    while (per * praw < wraw) per <<= 1;
    *nsub_per_seg = (int)per;
    *nseg = (int)((npass + per - 1) / per);
}

// ---- K1r: one segment length for the call, sized as plan_decimate sizes it for the mean stream; each stream gets the segments its
// own count needs (at least one: its state), so the grid follows the total, not the largest stream.  Reads Row::n_used, writes
// Row::seg0 (the prefix sum of the segment counts); *grid = their sum.  The filter-less modes have no cascade launch: 0 / 0.  false:
// more segments than a grid holds.
template <class Row>
inline bool plan_decimate_ragged(int log2decim, int fcpos, Row *rows, int nstreams, size_t total, int *nsub_per_seg, int *grid)
{
    const bool cen = fcpos == 2;
    *nsub_per_seg = 0; *grid = 0;
    if (log2decim < 1 || (!cen && log2decim < 3)) return true;
    int nseg = 0;
    plan_decimate(log2decim, fcpos, (total + (size_t)nstreams - 1) / (size_t)nstreams, nstreams, nsub_per_seg, &nseg);
    const size_t seg_raw = (size_t)*nsub_per_seg * decim_pass_raw(cen);
    size_t acc = 0;
    for (int s = 0; s < nstreams; ++s) {
        rows[s].seg0 = (int)acc;
        acc += rows[s].n_used ? (size_t)((rows[s].n_used + seg_raw - 1) / seg_raw) : 1;
    }
    if (acc > 0x7fffffffu) return false;
    *grid = (int)acc;
    return true;
}

// ---- K1m: per stream the VALU code runs the head [0, head) and the tail [tail_start, n_used) in pieces of tail_seg samples
// (npieces = 1 + tail pieces), the matrix-core waves run wps groups of 8 spans of `span` raw samples from `head` on.  The pieces go
// to piece_wgs workgroups: the first piece_early of them take piece_share pieces each, every other one a single piece.
// (DecimArgs::mf_* carries these to the kernels: set_mf_args, sdrhip_decim.cpp.)
struct MfPlan {
    size_t head, span, tail_start, tail_seg;
    int wps, npieces;
    int piece_wgs, piece_early, piece_share;
};

// piece workgroups (see decim_mfma_kernel): one piece each, unless the matrix-core workgroups own their CUs (LDS-DMA ring) and
// leave some free: then one EARLY workgroup per free CU with as many pieces as fit beside the matrix part (a piece of 16 Ki
// samples takes ~21 us, a step of the matrix-core waves ~0.2 us: half of the matrix part's time), the rest one piece each.
// items = the launch's pieces, nmf = its matrix-core workgroups
inline void mf_deal_pieces(int log2decim, size_t span, int items, int nmf, int n_cu, MfPlan *p)
{
    const size_t W = (size_t)64 << log2decim;
    p->piece_early = 0; p->piece_share = 0;
    if (mf_dma_applies(log2decim) && n_cu > nmf) {
        int early = n_cu - nmf;
        if (early > items) early = items;
        int share = (int)((W + span) / 6720);
        if (share < 3) share = 3;
        if (share > (items + early - 1) / early) share = (items + early - 1) / early;
        p->piece_early = early; p->piece_share = share;
    }
    const int rest = items - p->piece_early * p->piece_share;
    p->piece_wgs = p->piece_early + (rest > 0 ? rest : 0);
}

// fills *p; false when the call is too short (or the mode unsupported).  span_override != 0 forces the span length (tests);
// ring = the LDS-DMA ring depth the launch will use (DecimArgs::mf_ring: 2 = two waves per SIMD)
inline bool plan_decimate_mfma(int log2decim, int fcpos, size_t n_used, int nstreams, size_t span_override, int n_cu, int ring, MfPlan *p)
{
    // one wave per SIMD on all but one CU of every XCD (MI355X: 8 XCDs x 32 CUs -> 31 workgroups per XCD, 992 waves)
    const int nxcd = n_cu >= 64 && n_cu % 8 == 0 ? 8 : 1;
    const size_t waves1 = (size_t)4 * (size_t)(n_cu > nxcd ? n_cu - nxcd : n_cu);
    const size_t waves3 = 3 * waves1 - waves1 / 13; // a round of three waves per SIMD with some slack (2900 on MI355X)
    if (fcpos != 2 || log2decim < 2 || log2decim > 6) return false; // (decimate2_cen: the VALU kernel is HBM-bound, 63 % against 59 %)
    const size_t W = (size_t)64 << log2decim;     // one period of the schedule = the warm-up
    const size_t head = W > MF_HEAD_MIN ? W : MF_HEAD_MIN; // VALU head piece: whole passes, >= the warm-up of the first span
    if (n_used <= head) return false;
    const size_t n = n_used - head;
    size_t S;
    if (span_override) {
        S = (span_override + W - 1) / W * W;
    } else {
        const size_t total = n * (size_t)nstreams;
        if (log2decim <= 3) {
            // short cascades (decimate4 / 8): TWO waves per SIMD, 62 workgroups per XCD (1984 waves), the spans sized from
            // the wave count like below (tools/sweep_span.sh: 0.238 / 0.262 ms per 2^28 samples against 0.248 / 0.271 with
            // one round of three waves per SIMD, 0.250 / 0.318 with one wave per SIMD); three per SIMD for bigger banks
            S = (total / (waves3 * 8) + W - 1) / W * W;
            const size_t wps2 = 2 * waves1 / (size_t)nstreams;
            if (wps2 >= 1) {
                size_t S2 = n / (8 * wps2) / W * W;
                if (S2 == 0 || n / (8 * S2) > wps2) S2 += W; // (rounding down must not add a wave)
                if (S2 <= 256 * W && S2 >= 8 * W) S = S2;
            }
        } else {
            // decimate16 and up: with four and more stages per step a single wave keeps its SIMD as busy as three do
            // (tools/sweep_span.sh, tools/bench_streams.sh), so the spans can be long and the warm-up small (3 % at 32 Ki
            // samples and L = 4 against the 9 % of a three-waves-per-SIMD round).  One wave per SIMD: 31 workgroups per XCD
            // (992 waves; with all 32 CUs of an XCD taken -- 1016 waves -- the launch is 3 % slower, with 1056 it takes
            // half as long again: the launch lasts as long as its fullest CU), the spans as long as that allows, sized
            // from the wave count so that the VALU tail stays short.  Banks too big for that (spans beyond the limit of
            // the planner): spans of 32 Ki samples, the waves are dealt dynamically over many rounds.
            const size_t SL = 32768 > 8 * W ? 32768 : 8 * W;
            // (ring == 2, decimate16 only: the two-waves-per-SIMD experiment -- 62 workgroups per XCD, spans half as long)
            const size_t wps1 = (mf_dma_applies(log2decim) && ring == 2 ? 2 * waves1 : waves1) / (size_t)nstreams;
            S = SL;
            if (wps1 >= 1) {
                size_t S1 = n / (8 * wps1) / W * W;
                if (S1 == 0 || n / (8 * S1) > wps1) S1 += W; // (rounding down must not add a wave)
                // long periods (decimate32 / 64: W = 2048 / 4096) make that rounding coarse: one period less per span and a few
                // waves more than 31 CUs per XCD hold -- they land on the 32nd -- costs ~3 %, a period more of span + warm-up per
                // wave costs W / (S + W) (profiles/r04_decim_paths.txt: decimate64 0.2751 -> 0.2533 ms, decimate32 0.2513 -> 0.2447)
                if (S1 > 8 * W) {
                    const size_t S0 = S1 - W, wps0 = n / (8 * S0);
                    if (wps0 * (size_t)nstreams <= (size_t)4 * (size_t)n_cu && (S0 + W) * 105 < (S1 + W) * 100) S1 = S0;
                }
                if (S1 <= 256 * W) S = S1;
            }
        }
        // small calls: short spans (the launch lasts (W + S) / 32 steps of ~0.2 us whatever the size of the call)
        const size_t smin = (log2decim <= 3 ? 8 : 2) * W;
        if (S < smin) S = smin;
        if (S > 256 * W) S = 256 * W;
    }
    size_t wps = n / (8 * S);
    if (wps == 0 || wps > 0x7fffffffu / (size_t)nstreams) return false;
    if (8 * S * 4 >= 0xffffffffu) return false;   // lane offsets inside a wave are 32 bits
    size_t tail_start = head + wps * 8 * S;
    // the register-ring waves read up to 8 steps (256 samples) past their last span (the LDS-DMA ring clamps its run-ahead)
    if (n_used - tail_start < MF_READ_AHEAD) {
        if (--wps == 0) return false;
        tail_start = head + wps * 8 * S;
    }
    const size_t tail = n_used - tail_start;
    size_t ntail = (tail + MF_TAIL_SEG - 1) / MF_TAIL_SEG;
    if (ntail == 0) ntail = 1;                    // the (possibly empty) last piece stores the bank state
    p->head = head;
    p->span = S;
    p->wps = (int)wps;
    p->tail_start = tail_start;
    p->tail_seg = MF_TAIL_SEG;
    p->npieces = 1 + (int)ntail;
    mf_deal_pieces(log2decim, S, nstreams * p->npieces, (int)(((size_t)nstreams * wps + 3) / 4), n_cu, p);
    return true;
}

// ---- K1mr: the matrix-core launch of a ragged call.  The streams share the span, the head and the piece length -- those the
// uniform planner picks for the mean stream, so equal counts get the uniform launch's geometry; each has its own count of wave
// groups and pieces.  Reads Row::n_used; writes the stream's matrix-core waves mf_w0 .. mf_w0 + mf_wps - 1, its pieces mf_p0 ..
// mf_p0 + mf_np - 1, mf_head and mf_tail_start (RaggedRow, sdrhip_internal.h, says what the kernel makes of them).  In *p: wps = the
// launch's matrix-core waves, npieces = its pieces, tail_start = 0.  false when no stream is long enough for a span.
template <class Row>
inline bool plan_decimate_mfma_ragged(int log2decim, int fcpos, Row *rows, int nstreams, size_t span_override, int n_cu, int ring, MfPlan *p)
{
    size_t total = 0;
    for (int s = 0; s < nstreams; ++s) total += (size_t)rows[s].n_used;
    const int L = log2decim;
    const size_t mean = total / (size_t)nstreams / ((size_t)1 << L) * ((size_t)1 << L);
    MfPlan u;
    if (!plan_decimate_mfma(L, fcpos, mean, nstreams, span_override, n_cu, ring, &u)) return false;
    const size_t S = u.span, head = u.head, seg = u.tail_seg;
    long long waves = 0, pieces = 0;
    for (int s = 0; s < nstreams; ++s) {
        Row &r = rows[s];
        const size_t n = (size_t)r.n_used;
        size_t wps = n > head ? (n - head) / (8 * S) : 0;
        size_t tail_start = head + wps * 8 * S;
        if (wps && n - tail_start < MF_READ_AHEAD) { --wps; tail_start = head + wps * 8 * S; } // (the register ring's read-ahead)
        size_t h = head;
        if (!wps) { h = n < seg ? n : seg; tail_start = h; } // (no span: pieces alone, the first one from the state)
        const size_t tail = n - tail_start;
        const size_t np = 1 + (tail + seg - 1) / seg;
        r.mf_w0 = (int)waves; r.mf_wps = (int)wps;
        r.mf_p0 = (int)pieces; r.mf_np = (int)np;
        r.mf_head = h; r.mf_tail_start = tail_start;
        waves += (long long)wps;
        pieces += (long long)np;
        if (waves > 0x7fffffff || pieces > 0x7fffffff) return false;
    }
    if (waves == 0) return false;
    p->head = head; p->span = S; p->tail_seg = seg; p->tail_start = 0;
    p->wps = (int)waves; p->npieces = (int)pieces;
    mf_deal_pieces(L, S, (int)pieces, (int)((waves + 3) / 4), n_cu, p);
    return true;
}

// ---- what ragged_prepare decides for a ragged call and decimate_ragged_device launches
struct RaggedPlan {
    int nsub, grid; // K1r: passes per segment, workgroups
    bool mfma;      // K1mr was planned: `mf` and `ring` hold
    int ring;       // LDS-DMA ring depth of its decimate16 kernel (3 or 4)
    MfPlan mf;
};

} // namespace sdrhip
