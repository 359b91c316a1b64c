// decim_plan_test.cpp -- the decimator planners and the path rule (sdrdaemon_amd/csrc/decim_plan.h)
//  (a) against a transcription of the code they replaced: plan_decimate (decim_kernels.hip), plan_decimate_mfma and
//      plan_decimate_mfma_ragged (decim_mfma.hip) over DecimArgs / RaggedRow, the K1r loop of ragged_prepare and the three copies of
//      the path rule (decimate_device, decimate_mfma_applies, ragged_prepare in sdrhip.cpp).  Every output field must agree, and
//      `false` with `false`;
//  (b) against what the kernels rely on without checking, read off the plan alone: the head, the wave groups and the pieces cover
//      every stream exactly once, the register ring's read-ahead stays inside the stream, offsets and totals fit their types, and
//      the kernels' dealing rule hands every piece to exactly one workgroup and every workgroup a piece.
// Prints counters for tests/test_decim_plan.py and refuses to say OK unless every case it is there for was reached.
// Stand-alone: g++ -std=c++11, no library, no GPU.
#include "decim_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdrhip;

namespace {
int failures = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (failures++ < 20) { printf("MISMATCH %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                            \
    } while (0)

// ------------------------------------------------------------------------------------------------ the model: the code as it was
struct MArgs { // the fields of DecimArgs the planners touched
    size_t mf_head, mf_span, mf_tail_start, mf_tail_seg;
    int mf_wps, mf_npieces;
    int mf_piece_wgs, mf_piece_early, mf_piece_share;
    int mf_ring;
};
struct MRow { // ... and of RaggedRow
    uint64_t n_raw, n_used, n_dec;
    int seg0;
    int mf_w0, mf_wps, mf_p0, mf_np;
    uint64_t mf_head, mf_tail_start;
};
struct MOpt { int decim_path; size_t mfma_span, mfma_min; int mfma_ring; }; // CtxOptions
const int M_P0 = 2048;
bool m_mf_dma_applies(int ns) { return ns == 4; }

void m_plan_decimate(int log2decim, int fcpos, size_t n_used, int nstreams, int *nsub_per_seg, int *nseg) // decim_kernels.hip
{
    const bool cen = (fcpos == 2);
    const size_t praw = cen ? (size_t)M_P0 : (size_t)M_P0 * 4;
    size_t npass = (n_used + praw - 1) / praw;
    if (npass == 0) npass = 1;
    const int ns = cen ? log2decim : log2decim - 2;
    size_t period = (size_t)1 << (ns > 2 ? ns - 2 : 0);
    size_t per = period < 32 ? 32 : period;
    while (per > period && ((npass + per - 1) / per) * (size_t)nstreams < 2048) per >>= 1;
    while (per > 1 && ((npass + per - 1) / per) * (size_t)nstreams < 256) per >>= 1;
    const size_t wraw = (size_t)64 << log2decim;
    while (per * praw < wraw) per <<= 1;
    *nsub_per_seg = (int)per;
    *nseg = (int)((npass + per - 1) / per);
}

bool m_plan_decimate_mfma(int log2decim, int fcpos, size_t n_used, int nstreams, size_t span_override, int n_cu, MArgs *a) // decim_mfma.hip
{
    const int nxcd = n_cu >= 64 && n_cu % 8 == 0 ? 8 : 1;
    const size_t waves1 = (size_t)4 * (size_t)(n_cu > nxcd ? n_cu - nxcd : n_cu);
    const size_t waves3 = 3 * waves1 - waves1 / 13;
    if (fcpos != 2 || log2decim < 2 || log2decim > 6) return false;
    const size_t W = (size_t)64 << log2decim;
    const size_t head = W > 2048 ? W : 2048;
    if (n_used <= head) return false;
    const size_t n = n_used - head;
    size_t S;
    if (span_override) {
        S = (span_override + W - 1) / W * W;
    } else {
        const size_t total = n * (size_t)nstreams;
        if (log2decim <= 3) {
            S = (total / (waves3 * 8) + W - 1) / W * W;
            const size_t wps2 = 2 * waves1 / (size_t)nstreams;
            if (wps2 >= 1) {
                size_t S2 = n / (8 * wps2) / W * W;
                if (S2 == 0 || n / (8 * S2) > wps2) S2 += W;
                if (S2 <= 256 * W && S2 >= 8 * W) S = S2;
            }
        } else {
            const size_t SL = 32768 > 8 * W ? 32768 : 8 * W;
            const size_t wps1 = (m_mf_dma_applies(log2decim) && a->mf_ring == 2 ? 2 * waves1 : waves1) / (size_t)nstreams;
            S = SL;
            if (wps1 >= 1) {
                size_t S1 = n / (8 * wps1) / W * W;
                if (S1 == 0 || n / (8 * S1) > wps1) S1 += W;
                if (S1 > 8 * W) {
                    const size_t S0 = S1 - W, wps0 = n / (8 * S0);
                    if (wps0 * (size_t)nstreams <= (size_t)4 * (size_t)n_cu && (S0 + W) * 105 < (S1 + W) * 100) S1 = S0;
                }
                if (S1 <= 256 * W) S = S1;
            }
        }
        const size_t smin = (log2decim <= 3 ? 8 : 2) * W;
        if (S < smin) S = smin;
        if (S > 256 * W) S = 256 * W;
    }
    size_t wps = n / (8 * S);
    if (wps == 0 || wps > 0x7fffffffu / (size_t)nstreams) return false;
    if (8 * S * 4 >= 0xffffffffu) return false;
    size_t tail_start = head + wps * 8 * S;
    if (n_used - tail_start < 256u) {
        if (--wps == 0) return false;
        tail_start = head + wps * 8 * S;
    }
    const size_t tail = n_used - tail_start;
    const size_t seg = 16384;
    size_t ntail = (tail + seg - 1) / seg;
    if (ntail == 0) ntail = 1;
    a->mf_head = head;
    a->mf_span = S;
    a->mf_wps = (int)wps;
    a->mf_tail_start = tail_start;
    a->mf_tail_seg = seg;
    a->mf_npieces = 1 + (int)ntail;
    {
        const int items = nstreams * a->mf_npieces, nmf = (int)(((size_t)nstreams * wps + 3) / 4);
        a->mf_piece_early = 0; a->mf_piece_share = 0;
        if (m_mf_dma_applies(log2decim) && n_cu > nmf) {
            int early = n_cu - nmf;
            if (early > items) early = items;
            int share = (int)((W + S) / 6720);
            if (share < 3) share = 3;
            if (share > (items + early - 1) / early) share = (items + early - 1) / early;
            a->mf_piece_early = early; a->mf_piece_share = share;
        }
        const int rest = items - a->mf_piece_early * a->mf_piece_share;
        a->mf_piece_wgs = a->mf_piece_early + (rest > 0 ? rest : 0);
    }
    return true;
}

bool m_plan_decimate_mfma_ragged(int log2decim, int fcpos, MRow *rows, int nstreams, size_t span_override, int n_cu, MArgs *a) // decim_mfma.hip
{
    size_t total = 0;
    for (int s = 0; s < nstreams; ++s) total += (size_t)rows[s].n_used;
    const int L = log2decim;
    const size_t mean = total / (size_t)nstreams / ((size_t)1 << L) * ((size_t)1 << L);
    MArgs u = *a;
    if (!m_plan_decimate_mfma(L, fcpos, mean, nstreams, span_override, n_cu, &u)) return false;
    const size_t S = u.mf_span, head = u.mf_head, seg = u.mf_tail_seg;
    long long waves = 0, pieces = 0;
    for (int s = 0; s < nstreams; ++s) {
        MRow &r = rows[s];
        const size_t n = (size_t)r.n_used;
        size_t wps = n > head ? (n - head) / (8 * S) : 0;
        size_t tail_start = head + wps * 8 * S;
        if (wps && n - tail_start < 256u) { --wps; tail_start = head + wps * 8 * S; }
        size_t h = head;
        if (!wps) { h = n < seg ? n : seg; tail_start = h; }
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
    a->mf_head = head; a->mf_span = S; a->mf_tail_seg = seg; a->mf_tail_start = 0;
    a->mf_wps = (int)waves; a->mf_npieces = (int)pieces;
    {
        const int items = (int)pieces, nmf = (int)((waves + 3) / 4);
        const size_t W = (size_t)64 << L;
        a->mf_piece_early = 0; a->mf_piece_share = 0;
        if (m_mf_dma_applies(L) && n_cu > nmf) {
            int early = n_cu - nmf;
            if (early > items) early = items;
            int share = (int)((W + S) / 6720);
            if (share < 3) share = 3;
            if (share > (items + early - 1) / early) share = (items + early - 1) / early;
            a->mf_piece_early = early; a->mf_piece_share = share;
        }
        const int rest = items - a->mf_piece_early * a->mf_piece_share;
        a->mf_piece_wgs = a->mf_piece_early + (rest > 0 ? rest : 0);
    }
    return true;
}

size_t m_mfma_min_samples(const MOpt &o, int log2decim) { return o.mfma_min << (log2decim > 3 ? log2decim - 3 : 0); } // sdrhip.cpp

// the path rule as decimate_device had it (frame mode aside): `a` zeroed, mf_ring set, then the rule and the planner
bool m_device_use_mfma(const MOpt &env, int L, int fcpos, size_t n_used, int nstreams, int n_cu, bool coresident, MArgs *a)
{
    memset(a, 0, sizeof(*a));
    bool use_mfma = false;
    a->mf_ring = coresident ? 3 : env.mfma_ring;
    if (env.decim_path != DECIM_PATH_VALU && (env.decim_path == DECIM_PATH_MFMA || n_used * (size_t)nstreams >= m_mfma_min_samples(env, L)))
        use_mfma = m_plan_decimate_mfma(L, fcpos, n_used, nstreams, env.mfma_span, n_cu, a);
    return use_mfma;
}
// ... as decimate_mfma_applies had it
bool m_applies(const MOpt &env, int log2decim, int fcpos, size_t n_in, int nstreams, int n_cu)
{
    const size_t n_used = (n_in >> log2decim) << log2decim;
    if (env.decim_path == DECIM_PATH_VALU || (env.decim_path != DECIM_PATH_MFMA && n_used * (size_t)nstreams < m_mfma_min_samples(env, log2decim))) return false;
    MArgs tmp;
    memset(&tmp, 0, sizeof(tmp));
    tmp.mf_ring = env.mfma_ring;
    return m_plan_decimate_mfma(log2decim, fcpos, n_used, nstreams, env.mfma_span, n_cu, &tmp);
}
// ... and ragged_prepare in front of its upload: the rows' counts, K1r's geometry, the rule and K1mr's plan (the handle's r_* fields)
struct MRagged { int r_nsub, r_grid; bool r_mfma; MArgs r_mf; };
bool m_ragged_prepare(const MOpt &env, int log2decim, int fcpos, const size_t *n_in, MRow *rows, int S, int n_cu, MRagged *d)
{
    const unsigned L = (unsigned)log2decim;
    size_t total = 0;
    for (int s = 0; s < S; ++s) {
        rows[s].n_raw = n_in[s];
        rows[s].n_dec = n_in[s] >> L;
        rows[s].n_used = (uint64_t)(n_in[s] >> L) << L;
        total += (size_t)rows[s].n_used;
    }
    const bool cen = fcpos == 2;
    d->r_nsub = 0; d->r_grid = 0;
    if (L >= 1 && (cen || L >= 3)) {
        int nseg = 0;
        m_plan_decimate((int)L, fcpos, (total + (size_t)S - 1) / (size_t)S, S, &d->r_nsub, &nseg);
        const size_t seg_raw = (size_t)d->r_nsub * (size_t)(cen ? 2048 : 8192);
        size_t acc = 0;
        for (int s = 0; s < S; ++s) {
            rows[s].seg0 = (int)acc;
            acc += rows[s].n_used ? (size_t)((rows[s].n_used + seg_raw - 1) / seg_raw) : 1;
        }
        if (acc > 0x7fffffffu) return false; // fail(SDRHIP_EINVAL, "ragged call: too many segments")
        d->r_grid = (int)acc;
    }
    d->r_mfma = false;
    if (cen && L >= 2 && env.decim_path != DECIM_PATH_VALU && (env.decim_path == DECIM_PATH_MFMA || total >= m_mfma_min_samples(env, (int)L))) {
        memset(&d->r_mf, 0, sizeof(d->r_mf));
        d->r_mf.mf_ring = env.mfma_ring == 3 ? 3 : 4;
        d->r_mfma = m_plan_decimate_mfma_ragged((int)L, fcpos, rows, S, env.mfma_span, n_cu, &d->r_mf);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ the counters
struct Counters {
    long uniform_accepted, uniform_refused, wave_dropped, one_group_left, fixpoints, lane_limit, early_dealt, dealings_simulated, dealings_large;
    long rule_admitted, rule_refused_by_size, rule_refused_by_planner;
    long ragged_accepted, ragged_refused, streams_zero, streams_short, streams_one_group, streams_dropped_wave, equal_scripts, k1r_grids, k1r_none;
} cnt;

// ------------------------------------------------------------------------------------------------ (b) the invariants
// the pieces [tail_start, n_used) as the kernels cut them (decim_mfma.hip): piece i >= 1 starts at tail_start + (i - 1) * seg and ends a
// segment later, at n_used when that is sooner or when it is the last one
void check_pieces(size_t tail_start, size_t seg, int np, size_t n_used, const char *what)
{
    size_t pos = tail_start;
    for (int piece = 1; piece < np; ++piece) {
        const size_t s0 = tail_start + (size_t)(piece - 1) * seg;
        size_t s1 = s0 + seg;
        if (s1 > n_used || piece == np - 1) s1 = n_used;
        CHECK(s0 == pos && s0 <= n_used && s1 - s0 <= seg, "%s: piece %d of %d [%zu, %zu) after %zu, n_used %zu", what, piece, np, s0, s1, pos, n_used);
        if (s0 > n_used) return;
        pos = s1;
    }
    CHECK(pos == n_used, "%s: the pieces end at %zu of %zu", what, pos, n_used);
}

// the kernels' dealing rule (decim_mfma_kernel, decim_mfma_ragged_kernel): early workgroup j takes items j + k * early for k < share
// while the item is below both early * share and items; workgroup j >= early takes early * share + (j - early)
std::vector<unsigned char> g_hits;
void check_dealing(const MfPlan &p, long long items_ll, const char *what)
{
    CHECK(items_ll >= 1 && items_ll <= 0x7fffffff, "%s: %lld pieces", what, items_ll);
    if (items_ll < 1 || items_ll > 0x7fffffff) return;
    const int items = (int)items_ll;
    CHECK(p.piece_wgs >= 1 && p.piece_early >= 0 && p.piece_early <= p.piece_wgs && p.piece_share >= 0, "%s: wgs %d early %d share %d", what, p.piece_wgs, p.piece_early, p.piece_share);
    const long long nearly = (long long)p.piece_early * p.piece_share;
    CHECK(nearly <= 0x7fffffff, "%s: early * share", what);
    if (p.piece_early) ++cnt.early_dealt;
    if (items > (1 << 16)) {
        // (banks of tens of thousands of streams: the same rule in closed form -- the early part covers [0, min(nearly, items)) when
        // every early workgroup's first item is inside it, the single-piece workgroups the rest one by one)
        ++cnt.dealings_large;
        const long long early_part = nearly < items ? nearly : items;
        CHECK(p.piece_early <= early_part || p.piece_early == 0, "%s: an early workgroup without a piece", what);
        CHECK(early_part + (p.piece_wgs - p.piece_early) == items, "%s: %d workgroups (%d early x %d) for %d pieces", what, p.piece_wgs, p.piece_early, p.piece_share, items);
        return;
    }
    ++cnt.dealings_simulated;
    if (g_hits.size() < (size_t)items) g_hits.resize((size_t)items);
    memset(g_hits.data(), 0, (size_t)items);
    for (int j = 0; j < p.piece_wgs; ++j) {
        const int nmine = j < p.piece_early ? p.piece_share : 1;
        int got = 0;
        for (int k = 0; k < nmine; ++k) {
            const long long lx = j < p.piece_early ? j + (long long)k * p.piece_early : nearly + (j - p.piece_early);
            if (lx >= items || (j < p.piece_early && lx >= nearly)) break;
            ++g_hits[(size_t)lx];
            ++got;
        }
        CHECK(got >= 1, "%s: workgroup %d of %d gets no piece (early %d share %d items %d)", what, j, p.piece_wgs, p.piece_early, p.piece_share, items);
    }
    for (int i = 0; i < items; ++i) CHECK(g_hits[(size_t)i] == 1, "%s: piece %d of %d dealt %d times (wgs %d early %d share %d)", what, i, items, (int)g_hits[(size_t)i], p.piece_wgs, p.piece_early, p.piece_share);
}

void check_uniform_plan(const MfPlan &p, int L, size_t n_used, int nstreams)
{
    (void)L;
    CHECK(p.head <= n_used && p.wps >= 1 && p.span >= 1, "head %zu wps %d span %zu", p.head, p.wps, p.span);
    CHECK(p.head + (size_t)p.wps * 8 * p.span == p.tail_start && p.tail_start <= n_used, "head %zu + %d x 8 x %zu != tail_start %zu (n_used %zu)", p.head, p.wps, p.span, p.tail_start, n_used);
    CHECK(n_used - p.tail_start >= MF_READ_AHEAD, "tail of %zu samples behind the last span", n_used - p.tail_start);
    CHECK((unsigned long long)p.span * 8 * 4 < (1ull << 32), "span %zu", p.span);
    CHECK((long long)nstreams * p.wps <= 0x7fffffff && (long long)nstreams * p.npieces <= 0x7fffffff, "totals: %d x (%d, %d)", nstreams, p.wps, p.npieces);
    CHECK(p.npieces >= 2 && p.tail_seg >= 1, "npieces %d", p.npieces);
    check_pieces(p.tail_start, p.tail_seg, p.npieces, n_used, "uniform");
    check_dealing(p, (long long)nstreams * p.npieces, "uniform");
}

// the test's own row: the names the planners write through, nothing of the library's
struct TRow {
    uint64_t n_used;
    int seg0;
    int mf_w0, mf_wps, mf_p0, mf_np;
    uint64_t mf_head, mf_tail_start;
};

void check_ragged_plan(const MfPlan &p, const std::vector<TRow> &rows)
{
    long long waves = 0, pieces = 0;
    CHECK((unsigned long long)p.span * 8 * 4 < (1ull << 32) && p.span >= 1 && p.tail_seg >= 1, "span %zu", p.span);
    for (size_t s = 0; s < rows.size(); ++s) {
        const TRow &r = rows[s];
        const size_t n = (size_t)r.n_used;
        CHECK(r.mf_w0 == waves && r.mf_p0 == pieces, "stream %zu: first wave %d / piece %d, sums %lld / %lld", s, r.mf_w0, r.mf_p0, waves, pieces);
        CHECK(r.mf_wps >= 0 && r.mf_np >= 1, "stream %zu: wps %d np %d", s, r.mf_wps, r.mf_np);
        CHECK(r.mf_head <= n && r.mf_head + (uint64_t)r.mf_wps * 8 * p.span == r.mf_tail_start && r.mf_tail_start <= n, "stream %zu: head %llu wps %d tail_start %llu of %zu", s,
              (unsigned long long)r.mf_head, r.mf_wps, (unsigned long long)r.mf_tail_start, n);
        if (r.mf_wps > 0) {
            CHECK(r.mf_head == p.head, "stream %zu: its waves start at %llu, the launch's at %zu", s, (unsigned long long)r.mf_head, p.head); // (mf_wave starts at a.mf_head)
            CHECK(n - r.mf_tail_start >= MF_READ_AHEAD, "stream %zu: tail of %llu samples", s, (unsigned long long)(n - r.mf_tail_start));
        }
        if (r.mf_np == 1) CHECK(r.mf_wps == 0 && r.mf_head == n, "stream %zu: one piece for %zu samples, head %llu", s, n, (unsigned long long)r.mf_head); // (piece 0 from the state to the state)
        check_pieces((size_t)r.mf_tail_start, p.tail_seg, r.mf_np, r.mf_np == 1 ? (size_t)r.mf_tail_start : n, "ragged");
        waves += r.mf_wps;
        pieces += r.mf_np;
    }
    CHECK(waves == p.wps && pieces == p.npieces && waves >= 1, "totals %lld / %lld against %d / %d", waves, pieces, p.wps, p.npieces);
    check_dealing(p, pieces, "ragged");
}

void check_k1r(int L, int fcpos, const std::vector<TRow> &rows, int nsub, int grid)
{
    const size_t seg_raw = (size_t)nsub * decim_pass_raw(fcpos == 2);
    CHECK(nsub >= 1 && seg_raw >= ((size_t)64 << L), "segment of %d passes", nsub); // (a segment's warm-up starts inside the stream)
    for (size_t s = 0; s < rows.size(); ++s) {
        const long long next = s + 1 < rows.size() ? rows[s + 1].seg0 : grid;
        const long long mine = next - rows[s].seg0;
        CHECK(rows[s].seg0 >= 0 && mine >= 1, "stream %zu: segments %d .. %lld", s, rows[s].seg0, next);
        CHECK((unsigned long long)mine * seg_raw >= rows[s].n_used, "stream %zu: %lld segments of %zu for %llu samples", s, mine, seg_raw, (unsigned long long)rows[s].n_used);
    }
    CHECK(rows[0].seg0 == 0, "first segment %d", rows[0].seg0);
}

// ------------------------------------------------------------------------------------------------ (a) new against old
bool same_plan(const MfPlan &p, const MArgs &a)
{
    return p.head == a.mf_head && p.span == a.mf_span && p.tail_start == a.mf_tail_start && p.tail_seg == a.mf_tail_seg && p.wps == a.mf_wps &&
           p.npieces == a.mf_npieces && p.piece_wgs == a.mf_piece_wgs && p.piece_early == a.mf_piece_early && p.piece_share == a.mf_piece_share;
}

// one uniform call: planner against planner, the plan against the invariants; returns the span (0: refused)
size_t uniform_case(int L, int fcpos, size_t n_used, int nstreams, size_t span_override, int n_cu, int ring)
{
    int nsub = -1, nseg = -1, m_nsub = -2, m_nseg = -2;
    plan_decimate(L, fcpos, n_used, nstreams, &nsub, &nseg);
    m_plan_decimate(L, fcpos, n_used, nstreams, &m_nsub, &m_nseg);
    CHECK(nsub == m_nsub && nseg == m_nseg, "plan_decimate L %d fc %d n %zu S %d: %d / %d against %d / %d", L, fcpos, n_used, nstreams, nsub, nseg, m_nsub, m_nseg);
    // (K1: the segments cover the stream, and a later segment's warm-up starts inside it)
    CHECK(nsub >= 1 && nseg >= 1 && (size_t)nseg * nsub * decim_pass_raw(fcpos == 2) >= n_used && (size_t)nsub * decim_pass_raw(fcpos == 2) >= ((size_t)64 << L),
          "plan_decimate L %d fc %d n %zu S %d: %d x %d", L, fcpos, n_used, nstreams, nseg, nsub);

    MArgs a;
    memset(&a, 0, sizeof(a));
    a.mf_ring = ring;
    MfPlan p;
    const bool m_ok = m_plan_decimate_mfma(L, fcpos, n_used, nstreams, span_override, n_cu, &a);
    const bool ok = plan_decimate_mfma(L, fcpos, n_used, nstreams, span_override, n_cu, ring, &p);
    CHECK(ok == m_ok && (!ok || same_plan(p, a)), "plan_decimate_mfma L %d fc %d n %zu S %d span %zu cu %d ring %d: %d against %d", L, fcpos, n_used, nstreams, span_override, n_cu, ring,
          (int)ok, (int)m_ok);
    if (!ok) { ++cnt.uniform_refused; return 0; }
    ++cnt.uniform_accepted;
    check_uniform_plan(p, L, n_used, nstreams);
    const size_t groups = (n_used - p.head) / (8 * p.span);
    if (groups == (size_t)p.wps + 1) ++cnt.wave_dropped; // (a whole group more would fit: it went to the tail for the read-ahead's sake)
    if (p.wps == 1) ++cnt.one_group_left;
    return p.span;
}

// the three copies of the path rule against the one predicate in front of the planner
void rule_case(const MOpt &env, int L, int fcpos, size_t n_in, int nstreams, int n_cu, bool coresident)
{
    const size_t n_used = (n_in >> L) << L;
    MArgs a;
    const bool m_use = m_device_use_mfma(env, L, fcpos, n_used, nstreams, n_cu, coresident, &a);
    const int ring = coresident ? 3 : env.mfma_ring;
    MfPlan p;
    const bool admitted = mfma_admitted(env.decim_path, env.mfma_min, L, n_used * (size_t)nstreams);
    const bool use = admitted && plan_decimate_mfma(L, fcpos, n_used, nstreams, env.mfma_span, n_cu, ring, &p);
    CHECK(use == m_use && (!use || same_plan(p, a)), "decimate_device's rule: path %d min %zu L %d fc %d n %zu S %d: %d against %d", env.decim_path, env.mfma_min, L, fcpos, n_used, nstreams,
          (int)use, (int)m_use);
    MfPlan q;
    const bool applies = mfma_admitted(env.decim_path, env.mfma_min, L, n_used * (size_t)nstreams) && plan_decimate_mfma(L, fcpos, n_used, nstreams, env.mfma_span, n_cu, env.mfma_ring, &q);
    const bool m_app = m_applies(env, L, fcpos, n_in, nstreams, n_cu);
    CHECK(applies == m_app, "decimate_mfma_applies' rule: path %d min %zu L %d fc %d n %zu S %d: %d against %d", env.decim_path, env.mfma_min, L, fcpos, n_in, nstreams, (int)applies, (int)m_app);
    CHECK(mfma_min_samples(env.mfma_min, L) == m_mfma_min_samples(env, L), "mfma_min_samples L %d", L);
    if (use) ++cnt.rule_admitted;
    else if (!admitted) ++cnt.rule_refused_by_size;
    else ++cnt.rule_refused_by_planner;
}

unsigned long long g_seed = 1;
unsigned rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_seed >> 33); }

// one ragged call: ragged_prepare as it was against the three functions it is made of now
void ragged_case(const MOpt &env, int L, int fcpos, const std::vector<size_t> &n_in, int n_cu, bool equal_counts)
{
    const int S = (int)n_in.size();
    std::vector<MRow> mrows((size_t)S);
    std::vector<TRow> rows((size_t)S);
    memset(mrows.data(), 0, mrows.size() * sizeof(MRow));
    memset(rows.data(), 0, rows.size() * sizeof(TRow));
    MRagged m;
    memset(&m, 0, sizeof(m));
    const bool m_ok = m_ragged_prepare(env, L, fcpos, n_in.data(), mrows.data(), S, n_cu, &m);

    size_t total = 0;
    for (int s = 0; s < S; ++s) { rows[(size_t)s].n_used = (uint64_t)(n_in[(size_t)s] >> L) << L; total += (size_t)rows[(size_t)s].n_used; }
    RaggedPlan plan;
    memset(&plan, 0, sizeof(plan));
    const bool ok = plan_decimate_ragged(L, fcpos, rows.data(), S, total, &plan.nsub, &plan.grid);
    CHECK(ok == m_ok, "K1r L %d fc %d S %d: %d against %d", L, fcpos, S, (int)ok, (int)m_ok);
    if (!ok || !m_ok) return;
    CHECK(plan.nsub == m.r_nsub && plan.grid == m.r_grid, "K1r L %d fc %d S %d: %d / %d against %d / %d", L, fcpos, S, plan.nsub, plan.grid, m.r_nsub, m.r_grid);
    for (int s = 0; s < S; ++s) CHECK(rows[(size_t)s].seg0 == mrows[(size_t)s].seg0, "K1r stream %d: seg0 %d against %d", s, rows[(size_t)s].seg0, mrows[(size_t)s].seg0);
    if (plan.grid) { ++cnt.k1r_grids; check_k1r(L, fcpos, rows, plan.nsub, plan.grid); }
    else { ++cnt.k1r_none; CHECK(L == 0 || (fcpos != 2 && L <= 2), "no K1r grid at L %d fc %d", L, fcpos); }

    plan.ring = env.mfma_ring == 3 ? 3 : 4;
    plan.mfma = mfma_admitted(env.decim_path, env.mfma_min, L, total) && plan_decimate_mfma_ragged(L, fcpos, rows.data(), S, env.mfma_span, n_cu, plan.ring, &plan.mf);
    CHECK(plan.mfma == m.r_mfma, "K1mr path %d min %zu L %d fc %d S %d total %zu: %d against %d", env.decim_path, env.mfma_min, L, fcpos, S, total, (int)plan.mfma, (int)m.r_mfma);
    // (the rows: whatever either planner left in them, accepted or not -- the table goes up either way)
    for (int s = 0; s < S; ++s) {
        const TRow &r = rows[(size_t)s];
        const MRow &q = mrows[(size_t)s];
        CHECK(r.n_used == q.n_used && r.mf_w0 == q.mf_w0 && r.mf_wps == q.mf_wps && r.mf_p0 == q.mf_p0 && r.mf_np == q.mf_np && r.mf_head == q.mf_head && r.mf_tail_start == q.mf_tail_start,
              "K1mr stream %d of %d (L %d): w0 %d wps %d p0 %d np %d against %d %d %d %d", s, S, L, r.mf_w0, r.mf_wps, r.mf_p0, r.mf_np, q.mf_w0, q.mf_wps, q.mf_p0, q.mf_np);
    }
    if (!plan.mfma) { ++cnt.ragged_refused; return; }
    ++cnt.ragged_accepted;
    CHECK(same_plan(plan.mf, m.r_mf) && plan.ring == m.r_mf.mf_ring, "K1mr plan L %d S %d", L, S);
    check_ragged_plan(plan.mf, rows);
    for (int s = 0; s < S; ++s) {
        const TRow &r = rows[(size_t)s];
        if (r.n_used == 0) ++cnt.streams_zero;
        else if (r.n_used <= plan.mf.head) ++cnt.streams_short;
        if (r.mf_wps == 1) ++cnt.streams_one_group;
        if (r.n_used > plan.mf.head && (r.n_used - plan.mf.head) / (8 * plan.mf.span) == (uint64_t)r.mf_wps + 1) ++cnt.streams_dropped_wave;
    }
    if (equal_counts) {
        // equal counts get the uniform launch's geometry (tests/test_gpu_rx_ragged.py relies on it): its span and head, and with them
        // every stream's wave groups and pieces
        MfPlan u;
        const bool uok = plan_decimate_mfma(L, fcpos, (size_t)rows[0].n_used, S, env.mfma_span, n_cu, plan.ring, &u);
        CHECK(uok, "equal counts of %llu: the ragged plan without a uniform one", (unsigned long long)rows[0].n_used);
        if (uok) {
            CHECK(u.span == plan.mf.span && u.head == plan.mf.head && u.tail_seg == plan.mf.tail_seg, "equal counts: span %zu head %zu against the uniform %zu / %zu", plan.mf.span, plan.mf.head, u.span, u.head);
            for (int s = 0; s < S; ++s)
                CHECK(rows[(size_t)s].mf_wps == u.wps && rows[(size_t)s].mf_np == u.npieces && rows[(size_t)s].mf_tail_start == u.tail_start && rows[(size_t)s].mf_head == u.head, "equal counts: stream %d", s);
            ++cnt.equal_scripts;
        }
    }
}

// the scripts of per-stream counts: 0 equal, 1 a mix with zeros and streams shorter than the head, 2 the same with every third stream at
// exactly one wave group of the span the mix got, 3 one long stream among empty ones, 4 every stream shorter than the head
void ragged_scripts(const MOpt &env, int L, int fcpos, int S, int n_cu)
{
    const size_t W = (size_t)64 << L, head = W > MF_HEAD_MIN ? W : MF_HEAD_MIN;
    const size_t base = (size_t)1 << (12 + rnd() % 11); // 2^12 .. 2^22 samples
    std::vector<size_t> n((size_t)S);
    for (int kind = 0; kind < 5; ++kind) {
        for (int s = 0; s < S; ++s) {
            size_t v = 0;
            const unsigned pick = rnd() % 8;
            switch (kind) {
            case 0: v = base + 37; break;
            case 1: case 2: v = pick == 0 ? 0 : pick == 1 ? rnd() % head : pick == 2 ? head + rnd() % 512 : base / 2 + rnd() % base; break;
            case 3: v = s == S / 2 ? 8 * base + 5 : 0; break;
            default: v = rnd() % (head + 1); break;
            }
            n[(size_t)s] = v;
        }
        if (kind == 2) {
            // the span this mix gets (the new planner's word for it: ragged_case below holds it to the old one's)
            std::vector<TRow> rows((size_t)S);
            memset(rows.data(), 0, rows.size() * sizeof(TRow));
            for (int s = 0; s < S; ++s) rows[(size_t)s].n_used = (uint64_t)(n[(size_t)s] >> L) << L;
            MfPlan p;
            if (plan_decimate_mfma_ragged(L, fcpos, rows.data(), S, env.mfma_span, n_cu, env.mfma_ring == 3 ? 3 : 4, &p))
                for (int s = 0; s < S; s += 3) n[(size_t)s] = p.head + 8 * p.span + MF_READ_AHEAD + (s % 2 ? W : 0);
        }
        ragged_case(env, L, fcpos, n, n_cu, kind == 0);
    }
}
} // namespace

int main()
{
    static const int NSTREAMS[] = {1, 2, 3, 7, 64, 256, 1000, 65535};
    static const int NCU[] = {1, 8, 64, 256, 304};
    static const int RING[] = {2, 3, 4};

    // ---- the uniform planners
    for (int L = 1; L <= 6; ++L)
        for (int fcpos = 0; fcpos <= 2; ++fcpos)
            for (int nstreams : NSTREAMS)
                for (int n_cu : NCU)
                    for (int ring : RING) {
                        const size_t W = (size_t)64 << L, one = (size_t)1 << L, head = W > MF_HEAD_MIN ? W : MF_HEAD_MIN;
                        const size_t overrides[] = {0, W, 3 * W + 1};
                        for (size_t span_override : overrides) {
                            const size_t fixed[] = {0, one, head - one, head, head + one, (size_t)1 << 22, (size_t)1 << 28};
                            for (size_t n_used : fixed) uniform_case(L, fcpos, n_used, nstreams, span_override, n_cu, ring);
                            // head + 8 S k + d, S = the span the planner itself picks there: start from the span of a nearby size and
                            // follow the planner until it answers with the span the size was made of
                            static const int K[] = {1, 2, 5};
                            const long long D[] = {-(long long)one, 0, (long long)(255 / one * one), 256, 256 + (long long)one};
                            for (int k : K)
                                for (long long dd : D) {
                                    size_t S = (L <= 3 ? 8 : 2) * W, got = 0;
                                    for (int round = 0; round < 6; ++round) {
                                        const size_t n_used = (size_t)((long long)(head + 8 * S * (size_t)k) + dd);
                                        got = uniform_case(L, fcpos, n_used, nstreams, span_override, n_cu, ring);
                                        if (got == 0 || got == S) break;
                                        S = got;
                                    }
                                    if (got && got == S) ++cnt.fixpoints;
                                }
                        }
                    }
    // (the lane-offset limit needs a span of 2^27 samples, which only an override reaches, and a stream of 8 of them)
    for (int L = 2; L <= 6; ++L)
        for (int nstreams : {1, 3}) {
            MArgs a;
            memset(&a, 0, sizeof(a));
            a.mf_ring = 4;
            MfPlan p;
            const size_t n_used = ((size_t)1 << 31) + ((size_t)1 << 20), span = (size_t)1 << 27;
            const bool m_ok = m_plan_decimate_mfma(L, 2, n_used, nstreams, span, 256, &a), ok = plan_decimate_mfma(L, 2, n_used, nstreams, span, 256, 4, &p);
            CHECK(!ok && !m_ok, "a span of 2^27 samples accepted: %d / %d", (int)ok, (int)m_ok);
            CHECK(uniform_case(L, 2, n_used, nstreams, span / 2, 256, 4) == span / 2, "a span of 2^26 samples refused");
            ++cnt.lane_limit;
        }

    // ---- the path rule, three times
    {
        static const int PATHS[] = {DECIM_PATH_AUTO, DECIM_PATH_VALU, DECIM_PATH_MFMA};
        const size_t MINS[] = {0, (size_t)1 << 22, (size_t)1 << 26};
        for (int path : PATHS)
            for (size_t mfma_min : MINS)
                for (int ring : RING)
                    for (int L = 0; L <= 6; ++L)
                        for (int fcpos = 0; fcpos <= 2; ++fcpos)
                            for (int nstreams : NSTREAMS)
                                for (int n_cu : {8, 256, 304})
                                    for (int e = 10; e <= 28; e += 3) {
                                        const MOpt env = {path, e % 2 ? (size_t)0 : ((size_t)64 << L) * 3 + 1, mfma_min, ring};
                                        const size_t n_in = ((size_t)1 << e) + rnd() % 4096;
                                        rule_case(env, L, fcpos, n_in, nstreams, n_cu, (e & 4) != 0);
                                        // (at the threshold itself: the call's total one sample group below, and on it)
                                        const size_t per = mfma_min_samples(mfma_min, L) / (size_t)nstreams;
                                        if (per >= ((size_t)2 << L)) {
                                            rule_case(env, L, fcpos, per - ((size_t)1 << L), nstreams, n_cu, false);
                                            rule_case(env, L, fcpos, per + ((size_t)1 << L), nstreams, n_cu, false);
                                        }
                                    }
    }

    // ---- ragged calls: K1r's geometry, the rule and K1mr's plan
    {
        const MOpt ENVS[] = {{DECIM_PATH_AUTO, 0, (size_t)1 << 22, 4}, {DECIM_PATH_MFMA, 0, (size_t)1 << 22, 4}, {DECIM_PATH_MFMA, 0, (size_t)1 << 22, 3},
                             {DECIM_PATH_VALU, 0, (size_t)1 << 22, 4}, {DECIM_PATH_AUTO, 0, 0, 3}, {DECIM_PATH_MFMA, 1, 0, 4}, {DECIM_PATH_MFMA, 3, 0, 2}};
        for (const MOpt &e0 : ENVS)
            for (int L = 0; L <= 6; ++L)
                for (int fcpos = 0; fcpos <= 2; ++fcpos)
                    for (int nstreams : NSTREAMS)
                        for (int n_cu : NCU) {
                            if (nstreams == 65535 && n_cu != 256) continue; // (the largest bank: on the MI355X's count alone)
                            MOpt env = e0;
                            const size_t W = (size_t)64 << L;
                            env.mfma_span = e0.mfma_span == 0 ? 0 : e0.mfma_span == 1 ? W : 3 * W + 1; // span_override 0, W, 3 W + 1
                            g_seed = 1000003ull * (unsigned long long)L + 101ull * (unsigned long long)nstreams + (unsigned long long)(fcpos * 7 + n_cu);
                            ragged_scripts(env, L, fcpos, nstreams, n_cu);
                        }
    }

    printf("uniform plans accepted: %ld\nuniform plans refused: %ld\nwave groups given to the tail for the read-ahead: %ld\nplans of one wave group: %ld\n", cnt.uniform_accepted,
           cnt.uniform_refused, cnt.wave_dropped, cnt.one_group_left);
    printf("sizes on the planner's own span: %ld\nspans refused at the lane-offset limit: %ld\nplans with early piece workgroups: %ld\ndealings simulated: %ld\ndealings in closed form: %ld\n",
           cnt.fixpoints, cnt.lane_limit, cnt.early_dealt, cnt.dealings_simulated, cnt.dealings_large);
    printf("path rule admitted: %ld\npath rule refused by size: %ld\npath rule refused by the planner: %ld\n", cnt.rule_admitted, cnt.rule_refused_by_size, cnt.rule_refused_by_planner);
    printf("ragged plans accepted: %ld\nragged plans refused: %ld\nstreams at count 0: %ld\nstreams shorter than the head: %ld\nstreams of one wave group: %ld\n", cnt.ragged_accepted,
           cnt.ragged_refused, cnt.streams_zero, cnt.streams_short, cnt.streams_one_group);
    printf("streams with a wave group given to the tail: %ld\nequal-count scripts on the uniform geometry: %ld\nK1r grids: %ld\ncalls without a K1r grid: %ld\n", cnt.streams_dropped_wave,
           cnt.equal_scripts, cnt.k1r_grids, cnt.k1r_none);
    const long all[] = {cnt.uniform_accepted, cnt.uniform_refused, cnt.wave_dropped, cnt.one_group_left, cnt.fixpoints, cnt.lane_limit, cnt.early_dealt, cnt.dealings_simulated,
                        cnt.dealings_large, cnt.rule_admitted, cnt.rule_refused_by_size, cnt.rule_refused_by_planner, cnt.ragged_accepted, cnt.ragged_refused, cnt.streams_zero,
                        cnt.streams_short, cnt.streams_one_group, cnt.streams_dropped_wave, cnt.equal_scripts, cnt.k1r_grids, cnt.k1r_none};
    for (long v : all)
        if (v <= 0) { printf("a case was never reached\n"); return 1; }
    if (failures) { printf("%d mismatches\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
