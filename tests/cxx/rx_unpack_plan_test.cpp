// The unpack table (sdrdaemon_amd/csrc/rx_unpack_plan.h) against a literal walk of the packed bytes: block after block, stream after
// stream, sample after sample, each sample as long as its stream's format says -- with per-stream formats (K0x) and in the bank-wide
// form (K0p: fmt == NULL, every stream in one format), the latter also against the builder K0p had before it shared this table.
// Stand-alone (no GPU, no library); built with the address and undefined-behaviour sanitizers by tests/test_rx_unpack_plan.py.
#include "rx_unpack_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrhip;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures < 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// one case: cnt = nblk x S counts (block-major, stream-minor), fmt = S formats; stride_units = 0 packed, else strided rows (nblk = 1).
// bank: fmt holds S equal entries and the planner is asked in its bank-wide form (fmt == NULL, bank_fmt = that entry)
static void check_walk(const char *name, const std::vector<size_t> &cnt, size_t nblk, const std::vector<int> &fmt, uint64_t stride_units, bool bank)
{
    const size_t S = fmt.size();
    const int *pf = bank ? nullptr : fmt.data();
    const int bf = bank ? fmt[0] : -1; // (-1: never looked at while an array is given)
    // ---- the literal walk: byte offset of every row sample of every stream
    std::vector<std::vector<uint64_t> > at(S);
    uint64_t off = 0, nseg = 0;
    for (size_t b = 0; b < nblk; ++b)
        for (size_t s = 0; s < S; ++s) {
            const size_t bytes = fmt[s] == 0 ? 4 : 2;
            if (stride_units) off = 2 * (uint64_t)s * stride_units;
            nseg += cnt[b * S + s] ? 1 : 0;
            for (size_t i = 0; i < cnt[b * S + s]; ++i) { at[s].push_back(off); off += bytes; }
        }
    uint64_t sum_bytes = 0;
    for (size_t s = 0; s < S; ++s) sum_bytes += (uint64_t)at[s].size() * (fmt[s] == 0 ? 4 : 2);

    const UnpackXPlan m = unpackx_measure(cnt.data(), nblk, S, pf, bf);
    CHECK(m.fits, "%s", name);
    CHECK(m.nseg == nseg, "%s: nseg %llu, walk %llu", name, (unsigned long long)m.nseg, (unsigned long long)nseg);
    CHECK(m.bytes == sum_bytes, "%s: bytes %llu, walk %llu", name, (unsigned long long)m.bytes, (unsigned long long)sum_bytes);
    if (!stride_units) CHECK(off == sum_bytes, "%s", name);

    // (exactly sized: the sanitizer sees a write past either table)
    std::vector<UnpackXRow> rows(S + 1);
    std::vector<UnpackXSeg> segs((size_t)m.nseg);
    const UnpackXPlan p = unpackx_fill(cnt.data(), nblk, S, pf, stride_units, rows.data(), segs.data(), bf);
    CHECK(p.fits && p.nseg == m.nseg && p.bytes == m.bytes && p.grid == m.grid, "%s: fill and measure differ", name);

    uint64_t wg = 0, seg = 0;
    for (size_t s = 0; s < S; ++s) {
        const UnpackXRow &r = rows[s];
        CHECK(r.fmt == (uint32_t)fmt[s], "%s: stream %zu format", name, s);
        CHECK(r.total == at[s].size(), "%s: stream %zu total %u, walk %zu", name, s, r.total, at[s].size());
        CHECK(r.seg0 == seg, "%s: stream %zu seg0 %u, expected %llu", name, s, r.seg0, (unsigned long long)seg);
        CHECK(r.wg0 == wg, "%s: stream %zu wg0 %u, expected %llu", name, s, r.wg0, (unsigned long long)wg);
        // segments tile the row, and every row sample maps to the byte the walk gives
        uint64_t next = 0;
        const uint64_t upp = fmt[s] == 0 ? 2 : 1;
        for (uint32_t k = 0; k < r.nseg; ++k) {
            const UnpackXSeg &g = segs[r.seg0 + k];
            CHECK(g.n > 0 && g.dst == next, "%s: stream %zu segment %u starts at %u, expected %llu", name, s, k, g.dst, (unsigned long long)next);
            for (uint32_t j = 0; j < g.n && next + j < at[s].size(); ++j)
                CHECK(2 * (g.src + j * upp) == at[s][next + j], "%s: stream %zu sample %llu at byte %llu, walk %llu", name, s,
                      (unsigned long long)(next + j), (unsigned long long)(2 * (g.src + j * upp)), (unsigned long long)at[s][next + j]);
            next += g.n;
        }
        CHECK(next == at[s].size(), "%s: stream %zu segments cover %llu of %zu", name, s, (unsigned long long)next, at[s].size());
        seg += r.nseg;
        // the workgroups [wg0, wg0 + ceil(total / W)) cover the row once: workgroup w serves [w * W, min((w + 1) * W, total))
        wg += (at[s].size() + UNPACKX_WG_SAMPLES - 1) / UNPACKX_WG_SAMPLES;
    }
    CHECK(rows[S].wg0 == wg && rows[S].seg0 == seg && rows[S].nseg == 0 && rows[S].total == 0, "%s: sentinel", name);
    CHECK(p.grid == wg, "%s: grid %llu, expected %llu", name, (unsigned long long)p.grid, (unsigned long long)wg);
    // a workgroup index finds its stream: the last row whose wg0 is at or below it (K0x's search)
    for (uint64_t w = 0; w < wg; ++w) {
        size_t s = 0;
        for (size_t t = 0; t < S; ++t) if (rows[t].wg0 <= w) s = t;
        CHECK((w - rows[s].wg0) * UNPACKX_WG_SAMPLES < rows[s].total, "%s: workgroup %llu lands outside stream %zu", name, (unsigned long long)w, s);
    }
}

// the bank-wide table against a transcription of the builder K0p had of its own (sources counted in samples of the one format, rows
// without a format): segment order, dst, n, seg0, nseg, wg0, total, the sentinel row and the grid are equal, src is its sample
// index times the format's 2-byte units per sample
static void check_bank_builder(const char *name, const std::vector<size_t> &cnt, size_t nblk, size_t S, int bank_fmt)
{
    struct OldSeg { uint64_t src; uint32_t dst, n; };
    struct OldRow { uint32_t seg0, nseg, wg0, total; };
    size_t nseg = 0;
    for (size_t i = 0; i < cnt.size(); ++i) nseg += cnt[i] ? 1 : 0;
    std::vector<OldRow> orow(S + 1);
    std::vector<OldSeg> oseg(nseg);
    std::vector<uint64_t> src(cnt.size());
    {
        uint64_t acc = 0;
        for (size_t i = 0; i < cnt.size(); ++i) { src[i] = acc; acc += cnt[i]; }
    }
    uint64_t wg = 0;
    uint32_t k = 0;
    for (size_t s = 0; s < S; ++s) {
        OldRow &r = orow[s];
        uint64_t tot = 0;
        for (size_t blk = 0; blk < nblk; ++blk) tot += cnt[blk * S + s];
        r.seg0 = k; r.wg0 = (uint32_t)wg; r.total = (uint32_t)tot;
        uint32_t dst = 0;
        for (size_t blk = 0; blk < nblk; ++blk) {
            const size_t i = blk * S + s, n = cnt[i];
            if (!n) continue;
            oseg[k].src = src[i]; oseg[k].dst = dst; oseg[k].n = (uint32_t)n;
            dst += (uint32_t)n;
            ++k;
        }
        r.nseg = k - r.seg0;
        wg += (tot + 4096 - 1) / 4096;
    }
    orow[S].seg0 = k; orow[S].nseg = 0; orow[S].wg0 = (uint32_t)wg; orow[S].total = 0;

    std::vector<UnpackXRow> rows(S + 1);
    std::vector<UnpackXSeg> segs(nseg);
    const UnpackXPlan p = unpackx_fill(cnt.data(), nblk, S, nullptr, 0, rows.data(), segs.data(), bank_fmt);
    const uint64_t ups = bank_fmt == UNPACKX_S16 ? 2 : 1;
    CHECK(p.fits && p.nseg == nseg && p.grid == wg, "%s (bank %d): nseg %llu / %zu, grid %llu / %llu", name, bank_fmt, (unsigned long long)p.nseg, nseg,
          (unsigned long long)p.grid, (unsigned long long)wg);
    if (!p.fits || p.nseg != nseg) return;
    for (size_t s = 0; s <= S; ++s)
        CHECK(rows[s].seg0 == orow[s].seg0 && rows[s].nseg == orow[s].nseg && rows[s].wg0 == orow[s].wg0 && rows[s].total == orow[s].total,
              "%s (bank %d): row %zu", name, bank_fmt, s);
    for (size_t s = 0; s < S; ++s) CHECK(rows[s].fmt == (uint32_t)bank_fmt, "%s (bank %d): row %zu format", name, bank_fmt, s);
    for (size_t i = 0; i < nseg; ++i)
        CHECK(segs[i].src == oseg[i].src * ups && segs[i].dst == oseg[i].dst && segs[i].n == oseg[i].n, "%s (bank %d): segment %zu", name, bank_fmt, i);
}

// a case with its own formats, and (packed sources) the same counts in the bank-wide form of each format
static void check_case(const char *name, const std::vector<size_t> &cnt, size_t nblk, const std::vector<int> &fmt, uint64_t stride_units)
{
    check_walk(name, cnt, nblk, fmt, stride_units, false);
    if (stride_units) return;
    for (int f = UNPACKX_S16; f <= UNPACKX_S8; ++f) {
        check_walk(name, cnt, nblk, std::vector<int>(fmt.size(), f), 0, true);
        check_bank_builder(name, cnt, nblk, fmt.size(), f);
    }
}

int main()
{
    const size_t W = UNPACKX_WG_SAMPLES;
    // ---- hand-picked
    check_case("empty", std::vector<size_t>(3, 0), 1, {0, 1, 2}, 0);
    check_case("one block", {5, 7, 0, 9, 1, 8}, 1, {0, 1, 2, 1, 0, 2}, 0);
    check_case("odd 8-bit in front of int16", {3, 4, 0, 5, 6, 1}, 1, {1, 0, 2, 1, 0, 2}, 0);
    check_case("two odd rows: aligned again", {3, 5, 4}, 1, {1, 2, 0}, 0);
    check_case("zeros between", {1, 0, 0, 2, 0, 3}, 1, {1, 0, 1, 0, 2, 0}, 0);
    check_case("around W", {W - 1, W, W + 1, 2 * W, 2 * W + 1, 1}, 1, {0, 1, 2, 1, 0, 2}, 0);
    check_case("strided rows", {5, 7, 0, 9}, 1, {0, 1, 2, 1}, 2 * 12);
    check_case("strided rows, long", {W + 3, 7, W, 0}, 1, {1, 0, 2, 0}, 2 * ((W + 3 + 3) & ~(size_t)3));
    {
        // segments of 1..9 samples over many blocks: every chunk of a row straddles a boundary somewhere
        const size_t S = 4, nblk = 600;
        std::vector<size_t> c(S * nblk);
        for (size_t i = 0; i < c.size(); ++i) c[i] = 1 + (i * 7 + i / S) % 9;
        check_case("1..9 per segment", c, nblk, {1, 0, 2, 0}, 0);
        for (size_t i = 0; i < c.size(); i += 3) c[i] = 0;
        check_case("1..9 per segment with zeros", c, nblk, {0, 1, 1, 2}, 0);
    }
    // ---- random
    for (int it = 0; it < 300; ++it) {
        const size_t S = 1 + rnd() % 7, nblk = 1 + rnd() % 12;
        std::vector<int> f(S);
        for (size_t s = 0; s < S; ++s) f[s] = (int)(rnd() % 3);
        std::vector<size_t> c(S * nblk);
        for (size_t i = 0; i < c.size(); ++i) {
            const uint64_t kind = rnd() % 8;
            c[i] = kind == 0 ? 0 : kind < 5 ? 1 + rnd() % 9 : kind < 7 ? rnd() % 700 : W - 2 + rnd() % 5;
        }
        check_case("random", c, nblk, f, 0);
    }
    // ---- 32-bit fields: a row total, a segment and the grid that would not fit are refused, and nothing is written
    if (sizeof(size_t) > 4) {
        UnpackXRow canary[3];
        UnpackXSeg sc[4];
        for (int i = 0; i < 3; ++i) canary[i].total = 0xabcdu;
        const int f2[2] = {0, 1};
        const size_t big[2] = {(size_t)0xffffffffu - W + 1, 1};
        const size_t edge[2] = {(size_t)0xffffffffu - W, 1};
        const size_t two[4] = {(size_t)0x80000000u, 0, (size_t)0x80000000u, 0};
        const size_t huge[2] = {(size_t)1 << 40, 0};
        // (f = -1: the per-stream formats; else the bank-wide form of format f)
        for (int f = -1; f <= UNPACKX_S8; ++f) {
            const int *pf = f < 0 ? f2 : nullptr;
            CHECK(!unpackx_measure(big, 1, 2, pf, f).fits, "row total past 2^32 - W (%d)", f);
            CHECK(!unpackx_fill(big, 1, 2, pf, 0, canary, sc, f).fits && canary[0].total == 0xabcdu && canary[2].total == 0xabcdu, "nothing written (%d)", f);
            const UnpackXPlan e = unpackx_measure(edge, 1, 2, pf, f);
            CHECK(e.fits && e.grid == ((uint64_t)1 << 32) / W /* 2^20 - 1 workgroups and one for the second row */, "row total of 2^32 - 1 - W fits (%d)", f);
            CHECK(!unpackx_measure(two, 2, 2, pf, f).fits, "two blocks that sum past 32 bits (%d)", f);
            CHECK(!unpackx_measure(huge, 1, 2, pf, f).fits, "a count past 32 bits (%d)", f);
        }
        // (the grid: 2^31 workgroups of W samples need more streams than rows of 2^32 - W allow below ~2^19 streams: by sum)
        std::vector<size_t> many(600000, (size_t)0xffffffffu - W);
        std::vector<int> fm(many.size(), 1);
        const UnpackXPlan g = unpackx_measure(many.data(), 1, many.size(), fm.data()), gb = unpackx_measure(many.data(), 1, many.size(), nullptr, UNPACKX_S16);
        CHECK(g.grid > 0x7fffffffu && !g.fits && gb.grid == g.grid && !gb.fits, "grid past 2^31 - 1");
        // strided rows are one block
        const size_t c2[4] = {1, 2, 3, 4};
        CHECK(!unpackx_fill(c2, 2, 2, f2, 16, canary, sc).fits && canary[1].total == 0xabcdu, "strided rows: one block");
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
