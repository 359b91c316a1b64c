// rx_paced_order_test.cpp -- the paced departure order (sdrdaemon_amd/csrc/rx_paced_order.h) on a CPU, as a stand-alone program
// (built with the address and undefined-behaviour sanitizers by tests/test_rx_paced_order.py).  The yardstick is a literal sort of
// all (stream, datagram) pairs by the key (2 j + 1) / (2 D_s), compared as exact 64-bit cross products, ties by stream.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rx_depart_order.h"
#include "rx_paced_order.h"

using namespace sdrhip;

static int failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                   \
            std::printf("\n");                          \
            if (++failures > 20) std::exit(1);          \
        }                                               \
    } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (rng_state >> 8) % n;
}

struct Item {
    uint32_t s;
    uint64_t j, D;
};
static bool before(const Item &a, const Item &b)
{
    const uint64_t l = (2 * a.j + 1) * b.D, r = (2 * b.j + 1) * a.D;
    return l != r ? l < r : a.s < b.s;
}

// one batch: F[s] frames of B[s] datagrams, frames of stream s from src0[s] on, one every `pitch` bytes
static void check_batch(const std::vector<size_t> &F, const std::vector<size_t> &B, uint64_t pitch, const char *what)
{
    const size_t S = F.size();
    RxPacedOrder o;
    CHECK(o.plan(F.data(), B.data(), S), "%s: plan", what);
    std::vector<Item> all;
    std::vector<uint64_t> src0(S);
    uint64_t at = 4096 + 16 * rnd(64);
    for (size_t s = 0; s < S; ++s) {
        src0[s] = at;
        at += (F[s] + rnd(3)) * pitch;
        for (uint64_t j = 0; j < (uint64_t)F[s] * B[s]; ++j) {
            const Item it = {(uint32_t)s, j, (uint64_t)F[s] * B[s]};
            all.push_back(it);
        }
        CHECK(o.dgrams(s) == (uint64_t)F[s] * B[s] && o.blocks(s) == B[s], "%s: stream %zu", what, s);
    }
    std::sort(all.begin(), all.end(), before);
    const size_t n = all.size();
    CHECK(o.dgrams() == n && o.streams() == S && o.grid() == (n + 31) / 32, "%s: dgrams %llu, expected %zu", what, (unsigned long long)o.dgrams(), n);
    // exact-size arrays with a guard behind them: the sanitizer sees a write past the end, the guard a write of the wrong width
    std::vector<uint16_t> tags(n + 1, 0xabcd), tags2(n + 1, 0xabcd);
    std::vector<uint32_t> tab(n + 1, 0xdeadbeefu), tab2(n + 1, 0xdeadbeefu);
    o.tags(tags.data());
    CHECK(o.table(src0.data(), pitch, tab.data()), "%s: table", what);
    CHECK(o.fill(src0.data(), pitch, tags2.data(), tab2.data()), "%s: fill", what);
    CHECK(tags == tags2 && tab == tab2, "%s: the one merge and the two calls differ", what);
    CHECK(tags[n] == 0xabcd && tab[n] == 0xdeadbeefu, "%s: written past the end", what);
    std::vector<std::vector<uint64_t> > where(S);
    for (size_t i = 0; i < n; ++i) {
        const Item &it = all[i];
        CHECK(tags[i] == it.s, "%s: tag %zu = %u, expected %u", what, i, tags[i], it.s);
        CHECK(o.pos(it.s, it.j) == i, "%s: pos(%u, %llu) = %llu, expected %zu", what, it.s, (unsigned long long)it.j,
              (unsigned long long)o.pos(it.s, it.j), i);
        const uint64_t f = it.j / B[it.s], b = it.j % B[it.s];
        const uint64_t src = src0[it.s] + f * pitch + b * 512;
        CHECK((uint64_t)tab[i] * 16 == src, "%s: table %zu = %llu, expected %llu", what, i, (unsigned long long)tab[i] * 16, (unsigned long long)src);
        where[it.s].push_back(i);
    }
    // the gap guarantee, from the tags alone: between two consecutive datagrams of s, floor or ceil(D_t / D_s) of every other t
    std::vector<uint64_t> seen(S);
    for (size_t s = 0; s < S; ++s) {
        const uint64_t Ds = (uint64_t)F[s] * B[s];
        for (size_t k = 0; k + 1 < where[s].size(); ++k) {
            std::fill(seen.begin(), seen.end(), 0);
            for (uint64_t i = where[s][k] + 1; i < where[s][k + 1]; ++i) ++seen[tags[i]];
            for (size_t t = 0; t < S; ++t) {
                if (t == s) continue;
                const uint64_t Dt = (uint64_t)F[t] * B[t], lo = Dt / Ds, hi = (Dt + Ds - 1) / Ds;
                CHECK(seen[t] == lo || seen[t] == hi, "%s: %llu datagrams of %zu between %zu's %zu and %zu (%llu or %llu)", what,
                      (unsigned long long)seen[t], t, s, k, k + 1, (unsigned long long)lo, (unsigned long long)hi);
            }
        }
    }
}

static void check_counts(const std::vector<size_t> &F, size_t Ball, const char *what)
{
    check_batch(F, std::vector<size_t>(F.size(), Ball), Ball * 512, what);
    // the equal-frames plan is the same plan
    RxPacedOrder a, b;
    const std::vector<size_t> B(F.size(), Ball);
    CHECK(a.plan(F.data(), B.data(), F.size()) && b.plan(F.data(), Ball, F.size()), "%s: plans", what);
    std::vector<uint16_t> ta((size_t)a.dgrams()), tb((size_t)b.dgrams());
    a.tags(ta.data());
    b.tags(tb.data());
    CHECK(ta == tb, "%s: plan(F, B[]) and plan(F, B) differ", what);
}

static void equal_counts_are_round_robin(size_t S, size_t F, size_t B)
{
    const std::vector<size_t> Fs(S, F);
    RxPacedOrder p;
    RxDepartOrder e;
    CHECK(p.plan(Fs.data(), B, S) && e.plan(Fs.data(), B, S), "equal: plans");
    CHECK(p.dgrams() == e.dgrams(), "equal: dgrams");
    std::vector<uint16_t> tp((size_t)p.dgrams()), te((size_t)e.dgrams());
    p.tags(tp.data());
    e.tags(te.data());
    CHECK(tp == te, "equal: tags S %zu F %zu B %zu", S, F, B);
    for (size_t s = 0; s < S; ++s)
        for (size_t f = 0; f < F; ++f)
            for (size_t b = 0; b < B; ++b)
                CHECK(p.pos(s, f * B + b) == e.pos(s, f * B + b), "equal: pos(%zu, %zu, %zu)", s, f, b);
}

static void refusals()
{
    RxPacedOrder o;
    const size_t one[1] = {1}, B1[1] = {128};
    CHECK(!o.plan(one, B1, 0), "no stream");
    CHECK(o.streams() == 0 && o.dgrams() == 0, "a refused plan leaves nothing");
    {
        std::vector<size_t> F(65536, 0), B(65536, 128);
        CHECK(!o.plan(F.data(), B.data(), 65536), "65536 streams");
        CHECK(o.plan(F.data(), B.data(), 65535) && o.dgrams() == 0, "65535 streams");
    }
    const size_t B0[1] = {0};
    CHECK(!o.plan(one, B0, 1) && !o.plan(one, (size_t)0, 1), "B = 0");
    // D_s >= 2^31
    const size_t big[1] = {(size_t)1 << 24}, B128[1] = {128}, under[1] = {((size_t)1 << 24) - 1};
    CHECK(!o.plan(big, B128, 1), "D = 2^31");
    CHECK(o.plan(under, B128, 1) && o.dgrams() == (((uint64_t)1 << 24) - 1) * 128, "D = 2^31 - 128");
    const size_t huge[1] = {~(size_t)0};
    CHECK(!o.plan(huge, B128, 1) && !o.plan(huge, (size_t)3, 1), "F x B wraps");
    // the total: 33 streams of 2^31 - 128 datagrams pass 32 (2^31 - 1); 32 do not
    {
        std::vector<size_t> F(33, ((size_t)1 << 24) - 1);
        CHECK(!o.plan(F.data(), (size_t)128, 33), "total past the grid");
        CHECK(o.plan(F.data(), (size_t)128, 32) && o.grid() <= 0x7fffffffu, "total inside the grid");
    }
    // the table: alignment, a pitch shorter than the frame, 2^32 units
    const size_t F2[2] = {2, 1}, B2[2] = {129, 128};
    std::vector<uint32_t> tab(2 * 129 + 128 + 1, 7u);
    uint64_t src0[2] = {0, 1 << 20};
    CHECK(o.plan(F2, B2, 2), "plan");
    CHECK(o.table(src0, 129 * 512, tab.data()), "table");
    std::fill(tab.begin(), tab.end(), 7u);
    src0[1] = (1 << 20) + 8;
    CHECK(!o.table(src0, 129 * 512, tab.data()), "src0 no multiple of 16");
    src0[1] = 1 << 20;
    CHECK(!o.table(src0, 129 * 512 + 8, tab.data()), "pitch no multiple of 16");
    CHECK(!o.table(src0, 128 * 512, tab.data()), "pitch shorter than a frame");
    src0[1] = ((uint64_t)1 << 36) - 127 * 512; // (its last datagram begins at unit 2^32)
    CHECK(!o.table(src0, 129 * 512, tab.data()), "past 2^32 units");
    src0[1] -= 512;
    CHECK(o.table(src0, 129 * 512, tab.data()), "the last unit");
    uint32_t most = 0;
    for (size_t i = 0; i + 1 < tab.size(); ++i) most = tab[i] > most ? tab[i] : most;
    CHECK(most == 0xffffffffu - 31, "the last unit: %u", most);
    std::fill(tab.begin(), tab.end(), 7u);
    src0[0] = ~(uint64_t)0 - 15;
    CHECK(!o.table(src0, 129 * 512, tab.data()), "an offset that wraps");
    src0[0] = 0;
    CHECK(!o.table(src0, (uint64_t)1 << 40, tab.data()), "a pitch past the units");
    for (size_t i = 0; i < tab.size(); ++i) CHECK(tab[i] == 7u, "a refused table wrote entry %zu", i);
    RxPacedOrder fresh;
    CHECK(!fresh.fill(src0, 129 * 512, nullptr, tab.data()), "no plan");
}

int main()
{
    // hand-picked: zeros first, middle and last; one stream; the tie shape D = (3 B, B); every B_s the ABI knows
    { const size_t F[] = {0, 3, 0, 1, 2, 0}; check_counts(std::vector<size_t>(F, F + 6), 5, "zeros"); }
    { const size_t F[] = {0, 3, 0, 1, 2, 0}; check_counts(std::vector<size_t>(F, F + 6), 129, "zeros 129"); }
    { const size_t F[] = {4}; check_counts(std::vector<size_t>(F, F + 1), 136, "one stream"); }
    { const size_t F[] = {0}; check_counts(std::vector<size_t>(F, F + 1), 136, "one empty stream"); }
    { const size_t F[] = {3, 1}; check_counts(std::vector<size_t>(F, F + 2), 128, "tie 3:1"); }
    { const size_t F[] = {1, 3}; check_counts(std::vector<size_t>(F, F + 2), 129, "tie 1:3"); }
    { const size_t F[] = {4, 1, 1, 1}; check_counts(std::vector<size_t>(F, F + 4), 136, "the issue's example"); }
    {
        // the tie rule, literally: D = (3 B, B), key of datagram i of stream 1 = that of datagram 3 i + 1 of stream 0 -> 0 first
        const size_t F[] = {3, 1}, Bq = 128;
        RxPacedOrder o;
        CHECK(o.plan(F, Bq, 2), "tie plan");
        for (uint64_t i = 0; i < Bq; ++i) CHECK(o.pos(1, i) == o.pos(0, 3 * i + 1) + 1, "tie %llu", (unsigned long long)i);
    }
    {
        const size_t F[] = {2, 1, 3, 0, 1}, B[] = {128, 129, 160, 256, 256};
        check_batch(std::vector<size_t>(F, F + 5), std::vector<size_t>(B, B + 5), 256 * 512, "per-stream fecblk");
        const size_t F2[] = {2, 1, 3}, B2[] = {128, 129, 160};
        check_batch(std::vector<size_t>(F2, F2 + 3), std::vector<size_t>(B2, B2 + 3), 160 * 512 + 16, "per-stream fecblk, odd pitch");
        const size_t F3[] = {129, 128}, B3[] = {128, 129}; // (equal D_s from different frames: one group)
        check_batch(std::vector<size_t>(F3, F3 + 2), std::vector<size_t>(B3, B3 + 2), 129 * 512, "equal D, different B");
    }
    // random counts 0 .. 40 (B = 1: the counts are the datagrams), and frame multiples of 128, 129, 136, 160
    for (int it = 0; it < 300; ++it) {
        const size_t S = 1 + rnd(8);
        std::vector<size_t> F(S);
        for (size_t s = 0; s < S; ++s) F[s] = rnd(41);
        check_counts(F, 1, "random 0..40");
    }
    const size_t Bs[] = {128, 129, 136, 160};
    for (int it = 0; it < 24; ++it) {
        const size_t S = 1 + rnd(6);
        std::vector<size_t> F(S), B(S);
        for (size_t s = 0; s < S; ++s) { F[s] = rnd(4); B[s] = Bs[rnd(4)]; }
        check_batch(F, B, 160 * 512, "random frames, mixed B");
        check_counts(F, Bs[it % 4], "random frames");
    }
    equal_counts_are_round_robin(1, 3, 129);
    equal_counts_are_round_robin(5, 2, 136);
    equal_counts_are_round_robin(7, 1, 128);
    equal_counts_are_round_robin(64, 3, 5);
    refusals();
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
