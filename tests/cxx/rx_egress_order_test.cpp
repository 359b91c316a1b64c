// rx_egress_order_test.cpp -- sdrdaemon_amd/csrc/rx_egress_order.h against a literal simulation of the rounds: round j holds
// datagram j of every stream that still has one, streams in ascending order.  Stand-alone (tests/test_rx_egress_order.py builds it
// with the address and undefined-behaviour sanitizers); no GPU, no library.
#include "rx_egress_order.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrhip;

namespace {
int g_cases = 0;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            printf("FAILED %s:%d: %s (case %d)\n", __FILE__, __LINE__, #cond, g_cases);              \
            exit(1);                                                                                 \
        }                                                                                            \
    } while (0)

uint32_t rng_state = 12345;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Entry { size_t s, d; }; // datagram d (wire order) of stream s

// the definition, literally
std::vector<Entry> simulate(const std::vector<size_t> &F, size_t B)
{
    std::vector<Entry> out;
    for (size_t j = 0;; ++j) {
        bool any = false;
        for (size_t s = 0; s < F.size(); ++s)
            if (F[s] * B > j) { out.push_back(Entry{s, j}); any = true; }
        if (!any) break;
    }
    return out;
}

void check_case(const std::vector<size_t> &F, size_t B)
{
    ++g_cases;
    const size_t S = F.size();
    RxEgressOrder o;
    CHECK(o.plan(F.data(), S, B));
    const std::vector<Entry> sim = simulate(F, B);
    size_t N = 0;
    for (size_t s = 0; s < S; ++s) N += F[s] * B;
    CHECK(sim.size() == N && o.dgrams() == N && o.streams() == S && o.blocks_per_frame() == B);
    CHECK(o.wg_per_frame() == (B + 31) / 32 && o.grid() == (uint64_t)o.frames() * o.wg_per_frame());
    // positions: a permutation of 0 .. N - 1 that equals the simulation
    std::vector<int> seen(N, 0);
    for (size_t s = 0; s < S; ++s) {
        CHECK(o.frames(s) == F[s]);
        for (size_t f = 0; f < F[s]; ++f)
            for (size_t b = 0; b < B; ++b) {
                const uint64_t p = o.pos(s, f, b);
                CHECK(p < N);
                CHECK(!seen[p]++);
                CHECK(sim[p].s == s && sim[p].d == f * B + b);
            }
    }
    // the closed form's parts
    for (size_t s = 0; s < S; ++s)
        for (size_t f = 0; f < F[s]; ++f) {
            uint32_t A = 0, r = 0;
            for (size_t t = 0; t < S; ++t) { A += F[t] > f; r += t < s && F[t] > f; }
            CHECK(o.alive(f) == A && o.rank(s, f) == r);
        }
    // tags: the simulation's; every stream's subsequence in wire order
    std::vector<uint16_t> tags(N + 1, 0xabcd);
    o.tags(tags.data());
    CHECK(tags[N] == 0xabcd);
    std::vector<size_t> next(S, 0);
    for (size_t i = 0; i < N; ++i) {
        CHECK(tags[i] == sim[i].s);
        CHECK(sim[i].d == next[tags[i]]++);
    }
    for (size_t s = 0; s < S; ++s) CHECK(next[s] == F[s] * B);
    // the run table reproduces the positions: one run per delivered frame, stream-major, sources contiguous per stream
    std::vector<uint64_t> src0(S);
    for (size_t s = 0; s < S; ++s) src0[s] = (uint64_t)(s * 7 + 3) * 1000 * B * 512 + 16 * (rnd() % 5);
    std::vector<RxEgressRun> runs(o.frames() + 1);
    runs[o.frames()].src = 0x5a5a;
    CHECK(o.runs(src0.data(), runs.data()));
    CHECK(runs[o.frames()].src == 0x5a5a);
    size_t k = 0;
    for (size_t s = 0; s < S; ++s)
        for (size_t f = 0; f < F[s]; ++f, ++k) {
            CHECK(o.run(s, f) == k);
            const RxEgressRun &r = runs[k];
            CHECK(r.src == src0[s] + (uint64_t)f * B * 512);
            CHECK(r.src % 16 == 0 && r.dst % 512 == 0 && r.stride % 512 == 0 && r.stride >= 512);
            for (size_t b = 0; b < B; ++b) CHECK(r.dst + b * r.stride == o.pos(s, f, b) * 512);
        }
    CHECK(k == o.frames());
    if (N) { // a misaligned source is refused
        std::vector<uint64_t> bad(src0);
        for (size_t s = 0; s < S; ++s)
            if (F[s]) { bad[s] += 8; break; }
        CHECK(!o.runs(bad.data(), runs.data()));
    }
}

void check_refusals()
{
    RxEgressOrder o;
    std::vector<size_t> F(3, 1);
    CHECK(!o.plan(F.data(), 0, 160));
    CHECK(!o.plan(F.data(), 3, 0));
    CHECK(!o.plan(F.data(), 3, 0x10000));
    CHECK(o.frames() == 0 && o.dgrams() == 0 && o.streams() == 0);
    std::vector<size_t> many(65536, 0);
    CHECK(!o.plan(many.data(), many.size(), 160));
    CHECK(o.plan(many.data(), 65535, 160) && o.dgrams() == 0);
    // frames x workgroups per frame past 2^31 - 1: refused on the sums, nothing is sized
    const size_t wgpf = (160 + 31) / 32, most = 0x7fffffffu / wgpf;
    F[0] = (size_t)1 << 40; F[1] = 0; F[2] = 0;
    CHECK(!o.plan(F.data(), 3, 160));
    F[0] = ~(size_t)0; F[1] = 2;
    CHECK(!o.plan(F.data(), 3, 160)); // (a sum that would wrap)
    F[0] = most; F[1] = 1; F[2] = 0;
    CHECK(!o.plan(F.data(), 3, 160));
    F[0] = most / 2 + 1; F[1] = most / 2 + 1;
    CHECK(!o.plan(F.data(), 3, 160));
}
} // namespace

int main()
{
    const size_t Bs[5] = {128, 129, 160, 255, 256};
    for (int bi = 0; bi < 5; ++bi) {
        const size_t B = Bs[bi];
        check_case(std::vector<size_t>(5, 0), B);                   // all zero
        check_case(std::vector<size_t>(1, 3), B);                   // S = 1: the identity
        check_case(std::vector<size_t>(1, 0), B);
        check_case(std::vector<size_t>(6, 2), B);                   // all equal
        const size_t z0[5] = {0, 2, 3, 1, 1}, zm[5] = {2, 1, 0, 3, 1}, zl[5] = {1, 3, 2, 2, 0}, zz[5] = {0, 3, 0, 1, 0};
        check_case(std::vector<size_t>(z0, z0 + 5), B);             // a zero at the first,
        check_case(std::vector<size_t>(zm, zm + 5), B);             // a middle
        check_case(std::vector<size_t>(zl, zl + 5), B);             // and the last stream
        check_case(std::vector<size_t>(zz, zz + 5), B);
    }
    for (int i = 0; i < 60; ++i) {
        const size_t S = 1 + rnd() % 70, B = Bs[rnd() % 5];
        std::vector<size_t> F(S);
        for (size_t s = 0; s < S; ++s) F[s] = rnd() % 6;
        check_case(F, B);
    }
    check_refusals();
    printf("%d cases OK\n", g_cases);
    return 0;
}
