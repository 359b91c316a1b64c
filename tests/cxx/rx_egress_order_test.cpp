// rx_egress_order_test.cpp -- the equal-frames form of sdrdaemon_amd/csrc/rx_depart_order.h (every frame of the batch holds B
// datagrams: one run per delivered frame) against a literal simulation of the rounds: round j holds datagram j of every stream
// that still has one, streams in ascending order.  Stand-alone (tests/test_rx_egress_order.py builds it with the address and
// undefined-behaviour sanitizers); no GPU, no library.
#include "rx_depart_order.h"

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
    RxDepartOrder o;
    CHECK(o.plan(F.data(), B, S));
    const std::vector<Entry> sim = simulate(F, B);
    size_t N = 0, frames = 0;
    for (size_t s = 0; s < S; ++s) { N += F[s] * B; frames += F[s]; }
    CHECK(sim.size() == N && o.dgrams() == N && o.streams() == S);
    // one run per delivered frame, B datagrams each
    CHECK(o.nruns() == frames && o.max_count() == (frames ? B : 0));
    CHECK(o.wg_per_run() == (frames ? (B + 31) / 32 : 0) && o.grid() == (uint64_t)o.nruns() * o.wg_per_run());
    // positions: a permutation of 0 .. N - 1 that equals the simulation
    std::vector<int> seen(N, 0);
    for (size_t s = 0; s < S; ++s) {
        CHECK(o.dgrams(s) == F[s] * B && o.blocks(s) == B);
        for (size_t f = 0; f < F[s]; ++f)
            for (size_t b = 0; b < B; ++b) {
                const uint64_t p = o.pos(s, f * B + b);
                CHECK(p < N);
                CHECK(!seen[p]++);
                CHECK(sim[p].s == s && sim[p].d == f * B + b);
            }
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
    // the run table reproduces the positions: every (s, f) has exactly one run, whole frames, sources one pitch apart per stream
    const uint64_t pitch = (uint64_t)B * 512;
    std::vector<uint64_t> src0(S);
    for (size_t s = 0; s < S; ++s) src0[s] = (uint64_t)(s * 7 + 3) * 1000 * pitch + 16 * (rnd() % 5);
    std::vector<RxDepartRun> runs(o.nruns() + 1);
    runs[o.nruns()].src = 0x5a5a;
    CHECK(o.runs(src0.data(), pitch, runs.data()));
    CHECK(runs[o.nruns()].src == 0x5a5a);
    std::vector<size_t> first(S + 1, 0); // (stream-major numbering of the frames)
    for (size_t s = 0; s < S; ++s) first[s + 1] = first[s] + F[s];
    std::vector<int> has(frames, 0);
    bool equal_F = true;
    for (size_t s = 1; s < S; ++s) equal_F = equal_F && F[s] == F[0];
    for (size_t k = 0; k < o.nruns(); ++k) {
        const RxDepartRun &r = runs[k];
        const size_t s = o.run_stream(k);
        CHECK(s < S && o.run_first(k) % B == 0 && r.count == B && o.run_count(k) == B);
        const size_t f = (size_t)(o.run_first(k) / B);
        CHECK(f < F[s] && !has[first[s] + f]++);
        if (equal_F) CHECK(first[s] + f == k); // with equal F the table is stream-major
        CHECK(r.src == src0[s] + (uint64_t)f * pitch);
        CHECK(r.src % 16 == 0 && r.dst % 512 == 0 && r.stride % 512 == 0 && r.stride >= 512);
        // the closed form's parts: A_f = #{t : F_t > f}, r_f(s) = #{t < s : F_t > f}, base_f = B sum_{g<f} A_g
        uint64_t A = 0, rank = 0, base = 0;
        for (size_t t = 0; t < S; ++t) {
            A += F[t] > f;
            rank += t < s && F[t] > f;
            base += (uint64_t)B * (F[t] < f ? F[t] : f);
        }
        CHECK(r.stride == A * 512 && o.run_alive(k) == A);
        CHECK(r.dst == o.pos(s, f * B) * 512 && o.pos(s, f * B) == base + rank && o.run_pos(k) == base + rank);
        for (size_t b = 0; b < B; ++b) CHECK(r.dst + b * r.stride == o.pos(s, f * B + b) * 512);
    }
    for (size_t k = 0; k < frames; ++k) CHECK(has[k] == 1);
    if (N) { // a misaligned source is refused
        std::vector<uint64_t> bad(src0);
        for (size_t s = 0; s < S; ++s)
            if (F[s]) { bad[s] += 8; break; }
        CHECK(!o.runs(bad.data(), pitch, runs.data()));
    }
}

void check_refusals()
{
    RxDepartOrder o;
    std::vector<size_t> F(3, 1);
    CHECK(!o.plan(F.data(), 160, 0));
    CHECK(!o.plan(F.data(), (size_t)0, 3));
    CHECK(!o.plan(F.data(), 0x10000, 3));
    CHECK(!o.plan(F.data(), 257, 3)); // (the pipe never has more than 128 + 128)
    CHECK(o.nruns() == 0 && o.dgrams() == 0 && o.streams() == 0);
    std::vector<size_t> many(65536, 0);
    CHECK(!o.plan(many.data(), 160, many.size()));
    CHECK(o.plan(many.data(), 160, 65535) && o.dgrams() == 0);
    // runs x 8 workgroups (the longest run's) past 2^31 - 1: refused on the sums, nothing is sized
    const size_t most = 0x7fffffffu / 8;
    F[0] = (size_t)1 << 40; F[1] = 0; F[2] = 0;
    CHECK(!o.plan(F.data(), 160, 3));
    F[0] = ~(size_t)0; F[1] = 2;
    CHECK(!o.plan(F.data(), 160, 3)); // (a sum that would wrap)
    F[0] = most; F[1] = 1; F[2] = 0;
    CHECK(!o.plan(F.data(), 160, 3));
    F[0] = most / 2 + 1; F[1] = most / 2 + 1;
    CHECK(!o.plan(F.data(), 160, 3));
    std::vector<size_t> big(33, 0x7fffffffu / 256); // (each stream's count passes, their sum does not)
    CHECK(!o.plan(big.data(), 160, 33));
    CHECK(o.nruns() == 0 && o.dgrams() == 0 && o.streams() == 0);
    // the bound's own edge, (frames + S (S - 1)) x 8 <= 2^31 - 1, where it can be reached without 2^28 runs: frames of different
    // lengths, 16383 streams (S (S - 1) = 268386306) -- 49149 frames are accepted, 49150 refused
    const size_t S = 16383;
    std::vector<size_t> Fe(S, 3), Be(S, 1);
    Be[0] = 2;
    CHECK((49149 + (uint64_t)S * (S - 1)) * 8 <= 0x7fffffffu && (49150 + (uint64_t)S * (S - 1)) * 8 > 0x7fffffffu);
    CHECK(o.plan(Fe.data(), Be.data(), S) && o.dgrams() == 49149 + 3 && o.nruns() == 49149 + 1);
    Fe[S - 1] = 4;
    CHECK(!o.plan(Fe.data(), Be.data(), S) && o.nruns() == 0);
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
