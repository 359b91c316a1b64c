// rx_depart_order_test.cpp -- sdrdaemon_amd/csrc/rx_depart_order.h (the departure order of a batch whose streams' frames differ in
// length: per-stream fecblk) against a literal simulation of the rounds: round j holds datagram j of every stream that still has
// one, streams in ascending order.  Positions, tags, totals, the run table (every run inside one frame, at most 256 datagrams,
// at most sum F + S (S - 1) runs, 16-byte aligned) and, for equal lengths, the closed form base_f + b A_f + r_f(s).  Stand-alone
// (tests/test_rx_stream_fec_abi.py builds it with the address and undefined-behaviour sanitizers); no GPU, no library.
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

uint32_t rng_state = 4711;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Entry { size_t s; uint64_t d; }; // datagram d (wire order) of stream s

// the definition, literally
std::vector<Entry> simulate(const std::vector<size_t> &F, const std::vector<size_t> &B)
{
    std::vector<Entry> out;
    for (uint64_t j = 0;; ++j) {
        bool any = false;
        for (size_t s = 0; s < F.size(); ++s)
            if ((uint64_t)F[s] * B[s] > j) { out.push_back(Entry{s, j}); any = true; }
        if (!any) break;
    }
    return out;
}

void check_case(const std::vector<size_t> &F, const std::vector<size_t> &B)
{
    ++g_cases;
    const size_t S = F.size();
    RxDepartOrder o;
    CHECK(o.plan(F.data(), B.data(), S));
    const std::vector<Entry> sim = simulate(F, B);
    uint64_t N = 0, frames = 0;
    for (size_t s = 0; s < S; ++s) { N += (uint64_t)F[s] * B[s]; frames += F[s]; }
    CHECK(sim.size() == N && o.dgrams() == N && o.streams() == S);
    // positions: a permutation of 0 .. N - 1 that equals the simulation
    std::vector<int> seen(N, 0);
    for (size_t s = 0; s < S; ++s) {
        CHECK(o.dgrams(s) == (uint64_t)F[s] * B[s] && o.blocks(s) == B[s]);
        for (uint64_t j = 0; j < o.dgrams(s); ++j) {
            const uint64_t p = o.pos(s, j);
            CHECK(p < N);
            CHECK(!seen[p]++);
            CHECK(sim[p].s == s && sim[p].d == j);
        }
    }
    // tags: the simulation's; every stream's subsequence in wire order
    std::vector<uint16_t> tags(N + 1, 0xabcd);
    o.tags(tags.data());
    CHECK(tags[N] == 0xabcd);
    std::vector<uint64_t> next(S, 0);
    for (uint64_t i = 0; i < N; ++i) {
        CHECK(tags[i] == sim[i].s);
        CHECK(sim[i].d == next[tags[i]]++);
    }
    // the run table: every datagram in exactly one run, every run inside one frame, the bound on their number
    CHECK(o.nruns() <= frames + S * (S - 1));
    CHECK(o.max_count() <= RX_DEPART_MAX_COUNT && o.wg_per_run() == (o.max_count() + 31) / 32 && o.grid() == (uint64_t)o.nruns() * o.wg_per_run());
    const uint64_t pitch = 384 * 512; // (a slot of 384 blocks: more than any frame here)
    std::vector<uint64_t> src0(S);
    for (size_t s = 0; s < S; ++s) src0[s] = (uint64_t)(s * 7 + 3) * 1000 * pitch + 16 * (rnd() % 5);
    std::vector<RxDepartRun> runs(o.nruns() + 1);
    runs[o.nruns()].src = 0x5a5a;
    CHECK(o.runs(src0.data(), pitch, runs.data()));
    CHECK(runs[o.nruns()].src == 0x5a5a);
    std::vector<int> moved(N, 0);
    uint32_t longest = 0;
    for (size_t k = 0; k < o.nruns(); ++k) {
        const RxDepartRun &r = runs[k];
        const size_t s = o.run_stream(k);
        const uint64_t j0 = o.run_first(k);
        CHECK(s < S && r.count >= 1 && r.count <= RX_DEPART_MAX_COUNT && r.count == o.run_count(k));
        CHECK(j0 / B[s] == (j0 + r.count - 1) / B[s] && j0 + r.count <= o.dgrams(s)); // inside one frame
        CHECK(r.src % 16 == 0 && r.dst % 512 == 0 && r.stride % 512 == 0 && r.stride >= 512);
        CHECK(r.src == src0[s] + (j0 / B[s]) * pitch + (j0 % B[s]) * 512);
        CHECK(r.dst == o.run_pos(k) * 512 && r.stride == o.run_alive(k) * 512);
        for (uint32_t i = 0; i < r.count; ++i) {
            const uint64_t p = r.dst / 512 + (uint64_t)i * (r.stride / 512);
            CHECK(p < N && p == o.pos(s, j0 + i));
            CHECK(!moved[p]++);
        }
        longest = r.count > longest ? r.count : longest;
    }
    for (uint64_t i = 0; i < N; ++i) CHECK(moved[i] == 1);
    CHECK(longest == o.max_count());
    if (N) { // a misaligned source or pitch is refused
        std::vector<uint64_t> bad(src0);
        for (size_t s = 0; s < S; ++s)
            if (F[s]) { bad[s] += 8; break; }
        CHECK(!o.runs(bad.data(), pitch, runs.data()));
        CHECK(!o.runs(src0.data(), pitch + 8, runs.data()));
    }
    // equal lengths: the closed form base_f + b A_f + r_f(s) (A_f = #{t : F_t > f}, r_f(s) = #{t < s : F_t > f},
    // base_f = B sum_{g<f} A_g), one run per frame, and the equal-frames plan gives the same table
    bool equal = true;
    for (size_t s = 1; s < S; ++s) equal = equal && B[s] == B[0];
    if (equal) {
        CHECK(o.nruns() == frames);
        for (size_t s = 0; s < S; ++s)
            for (size_t f = 0; f < F[s]; ++f) {
                uint64_t A = 0, rank = 0, base = 0;
                for (size_t t = 0; t < S; ++t) {
                    A += F[t] > f;
                    rank += t < s && F[t] > f;
                    base += (uint64_t)B[0] * (F[t] < f ? F[t] : f);
                }
                for (size_t b = 0; b < B[0]; ++b) CHECK(o.pos(s, f * B[0] + b) == base + b * A + rank);
            }
        RxDepartOrder e;
        CHECK(e.plan(F.data(), B[0], S) && e.dgrams() == N && e.nruns() == o.nruns());
        std::vector<RxDepartRun> same(e.nruns());
        CHECK(e.runs(src0.data(), pitch, same.data()));
        for (size_t k = 0; k < e.nruns(); ++k)
            CHECK(same[k].src == runs[k].src && same[k].dst == runs[k].dst && same[k].stride == runs[k].stride && same[k].count == runs[k].count);
    }
}

void check_case(const size_t *F, const size_t *B, size_t S) { check_case(std::vector<size_t>(F, F + S), std::vector<size_t>(B, B + S)); }

// a stream whose last datagram falls `off` datagrams into a frame of stream 0 (off = 0: at its first, B0 - 1: at its last)
void check_cut(size_t off_or_last, bool last)
{
    for (size_t B0 = 256; B0 >= 128; --B0)
        for (size_t Bt = 128; Bt <= 256; ++Bt)
            for (size_t Ft = 1; Ft <= 3; ++Ft) {
                const size_t off = last ? B0 - 1 : off_or_last, D = Ft * Bt;
                if (D % B0 != off || D >= 3 * B0 || D < B0) continue;
                const size_t F[3] = {3, Ft, 2}, B[3] = {B0, Bt, 131};
                check_case(F, B, 3);
                const size_t F2[3] = {Ft, 1, 3}, B2[3] = {Bt, 200, B0}; // (the cutting stream in front, the cut one last)
                check_case(F2, B2, 3);
                return;
            }
    const bool geometry_found = false;
    CHECK(geometry_found);
}

void check_refusals()
{
    RxDepartOrder o;
    size_t F[3] = {1, 1, 1}, B[3] = {128, 160, 256};
    CHECK(!o.plan(F, B, 0));
    B[1] = 0;
    CHECK(!o.plan(F, B, 3));
    B[1] = 257;
    CHECK(!o.plan(F, B, 3));
    CHECK(o.nruns() == 0 && o.dgrams() == 0 && o.streams() == 0 && o.max_count() == 0);
    B[1] = 160;
    std::vector<size_t> many(65536, 0), Bm(65536, 160);
    CHECK(!o.plan(many.data(), Bm.data(), many.size()));
    // runs x workgroups per run past 2^31 - 1: refused on the sums, nothing is sized
    F[0] = (size_t)1 << 40;
    CHECK(!o.plan(F, B, 3));
    F[0] = ~(size_t)0;
    CHECK(!o.plan(F, B, 3));
    F[0] = 0x7fffffffu / 8; F[1] = 1;
    CHECK(!o.plan(F, B, 3));
    F[0] = 2; F[1] = 1;
    CHECK(o.plan(F, B, 3) && o.dgrams() == 2 * 128 + 160 + 256);
}

// `dump S F_0 .. F_{S-1} B_0 .. B_{S-1}`: the array as the class orders it, one "stream datagram" line per entry (for the Python
// test, which holds it against rounds() of tests/test_gpu_rx_egress.py)
int dump(int argc, char **argv)
{
    const size_t S = (size_t)atoi(argv[2]);
    if (S == 0 || (size_t)argc != 3 + 2 * S) return 2;
    std::vector<size_t> F(S), B(S);
    for (size_t s = 0; s < S; ++s) { F[s] = (size_t)atoi(argv[3 + s]); B[s] = (size_t)atoi(argv[3 + S + s]); }
    RxDepartOrder o;
    if (!o.plan(F.data(), B.data(), S)) return 3;
    std::vector<uint16_t> tags(o.dgrams());
    o.tags(tags.data());
    std::vector<uint64_t> which(o.dgrams(), ~(uint64_t)0);
    for (size_t s = 0; s < S; ++s)
        for (uint64_t j = 0; j < o.dgrams(s); ++j) which[o.pos(s, j)] = j;
    for (uint64_t i = 0; i < o.dgrams(); ++i) printf("%u %llu\n", (unsigned)tags[i], (unsigned long long)which[i]);
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc > 2 && argv[1][0] == 'd') return dump(argc, argv);
    // the frame counts of tests/test_gpu_rx_egress.py's PLAN (zeros at the first, a middle and the last stream, 0 .. 3 frames)
    const size_t PLAN[6][5] = {{0, 2, 1, 2, 1}, {1, 0, 3, 2, 0}, {2, 1, 0, 1, 3}, {3, 3, 2, 0, 2}, {1, 2, 0, 3, 0}, {0, 1, 1, 2, 1}};
    const size_t Bs[5] = {128, 129, 160, 255, 256}, Bhub[5] = {128, 129, 160, 255, 132}; // (the second: nb_fec 0, 1, 32, 127, 4)
    for (int p = 0; p < 6; ++p) {
        check_case(PLAN[p], Bs, 5);
        check_case(PLAN[p], Bhub, 5);
        for (int bi = 0; bi < 5; ++bi) check_case(std::vector<size_t>(PLAN[p], PLAN[p] + 5), std::vector<size_t>(5, Bs[bi])); // equal counts
    }
    for (int bi = 0; bi < 5; ++bi) {
        check_case(std::vector<size_t>(5, 0), std::vector<size_t>(5, Bs[bi]));  // all zero
        check_case(std::vector<size_t>(1, 3), std::vector<size_t>(1, Bs[bi]));  // one stream alone
        check_case(std::vector<size_t>(1, 0), std::vector<size_t>(1, Bs[bi]));
        check_case(std::vector<size_t>(6, 2), std::vector<size_t>(6, Bs[bi]));  // all equal
    }
    const size_t z0[5] = {0, 2, 3, 1, 1}, zm[5] = {2, 1, 0, 3, 1}, zl[5] = {1, 3, 2, 2, 0}, zz[5] = {0, 3, 0, 1, 0};
    check_case(z0, Bs, 5);  // F = 0 at the first,
    check_case(zm, Bs, 5);  // a middle
    check_case(zl, Bs, 5);  // and the last stream
    check_case(zz, Bs, 5);
    // a stream's end inside another stream's frame: at its first datagram, offsets 1, 31, 32, 33 (the workgroup share's edges), its last
    const size_t offs[5] = {0, 1, 31, 32, 33};
    for (int i = 0; i < 5; ++i) check_cut(offs[i], false);
    check_cut(0, true);
    for (int i = 0; i < 60; ++i) {
        const size_t S = 1 + rnd() % 40;
        std::vector<size_t> F(S), B(S);
        for (size_t s = 0; s < S; ++s) { F[s] = rnd() % 5; B[s] = 128 + rnd() % 129; }
        check_case(F, B);
    }
    check_refusals();
    printf("%d cases OK\n", g_cases);
    return 0;
}
