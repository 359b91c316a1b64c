// interp_ragged_plan_test.cpp -- the table of the sample-fed ragged interpolator launch (sdrdaemon_amd/csrc/interp_ragged_plan.h) on a
// CPU: every (stream, segment) that exists appears exactly once, a stream without input has the entry (s, 0) alone, a stream's
// segments tile its samples with the last one marked, equal counts give the uniform call's segments, and a launch that does not fit
// the kernels' 32-bit fields is refused before the table is touched.  Stand-alone: build with -fsanitize=address,undefined.
#include "interp_ragged_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace sdrhip;

static long long g_checks = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        ++g_checks;                                          \
        if (!(cond)) {                                       \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            return false;                                    \
        }                                                    \
    } while (0)

static const size_t COUNTS[] = {0, 1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 40000};
static const int NCOUNTS = (int)(sizeof(COUNTS) / sizeof(COUNTS[0]));
static const size_t SPANS[] = {0, 128, 256, 1024};

// the segment length the rules of the issue allow: K5w an even number of 128-input blocks (at most 16) or one block, K5 whole
// macro-cycles of 512 inputs (1024 at x2), a power of two of them up to 16
static bool seg_len_ok(InterpRoute route, int L, size_t span, const InterpRaggedPlan &p)
{
    if (route == IR_WAVE) {
        const size_t blocks = p.seg_len / 128;
        CHECK(p.seg_len % 128 == 0 && blocks >= 1 && blocks <= 16 && (blocks == 1 || blocks % 2 == 0), "K5w segment of %zu inputs", p.seg_len);
        if (span == 0) CHECK(blocks == 16, "default K5w segment of %zu blocks", blocks);
        else CHECK(blocks == (span / 128 > 16 ? 16 : span / 128), "span %zu gave %zu blocks", span, blocks);
        CHECK((size_t)p.nsub_per_seg == blocks, "nsub_per_seg %d", p.nsub_per_seg);
    } else if (route == IR_VALU) {
        const size_t mc = L == 1 ? 1024 : 512, per = p.seg_len / mc;
        CHECK(p.seg_len % mc == 0 && per >= 1 && per <= 16 && (per & (per - 1)) == 0, "K5 segment of %zu inputs", p.seg_len);
        CHECK((size_t)p.nsub_per_seg == per, "nsub_per_seg %d", p.nsub_per_seg);
    } else
        CHECK(p.seg_len == INTERP_COPY_SEG && p.seg_len % 4 == 0, "copy segment of %zu samples", p.seg_len);
    return true;
}

static bool check_bank(const std::vector<size_t> &n, int L, InterpRoute route, size_t span)
{
    const int S = (int)n.size();
    InterpRaggedPlan p;
    const char *why = nullptr;
    size_t max_n = 0, total = 0;
    for (int s = 0; s < S; ++s) { if (n[s] > max_n) max_n = n[s]; total += n[s]; }
    const int rc = interp_ragged_size(n.data(), S, L, route, span, &p, &why);
    if (max_n == 0) {
        CHECK(rc == INTERP_RAGGED_EMPTY && p.entries == 0 && p.grid == 0, "all-zero counts: rc %d", rc);
        return true;
    }
    CHECK(rc == INTERP_RAGGED_OK, "refused: %s", why ? why : "?");
    CHECK(p.route == route && p.max_n == max_n, "route / max_n");
    if (!seg_len_ok(route, L, span, p)) return false;
    size_t expect = 0;
    for (int s = 0; s < S; ++s) expect += n[s] ? (n[s] + p.seg_len - 1) / p.seg_len : 1;
    CHECK(p.entries == expect, "entries %u, expected %zu", p.entries, expect);
    CHECK(p.wpw == interp_pick_wpw(route, expect) && (p.wpw == 1 || p.wpw == 4), "wpw %d", p.wpw);
    CHECK(p.grid == (expect + p.wpw - 1) / p.wpw, "grid %u", p.grid);
    // the table, between guard words
    const size_t bytes = interp_ragged_table_bytes(S, p);
    CHECK(bytes == (size_t)S * 24 + expect * 8, "table bytes %zu", bytes);
    std::vector<unsigned char> buf(bytes + 16, 0xa5);
    const char *why2 = nullptr;
    InterpRaggedPlan p2;
    CHECK(interp_ragged_build(n.data(), S, L, route, span, 40004, 40004u << L, buf.data() + 8, bytes, &p2, &why2) == INTERP_RAGGED_OK, "build");
    CHECK(std::memcmp(&p, &p2, sizeof(p)) == 0, "build plans what size plans");
    for (int i = 0; i < 8; ++i) CHECK(buf[i] == 0xa5 && buf[8 + bytes + i] == 0xa5, "guard byte %d", i);
    std::vector<InterpMapRow> rows(S);
    std::vector<InterpMapEntry> ent(expect);
    std::memcpy(rows.data(), buf.data() + 8, (size_t)S * sizeof(InterpMapRow));
    if (expect) std::memcpy(ent.data(), buf.data() + 8 + (size_t)S * sizeof(InterpMapRow), expect * sizeof(InterpMapEntry));
    // every (stream, seg) once, stream-major; the segments of a stream tile [0, n_s) and the last one is marked
    size_t k = 0;
    for (int s = 0; s < S; ++s) {
        const size_t nseg = n[s] ? (n[s] + p.seg_len - 1) / p.seg_len : 1;
        CHECK(rows[s].n_in == n[s] && rows[s].nseg == (int)nseg, "row %d: n_in %u nseg %d", s, rows[s].n_in, rows[s].nseg);
        CHECK(rows[s].in_off == (uint64_t)s * 40004 && rows[s].out_off == (uint64_t)s * (40004u << L), "row %d offsets", s);
        size_t covered = 0;
        for (size_t g = 0; g < nseg; ++g, ++k) {
            CHECK(k < expect && ent[k].stream == (uint32_t)s && ent[k].seg == (uint32_t)g, "entry %zu is (%u, %u), expected (%d, %zu)", k, ent[k].stream,
                  ent[k].seg, s, g);
            size_t a, b;
            bool last;
            interp_ragged_segment(rows[s], ent[k], p.seg_len, &a, &b, &last);
            CHECK(a == covered && b >= a && b - a <= p.seg_len && (b > a || n[s] == 0), "stream %d segment %zu covers [%zu, %zu)", s, g, a, b);
            CHECK(last == (g + 1 == nseg), "stream %d segment %zu: last = %d", s, g, (int)last);
            covered = b;
        }
        CHECK(covered == n[s], "stream %d: %zu of %zu samples covered", s, covered, n[s]);
        if (n[s] == 0) CHECK(nseg == 1, "a stream without input has the entry (s, 0) alone");
    }
    CHECK(k == expect, "%zu entries walked of %zu", k, expect);
    // a buffer one byte short: refused, untouched
    std::vector<unsigned char> small(bytes, 0x5a);
    CHECK(interp_ragged_build(n.data(), S, L, route, span, 40004, 40004u << L, small.data(), bytes - 1, &p2, &why2) == INTERP_RAGGED_REFUSED, "short buffer");
    for (size_t i = 0; i < bytes; ++i) CHECK(small[i] == 0x5a, "short buffer touched at %zu", i);
    (void)total;
    return true;
}

// equal counts: the segment length and the per-stream segment count of the uniform planners, entries = nseg x streams
static bool check_equal(size_t n, int S, int L, InterpRoute route, size_t span)
{
    if (n == 0) return true;
    std::vector<size_t> v((size_t)S, n);
    InterpRaggedPlan p;
    const char *why = nullptr;
    CHECK(interp_ragged_size(v.data(), S, L, route, span, &p, &why) == INTERP_RAGGED_OK, "refused");
    int per = 0, nseg = 0;
    if (route == IR_WAVE) interp_plan_wave(n, span, &per, &nseg);
    else if (route == IR_VALU) interp_plan_valu(L, n, S, &per, &nseg);
    else return true;
    CHECK(p.nsub_per_seg == per && p.entries == (uint32_t)nseg * (uint32_t)S, "n %zu S %d L %d: per %d / %d, entries %u / %d", n, S, L, p.nsub_per_seg, per,
          p.entries, nseg * S);
    CHECK(p.wpw == interp_pick_wpw(route, (size_t)nseg * (size_t)S), "wpw");
    std::vector<InterpMapRow> rows(S);
    std::vector<InterpMapEntry> ent(p.entries);
    interp_ragged_fill(v.data(), S, p, n, n << L, rows.data(), ent.data());
    for (int s = 0; s < S; ++s)
        for (int g = 0; g < nseg; ++g)
            CHECK(ent[(size_t)s * nseg + g].stream == (uint32_t)s && ent[(size_t)s * nseg + g].seg == (uint32_t)g, "uniform entry (%d, %d)", s, g);
    return true;
}

static bool check_refusals()
{
    unsigned char tab[64];
    std::memset(tab, 0x77, sizeof(tab));
    InterpRaggedPlan p;
    const char *why = nullptr;
    const size_t big[2] = {5, (size_t)1 << 31};
    CHECK(interp_ragged_build(big, 2, 4, IR_WAVE, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED && why, "a count of 2^31");
    const size_t ok[2] = {5, INTERP_RAGGED_MAX_COUNT};
    CHECK(interp_ragged_size(ok, 2, 4, IR_WAVE, 0, &p, &why) == INTERP_RAGGED_OK && p.entries == 1 + (1u << 20), "2^31 - 1 samples: %u entries", p.entries);
    // 2^31 - 1 entries is the most: 64 streams of 2^31 - 1 samples in single blocks pass it
    std::vector<size_t> many(130, INTERP_RAGGED_MAX_COUNT);
    CHECK(interp_ragged_build(many.data(), 130, 4, IR_WAVE, 128, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED && why, "too many entries");
    CHECK(interp_ragged_size(many.data(), 127, 4, IR_WAVE, 128, &p, &why) == INTERP_RAGGED_OK && p.entries == 127u * (1u << 24) && p.wpw == 4 &&
              p.grid == 127u * (1u << 22),
          "127 x 2^24 entries");
    // routes and ratios that have no ragged kernel
    const size_t one[1] = {100};
    CHECK(interp_ragged_build(one, 1, 1, IR_WAVE, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "K5w has no x2");
    CHECK(interp_ragged_build(one, 1, 0, IR_VALU, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "K5 has no x1");
    CHECK(interp_ragged_build(one, 1, 2, IR_COPY, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "the copy is x1");
    CHECK(interp_ragged_build(one, 1, 7, IR_VALU, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "x128");
    CHECK(interp_ragged_build(one, 1, 4, IR_K6N, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "K6n");
    CHECK(interp_ragged_build(one, 0, 4, IR_WAVE, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_REFUSED, "no streams");
    const size_t zero[3] = {0, 0, 0};
    CHECK(interp_ragged_build(zero, 3, 4, IR_WAVE, 0, 0, 0, tab, sizeof(tab), &p, &why) == INTERP_RAGGED_EMPTY, "all zero");
    for (size_t i = 0; i < sizeof(tab); ++i) CHECK(tab[i] == 0x77, "a refused launch touched the table at %zu", i);
    // the route of the entry: a flag of its own, wave from x4 on unless the context says valu
    for (int L = -1; L <= 7; ++L)
        for (int wave = 0; wave < 2; ++wave) {
            const InterpPick k = interp_pick_mapped(L, wave != 0);
            if (L < 0 || L > 6) CHECK(k.route == IR_REFUSED && k.why, "L %d", L);
            else if (L == 0) CHECK(k.route == IR_COPY && k.variant == 0, "x1");
            else CHECK(k.route == (wave && L >= 2 ? IR_WAVE : IR_VALU) && k.variant == IV_MAPPED && k.wpw == 1, "L %d wave %d", L, wave);
        }
    CHECK((IV_MAPPED & (IV_GATHER | IV_COUNT | IV_S8 | IV_TABLE)) == 0, "a bit of its own");
    return true;
}

int main()
{
    // banks of 1..9 streams: S consecutive counts of the list from every start (wrapping), and the same with every other stream
    // emptied, every ratio, both routes (x1: the copy), every span
    long long banks = 0;
    for (int L = 0; L <= 6; ++L)
        for (int r = 0; r < 2; ++r) {
            const InterpRoute route = L == 0 ? IR_COPY : (r == 1 && L >= 2) ? IR_WAVE : IR_VALU;
            if (r == 1 && L < 2) continue;
            for (size_t span : SPANS) {
                if (span && route != IR_WAVE) continue; // (the override is K5w's)
                for (int S = 1; S <= 9; ++S)
                    for (int start = 0; start < NCOUNTS; ++start)
                        for (int step = 1; step <= 7; step += 3)
                            for (int holes = 0; holes < 2; ++holes) {
                                std::vector<size_t> n((size_t)S);
                                for (int s = 0; s < S; ++s) n[(size_t)s] = (holes && (s & 1)) ? 0 : COUNTS[(start + s * step) % NCOUNTS];
                                if (!check_bank(n, L, route, span)) return 1;
                                ++banks;
                            }
                for (int S = 1; S <= 9; ++S)
                    for (int c = 0; c < NCOUNTS; ++c)
                        if (!check_equal(COUNTS[c], S, L, route, span)) return 1;
            }
        }
    // workgroups of four: 4096 entries and more
    {
        std::vector<size_t> n(17);
        for (int s = 1; s < 17; ++s) n[(size_t)s] = (size_t)(240 + 6 * s) * 128 - 7 * (size_t)s; // (n[0] = 0: one entry)
        InterpRaggedPlan p;
        const char *why = nullptr;
        if (interp_ragged_size(n.data(), 17, 2, IR_WAVE, 128, &p, &why) != INTERP_RAGGED_OK || p.wpw != 4 || p.entries < 4096 || p.grid != (p.entries + 3) / 4) {
            std::printf("FAILED: workgroups of four: wpw %d, %u entries, grid %u\n", p.wpw, p.entries, p.grid);
            return 1;
        }
        n.resize(3);
        if (interp_ragged_size(n.data(), 3, 2, IR_WAVE, 128, &p, &why) != INTERP_RAGGED_OK || p.wpw != 1 || p.grid != p.entries) return 1;
        n.resize(17);
        for (int s = 3; s < 17; ++s) n[(size_t)s] = (size_t)(240 + 6 * s) * 128 - 7 * (size_t)s;
        if (!check_bank(n, 2, IR_WAVE, 128)) return 1;
    }
    if (!check_refusals()) return 1;
    std::printf("%lld banks, %lld checks\nOK\n", banks, g_checks);
    return 0;
}
