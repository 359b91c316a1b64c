// rx_step_plan_test.cpp -- the Rx step planner (sdrdaemon_amd/csrc/rx_step_plan.h) against a transcription of the code it
// replaced: the booleans of sdrhip_rx_process and the decisions of rx_ragged as they stood in sdrhip_rx.cpp.  The uniform step
// runs over the full cross product of its inputs, every output field must agree; the ragged step's K2r job, delivery shape and
// input route over theirs, the encoder groups on seeded random banks.  Stand-alone: g++ -std=c++11, no library, no GPU.
#include "rx_step_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdrhip;

namespace {
const size_t SPF = 16129; // SDRHIP_SAMPLES_PER_FRAME
const int GROUP = 2;      // GF_FRAMES_PER_GROUP

int failures = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (failures++ < 20) { printf("MISMATCH %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                            \
    } while (0)

// ------------------------------------------------------------------------------------------------ the model: the code as it was
// sdrhip_rx_process, from `const size_t deliver_now` to the delivery; launches and copies left out, every decision kept.  What a
// launch was handed is recorded where it went out
struct MOut {
    size_t deliver_now, deliver_fb;
    bool lin_branch, filterless, flip;
    bool fuse, coresident;
    bool use_lin; int elin_first, elin_pending;
    bool k2_now; size_t k2_skip_from, k2_skip_to;         // launch_frame_pack went out on its own, with these
    bool k2_packed; size_t pk_skip_from, pk_skip_to; int lin_straddle; // launch_gf_encode128_pack, with these
    bool enc_now, enc_generic, encode_later;             // fec_encode128_launch | fec_encode_device with a frame list | late.encode
    bool k_lin;                                          // the structured encoder's arguments carry the stream-order rows
    bool record_framed;
};

MOut m_process(const RxStepIn &i, size_t frame_bytes)
{
    MOut o = MOut();
    const int L = i.L, R = i.R;
    const size_t done = i.done;
    const uint64_t pending = i.pending;
    const size_t stream_bytes = i.stream_bytes;
    o.deliver_now = i.pipelined ? (i.late_have ? i.late_frames : 0) : done;
    o.deliver_fb = i.pipelined && i.late_have ? i.late_frame_bytes : frame_bytes;
    bool use_lin = false, pack_with_encoder = false;
    size_t fa_skip_from = 0, fa_skip_to = 0;
    int elin_first = 0, elin_pending = 0;
    const bool structured = R >= i.enc_min_rows && frame_bytes % 4 == 0;
    const bool filterless = L == 0 || (i.fcpos != 2 && L <= 2);
    const bool fuse = i.late_encode && (i.rx_fused == 1 || i.rx_fused == 2);
    const bool coresident = i.late_encode && i.rx_fused == 3 && i.ev_framed;
    const bool direct = i.rx_direct && !i.pipelined && stream_bytes < 0x3fffffffu;
    o.fuse = fuse; o.coresident = coresident; o.filterless = filterless;
    if (filterless || (!direct && i.mfma_applies)) {
        o.lin_branch = true;
        if (i.pipelined) o.flip = true;
        if (R >= i.enc_min_rows) { // fec_encode_fuses_framing(c, R)
            const size_t first = pending ? 1 : 0;
            if (done > first && frame_bytes % 4 == 0) {
                elin_first = (int)first; elin_pending = (int)pending;
                use_lin = true;
            }
        }
        if (use_lin) {
            fa_skip_from = (size_t)elin_first * SPF - (size_t)elin_pending;
            fa_skip_to = done * SPF - (size_t)elin_pending;
        }
        pack_with_encoder = !i.pipelined && i.rx_fused && structured && R > 0 && use_lin;
        if (!pack_with_encoder) { o.k2_now = true; o.k2_skip_from = fa_skip_from; o.k2_skip_to = fa_skip_to; }
    }
    o.use_lin = use_lin; o.elin_first = elin_first; o.elin_pending = elin_pending;
    bool encode_later = false;
    if (done && R > 0) {
        if (structured) {
            if (use_lin) o.k_lin = true;
            if (i.pipelined) {
                encode_later = true;
            } else if (pack_with_encoder) {
                if (elin_first == 1) { o.lin_straddle = 1; fa_skip_from = 0; }
                o.k2_packed = true; o.pk_skip_from = fa_skip_from; o.pk_skip_to = fa_skip_to;
            } else
                o.enc_now = true;
        } else
            o.enc_generic = true;
    }
    o.encode_later = encode_later;
    o.record_framed = i.pipelined && encode_later && i.rx_fused == 3;
    return o;
}

long uniform_cases = 0;
void check_uniform(const RxStepIn &in, size_t fb)
{
    const MOut m = m_process(in, fb);
    const RxStepPlan p = rx_step_plan(in, fb);
    const RxStepDelivery d = rx_step_delivery(in, fb);
    ++uniform_cases;
#define WHERE "L %d fc %d R %d min %d pipe %d late %d/%d evf %d fused %d direct %d pend %llu done %zu sb %zu mf %d", in.L, in.fcpos, in.R, in.enc_min_rows, \
    (int)in.pipelined, (int)in.late_have, (int)in.late_encode, (int)in.ev_framed, in.rx_fused, in.rx_direct, (unsigned long long)in.pending, in.done, in.stream_bytes, (int)in.mfma_applies
    CHECK(p.deliver_now == m.deliver_now && p.deliver_fb == m.deliver_fb && d.frames == m.deliver_now && d.frame_bytes == m.deliver_fb, WHERE);
    CHECK(p.stream_order() == m.lin_branch, WHERE);
    CHECK((p.route == RX_ROUTE_LIN_FILTERLESS) == m.filterless, WHERE); // (filter-less calls always take the stream-order branch)
    CHECK((p.route == RX_ROUTE_LIN_MFMA) == (m.lin_branch && !m.filterless), WHERE);
    CHECK(p.flip_lin == m.flip, WHERE);
    CHECK(p.fuse == m.fuse && p.coresident == m.coresident, WHERE);
    CHECK(p.use_lin == m.use_lin, WHERE);
    if (m.use_lin) CHECK(p.lin_first == m.elin_first && (int)p.lin_pending == m.elin_pending, WHERE);
    // K2: on its own, inside the encoder's launch, or (frame layout) not at all -- and what it skips where it runs
    CHECK((p.stream_order() && !p.k2_in_encoder) == m.k2_now && p.k2_in_encoder == m.k2_packed, WHERE);
    if (m.k2_now) CHECK(p.skip_from == m.k2_skip_from && p.skip_to == m.k2_skip_to, WHERE);
    if (m.k2_packed) CHECK(p.skip_from == m.pk_skip_from && p.skip_to == m.pk_skip_to, WHERE);
    CHECK((int)p.lin_straddle == m.lin_straddle, WHERE);
    CHECK((p.encoder == RX_ENC_GENERIC) == m.enc_generic && (p.encoder == RX_ENC_DEFERRED) == m.encode_later, WHERE);
    CHECK((p.encoder == RX_ENC_STRUCTURED) == (m.enc_now || m.k2_packed), WHERE);
    CHECK((p.encoder == RX_ENC_NONE) == !(m.enc_generic || m.encode_later || m.enc_now || m.k2_packed), WHERE);
    CHECK((p.use_lin && (p.encoder == RX_ENC_STRUCTURED || p.encoder == RX_ENC_DEFERRED)) == m.k_lin, WHERE);
    CHECK(p.record_framed == m.record_framed, WHERE);
    CHECK(rx_late_overlaps(in) == (in.rx_fused == 3 && in.ev_framed), WHERE); // rx_settle: `c->opt.rx_fused != 3 || !rx->ev_framed`, negated
#undef WHERE
}

void test_uniform()
{
    const int min_rows_set[2] = {1, 4};
    const uint64_t pend_set[3] = {0, 1, 16128};
    const size_t sb_set[3] = {(size_t)84 << 20, 0x3ffffffeu, 0x3fffffffu};
    for (int mi = 0; mi < 2; ++mi) {
        const int min_rows = min_rows_set[mi];
        const int R_set[7] = {0, 1, min_rows - 1, min_rows, 32, 33, 127};
        for (int bits = 0; bits < 16; ++bits)
            for (int fused = 0; fused < 4; ++fused)
                for (int direct = 0; direct < 2; ++direct)
                    for (int L = 0; L <= 6; ++L)
                        for (int fc = 0; fc < 3; ++fc)
                            for (int ri = 0; ri < 7; ++ri)
                                for (int mf = 0; mf < 2; ++mf)
                                    for (int pi = 0; pi < 3; ++pi)
                                        for (size_t done = 0; done < 4; ++done)
                                            for (int si = 0; si < 3; ++si) {
                                                RxStepIn in = RxStepIn();
                                                in.L = L; in.fcpos = fc; in.R = R_set[ri];
                                                in.pipelined = bits & 1; in.late_have = bits & 2; in.late_encode = bits & 4; in.ev_framed = bits & 8;
                                                in.late_frames = 3; in.late_frame_bytes = (size_t)(128 + 7) * 512;
                                                in.rx_fused = fused; in.rx_direct = direct; in.enc_min_rows = min_rows;
                                                in.pending = pend_set[pi]; in.done = done;
                                                in.stream_bytes = sb_set[si];
                                                in.mfma_applies = mf != 0;
                                                check_uniform(in, (size_t)(128 + in.R) * 512);
                                            }
    }
}

// ------------------------------------------------------------------------------------------------ the ragged step's decisions
void test_ragged_small()
{
    for (int b = 0; b < 32; ++b) {
        const bool direct = b & 1, sw = b & 2, follow = b & 4, follow_bits = b & 8, any = b & 16;
        // rx_ragged: `if (max_dec && (!direct || sw || follow || follow_bits)) { ... if (direct) meta only; else pack }`
        const int model = any && (!direct || sw || follow || follow_bits) ? (direct ? RX_K2R_META : RX_K2R_PACK) : RX_K2R_NONE;
        CHECK((int)rx_ragged_k2r(any, direct, sw, follow, follow_bits) == model, "k2r %d", b);
    }
    for (int b = 0; b < 32; ++b) {
        const bool mixed = b & 1, same_base = b & 2, same_done = b & 4, dev_rows = b & 8, host = b & 16;
        // rx_ragged: `if (mixed) per stream 2-D; else if (same_base && (same_done || !(dev_rows && mem == HOST))) rectangle; else linear`
        const int model = mixed ? RX_DELIVER_PITCHED : same_base && (same_done || !(dev_rows && host)) ? RX_DELIVER_RECTANGLE : RX_DELIVER_LINEAR;
        CHECK((int)rx_ragged_delivery(mixed, same_base, same_done, dev_rows, host) == model, "delivery %d", b);
    }
    for (int b = 0; b < 32; ++b) {
        const bool batch = b & 1, dev_rows = b & 2, formats = b & 4, s16 = b & 8, mem_dev = b & 16;
        // rx_ragged: fmts, wide8, in_dev; then `if (fmts) unpack; else if (!in_dev) stage;  if (wide8) widen`
        const bool fmts = !batch && !dev_rows ? formats : false;
        const bool wide8 = !s16 && !batch && !dev_rows && !fmts;
        const bool in_dev = mem_dev || dev_rows;
        const RxRaggedInput r = rx_ragged_input(batch, dev_rows, formats, s16, mem_dev);
        CHECK(r.unpack == fmts && r.stage == (!fmts && !in_dev) && r.widen == wide8 && r.in_dev == in_dev, "input %d", b);
    }
    const size_t sb[3] = {1000, 0x3ffffffeu, 0x3fffffffu};
    for (int b = 0; b < 4; ++b)
        for (int si = 0; si < 3; ++si) // rx_ragged: `plan.mfma && c->opt.rx_direct && stream_bytes < 0x3fffffffu`
            CHECK(rx_ragged_direct(b & 1, b >> 1, sb[si]) == ((b & 1) && (b >> 1) && sb[si] < 0x3fffffffu), "direct %d %d", b, si);
}

// the frame-list loop of rx_ragged, with its rx_flist_entries and rx_encode_form
size_t m_flist_entries(size_t sum_done) { return (sum_done / GROUP + 3) * GROUP; }
int m_encode_form(int min_rows, int rows) { return rows < min_rows ? 0 : rows <= 32 ? 1 : 2; }
struct MGroups { size_t k, g_first[3], g_count[3]; int g_rows[3]; };
MGroups m_groups(const std::vector<int> &fec, const std::vector<size_t> &done, const std::vector<size_t> &index0, int min_rows, std::vector<int32_t> &fl)
{
    MGroups g = MGroups();
    size_t k = 0;
    for (int form = 0; form < 3; ++form) {
        g.g_first[form] = k;
        for (size_t s = 0; s < fec.size(); ++s) {
            const int rs = fec[s];
            if (rs <= 0 || !done[s] || m_encode_form(min_rows, rs) != form) continue;
            g.g_rows[form] = rs > g.g_rows[form] ? rs : g.g_rows[form];
            for (size_t f = 0; f < done[s]; ++f) fl[k++] = (int32_t)(index0[s] + f);
        }
        while (k % GROUP) fl[k++] = -1;
        g.g_count[form] = k - g.g_first[form];
    }
    g.k = k;
    return g;
}

struct StreamOf {
    const std::vector<int> &fec; const std::vector<size_t> &done, &first;
    RxEncStream operator()(size_t s) const { const RxEncStream e = {fec[s], done[s], first[s]}; return e; }
};

void test_groups()
{
    const size_t S_set[4] = {1, 2, 3, 17};
    const int fec_set[7] = {0, 1, 3, 4, 32, 33, 64};
    srand(20241);
    for (int iter = 0; iter < 20000; ++iter) {
        const size_t S = S_set[rand() % 4], cap = 16;
        const int min_rows = iter & 1 ? 4 : 1;
        std::vector<int> fec(S);
        std::vector<size_t> done(S), first(S);
        size_t sum_done = 0;
        for (size_t s = 0; s < S; ++s) {
            fec[s] = fec_set[rand() % 7]; done[s] = (size_t)(rand() % 6); first[s] = s * cap + (size_t)(rand() % 8);
            sum_done += done[s];
        }
        CHECK(rx_flist_entries(sum_done) == m_flist_entries(sum_done), "entries %zu", sum_done);
        std::vector<int32_t> fa(rx_flist_entries(sum_done), 77), fb(fa);
        const MGroups m = m_groups(fec, done, first, min_rows, fa);
        const StreamOf of = {fec, done, first};
        const RxEncGroups g = rx_encode_groups(S, of, min_rows, fb.data());
        CHECK(g.k == m.k && g.k <= rx_flist_entries(sum_done), "iter %d k %zu %zu", iter, g.k, m.k);
        CHECK(fa == fb, "iter %d list", iter);
        for (int f = 0; f < 3; ++f) {
            CHECK(g.first[f] == m.g_first[f] && g.count[f] == m.g_count[f] && g.rows[f] == m.g_rows[f], "iter %d form %d", iter, f);
            CHECK(g.count[f] % GROUP == 0, "iter %d form %d", iter, f);
            CHECK(rx_encode_form(fec[0], min_rows) == m_encode_form(min_rows, fec[0]), "form");
        }
        // every completed frame of a stream with recovery blocks exactly once, in a group whose launch has at least its rows; the
        // streams without recovery blocks nowhere
        std::vector<int> seen(S * cap + 16, 0), rows_at(S * cap + 16, 0);
        for (int f = 0; f < 3; ++f)
            for (size_t i = g.first[f]; i < g.first[f] + g.count[f]; ++i)
                if (fb[i] >= 0) { ++seen[(size_t)fb[i]]; rows_at[(size_t)fb[i]] = g.rows[f]; }
        std::vector<int> want(seen.size(), 0), rows_of(seen.size(), 0);
        for (size_t s = 0; s < S; ++s)
            for (size_t f = 0; f < done[s] && fec[s] > 0; ++f) { ++want[first[s] + f]; rows_of[first[s] + f] = fec[s]; }
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == want[i] && rows_at[i] >= rows_of[i], "iter %d frame %zu seen %d want %d", iter, i, seen[i], want[i]);
    }
}
} // namespace

int main()
{
    test_uniform();
    test_ragged_small();
    test_groups();
    printf("uniform cases: %ld\n", uniform_cases);
    if (failures) { printf("%d mismatches\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
