// rx_frame_area_test.cpp -- RxFrameArea (sdrdaemon_amd/csrc/rx_frame_area.h) against a transcription of the decision code it
// replaced: the window blocks of sdrhip_rx_process and rx_ragged, rx_grow_area, and the eight sites that wrote the frame
// arithmetic out.  Call sequences run through both; after every call the capacity, every stream's position, the streams that
// moved, whether the old area was kept and advance()'s values must agree.  Stand-alone: g++ -std=c++11, no library, no GPU.
#include "rx_frame_area.h"

#include <cstdio>
#include <cstdlib>

using namespace sdrhip;

namespace {
const uint64_t FS = 16129; // SDRHIP_SAMPLES_PER_FRAME

int failures = 0;
#define CHECK(cond, ...)                                                                                             \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            if (failures++ < 20) { printf("MISMATCH %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                            \
    } while (0)

struct Outcome {
    std::vector<uint8_t> moved;
    bool kept_old, grew, wrapped;
    std::vector<RxAdvance> adv;
};

// ------------------------------------------------------------------------------------------------ the model: the code as it was
struct Model {
    size_t S, cap_frames;
    std::vector<size_t> r_base;
    std::vector<uint64_t> r_pending;
    std::vector<uint8_t> r_open;
    std::vector<uint16_t> r_count;
    int pipelined, rx_window;
    struct { bool have; size_t slot0, frames; } late;
    bool old_work;

    Model(size_t S_, int pipelined_, int rx_window_) : S(S_), cap_frames(0), r_base(S_, 0), r_pending(S_, 0), r_open(S_, 0), r_count(S_, 0),
                                                       pipelined(pipelined_), rx_window(rx_window_), old_work(false)
    {
        late.have = false; late.slot0 = 0; late.frames = 0;
    }
    bool rx_aligned() const
    {
        for (size_t s = 1; s < S; ++s)
            if (r_base[s] != r_base[0] || r_pending[s] != r_pending[0] || r_open[s] != r_open[0] || r_count[s] != r_count[0]) return false;
        return true;
    }
    // ---- the eight copies of the arithmetic (n_dec = the call's decimated samples of that stream)
    size_t max_frames(size_t n_dec) const // sdrhip_rx_max_frames
    {
        size_t now = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t f = (size_t)((r_pending[s] + n_dec) / FS);
            if (f > now) now = f;
        }
        if (!pipelined) return now;
        return late.have && late.frames > now ? late.frames : now;
    }
    void ragged_room(const size_t *n_dec, size_t *need_max, size_t *sum_done) const // rx_ragged_room
    {
        *need_max = 0; *sum_done = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t done = (size_t)((r_pending[s] + n_dec[s]) / FS);
            *need_max = done + 1 > *need_max ? done + 1 : *need_max;
            *sum_done += done;
        }
    }
    size_t async_sum_done(const size_t *n_dec) const // sdrhip_rx_async.cpp, and sdrhip_rx_datagrams_async.cpp likewise
    {
        size_t sum_done = 0;
        for (size_t s = 0; s < S; ++s) sum_done += (size_t)((r_pending[s] + n_dec[s]) / FS);
        return sum_done;
    }
    size_t dgram_async_sum_done(const size_t *n_dec) const
    {
        size_t sum_done = 0;
        for (size_t s = 0; s < S; ++s) sum_done += (size_t)((r_pending[s] + n_dec[s]) / FS);
        return sum_done;
    }
    size_t admit_max_done(const size_t *n_dec) const // sdrhip_rx_datagrams.cpp: admit
    {
        size_t max_done = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t done = (size_t)((r_pending[s] + n_dec[s]) / FS);
            if (done > max_done) max_done = done;
        }
        return max_done;
    }
    static bool import_refused(uint64_t pending, uint32_t open, uint32_t count) // sdrhip_stream_state.cpp: import validation
    {
        return open > 1 || pending >= FS || (!open && pending) || count > 0xffffu;
    }

    // ---- the uniform step: sdrhip_rx_process
    Outcome uniform(size_t n_dec)
    {
        Outcome o;
        o.moved.assign(S, 0); o.kept_old = o.grew = o.wrapped = false;
        const uint64_t pending = r_pending[0];
        const bool frame_open = r_open[0] != 0;
        const uint64_t total = pending + n_dec;
        const size_t done = (size_t)(total / FS);
        const uint64_t rest = total - (uint64_t)done * FS;
        const size_t need = done + 1;
        if (old_work && !(late.have && late.slot0 == SIZE_MAX)) old_work = false;
        if (r_base[0] + need > cap_frames) {
            const bool late_here = late.have && late.slot0 != SIZE_MAX;
            const bool wrap_hits_late = late_here && need > late.slot0;
            if (need > cap_frames || wrap_hits_late) {
                const size_t wmul = rx_window ? (size_t)rx_window : pipelined ? 4 : 2;
                const size_t ncap = need > cap_frames ? wmul * need : cap_frames;
                if (late_here) { old_work = true; late.slot0 = SIZE_MAX; o.kept_old = true; }
                cap_frames = ncap;
                o.grew = true;
            } else
                o.wrapped = true;
            r_base.assign(S, 0);
            o.moved.assign(S, 1);
        }
        const int first_new = frame_open ? 1 : 0;
        const int started = (int)(done + (rest > 0 ? 1 : 0)) - first_new;
        RxAdvance a;
        a.done = done; a.rest = rest; a.first_new = first_new; a.started = started;
        a.frame_count0 = (unsigned)r_count[0] + first_new;
        a.idx0 = first_new ? (uint64_t)FS - pending : 0;
        o.adv.assign(S, a);
        if (pipelined) { late.have = done > 0; late.frames = done; late.slot0 = r_base[0]; }
        r_base.assign(S, r_base[0] + done);
        r_pending.assign(S, rest);
        r_open.assign(S, rest > 0 ? 1 : 0);
        r_count.assign(S, (uint16_t)(r_count[0] + done));
        return o;
    }
    void flush() { late.have = false; } // sdrhip_rx_flush, and the empty pipelined call

    void rx_grow_area(size_t need_max)
    {
        const size_t wmul = rx_window ? (size_t)rx_window : 2;
        const size_t ncap = wmul * need_max;
        for (size_t s = 0; s < S; ++s) r_base[s] = 0;
        cap_frames = ncap;
    }
    // ---- the ragged step: rx_ragged
    Outcome ragged(const size_t *n_dec)
    {
        Outcome o;
        o.moved.assign(S, 0); o.kept_old = o.grew = o.wrapped = false;
        std::vector<size_t> done(S);
        std::vector<uint64_t> rest(S);
        for (size_t s = 0; s < S; ++s) {
            const uint64_t total = r_pending[s] + n_dec[s];
            done[s] = (size_t)(total / FS);
            rest[s] = total - (uint64_t)done[s] * FS;
        }
        size_t need_max = 0;
        for (size_t s = 0; s < S; ++s) if (done[s] + 1 > need_max) need_max = done[s] + 1;
        if (old_work && !late.have) old_work = false;
        if (need_max > cap_frames) {
            rx_grow_area(need_max);
            o.moved.assign(S, 1);
            o.grew = true;
        } else {
            for (size_t s = 0; s < S; ++s) {
                if (r_base[s] + done[s] + 1 <= cap_frames) continue;
                r_base[s] = 0;
                o.moved[s] = 1;
                o.wrapped = true;
            }
        }
        o.adv.resize(S);
        for (size_t s = 0; s < S; ++s) {
            RxAdvance &a = o.adv[s];
            const int first_new = r_open[s] ? 1 : 0;
            const int started = (int)(done[s] + (rest[s] > 0 ? 1 : 0)) - first_new;
            a.done = done[s]; a.rest = rest[s]; a.first_new = first_new; a.started = started;
            a.frame_count0 = (unsigned)r_count[s] + (unsigned)first_new;
            a.idx0 = first_new ? (uint64_t)FS - r_pending[s] : 0;
        }
        for (size_t s = 0; s < S; ++s) {
            r_base[s] += done[s];
            r_pending[s] = rest[s];
            r_open[s] = rest[s] > 0 ? 1 : 0;
            r_count[s] = (uint16_t)(r_count[s] + done[s]);
        }
        return o;
    }
    void reset_streams(const uint8_t *m) // sdrhip_rx_reset_streams
    {
        for (size_t s = 0; s < S; ++s) {
            if (m && !m[s]) continue;
            r_pending[s] = 0;
            r_open[s] = 0;
            r_count[s] = 0;
            if (!m) r_base[s] = 0;
        }
    }
};

// ------------------------------------------------------------------------------------------------ the type, driven as the pipe drives it
struct Pipe {
    RxFrameArea area;
    int pipelined, rx_window;
    struct { bool have, in_old; size_t first, frames; } late;
    bool old_work;

    Pipe(size_t S, int pipelined_, int rx_window_) : pipelined(pipelined_), rx_window(rx_window_), old_work(false)
    {
        area.init(S);
        late.have = late.in_old = false; late.first = late.frames = 0;
    }
    Outcome step(const size_t *n_dec, bool as_pipelined)
    {
        const size_t S = area.streams();
        Outcome o;
        o.adv.resize(S);
        std::vector<size_t> done(S);
        std::vector<uint64_t> rest(S);
        for (size_t s = 0; s < S; ++s) { o.adv[s] = area.advance(s, n_dec[s]); done[s] = o.adv[s].done; rest[s] = o.adv[s].rest; }
        if (old_work && !(late.have && late.in_old)) old_work = false;
        const size_t wmul = rx_window ? (size_t)rx_window : as_pipelined ? 4 : 2;
        const RxAreaPlan p = area.plan(done.data(), late.have && !late.in_old ? late.first : RX_NO_LATE, wmul);
        o.moved = p.to_slot0;
        o.kept_old = p.new_cap && p.keep_old;
        o.grew = p.new_cap != 0;
        o.wrapped = !p.new_cap && p.moves();
        if (o.kept_old) { old_work = true; late.in_old = true; }
        area.moved(p);
        if (as_pipelined) { late.have = done[0] > 0; late.frames = done[0]; late.first = area.slot(0); late.in_old = false; }
        area.commit(done.data(), rest.data());
        return o;
    }
    void flush() { late.have = false; }
};

struct Tally { long wraps, grows, kept; Tally() : wraps(0), grows(0), kept(0) {} };

void compare_state(const Model &m, const Pipe &p, const char *what, long seq, int call)
{
    CHECK(m.cap_frames == p.area.cap(), "%s seq %ld call %d: cap %zu / %zu", what, seq, call, m.cap_frames, p.area.cap());
    CHECK(m.rx_aligned() == p.area.aligned(), "%s seq %ld call %d: aligned", what, seq, call);
    CHECK(m.old_work == p.old_work, "%s seq %ld call %d: old area held", what, seq, call);
    for (size_t s = 0; s < m.S; ++s)
        CHECK(m.r_base[s] == p.area.slot(s) && m.r_pending[s] == p.area.pending(s) && (m.r_open[s] != 0) == p.area.open(s) &&
                  m.r_count[s] == p.area.count(s),
              "%s seq %ld call %d stream %zu: base %zu / %zu pending %llu / %llu open %d / %d count %u / %u", what, seq, call, s, m.r_base[s],
              p.area.slot(s), (unsigned long long)m.r_pending[s], (unsigned long long)p.area.pending(s), (int)m.r_open[s], (int)p.area.open(s),
              (unsigned)m.r_count[s], (unsigned)p.area.count(s));
}

void compare_outcome(const Outcome &a, const Outcome &b, const char *what, long seq, int call)
{
    CHECK(a.kept_old == b.kept_old && a.grew == b.grew && a.wrapped == b.wrapped, "%s seq %ld call %d: kept %d / %d grew %d / %d wrapped %d / %d", what,
          seq, call, (int)a.kept_old, (int)b.kept_old, (int)a.grew, (int)b.grew, (int)a.wrapped, (int)b.wrapped);
    CHECK(a.moved == b.moved, "%s seq %ld call %d: the streams that moved", what, seq, call);
    for (size_t s = 0; s < a.adv.size(); ++s) {
        const RxAdvance &x = a.adv[s], &y = b.adv[s];
        CHECK(x.done == y.done && x.rest == y.rest && x.first_new == y.first_new && x.started == y.started && x.idx0 == y.idx0 &&
                  x.frame_count0 == y.frame_count0,
              "%s seq %ld call %d stream %zu: advance {%zu %llu %d %d %llu %u} / {%zu %llu %d %d %llu %u}", what, seq, call, s, x.done,
              (unsigned long long)x.rest, x.first_new, x.started, (unsigned long long)x.idx0, x.frame_count0, y.done, (unsigned long long)y.rest,
              y.first_new, y.started, (unsigned long long)y.idx0, y.frame_count0);
    }
}

// the sites that only ask "how many frames would these counts complete", before the call
void compare_arithmetic(const Model &m, const Pipe &p, const size_t *n_dec, const char *what, long seq, int call)
{
    const size_t S = m.S;
    size_t need_max = 0, sum_done = 0, max_done = 0, most0 = 0;
    for (size_t s = 0; s < S; ++s) {
        const size_t d = p.area.advance(s, n_dec[s]).done, d0 = p.area.advance(s, n_dec[0]).done;
        need_max = d + 1 > need_max ? d + 1 : need_max;
        sum_done += d;
        max_done = d > max_done ? d : max_done;
        most0 = d0 > most0 ? d0 : most0;
    }
    if (p.pipelined && p.late.have && p.late.frames > most0) most0 = p.late.frames;
    size_t m_need = 0, m_sum = 0;
    m.ragged_room(n_dec, &m_need, &m_sum);
    CHECK(m.max_frames(n_dec[0]) == most0, "%s seq %ld call %d: max_frames", what, seq, call);
    CHECK(m_need == need_max && m_sum == sum_done, "%s seq %ld call %d: ragged_room", what, seq, call);
    CHECK(m.async_sum_done(n_dec) == sum_done && m.dgram_async_sum_done(n_dec) == sum_done, "%s seq %ld call %d: batch sizing", what, seq, call);
    CHECK(m.admit_max_done(n_dec) == max_done, "%s seq %ld call %d: admit", what, seq, call);
}

// one call as sdrhip_rx_process (uniform = true) or sdrhip_rx_process_ragged would route it
void call(Model &m, Pipe &p, const size_t *n_dec, bool uniform, const char *what, long seq, int i, Tally *t)
{
    const size_t S = m.S;
    compare_arithmetic(m, p, n_dec, what, seq, i);
    size_t most = 0;
    for (size_t s = 0; s < S; ++s) most = n_dec[s] > most ? n_dec[s] : most;
    if (most == 0) { // an empty call: nothing moves; a pipelined pipe delivers what waits
        if (uniform && m.pipelined && m.late.have) { m.flush(); p.flush(); }
        compare_state(m, p, what, seq, i);
        return;
    }
    const bool by_uniform_step = uniform && m.rx_aligned();
    CHECK(m.rx_aligned() == p.area.aligned(), "%s seq %ld call %d: aligned before the call", what, seq, i);
    const Outcome a = by_uniform_step ? m.uniform(n_dec[0]) : m.ragged(n_dec);
    const Outcome b = p.step(n_dec, by_uniform_step && p.pipelined);
    compare_outcome(a, b, what, seq, i);
    compare_state(m, p, what, seq, i);
    if (t) { t->wraps += b.wrapped; t->grows += b.grew; t->kept += b.kept_old; }
}

uint64_t rng_state;
uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

void fixed_sequences()
{
    { // 1. test_rx_pipe_window_wraps_and_grows: S = 2, log2decim 1
        const size_t pf = 16129 << 1;
        const size_t sizes[] = {pf / 2, pf, pf, pf + 2, pf - 2, pf, 3 * pf / 2, 6 * pf + 10, pf / 4, 9 * pf, pf, pf, 2 * pf};
        Model m(2, 0, 0);
        Pipe p(2, 0, 0);
        Tally t;
        for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
            const size_t n[2] = {sizes[i] >> 1, sizes[i] >> 1};
            call(m, p, n, true, "wraps_and_grows", 0, (int)i, &t);
        }
        CHECK(t.wraps > 0 && t.grows > 0, "wraps_and_grows: %ld wraps, %ld growths", t.wraps, t.grows);
    }
    { // 2. test_pipelined_many_calls_wrap_the_frame_window (decimated counts), delivery one call late, then the flush
        const size_t sizes[] = {64516, 16129, 64516, 5000, 5000, 16129, 700, 0, 5000, 64516, 48387, 64516, 48387, 48387, 64516, 150000,
                                5000, 16129, 16129, 700, 20000, 20000, 40000, 64516};
        Model m(2, 1, 0);
        Pipe p(2, 1, 0);
        Tally t;
        for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
            const size_t n[2] = {sizes[i], sizes[i]};
            call(m, p, n, true, "pipelined_many_calls", 0, (int)i, &t);
        }
        m.flush(); p.flush();
        compare_state(m, p, "pipelined_many_calls", 0, 99);
        CHECK(t.wraps > 0 && t.grows > 0 && t.kept > 0, "pipelined_many_calls: %ld wraps, %ld growths, %ld kept", t.wraps, t.grows, t.kept);
    }
    { // 4. ragged calls until the streams differ, a reset of some streams, a full reset, then uniform calls
        Model m(3, 0, 0);
        Pipe p(3, 0, 0);
        const size_t r[3] = {2 * 16129 + 100, 5000, 0};
        for (int i = 0; i < 6; ++i) call(m, p, r, false, "reset", 0, i, nullptr);
        CHECK(!p.area.aligned(), "reset: the ragged calls left the streams aligned");
        const uint8_t mask[3] = {0, 1, 0};
        m.reset_streams(mask); p.area.reset(mask);
        compare_state(m, p, "reset", 0, 10);
        CHECK(!p.area.aligned(), "reset: one stream reset aligned the bank");
        call(m, p, r, true, "reset", 0, 11, nullptr); // (a uniform call on the unaligned bank: the ragged route)
        m.reset_streams(nullptr); p.area.reset(nullptr);
        compare_state(m, p, "reset", 0, 12);
        CHECK(p.area.aligned(), "reset: a full reset must align the bank");
        const size_t u[3] = {3 * 16129 + 7, 3 * 16129 + 7, 3 * 16129 + 7};
        for (int i = 0; i < 12; ++i) call(m, p, u, true, "reset", 0, 20 + i, nullptr);
        // import: what a blob may carry, and a stream taking it over
        const uint64_t pend[] = {0, 1, 16128, 16129, 1ull << 40};
        for (size_t a = 0; a < 5; ++a)
            for (uint32_t open = 0; open < 3; ++open)
                for (uint32_t cnt = 0xfffe; cnt < 0x10001; ++cnt)
                    CHECK(Model::import_refused(pend[a], open, cnt) == !RxFrameArea::importable(pend[a], open, cnt), "importable(%llu, %u, %u)",
                          (unsigned long long)pend[a], open, cnt);
        m.r_pending[1] = 77; m.r_open[1] = 1; m.r_count[1] = 65535;
        p.area.import_stream(1, 77, 1, 65535);
        compare_state(m, p, "import", 0, 0);
        for (int i = 0; i < 4; ++i) call(m, p, u, true, "import", 0, 1 + i, nullptr);
    }
}

// 5. equal counts on aligned state: the ragged step's plan is the uniform step's
void ragged_equals_uniform(long seq, size_t S, int rx_window, const size_t *counts, int ncalls)
{
    Model mu(S, 0, rx_window), mr(S, 0, rx_window);
    Pipe p(S, 0, rx_window);
    for (int i = 0; i < ncalls; ++i) {
        const std::vector<size_t> n(S, counts[i]);
        if (!counts[i]) continue;
        const Outcome u = mu.uniform(counts[i]), r = mr.ragged(n.data()), t = p.step(n.data(), false);
        compare_outcome(u, r, "uniform / ragged model", seq, i);
        compare_outcome(u, t, "uniform model / type", seq, i);
        compare_state(mu, p, "uniform model / type", seq, i);
        compare_state(mr, p, "ragged model / type", seq, i);
    }
}

void random_sequences()
{
    const size_t SS[4] = {1, 2, 3, 5};
    const size_t counts[7] = {0, 1, 16128, 16129, 16130, 3 * 16129, 9 * 16129 + 7};
    const int windows[3] = {0, 1, 3};
    const int NCALLS = 40;
    Tally tally[4][2];
    for (long seq = 0; seq < 2000; ++seq) {
        rng_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)seq * 0x100000001b3ull;
        const int si = (int)(seq % 4);
        const size_t S = SS[si];
        const int pipelined = seq % 10 == 9 ? 1 : 0;
        const int rx_window = windows[rnd() % 3];
        Model m(S, pipelined, rx_window);
        Pipe p(S, pipelined, rx_window);
        size_t equal[NCALLS];
        for (int i = 0; i < NCALLS; ++i) {
            std::vector<size_t> n(S);
            const bool uniform = pipelined || rnd() % 3 == 0;
            equal[i] = counts[rnd() % 7];
            for (size_t s = 0; s < S; ++s) n[s] = uniform ? equal[i] : counts[rnd() % 7];
            call(m, p, n.data(), uniform, pipelined ? "random pipelined" : "random", seq, i, &tally[si][pipelined]);
        }
        if (!pipelined) ragged_equals_uniform(seq, S, rx_window, equal, NCALLS);
    }
    // (every tenth sequence is pipelined: seq % 10 == 9 meets seq % 4 = 1, 3 only -- S = 2 and 5; the other two get theirs here)
    for (long seq = 2000; seq < 2200; ++seq) {
        rng_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)seq * 0x100000001b3ull;
        const int si = seq % 2 ? 2 : 0;
        const int rx_window = windows[rnd() % 3];
        Model m(SS[si], 1, rx_window);
        Pipe p(SS[si], 1, rx_window);
        for (int i = 0; i < NCALLS; ++i) {
            const std::vector<size_t> n(SS[si], counts[rnd() % 7]);
            call(m, p, n.data(), true, "random pipelined", seq, i, &tally[si][1]);
        }
    }
    for (int si = 0; si < 4; ++si)
        for (int pl = 0; pl < 2; ++pl) {
            const Tally &t = tally[si][pl];
            printf("S = %zu%s: %ld in-place wraps, %ld growths, %ld old areas kept\n", SS[si], pl ? " pipelined" : "", t.wraps, t.grows, t.kept);
            CHECK(t.wraps > 0 && t.grows > 0 && (!pl || t.kept > 0), "S = %zu pipelined %d: a path was never reached", SS[si], pl);
        }
}
} // namespace

int main()
{
    fixed_sequences();
    random_sequences();
    if (failures) { printf("FAILED: %d mismatches\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
