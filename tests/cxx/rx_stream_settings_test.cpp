// rx_stream_settings_test.cpp -- RxStreamSettings, rx_ragged_counts and rx_join_counts (sdrdaemon_amd/csrc/rx_stream_settings.h)
// against a transcription of the code they replaced: the loose arrays of sdrhip_rx with their `X.empty() ? cfg.X : X[s]`
// expressions, rx_meta_record, the record cache of rx_stream_words, the refusal lines of the uniform entries, and the counting loops
// of rx_ragged, admit and rx_submit_batch.  Seeded scripts of setter calls, bank-value changes, ragged steps and datagram joins run
// through both; after every step every value must agree.  A few records are printed as hex for tests/test_rx_stream_settings.py,
// which forms them a third way.  Stand-alone: g++ -std=c++11, no library, no GPU.
#include "rx_stream_settings.h"

#include <cstdio>
#include <cstdlib>

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
struct Cfg { uint32_t center_frequency_khz, sample_rate; int nb_fec; unsigned sample_bits; int log2decim, fcpos; };

unsigned m_decimated_sample_size(unsigned log2decim, unsigned ss) // sdrhip_host.h
{
    if (log2decim == 0) return ss;
    const unsigned target = 16 - log2decim, trunk = ss < target ? 0 : ss - target;
    return ss + log2decim - trunk;
}
unsigned m_ragged_shift_word(unsigned log2decim, unsigned ss) // sdrhip_host.h: decimated_shifts, ragged_shift_word
{
    const unsigned target = 16 - log2decim;
    const unsigned norm = ss < target ? target - ss : 0, trunk = ss < target ? 0 : ss - target;
    return norm | (trunk << 8);
}
void m_meta_record(uint32_t fc, uint32_t sr, int nb_fec, unsigned ssd, unsigned w[6]) // sdrhip_rx.cpp: rx_meta_record
{
    uint8_t m[24];
    memcpy(m + 0, &fc, 4); memcpy(m + 4, &sr, 4);
    m[8] = (uint8_t)((ssd - 1) / 8 + 1);
    m[9] = (uint8_t)ssd;
    m[10] = 128; m[11] = (uint8_t)nb_fec;
    memset(m + 12, 0, 8);
    uint32_t crc = 0xFFFFFFFFu;
    for (int i = 0; i < 20; ++i) {
        crc ^= m[i];
        for (int k = 0; k < 8; ++k) crc = (crc & 1) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
    }
    crc ^= 0xFFFFFFFFu;
    memcpy(m + 20, &crc, 4);
    memcpy(w, m, 24);
}

struct Refused { bool is; size_t index; long value; }; // a setter's fail(SDRHIP_EINVAL, "...[%zu] = %d, must be ...")

struct Model {
    size_t S;
    Cfg cfg;
    std::vector<uint32_t> sm_fc, sm_rate;
    uint64_t sm_version;
    struct SmKey { uint64_t version; unsigned w2, fc, rate; int log2decim; } sm_key;
    std::vector<unsigned> sm_words;
    bool sm_uploaded;
    std::vector<int> sf_fec;
    std::vector<unsigned> sm_w2;
    std::vector<unsigned> sb_bits;
    uint64_t formed; // (not the parent's: counts the passes through the forming branch)

    Model(size_t S_, const Cfg &c) : S(S_), cfg(c), sm_version(0), sm_uploaded(false), formed(0)
    {
        const SmKey k = {~(uint64_t)0, 0, 0, 0, 0};
        sm_key = k;
    }
    // ---- the setters (sdrhip_rx.cpp), behind their lock and their refusals of pipe states
    void set_stream_meta(const uint32_t *center_frequency_khz, const uint32_t *sample_rate)
    {
        if (center_frequency_khz) sm_fc.assign(center_frequency_khz, center_frequency_khz + S);
        else sm_fc.clear();
        if (sample_rate) sm_rate.assign(sample_rate, sample_rate + S);
        else sm_rate.clear();
        ++sm_version;
    }
    Refused set_stream_fec(const int *nb_fec, int *most_out)
    {
        int most = cfg.nb_fec;
        if (nb_fec) {
            most = 0;
            for (size_t s = 0; s < S; ++s) {
                if (nb_fec[s] < 0 || nb_fec[s] > 128) { const Refused r = {true, s, nb_fec[s]}; return r; }
                most = nb_fec[s] > most ? nb_fec[s] : most;
            }
        }
        *most_out = most; // (rx_repitch to (128 + most) * 512 here)
        if (nb_fec) sf_fec.assign(nb_fec, nb_fec + S);
        else sf_fec.clear();
        ++sm_version;
        const Refused ok = {false, 0, 0};
        return ok;
    }
    Refused set_stream_bits(const unsigned *sample_bits)
    {
        if (sample_bits)
            for (size_t s = 0; s < S; ++s)
                if (sample_bits[s] < 1 || sample_bits[s] > 16) { const Refused r = {true, s, (long)sample_bits[s]}; return r; }
        if (sample_bits) sb_bits.assign(sample_bits, sample_bits + S);
        else sb_bits.clear();
        ++sm_version;
        const Refused ok = {false, 0, 0};
        return ok;
    }
    // ---- sdrhip_pipes.h
    int rx_fec_of(size_t s) const { return sf_fec.empty() ? cfg.nb_fec : sf_fec[s]; }
    int rx_fec_max() const
    {
        if (sf_fec.empty()) return cfg.nb_fec;
        int m = 0;
        for (size_t s = 0; s < sf_fec.size(); ++s) m = sf_fec[s] > m ? sf_fec[s] : m;
        return m;
    }
    bool rx_fec_mixed() const
    {
        for (size_t s = 1; s < sf_fec.size(); ++s)
            if (sf_fec[s] != sf_fec[0]) return true;
        return false;
    }
    unsigned rx_bits_of(size_t s) const { return sb_bits.empty() ? cfg.sample_bits : sb_bits[s]; }
    size_t rx_frame_bytes() const { return (size_t)(128 + rx_fec_max()) * 512; }
    size_t rx_stream_blocks(size_t s) const { return (size_t)(128 + rx_fec_of(s)); }
    size_t rx_stream_bytes(size_t s) const { return rx_stream_blocks(s) * 512; }
    size_t rx_join_unit() const { return cfg.log2decim == 1 && cfg.fcpos != 2 ? 4 : (size_t)1 << cfg.log2decim; }
    // ---- the getters' expressions
    uint32_t get_fc(size_t s) const { return sm_fc.empty() ? cfg.center_frequency_khz : sm_fc[s]; }
    uint32_t get_rate(size_t s) const { return sm_rate.empty() ? cfg.sample_rate : sm_rate[s]; }
    // ---- the two refusal lines of sdrhip_rx_process / _submit / _set_pipelined(1): 1 = the fecblk line, 2 = the sample-bits line
    int uniform_refused() const
    {
        if (!sf_fec.empty()) return 1;
        if (!sb_bits.empty()) return 2;
        return 0;
    }
    // ---- rx_stream_words
    const unsigned *rx_stream_words(unsigned ssd)
    {
        if (sm_fc.empty() && sm_rate.empty() && sf_fec.empty() && sb_bits.empty()) return nullptr;
        unsigned w[6];
        m_meta_record(cfg.center_frequency_khz, cfg.sample_rate, cfg.nb_fec, ssd, w);
        const SmKey key = {sm_version, w[2], w[0], w[1], cfg.log2decim};
        const SmKey &old = sm_key;
        if (key.version != old.version || key.w2 != old.w2 || key.fc != old.fc || key.rate != old.rate || key.log2decim != old.log2decim) {
            sm_words.resize(S * 3);
            sm_w2.resize(S);
            for (size_t s = 0; s < S; ++s) {
                m_meta_record(sm_fc.empty() ? cfg.center_frequency_khz : sm_fc[s], sm_rate.empty() ? cfg.sample_rate : sm_rate[s], rx_fec_of(s),
                              sb_bits.empty() ? ssd : m_decimated_sample_size((unsigned)cfg.log2decim, sb_bits[s]), w);
                unsigned *t = &sm_words[s * 3];
                t[0] = w[0]; t[1] = w[1]; t[2] = w[5];
                sm_w2[s] = w[2];
            }
            sm_key = key;
            sm_uploaded = false;
            ++formed;
        }
        return sm_words.data();
    }
    // ---- rx_ragged: the counting loop, and the words of its row loop
    struct Ragged {
        std::vector<RxAdvance> adv;
        std::vector<size_t> done;
        std::vector<uint64_t> rest;
        size_t max_in, max_done, sum_done, max_dec, max_row;
    };
    Ragged rx_ragged_counts(const RxFrameArea &area, const size_t *n_in) const
    {
        const int L = cfg.log2decim;
        Ragged r;
        r.adv.resize(S); r.done.resize(S); r.rest.resize(S);
        r.max_in = 0;
        for (size_t s = 0; s < S; ++s) if (n_in[s] > r.max_in) r.max_in = n_in[s];
        r.max_done = r.sum_done = r.max_dec = r.max_row = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t n_dec = n_in[s] >> L;
            r.adv[s] = area.advance(s, n_dec);
            r.done[s] = r.adv[s].done;
            r.rest[s] = r.adv[s].rest;
            if (r.done[s] > r.max_done) r.max_done = r.done[s];
            if (r.done[s] * rx_stream_bytes(s) > r.max_row) r.max_row = r.done[s] * rx_stream_bytes(s);
            if (n_dec > r.max_dec) r.max_dec = n_dec;
            r.sum_done += r.done[s];
        }
        return r;
    }
    void rx_ragged_row(size_t s, unsigned row[5]) // fc, rate, crc0, w2, shifts
    {
        const int L = cfg.log2decim;
        unsigned mw[6];
        m_meta_record(cfg.center_frequency_khz, cfg.sample_rate, cfg.nb_fec, m_decimated_sample_size((unsigned)L, cfg.sample_bits), mw);
        const unsigned *sw = rx_stream_words(m_decimated_sample_size((unsigned)L, cfg.sample_bits));
        row[0] = sw ? sw[s * 3] : mw[0]; row[1] = sw ? sw[s * 3 + 1] : mw[1];
        row[2] = sw ? sw[s * 3 + 2] : mw[5];
        row[3] = sw ? sm_w2[s] : mw[2];
        row[4] = m_ragged_shift_word((unsigned)L, rx_bits_of(s));
    }
    // ---- admit (sdrhip_rx_datagrams.cpp)
    void admit(const RxFrameArea &area, const std::vector<size_t> &carry, const size_t *n_released, size_t *max_done_out, size_t *max_row_out) const
    {
        const size_t U = rx_join_unit();
        size_t max_done = 0, max_row = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t fed = (carry[s] + n_released[s] * 16129) / U * U;
            const size_t done = area.advance(s, fed >> cfg.log2decim).done;
            if (done > max_done) max_done = done;
            if (done * rx_stream_bytes(s) > max_row) max_row = done * rx_stream_bytes(s);
        }
        *max_done_out = max_done; *max_row_out = max_row;
    }
    // ---- rx_submit_batch (sdrhip_rx_datagrams_async.cpp; sdrhip_rx_process_datagrams has its first four lines)
    struct Join { std::vector<size_t> fed, left; bool any; size_t sum_done, b_frames; };
    Join submit_batch(const RxFrameArea &area, const std::vector<size_t> &carry, const size_t *released) const
    {
        const size_t U = rx_join_unit();
        Join j;
        j.fed.resize(S); j.left.resize(S);
        j.any = false; j.sum_done = j.b_frames = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t k = released[s];
            const size_t total = carry[s] + k * 16129;
            j.fed[s] = total / U * U;
            j.left[s] = total - j.fed[s];
            j.any = j.any || j.fed[s] != 0;
            const size_t done = area.advance(s, j.fed[s] >> cfg.log2decim).done;
            j.sum_done += done;
            j.b_frames += done * rx_stream_bytes(s);
        }
        return j;
    }
};

// ------------------------------------------------------------------------------------------------ both sides, step by step
uint64_t rng_state;
uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

struct Tally { long zero_in, zero_done, several, inside_open, unit4, refused, formed, kept, mixed, equal_fec; };

struct Pair {
    size_t S;
    Model m;
    RxStreamSettings st;
    RxBankValues bank;
    RxFrameArea area;
    std::vector<size_t> carry;
    // (the harness's own record of what the cache was last formed for: the rule the type states)
    bool formed_once, since_taken;
    uint64_t formed_version;
    RxBankValues formed_bank;
    Tally *t;

    Pair(size_t S_, const Cfg &c, Tally *t_) : S(S_), m(S_, c), carry(S_, 0), formed_once(false), since_taken(false), formed_version(0), t(t_)
    {
        st.init(S);
        area.init(S);
        sync_bank();
        formed_bank = bank;
    }
    void sync_bank()
    {
        const RxBankValues b = {m.cfg.center_frequency_khz, m.cfg.sample_rate, m.cfg.nb_fec, m.cfg.sample_bits, m.cfg.log2decim};
        bank = b;
    }
    void compare(const char *what, long seq, int i)
    {
        for (size_t s = 0; s < S; ++s) {
            CHECK(st.fc(bank, s) == m.get_fc(s) && st.rate(bank, s) == m.get_rate(s), "%s seq %ld step %d: fc / rate of stream %zu", what, seq, i, s);
            CHECK(st.fec(bank, s) == m.rx_fec_of(s) && st.bits(bank, s) == m.rx_bits_of(s), "%s seq %ld step %d: fec / bits of stream %zu", what, seq, i, s);
            CHECK(st.stream_blocks(bank, s) == m.rx_stream_blocks(s), "%s seq %ld step %d: blocks of stream %zu", what, seq, i, s);
        }
        CHECK(st.fec_max(bank) == m.rx_fec_max() && st.fec_mixed() == m.rx_fec_mixed(), "%s seq %ld step %d: fec_max / fec_mixed", what, seq, i);
        CHECK(st.slot_blocks(bank) * RX_UDPSIZE == m.rx_frame_bytes(), "%s seq %ld step %d: slot bytes", what, seq, i);
        CHECK(st.version() == m.sm_version, "%s seq %ld step %d: version %llu / %llu", what, seq, i, (unsigned long long)st.version(), (unsigned long long)m.sm_version);
        CHECK((int)st.forces_ragged() == m.uniform_refused(), "%s seq %ld step %d: forces the ragged step", what, seq, i);
        if (m.rx_fec_mixed()) ++t->mixed;
        else if (!m.sf_fec.empty()) ++t->equal_fec;
        // ---- the records, and when they are formed
        const uint64_t formed0 = st.formed(), mformed0 = m.formed;
        const RxStreamRecords *r = st.records(bank);
        const unsigned *sw = m.rx_stream_words(m_decimated_sample_size((unsigned)m.cfg.log2decim, m.cfg.sample_bits));
        CHECK((r != nullptr) == (sw != nullptr) && (r != nullptr) == st.any(), "%s seq %ld step %d: records while %s array is set", what, seq, i, sw ? "an" : "no");
        if (r) {
            const bool due = !formed_once || st.version() != formed_version || !(bank == formed_bank);
            CHECK((st.formed() != formed0) == due && st.formed() - formed0 <= 1, "%s seq %ld step %d: formed %d, due %d", what, seq, i, (int)(st.formed() - formed0), (int)due);
            CHECK(m.formed == mformed0 || st.formed() != formed0, "%s seq %ld step %d: the model formed its records again, the type did not", what, seq, i);
            if (st.formed() != formed0) ++t->formed;
            else ++t->kept;
            formed_once = true; formed_version = st.version(); formed_bank = bank;
            // (the type forms them again for a bank-wide sample size that leaves the decimated size as it was -- the shifts it keeps
            // beside the words follow the size itself --, the model does not: changed() then says more than !sm_uploaded, never less)
            if (st.formed() != formed0) since_taken = true;
            CHECK(st.changed() == since_taken && (st.changed() || m.sm_uploaded), "%s seq %ld step %d: changed %d, formed since taken %d, uploaded %d", what, seq, i,
                  (int)st.changed(), (int)since_taken, (int)m.sm_uploaded);
            CHECK(r->words.size() == S * RX_STREAM_WORDS && r->w2.size() == S && r->shifts.size() == S, "%s seq %ld step %d: sizes", what, seq, i);
            CHECK(st.records(bank) == r && st.formed() - formed0 <= 1, "%s seq %ld step %d: asked twice, formed twice", what, seq, i);
        }
        for (size_t s = 0; s < S; ++s) { // the words of rx_ragged's row loop, with the shared record while no array is set
            unsigned row[5], mine[5], mw[6];
            m.rx_ragged_row(s, row);
            rx_meta_record(bank.center_frequency_khz, bank.sample_rate, bank.nb_fec, decimated_sample_size((unsigned)bank.log2decim, bank.sample_bits), mw);
            const unsigned *w = r ? &r->words[s * RX_STREAM_WORDS] : nullptr;
            mine[0] = w ? w[0] : mw[0]; mine[1] = w ? w[1] : mw[1]; mine[2] = w ? w[2] : mw[5];
            mine[3] = r ? r->w2[s] : mw[2];
            mine[4] = r ? r->shifts[s] : ragged_shift_word((unsigned)bank.log2decim, bank.sample_bits);
            CHECK(!memcmp(row, mine, sizeof(row)), "%s seq %ld step %d: row words of stream %zu: %08x %08x %08x %08x %08x / %08x %08x %08x %08x %08x", what, seq, i, s,
                  row[0], row[1], row[2], row[3], row[4], mine[0], mine[1], mine[2], mine[3], mine[4]);
        }
        if (r && rnd() % 3 == 0) { st.taken(); m.sm_uploaded = true; since_taken = false; } // (rx_stream_table has uploaded them)
    }

    // ---- the steps of a script
    void set_meta()
    {
        std::vector<uint32_t> fc(S), rate(S);
        for (size_t s = 0; s < S; ++s) { fc[s] = rnd() % 4 ? rnd() : 0xffffffffu; rate[s] = rnd(); }
        const uint32_t *a = rnd() % 3 ? fc.data() : nullptr, *b = rnd() % 3 ? rate.data() : nullptr;
        m.set_stream_meta(a, b);
        CHECK(st.set_meta(a, b).kind == RxSetResult::OK, "set_meta");
    }
    void set_fec()
    {
        static const int menu[6] = {0, 1, 31, 32, 33, 128};
        std::vector<int> v(S);
        const int same = menu[rnd() % 6];
        const unsigned kind = rnd() % 6; // 0: NULL, 1: equal counts, 2 .. 3: differing, 4 .. 5: one entry out of range
        for (size_t s = 0; s < S; ++s) v[s] = kind == 1 ? same : menu[rnd() % 6];
        if (kind >= 4) v[rnd() % 2 ? 0 : S - 1] = rnd() % 2 ? -1 : 129;
        const int *a = kind ? v.data() : nullptr;
        int most = -1;
        const Refused mr = m.set_stream_fec(a, &most);
        const RxSetResult adm = st.admit_fec(a);
        CHECK((adm.kind == RxSetResult::RANGE) == mr.is && (!mr.is || (adm.index == mr.index && adm.value == mr.value)), "admit_fec: %d [%zu] = %ld", (int)adm.kind, adm.index, adm.value);
        if (!mr.is) CHECK(st.slot_blocks_of(a, bank) == (size_t)(128 + most), "slot_blocks_of: %zu, most %d", st.slot_blocks_of(a, bank), most);
        const RxSetResult r = st.set_fec(a);
        CHECK(r.kind == adm.kind && r.index == adm.index && r.value == adm.value, "set_fec behind admit_fec");
        if (mr.is) ++t->refused;
    }
    void set_bits()
    {
        const unsigned L = (unsigned)m.cfg.log2decim, edge = 16 - L;
        std::vector<unsigned> v(S);
        const unsigned kind = rnd() % 6; // 0: NULL, 1 .. 3: sizes, 4 .. 5: one entry out of range
        for (size_t s = 0; s < S; ++s) {
            const unsigned pick = rnd() % 4;
            v[s] = pick == 0 ? 1 + rnd() % 16 : pick == 1 ? (edge > 1 ? edge - 1 : 1) : pick == 2 ? edge : (edge < 16 ? edge + 1 : 16);
        }
        if (kind >= 4) v[rnd() % 2 ? 0 : S - 1] = rnd() % 2 ? 0 : 17;
        const unsigned *a = kind ? v.data() : nullptr;
        const Refused mr = m.set_stream_bits(a);
        const RxSetResult r = st.set_bits(a);
        CHECK((r.kind == RxSetResult::RANGE) == mr.is && (!mr.is || (r.index == mr.index && r.value == mr.value)), "set_bits: %d [%zu] = %ld", (int)r.kind, r.index, r.value);
        if (mr.is) ++t->refused;
    }
    void change_bank()
    {
        static const int menu[6] = {0, 1, 31, 32, 33, 128};
        switch (rnd() % 7) {
        case 0: m.cfg.center_frequency_khz = rnd(); break;
        case 1: m.cfg.sample_rate = rnd(); break;
        case 2: m.cfg.nb_fec = menu[rnd() % 6]; break;
        case 3: m.cfg.sample_bits = 1 + rnd() % 16; break;
        case 4: m.cfg.log2decim = (int)(rnd() % 7); break;
        case 5: m.cfg.fcpos = (int)(rnd() % 3); break;
        default: break; // (sdrhip_rx_reconfigure with the values it has)
        }
        sync_bank();
    }
    void check_counts(const size_t *n_in, const char *what, long seq, int i, RxRaggedCounts *out)
    {
        const Model::Ragged a = m.rx_ragged_counts(area, n_in);
        RxRaggedCounts b = rx_ragged_counts(area, st, bank, n_in);
        CHECK(b.n_in == n_in && b.max_in == a.max_in && b.max_dec == a.max_dec && b.max_done == a.max_done && b.sum_done == a.sum_done && b.max_row == a.max_row,
              "%s seq %ld step %d: sums and maxima", what, seq, i);
        size_t bytes = 0;
        for (size_t s = 0; s < S; ++s) {
            const RxAdvance &x = a.adv[s], &y = b.adv[s];
            CHECK(x.done == y.done && x.rest == y.rest && x.first_new == y.first_new && x.started == y.started && x.idx0 == y.idx0 && x.frame_count0 == y.frame_count0,
                  "%s seq %ld step %d: advance of stream %zu", what, seq, i, s);
            CHECK(a.done[s] == b.done[s] && a.rest[s] == b.rest[s], "%s seq %ld step %d: done / rest of stream %zu", what, seq, i, s);
            bytes += a.done[s] * m.rx_stream_bytes(s);
            if (!n_in[s]) ++t->zero_in;
            else if (!a.done[s]) ++t->zero_done;
            else if (a.done[s] > 1) ++t->several;
            if (n_in[s] && area.open(s)) ++t->inside_open;
        }
        CHECK(b.bytes == bytes, "%s seq %ld step %d: delivered bytes %zu / %zu", what, seq, i, b.bytes, bytes);
        *out = b;
    }
    void ragged_step(long seq, int i)
    {
        static const size_t menu[8] = {0, 1, 5000, 16128, 16129, 16130, 3 * 16129 + 11, 9 * 16129 + 7}; // decimated samples
        std::vector<size_t> n_in(S);
        for (size_t s = 0; s < S; ++s) n_in[s] = (menu[rnd() % 8] << m.cfg.log2decim) + (rnd() & (((size_t)1 << m.cfg.log2decim) - 1));
        RxRaggedCounts n;
        check_counts(n_in.data(), "ragged", seq, i, &n);
        area.commit(n.done.data(), n.rest.data());
    }
    void datagram_step(long seq, int i)
    {
        std::vector<size_t> released(S);
        for (size_t s = 0; s < S; ++s) released[s] = rnd() % 3 == 0 ? 0 : rnd() % 5;
        const size_t U = m.rx_join_unit(); // (a reconfiguration may have changed it: what a row holds back can then exceed it)
        const Model::Join a = m.submit_batch(area, carry, released.data());
        const RxJoinCounts b = rx_join_counts(U, carry, released.data());
        CHECK(a.fed == b.fed && a.left == b.left && a.any == b.any, "join seq %ld step %d: fed / left / any", seq, i);
        RxRaggedCounts n;
        check_counts(b.fed.data(), "join", seq, i, &n);
        size_t max_done = 0, max_row = 0;
        m.admit(area, carry, released.data(), &max_done, &max_row);
        CHECK(n.max_done == max_done && n.max_row == max_row, "join seq %ld step %d: admit's max_done %zu / %zu, max_row %zu / %zu", seq, i, n.max_done, max_done, n.max_row, max_row);
        CHECK(n.sum_done == a.sum_done && n.bytes == a.b_frames, "join seq %ld step %d: submit's sum_done %zu / %zu, bytes %zu / %zu", seq, i, n.sum_done, a.sum_done, n.bytes, a.b_frames);
        if (U == 4 && m.cfg.log2decim == 1) ++t->unit4;
        area.commit(n.done.data(), n.rest.data());
        carry = b.left;
    }
};

void scripts(Tally *t)
{
    const size_t SS[4] = {1, 2, 8, 66};
    for (long seq = 0; seq < 1200; ++seq) {
        rng_state = 0x9e3779b97f4a7c15ull ^ (uint64_t)seq * 0x100000001b3ull;
        const size_t S = SS[seq % 4];
        const Cfg c = {rnd(), rnd(), (int)(rnd() % 129), 1 + rnd() % 16, (int)((seq / 4) % 7), (int)(rnd() % 3)};
        Pair p(S, c, t);
        p.compare("fresh", seq, -1);
        for (int i = 0; i < 40; ++i) {
            switch (rnd() % 8) {
            case 0: p.set_meta(); break;
            case 1: p.set_fec(); break;
            case 2: p.set_bits(); break;
            case 3: p.change_bank(); break;
            case 4: case 5: p.ragged_step(seq, i); break;
            default: p.datagram_step(seq, i); break;
            }
            p.compare("script", seq, i);
        }
    }
}

// the refusals at the first and the last index, spelled out: the old values stand and no version is counted
void refusals()
{
    const size_t SS[4] = {1, 2, 8, 66};
    const Cfg c = {100000, 48000, 8, 12, 3, 2};
    for (int si = 0; si < 4; ++si) {
        const size_t S = SS[si];
        Tally t = Tally();
        Pair p(S, c, &t);
        std::vector<int> fec(S, 32);
        std::vector<unsigned> bits(S, 8);
        fec[0] = 1; bits[S - 1] = 16;
        CHECK(p.st.set_fec(fec.data()).kind == RxSetResult::OK && p.st.set_bits(bits.data()).kind == RxSetResult::OK, "refusals: the values that stand");
        int most;
        (void)p.m.set_stream_fec(fec.data(), &most); (void)p.m.set_stream_bits(bits.data());
        p.compare("refusals", si, 0);
        const uint64_t v0 = p.st.version(), f0 = p.st.formed();
        const int bad_fec[2] = {-1, 129};
        const unsigned bad_bits[2] = {0, 17};
        for (int k = 0; k < 4; ++k) {
            const size_t at = k & 1 ? S - 1 : 0;
            std::vector<int> f2(S, 0);
            std::vector<unsigned> b2(S, 1);
            f2[at] = bad_fec[k >> 1]; b2[at] = bad_bits[k >> 1];
            const RxSetResult a = p.st.admit_fec(f2.data()), rf = p.st.set_fec(f2.data()), rb = p.st.set_bits(b2.data());
            CHECK(a.kind == RxSetResult::RANGE && rf.kind == RxSetResult::RANGE && rf.index == at && rf.value == bad_fec[k >> 1], "refusals: fec[%zu] = %d", at, bad_fec[k >> 1]);
            CHECK(rb.kind == RxSetResult::RANGE && rb.index == at && rb.value == (long)bad_bits[k >> 1], "refusals: bits[%zu] = %u", at, bad_bits[k >> 1]);
            p.compare("refusals", si, 1 + k); // (the model was not told: its values are the old ones)
        }
        CHECK(p.st.version() == v0 && p.st.formed() == f0, "refusals: a refused setter counted a version or formed the records");
    }
}

// records for the third witness: what the type forms for these settings, as the 24 bytes of the zero-stamp record
void print_records()
{
    const Cfg c = {433920, 250000, 8, 12, 0, 2};
    const uint32_t fc[4] = {0, 1, 1296000, 0xffffffffu}, rate[4] = {1, 48000, 0x80000000u, 31250};
    const int fec[4] = {0, 1, 33, 128};
    const unsigned bits[4] = {1, 8, 12, 16};
    for (int L = 0; L <= 6; L += 2) {
        Tally t = Tally();
        Pair p(4, c, &t);
        p.m.cfg.log2decim = L;
        p.sync_bank();
        CHECK(p.st.set_meta(fc, rate).kind == RxSetResult::OK && p.st.set_fec(fec).kind == RxSetResult::OK, "print_records: setters");
        if (L) CHECK(p.st.set_bits(bits).kind == RxSetResult::OK, "print_records: set_bits"); // (L = 0: the bank's 12 bits)
        const RxStreamRecords *r = p.st.records(p.bank);
        for (size_t s = 0; r && s < 4; ++s) {
            const unsigned w[6] = {r->words[s * 3], r->words[s * 3 + 1], r->w2[s], 0, 0, r->words[s * 3 + 2]};
            uint8_t m[24];
            memcpy(m, w, 24);
            printf("RECORD log2decim %d fc %u rate %u nb_fec %d bits %u : ", L, fc[s], rate[s], fec[s], L ? bits[s] : c.sample_bits);
            for (int k = 0; k < 24; ++k) printf("%02x", m[k]);
            printf("\n");
        }
    }
}
} // namespace

int main()
{
    Tally t = Tally();
    scripts(&t);
    refusals();
    print_records();
    printf("streams at count 0: %ld, completing no frame: %ld, several frames: %ld, windows inside an open frame: %ld, joins of unit 4: %ld\n", t.zero_in, t.zero_done,
           t.several, t.inside_open, t.unit4);
    printf("setters refused: %ld, records formed: %ld, kept: %ld, steps with differing fecblk: %ld, with equal fecblk: %ld\n", t.refused, t.formed, t.kept, t.mixed, t.equal_fec);
    CHECK(t.zero_in && t.zero_done && t.several && t.inside_open && t.unit4 && t.refused && t.formed && t.kept && t.mixed && t.equal_fec, "a case the scripts must reach was not reached");
    if (failures) { printf("%d mismatches\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
