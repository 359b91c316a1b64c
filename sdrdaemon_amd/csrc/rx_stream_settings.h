// rx_stream_settings.h -- the per-stream settings of an Rx bank (sdrhip_rx_set_stream_meta / _fec / _bits / _format): which value is in force
// for stream s, what a set array forces, the streams' zero-stamp records -- and the counts of a ragged step and of a datagram join:
// what the streams will complete and deliver for given sample counts.  Pure arithmetic (no HIP, no library header; the frame
// area beside it is the only neighbour it sees): sdrhip_rx.cpp and the asynchronous / datagram units ask it,
// tests/cxx/rx_stream_settings_test.cpp replays it on a CPU.  Its sample-size functions are marked for both sides under hipcc
// (RX_HD): KFb, the kernel of sdrhip_rx_set_follow_bits, runs them on the device; tests/cxx/rx_follow_bits_rule_test.cpp on a CPU.
#pragma once
#include "rx_frame_area.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <new>
#include <tuple>
#include <utility>
#include <vector>

namespace sdrhip {
constexpr size_t RX_NB_ORIGINAL = 128;    // original super blocks of a frame (SDRHIP_NB_ORIGINAL)
constexpr size_t RX_UDPSIZE = 512;        // bytes of a super block (SDRHIP_UDPSIZE)
constexpr size_t RX_STREAM_WORDS = 3;     // words per stream of the uniform step's device table (STREAM_META_WORDS)

// ---- the sample-size arithmetic, ONE text for the host and for KFb (rx_follow_bits_kernels.hip, the one kernel file that includes
// this header): RX_HD is empty without hipcc, so the CPU programs under tests/cxx run the code the kernel runs
#if defined(__HIPCC__)
#define RX_HD __host__ __device__
#else
#define RX_HD
#endif

// sampleSize after decimateN (Decimators.cpp:43-44, 112-113 ...): grows by log2decim, capped at 16 bits
RX_HD inline unsigned decimated_sample_size(unsigned log2decim, unsigned ss)
{
    if (log2decim == 0) return ss;
    const unsigned target = 16 - log2decim, trunk = ss < target ? 0 : ss - target;
    return ss + log2decim - trunk;
}
// ... and the output shift that gets it there, the one place the sample size enters a cascade: `x << norm >> trunk` in front of the
// int16 truncation (Decimators.cpp:27-32 decimate1: norm = 16 - ss; :43-44, 52-53, 62 and every decimateN: up to 16 - log2decim bits
// by norm, beyond them by trunk)
struct DecimShifts { unsigned norm, trunk; };
RX_HD inline DecimShifts decimated_shifts(unsigned log2decim, unsigned ss)
{
    const unsigned target = 16 - log2decim;
    const DecimShifts r = {ss < target ? target - ss : 0, ss < target ? 0 : ss - target};
    return r;
}
// the pair as a ragged launch's rows carry it (RaggedRow::shifts)
RX_HD inline unsigned ragged_shift_word(unsigned log2decim, unsigned ss)
{
    const DecimShifts sh = decimated_shifts(log2decim, ss);
    return sh.norm | (sh.trunk << 8);
}

// ---- the sample size followed from the incoming meta blocks (sdrhip_rx_set_follow_bits).  `in_w2` is the third word of the
// collector's m_outputMeta: m_sampleBytes, m_sampleBits, m_nbOriginalBlocks, m_nbFECBlocks from byte 0 up.  Only byte 1 is read
// (the indicator nibble of m_sampleBytes is the sender's business); a size outside 1..16 -- MetaDataFEC::init()'s 0 before the
// first block 0 is released, a sender that says 0, one that says more than an IQSample holds -- is no incoming size
RX_HD inline bool followed_sample_bits(unsigned in_w2, unsigned *bits)
{
    *bits = (in_w2 >> 8) & 0xffu;
    return *bits >= 1 && *bits <= 16;
}
// the third word of a stream's record with sampleBytes / sampleBits of the decimated size ssd (sdrdaemonrx.cpp:642-643) in bytes 0
// and 1; bytes 2 and 3 (128 and the stream's own nbFECBlocks) stay
RX_HD inline unsigned meta_w2_with_size(unsigned w2, unsigned ssd)
{
    return (w2 & 0xffff0000u) | ((ssd & 0xffu) << 8) | (((ssd - 1) / 8 + 1) & 0xffu);
}
// boost::crc_32_type over the little-endian bytes of `w`, 32 bit steps, and over the zero-stamp record {fc, rate, w2, 0, 0}
// (UDPSinkFEC.cpp:106-109; the byte-wise statement: rx_meta_record below)
RX_HD inline unsigned meta_crc_word(unsigned crc, unsigned w)
{
    crc ^= w;
    for (int k = 0; k < 32; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    return crc;
}
RX_HD inline unsigned meta_record_crc(unsigned fc, unsigned rate, unsigned w2)
{
    unsigned crc = 0xFFFFFFFFu;
    crc = meta_crc_word(crc, fc);
    crc = meta_crc_word(crc, rate);
    crc = meta_crc_word(crc, w2);
    crc = meta_crc_word(crc, 0u); // tv_sec
    crc = meta_crc_word(crc, 0u); // tv_usec
    return crc ^ 0xFFFFFFFFu;
}
// what KFb writes into a stream's row: the pair for (log2decim, b), the third word with b' = decimated_sample_size(log2decim, b),
// and the zero-stamp CRC of {fc, rate, that word}.  false (nothing formed): the stream has no incoming size
struct FollowedSize { unsigned shifts, w2, crc0; };
RX_HD inline bool followed_size_words(unsigned in_w2, unsigned log2decim, unsigned fc, unsigned rate, unsigned w2, FollowedSize *f)
{
    unsigned b;
    if (!followed_sample_bits(in_w2, &b)) return false;
    f->shifts = ragged_shift_word(log2decim, b);
    f->w2 = meta_w2_with_size(w2, decimated_sample_size(log2decim, b));
    f->crc0 = meta_record_crc(fc, rate, f->w2);
    return true;
}

// the 24-byte MetaDataFEC record (UDPSinkFEC.cpp:87-132) with a ZERO stamp, and in w[5] the boost::crc_32_type over its first 20
// bytes (:106-109): the affine part of every frame's CRC.  A frame's own stamp (the reference calls gettimeofday when it opens the
// frame, :90-104) is the call's plus its first sample's offset on the sample clock: w[3], w[4] and the CRC follow per frame on the
// device (frame_meta_words)
inline void rx_meta_record(uint32_t fc, uint32_t sr, int nb_fec, unsigned ssd, unsigned w[6])
{
    uint8_t m[24];
    memcpy(m + 0, &fc, 4); memcpy(m + 4, &sr, 4);
    m[8] = (uint8_t)((ssd - 1) / 8 + 1); // setSampleBytes((sampleSize - 1) / 8 + 1), sdrdaemonrx.cpp:643
    m[9] = (uint8_t)ssd;                 // setSampleBits(sampleSize), :642
    m[10] = (uint8_t)RX_NB_ORIGINAL; m[11] = (uint8_t)nb_fec;
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

// the bank-wide values (the configuration's): what serves a stream while the array of that setting is not set
struct RxBankValues {
    uint32_t center_frequency_khz, sample_rate;
    int nb_fec;
    unsigned sample_bits;
    int log2decim;
    bool operator==(const RxBankValues &o) const
    {
        return std::tie(center_frequency_khz, sample_rate, nb_fec, sample_bits, log2decim) == std::tie(o.center_frequency_khz, o.sample_rate, o.nb_fec, o.sample_bits, o.log2decim);
    }
};

enum RxSetting { RX_SET_NONE = 0, RX_SET_FEC, RX_SET_BITS, RX_SET_FORMAT };
// what a setter says.  RANGE: entry `index` = `value` is out of range; NO_MEMORY; either way the old values stand
struct RxSetResult {
    enum Kind { OK = 0, RANGE, NO_MEMORY } kind;
    size_t index;
    long value;
};

// the streams' records as the launches take them: {fc, rate, zero-stamp CRC} per stream (words, RX_STREAM_WORDS each: the uniform
// step's device table as it goes up), word 2 of each stream's record (sampleBytes, sampleBits, 128, nbFECBlocks) and its output
// shift (ragged_shift_word): the ragged rows' words
struct RxStreamRecords {
    std::vector<unsigned> words, w2, shifts;
};

class RxStreamSettings {
public:
    void init(size_t nstreams) { S_ = nstreams; }

    // ---- setters: an array of one value per stream, NULL = bank-wide again.  Range, then room, then the values: nothing can fail
    // between the first value that changes and the last.  Every call that sets counts as a new version
    RxSetResult set_meta(const uint32_t *center_frequency_khz, const uint32_t *sample_rate)
    {
        if (!room(fc_, center_frequency_khz) || !room(rate_, sample_rate)) return {RxSetResult::NO_MEMORY, 0, 0};
        put(fc_, center_frequency_khz);
        put(rate_, sample_rate);
        ++version_;
        return {RxSetResult::OK, 0, 0};
    }
    RxSetResult set_fec(const int *nb_fec) { return set(fec_, nb_fec, 0, 128, true); }
    RxSetResult set_bits(const unsigned *sample_bits) { return set(bits_, sample_bits, 1u, 16u, true); }
    // (the sample-fed entries' input format per stream, 0 / 1 / 2 = SDRHIP_IQ_S16 / _U8 / _S8: configuration of the input side alone,
    // no part of the streams' records -- the version stays)
    RxSetResult set_format(const int *fmt) { return set(fmt_, fmt, 0, 2, true, false); }
    // (the frame area's slots follow the largest count: admit_fec is set_fec without the change, for a caller that has to move the
    // open frames to slots of slot_blocks_of(nb_fec, bank) in between -- set_fec behind it cannot fail)
    RxSetResult admit_fec(const int *nb_fec) { return set(fec_, nb_fec, 0, 128, false); }
    uint64_t version() const { return version_; }

    // ---- the value in force for stream s
    uint32_t fc(const RxBankValues &b, size_t s) const { return fc_.empty() ? b.center_frequency_khz : fc_[s]; }
    uint32_t rate(const RxBankValues &b, size_t s) const { return rate_.empty() ? b.sample_rate : rate_[s]; }
    int fec(const RxBankValues &b, size_t s) const { return fec_.empty() ? b.nb_fec : fec_[s]; }
    unsigned bits(const RxBankValues &b, size_t s) const { return bits_.empty() ? b.sample_bits : bits_[s]; }
    int format(int bank_fmt, size_t s) const { return fmt_.empty() ? bank_fmt : fmt_[s]; }
    const int *formats() const { return fmt_.empty() ? nullptr : fmt_.data(); } // NULL: the bank-wide format serves every stream
    // per-stream fecblk: the largest count of the bank, whether two streams differ, the super blocks of a slot of the frame area (the
    // ONE pitch; slot_blocks_of: once nb_fec is set) and of the valid head of a frame of stream s
    int fec_max(const RxBankValues &b) const { return fec_.empty() ? b.nb_fec : *std::max_element(fec_.begin(), fec_.end()); }
    bool fec_mixed() const { return std::adjacent_find(fec_.begin(), fec_.end(), std::not_equal_to<int>()) != fec_.end(); }
    size_t slot_blocks(const RxBankValues &b) const { return RX_NB_ORIGINAL + (size_t)fec_max(b); }
    size_t slot_blocks_of(const int *nb_fec, const RxBankValues &b) const { return RX_NB_ORIGINAL + (size_t)(nb_fec ? *std::max_element(nb_fec, nb_fec + S_) : b.nb_fec); }
    size_t stream_blocks(const RxBankValues &b, size_t s) const { return RX_NB_ORIGINAL + (size_t)fec(b, s); }

    // ---- what the arrays force: any() = the streams have records of their own; while the fecblk, the sample-size or the format array
    // is set every step is the ragged step (the one named is the first of the three that is set)
    bool any() const { return !fc_.empty() || !rate_.empty() || !fec_.empty() || !bits_.empty(); }
    RxSetting forces_ragged() const { return !fec_.empty() ? RX_SET_FEC : !bits_.empty() ? RX_SET_BITS : !fmt_.empty() ? RX_SET_FORMAT : RX_SET_NONE; }

    // ---- the streams' records for the frames the next launch opens; NULL while no array is set (the shared record of the bank-wide
    // values serves every stream).  Formed again only when a setter was called or a bank-wide value has changed since they were formed
    const RxStreamRecords *records(const RxBankValues &b)
    {
        if (!any()) return nullptr;
        const std::pair<uint64_t, RxBankValues> key(version_, b);
        if (!(key == key_)) {
            rec_.words.resize(S_ * RX_STREAM_WORDS);
            rec_.w2.resize(S_);
            rec_.shifts.resize(S_);
            for (size_t s = 0; s < S_; ++s) {
                unsigned w[6];
                rx_meta_record(fc(b, s), rate(b, s), fec(b, s), decimated_sample_size((unsigned)b.log2decim, bits(b, s)), w);
                unsigned *t = &rec_.words[s * RX_STREAM_WORDS];
                t[0] = w[0]; t[1] = w[1]; t[2] = w[5];
                rec_.w2[s] = w[2];
                rec_.shifts[s] = ragged_shift_word((unsigned)b.log2decim, bits(b, s));
            }
            key_ = key;
            changed_ = true;
            ++formed_;
        }
        return &rec_;
    }
    // the records were formed again since taken() was last called (the uniform step's device table: it holds what was taken)
    bool changed() const { return changed_; }
    void taken() { changed_ = false; }
    uint64_t formed() const { return formed_; } // how often the records were formed

private:
    template <class T> bool room(std::vector<T> &to, const T *v)
    {
        try {
            if (v) to.reserve(S_);
        } catch (const std::bad_alloc &) {
            return false;
        }
        return true;
    }
    template <class T> void put(std::vector<T> &to, const T *v) // (behind room(): cannot fail)
    {
        if (v) to.assign(v, v + S_);
        else to.clear();
    }
    template <class T> RxSetResult set(std::vector<T> &to, const T *v, T lo, T hi, bool change, bool versioned = true)
    {
        for (size_t s = 0; v && s < S_; ++s)
            if (v[s] < lo || v[s] > hi) return {RxSetResult::RANGE, s, (long)v[s]};
        if (!room(to, v)) return {RxSetResult::NO_MEMORY, 0, 0};
        if (change) put(to, v);
        version_ += change && versioned ? 1 : 0;
        return {RxSetResult::OK, 0, 0};
    }

    size_t S_ = 0;
    std::vector<uint32_t> fc_, rate_; // empty: the field is bank-wide
    std::vector<int> fec_;
    std::vector<unsigned> bits_;
    std::vector<int> fmt_;
    uint64_t version_ = 0;            // counts the setters' calls
    std::pair<uint64_t, RxBankValues> key_ = {~(uint64_t)0, RxBankValues()}; // what rec_ was formed for
    RxStreamRecords rec_;
    bool changed_ = false;
    uint64_t formed_ = 0;
};

// ---- what a ragged step does for the counts n_in[s] (samples in front of the decimator): every caller that sizes a buffer, refuses
// a delivery or runs the step reads the ONE value.  It holds until the area commits a step (windows that move leave it as it is)
struct RxRaggedCounts {
    const size_t *n_in;         // the counts it was made from (the caller's array)
    std::vector<RxAdvance> adv; // per stream: what its decimated samples do to it,
    std::vector<size_t> done;   // the frames it completes
    std::vector<uint64_t> rest; // and the samples left in the frame that stays open
    size_t max_in, max_dec, max_done, sum_done;
    size_t max_row; // bytes of the longest dense delivery of a stream (its frames, 128 + its own fecblk super blocks each)
    size_t bytes;   // exactly the delivered bytes of all streams
};
inline RxRaggedCounts rx_ragged_counts(const RxFrameArea &area, const RxStreamSettings &st, const RxBankValues &b, const size_t *n_in)
{
    const size_t S = area.streams();
    RxRaggedCounts n = {n_in, std::vector<RxAdvance>(S), std::vector<size_t>(S), std::vector<uint64_t>(S), 0, 0, 0, 0, 0, 0};
    for (size_t s = 0; s < S; ++s) {
        const size_t n_dec = n_in[s] >> b.log2decim;
        n.adv[s] = area.advance(s, n_dec);
        const size_t done = n.done[s] = n.adv[s].done, row = done * st.stream_blocks(b, s) * RX_UDPSIZE;
        n.rest[s] = n.adv[s].rest;
        if (n_in[s] > n.max_in) n.max_in = n_in[s];
        if (n_dec > n.max_dec) n.max_dec = n_dec;
        if (done > n.max_done) n.max_done = done;
        if (row > n.max_row) n.max_row = row;
        n.sum_done += done;
        n.bytes += row;
    }
    return n;
}

// ---- the datagram entries' join: a stream holds `carry` samples back and releases `released` frames behind them; the largest
// multiple of `unit` (rx_join_unit) goes through the decimator now, the rest is held back again
struct RxJoinCounts {
    std::vector<size_t> fed, left;
    bool any; // a stream feeds its decimator
};
inline RxJoinCounts rx_join_counts(size_t unit, const std::vector<size_t> &carry, const size_t *released)
{
    RxJoinCounts j = {std::vector<size_t>(carry.size()), std::vector<size_t>(carry.size()), false};
    for (size_t s = 0; s < carry.size(); ++s) {
        const size_t total = carry[s] + released[s] * (size_t)RX_FRAME_SAMPLES;
        j.fed[s] = total / unit * unit;
        j.left[s] = total - j.fed[s];
        j.any = j.any || j.fed[s] != 0;
    }
    return j;
}
} // namespace sdrhip
