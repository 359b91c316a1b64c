// rx_depart_order.h -- the run order: the round-robin departure order of a batch the Rx pipe delivers as ONE datagram array
// (sdrhip_rx_set_egress, SDRHIP_EGRESS_ROUND_ROBIN).  Stream s delivered F_s frames of B_s datagrams, D_s = F_s B_s of them in the
// reference's wire order (frame after frame, blocks 0 .. B_s - 1 inside a frame, UDPSinkFEC.cpp:259).  The array is rounds
// j = 0, 1, 2, ... concatenated; round j holds datagram j of every stream with D_s > j, streams ascending:
//     pos(s, j) = sum_t min(D_t, j) + #{t < s : D_t > j}.
// Between two consecutive values of {D_t} the set of streams still sending is constant: for lo <= j < hi (lo, hi consecutive
// values, lo = 0 first) with A = #{t : D_t >= hi} and P = sum_t min(D_t, lo)
//     pos(s, j) = P + (j - lo) A + #{t < s : D_t >= hi},
// affine in j.  So the array is moved as runs (src, dst, stride, count), each inside one frame and one such interval; KR
// (rx_runs_kernels.hip) moves a run.
//   * Equal frames (B_s = B, the pipe's fecblk): every D_t is a multiple of B, so the intervals end on frame boundaries and no
//     frame is cut -- exactly one run per delivered frame, count = B.  With A_f = #{t : F_t > f}, r_f(s) = #{t < s : F_t > f} and
//     base_f = B sum_{g<f} A_g frame f of stream s goes to (base_f + r_f(s)) + b A_f, b < B.
//   * Frames of different lengths (per-stream fecblk, sdrhip_rx_set_stream_fec: B_s = 128 + nb_fec[s]): a stream's last datagram
//     can fall inside another stream's frame, which splits there.  At most sum_s F_s + S (S - 1) runs (every value of {D_t} cuts at
//     most one frame of each other stream).
// B_s <= 256 (the pipe never has more: 128 + nb_fec, nb_fec <= 128), so no run is longer than 256 datagrams = 8 workgroups, and
// the grid is checked as (runs at most) x 8 < 2^31 before anything is sized, a stream's frames as F_s x 256 < 2^31.  For equal
// frames that refuses 2^23 frames of one stream and 2^28 of a batch, more than the grid alone (frames x ceil(B / 32)) would: no
// batch that can exist lies there (a frame is at least 64 KiB: 2^23 of them are 512 GiB, 2^28 are 16 TiB).
// Pure host arithmetic (no HIP, no library header): sdrhip_rx_egress.cpp builds KR's table and the tags from it,
// tests/cxx/rx_egress_order_test.cpp (equal frames) and tests/cxx/rx_depart_order_test.cpp replay it on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rx_egress_limits.h"

namespace sdrhip {
constexpr uint32_t RX_DEPART_WG_DGRAMS = RX_EGRESS_WG_DGRAMS; // (KR's name for its workgroup's share)
constexpr uint32_t RX_DEPART_MAX_COUNT = 256;  // datagrams of a run at most (= the longest frame, 128 + 128)

// one run for KR: `count` datagrams back to back at `src` (bytes into the frame area) go to dst + i * stride (bytes into the
// departure-order array), i < count; src, dst and stride are multiples of 16
struct RxDepartRun {
    uint64_t src, dst;
    uint32_t stride, count;
};

class RxDepartOrder {
public:
    // F[s] = frames stream s delivered, B[s] = datagrams of each of them.  false (nothing usable afterwards): no stream or more
    // than 65535, a B outside 1..256, or a batch whose runs x workgroups per run pass KR's 31-bit grid
    bool plan(const size_t *F, const size_t *B, size_t nstreams) { return plan_(F, B, 0, nstreams); }
    // ... every frame of the batch holds blocks_per_frame datagrams: one run per delivered frame
    bool plan(const size_t *F, size_t blocks_per_frame, size_t nstreams) { return plan_(F, nullptr, blocks_per_frame, nstreams); }
    size_t streams() const { return ok_ ? D_.size() : 0; }
    uint64_t dgrams() const { return ok_ ? total_ : 0; }                 // entries of the array
    uint64_t dgrams(size_t s) const { return D_[s]; }                    // D_s
    size_t blocks(size_t s) const { return B_[s]; }                      // B_s
    size_t nruns() const { return ok_ ? run_s_.size() : 0; }
    uint32_t max_count() const { return ok_ ? max_count_ : 0; }          // datagrams of the longest run
    uint32_t wg_per_run() const { return (max_count() + RX_DEPART_WG_DGRAMS - 1) / RX_DEPART_WG_DGRAMS; }
    uint64_t grid() const { return (uint64_t)nruns() * wg_per_run(); }   // KR's workgroups for the runs
    // run k: stream, its first datagram j (counted over the stream's D_s), datagrams, first position, positions between two
    size_t run_stream(size_t k) const { return run_s_[k]; }
    uint64_t run_first(size_t k) const { return run_j_[k]; }
    uint32_t run_count(size_t k) const { return run_n_[k]; }
    uint64_t run_pos(size_t k) const { return run_pos_[k]; }
    uint32_t run_alive(size_t k) const { return run_a_[k]; }
    // the definition, evaluated for one datagram (j < D_s)
    uint64_t pos(size_t s, uint64_t j) const
    {
        const size_t i = (size_t)(std::upper_bound(hi_.begin(), hi_.end(), j) - hi_.begin()); // first interval with hi > j
        uint64_t rank = 0;
        for (size_t t = 0; t < s; ++t) rank += D_[t] >= hi_[i] ? 1u : 0u;
        return first_[i] + (j - (i ? hi_[i - 1] : 0)) * alive_[i] + rank;
    }
    // stream_of[i] for the dgrams() entries of the array
    void tags(uint16_t *stream_of) const
    {
        if (!ok_) return;
        // front to back: an interval's round (the streams still sending, ascending) once, then block copies of what is there
        uint16_t *o = stream_of;
        for (size_t i = 0; i < hi_.size(); ++i) {
            const uint16_t *round = o;
            for (size_t s = 0; s < D_.size(); ++s)
                if (D_[s] >= hi_[i]) *o++ = (uint16_t)s;
            const uint16_t *end = round + (hi_[i] - (i ? hi_[i - 1] : 0)) * alive_[i];
            while (o < end) o = std::copy(round, round + std::min(o - round, end - o), o);
        }
    }
    // KR's table, nruns() entries: src0[s] = bytes into the frame area at which stream s's delivered frames begin, one every
    // pitch_bytes (the area's slot pitch), B_s datagrams valid in each.  false: an offset or a pitch that is no multiple of 16
    bool runs(const uint64_t *src0, uint64_t pitch_bytes, RxDepartRun *out) const
    {
        if (pitch_bytes & 15u) return false;
        for (size_t k = 0; k < run_s_.size(); ++k) {
            const size_t s = run_s_[k];
            if (src0[s] & 15u) return false;
            const uint64_t f = run_j_[k] / B_[s], b = run_j_[k] - f * B_[s];
            out[k].src = src0[s] + f * pitch_bytes + b * RX_EGRESS_DGRAM_BYTES;
            out[k].dst = run_pos_[k] * RX_EGRESS_DGRAM_BYTES;
            out[k].stride = (uint32_t)(run_a_[k] * RX_EGRESS_DGRAM_BYTES);
            out[k].count = run_n_[k];
        }
        return true;
    }

private:
    bool plan_(const size_t *F, const size_t *B, size_t B_all, size_t nstreams)
    {
        ok_ = false;
        if (!nstreams || nstreams > RX_EGRESS_MAX_STREAMS) return false;
        const size_t S = nstreams;
        uint64_t total = 0, frames = 0;
        for (size_t s = 0; s < S; ++s) {
            const size_t b = B ? B[s] : B_all;
            if (!b || b > RX_DEPART_MAX_COUNT || F[s] > 0x7fffffffu / RX_DEPART_MAX_COUNT) return false;
            total += (uint64_t)F[s] * b; frames += F[s];
        }
        // (every run takes at most 8 workgroups; equal frames are never cut)
        if ((frames + (B ? (uint64_t)S * (S - 1) : 0)) * (RX_DEPART_MAX_COUNT / RX_DEPART_WG_DGRAMS) > 0x7fffffffu) return false;
        D_.resize(S); B_.resize(S);
        for (size_t s = 0; s < S; ++s) {
            B_[s] = B ? B[s] : B_all;
            D_[s] = (uint64_t)F[s] * B_[s];
        }
        hi_.clear();
        for (size_t s = 0; s < S; ++s) if (D_[s]) hi_.push_back(D_[s]);
        std::sort(hi_.begin(), hi_.end());
        hi_.erase(std::unique(hi_.begin(), hi_.end()), hi_.end());
        const size_t I = hi_.size();
        alive_.assign(I, 0); first_.assign(I, 0);
        for (size_t i = 0; i < I; ++i) {
            const uint64_t lo = i ? hi_[i - 1] : 0;
            uint64_t P = 0;
            uint32_t A = 0;
            for (size_t s = 0; s < S; ++s) { P += D_[s] < lo ? D_[s] : lo; A += D_[s] >= hi_[i] ? 1u : 0u; }
            first_[i] = P; alive_[i] = A;
        }
        // the runs, interval by interval (one rank pass per interval), streams ascending inside, cut at the frames' ends
        run_s_.clear(); run_j_.clear(); run_n_.clear(); run_pos_.clear(); run_a_.clear();
        max_count_ = 0;
        for (size_t i = 0; i < I; ++i) {
            const uint64_t lo = i ? hi_[i - 1] : 0, hi = hi_[i];
            uint32_t rank = 0;
            for (size_t s = 0; s < S; ++s) {
                if (D_[s] < hi) continue;
                for (uint64_t j = lo; j < hi;) {
                    const uint64_t frame_end = (j / B_[s] + 1) * B_[s];
                    const uint64_t end = frame_end < hi ? frame_end : hi;
                    run_s_.push_back((uint32_t)s); run_j_.push_back(j); run_n_.push_back((uint32_t)(end - j));
                    run_pos_.push_back(first_[i] + (j - lo) * alive_[i] + rank); run_a_.push_back(alive_[i]);
                    max_count_ = (uint32_t)(end - j) > max_count_ ? (uint32_t)(end - j) : max_count_;
                    j = end;
                }
                ++rank;
            }
        }
        total_ = total;
        ok_ = true;
        return true;
    }

    bool ok_ = false;
    uint64_t total_ = 0;
    uint32_t max_count_ = 0;
    std::vector<uint64_t> D_;      // [S]
    std::vector<size_t> B_;        // [S]
    std::vector<uint64_t> hi_;     // the distinct non-zero D_t, ascending: interval i is [hi_[i - 1], hi_[i])
    std::vector<uint32_t> alive_;  // [intervals] A
    std::vector<uint64_t> first_;  // [intervals] P
    std::vector<uint32_t> run_s_, run_n_, run_a_;
    std::vector<uint64_t> run_j_, run_pos_;
};
} // namespace sdrhip
