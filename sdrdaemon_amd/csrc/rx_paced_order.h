// rx_paced_order.h -- the paced departure order of a batch the Rx pipe delivers as ONE datagram array (sdrhip_rx_set_egress,
// SDRHIP_EGRESS_PACED).  Stream s delivers D_s datagrams in the reference's wire order (frame after frame, blocks 0 .. B_s - 1
// inside a frame, UDPSinkFEC.cpp:259): D_s = F_s B_s, B_s the same for every stream unless sdrhip_rx_set_stream_fec made them
// differ.  A sender that spaces its D_s datagrams evenly over the batch period (what every sdrdaemonrx process does with txDelay,
// UDPSinkFEC.cpp:259-282) puts datagram j at the midpoint of its share of the period: the departure key
//     k(s, j) = (2 j + 1) / (2 D_s).
// The array lists all datagrams by ascending key, ties by ascending stream.  Keys are compared exactly, as the 64-bit cross products
// (2 j + 1) D_t against (2 i + 1) D_s: D_s < 2^31 is required, so a product stays below 2^63.  No floating point anywhere.
// Closed form (floor divisions; a stream with D_t = 0 contributes nothing):
//     pos(s, j) = j + sum_{t<s} min(D_t, ((2 j + 1) D_t / D_s + 1) / 2) + sum_{t>s} min(D_t, (((2 j + 1) D_t - 1) / D_s + 1) / 2)
// (the datagrams i of t with (2 i + 1) D_s <= (2 j + 1) D_t for t < s, < for t > s).
// What follows from it:
//   * equal counts give exactly the round-robin array of rx_depart_order.h (all keys of a round coincide, the tie rule orders it);
//   * the no-burst guarantee: between two consecutive datagrams of stream s lie floor(D_t / D_s) or ceil(D_t / D_s) datagrams of
//     every other stream t, never more and never fewer (the keys of s are 1 / D_s apart, those of t 1 / D_t).
// The destinations of a stream are no constant-stride runs, so KP (rx_paced_kernels.hip) is a gather keyed by destination: table
// entry i = the source of the array's datagram i in 16-byte units into the frame area.  Tags and table come out of ONE merge over
// the streams: streams with the same D_s share their keys and form a group, the groups are merged through a binary heap -- O(n)
// for equal counts, O(n log S) at most.
// Pure host arithmetic (no HIP, no library header): sdrhip_rx_egress.cpp builds KP's table and the tags from it,
// tests/cxx/rx_paced_order_test.cpp replays it on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rx_egress_limits.h"

namespace sdrhip {
constexpr uint64_t RX_PACED_MAX_STREAM_DGRAMS = 0x7fffffffu; // D_s at most: the cross products fit 64 bits
constexpr uint64_t RX_PACED_MAX_DGRAMS = (uint64_t)0x7fffffffu * RX_EGRESS_WG_DGRAMS; // KP's grid has 31 bits

class RxPacedOrder {
public:
    // F[s] = frames stream s delivered, B[s] = datagrams of each of them.  false (nothing usable afterwards): no stream or more
    // than 65535, a B[s] of 0, a D_s >= 2^31, or a total whose workgroups pass KP's 31-bit grid -- checked on the sums before
    // anything is sized; nothing is truncated
    bool plan(const size_t *F, const size_t *B, size_t nstreams) { return plan_(F, B, 0, nstreams); }
    // ... every frame of the batch holds blocks_per_frame datagrams
    bool plan(const size_t *F, size_t blocks_per_frame, size_t nstreams) { return plan_(F, nullptr, blocks_per_frame, nstreams); }

    size_t streams() const { return ok_ ? D_.size() : 0; }
    uint64_t dgrams() const { return ok_ ? total_ : 0; }   // entries of the array
    uint64_t dgrams(size_t s) const { return D_[s]; }      // D_s
    size_t blocks(size_t s) const { return B_[s]; }        // B_s
    uint64_t grid() const { return (dgrams() + RX_EGRESS_WG_DGRAMS - 1) / RX_EGRESS_WG_DGRAMS; } // KP's workgroups for the datagrams

    // the closed form, evaluated for one datagram (j < D_s)
    uint64_t pos(size_t s, uint64_t j) const
    {
        const uint64_t Ds = D_[s], k = 2 * j + 1;
        uint64_t p = j;
        for (size_t t = 0; t < D_.size(); ++t) {
            const uint64_t Dt = D_[t];
            if (t == s || !Dt) continue;
            const uint64_t c = t < s ? (k * Dt / Ds + 1) / 2 : ((k * Dt - 1) / Ds + 1) / 2;
            p += c < Dt ? c : Dt;
        }
        return p;
    }

    // stream_of[i] for the dgrams() entries of the array
    void tags(uint16_t *stream_of) { merge_(stream_of, nullptr, nullptr, 0); }
    // KP's table, dgrams() entries: out[i] = the source of the array's datagram i in 16-byte units into the frame area.  src0[s] =
    // bytes into the area at which stream s's delivered frames begin (read for the streams that delivered), one frame every
    // pitch_bytes, B_s datagrams valid in each.  false (nothing written): an offset or a pitch that is no multiple of 16, a pitch
    // shorter than a stream's frame, or a datagram at or past 2^32 units
    bool table(const uint64_t *src0, uint64_t pitch_bytes, uint32_t *out) { return fill(src0, pitch_bytes, nullptr, out); }
    // both in the one merge (either may be NULL)
    bool fill(const uint64_t *src0, uint64_t pitch_bytes, uint16_t *stream_of, uint32_t *out)
    {
        if (!ok_) return false;
        if (out) {
            if (pitch_bytes & 15u) return false;
            for (size_t s = 0; s < D_.size(); ++s) {
                if (!D_[s]) continue;
                const uint64_t F = D_[s] / B_[s];
                if ((src0[s] & 15u) || (uint64_t)B_[s] * RX_EGRESS_DGRAM_BYTES > pitch_bytes) return false;
                const uint64_t most = (uint64_t)0xffffffffu * 16; // (bytes: the sum below cannot wrap)
                if (src0[s] > most || (F - 1 && F - 1 > most / pitch_bytes)) return false;
                const uint64_t last = src0[s] + (F - 1) * pitch_bytes + (uint64_t)(B_[s] - 1) * RX_EGRESS_DGRAM_BYTES;
                if (last / 16 > 0xffffffffu) return false;
            }
        }
        merge_(stream_of, out, src0, pitch_bytes);
        return true;
    }

private:
    struct Group {
        uint64_t D, j;      // the datagrams of each of its streams, the next one
        size_t first, n;    // its streams: order_[first .. first + n), ascending
    };
    // the heap's "comes later": key (2 j_a + 1) / (2 D_a) above that of b, a tie by the first (smallest) stream
    struct Later {
        const std::vector<Group> *g;
        const std::vector<uint32_t> *order;
        bool operator()(uint32_t a, uint32_t b) const
        {
            const Group &x = (*g)[a], &y = (*g)[b];
            const uint64_t l = (2 * x.j + 1) * y.D, r = (2 * y.j + 1) * x.D;
            return l != r ? l > r : (*order)[x.first] > (*order)[y.first];
        }
    };

    bool plan_(const size_t *F, const size_t *B, size_t B_all, size_t nstreams)
    {
        ok_ = false;
        if (!nstreams || nstreams > RX_EGRESS_MAX_STREAMS) return false;
        const size_t S = nstreams;
        uint64_t total = 0;
        for (size_t s = 0; s < S; ++s) {
            const uint64_t b = B ? B[s] : B_all;
            if (!b || b > RX_PACED_MAX_STREAM_DGRAMS || (uint64_t)F[s] > RX_PACED_MAX_STREAM_DGRAMS / b) return false;
            total += (uint64_t)F[s] * b; // (S x 2^31 at most)
        }
        if (total > RX_PACED_MAX_DGRAMS) return false;
        D_.resize(S); B_.resize(S);
        for (size_t s = 0; s < S; ++s) {
            B_[s] = B ? B[s] : B_all;
            D_[s] = (uint64_t)F[s] * B_[s];
        }
        // the groups: streams of equal D_s, ascending inside (a stable sort of the streams that deliver by D_s)
        order_.clear();
        for (size_t s = 0; s < S; ++s)
            if (D_[s]) order_.push_back((uint32_t)s);
        const std::vector<uint64_t> &D = D_;
        std::stable_sort(order_.begin(), order_.end(), [&D](uint32_t a, uint32_t b) { return D[a] < D[b]; });
        groups_.clear();
        for (size_t i = 0; i < order_.size(); ++i) {
            if (groups_.empty() || groups_.back().D != D_[order_[i]]) {
                const Group g = {D_[order_[i]], 0, i, 0};
                groups_.push_back(g);
            }
            ++groups_.back().n;
        }
        total_ = total;
        ok_ = true;
        return true;
    }

    // the merge: stream_of and / or the table (src0, pitch as for table(); checked by the caller)
    void merge_(uint16_t *stream_of, uint32_t *out, const uint64_t *src0, uint64_t pitch_bytes)
    {
        if (!ok_) return;
        const size_t S = D_.size();
        cur_.assign(S, 0); blk_.assign(S, 0);
        if (out)
            for (size_t s = 0; s < S; ++s)
                if (D_[s]) cur_[s] = src0[s] / 16;
        const uint64_t step = RX_EGRESS_DGRAM_BYTES / 16;
        heap_.clear();
        for (size_t g = 0; g < groups_.size(); ++g) { groups_[g].j = 0; heap_.push_back((uint32_t)g); }
        const Later later = {&groups_, &order_};
        std::make_heap(heap_.begin(), heap_.end(), later);
        uint64_t i = 0;
        while (!heap_.empty()) {
            // the groups whose next key is the smallest: nearly always one; several (a tie between groups) give their streams merged
            std::pop_heap(heap_.begin(), heap_.end(), later);
            size_t tied = 1;
            const Group &g0 = groups_[heap_.back()];
            while (tied < heap_.size()) {
                const Group &g1 = groups_[heap_.front()];
                if ((2 * g1.j + 1) * g0.D != (2 * g0.j + 1) * g1.D) break;
                std::pop_heap(heap_.begin(), heap_.end() - tied, later);
                ++tied;
            }
            const uint32_t *ss = &order_[g0.first];
            size_t ns = g0.n;
            if (tied > 1) {
                tie_.clear();
                for (size_t k = 0; k < tied; ++k) {
                    const Group &g = groups_[heap_[heap_.size() - 1 - k]];
                    tie_.insert(tie_.end(), order_.begin() + (std::ptrdiff_t)g.first, order_.begin() + (std::ptrdiff_t)(g.first + g.n));
                }
                std::sort(tie_.begin(), tie_.end());
                ss = tie_.data(); ns = tie_.size();
            }
            for (size_t k = 0; k < ns; ++k, ++i) {
                const uint32_t s = ss[k];
                if (stream_of) stream_of[i] = (uint16_t)s;
                if (!out) continue;
                out[i] = (uint32_t)cur_[s];
                if (++blk_[s] == B_[s]) { // (the next frame: one every pitch)
                    blk_[s] = 0;
                    cur_[s] += pitch_bytes / 16 - (uint64_t)(B_[s] - 1) * step;
                } else {
                    cur_[s] += step;
                }
            }
            // the tied groups lie at the heap's end: each goes back with its next datagram, or leaves
            size_t live = heap_.size() - tied;
            for (size_t k = 0; k < tied; ++k) {
                const uint32_t g = heap_[heap_.size() - tied + k];
                if (++groups_[g].j < groups_[g].D) {
                    heap_[live++] = g;
                    std::push_heap(heap_.begin(), heap_.begin() + (std::ptrdiff_t)live, later);
                }
            }
            heap_.resize(live);
        }
    }

    bool ok_ = false;
    uint64_t total_ = 0;
    std::vector<uint64_t> D_;       // [S]
    std::vector<size_t> B_;         // [S]
    std::vector<uint32_t> order_;   // the streams that deliver, by D_s then stream
    std::vector<Group> groups_;     // runs of equal D_s in order_
    std::vector<uint32_t> heap_, tie_;
    std::vector<uint64_t> cur_;     // [S] the next datagram's source in 16-byte units
    std::vector<size_t> blk_;       // [S] ... and its block inside its frame
};
} // namespace sdrhip
