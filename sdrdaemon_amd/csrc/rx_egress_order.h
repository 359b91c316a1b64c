// rx_egress_order.h -- the departure order of a batch the Rx pipe delivers as ONE datagram array (sdrhip_rx_set_egress,
// SDRHIP_EGRESS_ROUND_ROBIN).  Stream s delivered F_s frames of B datagrams: D_s = F_s B datagrams in the reference's wire order
// (frame after frame, blocks 0 .. B - 1 inside a frame, UDPSinkFEC.cpp:259).  The array is rounds j = 0, 1, 2, ... concatenated;
// round j holds datagram j of every stream with D_s > j, streams in ascending order.  Every round of frame number f (j = f B + b)
// holds the same streams -- those with F_t > f -- so with A_f = #{t : F_t > f}, r_f(s) = #{t < s : F_t > f} and
// base_f = B sum_{g<f} A_g the position of block b of frame f of stream s is
//     pos(s, f, b) = base_f + b A_f + r_f(s):
// a frame's B datagrams go out at a constant stride, which is all KE (rx_egress_kernels.hip) needs: one run per delivered frame.
// Pure host arithmetic (no HIP, no library header): sdrhip_rx_egress.cpp builds KE's table and the tags from it,
// tests/cxx/rx_egress_order_test.cpp replays it on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sdrhip {
constexpr uint64_t RX_EGRESS_DGRAM_BYTES = 512;
constexpr uint32_t RX_EGRESS_WG_DGRAMS = 32;  // datagrams a KE workgroup moves (256 lanes x 4 chunks of 16 bytes)
constexpr size_t RX_EGRESS_MAX_STREAMS = 65535; // (a tag is a uint16_t)

// one delivered frame for KE: its B datagrams lie back to back at `src` (bytes into the frame area) and go to dst + b * stride
// (bytes into the departure-order array); all three are multiples of 16
struct RxEgressRun {
    uint64_t src, dst, stride;
};

class RxEgressOrder {
public:
    // F[s] = frames stream s delivered, B = datagrams per frame.  false (nothing usable afterwards): no stream or more than 65535,
    // B = 0, or a batch whose frames x workgroups per frame pass KE's 32-bit grid -- checked on the sums before anything is sized
    bool plan(const size_t *F, size_t nstreams, size_t blocks_per_frame)
    {
        ok_ = false;
        if (!nstreams || nstreams > RX_EGRESS_MAX_STREAMS || !blocks_per_frame || blocks_per_frame > 0xffffu) return false;
        B_ = blocks_per_frame;
        wgpf_ = (uint32_t)((B_ + RX_EGRESS_WG_DGRAMS - 1) / RX_EGRESS_WG_DGRAMS);
        const uint64_t max_frames = 0x7fffffffu / wgpf_;
        uint64_t total = 0;
        size_t fmax = 0;
        for (size_t s = 0; s < nstreams; ++s) {
            if (F[s] > max_frames || total + F[s] > max_frames) return false;
            total += F[s];
            fmax = F[s] > fmax ? F[s] : fmax;
        }
        first_.resize(nstreams + 1);
        rank_.resize((size_t)total);
        alive_.assign(fmax, 0);
        size_t k = 0;
        for (size_t s = 0; s < nstreams; ++s) { // (ascending s: the streams counted so far are the t < s)
            first_[s] = k;
            for (size_t f = 0; f < F[s]; ++f) rank_[k++] = alive_[f]++;
        }
        first_[nstreams] = k;
        base_.resize(fmax);
        uint64_t acc = 0;
        for (size_t f = 0; f < fmax; ++f) { base_[f] = acc; acc += (uint64_t)B_ * alive_[f]; }
        ok_ = true;
        return true;
    }
    size_t streams() const { return ok_ ? first_.size() - 1 : 0; }
    size_t blocks_per_frame() const { return B_; }
    size_t frames() const { return ok_ ? rank_.size() : 0; }                  // delivered frames = runs
    size_t frames(size_t s) const { return first_[s + 1] - first_[s]; }
    uint64_t dgrams() const { return (uint64_t)frames() * B_; }
    uint32_t wg_per_frame() const { return wgpf_; }
    uint64_t grid() const { return (uint64_t)frames() * wgpf_; }             // KE's workgroups for the frames (at most 2^31 - 1)
    size_t run(size_t s, size_t f) const { return first_[s] + f; }           // frame f of stream s in the table: stream-major
    uint32_t alive(size_t f) const { return alive_[f]; }                     // A_f
    uint32_t rank(size_t s, size_t f) const { return rank_[first_[s] + f]; } // r_f(s)
    uint64_t base(size_t f) const { return base_[f]; }                       // base_f
    uint64_t pos(size_t s, size_t f, size_t b) const { return base_[f] + (uint64_t)b * alive_[f] + rank(s, f); }

    // stream_of[i] for the dgrams() entries of the array
    void tags(uint16_t *stream_of) const
    {
        const size_t S = streams();
        std::vector<uint16_t> live;
        uint16_t *o = stream_of;
        for (size_t f = 0; f < alive_.size(); ++f) {
            live.clear();
            for (size_t s = 0; s < S; ++s)
                if (frames(s) > f) live.push_back((uint16_t)s);
            for (size_t b = 0; b < B_; ++b)
                for (size_t i = 0; i < live.size(); ++i) *o++ = live[i];
        }
    }
    // KE's table, frames() entries: src0[s] = bytes into the frame area at which stream s's delivered frames begin (read for the
    // streams that delivered).  false: an offset that is no multiple of 16
    bool runs(const uint64_t *src0, RxEgressRun *out) const
    {
        const size_t S = streams();
        const uint64_t fb = (uint64_t)B_ * RX_EGRESS_DGRAM_BYTES;
        for (size_t s = 0; s < S; ++s)
            for (size_t f = 0; f < frames(s); ++f) {
                if (src0[s] & 15u) return false;
                RxEgressRun &r = out[first_[s] + f];
                r.src = src0[s] + f * fb;
                r.dst = pos(s, f, 0) * RX_EGRESS_DGRAM_BYTES;
                r.stride = (uint64_t)alive_[f] * RX_EGRESS_DGRAM_BYTES;
            }
        return true;
    }

private:
    bool ok_ = false;
    size_t B_ = 0;
    uint32_t wgpf_ = 0;
    std::vector<size_t> first_;   // [S + 1] first run of stream s
    std::vector<uint32_t> rank_;  // [frames] r_f(s), stream-major
    std::vector<uint32_t> alive_; // [max F] A_f
    std::vector<uint64_t> base_;  // [max F] base_f
};
} // namespace sdrhip
