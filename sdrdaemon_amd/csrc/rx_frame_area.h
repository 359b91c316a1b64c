// rx_frame_area.h -- the bookkeeping of the Rx pipe's frame area [stream][slot][128 + nb_fec][512]: where every stream's window
// stands, what a call completes, where the windows go when one would pass the end, and what the last call delivered.  Pure host
// arithmetic (no HIP, no library header): sdrhip_rx.cpp carries a plan out, tests/cxx/rx_frame_area_test.cpp replays it on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sdrhip {
constexpr uint64_t RX_FRAME_SAMPLES = 127 * 127;    // samples of one frame (SDRHIP_SAMPLES_PER_FRAME)
constexpr size_t RX_NO_LATE = ~(size_t)0;           // plan(): no frames wait for delivery in this area

// what n_dec decimated samples do to one stream
struct RxAdvance {
    size_t done;           // frames completed
    uint64_t rest;         // samples left in the frame that stays open
    int first_new;         // 1: slot 0 of the window holds a frame that was opened earlier (it has its meta block)
    int started;           // frames whose first sample arrives now: slots first_new .. first_new + started - 1
    uint64_t idx0;         // sample index, counted from the call's first sample, at which frame first_new starts
    unsigned frame_count0; // m_frameCount of frame first_new
};

// where the windows go before a call writes
struct RxAreaPlan {
    size_t new_cap = 0;            // slots per stream of a new area (0: the area stays)
    bool keep_old = false;         // frames wait for delivery in the old area: it is kept beside the new one
    std::vector<uint8_t> to_slot0; // per stream: its window goes to slot 0 (of the new area, or in place), its open frame with it
    bool moves() const
    {
        for (size_t s = 0; s < to_slot0.size(); ++s)
            if (to_slot0[s]) return true;
        return false;
    }
};

class RxFrameArea {
public:
    void init(size_t nstreams)
    {
        cap_ = 0;
        base_.assign(nstreams, 0); pending_.assign(nstreams, 0); open_.assign(nstreams, 0); count_.assign(nstreams, 0);
    }
    size_t streams() const { return base_.size(); }
    size_t cap() const { return cap_; }                    // slots per stream
    size_t slot(size_t s) const { return base_[s]; }       // slot of the frame being filled: the first of the next window
    const size_t *slots() const { return base_.data(); }
    uint64_t pending(size_t s) const { return pending_[s]; } // samples in that frame
    bool open(size_t s) const { return open_[s] != 0; }    // it has its meta block (a frame was started)
    uint16_t count(size_t s) const { return count_[s]; }   // its m_frameCount
    size_t index(size_t s, size_t f = 0) const { return s * cap_ + base_[s] + f; } // frame f of stream s's window, counted over the area

    // every stream stands at the same position (the uniform step, pipelined mode and uniform batches need it)
    bool aligned() const
    {
        for (size_t s = 1; s < base_.size(); ++s)
            if (base_[s] != base_[0] || pending_[s] != pending_[0] || open_[s] != open_[0] || count_[s] != count_[0]) return false;
        return true;
    }

    RxAdvance advance(size_t s, size_t n_dec) const
    {
        RxAdvance a;
        const uint64_t total = pending_[s] + n_dec;
        a.done = (size_t)(total / RX_FRAME_SAMPLES);
        a.rest = total - (uint64_t)a.done * RX_FRAME_SAMPLES;
        a.first_new = open_[s] ? 1 : 0;
        a.started = (int)(a.done + (a.rest > 0 ? 1 : 0)) - a.first_new;
        a.idx0 = a.first_new ? RX_FRAME_SAMPLES - pending_[s] : 0;
        a.frame_count0 = (unsigned)count_[s] + (unsigned)a.first_new;
        return a;
    }

    // Stream s is about to fill slots slot(s) .. slot(s) + done[s].  A call that needs more slots than the area has gets a new area
    // of window_multiple times the largest need, every window at slot 0.  Otherwise a window that would pass the end goes to slot 0
    // in place, the others stay.  late_slot0 (pipelined mode): frames wait for delivery from that slot on; a wrapped window that
    // would reach them gets a new area of the same capacity instead, and the old one is kept.
    RxAreaPlan plan(const size_t *done, size_t late_slot0, size_t window_multiple) const
    {
        RxAreaPlan p;
        const size_t S = base_.size();
        size_t need_max = 0;
        for (size_t s = 0; s < S; ++s) need_max = done[s] + 1 > need_max ? done[s] + 1 : need_max;
        bool hits_late = false;
        p.to_slot0.assign(S, 0);
        if (need_max > cap_) p.new_cap = window_multiple * need_max;
        else
            for (size_t s = 0; s < S; ++s) {
                if (base_[s] + done[s] + 1 <= cap_) continue;
                p.to_slot0[s] = 1;
                hits_late = hits_late || (late_slot0 != RX_NO_LATE && done[s] + 1 > late_slot0); // [0, need) against [slot0, ...)
            }
        if (hits_late) p.new_cap = cap_;
        if (p.new_cap) {
            p.to_slot0.assign(S, 1);
            p.keep_old = late_slot0 != RX_NO_LATE;
        }
        return p;
    }
    // a new area of the same capacity with other slots (a fecblk change): every window to slot 0; nothing if there is no area yet
    RxAreaPlan replan() const
    {
        RxAreaPlan p;
        p.new_cap = cap_;
        p.to_slot0.assign(base_.size(), cap_ ? 1 : 0);
        return p;
    }
    // the plan has been carried out
    void moved(const RxAreaPlan &p)
    {
        if (p.new_cap) cap_ = p.new_cap;
        for (size_t s = 0; s < base_.size(); ++s)
            if (p.to_slot0[s]) base_[s] = 0;
    }
    // the call has written: the frame still being filled opens the next call's window
    void commit(const size_t *done, const uint64_t *rest)
    {
        for (size_t s = 0; s < base_.size(); ++s) {
            base_[s] += done[s];
            pending_[s] = rest[s];
            open_[s] = rest[s] > 0 ? 1 : 0;
            count_[s] = (uint16_t)(count_[s] + done[s]);
        }
    }

    // UDPSinkFEC's constructor for the streams named (mask NULL: every stream): the open frame is dropped where it lies.  When every
    // stream was reset no frame is open anywhere, so every window goes back to slot 0 as well: the streams are aligned() again
    void reset(const uint8_t *mask)
    {
        for (size_t s = 0; s < base_.size(); ++s) {
            if (mask && !mask[s]) continue;
            pending_[s] = 0; open_[s] = 0; count_[s] = 0;
            if (!mask) base_[s] = 0;
        }
    }
    // a framing state a stream can be in (sdrhip_rx_import_stream checks a blob's before anything moves) ...
    static bool importable(uint64_t pending, uint32_t open, uint32_t count)
    {
        return open <= 1 && pending < RX_FRAME_SAMPLES && (open || !pending) && count <= 0xffffu;
    }
    // ... and stream s takes it over; its window stays where it is
    void import_stream(size_t s, uint64_t pending, uint32_t open, uint32_t count)
    {
        pending_[s] = pending; open_[s] = (uint8_t)open; count_[s] = (uint16_t)count;
    }

private:
    size_t cap_ = 0;
    std::vector<size_t> base_;
    std::vector<uint64_t> pending_;
    std::vector<uint8_t> open_;
    std::vector<uint16_t> count_;
};

// The frames the last call DELIVERED: frame f of stream s lies at base() + s * stride() + (first(s) + f) * frame bytes, f < frames(s).
// base() is the area they lie in -- the current one, or the kept old one behind a pipelined call that got a new area
class RxView {
public:
    const uint8_t *base() const { return base_; }
    size_t stride() const { return stride_; } // bytes between streams
    size_t first(size_t s) const { return first_[s]; }
    size_t frames(size_t s) const { return frames_[s]; }
    void init(size_t nstreams) { set(nullptr, 0, nstreams, 0, 0); }
    void clear() { base_ = nullptr; stride_ = 0; first_.assign(first_.size(), 0); frames_.assign(frames_.size(), 0); }
    // every stream shows the same window (sdrhip_rx_frames_view can describe it)
    bool uniform() const
    {
        for (size_t s = 1; s < first_.size(); ++s)
            if (first_[s] != first_[0] || frames_[s] != frames_[0]) return false;
        return true;
    }
    // the same window of every stream / each stream's own
    void set(const uint8_t *area, size_t stream_stride, size_t nstreams, size_t first_slot, size_t n)
    {
        base_ = area; stride_ = stream_stride; first_.assign(nstreams, first_slot); frames_.assign(nstreams, n);
    }
    void set_each(const uint8_t *area, size_t stream_stride, size_t nstreams, const size_t *first_slot, const size_t *n)
    {
        base_ = area; stride_ = stream_stride; first_.assign(first_slot, first_slot + nstreams); frames_.assign(n, n + nstreams);
    }
    size_t offset(size_t s, size_t frame_bytes) const { return s * stride_ + first_[s] * frame_bytes; } // of stream s's window, from base()
    const uint8_t *window(size_t s, size_t frame_bytes) const { return base_ ? base_ + offset(s, frame_bytes) : nullptr; }

private:
    const uint8_t *base_ = nullptr;
    size_t stride_ = 0;
    std::vector<size_t> first_, frames_;
};
} // namespace sdrhip
