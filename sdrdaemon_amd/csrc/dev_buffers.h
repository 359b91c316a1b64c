// dev_buffers.h -- what owns device memory, pinned host memory, events and the context reference in libsdrhip.so's host layer.
// Every type here releases what it holds in its destructor and is move-only: a handle struct that holds them by value needs no
// release list, and handing a buffer over is a move (the target frees what it held, the source is left empty).
// Host-only C++11, header-only: standard headers, the HIP runtime API and the error codes, nothing of the library (a stand-alone
// program can build it: tests/cxx/dev_buffers_test.cpp).
#pragma once
#include "../../include/sdrhip.h"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace sdrhip {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void ctx_retain(sdrhip_ctx *c);
void ctx_release(sdrhip_ctx *c);

// a reference on the context: a handle holds one as its FIRST member, so that it goes last -- behind every buffer and event of the
// handle, whose destructors run while the context (its device, its streams) still exists
class CtxRef {
    sdrhip_ctx *c;

public:
    explicit CtxRef(sdrhip_ctx *ctx) : c(ctx) { if (c) ctx_retain(c); }
    CtxRef(const CtxRef &) = delete;
    CtxRef &operator=(const CtxRef &) = delete;
    CtxRef(CtxRef &&o) noexcept : c(o.c) { o.c = nullptr; }
    CtxRef &operator=(CtxRef &&o) noexcept
    {
        if (this != &o) { if (c) ctx_release(c); c = o.c; o.c = nullptr; }
        return *this;
    }
    ~CtxRef() { if (c) ctx_release(c); }
    operator sdrhip_ctx *() const { return c; }
    sdrhip_ctx *operator->() const { return c; }
};

// one event, created on first use (ensure)
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() {}
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept
    {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~DevEvent() { reset(); }
    int ensure(unsigned flags = hipEventDisableTiming)
    {
        if (!e && hipEventCreateWithFlags(&e, flags) != hipSuccess) { e = nullptr; return fail(SDRHIP_EDEVICE, "hipEventCreate"); }
        return SDRHIP_OK;
    }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// growable device scratch buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t n) { return n <= cap ? 0 : alloc_exact(n + n / 4 + 256); }
    // exactly n bytes, whatever it held (the handles' state arrays: allocated once, never over-allocated)
    int alloc_exact(size_t n)
    {
        release();
        if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; return fail(SDRHIP_ENOMEM, "hipMalloc(%zu) failed", n); }
        cap = n;
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// growable pinned host staging buffer; reuse waits for the previous upload that read from it
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevEvent ev;
    bool pending = false;
    PinnedBuf() {}
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap), ev(std::move(o.ev)), pending(o.pending) { o.p = nullptr; o.cap = 0; o.pending = false; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap; ev = std::move(o.ev); pending = o.pending;
            o.p = nullptr; o.cap = 0; o.pending = false;
        }
        return *this;
    }
    ~PinnedBuf() { release(); }
    int reserve(size_t n) // also waits for the pending upload
    {
        wait();
        if (n <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = n + n / 2 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return fail(SDRHIP_ENOMEM, "hipHostMalloc(%zu) failed", want); }
        cap = want;
        return ev.ensure();
    }
    void mark(hipStream_t s) // call after enqueueing the copies that read from p
    {
        if (ev && hipEventRecord(ev, s) == hipSuccess) pending = true;
    }
    void release()
    {
        wait();
        if (p) (void)hipHostFree(p);
        ev.reset();
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }

private:
    void wait()
    {
        if (pending) (void)hipEventSynchronize(ev);
        pending = false;
    }
};

// Four pinned versions of something that goes up once per call: the next of four, whose reuse waits for that version's own upload,
// four calls back -- a run of calls does not wait for the call before it
struct PinnedVersions {
    PinnedBuf v[4];
    int sel = 0;
    PinnedBuf &peek() { return v[(sel + 1) & 3]; } // the next version, not yet taken
    void advance() { sel = (sel + 1) & 3; }
    PinnedBuf &next() { advance(); return v[sel]; }
};

// A small table that launches in flight keep reading while later calls change it: a new version goes up from the next of four
// pinned versions into the device table the previous version does NOT occupy -- a launch that was enqueued with the previous
// table, a deferred one that kept its pointer, never sees a later version
struct TableVersions {
    PinnedVersions pin;
    DevBuf dev[2];
    int dev_sel = 0;
    const void *current() const { return dev[dev_sel].p; }
    // `bytes` of src become the current version, enqueued on `stream`; a failure leaves the current version as it was
    int upload(hipStream_t stream, const void *src, size_t bytes, const void **out)
    {
        PinnedBuf &from = pin.peek();
        DevBuf &tab = dev[dev_sel ^ 1];
        int rc;
        if ((rc = from.reserve(bytes))) return rc;
        if ((rc = tab.reserve(bytes))) return rc;
        memcpy(from.p, src, bytes);
        if (hipMemcpyAsync(tab.p, from.p, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) // (not counted: a table)
            return fail(SDRHIP_EDEVICE, "hipMemcpyAsync of a table version");
        from.mark(stream);
        pin.advance();
        dev_sel ^= 1;
        *out = tab.p;
        return SDRHIP_OK;
    }
};

// The ring of batches behind a pipe's submit / collect entries, created on first use with depth 4.  B has `state` (0 free, 1 being
// filled, 2 in flight, 3 collected and lent to the caller: sdrhip_rx_collect_egress) and the DevEvent `done`, and owns its buffers.
// tail = the batch being filled, head = the next one to collect.  A lent batch lies behind head and keeps its slot until it is released.
template <class B> struct BatchRing {
    std::vector<B> v;
    size_t head = 0, tail = 0;

    void wait_all() // for the events of batches that may still be in flight (destruction)
    {
        for (auto &b : v)
            if (b.done) (void)hipEventSynchronize(b.done);
    }
    void reset(size_t depth) { v.clear(); v.resize(depth); head = tail = 0; } // (the caller refuses while anything is in flight)
    B &tail_batch() { if (v.empty()) v.resize(4); return v[tail % v.size()]; }
    // a batch that is being filled, in flight or lent and satisfies pred
    template <class P> bool any(P pred) const
    {
        for (const auto &b : v)
            if (b.state != 0 && pred(b)) return true;
        return false;
    }
    bool busy() const { return any([](const B &) { return true; }); }
    // the oldest batch once it has finished.  wait = 1: a batch that is still being filled goes out as it is (launch_filling, the
    // end of a stream), then the wait happens OUTSIDE the context lock: the submitting thread -- the reference's source / reader
    // thread -- keeps feeding the ring while the collecting thread sleeps on the oldest batch's event
    template <class F> int wait_oldest(std::unique_lock<std::recursive_mutex> &lock_, int wait, const char *who, F launch_filling, B **bp)
    {
        if (v.empty()) return fail(SDRHIP_EBUSY, "%s: nothing was submitted", who);
        for (;;) {
            B &h = v[head % v.size()];
            // (SDRHIP_OK always means: one batch collected -- possibly empty; a lent batch at the head of a ring it fills was collected)
            if (h.state == 0 || h.state == 3) return fail(SDRHIP_EBUSY, "%s: nothing was submitted", who);
            if (h.state == 1) {
                if (!wait) return fail(SDRHIP_EBUSY, "%s: the oldest batch is still being filled (wait = 1 launches it as it is)", who);
                int rc = launch_filling(h);
                if (rc) return rc;
                ++tail;
            }
            const hipError_t q = hipEventQuery(h.done);
            if (q == hipSuccess) { *bp = &h; break; }
            if (q != hipErrorNotReady) return fail(SDRHIP_EDEVICE, "hipEventQuery: %s", hipGetErrorString(q));
            if (!wait) return fail(SDRHIP_EBUSY, "%s: the oldest batch is still in flight", who);
            const size_t at = head;
            hipEvent_t ev = h.done;
            lock_.unlock();
            const hipError_t w = hipEventSynchronize(ev);
            lock_.lock();
            if (w != hipSuccess) return fail(SDRHIP_EDEVICE, "hipEventSynchronize: %s", hipGetErrorString(w));
            if (head == at) { *bp = &v[at % v.size()]; break; }
            // (another thread collected that batch meanwhile: look at the new head)
        }
        return SDRHIP_OK;
    }
};

} // namespace sdrhip
