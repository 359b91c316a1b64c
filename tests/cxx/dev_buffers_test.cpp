// dev_buffers_test.cpp -- sdrdaemon_amd/csrc/dev_buffers.h on a CPU, under the address and undefined-behaviour sanitizers.
// No HIP library is linked: the HIP functions the header calls are defined HERE, over malloc, with a ledger of what is live
// (device blocks, pinned blocks, events; per event "recorded and not yet waited for") and a log of the calls.  A free or a destroy
// of something that is not live, and a free of a pinned block whose upload nobody waited for, end the program at once.
// Driven by tests/test_dev_buffers.py.
#include "dev_buffers.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>

struct sdrhip_ctx { int refs; };

// ------------------------------------------------------------------------------------------------ the ledger and the fakes
namespace {
struct Block { size_t bytes; int serial; };
struct Event { bool pending; int serial; };
std::map<void *, Block> g_dev, g_pin;
std::map<hipEvent_t, Event> g_ev;
std::map<void *, hipEvent_t> g_guard; // pinned block -> the event recorded behind the upload that reads it (PinnedBuf::mark)
std::vector<std::string> g_log;
int g_serial = 0;
long g_allocs = 0, g_fail_at = 0; // allocation calls so far (hipMalloc, hipHostMalloc, hipEventCreateWithFlags); the one that fails (0: none)
int g_failed = 0;                 // what failed since the test last cleared it: 1 memory, 2 event

[[noreturn]] void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stdout, fmt, ap);
    va_end(ap);
    fputs("\nFAILED\n", stdout);
    exit(1);
}
#define CHECK(cond) do { if (!(cond)) die("%s:%d: %s", __FILE__, __LINE__, #cond); } while (0)

void note(const char *op, long a, long b = -1)
{
    char buf[96];
    snprintf(buf, sizeof(buf), "%s %ld %ld", op, a, b);
    g_log.push_back(buf);
}
bool refuse()
{
    ++g_allocs;
    return g_fail_at && g_allocs == g_fail_at;
}
void ledger_reset()
{
    CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
    g_guard.clear(); g_log.clear();
    g_serial = 0; g_allocs = 0; g_fail_at = 0; g_failed = 0;
}
bool is_pending(hipEvent_t e) { return e && g_ev.count(e) && g_ev[e].pending; }
} // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n)
{
    if (refuse()) { g_failed = 1; note("hipMalloc-fails", (long)n); return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    g_dev[*p] = Block{n, ++g_serial};
    note("hipMalloc", (long)n, g_serial);
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    if (!g_dev.count(p)) die("hipFree of a block that is not live");
    note("hipFree", g_dev[p].serial);
    g_dev.erase(p);
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    if (refuse()) { g_failed = 1; note("hipHostMalloc-fails", (long)n); return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    g_pin[*p] = Block{n, ++g_serial};
    note("hipHostMalloc", (long)n, g_serial);
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    if (!g_pin.count(p)) die("hipHostFree of a block that is not live");
    if (g_guard.count(p) && is_pending(g_guard[p])) die("hipHostFree of a block whose upload nobody waited for");
    note("hipHostFree", g_pin[p].serial);
    g_guard.erase(p);
    g_pin.erase(p);
    free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    if (flags != hipEventDisableTiming) die("an event with other flags than hipEventDisableTiming");
    if (refuse()) { g_failed = 2; note("hipEventCreate-fails", 0); return hipErrorOutOfMemory; }
    *e = static_cast<hipEvent_t>(malloc(1));
    g_ev[*e] = Event{false, ++g_serial};
    note("hipEventCreate", g_serial);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (!g_ev.count(e)) die("hipEventRecord of an event that is not live");
    g_ev[e].pending = true;
    note("hipEventRecord", g_ev[e].serial);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    if (!g_ev.count(e)) die("hipEventSynchronize of an event that is not live");
    g_ev[e].pending = false;
    note("hipEventSynchronize", g_ev[e].serial);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!g_ev.count(e)) die("hipEventDestroy of an event that is not live (destroyed twice?)");
    for (const auto &g : g_guard)
        if (g.second == e && g_ev[e].pending) die("hipEventDestroy of the event a live pinned block still waits for");
    note("hipEventDestroy", g_ev[e].serial);
    g_ev.erase(e);
    free(e);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t)
{
    if (kind != hipMemcpyHostToDevice || !g_dev.count(dst) || g_dev[dst].bytes < n) die("hipMemcpyAsync: not an upload into a live device block of that size");
    if (!g_pin.count(const_cast<void *>(src)) || g_pin[const_cast<void *>(src)].bytes < n) die("hipMemcpyAsync: not from a live pinned block of that size");
    memcpy(dst, src, n);
    note("hipMemcpyAsync", (long)n, g_dev[dst].serial);
    return hipSuccess;
}
}

namespace sdrhip {
int fail(int code, const char *, ...) { return code; }
void ctx_retain(sdrhip_ctx *c) { ++c->refs; }
void ctx_release(sdrhip_ctx *c) { if (--c->refs < 0) die("ctx_release without a reference"); }
} // namespace sdrhip

using namespace sdrhip;

// ------------------------------------------------------------------------------------------------ 2. compile-time properties
namespace {
struct TestBatch { // what the pipes' batches are made of
    DevBuf din;
    PinnedBuf in;
    DevEvent done;
    int state = 0;
};
template <class T> constexpr bool move_only()
{
    return !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value && std::is_nothrow_move_constructible<T>::value &&
           std::is_nothrow_move_assignable<T>::value;
}
static_assert(move_only<DevBuf>(), "DevBuf");
static_assert(move_only<PinnedBuf>(), "PinnedBuf");
static_assert(move_only<DevEvent>(), "DevEvent");
static_assert(move_only<CtxRef>(), "CtxRef");
static_assert(move_only<PinnedVersions>(), "PinnedVersions");
static_assert(move_only<TableVersions>(), "TableVersions");
static_assert(move_only<TestBatch>(), "a batch of them (std::vector<Batch>::resize moves)");

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};
hipStream_t const STREAM = nullptr;

// ------------------------------------------------------------------------------------------------ invariants of one object
void check(const DevBuf &b)
{
    if (!b.p) { CHECK(b.cap == 0); return; }
    CHECK(g_dev.count(b.p) && g_dev[b.p].bytes == b.cap);
}
void check(const PinnedBuf &b)
{
    CHECK(!b.pending || b.ev.e);
    CHECK(!b.ev.e || g_ev.count(b.ev.e));
    if (!b.p) { CHECK(b.cap == 0); return; }
    CHECK(g_pin.count(b.p) && g_pin[b.p].bytes == b.cap);
}
void check_empty(const DevBuf &b) { CHECK(b.p == nullptr && b.cap == 0); }
void check_empty(const PinnedBuf &b) { CHECK(b.p == nullptr && b.cap == 0 && !b.pending && b.ev.e == nullptr); }
// what a reserve must have answered, given what the fakes refused meanwhile
void check_reserve(int rc, const DevBuf &b, size_t n)
{
    if (g_failed == 1) { CHECK(rc == SDRHIP_ENOMEM); check_empty(b); }
    else { CHECK(rc == SDRHIP_OK && b.cap >= n); }
    g_failed = 0;
}
void check_reserve(int rc, const PinnedBuf &b, size_t n)
{
    CHECK(!b.pending && !is_pending(b.ev.e)); // (handed out again: the upload that read it was waited for)
    if (g_failed == 1) { CHECK(rc == SDRHIP_ENOMEM && b.p == nullptr && b.cap == 0); }
    else if (g_failed == 2) { CHECK(rc == SDRHIP_EDEVICE && b.cap >= n && b.ev.e == nullptr); }
    else { CHECK(rc == SDRHIP_OK && b.cap >= n); } // (the event comes with the first block)
    g_failed = 0;
}
void mark(PinnedBuf &b)
{
    if (!b.p) return; // (a reserve that failed: its caller returns, nothing is uploaded)
    b.mark(STREAM);
    if (b.p && b.ev.e) { CHECK(b.pending && is_pending(b.ev.e)); g_guard[b.p] = b.ev.e; }
    else CHECK(!b.pending);
}
void do_reserve(DevBuf &b, size_t n) { check_reserve(b.reserve(n), b, n); }
void do_reserve(PinnedBuf &b, size_t n) { check_reserve(b.reserve(n), b, n); }
void after_use(DevBuf &) {}
void after_use(PinnedBuf &b) { mark(b); }

// ------------------------------------------------------------------------------------------------ 1. / 4. seeded scripts
// One step on objects a, b of a kind: reserve, grow, move-construct, move-assign (onto empty or not), swap, self-move, release,
// scope exit
template <class T> void step(Rng &r, T &a, T &b)
{
    switch (r.below(9)) {
    case 0: do_reserve(a, r.below(5000)); after_use(a); break;
    case 1: do_reserve(a, a.cap + 1 + r.below(300)); if (r.below(2)) after_use(a); break; // grows
    case 2: { // move-construct; the new object goes at the end of its scope, or comes back
        void *p = a.p;
        const size_t cap = a.cap;
        T t(std::move(a));
        check_empty(a);
        CHECK(t.p == p && t.cap == cap);
        check(t);
        if (r.below(2)) { a = std::move(t); check_empty(t); CHECK(a.p == p); }
        break;
    }
    case 3: { // move-assign, onto whatever a holds
        void *p = b.p;
        const size_t cap = b.cap;
        a = std::move(b);
        check_empty(b);
        CHECK(a.p == p && a.cap == cap);
        break;
    }
    case 4: { // ... onto an empty one
        a.release();
        check_empty(a);
        a = std::move(b);
        check_empty(b);
        break;
    }
    case 5: { void *pa = a.p, *pb = b.p; std::swap(a, b); CHECK(a.p == pb && b.p == pa); break; }
    case 6: { // self-move
        void *p = a.p;
        const size_t cap = a.cap;
        T &same = a;
        a = std::move(same);
        CHECK(a.p == p && a.cap == cap);
        break;
    }
    case 7: a.release(); check_empty(a); break;
    default: { T t; do_reserve(t, 1 + r.below(2000)); after_use(t); if (r.below(2)) std::swap(t, b); break; } // scope exit
    }
    check(a);
    check(b);
}

const void *g_src; // 8192 bytes to upload from
long script(uint64_t seed, int steps, long fail_at)
{
    ledger_reset();
    g_fail_at = fail_at;
    Rng r(seed);
    {
        DevBuf d[5];
        PinnedBuf p[5];
        DevEvent e[3];
        TableVersions tv;
        for (int i = 0; i < steps; ++i) {
            const uint32_t kind = r.below(10), x = r.below(5), y = (x + 1 + r.below(4)) % 5;
            if (kind < 4) step(r, d[x], d[y]);
            else if (kind < 8) step(r, p[x], p[y]);
            else if (kind == 8) {
                DevEvent &ev = e[x % 3];
                const int rc = ev.ensure();
                CHECK(g_failed == 2 ? (rc == SDRHIP_EDEVICE && !ev.e) : (rc == SDRHIP_OK && ev.e));
                g_failed = 0;
                if (r.below(3) == 0) { DevEvent t(std::move(ev)); CHECK(!ev.e); if (r.below(2)) e[(x + 1) % 3] = std::move(t); }
            } else {
                const void *was = tv.current(), *out = nullptr;
                const size_t n = 1 + r.below(8192);
                const int rc = tv.upload(STREAM, g_src, n, &out);
                if (g_failed) { CHECK(rc == (g_failed == 1 ? SDRHIP_ENOMEM : SDRHIP_EDEVICE) && tv.current() == was); }
                else {
                    CHECK(rc == SDRHIP_OK && out == tv.current() && out != was && memcmp(out, g_src, n) == 0);
                    g_guard[tv.pin.v[tv.pin.sel].p] = tv.pin.v[tv.pin.sel].ev.e;
                }
                g_failed = 0;
                CHECK(!was || g_dev.count(const_cast<void *>(was))); // (a launch in flight may still read the previous version)
            }
        }
    }
    CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
    return g_allocs;
}

// ------------------------------------------------------------------------------------------------ 3. PinnedBuf waits
void pinned_waits()
{
    ledger_reset();
    for (int how = 0; how < 5; ++how) {
        PinnedBuf a;
        do_reserve(a, 100);
        mark(a);
        hipEvent_t ev = a.ev.e;
        CHECK(is_pending(ev));
        PinnedBuf other;
        do_reserve(other, 10);
        const size_t logged = g_log.size();
        switch (how) {
        case 0: do_reserve(a, 50); CHECK(a.p); break;         // handed out again as it is: behind the wait
        case 1: do_reserve(a, 100000); break;                 // grows: the old block is freed behind the wait
        case 2: a.release(); check_empty(a); break;
        case 3: a = std::move(other); break;                  // a move-assignment onto it
        default: break;                                       // the destructor, at the end of this scope
        }
        if (how < 4) {
            CHECK(g_log.size() > logged && g_log[logged].compare(0, 19, "hipEventSynchronize") == 0);
            CHECK(!is_pending(ev));
        }
        // (the fakes end the program if the block goes before the wait: how = 4 is checked by them alone)
    }
    // a pending buffer that moves on takes its event and its wait with it
    {
        PinnedBuf a, b;
        do_reserve(a, 100);
        mark(a);
        b = std::move(a);
        check_empty(a);
        CHECK(b.pending && is_pending(b.ev.e));
        do_reserve(a, 10); // (the moved-from one is usable, with an event of its own)
        CHECK(a.ev.e && a.ev.e != b.ev.e);
    }
    CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
}

// ------------------------------------------------------------------------------------------------ 5. TableVersions against the rotation it replaces
// the rotation as rx_stream_table, stream_mask_upload and the x_pin selection spelt it out before
struct OldRotation {
    PinnedBuf pin[4];
    DevBuf dev[2];
    int pin_sel = 0, dev_sel = 0;
    int upload(hipStream_t stream, const void *src, size_t bytes, const void **out)
    {
        PinnedBuf &from = pin[(pin_sel + 1) & 3];
        DevBuf &tab = dev[dev_sel ^ 1];
        int rc;
        if ((rc = from.reserve(bytes))) return rc;
        if ((rc = tab.reserve(bytes))) return rc;
        memcpy(from.p, src, bytes);
        if (hipMemcpyAsync(tab.p, from.p, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return SDRHIP_EDEVICE;
        from.mark(stream);
        pin_sel = (pin_sel + 1) & 3;
        dev_sel ^= 1;
        *out = tab.p;
        return SDRHIP_OK;
    }
};
struct OldPinned {
    PinnedBuf x_pin[4];
    int x_pin_sel = 0;
    PinnedBuf &next() { x_pin_sel = (x_pin_sel + 1) & 3; return x_pin[x_pin_sel]; }
};

std::vector<size_t> upload_sizes(uint64_t seed)
{
    Rng r(seed);
    std::vector<size_t> n;
    // (small tables that fit, then growth of one device table while the other is current, then a mix)
    for (int i = 0; i < 6; ++i) n.push_back(64);
    n.push_back(3000); n.push_back(64); n.push_back(64); n.push_back(8000); n.push_back(8100);
    for (int i = 0; i < 200; ++i) n.push_back(1 + (r.below(4) ? r.below(600) : r.below(8192)));
    return n;
}

void table_versions(uint64_t seed)
{
    const std::vector<size_t> sizes = upload_sizes(seed);
    std::vector<std::pair<int, int> > idx_old, idx_new;
    std::vector<std::string> log_old;
    ledger_reset();
    {
        OldRotation o;
        for (size_t n : sizes) {
            const void *out = nullptr;
            CHECK(o.upload(STREAM, g_src, n, &out) == SDRHIP_OK);
            idx_old.push_back(std::make_pair(o.pin_sel, o.dev_sel));
        }
    }
    log_old = g_log;
    ledger_reset();
    {
        TableVersions t;
        CHECK(t.current() == nullptr);
        for (size_t n : sizes) {
            const void *was = t.current(), *out = nullptr;
            const int was_sel = t.dev_sel;
            const size_t logged = g_log.size();
            CHECK(t.upload(STREAM, g_src, n, &out) == SDRHIP_OK);
            idx_new.push_back(std::make_pair(t.pin.sel, t.dev_sel));
            CHECK(out == t.current() && out == t.dev[t.dev_sel].p && memcmp(out, g_src, n) == 0);
            // never the table the previous version occupies, which stays where and what it was: growing one frees only that one
            CHECK(t.dev_sel == (was_sel ^ 1) && out != was);
            if (was) {
                CHECK(t.dev[was_sel].p == was && g_dev.count(const_cast<void *>(was)));
                const std::string freed = "hipFree " + std::to_string(g_dev[const_cast<void *>(was)].serial) + " ";
                for (size_t i = logged; i < g_log.size(); ++i) CHECK(g_log[i].compare(0, freed.size(), freed) != 0);
            }
        }
    }
    CHECK(idx_new == idx_old);
    CHECK(g_log == log_old);
    for (size_t i = 0; i < idx_old.size(); ++i) CHECK(idx_old[i].first == (int)((i + 1) & 3) && idx_old[i].second == (int)((i + 1) & 1));

    // the pinned half alone
    std::vector<int> sel_old, sel_new;
    ledger_reset();
    {
        OldPinned o;
        for (size_t n : sizes) { PinnedBuf &b = o.next(); CHECK(b.reserve(n) == SDRHIP_OK); b.mark(STREAM); sel_old.push_back(o.x_pin_sel); }
    }
    log_old = g_log;
    ledger_reset();
    {
        PinnedVersions v;
        for (size_t n : sizes) {
            PinnedBuf &peeked = v.peek();
            PinnedBuf &b = v.next();
            CHECK(&b == &peeked && &b == &v.v[v.sel]);
            CHECK(b.reserve(n) == SDRHIP_OK);
            b.mark(STREAM);
            sel_new.push_back(v.sel);
        }
    }
    CHECK(sel_new == sel_old && g_log == log_old);
    CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
}

// ------------------------------------------------------------------------------------------------ 6. a ring of batches
void fill(BatchRing<TestBatch> &ring)
{
    ring.tail_batch(); // (created on first use)
    for (size_t i = 0, n = ring.v.size(); i < n; ++i) {
        TestBatch &b = ring.tail_batch();
        CHECK(b.state == 0);
        do_reserve(b.din, 1000 + 100 * i);
        do_reserve(b.in, 500 + 10 * i);
        CHECK(b.done.ensure() == SDRHIP_OK);
        mark(b.in);
        CHECK(hipEventRecord(b.done, STREAM) == hipSuccess);
        b.state = 2;
        ++ring.tail;
    }
}
void ring_of_batches()
{
    ledger_reset();
    {
        BatchRing<TestBatch> ring;
        CHECK(!ring.busy());
        fill(ring);
        CHECK(ring.v.size() == 4 && ring.busy() && g_ev.size() == 8 && g_dev.size() == 4 && g_pin.size() == 4);
        ring.wait_all();
        for (auto &b : ring.v) { CHECK(!is_pending(b.done)); b.state = 0; }
        ring.reset(7); // (the fakes end the program if an event is destroyed twice)
        CHECK(ring.v.size() == 7 && ring.head == 0 && ring.tail == 0 && !ring.busy());
        CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
        fill(ring);
        CHECK(g_ev.size() == 14 && g_dev.size() == 7 && g_pin.size() == 7);
        ring.reset(2); // ... to a smaller depth as well
        CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
        fill(ring);
        ring.wait_all();
    } // destroyed with its batches
    CHECK(g_dev.empty() && g_pin.empty() && g_ev.empty());
}

void ctx_refs()
{
    sdrhip_ctx c = {0};
    {
        CtxRef a(&c);
        CHECK(c.refs == 1 && a == &c && a->refs == 1);
        CtxRef b(std::move(a));
        CHECK(c.refs == 1 && a == nullptr && b == &c);
        CtxRef d(&c);
        CHECK(c.refs == 2);
        d = std::move(b);
        CHECK(c.refs == 1 && b == nullptr);
        CtxRef &same = d;
        d = std::move(same);
        CHECK(c.refs == 1 && d == &c);
    }
    CHECK(c.refs == 0);
}
} // namespace

int main()
{
    std::vector<unsigned char> src(8192);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char)(i * 131 + 7);
    g_src = src.data();

    long steps = 0;
    for (uint64_t seed = 1; seed <= 8; ++seed) { script(seed, 2500, 0); steps += 2500; }
    // every allocation of a script refused in turn: the failing call says so, everything else survives, nothing is left
    long refused = 0;
    for (uint64_t seed = 11; seed <= 12; ++seed) {
        const long allocs = script(seed, 400, 0);
        CHECK(allocs > 100);
        for (long k = 1; k <= allocs; ++k) script(seed, 400, k);
        refused += allocs;
    }
    pinned_waits();
    for (uint64_t seed = 21; seed <= 24; ++seed) table_versions(seed);
    ring_of_batches();
    ctx_refs();
    ledger_reset();
    printf("%ld script steps, %ld refused allocations\nOK\n", steps, refused);
    return 0;
}
