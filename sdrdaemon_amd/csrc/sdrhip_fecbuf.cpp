// sdrhip_fecbuf.cpp -- host side of the FEC buffer bank (include/sdrhip.h, sdrhip_fecbuf_*): nstreams SDRdaemonFECBuffer
// collectors fed raw datagrams.  A call: upload of the per-stream datagram counts, the classify pass (fecbuf_kernels.hip), ONE
// read-back of the per-stream frame counts and the batch's highest recovery row (they size the grids and pick the decoder),
// then the scatter pass, the batched decoder on the frames that need it (sdrhip_fec.cpp, unchanged) and the copy of its output
// to the frames' places.  The collector state is double-buffered on the device: a call reads state[cur], writes
// state[cur ^ 1], and only a call that got past every check flips `cur` (an SDRHIP_EINVAL call consumes nothing).
#include "sdrhip_host.h"

#include <cstring>
#include <memory>
#include <new>
#include <vector>

using namespace sdrhip;

struct sdrhip_fecbuf {
    CtxRef ctx;                  // (first: released last)
    int nstreams;
    int cur = 0;                 // state[cur] is the committed collector state
    DevBuf state[2];             // [S] FecBufState each
    DevBuf carry;                // [2][S][128][512] the open slots' first 128 super blocks
    DevBuf small;                // ndg [S], job_off [S + 1], dbase [S], rec_base [S] (int64), counts [S][FB_COUNTS], pub [S][max_frames]
    DevBuf rec, stage, dmap, dec_out, dec_b0;
    DevBuf hin, hout, hb0;       // SDRHIP_MEM_HOST staging on the device
    DevBuf demux;                // sdrhip_fecbuf_write_and_read_tagged: the places of the datagrams, then the rows KX sorted them into
    PinnedBuf pin_up, pin_down, pin_in;
    // ---- asynchronous Tx batches (sdrhip_tx_submit_datagrams): the host's shadow of the classification part of state[cur]
    std::vector<FecBufShadow> shadow;
    bool shadow_ok = false;      // false: refreshed from the device before the next asynchronous batch (creation, reset, a synchronous call)
    int async_busy = 0;          // the owning Tx / Rx handle has asynchronous datagram batches in flight: reset and write_and_read are refused
    DevBuf atab;                 // their tables, counts and public records (fecbuf_packed)
    // ---- the Rx pipe fed datagrams (sdrhip_rx_process_datagrams): samples each stream holds back between calls (fecbuf_join_carry)
    DevBuf join_carry;
    std::vector<size_t> join_carry_host;
    StreamMask reset_mask;       // sdrhip_fecbuf_reset_streams
    explicit sdrhip_fecbuf(sdrhip_ctx *c) : ctx(c) {}
    FecBufState *st(int half) const { return state[half].as<FecBufState>(); }
};

namespace sdrhip {
void fecbuf_fresh_state(FecBufState *x)
{
    memset(x, 0, sizeof(*x));
    x->head = -1; x->maxrow = -1; x->b0 = -1;
    x->min_blocks = 256;
    // MetaDataFEC::init(): zero, m_nbFECBlocks = -1 (byte 11)
    x->cur_meta[2] = x->out_meta[2] = 0xff000000u;
}

void fecbuf_reset_part(sdrhip_fecbuf *b, StreamResetArgs *a)
{
    a->fb[0] = b->st(0); a->fb[1] = b->st(1);
    a->carry = b->join_carry.as<unsigned>(); // (NULL while no datagram entry of an Rx pipe has run: nothing is held back)
    fecbuf_fresh_state(&a->fb_init.st);
}

void fecbuf_reset_done(sdrhip_fecbuf *b, const uint8_t *mask)
{
    // the host's copies follow by themselves: no read-back, and the shadow stays valid for the next asynchronous batch
    FecBufShadow fresh = FecBufShadow();
    fresh.head = -1; fresh.maxrow = -1;
    for (int s = 0; s < b->nstreams; ++s) {
        if (mask && !mask[s]) continue;
        if (b->shadow_ok) b->shadow[(size_t)s] = fresh;
        if (b->join_carry.p) b->join_carry_host[(size_t)s] = 0;
    }
}

void fecbuf_stream_ref(sdrhip_fecbuf *b, int s, FecBufStreamRef *out)
{
    out->st[0] = b->st(b->cur) + s; out->st[1] = b->st(b->cur ^ 1) + s;
    out->carry = b->carry.as<uint8_t>() + (size_t)s * 128 * SDRHIP_UDPSIZE;
    out->carry_half = (size_t)b->nstreams * 128 * SDRHIP_UDPSIZE;
}

void fecbuf_import_host(sdrhip_fecbuf *b, int s, const FecBufState &st, size_t carry)
{
    if (b->shadow_ok) {
        FecBufShadow &h = b->shadow[(size_t)s];
        h.head = st.head; h.count = st.count; h.recov = st.recov; h.maxrow = st.maxrow; h.dup = st.dup;
        for (int q = 0; q < 4; ++q) h.pres[q] = st.pres[q];
    }
    if (b->join_carry.p) b->join_carry_host[(size_t)s] = carry;
}
} // namespace sdrhip

namespace {
constexpr size_t PAYLOAD = (size_t)127 * SDRHIP_BLOCK_BYTES;

// the per-call table of a driver, as byte offsets that hold for the host's copy and the device's alike.  The host fills and
// uploads [0, upload): ints [ndg S][job_off S + 1][dbase S] (packed: [expect S x 4]) [pad], then int64 rec_base [S] (packed:
// dg_off [S]).  Behind them the device alone has the counts [S][FB_COUNTS] and the public records [S][max_frames]
struct FecBufTable {
    bool packed;
    size_t ndg, job_off, dbase, expect, rec_base, dg_off, counts, pub;
    size_t upload, total;
};
FecBufTable fecbuf_table(int S, size_t max_frames, bool packed)
{
    const size_t n = (size_t)S;
    FecBufTable t;
    t.packed = packed;
    t.ndg = 0; t.job_off = n * 4; t.dbase = (2 * n + 1) * 4; t.expect = (3 * n + 1) * 4;
    // (the synchronous table has neither expect nor dg_off; it keeps the one spare int it always had in front of its padding)
    t.rec_base = (((packed ? 7 * n + 1 : 3 * n + 2) + 3) & ~(size_t)3) * 4;
    t.dg_off = t.rec_base + n * 8;
    t.counts = t.dg_off + (packed ? n * 8 : 0);
    t.pub = t.counts + n * FB_COUNTS * 4;
    t.upload = t.counts;
    t.total = t.pub + n * max_frames * sizeof(FecBufPub);
    return t;
}
template <class T> T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off); }

// what a call brings, into the host's table: ndg, rec_base, packed: dg_off; returns the internal records the call needs
long long table_inputs(const FecBufTable &t, void *host, const size_t *n_dgrams, int S)
{
    int *ndg = at<int>(host, t.ndg);
    long long *rb = at<long long>(host, t.rec_base), *doff = at<long long>(host, t.dg_off);
    long long nrec = 0, off = 0;
    for (int s = 0; s < S; ++s) {
        ndg[s] = (int)n_dgrams[s];
        rb[s] = nrec; nrec += (long long)n_dgrams[s] + 1;
        if (t.packed) { doff[s] = off; off += (long long)(n_dgrams[s] * SDRHIP_UDPSIZE); }
    }
    return nrec;
}

// what the classification gives, into the host's table: the prefix sums job_off and dbase (packed: expect, for the shadow check)
// over stream s's {K, D, maxrow, maxrec} at x + s * stride (the read-back counts, or the shadow's res); returns the grids and
// the batch's highest recovery row and count
struct FecBufSums {
    int njobs, nslots, maxrow, maxrec;
};
FecBufSums table_sums(const FecBufTable &t, void *host, const int *x, size_t stride, int S)
{
    int *job_off = at<int>(host, t.job_off), *dbase = at<int>(host, t.dbase), *expect = at<int>(host, t.expect);
    FecBufSums n = {0, 0, -1, 0};
    for (int s = 0; s < S; ++s, x += stride) {
        job_off[s] = n.njobs; n.njobs += x[FB_K] + 1;
        dbase[s] = n.nslots; n.nslots += x[FB_D];
        for (int q = 0; t.packed && q < 4; ++q) expect[4 * s + q] = x[q];
        n.maxrow = x[FB_MAXROW] > n.maxrow ? x[FB_MAXROW] : n.maxrow;
        n.maxrec = x[FB_MAXREC] > n.maxrec ? x[FB_MAXREC] : n.maxrec;
    }
    job_off[S] = n.njobs;
    return n;
}

// the kernels' arguments but the decoder's scratch (fecbuf_scratch): the table at `dev`, the records, the state and the carry
FecBufArgs fecbuf_args(const sdrhip_fecbuf *b, const FecBufTable &t, uint8_t *dev, const uint8_t *dg, size_t dg_stride, uint8_t *data_out,
                       size_t data_stride, uint8_t *block0_out, size_t max_frames)
{
    FecBufArgs a;
    memset(&a, 0, sizeof(a));
    a.dg = dg; a.dg_stride = dg_stride;
    a.ndg = at<const int>(dev, t.ndg);
    a.job_off = at<const int>(dev, t.job_off);
    a.dbase = at<const int>(dev, t.dbase);
    a.rec_base = at<const long long>(dev, t.rec_base);
    a.counts = at<int>(dev, t.counts);
    a.pub = at<FecBufPub>(dev, t.pub);
    a.rec = b->rec.as<FecBufRec>();
    a.max_frames = (int)max_frames;
    a.st_cur = b->st(b->cur); a.st_next = b->st(b->cur ^ 1);
    a.carry_cur_base = b->carry.as<uint8_t>(); a.carry_base = b->carry.as<uint8_t>();
    a.nstreams = b->nstreams;
    a.data_out = data_out; a.data_stride = data_stride; a.block0_out = block0_out;
    return a;
}

// everything that can fail for want of memory before the state moves on: staging, map and decoder output of nslots frames
// (settled, asynchronous batches: a buffer that grows waits for the batches in flight)
int fecbuf_scratch(sdrhip_fecbuf *b, FecBufArgs &a, int nslots, bool settled)
{
    if (nslots <= 0) return SDRHIP_OK; // (a.stage .. a.dec_b0 stay NULL: no job has a staging slot)
    sdrhip_ctx *c = b->ctx;
    const size_t n = (size_t)nslots;
    auto grow = [&](DevBuf &d, size_t bytes) { return settled ? reserve_settled(c, d, bytes) : d.reserve(bytes); };
    int rc;
    if ((rc = grow(b->stage, n * 128 * SDRHIP_UDPSIZE))) return rc;
    if ((rc = grow(b->dmap, n * 2 * sizeof(int)))) return rc;
    if ((rc = grow(b->dec_out, n * PAYLOAD))) return rc;
    if (a.block0_out && (rc = grow(b->dec_b0, n * SDRHIP_BLOCK_BYTES))) return rc;
    a.stage = b->stage.as<uint8_t>(); a.dmap = b->dmap.as<int>();
    a.dec_out = b->dec_out.as<uint8_t>(); a.dec_b0 = a.block0_out ? b->dec_b0.as<uint8_t>() : nullptr;
    return SDRHIP_OK;
}

// tables known, scratch reserved: the scatter pass, the commit, the batched decoder on the frames that need it and the copy of
// its output to the frames' places.  dg_off (device): the packed passes (else the strided ones); join: their row forms.  next /
// committed (asynchronous batches): the shadow the commit moves to, and whether it happened (a failure behind it loses the batch)
int fecbuf_passes(sdrhip_fecbuf *b, const FecBufArgs &a, const long long *dg_off, const FecBufJoin *join, const FecBufSums &n,
                  const std::vector<FecBufShadow> *next, bool *committed)
{
    sdrhip_ctx *c = b->ctx;
    const unsigned *row_off = join ? join->row_off : nullptr;
    const int kind = (dg_off ? 2 : 0) | (join ? 1 : 0);
    hipError_t e = kind == 3   ? launch_fecbuf_scatter_packed_rows(a, dg_off, row_off, n.njobs, n.nslots, c->stream)
                   : kind == 2 ? launch_fecbuf_scatter_packed(a, dg_off, n.njobs, n.nslots, c->stream)
                   : kind == 1 ? launch_fecbuf_scatter_rows(a, row_off, n.njobs, c->stream)
                               : launch_fecbuf_scatter(a, n.njobs, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf scatter launch: %s", hipGetErrorString(e));
    b->cur ^= 1; // (committed: the scatter pass has written the new carry slots)
    if (next) b->shadow = *next;
    if (committed) *committed = true;
    if (n.nslots <= 0) return SDRHIP_OK;
    // the promise is the batch's highest collected row, never a count: <= 32 rows (indices 0..31) take the one-launch decoder
    const int max_rows = (n.maxrow < 32 && n.maxrec <= 32) ? 32 : 128;
    if (int rc = fec_decode_device(c, b->stage.as<uint8_t>(), (size_t)128 * SDRHIP_UDPSIZE, nullptr, (size_t)n.nslots, b->dec_out.as<uint8_t>(), PAYLOAD,
                                   a.block0_out ? b->dec_b0.as<uint8_t>() : nullptr, nullptr, nullptr, max_rows))
        return rc;
    e = kind == 3   ? launch_fecbuf_copy_guarded_rows(a, row_off, n.nslots, c->stream)
        : kind == 2 ? launch_fecbuf_copy_guarded(a, n.nslots, c->stream)
        : kind == 1 ? launch_fecbuf_copy_rows(a, row_off, n.nslots, c->stream)
                    : launch_fecbuf_copy(a, n.nslots, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf copy launch: %s", hipGetErrorString(e));
    return SDRHIP_OK;
}

int fecbuf_init_state(sdrhip_fecbuf *b)
{
    std::vector<FecBufState> st((size_t)b->nstreams);
    for (FecBufState &x : st) fecbuf_fresh_state(&x);
    b->cur = 0;
    b->shadow_ok = false;
    if (b->join_carry.p) { // (the remainder rows go with the collector)
        HIP_TRY(hipMemsetAsync(b->join_carry.p, 0, (size_t)b->nstreams * sizeof(unsigned), b->ctx->stream));
        b->join_carry_host.assign((size_t)b->nstreams, 0);
    }
    HIP_TRY(link_copy(b->ctx, b->st(0), st.data(), st.size() * sizeof(FecBufState), hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    return SDRHIP_OK;
}

// the device-pointer core: dgrams / data_out / block0_out on the device
int fecbuf_device(sdrhip_fecbuf *b, const uint8_t *dg, const size_t *n_dgrams, size_t dg_stride, uint8_t *data_out, size_t data_stride,
                  uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames, const FecBufJoin *join = nullptr)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    b->shadow_ok = false; // (the collector moves without the host's shadow)
    const FecBufTable t = fecbuf_table(S, max_frames, false);
    if ((rc = b->small.reserve(t.total))) return rc;
    if ((rc = b->pin_up.reserve(t.upload))) return rc;
    if ((rc = b->pin_down.reserve(t.total - t.counts))) return rc;
    const long long nrec = table_inputs(t, b->pin_up.p, n_dgrams, S);
    if ((rc = b->rec.reserve((size_t)nrec * sizeof(FecBufRec)))) return rc;
    uint8_t *sm = b->small.as<uint8_t>();
    HIP_TRY(link_copy(c, sm, b->pin_up.p, t.upload, hipMemcpyHostToDevice, c->stream));
    b->pin_up.mark(c->stream);

    FecBufArgs a = fecbuf_args(b, t, sm, dg, dg_stride, data_out, data_stride, block0_out, max_frames);
    hipError_t e = launch_fecbuf_classify(a, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf classify launch: %s", hipGetErrorString(e));
    // the one read-back: counts + public records
    HIP_TRY(link_copy(c, b->pin_down.p, sm + t.counts, t.total - t.counts, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int *cnt = b->pin_down.as<int>();
    const FecBufPub *pub = at<const FecBufPub>(b->pin_down.p, t.pub - t.counts);
    bool room = true;
    for (int s = 0; s < S; ++s) {
        n_frames[s] = (size_t)cnt[(size_t)s * FB_COUNTS + FB_K];
        if (n_frames[s] > max_frames) room = false;
    }
    const FecBufSums n = table_sums(t, b->pin_up.p, cnt, FB_COUNTS, S);
    if (!room) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: a stream releases more than max_frames = %zu frames (n_frames has the counts; nothing was consumed)", max_frames);
    if (join && join->admit && (rc = join->admit(join->arg, n_frames))) return rc;
    if ((rc = fecbuf_scratch(b, a, n.nslots, false))) return rc;
    for (int s = 0; s < S; ++s) {
        const FecBufPub *p = pub + (size_t)s * max_frames;
        for (size_t k = 0; k < n_frames[s]; ++k) {
            sdrhip_fecbuf_frame &o = info_out[(size_t)s * max_frames + k];
            o.frame_index = p[k].frame_index; o.block_count = p[k].block_count; o.recovery_count = p[k].recovery_count; o.flags = p[k].flags;
        }
    }
    // (job_off and dbase: the columns the read-back filled)
    HIP_TRY(link_copy(c, sm + t.job_off, b->pin_up.as<uint8_t>() + t.job_off, t.expect - t.job_off, hipMemcpyHostToDevice, c->stream));
    b->pin_up.mark(c->stream);
    return fecbuf_passes(b, a, nullptr, join, n, nullptr, nullptr);
}
} // namespace

extern "C" int sdrhip_fecbuf_create(sdrhip_ctx *ctx, int nstreams, sdrhip_fecbuf **out)
{
    if (!ctx || !out || nstreams <= 0 || nstreams > 65535) return fail(SDRHIP_EINVAL, "fecbuf_create: bad argument");
    std::unique_ptr<sdrhip_fecbuf> b; // (in front of the lock: a failure deletes it behind the lock's scope)
    sdrhip::CtxLock lock_(ctx);
    if (sdrhip_device_count() <= 0) return fail(SDRHIP_EDEVICE, "fecbuf_create: no GPU");
    HIP_TRY(hipSetDevice(ctx->device));
    b.reset(new (std::nothrow) sdrhip_fecbuf(ctx));
    if (!b) return fail(SDRHIP_ENOMEM, "out of host memory");
    b->nstreams = nstreams;
    const size_t sb = (size_t)nstreams * sizeof(FecBufState), cb = (size_t)2 * nstreams * 128 * SDRHIP_UDPSIZE;
    if (b->state[0].alloc_exact(sb) || b->state[1].alloc_exact(sb) || b->carry.alloc_exact(cb)) return fail(SDRHIP_ENOMEM, "hipMalloc fecbuf state");
    int rc = fecbuf_init_state(b.get());
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; } // (nothing of the upload stays in flight when the state goes)
    *out = b.release();
    return SDRHIP_OK;
}

extern "C" void sdrhip_fecbuf_destroy(sdrhip_fecbuf *b)
{
    if (!b) return;
    sdrhip_ctx *c = b->ctx;
    {
        sdrhip::CtxLock lock_(c);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    delete b; // (no lock held: the last reference frees the mutex)
}

extern "C" int sdrhip_fecbuf_reset(sdrhip_fecbuf *b)
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip::CtxLock lock_(b->ctx);
    if (b->async_busy) return fail(SDRHIP_EINVAL, "fecbuf_reset: the owning pipe's asynchronous datagram batches are in flight: collect them first");
    HIP_TRY(hipSetDevice(b->ctx->device));
    return fecbuf_init_state(b);
}

// (on a pipe's own collector this is allowed while the pipe's datagram batches are in flight: they keep what they were enqueued
// with, the launch goes behind them and the shadow already stands behind the last submit)
extern "C" int sdrhip_fecbuf_reset_streams(sdrhip_fecbuf *b, const uint8_t *mask)
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip::CtxLock lock_(b->ctx);
    return stream_reset_bank(b->ctx, b->reset_mask, mask, b->nstreams,
                             [b](StreamResetArgs *a) { fecbuf_reset_part(b, a); }, [b](const uint8_t *m) { fecbuf_reset_done(b, m); });
}

namespace {
// the counts of one call / batch (`unit` names it in the message): *sum = all datagrams, *nmax = the most of a stream
int count_dgrams(int S, const size_t *n_dgrams, const char *who, const char *unit, size_t *sum, size_t *nmax)
{
    *sum = *nmax = 0;
    for (int s = 0; s < S; ++s) {
        if (n_dgrams[s] > 0x3fffffffu) return fail(SDRHIP_EINVAL, "%s: too many datagrams in one %s", who, unit);
        *sum += n_dgrams[s];
        *nmax = n_dgrams[s] > *nmax ? n_dgrams[s] : *nmax;
    }
    return SDRHIP_OK;
}

// the datagram arguments of a call (sdrhip_fecbuf_write_and_read, sdrhip_tx_process_datagrams); *nmax = the most datagrams of a stream
int check_dgrams(int S, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, const char *who, size_t *nmax)
{
    if (int e = check_mem(mem)) return e;
    size_t sum = 0;
    if (int e = count_dgrams(S, n_dgrams, who, "call", &sum, nmax)) return e;
    if (*nmax > 0 && !dgrams) return fail(SDRHIP_EINVAL, "%s: NULL dgrams", who);
    if (S > 1 && *nmax > 0 && dgram_stride_bytes < *nmax * SDRHIP_UDPSIZE) return fail(SDRHIP_EINVAL, "%s: dgram_stride_bytes below n_dgrams x 512", who);
    return SDRHIP_OK;
}

// host memory: the datagrams go up as one 2-D copy (from sdrhip_host_alloc memory in place, else through a pinned buffer) to
// b->hin, `row` bytes per stream.  exact (the Rx pipe's join: its link traffic is bounded by the datagrams themselves): streams
// with fewer datagrams than the longest go up one by one, n_dgrams[s] x 512 bytes each
int upload_dgrams(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, size_t row, bool exact = false)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    if (!row) return SDRHIP_OK;
    if ((rc = b->hin.reserve((size_t)S * row))) return rc;
    const uint8_t *src = dgrams;
    size_t sstride = S > 1 ? dgram_stride_bytes : row;
    if (!host_is_pinned(dgrams, (size_t)(S - 1) * sstride + row)) {
        if ((rc = b->pin_in.reserve((size_t)S * row))) return rc;
        for (int s = 0; s < S; ++s) memcpy(b->pin_in.as<uint8_t>() + (size_t)s * row, dgrams + (size_t)s * sstride, n_dgrams[s] * SDRHIP_UDPSIZE);
        src = b->pin_in.as<uint8_t>(); sstride = row;
    }
    bool ragged = false;
    for (int s = 0; s < S; ++s) ragged = ragged || n_dgrams[s] * SDRHIP_UDPSIZE != row;
    if (exact && ragged) {
        for (int s = 0; s < S; ++s)
            if (n_dgrams[s])
                HIP_TRY(link_copy(c, b->hin.as<uint8_t>() + (size_t)s * row, src + (size_t)s * sstride, n_dgrams[s] * SDRHIP_UDPSIZE,
                                  hipMemcpyHostToDevice, c->stream));
    } else
        HIP_TRY(link_copy2d(c, b->hin.p, row, src, sstride, row, (size_t)S, hipMemcpyHostToDevice, c->stream));
    if (src != dgrams) b->pin_in.mark(c->stream);
    return SDRHIP_OK;
}

// the output arguments of the bank's call (`who`: sdrhip_fecbuf_write_and_read and its tagged twin), and their alignment on the device
int check_outputs(int S, const uint8_t *data_out, size_t data_stride_bytes, size_t max_frames, const sdrhip_fecbuf_frame *info_out, const char *who)
{
    if (max_frames > 0 && (!data_out || !info_out)) return fail(SDRHIP_EINVAL, "%s: NULL data_out / info_out", who);
    if (max_frames > 0x3fffffffu) return fail(SDRHIP_EINVAL, "%s: max_frames too large", who);
    if (S > 1 && max_frames > 0 && data_stride_bytes < max_frames * PAYLOAD) return fail(SDRHIP_EINVAL, "%s: data_stride_bytes below max_frames x 127 x 508", who);
    return SDRHIP_OK;
}
int check_outputs_aligned(int S, const uint8_t *data_out, size_t data_stride_bytes, const uint8_t *block0_out, const char *who)
{
    if ((reinterpret_cast<uintptr_t>(data_out) & 3u) || (reinterpret_cast<uintptr_t>(block0_out) & 3u) || (S > 1 && data_stride_bytes % 4))
        return fail(SDRHIP_EALIGN, "%s: data_out / block0_out / data_stride_bytes must be 4-byte aligned", who);
    return SDRHIP_OK;
}
// the call behind its checks.  staged (host memory): the datagrams are on the device already (fecbuf_collect)
int write_and_read_checked(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, uint8_t *data_out,
                           size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames,
                           int mem, const uint8_t *staged);
} // namespace

extern "C" int sdrhip_fecbuf_write_and_read(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                            uint8_t *data_out, size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames,
                                            sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem)
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip_ctx *c = b->ctx;
    sdrhip::CtxLock lock_(c);
    const int S = b->nstreams;
    if (!n_dgrams || !n_frames) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: NULL n_dgrams / n_frames");
    if (b->async_busy) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: the owning pipe's asynchronous datagram batches are in flight: collect them first");
    size_t nmax = 0;
    int rc;
    if ((rc = check_dgrams(S, dgrams, n_dgrams, dgram_stride_bytes, mem, "fecbuf_write_and_read", &nmax))) return rc;
    if ((rc = check_outputs(S, data_out, data_stride_bytes, max_frames, info_out, "fecbuf_write_and_read"))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (mem == SDRHIP_MEM_DEVICE) {
        if ((nmax > 0 && !aligned16(dgrams)) || (S > 1 && dgram_stride_bytes % 16))
            return fail(SDRHIP_EALIGN, "fecbuf_write_and_read: dgrams / dgram_stride_bytes must be 16-byte aligned");
        if ((rc = check_outputs_aligned(S, data_out, data_stride_bytes, block0_out, "fecbuf_write_and_read"))) return rc;
    }
    return write_and_read_checked(b, dgrams, n_dgrams, dgram_stride_bytes, data_out, data_stride_bytes, block0_out, max_frames, info_out, n_frames, mem,
                                  nullptr);
}

namespace {
int write_and_read_checked(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, uint8_t *data_out,
                           size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames,
                           int mem, const uint8_t *staged)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    // both memories go through fecbuf_collect (host: it stages the datagrams and downloads block 0).  Host memory adds only what its
    // other callers do not need, their data staying on the device: the frames go to b->hout and come down from there below
    const bool host = mem == SDRHIP_MEM_HOST;
    const size_t drow = max_frames * PAYLOAD;
    if (host && drow && (rc = b->hout.reserve((size_t)S * drow + 4))) return rc;
    const int *counts = nullptr;
    rc = fecbuf_collect(b, dgrams, n_dgrams, dgram_stride_bytes, mem, host ? b->hout.as<uint8_t>() : data_out, host ? drow : data_stride_bytes,
                        block0_out, max_frames, info_out, n_frames, &counts, nullptr, staged);
    if (rc || !host) return rc;
    for (int s = 0; s < S; ++s)
        if (n_frames[s])
            HIP_TRY(link_copy(c, data_out + (size_t)s * data_stride_bytes, b->hout.as<uint8_t>() + (size_t)s * drow, n_frames[s] * PAYLOAD,
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}
} // namespace

namespace sdrhip {
int fecbuf_check_dgrams(const sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, const char *who)
{
    size_t nmax = 0;
    int rc = check_dgrams(b->nstreams, dgrams, n_dgrams, dgram_stride_bytes, mem, who, &nmax);
    if (rc) return rc;
    if (mem == SDRHIP_MEM_DEVICE && ((nmax > 0 && !aligned16(dgrams)) || (b->nstreams > 1 && dgram_stride_bytes % 16)))
        return fail(SDRHIP_EALIGN, "%s: dgrams / dgram_stride_bytes must be 16-byte aligned", who);
    return SDRHIP_OK;
}

int fecbuf_collect(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, uint8_t *data_out,
                   size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames,
                   const int **counts, const FecBufJoin *join, const uint8_t *staged)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    if (mem == SDRHIP_MEM_DEVICE)
        rc = fecbuf_device(b, dgrams, n_dgrams, dgram_stride_bytes, data_out, data_stride_bytes, block0_out, max_frames, info_out, n_frames, join);
    else {
        size_t nmax = 0;
        for (int s = 0; s < S; ++s) nmax = n_dgrams[s] > nmax ? n_dgrams[s] : nmax;
        const size_t row = nmax * SDRHIP_UDPSIZE;
        if (block0_out && max_frames && (rc = b->hb0.reserve((size_t)S * max_frames * SDRHIP_BLOCK_BYTES))) return rc;
        if (!staged && (rc = upload_dgrams(b, dgrams, n_dgrams, dgram_stride_bytes, row, join != nullptr))) return rc;
        rc = fecbuf_device(b, staged ? staged : b->hin.as<uint8_t>(), n_dgrams, row, data_out, data_stride_bytes, block0_out ? b->hb0.as<uint8_t>() : nullptr,
                           max_frames, info_out, n_frames, join);
        if (!rc && block0_out)
            for (int s = 0; s < S; ++s)
                if (n_frames[s])
                    HIP_TRY(link_copy(c, block0_out + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES, b->hb0.as<uint8_t>() + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES,
                                      n_frames[s] * SDRHIP_BLOCK_BYTES, hipMemcpyDeviceToHost, c->stream));
    }
    if (rc) return rc;
    *counts = at<const int>(b->small.p, fecbuf_table(S, max_frames, false).counts);
    return SDRHIP_OK;
}
} // namespace sdrhip

// --------------------------------------------------------------------------- asynchronous Tx batches: no read-back
// sdrhip_tx_submit_datagrams sizes the grids and picks the decoder from the host's own run of the classify pass's rule over the
// headers it stages anyway (4 bytes per 512): a per-stream shadow of head, count, recov, maxrow, pres, dup gives every number the
// bank's read-back gives (SDRdaemonFECBuffer.cpp:112-170).  The classify pass still writes its own counts (the interpolator reads
// them); a check kernel compares the two and raises "fecbuf_shadow_mismatch".
namespace sdrhip {
int fecbuf_shadow(sdrhip_fecbuf *b, std::vector<FecBufShadow> *out)
{
    const int S = b->nstreams;
    if (!b->shadow_ok) { // (the first batch after anything else moved the collector: one copy + one synchronisation)
        std::vector<FecBufState> st((size_t)S);
        HIP_TRY(hipMemcpyAsync(st.data(), b->st(b->cur), st.size() * sizeof(FecBufState), hipMemcpyDeviceToHost, b->ctx->stream));
        HIP_TRY(hipStreamSynchronize(b->ctx->stream));
        b->shadow.assign((size_t)S, FecBufShadow());
        for (int s = 0; s < S; ++s) {
            FecBufShadow &h = b->shadow[(size_t)s];
            const FecBufState &x = st[(size_t)s];
            h.head = x.head; h.count = x.count; h.recov = x.recov; h.maxrow = x.maxrow; h.dup = x.dup;
            for (int q = 0; q < 4; ++q) h.pres[q] = x.pres[q];
        }
        b->shadow_ok = true;
    }
    *out = b->shadow;
    return SDRHIP_OK;
}

void fecbuf_shadow_step(FecBufShadow &h, uint32_t hd, int res[4])
{
    const int fi = (int)(hd & 0xffffu), bi = (int)((hd >> 16) & 0xffu);
    if (fi != h.head) { // another frame index releases the open slot (the first datagram: the initial one)
        ++res[0];
        if (h.count >= 128 && h.recov > 0 && !h.dup) { // (to the decoder: the frames cm256_decode repairs)
            ++res[1];
            res[2] = h.maxrow > res[2] ? h.maxrow : res[2];
            res[3] = h.recov > res[3] ? h.recov : res[3];
        }
        h.head = fi; h.count = 0; h.recov = 0; h.maxrow = -1; h.dup = 0;
        h.pres[0] = h.pres[1] = h.pres[2] = h.pres[3] = 0u;
    }
    if (h.count < 128) { // (the first 128 arrivals)
        if (bi >= 128) {
            ++h.recov;
            h.maxrow = bi - 128 > h.maxrow ? bi - 128 : h.maxrow;
        } else {
            const unsigned bit = 1u << (bi & 31);
            if (h.pres[bi >> 5] & bit) h.dup = 1;
            h.pres[bi >> 5] |= bit;
        }
    }
    ++h.count;
}

void fecbuf_shadow_run(FecBufShadow &h, const uint8_t *dg, size_t n, int res[4])
{
    int r[4] = {0, 0, -1, 0}; // K, D, maxrow, maxrec
    for (size_t i = 0; i < n; ++i) {
        uint32_t hd;
        memcpy(&hd, dg + i * SDRHIP_UDPSIZE, 4);
        fecbuf_shadow_step(h, hd, r);
    }
    res[0] = r[0]; res[1] = r[1]; res[2] = r[2]; res[3] = r[3];
}

int fecbuf_tag_counts(int S, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total, const char *who, size_t *counts, size_t *sum,
                      size_t *nmax)
{
    *sum = *nmax = 0;
    for (int s = 0; s < S; ++s) counts[s] = 0;
    if (S > 65535) return fail(SDRHIP_EINVAL, "%s: a bank of more than 65535 streams has no 16-bit tags", who);
    if (n_total > 0x3fffffffu) return fail(SDRHIP_EINVAL, "%s: too many datagrams in one batch", who);
    if (n_total && !stream_of) return fail(SDRHIP_EINVAL, "%s: NULL stream_of", who);
    if (n_total && !dgrams) return fail(SDRHIP_EINVAL, "%s: NULL dgrams", who);
    for (size_t i = 0; i < n_total; ++i) {
        const unsigned t = stream_of[i];
        if (t == SDRHIP_DGRAM_SKIP) continue;
        if (t >= (unsigned)S) return fail(SDRHIP_EINVAL, "%s: stream_of[%zu] = %u is neither a stream of the bank nor SDRHIP_DGRAM_SKIP", who, i, t);
        ++counts[t];
    }
    for (int s = 0; s < S; ++s) {
        *sum += counts[s];
        *nmax = counts[s] > *nmax ? counts[s] : *nmax;
    }
    return SDRHIP_OK;
}

// the places of a tagged array's datagrams: dest[i] = next[tag]++ (next[s] = stream s's first place on entry), 0xffffffff: skipped
static void tag_dest(const uint16_t *tags, size_t n_total, size_t *next, uint32_t *dest)
{
    for (size_t i = 0; i < n_total; ++i) dest[i] = tags[i] == SDRHIP_DGRAM_SKIP ? 0xffffffffu : (uint32_t)next[tags[i]]++;
}

// ---- a batch of sdrhip_tx_submit_datagrams / sdrhip_rx_submit_datagrams (`who`) on its way up
int fecbuf_batch_check(FecBufBatch *in, int S, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, const char *who)
{
    in->S = S; in->dgrams = dgrams; in->n_dgrams = n_dgrams; in->stride = dgram_stride_bytes;
    if (int e = count_dgrams(S, n_dgrams, who, "batch", &in->sum, &in->nmax)) return e;
    in->packed = dgram_stride_bytes == SDRHIP_PACKED || S == 1;
    in->bytes_in = in->dev_bytes = in->sum * SDRHIP_UDPSIZE;
    in->inplace = false;
    if (in->sum && !dgrams) return fail(SDRHIP_EINVAL, "%s: NULL dgrams", who);
    if (!in->packed && dgram_stride_bytes < in->nmax * SDRHIP_UDPSIZE)
        return fail(SDRHIP_EINVAL, "%s: dgram_stride_bytes is neither SDRHIP_PACKED nor at least the largest count x 512", who);
    return SDRHIP_OK;
}

int fecbuf_batch_check_tagged(FecBufBatch *in, int S, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total, const char *who)
{
    in->S = S; in->dgrams = dgrams; in->stride = SDRHIP_PACKED;
    in->packed = true; in->inplace = false;
    in->tags = stream_of; in->n_total = n_total;
    in->counts.assign((size_t)S, 0);
    in->n_dgrams = in->counts.data();
    if (int e = fecbuf_tag_counts(S, dgrams, stream_of, n_total, who, in->counts.data(), &in->sum, &in->nmax)) return e;
    in->bytes_in = n_total * SDRHIP_UDPSIZE;
    in->dev_bytes = in->sum * SDRHIP_UDPSIZE + n_total * (SDRHIP_UDPSIZE + sizeof(uint32_t));
    return SDRHIP_OK;
}

// stream s's row in the caller's memory; off = the bytes of the streams in front of it
static const uint8_t *row_of(const FecBufBatch &in, int s, size_t off)
{
    return in.packed ? in.dgrams + off : in.dgrams + (size_t)s * in.stride;
}

// the tagged form: one memcpy, one walk in arrival order (the shadow's step and the datagram's place)
static int batch_stage_tagged(FecBufBatch *in, PinnedBuf &arena, PinnedBuf &tab, std::vector<FecBufShadow> &sh, int *res)
{
    const int S = in->S;
    const size_t n = in->n_total;
    in->inplace = n && host_is_pinned(in->dgrams, in->bytes_in);
    const uint8_t *src = in->dgrams;
    if (n && !in->inplace) {
        if (int rc = arena.reserve(in->bytes_in)) return rc; // (waits for the upload of this slot's last batch)
        memcpy(arena.p, in->dgrams, in->bytes_in);
        src = arena.as<uint8_t>();
    }
    // (dest lies behind the table fecbuf_packed fills: its reserve of the smaller size keeps the buffer)
    const size_t tab_bytes = fecbuf_table(S, 0, true).upload;
    if (int rc = tab.reserve(tab_bytes + n * sizeof(uint32_t))) return rc;
    in->dest = at<uint32_t>(tab.p, tab_bytes);
    std::vector<size_t> next((size_t)S);
    size_t first = 0;
    for (int s = 0; s < S; ++s) {
        next[(size_t)s] = first; first += in->counts[(size_t)s];
        int *r = res + (size_t)s * 4;
        r[0] = 0; r[1] = 0; r[2] = -1; r[3] = 0;
    }
    for (size_t i = 0; i < n; ++i) {
        const unsigned t = in->tags[i];
        if (t == SDRHIP_DGRAM_SKIP) { in->dest[i] = 0xffffffffu; continue; }
        in->dest[i] = (uint32_t)next[t]++;
        uint32_t hd;
        memcpy(&hd, src + i * SDRHIP_UDPSIZE, 4);
        fecbuf_shadow_step(sh[t], hd, res + (size_t)t * 4);
    }
    return SDRHIP_OK;
}

int fecbuf_batch_stage(FecBufBatch *in, PinnedBuf &arena, PinnedBuf &tab, std::vector<FecBufShadow> &sh, int *res)
{
    if (in->n_total) return batch_stage_tagged(in, arena, tab, sh, res);
    const int S = in->S;
    in->inplace = in->sum && host_is_pinned(in->dgrams, in->packed ? in->bytes_in : (size_t)(S - 1) * in->stride + in->nmax * SDRHIP_UDPSIZE);
    if (in->sum && !in->inplace)
        if (int rc = arena.reserve(in->bytes_in)) return rc; // (waits for the upload of this slot's last batch)
    size_t off = 0;
    for (int s = 0; s < S; ++s) {
        const size_t nb = in->n_dgrams[s] * SDRHIP_UDPSIZE;
        const uint8_t *src = row_of(*in, s, off);
        if (nb && !in->inplace) {
            memcpy(arena.as<uint8_t>() + off, src, nb);
            src = arena.as<uint8_t>() + off;
        }
        fecbuf_shadow_run(sh[(size_t)s], src, in->n_dgrams[s], res + (size_t)s * 4);
        off += nb;
    }
    return SDRHIP_OK;
}

int fecbuf_batch_upload(sdrhip_ctx *c, const FecBufBatch &in, PinnedBuf &arena, uint8_t *pk)
{
    if (in.n_total) { // tagged: the arrival array and its places behind the packed area, then KX
        uint8_t *raw = pk + in.sum * SDRHIP_UDPSIZE;
        uint32_t *dest = reinterpret_cast<uint32_t *>(raw + in.bytes_in);
        HIP_TRY(link_copy(c, raw, in.inplace ? static_cast<const void *>(in.dgrams) : arena.p, in.bytes_in, hipMemcpyHostToDevice, c->stream));
        if (!in.inplace) arena.mark(c->stream);
        HIP_TRY(link_copy(c, dest, in.dest, in.n_total * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        const hipError_t e = in.sum ? launch_dgram_demux(raw, dest, in.n_total, pk, c->stream) : hipSuccess;
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "datagram demultiplexer launch: %s", hipGetErrorString(e));
        return SDRHIP_OK;
    }
    if (in.sum && !in.inplace) {
        HIP_TRY(link_copy(c, pk, arena.p, in.bytes_in, hipMemcpyHostToDevice, c->stream));
        arena.mark(c->stream);
    } else if (in.sum) {
        size_t off = 0;
        for (int s = 0; s < in.S;) {
            const uint8_t *p0 = row_of(in, s, off);
            size_t n = in.n_dgrams[s] * SDRHIP_UDPSIZE;
            int j = s + 1;
            // (packed input is one run; a strided row joins the next one when it fills its stride)
            for (; j < in.S && p0 + n == row_of(in, j, off + n); ++j) n += in.n_dgrams[j] * SDRHIP_UDPSIZE;
            if (n) HIP_TRY(link_copy(c, pk + off, p0, n, hipMemcpyHostToDevice, c->stream));
            off += n;
            s = j;
        }
    }
    return SDRHIP_OK;
}

int fecbuf_batch_lost(const char *who, int rc)
{
    const std::string m = sdrhip_last_error();
    return fail(rc, "%s: %s (the batch is lost)", who, m.c_str());
}

int fecbuf_packed(sdrhip_fecbuf *b, const uint8_t *dg, const size_t *n_dgrams, const int *res, const std::vector<FecBufShadow> &next,
                  PinnedBuf &tab, uint8_t *data_out, size_t data_stride, uint8_t *block0_out, size_t max_frames, unsigned *mismatch,
                  bool *committed, const int **counts, const FecBufPub **pub, const FecBufJoin *join)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    *committed = false;
    const FecBufTable t = fecbuf_table(S, max_frames, true);
    if ((rc = tab.reserve(t.upload))) return rc; // (waits for the upload of this batch slot's last use)
    const long long nrec = table_inputs(t, tab.p, n_dgrams, S);
    const FecBufSums n = table_sums(t, tab.p, res, 4, S);
    // (a buffer that grows waits for the batches in flight)
    if ((rc = reserve_settled(c, b->atab, t.total))) return rc;
    if ((rc = reserve_settled(c, b->rec, (size_t)nrec * sizeof(FecBufRec)))) return rc;
    uint8_t *dev = b->atab.as<uint8_t>();
    FecBufArgs a = fecbuf_args(b, t, dev, dg, 0, data_out, data_stride, block0_out, max_frames);
    if ((rc = fecbuf_scratch(b, a, n.nslots, true))) return rc;
    HIP_TRY(hipMemcpyAsync(dev, tab.p, t.upload, hipMemcpyHostToDevice, c->stream)); // (not counted: a table)
    tab.mark(c->stream);
    const long long *dg_off = at<const long long>(dev, t.dg_off);
    hipError_t e = launch_fecbuf_classify_packed(a, dg_off, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf classify launch: %s", hipGetErrorString(e));
    if ((e = launch_fecbuf_shadow_check(a.counts, at<const int>(dev, t.expect), S, mismatch, c->stream)) != hipSuccess)
        return fail(SDRHIP_EDEVICE, "fecbuf shadow check launch: %s", hipGetErrorString(e));
    if (n.nslots > 0) HIP_TRY(hipMemsetAsync(a.dmap, 0xff, (size_t)n.nslots * 2 * sizeof(int), c->stream)); // (the guarded copy skips what stays -1)
    if ((rc = fecbuf_passes(b, a, dg_off, join, n, &next, committed))) return rc;
    *counts = a.counts;
    *pub = a.pub;
    return SDRHIP_OK;
}

void fecbuf_set_async_busy(sdrhip_fecbuf *b, bool busy) { b->async_busy = busy ? 1 : 0; }

int fecbuf_join_carry(sdrhip_fecbuf *b, unsigned **dev, std::vector<size_t> **host)
{
    if (!b->join_carry.p) {
        int rc = b->join_carry.reserve((size_t)b->nstreams * sizeof(unsigned));
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(b->join_carry.p, 0, (size_t)b->nstreams * sizeof(unsigned), b->ctx->stream));
        b->join_carry_host.assign((size_t)b->nstreams, 0);
    }
    *dev = b->join_carry.as<unsigned>();
    *host = &b->join_carry_host;
    return SDRHIP_OK;
}

const FecBufState *fecbuf_committed_state(const sdrhip_fecbuf *b) { return b->st(b->cur); }
} // namespace sdrhip

// --------------------------------------------------------------------------- the bank's call on an arrival-order array
// One walk over the tags for the counts (it refuses a bad tag before anything moves), one for the places: the bank's kernels read
// stream s's row at s * nmax * 512, so datagram i goes to row-start + its rank within the stream.  The array goes up as it is (host
// memory: in place or through ONE memcpy), KX sorts it into the handle's own rows, and the call goes on as the untagged one does.
extern "C" int sdrhip_fecbuf_write_and_read_tagged(sdrhip_fecbuf *b, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total,
                                                   uint8_t *data_out, size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames,
                                                   sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem)
{
    const char *who = "fecbuf_write_and_read_tagged";
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip_ctx *c = b->ctx;
    sdrhip::CtxLock lock_(c);
    const int S = b->nstreams;
    if (!n_frames) return fail(SDRHIP_EINVAL, "%s: NULL n_frames", who);
    if (b->async_busy) return fail(SDRHIP_EINVAL, "%s: the owning pipe's asynchronous datagram batches are in flight: collect them first", who);
    int rc;
    if ((rc = check_mem(mem))) return rc;
    std::vector<size_t> counts((size_t)S);
    size_t sum = 0, nmax = 0;
    if ((rc = fecbuf_tag_counts(S, dgrams, stream_of, n_total, who, counts.data(), &sum, &nmax))) return rc;
    if ((rc = check_outputs(S, data_out, data_stride_bytes, max_frames, info_out, who))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool host = mem == SDRHIP_MEM_HOST;
    if (!host) {
        if (n_total && !aligned16(dgrams)) return fail(SDRHIP_EALIGN, "%s: dgrams must be 16-byte aligned", who);
        if ((rc = check_outputs_aligned(S, data_out, data_stride_bytes, block0_out, who))) return rc;
    }
    const size_t row = nmax * SDRHIP_UDPSIZE;
    if (sum) {
        const size_t bytes = n_total * SDRHIP_UDPSIZE, rows_bytes = (size_t)S * row, dest_bytes = n_total * sizeof(uint32_t);
        const bool pinned = host && host_is_pinned(dgrams, bytes);
        const size_t staged_bytes = host && !pinned ? bytes : 0;
        if ((rc = b->pin_in.reserve(staged_bytes + dest_bytes))) return rc;
        if ((rc = b->demux.reserve(rows_bytes + dest_bytes))) return rc;
        if (host && (rc = b->hin.reserve(bytes))) return rc;
        uint32_t *dest = at<uint32_t>(b->pin_in.p, staged_bytes);
        std::vector<size_t> next((size_t)S);
        for (int s = 0; s < S; ++s) next[(size_t)s] = (size_t)s * nmax;
        tag_dest(stream_of, n_total, next.data(), dest);
        const uint8_t *src = dgrams;
        if (host) {
            const void *from = dgrams;
            if (!pinned) { memcpy(b->pin_in.p, dgrams, bytes); from = b->pin_in.p; }
            HIP_TRY(link_copy(c, b->hin.p, from, bytes, hipMemcpyHostToDevice, c->stream));
            src = b->hin.as<uint8_t>();
        }
        uint32_t *dest_dev = at<uint32_t>(b->demux.p, rows_bytes);
        HIP_TRY(link_copy(c, dest_dev, dest, dest_bytes, hipMemcpyHostToDevice, c->stream));
        b->pin_in.mark(c->stream);
        const hipError_t e = launch_dgram_demux(src, dest_dev, n_total, b->demux.as<uint8_t>(), c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "datagram demultiplexer launch: %s", hipGetErrorString(e));
    }
    return write_and_read_checked(b, b->demux.as<uint8_t>(), counts.data(), row, data_out, data_stride_bytes, block0_out, max_frames, info_out,
                                  n_frames, mem, sum && host ? b->demux.as<uint8_t>() : nullptr);
}

extern "C" int sdrhip_fecbuf_stats(sdrhip_fecbuf *b, int stream, int *cur_nb_blocks, int *cur_nb_recovery, int *min_nb_blocks, int *max_nb_recovery,
                                   uint8_t current_meta[24], uint8_t output_meta[24])
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip::CtxLock lock_(b->ctx);
    if (stream < 0 || stream >= b->nstreams) return fail(SDRHIP_EINVAL, "fecbuf_stats: stream out of range");
    HIP_TRY(hipSetDevice(b->ctx->device));
    FecBufState x;
    FecBufState *d = b->st(b->cur) + stream;
    HIP_TRY(link_copy(b->ctx, &x, d, sizeof(x), hipMemcpyDeviceToHost, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    if (cur_nb_blocks) *cur_nb_blocks = x.cur_blocks;
    if (cur_nb_recovery) *cur_nb_recovery = x.cur_recov;
    if (current_meta) memcpy(current_meta, x.cur_meta, 24);
    if (output_meta) memcpy(output_meta, x.out_meta, 24);
    // getMinNbBlocks / getMaxNbRecovery reset what they read (SDRdaemonFECBuffer.h:115-126)
    int upd[4] = {x.cur_blocks, x.cur_recov, x.min_blocks, x.max_recov};
    if (min_nb_blocks) { *min_nb_blocks = x.min_blocks; upd[2] = 256; }
    if (max_nb_recovery) { *max_nb_recovery = x.max_recov; upd[3] = 0; }
    if (min_nb_blocks || max_nb_recovery) {
        HIP_TRY(link_copy(b->ctx, &d->cur_blocks, upd, sizeof(upd), hipMemcpyHostToDevice, b->ctx->stream));
        HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    }
    return SDRHIP_OK;
}
