// sdrhip_fecbuf.cpp -- host side of the FEC buffer bank (include/sdrhip.h, sdrhip_fecbuf_*): nstreams SDRdaemonFECBuffer
// collectors fed raw datagrams.  A call: upload of the per-stream datagram counts, the classify pass (fecbuf_kernels.hip), ONE
// read-back of the per-stream frame counts and the batch's highest recovery row (they size the grids and pick the decoder),
// then the scatter pass, the batched decoder on the frames that need it (sdrhip_fec.cpp, unchanged) and the copy of its output
// to the frames' places.  The collector state is double-buffered on the device: a call reads state[cur], writes
// state[cur ^ 1], and only a call that got past every check flips `cur` (an SDRHIP_EINVAL call consumes nothing).
#include "sdrhip_host.h"

#include <cstring>
#include <new>
#include <vector>

using namespace sdrhip;

struct sdrhip_fecbuf {
    sdrhip_ctx *ctx;
    int nstreams;
    int cur = 0;                 // state[cur] is the committed collector state
    FecBufState *state[2] = {nullptr, nullptr};
    uint8_t *carry = nullptr;    // [2][S][128][512] the open slots' first 128 super blocks
    DevBuf small;                // ndg [S], job_off [S + 1], dbase [S], rec_base [S] (int64), counts [S][FB_COUNTS], pub [S][max_frames]
    DevBuf rec, stage, dmap, dec_out, dec_b0;
    DevBuf hin, hout, hb0;       // SDRHIP_MEM_HOST staging on the device
    PinnedBuf pin_up, pin_down, pin_in;
    // ---- asynchronous Tx batches (sdrhip_tx_submit_datagrams): the host's shadow of the classification part of state[cur]
    std::vector<FecBufShadow> shadow;
    bool shadow_ok = false;      // false: refreshed from the device before the next asynchronous batch (creation, reset, a synchronous call)
    int async_busy = 0;          // the owning Tx / Rx handle has asynchronous datagram batches in flight: reset and write_and_read are refused
    DevBuf atab;                 // their tables, counts and public records (fecbuf_packed)
    // ---- the Rx pipe fed datagrams (sdrhip_rx_process_datagrams): samples each stream holds back between calls (fecbuf_join_carry)
    DevBuf join_carry;
    std::vector<size_t> join_carry_host;
};

namespace {
constexpr size_t PAYLOAD = (size_t)127 * SDRHIP_BLOCK_BYTES;

// byte offset of the per-stream counts ([S][FB_COUNTS]) in `small`, behind [ndg S][job_off S + 1][dbase S][pad] ints and rec_base (int64)
size_t counts_offset(int S) { return (((size_t)3 * S + 2 + 3) & ~(size_t)3) * 4 + (size_t)S * 8; }

int fecbuf_init_state(sdrhip_fecbuf *b)
{
    std::vector<FecBufState> st((size_t)b->nstreams);
    for (FecBufState &x : st) {
        memset(&x, 0, sizeof(x));
        x.head = -1; x.maxrow = -1; x.b0 = -1;
        x.min_blocks = 256;
        // MetaDataFEC::init(): zero, m_nbFECBlocks = -1 (byte 11)
        x.cur_meta[2] = x.out_meta[2] = 0xff000000u;
    }
    b->cur = 0;
    b->shadow_ok = false;
    if (b->join_carry.p) { // (the remainder rows go with the collector)
        HIP_TRY(hipMemsetAsync(b->join_carry.p, 0, (size_t)b->nstreams * sizeof(unsigned), b->ctx->stream));
        b->join_carry_host.assign((size_t)b->nstreams, 0);
    }
    HIP_TRY(link_copy(b->ctx, b->state[0], st.data(), st.size() * sizeof(FecBufState), hipMemcpyHostToDevice, b->ctx->stream));
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
    // small per-call arrays: [ndg S][job_off S + 1][dbase S][pad] ints, then rec_base (int64), counts, public records
    const size_t ints = ((size_t)3 * S + 2 + 3) & ~(size_t)3;
    const size_t off_rb = ints * 4, off_cnt = counts_offset(S), off_pub = off_cnt + (size_t)S * FB_COUNTS * 4;
    const size_t small_bytes = off_pub + (size_t)S * max_frames * sizeof(FecBufPub);
    if ((rc = b->small.reserve(small_bytes))) return rc;
    if ((rc = b->pin_up.reserve(off_cnt))) return rc;
    if ((rc = b->pin_down.reserve(small_bytes - off_cnt))) return rc;
    int *up = b->pin_up.as<int>();
    long long *rb = reinterpret_cast<long long *>(b->pin_up.as<uint8_t>() + off_rb);
    long long nrec = 0;
    for (int s = 0; s < S; ++s) {
        up[s] = (int)n_dgrams[s];
        rb[s] = nrec;
        nrec += (long long)n_dgrams[s] + 1;
    }
    if ((rc = b->rec.reserve((size_t)nrec * sizeof(FecBufRec)))) return rc;
    uint8_t *sm = b->small.as<uint8_t>();
    HIP_TRY(link_copy(c, sm, b->pin_up.p, off_cnt, hipMemcpyHostToDevice, c->stream));
    b->pin_up.mark(c->stream);

    FecBufArgs a;
    memset(&a, 0, sizeof(a));
    a.dg = dg; a.dg_stride = dg_stride;
    a.ndg = reinterpret_cast<const int *>(sm);
    a.job_off = reinterpret_cast<const int *>(sm) + S;
    a.dbase = reinterpret_cast<const int *>(sm) + 2 * S + 1;
    a.rec_base = reinterpret_cast<const long long *>(sm + off_rb);
    a.counts = reinterpret_cast<int *>(sm + off_cnt);
    a.pub = reinterpret_cast<FecBufPub *>(sm + off_pub);
    a.rec = b->rec.as<FecBufRec>();
    a.max_frames = (int)max_frames;
    a.st_cur = b->state[b->cur]; a.st_next = b->state[b->cur ^ 1];
    a.carry_cur_base = b->carry; a.carry_base = b->carry;
    a.nstreams = S;
    a.data_out = data_out; a.data_stride = data_stride; a.block0_out = block0_out;
    hipError_t e = launch_fecbuf_classify(a, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf classify launch: %s", hipGetErrorString(e));
    // the one read-back: counts + public records
    HIP_TRY(link_copy(c, b->pin_down.p, sm + off_cnt, small_bytes - off_cnt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int *cnt = b->pin_down.as<int>();
    const FecBufPub *pub = reinterpret_cast<const FecBufPub *>(b->pin_down.as<uint8_t>() + (off_pub - off_cnt));
    bool room = true;
    int njobs = 0, nslots = 0, maxrow = -1, maxrec = 0;
    for (int s = 0; s < S; ++s) {
        const int *x = cnt + (size_t)s * FB_COUNTS;
        n_frames[s] = (size_t)x[FB_K];
        if ((size_t)x[FB_K] > max_frames) room = false;
        up[S + s] = njobs;
        up[2 * S + 1 + s] = nslots;
        njobs += x[FB_K] + 1;
        nslots += x[FB_D];
        if (x[FB_MAXROW] > maxrow) maxrow = x[FB_MAXROW];
        if (x[FB_MAXREC] > maxrec) maxrec = x[FB_MAXREC];
    }
    up[2 * S] = njobs;
    if (!room) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: a stream releases more than max_frames = %zu frames (n_frames has the counts; nothing was consumed)", max_frames);
    if (join && join->admit && (rc = join->admit(join->arg, n_frames))) return rc;
    // everything that can fail for want of memory before the state moves on
    if (nslots > 0) {
        if ((rc = b->stage.reserve((size_t)nslots * 128 * SDRHIP_UDPSIZE))) return rc;
        if ((rc = b->dmap.reserve((size_t)nslots * 2 * sizeof(int)))) return rc;
        if ((rc = b->dec_out.reserve((size_t)nslots * PAYLOAD))) return rc;
        if (block0_out && (rc = b->dec_b0.reserve((size_t)nslots * SDRHIP_BLOCK_BYTES))) return rc;
    }
    for (int s = 0; s < S; ++s) {
        const FecBufPub *p = pub + (size_t)s * max_frames;
        for (size_t k = 0; k < n_frames[s]; ++k) {
            sdrhip_fecbuf_frame &o = info_out[(size_t)s * max_frames + k];
            o.frame_index = p[k].frame_index; o.block_count = p[k].block_count; o.recovery_count = p[k].recovery_count; o.flags = p[k].flags;
        }
    }
    HIP_TRY(link_copy(c, sm + (size_t)S * 4, up + S, ((size_t)2 * S + 1) * 4, hipMemcpyHostToDevice, c->stream));
    b->pin_up.mark(c->stream);
    a.stage = b->stage.as<uint8_t>(); a.dmap = b->dmap.as<int>();
    a.dec_out = b->dec_out.as<uint8_t>(); a.dec_b0 = block0_out ? b->dec_b0.as<uint8_t>() : nullptr;
    e = join ? launch_fecbuf_scatter_rows(a, join->row_off, njobs, c->stream) : launch_fecbuf_scatter(a, njobs, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf scatter launch: %s", hipGetErrorString(e));
    b->cur ^= 1; // (committed: the scatter pass has written the new carry slots)
    if (nslots > 0) {
        // the promise is the batch's highest collected row, never a count: <= 32 rows (indices 0..31) take the one-launch decoder
        const int max_rows = (maxrow < 32 && maxrec <= 32) ? 32 : 128;
        if ((rc = fec_decode_device(c, b->stage.as<uint8_t>(), (size_t)128 * SDRHIP_UDPSIZE, nullptr, (size_t)nslots, b->dec_out.as<uint8_t>(), PAYLOAD,
                                    block0_out ? b->dec_b0.as<uint8_t>() : nullptr, nullptr, nullptr, max_rows)))
            return rc;
        e = join ? launch_fecbuf_copy_rows(a, join->row_off, nslots, c->stream) : launch_fecbuf_copy(a, nslots, c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf copy launch: %s", hipGetErrorString(e));
    }
    return SDRHIP_OK;
}
} // namespace

extern "C" int sdrhip_fecbuf_create(sdrhip_ctx *ctx, int nstreams, sdrhip_fecbuf **out)
{
    if (!ctx || !out || nstreams <= 0 || nstreams > 65535) return fail(SDRHIP_EINVAL, "fecbuf_create: bad argument");
    sdrhip::CtxLock lock_(ctx);
    if (sdrhip_device_count() <= 0) return fail(SDRHIP_EDEVICE, "fecbuf_create: no GPU");
    HIP_TRY(hipSetDevice(ctx->device));
    sdrhip_fecbuf *b = new (std::nothrow) sdrhip_fecbuf();
    if (!b) return fail(SDRHIP_ENOMEM, "out of host memory");
    b->ctx = ctx; b->nstreams = nstreams;
    const size_t sb = (size_t)nstreams * sizeof(FecBufState), cb = (size_t)2 * nstreams * 128 * SDRHIP_UDPSIZE;
    if (hipMalloc(reinterpret_cast<void **>(&b->state[0]), sb) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&b->state[1]), sb) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&b->carry), cb) != hipSuccess) {
        if (b->state[0]) (void)hipFree(b->state[0]);
        if (b->state[1]) (void)hipFree(b->state[1]);
        delete b;
        return fail(SDRHIP_ENOMEM, "hipMalloc fecbuf state");
    }
    ctx_retain(ctx);
    int rc = fecbuf_init_state(b);
    if (rc) { sdrhip_fecbuf_destroy(b); return rc; }
    *out = b;
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
        (void)hipFree(b->state[0]); (void)hipFree(b->state[1]); (void)hipFree(b->carry);
        b->small.release(); b->rec.release(); b->stage.release(); b->dmap.release(); b->dec_out.release(); b->dec_b0.release();
        b->hin.release(); b->hout.release(); b->hb0.release();
        b->pin_up.release(); b->pin_down.release(); b->pin_in.release();
        b->atab.release();
        b->join_carry.release();
    }
    delete b;
    ctx_release(c);
}

extern "C" int sdrhip_fecbuf_reset(sdrhip_fecbuf *b)
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip::CtxLock lock_(b->ctx);
    if (b->async_busy) return fail(SDRHIP_EINVAL, "fecbuf_reset: the owning pipe's asynchronous datagram batches are in flight: collect them first");
    HIP_TRY(hipSetDevice(b->ctx->device));
    return fecbuf_init_state(b);
}

namespace {
// the datagram arguments of a call (sdrhip_fecbuf_write_and_read, sdrhip_tx_process_datagrams); *nmax = the most datagrams of a stream
int check_dgrams(int S, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes, int mem, const char *who, size_t *nmax)
{
    if (int e = check_mem(mem)) return e;
    *nmax = 0;
    for (int s = 0; s < S; ++s) {
        if (n_dgrams[s] > 0x3fffffffu) return fail(SDRHIP_EINVAL, "%s: too many datagrams in one call", who);
        *nmax = n_dgrams[s] > *nmax ? n_dgrams[s] : *nmax;
    }
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
    if (max_frames > 0 && (!data_out || !info_out)) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: NULL data_out / info_out");
    if (max_frames > 0x3fffffffu) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: max_frames too large");
    if (S > 1 && max_frames > 0 && data_stride_bytes < max_frames * PAYLOAD) return fail(SDRHIP_EINVAL, "fecbuf_write_and_read: data_stride_bytes below max_frames x 127 x 508");
    HIP_TRY(hipSetDevice(c->device));
    if (mem == SDRHIP_MEM_DEVICE) {
        if ((nmax > 0 && !aligned16(dgrams)) || (S > 1 && dgram_stride_bytes % 16))
            return fail(SDRHIP_EALIGN, "fecbuf_write_and_read: dgrams / dgram_stride_bytes must be 16-byte aligned");
        if ((reinterpret_cast<uintptr_t>(data_out) & 3u) || (reinterpret_cast<uintptr_t>(block0_out) & 3u) || (S > 1 && data_stride_bytes % 4))
            return fail(SDRHIP_EALIGN, "fecbuf_write_and_read: data_out / block0_out / data_stride_bytes must be 4-byte aligned");
        return fecbuf_device(b, dgrams, n_dgrams, dgram_stride_bytes, data_out, data_stride_bytes, block0_out, max_frames, info_out, n_frames);
    }
    // host memory: the datagrams go up as one 2-D copy (from sdrhip_host_alloc memory in place, else through a pinned buffer)
    const size_t row = nmax * SDRHIP_UDPSIZE, drow = max_frames * PAYLOAD;
    if (drow && (rc = b->hout.reserve((size_t)S * drow + 4))) return rc;
    if (block0_out && max_frames && (rc = b->hb0.reserve((size_t)S * max_frames * SDRHIP_BLOCK_BYTES))) return rc;
    if ((rc = upload_dgrams(b, dgrams, n_dgrams, dgram_stride_bytes, row))) return rc;
    if ((rc = fecbuf_device(b, b->hin.as<uint8_t>(), n_dgrams, row, b->hout.as<uint8_t>(), drow, block0_out ? b->hb0.as<uint8_t>() : nullptr,
                            max_frames, info_out, n_frames)))
        return rc;
    for (int s = 0; s < S; ++s) {
        if (!n_frames[s]) continue;
        HIP_TRY(link_copy(c, data_out + (size_t)s * data_stride_bytes, b->hout.as<uint8_t>() + (size_t)s * drow,
                          n_frames[s] * PAYLOAD, hipMemcpyDeviceToHost, c->stream));
        if (block0_out)
            HIP_TRY(link_copy(c, block0_out + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES, b->hb0.as<uint8_t>() + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES,
                              n_frames[s] * SDRHIP_BLOCK_BYTES, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

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
                   const int **counts, const FecBufJoin *join)
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
        if ((rc = upload_dgrams(b, dgrams, n_dgrams, dgram_stride_bytes, row, join != nullptr))) return rc;
        rc = fecbuf_device(b, b->hin.as<uint8_t>(), n_dgrams, row, data_out, data_stride_bytes, block0_out ? b->hb0.as<uint8_t>() : nullptr,
                           max_frames, info_out, n_frames, join);
        if (!rc && block0_out)
            for (int s = 0; s < S; ++s)
                if (n_frames[s])
                    HIP_TRY(link_copy(c, block0_out + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES, b->hb0.as<uint8_t>() + (size_t)s * max_frames * SDRHIP_BLOCK_BYTES,
                                      n_frames[s] * SDRHIP_BLOCK_BYTES, hipMemcpyDeviceToHost, c->stream));
    }
    if (rc) return rc;
    *counts = reinterpret_cast<const int *>(b->small.as<uint8_t>() + counts_offset(S));
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
        HIP_TRY(hipMemcpyAsync(st.data(), b->state[b->cur], st.size() * sizeof(FecBufState), hipMemcpyDeviceToHost, b->ctx->stream));
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

void fecbuf_shadow_run(FecBufShadow &h, const uint8_t *dg, size_t n, int res[4])
{
    int K = 0, D = 0, maxrow = -1, maxrec = 0;
    for (size_t i = 0; i < n; ++i) {
        uint32_t hd;
        memcpy(&hd, dg + i * SDRHIP_UDPSIZE, 4);
        const int fi = (int)(hd & 0xffffu), bi = (int)((hd >> 16) & 0xffu);
        if (fi != h.head) { // another frame index releases the open slot (the first datagram: the initial one)
            ++K;
            if (h.count >= 128 && h.recov > 0 && !h.dup) { // (to the decoder: the frames cm256_decode repairs)
                ++D;
                maxrow = h.maxrow > maxrow ? h.maxrow : maxrow;
                maxrec = h.recov > maxrec ? h.recov : maxrec;
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
    res[0] = K; res[1] = D; res[2] = maxrow; res[3] = maxrec;
}

int fecbuf_packed(sdrhip_fecbuf *b, const uint8_t *dg, const size_t *n_dgrams, const int *res, const std::vector<FecBufShadow> &next,
                  PinnedBuf &tab, uint8_t *data_out, size_t data_stride, uint8_t *block0_out, size_t max_frames, unsigned *mismatch,
                  bool *committed, const int **counts, const FecBufPub **pub, const FecBufJoin *join)
{
    sdrhip_ctx *c = b->ctx;
    const int S = b->nstreams;
    int rc;
    *committed = false;
    // tables: [ndg S][job_off S + 1][dbase S][expect S x 4][pad] ints, rec_base [S], dg_off [S] (int64); on the device the counts
    // [S][FB_COUNTS] and the public records [S][max_frames] follow
    const size_t ints = ((size_t)7 * S + 1 + 3) & ~(size_t)3;
    const size_t off_rb = ints * 4, off_do = off_rb + (size_t)S * 8, off_cnt = off_do + (size_t)S * 8;
    const size_t off_pub = off_cnt + (size_t)S * FB_COUNTS * 4, bytes = off_pub + (size_t)S * max_frames * sizeof(FecBufPub);
    if ((rc = tab.reserve(off_cnt))) return rc; // (waits for the upload of this batch slot's last use)
    int *ndg = tab.as<int>(), *job_off = ndg + S, *dbase = job_off + S + 1, *expect = dbase + S;
    long long *rb = reinterpret_cast<long long *>(tab.as<uint8_t>() + off_rb), *doff = reinterpret_cast<long long *>(tab.as<uint8_t>() + off_do);
    long long nrec = 0, off = 0;
    int njobs = 0, nslots = 0, maxrow = -1, maxrec = 0;
    for (int s = 0; s < S; ++s) {
        const int *x = res + 4 * s;
        ndg[s] = (int)n_dgrams[s];
        rb[s] = nrec; nrec += (long long)n_dgrams[s] + 1;
        doff[s] = off; off += (long long)(n_dgrams[s] * SDRHIP_UDPSIZE);
        job_off[s] = njobs; njobs += x[0] + 1;
        dbase[s] = nslots; nslots += x[1];
        for (int q = 0; q < 4; ++q) expect[4 * s + q] = x[q];
        maxrow = x[2] > maxrow ? x[2] : maxrow;
        maxrec = x[3] > maxrec ? x[3] : maxrec;
    }
    job_off[S] = njobs;
    // everything that can fail for want of memory before the state moves on (a buffer that grows waits for the batches in flight)
    if ((rc = reserve_settled(c, b->atab, bytes))) return rc;
    if ((rc = reserve_settled(c, b->rec, (size_t)nrec * sizeof(FecBufRec)))) return rc;
    if (nslots > 0) {
        if ((rc = reserve_settled(c, b->stage, (size_t)nslots * 128 * SDRHIP_UDPSIZE))) return rc;
        if ((rc = reserve_settled(c, b->dmap, (size_t)nslots * 2 * sizeof(int)))) return rc;
        if ((rc = reserve_settled(c, b->dec_out, (size_t)nslots * PAYLOAD))) return rc;
        if (block0_out && (rc = reserve_settled(c, b->dec_b0, (size_t)nslots * SDRHIP_BLOCK_BYTES))) return rc;
    }
    uint8_t *t = b->atab.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(t, tab.p, off_cnt, hipMemcpyHostToDevice, c->stream)); // (not counted: a table)
    tab.mark(c->stream);
    FecBufArgs a;
    memset(&a, 0, sizeof(a));
    a.dg = dg; a.dg_stride = 0;
    a.ndg = reinterpret_cast<const int *>(t);
    a.job_off = a.ndg + S;
    a.dbase = a.job_off + S + 1;
    a.rec_base = reinterpret_cast<const long long *>(t + off_rb);
    a.counts = reinterpret_cast<int *>(t + off_cnt);
    a.pub = reinterpret_cast<FecBufPub *>(t + off_pub);
    a.rec = b->rec.as<FecBufRec>();
    a.max_frames = (int)max_frames;
    a.st_cur = b->state[b->cur]; a.st_next = b->state[b->cur ^ 1];
    a.carry_cur_base = b->carry; a.carry_base = b->carry;
    a.nstreams = S;
    a.data_out = data_out; a.data_stride = data_stride; a.block0_out = block0_out;
    a.stage = nslots ? b->stage.as<uint8_t>() : nullptr; a.dmap = nslots ? b->dmap.as<int>() : nullptr;
    a.dec_out = nslots ? b->dec_out.as<uint8_t>() : nullptr; a.dec_b0 = nslots && block0_out ? b->dec_b0.as<uint8_t>() : nullptr;
    const long long *dg_off = reinterpret_cast<const long long *>(t + off_do);
    hipError_t e = launch_fecbuf_classify_packed(a, dg_off, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf classify launch: %s", hipGetErrorString(e));
    if ((e = launch_fecbuf_shadow_check(a.counts, reinterpret_cast<const int *>(t) + 3 * S + 1, S, mismatch, c->stream)) != hipSuccess)
        return fail(SDRHIP_EDEVICE, "fecbuf shadow check launch: %s", hipGetErrorString(e));
    if (nslots > 0) HIP_TRY(hipMemsetAsync(a.dmap, 0xff, (size_t)nslots * 2 * sizeof(int), c->stream)); // (the guarded copy skips what stays -1)
    e = join ? launch_fecbuf_scatter_packed_rows(a, dg_off, join->row_off, njobs, nslots, c->stream)
             : launch_fecbuf_scatter_packed(a, dg_off, njobs, nslots, c->stream);
    if (e != hipSuccess)
        return fail(SDRHIP_EDEVICE, "fecbuf scatter launch: %s", hipGetErrorString(e));
    b->cur ^= 1; // (committed: the scatter pass has written the new carry slots)
    b->shadow = next;
    *committed = true;
    if (nslots > 0) {
        // the promise is the batch's highest collected row, never a count (as fecbuf_device)
        const int max_rows = (maxrow < 32 && maxrec <= 32) ? 32 : 128;
        if ((rc = fec_decode_device(c, b->stage.as<uint8_t>(), (size_t)128 * SDRHIP_UDPSIZE, nullptr, (size_t)nslots, b->dec_out.as<uint8_t>(), PAYLOAD,
                                    block0_out ? b->dec_b0.as<uint8_t>() : nullptr, nullptr, nullptr, max_rows)))
            return rc;
        e = join ? launch_fecbuf_copy_guarded_rows(a, join->row_off, nslots, c->stream) : launch_fecbuf_copy_guarded(a, nslots, c->stream);
        if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "fecbuf copy launch: %s", hipGetErrorString(e));
    }
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

const FecBufState *fecbuf_committed_state(const sdrhip_fecbuf *b) { return b->state[b->cur]; }
} // namespace sdrhip

extern "C" int sdrhip_fecbuf_stats(sdrhip_fecbuf *b, int stream, int *cur_nb_blocks, int *cur_nb_recovery, int *min_nb_blocks, int *max_nb_recovery,
                                   uint8_t current_meta[24], uint8_t output_meta[24])
{
    if (!b) return fail(SDRHIP_EINVAL, "fecbuf is NULL");
    sdrhip::CtxLock lock_(b->ctx);
    if (stream < 0 || stream >= b->nstreams) return fail(SDRHIP_EINVAL, "fecbuf_stats: stream out of range");
    HIP_TRY(hipSetDevice(b->ctx->device));
    FecBufState x;
    FecBufState *d = b->state[b->cur] + stream;
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
