// sdrhip_stream_state.cpp -- per-stream lifecycle of include/sdrhip.h: what the reset entries of the banks and the pipes share
// (the mask's way up, KR's launch) and the pipes' own entries.  One stream of the reference is one sdrdaemonrx / sdrdaemontx
// process; restarting it gives that stream constructor state and disturbs no other.  Here: one small launch on the context's
// stream behind everything submitted so far, host bookkeeping for the streams named, no synchronisation and no read-back.
#include "sdrhip_pipes.h"

using namespace sdrhip;

namespace sdrhip {
int stream_mask_upload(sdrhip_ctx *c, StreamMask &m, const uint8_t *mask, int S, const uint8_t **dev, int *n_set)
{
    *dev = nullptr;
    int n = S;
    if (mask) {
        n = 0;
        for (int s = 0; s < S; ++s) n += mask[s] ? 1 : 0;
    }
    *n_set = n;
    if (n == 0 || n == S) return SDRHIP_OK;
    const void *tab = nullptr;
    if (int rc = m.upload(c->stream, mask, (size_t)S, &tab)) return rc;
    *dev = static_cast<const uint8_t *>(tab);
    return SDRHIP_OK;
}

int stream_reset_launch(sdrhip_ctx *c, const StreamResetArgs &a)
{
    const hipError_t e = launch_stream_reset(a, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "stream reset launch: %s", hipGetErrorString(e));
    return SDRHIP_OK;
}
} // namespace sdrhip

// UDPSinkFEC's and Downsampler's constructors for the streams named (UDPSinkFEC.cpp:28-60: m_frameCount 0, no open frame;
// Decimators.h:56-70), and SDRdaemonFECBuffer's where the handle collects datagrams
extern "C" int sdrhip_rx_reset_streams(sdrhip_rx *rx, const uint8_t *mask)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (rx->ring.any([](const sdrhip_rx::Batch &b) { return b.state == 1; }))
        return fail(SDRHIP_EINVAL, "rx_reset_streams: an asynchronous batch is being filled: collect it first");
    if (rx->late.have) return fail(SDRHIP_EINVAL, "rx_reset_streams: frames of the previous call wait for delivery (pipelined mode): sdrhip_rx_flush them first");
    return stream_reset_bank(
        rx->ctx, rx->reset_mask, mask, rx->nstreams,
        [rx](StreamResetArgs *a) {
            decimators_reset_part(rx->dec, a);
            if (rx->fb) fecbuf_reset_part(rx->fb, a);
        },
        [rx](const uint8_t *m) {
            decimators_reset_done(rx->dec, m == nullptr);
            if (rx->fb) fecbuf_reset_done(rx->fb, m);
            // the open frame is dropped where it lies (its slot keeps the stale bytes: the next frame the stream opens writes every
            // block).  When every stream was reset no frame is open anywhere, so every window goes back to slot 0 as well: the
            // streams stand at the same position again (aligned) whatever ragged steps moved their windows apart before, and the
            // uniform step, pipelined mode and uniform batches are available as on a fresh handle.  (Launches in flight that read
            // the old windows are ahead of the next call's on the context's stream.)
            rx->area.reset(m);
        });
}

extern "C" int sdrhip_tx_reset_streams(sdrhip_tx *tx, const uint8_t *mask)
{
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (tx->late.have) return fail(SDRHIP_EINVAL, "tx_reset_streams: a pipelined batch waits: sdrhip_tx_flush it first");
    return stream_reset_bank(
        tx->ctx, tx->reset_mask, mask, tx->nstreams,
        [tx](StreamResetArgs *a) {
            interpolators_reset_part(tx->itp, a);
            if (tx->fb) fecbuf_reset_part(tx->fb, a);
        },
        [tx](const uint8_t *m) {
            if (tx->fb) fecbuf_reset_done(tx->fb, m);
        });
}

// --------------------------------------------------------------------------- export / import of one stream
// The blob (host memory, opaque to the caller): a 16-byte header {magic, version, kind, total bytes}, the host's part of the
// stream's state, then the device's part exactly as KG packs it -- fixed offsets and a fixed size per kind, whatever the
// configuration.  A piece the stream does not have (no open frame, no collector, nothing held back) is zero filled.
namespace {
constexpr uint32_t BLOB_MAGIC = 0x53524453u; // "SDRS"
constexpr uint32_t BLOB_VERSION = 1, BLOB_RX = 1, BLOB_TX = 2;
struct BlobHead { uint32_t magic, version, kind, bytes; };
struct RxBlobHost {
    uint32_t hb_variant, stage0_int16; // the half-band variant the histories belong to; m_decimator2's history fits int16
    uint32_t r_open, r_count;          // the open frame has its meta block; its m_frameCount
    uint64_t r_pending;                // decimated samples in the open frame
    uint32_t has_collector, carry;     // the collector part below is meaningful; samples held back in front of the decimator
};
struct TxBlobHost { uint32_t has_collector, pad[3]; };
constexpr size_t SLOT_BYTES = (size_t)SDRHIP_NB_ORIGINAL * SDRHIP_UDPSIZE; // the 128 original super blocks of a frame / a carry buffer
constexpr size_t HELD_BYTES = 64 * 4;                                       // at most 63 samples held back
constexpr size_t RX_ROW = 0, RX_FRAME = RX_ROW + DEC_STATE_WORDS * 4, RX_ST = RX_FRAME + SLOT_BYTES, RX_CARRY = RX_ST + sizeof(FecBufState),
                 RX_HELD = RX_CARRY + SLOT_BYTES, RX_DEV_BYTES = RX_HELD + HELD_BYTES;
constexpr size_t TX_ROW = 0, TX_ST = TX_ROW + INT_STATE_WORDS * 4, TX_CARRY = TX_ST + sizeof(FecBufState), TX_DEV_BYTES = TX_CARRY + SLOT_BYTES;
constexpr size_t RX_HOST_BYTES = sizeof(BlobHead) + sizeof(RxBlobHost), TX_HOST_BYTES = sizeof(BlobHead) + sizeof(TxBlobHost);
constexpr size_t RX_BLOB_BYTES = RX_HOST_BYTES + RX_DEV_BYTES, TX_BLOB_BYTES = TX_HOST_BYTES + TX_DEV_BYTES;
static_assert(sizeof(BlobHead) == 16 && sizeof(RxBlobHost) == 32 && sizeof(TxBlobHost) == 16, "blob layout");
static_assert(sizeof(FecBufState) % 16 == 0 && RX_DEV_BYTES % 16 == 0 && TX_DEV_BYTES % 16 == 0, "KG / KS move 16-byte pieces");

void add_seg(StreamCopyArgs *a, const void *src, void *dst, size_t bytes)
{
    StreamCopySeg &g = a->seg[a->nseg++];
    g.src = static_cast<const uint8_t *>(src); g.dst = static_cast<uint8_t *>(dst); g.bytes = (uint32_t)bytes; g.wg0 = 0;
}

int check_head(const void *blob, size_t bytes, uint32_t kind, size_t want, const char *who)
{
    if (!blob) return fail(SDRHIP_EINVAL, "%s: NULL blob", who);
    if (bytes != want) return fail(SDRHIP_EINVAL, "%s: the blob has %zu bytes, a stream's state has %zu", who, bytes, want);
    BlobHead h;
    memcpy(&h, blob, sizeof(h));
    if (h.magic != BLOB_MAGIC || h.version != BLOB_VERSION || h.kind != kind || h.bytes != want)
        return fail(SDRHIP_EINVAL, "%s: not a stream blob of this kind and version (magic %08x, version %u, kind %u, %u bytes)", who, h.magic, h.version,
                    h.kind, h.bytes);
    return SDRHIP_OK;
}

// a collector state as the classify pass can have left it: the kernels index the carry buffers and their ranks with these fields
int check_state(const FecBufState &st, const char *who)
{
    if (st.cbuf < 0 || st.cbuf > 1 || st.count < 0 || st.recov < 0 || st.recov > 128 || st.maxrow < -1 || st.maxrow > 127 || st.b0 < -1 || st.b0 > 127 ||
        (st.b0 >= st.count && st.b0 >= 0) || st.head < -1 || st.head > 0xffff)
        return fail(SDRHIP_EINVAL, "%s: the blob's collector state is not one a collector can be in", who);
    return SDRHIP_OK;
}

// the export's tail: KG into `dev`, ONE copy of the packed bytes to the host, ONE synchronisation
int export_run(sdrhip_ctx *c, StreamCopyArgs &a, DevBuf &dev, size_t dev_bytes, void *host)
{
    const uint32_t grid = stream_copy_plan(&a);
    const hipError_t e = launch_stream_gather(a, grid, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "stream gather launch: %s", hipGetErrorString(e));
    HIP_TRY(link_copy(c, host, dev.p, dev_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDRHIP_OK;
}

// What the open slot has not filled of its carry buffer (ranks from min(count, 128) on) and what lies behind the held-back samples is
// whatever earlier frames left there: zero in the blob, like every piece the stream does not have -- a reset stream's blob is a
// never-used stream's, byte for byte.  `part`: the blob's device part, already on the host
void blank_unused_carry(uint8_t *part, size_t off_st, size_t off_carry)
{
    FecBufState st;
    memcpy(&st, part + off_st, sizeof(st));
    const size_t n = st.count < 0 ? 0 : st.count > SDRHIP_NB_ORIGINAL ? (size_t)SDRHIP_NB_ORIGINAL : (size_t)st.count;
    memset(part + off_carry + n * SDRHIP_UDPSIZE, 0, ((size_t)SDRHIP_NB_ORIGINAL - n) * SDRHIP_UDPSIZE);
}

// the collector's pieces of a gather: the committed state, the carry buffer it names (picked on the device)
void gather_collector(sdrhip_fecbuf *fb, int s, uint8_t *dev, size_t off_st, size_t off_carry, StreamCopyArgs *a)
{
    FecBufStreamRef r;
    fecbuf_stream_ref(fb, s, &r);
    add_seg(a, r.st[0], dev + off_st, sizeof(FecBufState));
    a->carry_seg = a->nseg; a->cbuf_from = r.st[0]; a->carry_half = r.carry_half;
    add_seg(a, r.carry, dev + off_carry, SLOT_BYTES);
}
// ... of a scatter: the state into both halves, the carry buffer the state names (the host reads it in the blob)
void scatter_collector(sdrhip_fecbuf *fb, int s, const uint8_t *dev, size_t off_st, size_t off_carry, const FecBufState &st, bool carry, StreamCopyArgs *a)
{
    FecBufStreamRef r;
    fecbuf_stream_ref(fb, s, &r);
    add_seg(a, dev + off_st, r.st[0], sizeof(FecBufState));
    add_seg(a, dev + off_st, r.st[1], sizeof(FecBufState));
    if (carry) add_seg(a, dev + off_carry, r.carry + (st.cbuf ? r.carry_half : 0), SLOT_BYTES);
}

// the import's tail: the device part up from the pinned staging (filled by the caller), then KS
int import_run(sdrhip_ctx *c, StreamCopyArgs &a, PinnedBuf &pin, DevBuf &dev, size_t dev_bytes)
{
    HIP_TRY(link_copy(c, dev.p, pin.p, dev_bytes, hipMemcpyHostToDevice, c->stream));
    pin.mark(c->stream);
    const uint32_t grid = stream_copy_plan(&a);
    const hipError_t e = launch_stream_scatter(a, grid, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "stream scatter launch: %s", hipGetErrorString(e));
    return SDRHIP_OK;
}

int rx_movable(const sdrhip_rx *rx, int stream, const char *who)
{
    if (stream < 0 || stream >= rx->nstreams) return fail(SDRHIP_EINVAL, "%s: stream %d of %d", who, stream, rx->nstreams);
    if (rx_batches_active(rx)) return fail(SDRHIP_EINVAL, "%s: asynchronous batches are being filled or in flight: collect them first", who);
    if (rx->late.have) return fail(SDRHIP_EINVAL, "%s: frames of the previous call wait for delivery (pipelined mode): sdrhip_rx_flush them first", who);
    return SDRHIP_OK;
}
int tx_movable(const sdrhip_tx *tx, int stream, const char *who)
{
    if (stream < 0 || stream >= tx->nstreams) return fail(SDRHIP_EINVAL, "%s: stream %d of %d", who, stream, tx->nstreams);
    if (tx->ring.busy()) return fail(SDRHIP_EINVAL, "%s: asynchronous batches are in flight: collect them first", who);
    if (tx->late.have) return fail(SDRHIP_EINVAL, "%s: a pipelined batch waits: sdrhip_tx_flush it first", who);
    return SDRHIP_OK;
}
} // namespace

extern "C" size_t sdrhip_rx_stream_state_bytes(const sdrhip_rx *rx) { return rx ? RX_BLOB_BYTES : 0; }
extern "C" size_t sdrhip_tx_stream_state_bytes(const sdrhip_tx *tx) { return tx ? TX_BLOB_BYTES : 0; }

extern "C" int sdrhip_rx_export_stream(sdrhip_rx *rx, int stream, void *blob, size_t bytes)
{
    const char *who = "rx_export_stream";
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (!blob || bytes != RX_BLOB_BYTES) return fail(SDRHIP_EINVAL, "%s: the blob must have sdrhip_rx_stream_state_bytes() = %zu bytes", who, RX_BLOB_BYTES);
    if (int rc = rx_movable(rx, stream, who)) return rc;
    sdrhip_ctx *c = rx->ctx;
    const size_t s = (size_t)stream;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = reserve_settled(c, rx->x_blob, RX_DEV_BYTES))) return rc;
    uint8_t *dev = rx->x_blob.as<uint8_t>();
    RxBlobHost h;
    memset(&h, 0, sizeof(h));
    h.hb_variant = (uint32_t)rx->cfg.hb_variant; h.stage0_int16 = decimators_stage0_int16(rx->dec) ? 1 : 0;
    h.r_open = rx->area.open(s); h.r_count = rx->area.count(s); h.r_pending = rx->area.pending(s);
    HIP_TRY(hipMemsetAsync(dev, 0, RX_DEV_BYTES, c->stream)); // (the pieces the stream does not have)
    StreamCopyArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_seg = -1;
    add_seg(&a, decimators_row(rx->dec, stream, 0), dev + RX_ROW, DEC_STATE_WORDS * 4);
    if (h.r_open) {
        add_seg(&a, rx->work.as<uint8_t>() + rx->area.index(s) * rx_frame_bytes(rx), dev + RX_FRAME, SLOT_BYTES);
    }
    if (rx->fb) {
        unsigned *carry_dev = nullptr;
        std::vector<size_t> *carry = nullptr;
        if ((rc = fecbuf_join_carry(rx->fb, &carry_dev, &carry))) return rc;
        h.has_collector = 1; h.carry = (uint32_t)(*carry)[s];
        gather_collector(rx->fb, stream, dev, RX_ST, RX_CARRY, &a);
        if (h.carry && rx->j_rows.p) add_seg(&a, rx->j_rows.as<uint8_t>() + s * rx->j_row_len * 4, dev + RX_HELD, HELD_BYTES);
    }
    uint8_t *out = static_cast<uint8_t *>(blob);
    if ((rc = export_run(c, a, rx->x_blob, RX_DEV_BYTES, out + RX_HOST_BYTES))) return rc;
    if (h.has_collector) {
        blank_unused_carry(out + RX_HOST_BYTES, RX_ST, RX_CARRY);
        const size_t held = h.carry > 63 ? HELD_BYTES : (size_t)h.carry * 4;
        memset(out + RX_HOST_BYTES + RX_HELD + held, 0, HELD_BYTES - held);
    }
    const BlobHead head = {BLOB_MAGIC, BLOB_VERSION, BLOB_RX, (uint32_t)RX_BLOB_BYTES};
    memcpy(out, &head, sizeof(head));
    memcpy(out + sizeof(head), &h, sizeof(h));
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_import_stream(sdrhip_rx *rx, int stream, const void *blob, size_t bytes)
{
    const char *who = "rx_import_stream";
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    int rc;
    if ((rc = check_head(blob, bytes, BLOB_RX, RX_BLOB_BYTES, who))) return rc;
    if ((rc = rx_movable(rx, stream, who))) return rc;
    const uint8_t *in = static_cast<const uint8_t *>(blob);
    RxBlobHost h;
    FecBufState st;
    memcpy(&h, in + sizeof(BlobHead), sizeof(h));
    memcpy(&st, in + RX_HOST_BYTES + RX_ST, sizeof(st));
    if ((int)h.hb_variant != rx->cfg.hb_variant) return fail(SDRHIP_EINVAL, "%s: the blob's histories belong to hb_variant %u, the bank runs %d", who, h.hb_variant, rx->cfg.hb_variant);
    if (!RxFrameArea::importable(h.r_pending, h.r_open, h.r_count) || h.carry > 63 || h.has_collector > 1 ||
        (!h.has_collector && h.carry))
        return fail(SDRHIP_EINVAL, "%s: the blob's framing state is not one a stream can be in", who);
    if (h.has_collector && (rc = check_state(st, who))) return rc;
    sdrhip_ctx *c = rx->ctx;
    const size_t s = (size_t)stream;
    HIP_TRY(hipSetDevice(c->device));
    // ---- everything that allocates comes first: the collector (the blob has one, the bank not yet), the rows, a frame area
    if (h.has_collector && (rc = rx_collector(rx))) return rc;
    unsigned *carry_dev = nullptr;
    std::vector<size_t> *carry = nullptr;
    if (rx->fb && (rc = fecbuf_join_carry(rx->fb, &carry_dev, &carry))) return rc;
    if (h.carry && (rc = rx_join_rows(rx, 0, who))) return rc;
    if (h.r_open && (rc = rx_area_room(rx, nullptr))) return rc;
    if ((rc = reserve_settled(c, rx->x_blob, RX_DEV_BYTES))) return rc;
    PinnedBuf &pin = rx->x_pin.next();
    if ((rc = pin.reserve(RX_DEV_BYTES))) return rc;
    memcpy(pin.p, in + RX_HOST_BYTES, RX_DEV_BYTES);
    if (!h.has_collector) { // (the source had no collector: the bank's own begins as the constructor leaves it)
        fecbuf_fresh_state(&st);
        memcpy(pin.as<uint8_t>() + RX_ST, &st, sizeof(st));
    }
    const uint8_t *dev = rx->x_blob.as<uint8_t>();
    StreamCopyArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_seg = -1;
    add_seg(&a, dev + RX_ROW, decimators_row(rx->dec, stream, 0), DEC_STATE_WORDS * 4);
    add_seg(&a, dev + RX_ROW, decimators_row(rx->dec, stream, 1), DEC_STATE_WORDS * 4);
    if (h.r_open) { // (its 128 original blocks, the meta block it was opened with among them; encoded with the fecblk in force when it completes)
        add_seg(&a, dev + RX_FRAME, rx->work.as<uint8_t>() + rx->area.index(s) * rx_frame_bytes(rx), SLOT_BYTES);
    }
    if (rx->fb) {
        scatter_collector(rx->fb, stream, dev, RX_ST, RX_CARRY, st, h.has_collector != 0, &a);
        if (h.carry) add_seg(&a, dev + RX_HELD, rx->j_rows.as<uint8_t>() + s * rx->j_row_len * 4, HELD_BYTES);
        a.word_dst = carry_dev + s; a.word_val = h.carry;
    }
    if ((rc = import_run(c, a, pin, rx->x_blob, RX_DEV_BYTES))) return rc;
    rx->area.import_stream(s, h.r_pending, h.r_open, h.r_count);
    if (!h.stage0_int16) decimators_clear_stage0_int16(rx->dec);
    if (rx->fb) fecbuf_import_host(rx->fb, stream, st, h.carry);
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_export_stream(sdrhip_tx *tx, int stream, void *blob, size_t bytes)
{
    const char *who = "tx_export_stream";
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    if (!blob || bytes != TX_BLOB_BYTES) return fail(SDRHIP_EINVAL, "%s: the blob must have sdrhip_tx_stream_state_bytes() = %zu bytes", who, TX_BLOB_BYTES);
    if (int rc = tx_movable(tx, stream, who)) return rc;
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = reserve_settled(c, tx->x_blob, TX_DEV_BYTES))) return rc;
    uint8_t *dev = tx->x_blob.as<uint8_t>();
    TxBlobHost h;
    memset(&h, 0, sizeof(h));
    HIP_TRY(hipMemsetAsync(dev, 0, TX_DEV_BYTES, c->stream));
    StreamCopyArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_seg = -1;
    add_seg(&a, interpolators_row(tx->itp, stream, 0), dev + TX_ROW, INT_STATE_WORDS * 4);
    if (tx->fb) {
        h.has_collector = 1;
        gather_collector(tx->fb, stream, dev, TX_ST, TX_CARRY, &a);
    }
    uint8_t *out = static_cast<uint8_t *>(blob);
    if ((rc = export_run(c, a, tx->x_blob, TX_DEV_BYTES, out + TX_HOST_BYTES))) return rc;
    if (h.has_collector) blank_unused_carry(out + TX_HOST_BYTES, TX_ST, TX_CARRY);
    const BlobHead head = {BLOB_MAGIC, BLOB_VERSION, BLOB_TX, (uint32_t)TX_BLOB_BYTES};
    memcpy(out, &head, sizeof(head));
    memcpy(out + sizeof(head), &h, sizeof(h));
    return SDRHIP_OK;
}

extern "C" int sdrhip_tx_import_stream(sdrhip_tx *tx, int stream, const void *blob, size_t bytes)
{
    const char *who = "tx_import_stream";
    if (!tx) return fail(SDRHIP_EINVAL, "tx is NULL");
    sdrhip::CtxLock lock_(tx->ctx);
    int rc;
    if ((rc = check_head(blob, bytes, BLOB_TX, TX_BLOB_BYTES, who))) return rc;
    if ((rc = tx_movable(tx, stream, who))) return rc;
    const uint8_t *in = static_cast<const uint8_t *>(blob);
    TxBlobHost h;
    FecBufState st;
    memcpy(&h, in + sizeof(BlobHead), sizeof(h));
    memcpy(&st, in + TX_HOST_BYTES + TX_ST, sizeof(st));
    if (h.has_collector > 1) return fail(SDRHIP_EINVAL, "%s: the blob's state is not one a stream can be in", who);
    if (h.has_collector && (rc = check_state(st, who))) return rc;
    sdrhip_ctx *c = tx->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (h.has_collector && (rc = tx_collector(tx))) return rc;
    if ((rc = reserve_settled(c, tx->x_blob, TX_DEV_BYTES))) return rc;
    PinnedBuf &pin = tx->x_pin.next();
    if ((rc = pin.reserve(TX_DEV_BYTES))) return rc;
    memcpy(pin.p, in + TX_HOST_BYTES, TX_DEV_BYTES);
    if (!h.has_collector) {
        fecbuf_fresh_state(&st);
        memcpy(pin.as<uint8_t>() + TX_ST, &st, sizeof(st));
    }
    const uint8_t *dev = tx->x_blob.as<uint8_t>();
    StreamCopyArgs a;
    memset(&a, 0, sizeof(a));
    a.carry_seg = -1;
    add_seg(&a, dev + TX_ROW, interpolators_row(tx->itp, stream, 0), INT_STATE_WORDS * 4);
    add_seg(&a, dev + TX_ROW, interpolators_row(tx->itp, stream, 1), INT_STATE_WORDS * 4);
    if (tx->fb) scatter_collector(tx->fb, stream, dev, TX_ST, TX_CARRY, st, h.has_collector != 0, &a);
    if ((rc = import_run(c, a, pin, tx->x_blob, TX_DEV_BYTES))) return rc;
    if (tx->fb) fecbuf_import_host(tx->fb, stream, st, 0);
    return SDRHIP_OK;
}
