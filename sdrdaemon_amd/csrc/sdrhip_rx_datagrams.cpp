// sdrhip_rx_datagrams.cpp -- the Rx pipe fed raw FEC datagrams (sdrhip_rx_process_datagrams): sdrdaemontx's receive half chained
// to sdrdaemonrx's send half for every stream.  UDPSourceFEC::read -> SDRdaemonFECBuffer::writeAndRead (sdrdaemontx.cpp:449-498)
// collects and repairs what an undecimated radio head sent; the released payloads go behind the samples the stream held back,
// the largest multiple of the decimation unit goes through Downsampler::process -> UDPSinkFEC::write (sdrdaemonrx.cpp:619-644)
// as ONE ragged step (rx_ragged), and KJ (rx_join_kernels.hip) moves every stream's new remainder to the head of its row.  The
// samples between collector and decimator stay on the device.
#include "sdrhip_pipes.h"

using namespace sdrhip;

namespace {
// asked with the call's release counts while the collector has not moved: what each stream feeds its decimator and holds back
// (join), what the ragged step will make of it (n) -- and whether it would refuse the delivery.  The call goes on with both
struct Admit {
    const sdrhip_rx *rx;
    const std::vector<size_t> *carry;
    const uint8_t *frames_out;
    size_t frame_stride_bytes;
    int mem;
    RxJoinCounts join;
    RxRaggedCounts n;
};
int admit(void *arg, const size_t *n_released)
{
    Admit &a = *static_cast<Admit *>(arg);
    a.join = rx_join_counts(rx_join_unit(a.rx->cfg), *a.carry, n_released);
    a.n = rx_counts(a.rx, a.join.fed.data());
    return rx_refuse_delivery("rx_process_datagrams", a.n, a.frames_out, a.frame_stride_bytes, a.mem, true);
}
} // namespace

int sdrhip::rx_collector(sdrhip_rx *rx)
{
    return rx->fb ? SDRHIP_OK : sdrhip_fecbuf_create(rx->ctx, rx->nstreams, &rx->fb);
}

int sdrhip::rx_join_rows(sdrhip_rx *rx, size_t max_released, const char *who)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    const size_t row_len = (63 + max_released * SDRHIP_SAMPLES_PER_FRAME + 3) & ~(size_t)3;
    if (row_len <= rx->j_row_len) return SDRHIP_OK;
    DevBuf bigger;
    int rc;
    if ((rc = bigger.reserve((size_t)S * row_len * 4))) return rc;
    hipError_t e = hipSuccess;
    if (rx->j_rows.p)
        e = hipMemcpy2DAsync(bigger.p, row_len * 4, rx->j_rows.p, rx->j_row_len * 4, 64 * 4, (size_t)S, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (earlier launches may still use the old rows)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return fail(SDRHIP_EDEVICE, "%s: moving the rows: %s", who, hipGetErrorString(e));
    }
    rx->j_rows = std::move(bigger);
    rx->j_row_len = row_len;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_collector(sdrhip_rx *rx, sdrhip_fecbuf **out)
{
    if (!rx || !out) return fail(SDRHIP_EINVAL, "rx_collector: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    int rc = rx_collector(rx);
    if (rc) return rc;
    *out = rx->fb;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_carry(const sdrhip_rx *rx, size_t *carry)
{
    if (!rx || !carry) return fail(SDRHIP_EINVAL, "rx_carry: NULL argument");
    sdrhip::CtxLock lock_(rx->ctx);
    unsigned *dev = nullptr;
    std::vector<size_t> *host = nullptr;
    if (rx->fb) {
        HIP_TRY(hipSetDevice(rx->ctx->device));
        int rc = fecbuf_join_carry(rx->fb, &dev, &host);
        if (rc) return rc;
    }
    for (int s = 0; s < rx->nstreams; ++s) carry[s] = host ? (*host)[(size_t)s] : 0;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_process_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                           const uint32_t *tv_sec, const uint32_t *tv_usec, size_t max_released, uint8_t *frames_out,
                                           size_t frame_stride_bytes, sdrhip_fecbuf_frame *info_out, size_t *n_released, size_t *n_frames,
                                           int mem)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_dgrams || !tv_sec || !tv_usec || !n_released || !n_frames)
        return fail(SDRHIP_EINVAL, "rx_process_datagrams: NULL count, stamp, n_released or n_frames array");
    sdrhip::CtxLock lock_(rx->ctx);
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    for (int s = 0; s < S; ++s) n_released[s] = n_frames[s] = 0;
    // ---- everything that can be refused is checked before the collector moves
    if (int e = check_mem(mem)) return e;
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "rx_process_datagrams: not available in pipelined mode");
    if (rx_batches_active(rx)) return fail(SDRHIP_EINVAL, "rx_process_datagrams: asynchronous batches are being filled or in flight: collect them first");
    if (max_released > 0x3fffffffu) return fail(SDRHIP_EINVAL, "rx_process_datagrams: max_released too large");
    if (max_released > 0 && !info_out) return fail(SDRHIP_EINVAL, "rx_process_datagrams: NULL info_out");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = rx_collector(rx))) return rc;
    if ((rc = fecbuf_check_dgrams(rx->fb, dgrams, n_dgrams, dgram_stride_bytes, mem, "rx_process_datagrams"))) return rc;
    unsigned *carry_dev = nullptr;
    std::vector<size_t> *carry = nullptr;
    if ((rc = fecbuf_join_carry(rx->fb, &carry_dev, &carry))) return rc;
    if (max_released > 0 && (rc = rx_join_rows(rx, max_released, "rx_process_datagrams"))) return rc;
    const size_t U = rx_join_unit(rx->cfg);
    Admit ad = {rx, carry, frames_out, frame_stride_bytes, mem, RxJoinCounts(), RxRaggedCounts()};
    const FecBufJoin join = {carry_dev, admit, &ad};
    const int *counts = nullptr;
    if ((rc = fecbuf_collect(rx->fb, dgrams, n_dgrams, dgram_stride_bytes, mem, max_released ? rx->j_rows.as<uint8_t>() : nullptr,
                             rx->j_row_len * 4, nullptr, max_released, info_out, n_released, &counts, &join)))
        return rc; // (SDRHIP_EINVAL: nothing consumed, nothing has run behind the classify pass)
    // ---- the collector's state has moved on: from here a failure loses the call's samples, it is never replayed
    // (ad.join / ad.n: admit's, counted from these n_released behind the read-back)
    if (!ad.join.any) { // (nothing released, and no row holds a whole unit: rows and remainders stay)
        rx->view.clear();
        return SDRHIP_OK;
    }
    // (follow: the state this call's collection committed -- fecbuf_collect has flipped the double buffer)
    const RxFramesOut out = {frames_out, frame_stride_bytes, n_frames, mem};
    const RxRaggedCall rows = {false, true, nullptr, rx->follow_meta ? fecbuf_committed_state(rx->fb) : nullptr,
                               rx->follow_bits ? fecbuf_committed_state(rx->fb) : nullptr};
    if ((rc = rx_ragged(rx, rx->j_rows.as<int16_t>(), ad.n, rx->j_row_len, tv_sec, tv_usec, out, rows))) return rc;
    hipError_t e = launch_rx_join_carry(rx->j_rows.as<int16_t>(), rx->j_row_len, carry_dev, counts, (unsigned)U, S, c->stream);
    if (e != hipSuccess) return fail(SDRHIP_EDEVICE, "rx join launch: %s", hipGetErrorString(e));
    *carry = ad.join.left;
    return SDRHIP_OK;
}
