// sdrhip_rx_async.cpp -- the asynchronous host-pointer entries of the Rx pipe (submit / collect, uniform and ragged batches).
#include "sdrhip_pipes.h"

using namespace sdrhip;

// --------------------------------------------------------------------------- asynchronous host-pointer Rx entry
// sdrdaemonrx's chain is asynchronous end to end (source thread -> source_buffer -> main loop -> output_buffer -> writer ->
// transmit thread, sdrdaemonrx.cpp:555-663): a block's frames leave the process long after Downsampler::process returned.
// sdrhip_rx_process on host pointers is one synchronous launch per block (38 us for a 65 536-sample TestSource block, of which
// the GPU works ~10); submit / collect give the host-pointer path the same asynchrony: blocks are appended to a pinned
// staging buffer (or taken in place from sdrhip_host_alloc memory), every `blocks` of them go out as ONE upload + launch +
// download on the context's stream, and the frames are collected later, batch by batch, in order.
namespace {
int rx_launch_batch(sdrhip_rx *rx, sdrhip_rx::Batch &b)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    // (8-bit input: the batch goes up as bytes, rows of a multiple of 8 samples; sdrhip_rx_process widens it on the device)
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2;
    const size_t dstride = esz == 4 ? (b.n_in + 3) & ~(size_t)3 : (b.n_in + 7) & ~(size_t)7;
    int rc;
    if ((rc = b.din.reserve((size_t)S * dstride * esz + 16))) return rc;
    // uploads: runs of blocks that are adjacent in host memory go out as ONE 2-D copy (a run of staged blocks -- stream-major in
    // the pinned arena -- or of in-place blocks cut from one buffer)
    size_t off = 0;
    for (size_t i = 0; i < b.blocks.size();) {
        const char *src = reinterpret_cast<const char *>(b.blocks[i].first);
        size_t sstride = b.strides[i], n = b.blocks[i].second, j = i + 1;
        if (!src) { // staged: [stream][in_cap] at sample offset `off` of every row (all staged blocks of a batch are one run)
            src = b.in.as<char>() + off * esz;
            sstride = b.in_cap;
            while (j < b.blocks.size() && !b.blocks[j].first) n += b.blocks[j++].second;
        } else {
            while (j < b.blocks.size() && reinterpret_cast<const char *>(b.blocks[j].first) == src + n * esz && b.strides[j] == sstride) n += b.blocks[j++].second;
        }
        if (S == 1) HIP_TRY(link_copy(c, b.din.as<char>() + off * esz, src, n * esz, hipMemcpyHostToDevice, c->stream)); // (no pitch limits)
        else HIP_TRY(link_copy2d(c, b.din.as<char>() + off * esz, dstride * esz, src, sstride * esz, n * esz, S, hipMemcpyHostToDevice, c->stream));
        off += n;
        i = j;
    }
    b.in.mark(c->stream);
    // everything that can fail for want of memory happens BEFORE the samples are consumed: a batch that failed here, or that
    // sdrhip_rx_process refused before its decimator launch went out, is launched again by the next submit / collect; one that fails
    // behind the decimator launch (rx->consumed) is dropped: its samples are in the filter state already, replaying them would
    // duplicate samples and shift every later stamp
    b.frame_bytes = (size_t)(SDRHIP_NB_ORIGINAL + rx->cfg.nb_fec) * SDRHIP_UDPSIZE;
    b.egress = 0;
    const size_t nf_max = sdrhip_rx_max_frames(rx, b.n_in);
    if (nf_max && (rc = b.out.reserve((size_t)S * nf_max * b.frame_bytes))) return rc;
    if ((rc = b.done.ensure())) return rc;
    size_t nf = 0;
    rc = sdrhip_rx_process(rx, b.din.as<int16_t>(), b.n_in, dstride, b.tv_sec, b.tv_usec, nullptr, 0, &nf, SDRHIP_MEM_DEVICE);
    if (rc) {
        if (rx->consumed) b.state = 0; // consumed and lost: never replayed (the pipe's own error stands)
        return rc;
    }
    b.frames = nf;
    hipError_t e = hipSuccess;
    if (nf > nf_max) e = hipErrorInvalidValue; // (cannot happen: rx_max_frames is the pipe's own bound)
    else if (nf && S == 1) e = link_copy(c, b.out.p, rx->view.window(0, b.frame_bytes), nf * b.frame_bytes, hipMemcpyDeviceToHost, c->stream);
    else if (nf) e = link_copy2d(c, b.out.p, nf * b.frame_bytes, rx->view.window(0, b.frame_bytes), rx->view.stride(), nf * b.frame_bytes, S, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) {
        b.state = 0; // consumed and lost: never replayed
        return fail(SDRHIP_EDEVICE, "rx batch download: %s (the batch's %zu frames per stream are lost)", hipGetErrorString(e), nf);
    }
    b.state = 2;
    return SDRHIP_OK;
}

// a ragged batch: ONE upload per run of adjacent packed memory -> K0p lays the rows out (and widens 8-bit input) -> per stream one
// sdrhip_rx_process_ragged step of the batch's summed counts with its first block's stamps -> the frames every stream delivered,
// compacted in stream order -> ONE download of exactly those frames.  Failure rules of rx_launch_batch: everything that can fail
// for want of memory happens before the decimator launch (the batch is launched again later); a failure behind it (rx->consumed)
// drops the batch.
int rx_launch_ragged(sdrhip_rx *rx, sdrhip_rx::Batch &b)
{
    sdrhip_ctx *c = rx->ctx;
    const int S = rx->nstreams;
    const size_t nblk = b.r_cnt.size() / (size_t)S;
    // (per-stream input format, sdrhip_rx_set_stream_format: K0x in K0p's place over the same table, rx_unpack_plan.h; the setter is
    // refused while a batch is being filled or in flight, so the formats are the ones the batch's bytes were staged with)
    const int *fmts = rx->streams.formats();
    const UnpackXPlan m = unpackx_measure(b.r_cnt.data(), nblk, (size_t)S, fmts, rx->in_fmt);
    const size_t pk_bytes = (size_t)m.bytes;
    // (what the step below completes: the buffers are sized from it before anything is consumed)
    const RxRaggedCounts n = rx_counts(rx, b.r_tot.data());
    const size_t sum_done = n.sum_done, dstride = (n.max_in + 7) & ~(size_t)7;
    const size_t fb = rx_frame_bytes(rx); // (per-stream fecblk: the slot pitch, a bound on every stream's frame)
    const size_t rows_bytes = (size_t)(S + 1) * sizeof(UnpackXRow), tab_bytes = rows_bytes + (size_t)m.nseg * sizeof(UnpackXSeg);
    const size_t list_off = (tab_bytes + 15) & ~(size_t)15;
    int rc;
    if ((rc = b.r_tab.reserve(list_off + sum_done * 4 + 16))) return rc; // (waits for the table upload of this batch's last use)
    if (list_off + sum_done * 4 + 16 > rx->a_tab.cap || pk_bytes + 64 > rx->a_pk.cap || (size_t)S * dstride * 4 + 16 > rx->a_din.cap ||
        sum_done * fb > rx->a_frames.cap)
        HIP_TRY(hipStreamSynchronize(c->stream)); // (a device buffer grows: batches in flight may still use the old one)
    if ((rc = rx->a_tab.reserve(list_off + sum_done * 4 + 16))) return rc;
    if ((rc = rx->a_pk.reserve(pk_bytes + 64))) return rc;
    if ((rc = rx->a_din.reserve((size_t)S * dstride * 4 + 16))) return rc;
    if (sum_done && (rc = b.out.reserve(sum_done * fb))) return rc;
    if (sum_done && (rc = rx->a_frames.reserve(sum_done * fb))) return rc;
    if ((rc = b.done.ensure())) return rc;
    b.egress = rx->egress; // (set_egress is refused while a batch is being filled: the order of the batch's first block)
    if (b.egress && (rc = rx_egress_room(rx, b, sum_done, fb / SDRHIP_UDPSIZE))) return rc;

    // ---- the table: segments stream by stream (block order inside), sources at their packed offsets (block-major, stream-minor)
    if (!unpackx_fill(b.r_cnt.data(), nblk, (size_t)S, fmts, 0, b.r_tab.as<UnpackXRow>(),
                      reinterpret_cast<UnpackXSeg *>(b.r_tab.as<char>() + rows_bytes), rx->in_fmt).fits)
        return fail(SDRHIP_EINVAL, "rx batch: too many samples for one launch");

    // ---- uploads: the packed samples, one copy per run of adjacent memory (staged runs are adjacent in the arena), then the table
    uint8_t *pk = rx->a_pk.as<uint8_t>();
    size_t off = 0;
    for (size_t i = 0; i < b.r_runs.size();) {
        const char *p0 = b.r_runs[i].p ? b.r_runs[i].p : b.in.as<char>() + b.r_runs[i].off;
        size_t n = b.r_runs[i].bytes, j = i + 1;
        for (; j < b.r_runs.size(); ++j) {
            const char *pj = b.r_runs[j].p ? b.r_runs[j].p : b.in.as<char>() + b.r_runs[j].off;
            if ((b.r_runs[j].p == nullptr) != (b.r_runs[i].p == nullptr) || pj != p0 + n) break;
            n += b.r_runs[j].bytes;
        }
        HIP_TRY(link_copy(c, pk + off, p0, n, hipMemcpyHostToDevice, c->stream));
        off += n;
        i = j;
    }
    b.in.mark(c->stream);
    if ((rc = rx_unpack_launch(rx, b.r_tab, rx->a_tab, tab_bytes, fmts, pk, rx->a_din.as<int16_t>(), dstride, (unsigned)m.grid))) return rc;

    // ---- the batch as one ragged step
    std::vector<size_t> nf((size_t)S, 0);
    const RxFramesOut view_only = {nullptr, 0, nf.data(), SDRHIP_MEM_DEVICE};
    const RxRaggedCall batch = {true, false, nullptr, nullptr, nullptr};
    rc = rx_ragged(rx, rx->a_din.as<int16_t>(), n, dstride, b.r_sec.data(), b.r_usec.data(), view_only, batch);
    if (rc) {
        if (rx->consumed) b.state = 0; // consumed and lost: never replayed (the pipe's own error stands)
        return rc;
    }

    // ---- download: the delivered frames of every stream, compacted in stream order, in ONE copy
    int32_t *list = reinterpret_cast<int32_t *>(b.r_tab.as<char>() + list_off);
    size_t nl = 0;
    hipError_t e = hipSuccess;
    for (int s = 0; s < S; ++s)
        for (size_t f = 0; f < nf[(size_t)s]; ++f) list[nl++] = (int32_t)(rx->view.offset((size_t)s, fb) / fb + f);
    // (departure order: KR / KP in the gather's place writes the same buffer, sdrhip_rx_egress.cpp)
    if (e == hipSuccess && nl && b.egress) e = rx_egress_launch(rx, b, nf.data(), fb, nullptr, 0, nullptr);
    else if (e == hipSuccess && nl) e = hipMemcpyAsync(rx->a_tab.as<char>() + list_off, list, nl * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nl && !b.egress) {
        b.r_tab.mark(c->stream);
        e = launch_frame_gather(rx->work.as<uint8_t>(), fb, reinterpret_cast<const int32_t *>(rx->a_tab.as<char>() + list_off), nl,
                                rx->a_frames.as<uint8_t>(), c->stream);
    }
    // (a departure-order batch of frames of different lengths: exactly its datagrams)
    const size_t down = b.egress && !b.e_blocks.empty() ? b.e_dgrams * SDRHIP_UDPSIZE : nl * fb;
    if (e == hipSuccess && nl) e = link_copy(c, b.out.p, rx->a_frames.p, down, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(b.done, c->stream);
    if (e != hipSuccess) {
        b.state = 0; // consumed and lost: never replayed
        return fail(SDRHIP_EDEVICE, "rx ragged batch download: %s (the batch's %zu frames are lost)", hipGetErrorString(e), nl);
    }
    b.r_frames.assign(nf.begin(), nf.end());
    b.frame_bytes = fb;
    b.state = 2;
    return SDRHIP_OK;
}
} // namespace

int sdrhip::rx_launch_filling(sdrhip_rx *rx, sdrhip_rx::Batch &b) { return b.ragged ? rx_launch_ragged(rx, b) : rx_launch_batch(rx, b); }

extern "C" int sdrhip_rx_set_async(sdrhip_rx *rx, int depth, int blocks)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (depth < 1 || depth > 64 || blocks < 1 || blocks > 1024) return fail(SDRHIP_EINVAL, "rx_set_async: depth 1..64, blocks 1..1024");
    if (rx->ring.busy()) return fail(SDRHIP_EINVAL, "rx_set_async: batches are in flight or lent: collect and release them first");
    rx->ring.reset((size_t)depth);
    rx->a_blocks = blocks;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_submit(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec, uint32_t tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    sdrhip::CtxLock lock_(rx->ctx);
    if (int e = rx_refuse_uniform("rx_submit", "sdrhip_rx_submit_ragged", rx->streams.forces_ragged())) return e;
    if (rx->egress) return fail(SDRHIP_EINVAL, "rx_submit: uniform batches have no departure order (sdrhip_rx_set_egress): use sdrhip_rx_submit_ragged with equal counts");
    if (n_in == 0) return SDRHIP_OK;
    if (!iq_in) return fail(SDRHIP_EINVAL, "rx_submit: NULL input");
    if (rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_submit: asynchronous datagram batches are in flight: sdrhip_rx_collect_datagrams them first");
    if (!rx->area.aligned()) return fail(SDRHIP_EINVAL, "rx_submit: ragged calls left the streams at different frame positions");
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_submit: ragged batches are being filled or in flight: collect them first");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    const int S = rx->nstreams;
    if (S == 1) in_stride = n_in;
    sdrhip_rx::Batch &b = rx->ring.tail_batch();
    if (b.state >= 2) return fail(SDRHIP_EBUSY, "rx_submit: every batch of the ring is in flight or lent: sdrhip_rx_collect first");
    if (b.state == 0) {
        b.blocks.clear(); b.strides.clear(); b.n_in = 0; b.tv_sec = tv_sec; b.tv_usec = tv_usec; b.state = 1; b.ragged = false;
        b.in_cap = 0; // no staged rows yet: the first pageable block of this batch (re)claims the arena
    }
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2; // bytes per sample (sdrhip_rx_set_input_format)
    const char *src = reinterpret_cast<const char *>(iq_in);
    if (host_is_pinned(iq_in, ((size_t)(S - 1) * in_stride + n_in) * esz)) {
        b.blocks.push_back(std::make_pair(iq_in, n_in)); // in place: the caller keeps it untouched until the batch is collected
        b.strides.push_back(in_stride);
    } else {
        // staged: row s of the pinned arena holds stream s, the block at the batch's current sample offset
        // (in-place blocks in front of it leave their part of the rows unused: a block always sits at its batch offset)
        const size_t need = b.n_in + n_in;
        if (b.in_cap == 0) { // first staged block of the batch, whatever came before it in place
            const size_t cap = (size_t)rx->a_blocks * n_in > need ? (size_t)rx->a_blocks * n_in : need;
            int rc = b.in.reserve((size_t)S * cap * esz); // (waits for the upload of the batch that used this buffer last)
            if (rc) return rc;
            b.in_cap = cap;
        } else if (need > b.in_cap) { // blocks longer than the first one: re-lay the rows out in a bigger arena
            PinnedBuf bigger;
            const size_t ncap = 2 * need;
            int rc = bigger.reserve((size_t)S * ncap * esz);
            if (rc) return rc;
            for (int s = 0; s < S; ++s) memcpy(bigger.as<char>() + (size_t)s * ncap * esz, b.in.as<char>() + (size_t)s * b.in_cap * esz, b.n_in * esz);
            b.in = std::move(bigger);
            b.in_cap = ncap;
        }
        for (int s = 0; s < S; ++s) memcpy(b.in.as<char>() + ((size_t)s * b.in_cap + b.n_in) * esz, src + (size_t)s * in_stride * esz, n_in * esz);
        b.blocks.push_back(std::make_pair((const int16_t *)nullptr, n_in));
        b.strides.push_back(n_in);
    }
    b.n_in += n_in;
    if ((int)b.blocks.size() >= rx->a_blocks) {
        int rc = rx_launch_batch(rx, b);
        if (rc) return rc;
        ++rx->ring.tail;
    }
    return SDRHIP_OK;
}

// the oldest batch of the ring once it has finished; wait = 1 launches a partly filled one as it is (the end of a stream)
static int rx_oldest(sdrhip_rx *rx, std::unique_lock<std::recursive_mutex> &lock_, int wait, const char *who, sdrhip_rx::Batch **bp)
{
    return rx->ring.wait_oldest(lock_, wait, who, [rx](sdrhip_rx::Batch &b) { return rx_launch_filling(rx, b); }, bp);
}

extern "C" int sdrhip_rx_collect(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames, int wait)
{
    if (!rx || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    *n_frames = 0;
    if (rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_collect: asynchronous datagram batches are in flight: sdrhip_rx_collect_datagrams them first");
    if (rx_has_batches(rx, true)) return fail(SDRHIP_EINVAL, "rx_collect: ragged batches are being filled or in flight: use sdrhip_rx_collect_ragged");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    int rc = rx_oldest(rx, lock_, wait, "rx_collect", &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    const int S = rx->nstreams;
    if (b.frames > max_frames) { // (the batch stays where it is: call again with room for *n_frames frames per stream)
        *n_frames = b.frames;
        return fail(SDRHIP_EINVAL, "rx_collect: the batch holds %zu frames per stream, frames_out has room for %zu", b.frames, max_frames);
    }
    if (b.frames) {
        if (!frames_out) return fail(SDRHIP_EINVAL, "rx_collect: NULL frames_out");
        const size_t row = b.frames * b.frame_bytes;
        if (S > 1 && frame_stride_bytes < row) return fail(SDRHIP_EINVAL, "rx_collect: frame stride too small");
        for (int s = 0; s < S; ++s) memcpy(frames_out + (size_t)s * (S > 1 ? frame_stride_bytes : row), b.out.as<char>() + (size_t)s * row, row);
    }
    *n_frames = b.frames;
    b.state = 0;
    ++rx->ring.head;
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_submit_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                                       const uint32_t *tv_usec)
{
    if (!rx) return fail(SDRHIP_EINVAL, "rx is NULL");
    if (!n_in || !tv_sec || !tv_usec) return fail(SDRHIP_EINVAL, "rx_submit_ragged: NULL count or stamp array");
    sdrhip::CtxLock lock_(rx->ctx);
    // ---- everything that can be refused is checked before anything is consumed
    const int S = rx->nstreams;
    size_t max_in = 0, sum = 0;
    for (int s = 0; s < S; ++s) { sum += n_in[s]; if (n_in[s] > max_in) max_in = n_in[s]; }
    if (in_stride != SDRHIP_PACKED && in_stride < max_in)
        return fail(SDRHIP_EINVAL, "rx_submit_ragged: in_stride is neither SDRHIP_PACKED nor at least the largest count");
    if (sum && !iq_in) return fail(SDRHIP_EINVAL, "rx_submit_ragged: NULL input");
    if (rx->pipelined) return fail(SDRHIP_EINVAL, "rx_submit_ragged: not available in pipelined mode");
    if (rx_fec_mixed(rx) && !rx->egress)
        return fail(SDRHIP_EINVAL, "rx_submit_ragged: the streams' fecblk differ (sdrhip_rx_set_stream_fec): such a batch is delivered in departure order only, sdrhip_rx_set_egress first");
    if (rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_submit_ragged: asynchronous datagram batches are in flight: sdrhip_rx_collect_datagrams them first");
    if (rx_has_batches(rx, false)) return fail(SDRHIP_EINVAL, "rx_submit_ragged: uniform batches are being filled or in flight: collect them first");
    sdrhip_rx::Batch &b = rx->ring.tail_batch();
    if (b.state >= 2) return fail(SDRHIP_EBUSY, "rx_submit_ragged: every batch of the ring is in flight or lent: collect or release one first");
    for (int s = 0; s < S; ++s) // (the unpack table holds 32-bit row positions)
        if ((b.state == 1 ? b.r_tot[(size_t)s] : 0) + n_in[s] > (size_t)0xffffffffu - UNPACKX_WG_SAMPLES)
            return fail(SDRHIP_EINVAL, "rx_submit_ragged: a stream's batch would exceed 2^32 - 4096 samples");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    const size_t esz = rx->in_fmt == IQF_S16 ? 4 : 2; // bytes per sample (sdrhip_rx_set_input_format)
    const char *src = reinterpret_cast<const char *>(iq_in);
    // (per-stream input format: a row's bytes follow its own format; a strided row starts at 4-byte unit s * in_stride whatever it holds)
    const int *fmts = rx->streams.formats();
    const size_t unit = fmts ? 4 : esz;
    size_t sum_bytes = 0;
    for (int s = 0; s < S; ++s) sum_bytes += n_in[s] * (fmts ? unpackx_sample_bytes(fmts[s]) : esz);
    const bool inplace = in_stride == SDRHIP_PACKED && sum && host_is_pinned(iq_in, sum_bytes);
    if (sum && !inplace) { // (the arena: the staged blocks of the batch back to back, packed)
        const size_t used = b.state == 1 ? b.r_used : 0, need = used + sum_bytes;
        if (used == 0) {
            const size_t cap = (size_t)rx->a_blocks * sum_bytes > need ? (size_t)rx->a_blocks * sum_bytes : need;
            int rc = b.in.reserve(cap); // (waits for the upload of the batch that used this buffer last)
            if (rc) return rc;
        } else if (need > b.in.cap) {
            PinnedBuf bigger;
            int rc = bigger.reserve(2 * need);
            if (rc) return rc;
            memcpy(bigger.p, b.in.p, used);
            b.in = std::move(bigger);
        }
    }
    if (b.state == 0) { // the batch's first block: its stamps are the batch's
        b.ragged = true; b.state = 1;
        b.r_runs.clear(); b.r_cnt.clear(); b.r_used = 0;
        b.r_tot.assign((size_t)S, 0);
        b.r_sec.assign(tv_sec, tv_sec + S); b.r_usec.assign(tv_usec, tv_usec + S);
    }
    if (inplace) { // in place: the caller keeps it untouched until the batch is collected
        b.r_runs.push_back(sdrhip_rx::Batch::Run{src, 0, sum_bytes});
    } else if (sum) { // staged packed: one memcpy per non-empty row, never the padding of a strided row
        rx_pack_rows(b.in.as<char>() + b.r_used, src, in_stride * unit, n_in, fmts, rx->in_fmt, (size_t)S);
        b.r_runs.push_back(sdrhip_rx::Batch::Run{nullptr, b.r_used, sum_bytes});
        b.r_used += sum_bytes;
    }
    b.r_cnt.insert(b.r_cnt.end(), n_in, n_in + S);
    for (int s = 0; s < S; ++s) b.r_tot[(size_t)s] += n_in[s];
    if ((int)(b.r_cnt.size() / (size_t)S) >= rx->a_blocks) {
        int rc = rx_launch_ragged(rx, b);
        if (rc) return rc;
        ++rx->ring.tail;
    }
    return SDRHIP_OK;
}

extern "C" int sdrhip_rx_collect_ragged(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames,
                                        int wait)
{
    if (!rx || !n_frames) return fail(SDRHIP_EINVAL, "rx_collect_ragged: NULL argument");
    std::unique_lock<std::recursive_mutex> lock_(rx->ctx->mtx);
    const int S = rx->nstreams;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    if (rx_dgrams_in_flight(rx)) return fail(SDRHIP_EINVAL, "rx_collect_ragged: asynchronous datagram batches are in flight: use sdrhip_rx_collect_datagrams");
    if (rx_has_batches(rx, false)) return fail(SDRHIP_EINVAL, "rx_collect_ragged: uniform batches are being filled or in flight: use sdrhip_rx_collect");
    HIP_TRY(hipSetDevice(rx->ctx->device));
    sdrhip_rx::Batch *bp = nullptr;
    int rc = rx_oldest(rx, lock_, wait, "rx_collect_ragged", &bp);
    if (rc) return rc;
    sdrhip_rx::Batch &b = *bp;
    if (b.egress) return fail(SDRHIP_EINVAL, "rx_collect_ragged: the batch was launched in departure order: use sdrhip_rx_collect_egress (the batch stays)");
    size_t most = 0;
    for (int s = 0; s < S; ++s) if (b.r_frames[(size_t)s] > most) most = b.r_frames[(size_t)s];
    if (most > max_frames) { // (the batch stays where it is: call again with room for the largest n_frames[s])
        for (int s = 0; s < S; ++s) n_frames[s] = b.r_frames[(size_t)s];
        return fail(SDRHIP_EINVAL, "rx_collect_ragged: a stream of the batch holds %zu frames, frames_out has room for %zu", most, max_frames);
    }
    if (most) {
        if (!frames_out) return fail(SDRHIP_EINVAL, "rx_collect_ragged: NULL frames_out");
        if (S > 1 && frame_stride_bytes < most * b.frame_bytes) return fail(SDRHIP_EINVAL, "rx_collect_ragged: frame stride too small");
        size_t off = 0;
        for (int s = 0; s < S; ++s) {
            const size_t row = b.r_frames[(size_t)s] * b.frame_bytes;
            if (row) memcpy(frames_out + (size_t)s * frame_stride_bytes, b.out.as<char>() + off, row);
            off += row;
        }
    }
    for (int s = 0; s < S; ++s) n_frames[s] = b.r_frames[(size_t)s];
    b.state = 0;
    ++rx->ring.head;
    return SDRHIP_OK;
}
