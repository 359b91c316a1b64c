// fecbuf_passes.h -- the classify, scatter and copy passes of the FEC buffer bank (fecbuf_kernels.hip describes them), included
// inside `namespace sdrhip { namespace {`: with FB_PACKED 0 by fecbuf_kernels.hip (the kernels of the bank's calls), with
// FB_PACKED 1 by tx_async_kernels.hip (the instantiations of the asynchronous Tx batches, sdrhip_tx_submit_datagrams).  Packed: stream s's datagrams lie back to back at a.dg + dg_off[s], and
// the scatter grid is the host's shadow of the classification: a job past the classify pass's own count, a frame at or past
// max_frames and a staging slot at or past nslots are skipped, and the copy skips a slot the scatter pass did not fill (dmap preset
// to -1), so that counts that disagree with the shadow (the shadow check counts them) never write outside the buffers.  (One text
// for both: the bank's kernels compile to the instructions they had.)
// With FB_ROWS 1 (and FB_PACKED 0) by rx_join_kernels.hip: the scatter and copy passes alone, for the Rx pipe fed datagrams
// (sdrhip_rx_process_datagrams): stream s's payloads go row_off[s] samples behind a.data_out + s * a.data_stride, behind the
// samples the stream's row holds back from earlier calls.
// With FB_PACKED 1 and FB_ROWS 1 by rx_dgram_async_kernels.hip: the scatter and the guarded copy pass of asynchronous datagram-fed Rx
// batches (sdrhip_rx_submit_datagrams): packed datagrams in, payloads behind row_off[s]; on top of the packed guards a frame whose
// payload would end past the stream's row (a.data_stride bytes) is skipped.
#ifndef FB_ROWS
#define FB_ROWS 0
#endif
#ifndef SDRHIP_FECBUF_PASSES_COMMON
#define SDRHIP_FECBUF_PASSES_COMMON
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));

constexpr int CL_NT = 1024; // classify: datagrams per chunk = threads per workgroup
constexpr int CL_NW = CL_NT / 64;
constexpr int SC_NT = 256;  // scatter / copy
constexpr size_t SB = 512, PAYLOAD = 127 * 508, CARRY_STREAM = 128 * 512;

__device__ __forceinline__ unsigned load_header(const uint8_t *dg, long long i)
{
    return __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(dg + (size_t)i * SB));
}

// exclusive prefix over the workgroup of a per-thread flag; *total = the workgroup's count.  Two barriers.
__device__ __forceinline__ int wg_scan(bool flag, int *w_cnt, int *total)
{
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const unsigned long long m = __ballot(flag);
    if (lane == 0) w_cnt[wv] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < CL_NW; ++w) {
        const int c = w_cnt[w];
        before += w < wv ? c : 0;
        all += c;
    }
    __syncthreads();
    *total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// copies `ndw` dwords, four loads in flight per thread before their stores
__device__ __forceinline__ void copy_dwords(unsigned *dst, const unsigned *src, int ndw)
{
    int j = (int)threadIdx.x;
    for (; j + 3 * SC_NT < ndw; j += 4 * SC_NT) {
        const unsigned v0 = __builtin_nontemporal_load(src + j), v1 = __builtin_nontemporal_load(src + j + SC_NT);
        const unsigned v2 = __builtin_nontemporal_load(src + j + 2 * SC_NT), v3 = __builtin_nontemporal_load(src + j + 3 * SC_NT);
        dst[j] = v0; dst[j + SC_NT] = v1; dst[j + 2 * SC_NT] = v2; dst[j + 3 * SC_NT] = v3;
    }
    for (; j < ndw; j += SC_NT) dst[j] = __builtin_nontemporal_load(src + j);
}

#endif

#if FB_PACKED
#define FB_STREAM_DG(s) (a.dg + dg_off[s])
#else
#define FB_STREAM_DG(s) (a.dg + (size_t)(s) * a.dg_stride)
#endif
#if FB_ROWS
#define FB_STREAM_OUT(s) (a.data_out + (size_t)(s) * a.data_stride + (size_t)row_off[s] * 4)
#else
#define FB_STREAM_OUT(s) (a.data_out + (size_t)(s) * a.data_stride)
#endif
#if FB_PACKED && FB_ROWS
#define FB_PAST_ROW(s, k) ((size_t)row_off[s] * 4 + (size_t)((k) + 1) * PAYLOAD > a.data_stride)
#endif

#if !FB_ROWS
#if FB_PACKED
__global__ __launch_bounds__(CL_NT) void fecbuf_classify_packed_kernel(FecBufArgs a, const long long *dg_off)
#else
__global__ __launch_bounds__(CL_NT) void fecbuf_classify_kernel(FecBufArgs a)
#endif
{
    const int s = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = a.ndg[s];
    const uint8_t *dg = FB_STREAM_DG(s);
    const FecBufState &S0 = a.st_cur[s];
    FecBufRec *rec = a.rec + a.rec_base[s];
    FecBufPub *pub = a.pub + (size_t)s * a.max_frames;

    __shared__ unsigned l_fi[CL_NT];
    __shared__ int l_recov[CL_NT + 1], l_maxrow[CL_NT + 1], l_dup[CL_NT + 1];
    __shared__ unsigned l_pres[CL_NT + 1][4];
    __shared__ int w_cnt[CL_NW], w_last[CL_NW];
    // the frame open at the start of the chunk (ordinal, segment start, frame index, accumulators)
    __shared__ int r_ord, r_seg, r_head, r_recov, r_maxrow, r_dup, r_dcount;
    __shared__ unsigned r_pres[4];
    // stream results
    __shared__ int x_min, x_max, x_last, x_cur_b, x_cur_r, x_maxrow, x_maxrec;
    __shared__ int o_count, o_recov, o_maxrow, o_dup, o_ord, o_b0;
    __shared__ unsigned o_pres[4], o_head;
    // meta events of the chunk's frames (bit 0: released with block 0 -> m_outputMeta, bit 1: reached 128 blocks with block 0 ->
    // m_currentMeta), their MetaDataFEC; the two metas
    __shared__ int l_b0[CL_NT + 1];
    __shared__ unsigned char q_flag[CL_NT + 1];
    __shared__ unsigned q_meta[CL_NT + 1][5];
    __shared__ unsigned m_meta[2][5];
    __shared__ int r_b0;
    const uint8_t *carry_rd = a.carry_cur_base + ((size_t)S0.cbuf * a.nstreams + s) * CARRY_STREAM;
    // the MetaDataFEC (20 bytes) of a frame: block 0's last arrival among its first 128 (rank b0 from segment start seg)
    auto meta_src = [&](int seg, int b0) -> const unsigned * {
        const long long pos = (long long)seg + b0;
        return reinterpret_cast<const unsigned *>((pos < 0 ? carry_rd + (size_t)b0 * SB : dg + (size_t)pos * SB) + 4);
    };

    if (t == 0) {
        r_ord = 0; r_seg = -S0.count; r_head = S0.head;
        r_recov = S0.recov; r_maxrow = S0.maxrow; r_dup = S0.dup;
        for (int q = 0; q < 4; ++q) r_pres[q] = S0.pres[q];
        r_dcount = 0; r_b0 = S0.b0; o_b0 = S0.b0;
        for (int q = 0; q < 5; ++q) { m_meta[0][q] = S0.out_meta[q]; m_meta[1][q] = S0.cur_meta[q]; }
        x_min = S0.min_blocks; x_max = S0.max_recov; x_last = -1; x_cur_b = S0.cur_blocks; x_cur_r = S0.cur_recov;
        x_maxrow = -1; x_maxrec = 0;
        o_ord = 0; o_count = S0.count; o_recov = S0.recov; o_maxrow = S0.maxrow; o_dup = S0.dup; o_head = (unsigned)S0.head;
        for (int q = 0; q < 4; ++q) o_pres[q] = S0.pres[q];
        // datagram 0 of another frame releases the carried slot (ordinal 0) at once: its record comes from the state
        if (n > 0 && (int)(load_header(dg, 0) & 0xffffu) != S0.head) {
            const int bc = S0.count;
            const bool meta = S0.b0 >= 0;
            const bool dec = bc >= 128 && S0.recov > 0 && !S0.dup;
            unsigned fl = (bc >= 128 ? FB_DECODED : 0) | (meta ? FB_META : 0);
            if (bc >= 128 && S0.recov > 0) fl |= S0.dup ? FB_DECODE_ERROR : FB_REPAIRED;
            rec[0] = FecBufRec{-bc, bc, dec ? 0 : -1, (int)fl};
            if (a.max_frames > 0) pub[0] = FecBufPub{S0.head, bc, S0.recov, fl};
            if (dec) { r_dcount = 1; x_maxrow = S0.maxrow; x_maxrec = S0.recov; }
            // (SDRdaemonFECBuffer compares only the first 12 bytes of MetaDataFEC before it assigns: MetaDataFEC::operator==)
            if (meta) {
                const unsigned *m = meta_src(-bc, S0.b0);
                unsigned v[5];
                for (int q = 0; q < 5; ++q) v[q] = m[q];
                for (int which = 0; which < (bc >= 128 ? 2 : 1); ++which)
                    if (v[0] != m_meta[which][0] || v[1] != m_meta[which][1] || v[2] != m_meta[which][2])
                        for (int q = 0; q < 5; ++q) m_meta[which][q] = v[q];
            }
            x_min = min(x_min, bc); x_max = max(x_max, S0.recov); x_last = 0; x_cur_b = bc; x_cur_r = S0.recov;
        }
    }
    __syncthreads();

    for (int base = 0; base < n; base += CL_NT) {
        const int i = base + t;
        const bool valid = i < n;
        const unsigned h = valid ? load_header(dg, i) : 0u;
        const unsigned fi = h & 0xffffu;
        const int bi = (int)((h >> 16) & 0xffu);
        l_fi[t] = fi;
        __syncthreads();
        const bool start = valid && (t == 0 ? (int)fi != r_head : fi != l_fi[t - 1]);
        const unsigned long long sm = __ballot(start);
        // ordinal and segment start (last start at or before i)
        if (lane == 0) {
            w_cnt[wv] = __popcll(sm);
            w_last[wv] = sm ? base + wv * 64 + 63 - __clzll(sm) : -0x7fffffff - 1;
        }
        // accumulators of the chunk's frames (entry 0: the frame open at the chunk's start, unless datagram `base` starts one)
        const bool cont = l_fi[0] == (unsigned)r_head; // (datagram `base` continues the running frame; base < n here)
        for (int e = t; e <= CL_NT; e += CL_NT) {
            const bool carry = e == 0 && cont;
            l_recov[e] = carry ? r_recov : 0;
            l_maxrow[e] = carry ? r_maxrow : -1;
            l_dup[e] = carry ? r_dup : 0;
            l_b0[e] = carry ? r_b0 : -1;
            q_flag[e] = 0;
            for (int q = 0; q < 4; ++q) l_pres[e][q] = carry ? r_pres[q] : 0u;
        }
        __syncthreads();
        int ord = r_ord, seg = r_seg;
        for (int w = 0; w < wv; ++w) { ord += w_cnt[w]; seg = max(seg, w_last[w]); }
        const unsigned long long le = sm & (~0ull >> (63 - lane));
        ord += __popcll(le);
        if (le) seg = base + wv * 64 + 63 - __clzll(le);
        const int ord_first = r_ord + (cont ? 0 : 1);
        const int lo = ord - ord_first;
        const int rank = i - seg;
        if (valid && rank < 128) {
            if (bi >= 128) {
                atomicAdd(&l_recov[lo], 1);
                atomicMax(&l_maxrow[lo], bi - 128);
            } else {
                if (bi == 0) atomicMax(&l_b0[lo], rank);
                const unsigned bit = 1u << (bi & 31);
                if (atomicOr(&l_pres[lo][bi >> 5], bit) & bit) l_dup[lo] = 1;
            }
        }
        // is datagram i the last of a released frame?
        bool end = false;
        if (valid && i + 1 < n) {
            const unsigned nfi = t + 1 < CL_NT ? l_fi[t + 1] : (load_header(dg, i + 1) & 0xffffu);
            end = nfi != fi;
        }
        __syncthreads();
        const int bc = rank + 1;
        int recov = 0, maxrow = -1, dup = 0;
        int b0 = -1;
        if (valid && (end || i == n - 1)) { recov = l_recov[lo]; maxrow = l_maxrow[lo]; dup = l_dup[lo]; b0 = l_b0[lo]; }
        const bool meta = b0 >= 0;
        const int mev = meta ? (end ? 1 : 0) | (bc >= 128 ? 2 : 0) : 0;
        if (mev) {
            const unsigned *m = meta_src(seg, b0);
            for (int q = 0; q < 5; ++q) q_meta[lo][q] = m[q];
            q_flag[lo] = (unsigned char)mev;
        }
        const bool dec = end && bc >= 128 && recov > 0 && !dup;
        int ndec = 0;
        const int drank = wg_scan(dec, w_cnt, &ndec);
        if (end) {
            unsigned fl = (bc >= 128 ? FB_DECODED : 0) | (meta ? FB_META : 0);
            if (bc >= 128 && recov > 0) fl |= dup ? FB_DECODE_ERROR : FB_REPAIRED;
            rec[ord] = FecBufRec{seg, bc, dec ? r_dcount + drank : -1, (int)fl};
            if (ord < a.max_frames) pub[ord] = FecBufPub{(int)fi, bc, recov, fl};
            if (dec) { atomicMax(&x_maxrow, maxrow); atomicMax(&x_maxrec, recov); }
            atomicMin(&x_min, bc);
            atomicMax(&x_max, recov);
            atomicMax(&x_last, ord);
        }
        if (valid && i == n - 1) { // the open slot after the call
            o_ord = ord; o_count = bc; o_recov = recov; o_maxrow = maxrow; o_dup = dup; o_head = fi;
            rec[ord] = FecBufRec{seg, bc, -1, 0}; o_b0 = b0;
            for (int q = 0; q < 4; ++q) o_pres[q] = l_pres[lo][q];
        }
        __syncthreads();
        if (wv == 0) { // the chunk's meta events in frame order (wave 0; a handful per chunk)
            for (int e0 = 0; e0 <= CL_NT; e0 += 64) {
                const int e = e0 + lane;
                unsigned long long qm = __ballot(e <= CL_NT && q_flag[e] != 0);
                while (qm) {
                    const int ee = e0 + __builtin_ctzll(qm);
                    qm &= qm - 1ull;
                    const int fl = q_flag[ee];
                    for (int which = 0; which < 2; ++which)
                        if ((fl >> which) & 1)
                            if (q_meta[ee][0] != m_meta[which][0] || q_meta[ee][1] != m_meta[which][1] || q_meta[ee][2] != m_meta[which][2])
                                if (lane < 5) m_meta[which][lane] = q_meta[ee][lane];
                }
            }
        }
        if (end && ord == x_last) { x_cur_b = bc; x_cur_r = recov; }
        if (t == CL_NT - 1 && valid) { // the frame open at the end of the chunk runs on
            r_ord = ord; r_seg = seg; r_head = (int)fi;
            r_recov = l_recov[lo]; r_maxrow = l_maxrow[lo]; r_dup = l_dup[lo]; r_b0 = l_b0[lo];
            for (int q = 0; q < 4; ++q) r_pres[q] = l_pres[lo][q];
        }
        if (t == 0) r_dcount += ndec;
        __syncthreads();
    }

    if (t == 0) {
        if (n == 0) rec[0] = FecBufRec{-S0.count, S0.count, -1, 0}; // (the open slot runs on untouched)
        FecBufState &N = a.st_next[s];
        N.head = n > 0 ? (int)o_head : S0.head;
        N.count = o_count; N.recov = o_recov; N.maxrow = o_maxrow; N.dup = o_dup;
        for (int q = 0; q < 4; ++q) N.pres[q] = o_pres[q];
        N.cbuf = o_ord == 0 ? S0.cbuf : S0.cbuf ^ 1;
        N.cur_blocks = x_cur_b; N.cur_recov = x_cur_r; N.min_blocks = x_min; N.max_recov = x_max;
        for (int q = 0; q < 5; ++q) { N.cur_meta[q] = m_meta[1][q]; N.out_meta[q] = m_meta[0][q]; }
        N.cur_meta[5] = N.out_meta[5] = 0u;
        N.b0 = o_b0; N.pad = 0;
        int *c = a.counts + (size_t)s * FB_COUNTS;
        c[FB_K] = o_ord; c[FB_D] = r_dcount; c[FB_MAXROW] = x_maxrow; c[FB_MAXREC] = x_maxrec; 
        c[6] = c[7] = 0;
    }
}
#endif // !FB_ROWS

#if FB_PACKED && FB_ROWS
__global__ __launch_bounds__(SC_NT) void fecbuf_scatter_packed_rows_kernel(FecBufArgs a, const long long *dg_off, int nslots, const unsigned *row_off)
#elif FB_PACKED
__global__ __launch_bounds__(SC_NT) void fecbuf_scatter_packed_kernel(FecBufArgs a, const long long *dg_off, int nslots)
#elif FB_ROWS
__global__ __launch_bounds__(SC_NT) void fecbuf_scatter_rows_kernel(FecBufArgs a, const unsigned *row_off)
#else
__global__ __launch_bounds__(SC_NT) void fecbuf_scatter_kernel(FecBufArgs a)
#endif
{
    const int job = (int)blockIdx.x, t = (int)threadIdx.x;
    // the stream of this job: job_off[s] <= job < job_off[s + 1]
    int lo = 0, hi = a.nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.job_off[mid] <= job) lo = mid; else hi = mid - 1;
    }
    const int s = lo, k = job - a.job_off[s];
    const int *cnt = a.counts + (size_t)s * FB_COUNTS;
    const int K = cnt[FB_K];
#if FB_PACKED
    if (k > K || (k < K && k >= a.max_frames)) return; // (the grid is the shadow's: see the file's head)
#endif
    const FecBufRec r = a.rec[a.rec_base[s] + k];
    const uint8_t *dg = FB_STREAM_DG(s);
    const uint8_t *carry_rd = a.carry_cur_base + ((size_t)a.st_cur[s].cbuf * a.nstreams + s) * CARRY_STREAM;
    const int stored = min(r.count, 128);

    __shared__ int s_win[128];
    __shared__ unsigned char s_idx[128];
    if (t < 128) s_win[t] = -1;
    __syncthreads();
    if (t < stored) {
        const long long pos = (long long)r.start + t;
        const uint8_t *src = pos < 0 ? carry_rd + (size_t)t * SB : dg + (size_t)pos * SB;
        const int bi = (int)((*reinterpret_cast<const unsigned *>(src) >> 16) & 0xffu);
        s_idx[t] = (unsigned char)bi;
        if (bi < 128) atomicMax(&s_win[bi], t); // the last arrival of an original wins (m_frame.m_blocks[blockIndex] = ...)
    }
    __syncthreads();
    auto src_of = [&](int rank) -> const uint8_t * {
        const long long pos = (long long)r.start + rank;
        return pos < 0 ? carry_rd + (size_t)rank * SB : dg + (size_t)pos * SB;
    };

    if (k == K) {
        // open slot: its new arrivals among the first 128 go to the carry buffer of the next call (another buffer than the one
        // read here when the slot is a new one: the state of the call in front stays intact until this call commits)
        uint8_t *carry_wr = a.carry_base + ((size_t)a.st_next[s].cbuf * a.nstreams + s) * CARRY_STREAM;
        const int first = r.start < 0 ? -r.start : 0; // (ranks below come from the carry buffer and are there already)
        const int nq = (stored - first) * (int)(SB / 16);
        for (int j = t; j < nq; j += SC_NT) {
            const int rank = first + j / (int)(SB / 16), q = j % (int)(SB / 16);
            reinterpret_cast<uint4_t *>(carry_wr + (size_t)rank * SB)[q] = reinterpret_cast<const uint4_t *>(src_of(rank))[q];
        }
        return;
    }

    if (r.dslot >= 0) {
        // to the decoder: the 128 arrivals as received (no repeated original in such a frame)
        const int slot = a.dbase[s] + r.dslot;
#if FB_PACKED
        if (slot >= nslots) return;
#endif
        uint8_t *st = a.stage + (size_t)slot * CARRY_STREAM;
        if (t == 0) { a.dmap[2 * slot] = s; a.dmap[2 * slot + 1] = k; }
        for (int j = t; j < 128 * (int)(SB / 16); j += SC_NT) {
            const int rank = j / (int)(SB / 16), q = j % (int)(SB / 16);
            reinterpret_cast<uint4_t *>(st + (size_t)rank * SB)[q] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t *>(src_of(rank)) + q);
        }
        return;
    }

    // straight to the output: getSlotData (blocks 1..127 in place, 16129 dwords) and block 0
#if FB_PACKED && FB_ROWS
    if (FB_PAST_ROW(s, k)) return;
#endif
    unsigned *out = reinterpret_cast<unsigned *>(FB_STREAM_OUT(s) + (size_t)k * PAYLOAD);
    for (int j = t; j < 127 * 127; j += SC_NT) {
        const int b = 1 + j / 127, w = j % 127;
        const int win = s_win[b];
        out[j] = win >= 0 ? reinterpret_cast<const unsigned *>(src_of(win) + 4)[w] : 0u;
    }
    if (a.block0_out && t < 127) {
        unsigned *o0 = reinterpret_cast<unsigned *>(a.block0_out + ((size_t)s * a.max_frames + k) * 508);
        o0[t] = s_win[0] >= 0 ? reinterpret_cast<const unsigned *>(src_of(s_win[0]) + 4)[t] : 0u;
    }
}

#if FB_PACKED && FB_ROWS
__global__ __launch_bounds__(SC_NT) void fecbuf_copy_guarded_rows_kernel(FecBufArgs a, const unsigned *row_off)
#elif FB_PACKED
__global__ __launch_bounds__(SC_NT) void fecbuf_copy_guarded_kernel(FecBufArgs a)
#elif FB_ROWS
__global__ __launch_bounds__(SC_NT) void fecbuf_copy_rows_kernel(FecBufArgs a, const unsigned *row_off)
#else
__global__ __launch_bounds__(SC_NT) void fecbuf_copy_kernel(FecBufArgs a)
#endif
{
    const int slot = (int)blockIdx.x;
    const int s = a.dmap[2 * slot], k = a.dmap[2 * slot + 1];
#if FB_PACKED
    if (s < 0 || s >= a.nstreams || k < 0 || k >= a.max_frames) return;
#endif
#if FB_PACKED && FB_ROWS
    if (FB_PAST_ROW(s, k)) return;
#endif
    copy_dwords(reinterpret_cast<unsigned *>(FB_STREAM_OUT(s) + (size_t)k * PAYLOAD),
                reinterpret_cast<const unsigned *>(a.dec_out + (size_t)slot * PAYLOAD), 127 * 127);
    if (a.block0_out && threadIdx.x < 127)
        reinterpret_cast<unsigned *>(a.block0_out + ((size_t)s * a.max_frames + k) * 508)[threadIdx.x] =
            reinterpret_cast<const unsigned *>(a.dec_b0 + (size_t)slot * 508)[threadIdx.x];
}

#undef FB_STREAM_DG
#undef FB_STREAM_OUT
#undef FB_PAST_ROW
#undef FB_ROWS
