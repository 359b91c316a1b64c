// rx_unpack_body.h -- the Rx pipe's input pass as device code: incoming samples -> the [stream][stride] int16 rows the decimators read.
// Shared by K0 (convert_kernels.hip), K0r (rx_ragged_kernels.hip), K0p (rx_async_kernels.hip) and K0x, the per-stream-format kernel;
// include it inside namespace sdrhip's anonymous namespace, behind sdrhip_internal.h.  Three pieces:
//  * iq8_widen2: the byte-to-int16 rule.  RtlSdrSource's IQSample(buf[2i] - 128, buf[2i + 1] - 128) (RtlSdrSource.cpp:542-553) and
//    HackRFSource's IQSample(buf[2i], buf[2i + 1]) (HackRFSource.cpp:661-674); offset binary is two's complement with the top bit
//    flipped, b - 128 = (int8)(b ^ 0x80), so U8 is S8 behind one XOR per dword.
//  * iq8_widen_row (K0, K0r): one 8-bit row of n samples.  A lane takes 8 samples, one 16-byte load and two 16-byte stores; the row's
//    last n % 8 samples go sample by sample, so no lane reads or writes past the row's n samples.
//  * unpack_body (K0p, K0x): one workgroup's part of a row that a table of segments (rx_unpack_plan.h) describes.  Every lane writes
//    16-byte-aligned chunks of its row (4 int16 samples, or 8 widened 8-bit samples as two 16-byte stores), so no two lanes share a
//    chunk; a chunk that lies wholly in one segment is read with one 16-byte load, one that straddles segments or the row's end is
//    assembled per sample.  ODD: a segment may start at an odd 2-byte unit -- an 8-bit segment behind an odd count, an int16 one
//    behind an odd number of 8-bit samples.  Its chunks are read as the dwords around them and realigned by 2 bytes: the 2 bytes in
//    front of the chunk (inside the source: the unit is odd, so at least 1) and 2 behind it (inside a packed source's 64-byte pad at
//    the very end).  Without ODD the realignment and the two-halves load of an int16 sample compile out.  Strided rows start on 16
//    bytes, so no chunk of theirs is realigned, and the per-sample path reads a sample's own bytes alone.  No scratch, no LDS.

typedef unsigned rxu_uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned rxu_uint4a4_t __attribute__((ext_vector_type(4), aligned(4))); // 16-byte load from a dword-aligned address

// two samples {re, im, re, im} of one dword -> two IQSample dwords
template <int FMT> __device__ __forceinline__ void iq8_widen2(unsigned x, unsigned &lo, unsigned &hi)
{
    if (FMT == IQF_U8) x ^= 0x80808080u;
    const int b0 = (int)(x << 24) >> 24, b1 = (int)(x << 16) >> 24, b2 = (int)(x << 8) >> 24, b3 = (int)x >> 24;
    lo = ((unsigned)b0 & 0xffffu) | ((unsigned)b1 << 16);
    hi = ((unsigned)b2 & 0xffffu) | ((unsigned)b3 << 16);
}

// n samples of one 8-bit row (16-byte aligned, as orow is) by the workgroups of blockIdx.y's row, 256 lanes each
template <int FMT> __device__ __forceinline__ void iq8_widen_row(const uint8_t *row, unsigned *orow, size_t n)
{
    const size_t groups = n >> 3;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const rxu_uint4_t v = SDRHIP_STREAM_LOAD(reinterpret_cast<const rxu_uint4_t *>(row) + g);
        unsigned w[8];
        iq8_widen2<FMT>(v.x, w[0], w[1]);
        iq8_widen2<FMT>(v.y, w[2], w[3]);
        iq8_widen2<FMT>(v.z, w[4], w[5]);
        iq8_widen2<FMT>(v.w, w[6], w[7]);
        rxu_uint4_t *o = reinterpret_cast<rxu_uint4_t *>(orow + 8 * g);
        o[0] = (rxu_uint4_t){w[0], w[1], w[2], w[3]};
        o[1] = (rxu_uint4_t){w[4], w[5], w[6], w[7]};
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const size_t i = (groups << 3) + threadIdx.x;
        const unsigned x = (unsigned)row[2 * i] | ((unsigned)row[2 * i + 1] << 8);
        unsigned lo, hi;
        iq8_widen2<FMT>(x, lo, hi);
        orow[i] = lo;
    }
}

// the sample at 2-byte unit u as an int16 IQ dword (ODD: an int16 sample may sit 2 bytes off a dword, two 2-byte loads)
template <int FMT, bool ODD> __device__ __forceinline__ unsigned unpack_sample(const uint16_t *src, uint64_t u)
{
    if (FMT == IQF_S16) return ODD ? (unsigned)src[u] | ((unsigned)src[u + 1] << 16) : *reinterpret_cast<const unsigned *>(src + u);
    unsigned lo, hi;
    iq8_widen2<FMT>((unsigned)src[u], lo, hi);
    return lo;
}

// the last segment of [lo, hi] that starts at or before row sample x
__device__ __forceinline__ int unpack_find_seg(const UnpackXSeg *segs, int lo, int hi, uint32_t x)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].dst <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the stream that workgroup b serves: the last row whose first workgroup is at or below b (blockIdx alone decides it)
__device__ __forceinline__ int unpack_find_row(const UnpackXRow *rows, int nstreams, uint32_t b)
{
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].wg0 <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// one workgroup's part [d0, d1) of a row of format FMT: sg = the row's nseg segments, total its samples
template <int FMT, bool ODD> __device__ __forceinline__ void unpack_body(const uint16_t *src, unsigned *orow, const UnpackXSeg *sg, int nseg, uint32_t total,
                                                                         uint32_t d0, uint32_t d1)
{
    constexpr uint32_t SPC = FMT == IQF_S16 ? 4 : 8; // row samples per lane and chunk
    constexpr uint32_t UPS = FMT == IQF_S16 ? 2 : 1; // 2-byte units per sample
    const int k0 = unpack_find_seg(sg, 0, nseg - 1, d0), k1 = unpack_find_seg(sg, k0, nseg - 1, d1 - 1);
    for (uint32_t c = d0 + threadIdx.x * SPC; c < d1; c += 256 * SPC) {
        int k = unpack_find_seg(sg, k0, k1, c);
        const UnpackXSeg g = sg[k];
        unsigned w[SPC];
        if (c + SPC <= g.dst + g.n) { // the chunk lies in one segment: one 16-byte load
            const uint64_t u = g.src + (uint64_t)(c - g.dst) * UPS;
            unsigned x[4];
            if (!ODD || (u & 1) == 0) {
                const rxu_uint4a4_t v = *reinterpret_cast<const rxu_uint4a4_t *>(src + u);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else { // (odd unit: the dwords around the chunk, realigned by 2 bytes)
                const uint16_t *p = src + u - 1;
                const rxu_uint4a4_t v = *reinterpret_cast<const rxu_uint4a4_t *>(p);
                const unsigned e = reinterpret_cast<const unsigned *>(p)[4];
                x[0] = __builtin_amdgcn_alignbit(v.y, v.x, 16);
                x[1] = __builtin_amdgcn_alignbit(v.z, v.y, 16);
                x[2] = __builtin_amdgcn_alignbit(v.w, v.z, 16);
                x[3] = __builtin_amdgcn_alignbit(e, v.w, 16);
            }
            if constexpr (FMT == IQF_S16) {
                w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) iq8_widen2<FMT>(x[j], w[2 * j], w[2 * j + 1]);
            }
        } else { // the chunk straddles segments or the row's end: sample by sample
#pragma unroll
            for (uint32_t j = 0; j < SPC; ++j) {
                const uint32_t i = c + j;
                w[j] = 0;
                if (i >= total) continue;
                while (sg[k].dst + sg[k].n <= i) ++k;
                w[j] = unpack_sample<FMT, ODD>(src, sg[k].src + (uint64_t)(i - sg[k].dst) * UPS);
            }
        }
        rxu_uint4_t *o = reinterpret_cast<rxu_uint4_t *>(orow + c);
        o[0] = (rxu_uint4_t){w[0], w[1], w[2], w[3]};
        if constexpr (SPC == 8) o[1] = (rxu_uint4_t){w[4], w[5], w[6], w[7]};
    }
}
