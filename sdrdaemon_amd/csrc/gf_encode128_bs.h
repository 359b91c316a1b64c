// gf_encode128_bs.h -- the additive-FFT encoder of gf_encode128_fft.h with its middle stages bit-sliced (context option
// enc_form = bitslice).  Include inside namespace sdrhip { namespace { ... } } behind gf_encode128_fft.h (its tables, exchange
// layout, fft_* helpers).
//
// Same bytes, same mapping (a lane owns one 4-byte column of 64 blocks, a workgroup is one frame in four waves = column half x
// block half), same network.  What changes is how a constant multiplication a ^= c * b is done where it can be done for eight
// blocks at once.  In the table form it is ~10 VALU per 4 bytes (selector extraction, three v_perm_b32, xor3 / xor) plus an LDS
// record per block.  A multiplication by a FIXED c is an 8 x 8 matrix over GF(2): with the bytes stored as bit planes (plane p = bit
// p of 32 bytes) it is a fixed XOR tree, sum over p of ceil(weight of row p / 2) v_xor3 / v_bitop3, ~18 for 32 bytes.
//
// Which stages can be bit-sliced in this mapping: a lane's 64 values are eight OCTETS of blocks (8m .. 8m + 7).  Transposing an octet
// -- 8 dwords = 4 bytes of 8 blocks -- gives 8 planes of 32 bits, and every bit of a plane then belongs to a different block of the
// octet.  A butterfly of stage k has one constant that depends on the block-index bits above k: for k >= 3 the octet's eight blocks
// share it and the butterfly pairs whole octets, so the plane form applies; stages 0..2 pair blocks INSIDE an octet with per-block
// constants and stay in the table form.  So, per wave:
//   1. inverse stages 0..2 per octet (table form, 7 blocks per octet), then the octet's bit transpose;
//   2. inverse stages 3..5 and the t5 fold on planes (compile-time XOR trees);
//   3. the exchange of gf_encode128_fft.h (t6, first stage of the size-32 transform) on planes -- the exchange area holds planes now;
//   4. the size-16 transform's first stage (stage 3) on planes, transpose back, stages 2..0 and the row scales in the table form.
// 16 + 6 + 1 plane multiplications (block half 1; block half 0: 9 + 0 + 1) replace 184 (80) table ones per column: 12.56 M -> 10.30 M
// VALU wave-instructions, 37.1 -> 31.6 us per 1040 frames (profiles/bs_enc_form_ab.txt).
// tools/bs_ledger.py counts the compiled loop; tests/test_bitslice_encoder_model.py is this network in numpy.
#pragma once

// ---- GF(256) at compile time: the field of gf256.h (polynomial 0x14D) and the constants of cm256_fft_tables
__host__ __device__ constexpr unsigned bs_gmul(unsigned a, unsigned b)
{
    unsigned r = 0u;
    for (int i = 0; i < 8; ++i) {
        if (b >> i & 1u) r ^= a;
        a <<= 1;
        if (a & 0x100u) a ^= 0x14Du;
    }
    return r;
}
__host__ __device__ constexpr unsigned bs_ginv(unsigned a)
{
    unsigned r = 1u; // a^254
    for (int i = 0; i < 254; ++i) r = bs_gmul(r, a);
    return r;
}
// subspace polynomial of V_k = {0 .. 2^k - 1}: s_0(x) = x, s_{k+1}(x) = s_k(x) (s_k(x) ^ s_k(2^k)); s^_k = s_k / s_k(2^k)
__host__ __device__ constexpr unsigned bs_s(int k, unsigned x)
{
    unsigned v = x;
    for (int i = 0; i < k; ++i) v = bs_gmul(v, v ^ bs_s(i, 1u << i)); // (recursion on i < k only: depth 8 at most)
    return v;
}
__host__ __device__ constexpr unsigned bs_shat(int k, unsigned x) { return bs_gmul(bs_s(k, x), bs_ginv(bs_s(k, 1u << k))); }

// row p of the GF(2) matrix of "multiply by c": bit q set when bit p of c * 2^q is
struct BsMat { unsigned char row[8]; };
__host__ __device__ constexpr BsMat bs_mat(unsigned c)
{
    BsMat m{};
    for (int q = 0; q < 8; ++q) {
        const unsigned col = bs_gmul(c, 1u << q);
        for (int p = 0; p < 8; ++p)
            if (col >> p & 1u) m.row[p] = (unsigned char)(m.row[p] | (1u << q));
    }
    return m;
}

// the set bits of a matrix row, in order
struct BsTerms { int n; int q[8]; };
__host__ __device__ constexpr BsTerms bs_terms(unsigned row)
{
    BsTerms t{};
    for (int q = 0; q < 8; ++q)
        if (row >> q & 1u) t.q[t.n++] = q;
    return t;
}

// a ^= c * b on 8 planes: one XOR tree per output plane
template <unsigned C> __device__ __forceinline__ void bs_muladd(unsigned *a, const unsigned *b)
{
    if constexpr (C != 0u) {
        fft_for<8>([&](auto pc) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            constexpr unsigned row = bs_mat(C).row[p];
            // the row's terms two at a time into v_bitop3 (xor3); left to itself the compiler keeps most of the chain in v_xor_b32
            constexpr BsTerms T = bs_terms(row);
            unsigned acc = a[p];
            fft_for<T.n / 2>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value;
                acc = x3(acc, b[T.q[2 * i]], b[T.q[2 * i + 1]]);
            });
            if constexpr (T.n & 1) acc ^= b[T.q[T.n - 1]];
            asm volatile("" : "+v"(acc)); // (one plane after the other: the trees of a block are not interleaved, nor hoisted)
            a[p] = acc;
        });
    }
}
// b ^= a on 8 planes
__device__ __forceinline__ void bs_xor8(unsigned *b, const unsigned *a)
{
    fft_for<8>([&](auto pc) __attribute__((always_inline)) { b[decltype(pc)::value] ^= a[decltype(pc)::value]; });
}

// 8 dwords <-> 8 planes: for every byte position B the 8 x 8 bit matrix (dword t, bit p) is transposed to (plane p, bit t), three
// delta-swap stages of v_bfi_b32 and two shifts per register pair.  An involution: the same call transposes back.
__device__ __forceinline__ void bs_transpose8(unsigned *x)
{
    fft_for<3>([&](auto sc) __attribute__((always_inline)) {
        constexpr int j = 4 >> decltype(sc)::value;
        constexpr unsigned m = j == 4 ? 0x0F0F0F0Fu : j == 2 ? 0x33333333u : 0x55555555u;
        fft_for<8>([&](auto tc) __attribute__((always_inline)) {
            constexpr int t = decltype(tc)::value;
            if constexpr ((t & j) == 0) {
                const unsigned a = x[t], b = x[t + j];
                unsigned lo = (a & m) | ((b << j) & ~m), hi = ((a >> j) & m) | (b & ~m);
                asm volatile("" : "+v"(lo), "+v"(hi));
                x[t] = lo;
                x[t + j] = hi;
            }
        });
    });
}

// inverse stages 0..2 of octet M in the table form: block j of stage k (k < 3) sits in the octet, table 63 hf + 64 - (64 >> k) + j.
// Blocks in order n = 0..6: stage 0 (four), stage 1 (two), stage 2 (one); the next block's table is on its way while one is applied.
template <int HF, int M> __device__ __forceinline__ void bs_inv_octet(unsigned (&d)[64], FftTabs &R, unsigned lh)
{
    fft_for<7>([&](auto nc) __attribute__((always_inline)) {
        constexpr int n = decltype(nc)::value, g = M * 7 + n, P = g & 1;
        constexpr int k = n < 4 ? 0 : n < 6 ? 1 : 2, jj = n < 4 ? n : n < 6 ? n - 4 : 0;
        constexpr int j = M * (4 >> k) + jj, h = 1 << k, blk = j * 2 * h;
        fft_wait<P>(R);
        if constexpr (g + 1 < 56) {
            constexpr int n1 = (g + 1) % 7, m1 = (g + 1) / 7;
            constexpr int k1 = n1 < 4 ? 0 : n1 < 6 ? 1 : 2, jj1 = n1 < 4 ? n1 : n1 < 6 ? n1 - 4 : 0;
            fft_issue<P ^ 1, 64 - (64 >> k1) + m1 * (4 >> k1) + jj1>(R, lh);
        }
#pragma unroll
        for (int i = 0; i < h; ++i) d[blk + h + i] ^= d[blk + i];
        if constexpr (j != 0 || HF != 0) { // (the leading block of every stage of the first half: constant 0)
#pragma unroll
            for (int i = 0; i < h; ++i) fft_muladd<P>(d[blk + i], d[blk + h + i], R);
        }
    });
    bs_transpose8(&d[8 * M]);
}

// inverse stages 3..5 on planes (octet o of the wave = d[8 o .. 8 o + 7]) and the t5 fold: octets 0..3 hold the half's 32
// coefficients on 128 + V5 afterwards (as planes)
template <int HF> __device__ __forceinline__ void bs_inverse_high(unsigned (&d)[64])
{
    fft_for<3>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = 3 + decltype(kc)::value, ho = 1 << (k - 3); // octets per butterfly side
        fft_for<(32 >> k)>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            constexpr unsigned c = bs_shat(k, (64u * HF) ^ ((unsigned)j << (k + 1)));
            fft_for<ho>([&](auto ic) __attribute__((always_inline)) {
                constexpr int lo = 8 * (2 * j * ho + decltype(ic)::value), hi = lo + 8 * ho;
                bs_xor8(&d[hi], &d[lo]);
                bs_muladd<c>(&d[lo], &d[hi]);
            });
        });
    });
    constexpr unsigned t5 = bs_shat(5, 128u);
    fft_for<4>([&](auto oc) __attribute__((always_inline)) { constexpr int o = decltype(oc)::value; bs_muladd<t5>(&d[8 * o], &d[8 * (o + 4)]); });
}

template <int HF> __device__ __forceinline__ void gf_encode128_bs_wave(const Enc128Args &a, int fi, unsigned char *ldsraw, int ch, int xslot)
{
    constexpr int hf = HF;
    const unsigned la = lds_addr(ldsraw);
    const int lane = (int)fft_lane();
    const int fr = a.gen_done > 0 ? (fi / a.gen_done) * a.gen_cap + fi % a.gen_done : (a.frame_list ? __builtin_amdgcn_readfirstlane(a.frame_list[fi]) : fi);
    if (fr < 0 || fr >= a.nframes) return; // (workgroup-uniform: all four waves leave in front of the barriers below)
    const int col = ch * 64 + lane;
    const bool live = col < 127;
    const unsigned lc = live ? (unsigned)col : 126u;
    // input handling: gf_encode128_fft_wave's, statement for statement (frame list, meta block, fused framing copy, straddle)
    const unsigned *fbase = reinterpret_cast<const unsigned *>(a.in + (size_t)fr * a.in_frame_bytes) + 1;
    unsigned *obase = reinterpret_cast<unsigned *>(a.out + (size_t)fr * a.out_frame_bytes) + 1;
    const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(fbase), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(obase, 0, 0x7fffffff, 0x00020000);
    const unsigned lc4 = 4u * lc;
    unsigned hdr0 = 0u, blk0 = 0u;
    bool own0 = false;
    if (a.meta_count > 0 && a.gen_done > 0) {
        const int f = fr % a.gen_cap, mi = f - a.meta_first;
        if (mi >= 0 && mi < a.meta_count) {
            unsigned w[6], base[6], rate;
            stream_meta_base(a.meta_w, a.meta_rate, a.meta_tab, fr / a.gen_cap, base, rate);
            frame_meta_words(base, a.meta_idx0, rate, mi, w);
            own0 = true;
            hdr0 = (a.meta_frame_count0 + (unsigned)mi) & 0xffffu;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (col == k) blk0 = w[k];
        }
    }
    if (!own0) hdr0 = fbase[-1];
    bool fused = false, strad = false;
    const unsigned *lbase = fbase, *sbase = fbase;
    if (a.lin) {
        const int s = fr / a.lin_cap, f = fr - s * a.lin_cap;
        if (f >= a.lin_first) {
            fused = true;
            lbase = a.lin + (size_t)s * a.lin_stride + ((size_t)f * 16129u - (size_t)a.lin_pending) - 127;
        } else if (a.lin_straddle && f == 0) {
            strad = true;
            sbase = a.lin + (size_t)s * a.lin_stride;
        }
    }
    unsigned *const xch0 = reinterpret_cast<unsigned *>(ldsraw + FFT_TAB_BYTES) + xslot * FFT_XCH_DWORDS;

    unsigned d[64];
    const int b0 = 64 * hf;
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(lbase), 0, 0x7fffffff, 0x00020000);
    const int pitch = fused ? 508 : 512;
    {
        const unsigned v0 = __builtin_amdgcn_raw_buffer_load_b32(rf, lc4, 0, 0);
        const unsigned vb = __builtin_amdgcn_raw_buffer_load_b32(rl, lc4, (hf ? b0 : 1) * pitch, 0);
        d[0] = hf ? vb : (own0 ? blk0 : v0);
    }
#pragma unroll
    for (int i = 1; i < 64; ++i) d[i] = __builtin_amdgcn_raw_buffer_load_b32(rl, lc4, (b0 + i) * pitch, ENC_LOAD_AUX);
    if (strad) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(sbase), 0, 0x7fffffff, 0x00020000);
        // (eight blocks at a time: sixteen, as gf_encode128_fft_wave does, spill here)
        fft_for<8>([&](auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            unsigned vl[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int w = (b0 + 8 * g + i - 1) * 127 - a.lin_pending + (int)lc;
                vl[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, w < 0 ? 0u : 4u * (unsigned)w, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int b = b0 + 8 * g + i, w = (b - 1) * 127 - a.lin_pending + (int)lc;
                d[8 * g + i] = (b != 0 && w >= 0) ? vl[i] : d[8 * g + i];
            }
            asm volatile("" ::: "memory");
        });
    }
    if ((fused || strad) && live) {
#pragma unroll
        for (int i = 0; i < 64; ++i) __builtin_amdgcn_raw_buffer_store_b32(d[i], rf, lc4, (b0 + i) * 512, 0);
    }
    // parity of the 64 values, parked in LDS for the row loop (one long-lived register less)
    {
        unsigned par = 0u;
#pragma unroll
        for (int i = 0; i < 64; i += 2) par = x3(par, d[i], d[i + 1]);
        (xch0 + fft_lane())[(32 + hf) * 64] = par;
    }

    // 1. inverse stages 0..2 per octet, table form; each octet to planes behind them
    {
        FftTabs R;
        const unsigned lh = la + (unsigned)(hf * 63 * 32);
        fft_issue<0, 0>(R, lh);
        fft_for<8>([&](auto mc) __attribute__((always_inline)) {
            bs_inv_octet<HF, decltype(mc)::value>(d, R, lh);
        });
    }
    // 2. stages 3..5 and the t5 fold on planes
    bs_inverse_high<HF>(d);
    // 3. the exchange (gf_encode128_fft.h: fft_rows16) on planes: the hf = 0 wave's 4 octets down, t6 and stage 4 in the hf = 1
    // wave, octets 0..1 (rows 0..15) back.  Plane p of octet o is exchange slot 8 o + p.
    unsigned e[16];
    unsigned *const xch = xch0 + fft_lane();
    if constexpr (hf == 0) {
#pragma unroll
        for (int i = 0; i < 32; ++i) xch[i * 64] = d[i];
    }
    __syncthreads();
    if constexpr (hf != 0) {
        constexpr unsigned t6 = bs_shat(6, 128u), s4 = bs_shat(4, 128u);
        fft_for<2>([&](auto oc) __attribute__((always_inline)) {
            constexpr int o = decltype(oc)::value;
            unsigned va[8], vb[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) { va[p] = xch[(8 * o + p) * 64]; vb[p] = xch[(8 * (o + 2) + p) * 64]; }
            bs_xor8(&d[8 * o], va);
            bs_muladd<t6>(va, &d[8 * o]);
            bs_xor8(&d[8 * (o + 2)], vb);
            bs_muladd<t6>(vb, &d[8 * (o + 2)]);
            bs_muladd<s4>(va, vb);
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                e[8 * o + p] = vb[p] ^ va[p];
                xch[(8 * o + p) * 64] = va[p];
            }
        });
    }
    __syncthreads();
    if constexpr (hf == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i] = xch[i * 64];
    }
    // 4. stage 3 of the size-32 transform (one block per wave: rows 16 hf .. 16 hf + 15) on planes, back to bytes, stages 2..0 and
    // the row scales in the table form (fft_forward16's blocks n = 1..14)
    {
        constexpr unsigned c3 = bs_shat(3, 128u ^ ((unsigned)hf << 4));
        bs_muladd<c3>(&e[0], &e[8]);
        bs_xor8(&e[8], &e[0]);
        bs_transpose8(&e[0]);
        bs_transpose8(&e[8]);
        FftTabs R;
        auto base = [&](int k) { return la + (unsigned)hf * (unsigned)((8 >> k) * 32); };
        fft_issue<1, 128 + 32 - 8>(R, base(2));
        fft_for<14>([&](auto nc) __attribute__((always_inline)) {
            constexpr int n = decltype(nc)::value + 1;
            constexpr int k = n < 3 ? 2 : n < 7 ? 1 : 0;
            constexpr int j = n - ((8 >> k) - 1);
            constexpr int h = 1 << k, blk = j * 2 * h, P = n & 1;
            fft_wait<P>(R);
            if constexpr (n + 1 < 15) {
                constexpr int n1 = n + 1, k1 = n1 < 3 ? 2 : n1 < 7 ? 1 : 0, j1 = n1 - ((8 >> k1) - 1);
                fft_issue<P ^ 1, 128 + 32 - (32 >> k1) + j1>(R, base(k1));
            }
#pragma unroll
            for (int i = 0; i < h; ++i) {
                fft_muladd<P>(e[blk + i], e[blk + h + i], R);
                e[blk + h + i] ^= e[blk + i];
            }
        });
    }
    // rows 16 hf + i: gf_encode128_fft_wave's tail
    {
        FftTabs R;
        const unsigned ln = fft_lane(), col = (unsigned)ch * 64u + ln;
        const bool live = col < 127u;
        const unsigned lc = live ? col : 126u, lc4 = 4u * lc;
        const unsigned par = (xch0 + ln)[32 * 64] ^ (xch0 + ln)[33 * 64];
        const unsigned lk = la + (unsigned)hf * 512u;
        fft_issue<0, 160>(R, lk);
        fft_for<16>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value, P = i & 1;
            fft_wait<P>(R);
            if constexpr (i + 1 < 16) fft_issue<P ^ 1, 160 + i + 1>(R, lk);
            const int r = 16 * hf + i;
            if (r < a.rows && live) {
                unsigned v = par;
                fft_muladd<P>(v, e[i], R);
                __builtin_amdgcn_raw_buffer_store_b32(v, ro, lc4, r * 512, 0);
                if (col == 0) (obase + (size_t)r * 128)[-1] = (hdr0 & 0xffffu) | ((unsigned)(128 + r) << 16);
            }
        });
    }
}

__device__ __forceinline__ void gf_encode128_bs_wg(const Enc128Args &a, int fi, unsigned char *ldsraw)
{
    fft_fill_tables(a, ldsraw);
    fec_stagger_sleep(fi, a.stagger, a.stagger_div);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wv >> 1) gf_encode128_bs_wave<1>(a, fi, ldsraw, wv & 1, wv & 1);
    else gf_encode128_bs_wave<0>(a, fi, ldsraw, wv & 1, wv & 1);
}
