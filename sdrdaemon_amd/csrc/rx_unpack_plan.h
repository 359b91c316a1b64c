// rx_unpack_plan.h -- the table of the unpack kernels (rx_unpack_body.h): a batch of sample-fed blocks -> the rows and segments the
// kernel walks.  One table serves K0p (rx_async_kernels.hip: every stream in the bank's format, fmt == NULL below) and K0x
// (rx_unpack_mixed_kernels.hip: each stream in its own, sdrhip_rx_set_stream_format).  A segment is the samples of one (block, stream) with a
// non-zero count; its source is counted in 2-BYTE UNITS from the start of the upload (an 8-bit sample is one unit, an int16 sample
// two), so that an int16 row behind an odd number of 8-bit samples starts at an odd unit: 2 bytes off a dword boundary.  The table
// lists the segments stream by stream, block order inside: a stream's segments tile its row from sample 0 on.  Pure host arithmetic
// (C++11, standard headers only): rx_launch_ragged and rx_ragged ask it, tests/cxx/rx_unpack_plan_test.cpp replays it on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdrhip {
constexpr unsigned UNPACKX_WG_SAMPLES = 4096; // row samples per workgroup (256 lanes x 16 B of int16 output x 4)
constexpr int UNPACKX_S16 = 0, UNPACKX_U8 = 1, UNPACKX_S8 = 2; // (= SDRHIP_IQ_* of include/sdrhip.h)

struct UnpackXSeg {
    uint64_t src; // first sample of the segment: 2-byte units from the start of the source
    uint32_t dst; // its first sample in the stream's row
    uint32_t n;   // samples
};
struct UnpackXRow {      // one per stream, then one sentinel row (wg0 = the grid)
    uint32_t seg0, nseg; // the stream's segments in the table
    uint32_t wg0;        // its first workgroup: stream s has ceil(total / UNPACKX_WG_SAMPLES) of them (none for an empty row)
    uint32_t total;      // samples of the row
    uint32_t fmt;        // the stream's format (K0x reads it; K0p has the bank's as a template argument)
    uint32_t unused[3];
};

inline bool unpackx_format_ok(int fmt) { return fmt == UNPACKX_S16 || fmt == UNPACKX_U8 || fmt == UNPACKX_S8; }
inline size_t unpackx_sample_bytes(int fmt) { return fmt == UNPACKX_S16 ? 4 : 2; }

struct UnpackXPlan {
    uint64_t nseg;  // segments of the table
    uint64_t bytes; // sample bytes of a packed source: sum n * bytes(fmt)
    uint64_t grid;  // workgroups
    bool fits;      // every 32-bit field of the table holds its value and the grid is one launch
};

// what the table of these counts needs; cnt = nblk x S counts, block-major and stream-minor; fmt = S formats, or NULL: every stream
// has bank_fmt (which is not looked at while an array is given).  Nothing is written
inline UnpackXPlan unpackx_measure(const size_t *cnt, size_t nblk, size_t S, const int *fmt, int bank_fmt = UNPACKX_S16)
{
    UnpackXPlan p = {0, 0, 0, true};
    for (size_t s = 0; s < S; ++s) {
        const size_t bytes = unpackx_sample_bytes(fmt ? fmt[s] : bank_fmt);
        uint64_t total = 0;
        for (size_t b = 0; b < nblk; ++b) {
            const uint64_t n = cnt[b * S + s];
            if (!n) continue;
            if (n > 0xffffffffu || total + n < total) p.fits = false;
            total += n;
            p.bytes += n * bytes;
            ++p.nseg;
        }
        if (total > (uint64_t)0xffffffffu - UNPACKX_WG_SAMPLES) p.fits = false;
        p.grid += (total + UNPACKX_WG_SAMPLES - 1) / UNPACKX_WG_SAMPLES;
    }
    if (p.grid > 0x7fffffffu || p.nseg > 0xffffffffu || S > 0x7fffffffu) p.fits = false;
    return p;
}

// the table.  rows: S + 1 entries, segs: unpackx_measure().nseg entries.  stride_units = 0: the source is packed, block after
// block, stream after stream inside a block, each row n * bytes(fmt) long.  stride_units != 0 (one block): the source is strided
// rows, row s at 2-byte unit s * stride_units whatever its format.  fmt == NULL: every stream has bank_fmt, as in unpackx_measure.
// Returns the measure; writes nothing when it does not fit
inline UnpackXPlan unpackx_fill(const size_t *cnt, size_t nblk, size_t S, const int *fmt, uint64_t stride_units, UnpackXRow *rows, UnpackXSeg *segs,
                                int bank_fmt = UNPACKX_S16)
{
    const UnpackXPlan p = unpackx_measure(cnt, nblk, S, fmt, bank_fmt);
    if (!p.fits || (stride_units && nblk != 1)) {
        UnpackXPlan bad = p;
        bad.fits = false;
        return bad;
    }
    // (stream-major table from a block-major walk: a row's nseg and total serve as its cursors on the way)
    uint32_t k = 0;
    for (size_t s = 0; s < S; ++s) {
        UnpackXRow &r = rows[s];
        r.seg0 = k; r.nseg = 0; r.wg0 = 0; r.total = 0; r.fmt = (uint32_t)(fmt ? fmt[s] : bank_fmt);
        r.unused[0] = r.unused[1] = r.unused[2] = 0;
        for (size_t b = 0; b < nblk; ++b) k += cnt[b * S + s] ? 1 : 0;
    }
    uint64_t at = 0; // 2-byte units of the packed source in front of the segment
    for (size_t b = 0; b < nblk; ++b)
        for (size_t s = 0; s < S; ++s) {
            const size_t n = cnt[b * S + s];
            if (!n) continue;
            UnpackXRow &r = rows[s];
            UnpackXSeg &g = segs[r.seg0 + r.nseg++];
            g.src = stride_units ? (uint64_t)s * stride_units : at;
            g.dst = r.total;
            g.n = (uint32_t)n;
            r.total += (uint32_t)n;
            at += (uint64_t)n * (unpackx_sample_bytes((int)r.fmt) / 2);
        }
    uint64_t wg = 0;
    for (size_t s = 0; s < S; ++s) {
        rows[s].wg0 = (uint32_t)wg;
        wg += ((uint64_t)rows[s].total + UNPACKX_WG_SAMPLES - 1) / UNPACKX_WG_SAMPLES;
    }
    UnpackXRow &e = rows[S];
    e.seg0 = k; e.nseg = 0; e.wg0 = (uint32_t)wg; e.total = 0; e.fmt = 0;
    e.unused[0] = e.unused[1] = e.unused[2] = 0;
    return p;
}
} // namespace sdrhip
