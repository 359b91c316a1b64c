// rx_records_body.h -- the records half of the departure-order delivery kernels KR and KP as device code shared by both: the
// collector's public records of a datagram batch lie [stream][kmax], stream s released cnt of them; record k of stream s goes to
// out + rec.dst + 16 (pre + k), {pre, cnt} per stream (one 16-byte entry) from the host's own counts.  One workgroup takes NT x PER
// record slots; slot i = record i % kmax of stream i / kmax.  The record loads do not wait for the places.
// Include inside namespace sdrhip { namespace { ... } }.
#pragma once
template <int NT, int PER> __device__ __forceinline__ void deliver_records_wg(unsigned wg, const RxEgressRecords &rec, uint8_t *out)
{
    typedef unsigned rec_uint4_t __attribute__((ext_vector_type(4)));
    const unsigned i0 = wg * (unsigned)(NT * PER) + threadIdx.x;
    const rec_uint4_t *recs = reinterpret_cast<const rec_uint4_t *>(rec.records);
    unsigned rk[PER];
    rec_uint4_t v[PER], p[PER]; // p = {pre, cnt, -, -} of the slot's stream
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const unsigned i = i0 + j * NT < rec.nslots ? i0 + j * NT : rec.nslots - 1;
        const unsigned s = i / rec.kmax;
        rk[j] = i - s * rec.kmax;
        v[j] = __builtin_nontemporal_load(recs + i);
        p[j] = reinterpret_cast<const rec_uint4_t *>(rec.place)[s];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) asm volatile("" : "+v"(v[j]), "+v"(p[j]));
    rec_uint4_t *rdst = reinterpret_cast<rec_uint4_t *>(out + rec.dst);
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (i0 + j * NT < rec.nslots && rk[j] < p[j].y) rdst[(uint64_t)p[j].x + rk[j]] = v[j];
}
