// rx_follow_bits_rule_test.cpp -- the rule of sdrhip_rx_set_follow_bits on a CPU: the arithmetic KFb runs (rx_stream_settings.h:
// followed_size_words and what it calls, one text for host and device) for every log2decim 0..6 and every value 0..255 of the
// incoming sampleBits byte.  The program checks what it can check alone -- which bytes are admitted, that only byte 1 of the
// incoming word is read, that the merge keeps bytes 2 and 3 of the row's word, that nothing is written for a byte that is not
// admitted, and the CRC restatement against rx_meta_record -- and prints one line per case for tests/test_rx_follow_bits_rule.py,
// which holds the pair and the decimated size against the decimators themselves.
#include "rx_stream_settings.h"

#include <cstdio>
#include <cstdlib>

using namespace sdrhip;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);                     \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

int main()
{
    // rows as the host forms them: frequency, rate, fecblk and the host's own size vary with the case
    const uint32_t fcs[4] = {435000u, 3000000000u, 4294967295u, 0u};
    const uint32_t rates[4] = {625000u, 48000u, 1u, 0u};
    const int fecs[4] = {32, 0, 128, 7};
    unsigned long admitted = 0, refused = 0, crcs = 0;
    for (unsigned L = 0; L <= 6; ++L) {
        for (unsigned byte = 0; byte <= 255; ++byte) {
            const unsigned k = (L * 256 + byte) & 3, host_bits = 1 + (L * 5 + byte) % 16;
            const uint32_t fc = fcs[k], rate = rates[(k + L) & 3];
            const int nb_fec = fecs[(k + byte / 4) & 3];
            unsigned host[6];
            rx_meta_record(fc, rate, nb_fec, decimated_sample_size(L, host_bits), host);
            // the incoming word: the byte under test in byte 1, everything else (the indicator nibble of m_sampleBytes, the sender's
            // block counts) noise that must not matter
            const unsigned noise = 0x9e3779b9u * (byte + 1) + L;
            const unsigned in_w2 = (noise & 0xffff00ffu) | (byte << 8);
            FollowedSize f = {0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu};
            const bool ok = followed_size_words(in_w2, L, host[0], host[1], host[2], &f);
            unsigned b = 0;
            CHECK(followed_sample_bits(in_w2, &b) == ok && b == byte);
            CHECK(ok == (byte >= 1 && byte <= 16));
            FollowedSize g = {0xdeadbeefu, 0xdeadbeefu, 0xdeadbeefu};
            CHECK(followed_size_words(byte << 8, L, host[0], host[1], host[2], &g) == ok);
            CHECK(g.shifts == f.shifts && g.w2 == f.w2 && g.crc0 == f.crc0); // (only byte 1 is read)
            if (!ok) {
                CHECK(f.shifts == 0xdeadbeefu && f.w2 == 0xdeadbeefu && f.crc0 == 0xdeadbeefu); // (nothing formed: the row stays)
                ++refused;
                printf("CASE L %u byte %u admitted 0\n", L, byte);
                continue;
            }
            ++admitted;
            const unsigned ssd = decimated_sample_size(L, byte);
            const DecimShifts sh = decimated_shifts(L, byte);
            CHECK(f.shifts == (sh.norm | (sh.trunk << 8)) && f.shifts == ragged_shift_word(L, byte));
            CHECK((f.w2 >> 16) == (host[2] >> 16));                           // bytes 2 and 3: 128 and the stream's own nbFECBlocks
            CHECK(((f.w2 >> 16) & 0xffu) == 128u && (f.w2 >> 24) == (unsigned)nb_fec);
            CHECK(((f.w2 >> 8) & 0xffu) == ssd && (f.w2 & 0xffu) == (ssd - 1) / 8 + 1);
            // the record a one-stream pipe configured with sample_bits = byte forms: the same third word, the same CRC
            unsigned twin[6];
            rx_meta_record(fc, rate, nb_fec, ssd, twin);
            CHECK(twin[0] == host[0] && twin[1] == host[1] && twin[2] == f.w2 && twin[5] == f.crc0);
            CHECK(meta_record_crc(host[0], host[1], host[2]) == host[5]); // (and the restatement on the host's own record)
            crcs += 2;
            printf("CASE L %u byte %u admitted 1 norm %u trunk %u bits %u w2 %08x fc %u rate %u crc %08x\n", L, byte, sh.norm, sh.trunk, ssd, f.w2,
                   host[0], host[1], f.crc0);
        }
    }
    CHECK(admitted == 7 * 16 && refused == 7 * 240);
    printf("admitted: %lu\nrefused: %lu\ncrcs held against rx_meta_record: %lu\nOK\n", admitted, refused, crcs);
    return 0;
}
