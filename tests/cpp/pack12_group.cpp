// pack12_group.cpp -- the pack of one Airspy packed 12-bit group (csrc/packed12.h pack12_group: the function the 12-bit gather
// kernel runs, compiled for the host) against the format's known answers (those of tests/cpp/packed12.cpp, read the other way),
// against its definition (eight 12-bit fields of one 96-bit big-endian number) and against unpack12_group, its inverse: every code
// at every position, random groups, and samples above 4095, of which the low 12 bits are packed; run by
// tests/test_gather_pack12_cpu.py under AddressSanitizer and UBSan.
#include <cstdio>
#include <cstring>
#include <random>

#include "../../adsbdec_amd/csrc/packed12.h"

static void words(const unsigned char *b, uint32_t w[3])
{
    for (int k = 0; k < 3; k++)
        w[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 | (uint32_t)b[4 * k + 3] << 24;
}

static int same(const uint32_t got[3], const uint32_t want[3], const char *what)
{
    for (int k = 0; k < 3; k++) {
        if (got[k] != want[k]) {
            printf("%s: word %d = %08x, want %08x\n", what, k, got[k], want[k]);
            return 1;
        }
    }
    return 0;
}

int main()
{
    const unsigned char kat1[12] = {0x78, 0x56, 0x34, 0x12, 0xf0, 0xde, 0xbc, 0x9a, 0x78, 0x56, 0x34, 0x12};
    const uint16_t in1[8] = {0x123, 0x456, 0x789, 0xabc, 0xdef, 0x012, 0x345, 0x678};
    const unsigned char kat2[12] = {0xff, 0x02, 0x18, 0x00, 0x00, 0x80, 0xff, 0xf7, 0x0f, 0x0f, 0x5a, 0xa5};
    const uint16_t in2[8] = {0x001, 0x802, 0xfff, 0x7ff, 0x800, 0x0a5, 0x5a0, 0xf0f};
    uint32_t w[3], want[3];
    words(kat1, want);
    adsb::pack12_group(in1, w);
    if (same(w, want, "known answer 1"))
        return 1;
    words(kat2, want);
    adsb::pack12_group(in2, w);
    if (same(w, want, "known answer 2"))
        return 1;
    // the fill of a clipped piece: eight codes 2048 are the bytes 00 08 80 | 80 00 08 | 08 80 00 of the words 0x80080080 0x08008008 0x00800800
    const uint16_t fill[8] = {2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048};
    const uint32_t fill_want[3] = {0x80080080u, 0x08008008u, 0x00800800u};
    adsb::pack12_group(fill, w);
    if (same(w, fill_want, "eight codes 2048"))
        return 1;
    std::mt19937 rng(20261021);
    long groups = 0;
    for (int pos = 0; pos < 8; pos++) {
        for (uint32_t code = 0; code < 4096; code++) {
            uint16_t s[8], high[8], back[8];
            for (int k = 0; k < 8; k++)
                s[k] = (uint16_t)(rng() & 0xfff);
            s[pos] = (uint16_t)code;
            // the definition: field k of the 96-bit big-endian number w0:w1:w2 is bits [84 - 12 k, 96 - 12 k)
            unsigned char bits[96];
            for (int k = 0; k < 8; k++)
                for (int b = 0; b < 12; b++)
                    bits[12 * k + b] = (s[k] >> (11 - b)) & 1;
            for (int q = 0; q < 3; q++) {
                want[q] = 0;
                for (int b = 0; b < 32; b++)
                    want[q] = (want[q] << 1) | bits[32 * q + b];
            }
            adsb::pack12_group(s, w);
            if (same(w, want, "definition"))
                return 1;
            // the inverse
            adsb::unpack12_group(w[0], w[1], w[2], back);
            if (memcmp(back, s, sizeof s) != 0) {
                printf("unpack12_group(pack12_group(s)) != s at position %d, code %03x\n", pos, code);
                return 1;
            }
            // bits 12 .. 15 of a sample are dropped, whatever they are
            for (int k = 0; k < 8; k++)
                high[k] = (uint16_t)(s[k] | ((rng() & 0xf) << 12));
            adsb::pack12_group(high, w);
            if (same(w, want, "samples above 4095"))
                return 1;
            groups++;
        }
    }
    // ... and the other way round: any three words survive unpack, then pack
    for (long i = 0; i < 200000; i++) {
        const uint32_t v[3] = {(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng()};
        uint16_t s[8];
        adsb::unpack12_group(v[0], v[1], v[2], s);
        adsb::pack12_group(s, w);
        if (same(w, v, "pack12_group(unpack12_group(w))"))
            return 1;
    }
    printf("pack12_group ok: 3 known answers, %ld groups, 200000 random words\n", groups);
    return 0;
}
