// packed12.cpp -- the unpack of one Airspy packed 12-bit group (csrc/packed12.h: the function the unpack kernel runs, compiled
// for the host) against the format's known answers and its definition (w0:w1:w2 as one 96-bit big-endian number of eight
// 12-bit fields), every code at every position; run by tests/test_packed12_cpu.py.
#include <cstdio>
#include <cstring>
#include <random>

#include "../../adsbdec_amd/csrc/packed12.h"

static void words(const unsigned char *b, uint32_t w[3])
{
    for (int k = 0; k < 3; k++)
        w[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 | (uint32_t)b[4 * k + 3] << 24;
}

static int check(const uint32_t w[3], const uint16_t want[8], const char *what)
{
    uint16_t s[8];
    uint32_t pairs[4];
    adsb::unpack12_group(w[0], w[1], w[2], s);
    adsb::unpack12_group_pairs(w[0], w[1], w[2], pairs);
    for (int k = 0; k < 8; k++) {
        if (s[k] != want[k] || (uint16_t)(pairs[k / 2] >> (16 * (k % 2))) != want[k]) {
            printf("%s: sample %d = %03x (pairs %03x), want %03x\n", what, k, s[k], (pairs[k / 2] >> (16 * (k % 2))) & 0xffff, want[k]);
            return 1;
        }
    }
    return 0;
}

int main()
{
    const unsigned char kat1[12] = {0x78, 0x56, 0x34, 0x12, 0xf0, 0xde, 0xbc, 0x9a, 0x78, 0x56, 0x34, 0x12};
    const uint16_t want1[8] = {0x123, 0x456, 0x789, 0xabc, 0xdef, 0x012, 0x345, 0x678};
    const unsigned char kat2[12] = {0xff, 0x02, 0x18, 0x00, 0x00, 0x80, 0xff, 0xf7, 0x0f, 0x0f, 0x5a, 0xa5};
    const uint16_t want2[8] = {0x001, 0x802, 0xfff, 0x7ff, 0x800, 0x0a5, 0x5a0, 0xf0f};
    uint32_t w[3];
    words(kat1, w);
    if (check(w, want1, "known answer 1"))
        return 1;
    words(kat2, w);
    if (check(w, want2, "known answer 2"))
        return 1;
    // the definition: field k of the 96-bit big-endian number w0:w1:w2 is bits [84 - 12 k, 96 - 12 k)
    std::mt19937 rng(20261015);
    long groups = 0;
    for (int pos = 0; pos < 8; pos++) {
        for (uint32_t code = 0; code < 4096; code++) {
            uint16_t s[8];
            for (int k = 0; k < 8; k++)
                s[k] = (uint16_t)(rng() & 0xfff);
            s[pos] = (uint16_t)code;
            unsigned char bits[96];
            for (int k = 0; k < 8; k++)
                for (int b = 0; b < 12; b++)
                    bits[12 * k + b] = (s[k] >> (11 - b)) & 1;
            for (int q = 0; q < 3; q++) {
                w[q] = 0;
                for (int b = 0; b < 32; b++)
                    w[q] = (w[q] << 1) | bits[32 * q + b];
            }
            if (check(w, s, "definition"))
                return 1;
            groups++;
        }
    }
    printf("packed12 ok: 2 known answers, %ld groups\n", groups);
    return 0;
}
