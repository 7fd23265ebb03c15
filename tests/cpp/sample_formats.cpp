// sample_formats.cpp -- the two sample functions the conversion kernels run (csrc/sample_format.h, compiled for the host) against
// the formats' definitions: every int16 value, every code through both formats and back, and the float32 edge cases, each
// restated here in integer / binary64 arithmetic.  `sample_formats <fmt> <in> <out>` converts a file of samples instead and writes
// (uint16 code, uint16 what) pairs: tests/test_sample_formats_cpu.py holds those against adsbdec_amd/sample_formats.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../adsbdec_amd/csrc/sample_format.h"

using namespace adsb;

static uint32_t bits_of(float x)
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

static float float_of(uint32_t b)
{
    float x;
    memcpy(&x, &b, 4);
    return x;
}

// the definition in binary64, where 2048 x is exact for every binary32 x
static uint32_t float_definition(uint32_t bits, uint32_t *what)
{
    const double v = (double)float_of(bits);
    if (std::isnan(v)) {
        *what = kSampleClamped;
        return 2048;
    }
    const double r = std::nearbyint(v * 2048.0); // (the default rounding mode: ties to even)
    if (r < -2048.0 || r > 2047.0) {
        *what = kSampleClamped;
        return r < 0 ? 0 : 4095;
    }
    *what = (r / 2048.0 == v) ? kSampleExact : kSampleInexact;
    return (uint32_t)((long)r + 2048);
}

static long g_float_cases = 0;

static int check_float(uint32_t bits, const char *what_case)
{
    uint32_t w, ww;
    const uint32_t c = float32_real_code(bits, &w), cw = float_definition(bits, &ww);
    g_float_cases++;
    if (c == cw && w == ww)
        return 0;
    printf("%s: bits %08x (%g): code %u what %u, want %u %u\n", what_case, bits, (double)float_of(bits), c, w, cw, ww);
    return 1;
}

static int expect_float(uint32_t bits, uint32_t code, uint32_t what, const char *what_case)
{
    uint32_t w;
    const uint32_t c = float32_real_code(bits, &w);
    if (c == code && w == what)
        return check_float(bits, what_case);
    printf("%s: bits %08x: code %u what %u, want %u %u\n", what_case, bits, c, w, code, what);
    return 1;
}

static int convert_file(int fmt, const char *in, const char *out)
{
    const size_t elem = format_element_bytes(fmt);
    FILE *f = elem ? fopen(in, "rb") : nullptr, *g = elem ? fopen(out, "wb") : nullptr;
    if (!f || !g)
        return 2;
    unsigned char b[4];
    while (fread(b, 1, elem, f) == elem) {
        const uint32_t bits = elem == 2 ? (uint32_t)b[0] | (uint32_t)b[1] << 8
                                        : (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
        uint32_t w;
        const uint32_t c = fmt == kFmtInt16Real ? sample_code<kFmtInt16Real>(bits, &w) : sample_code<kFmtFloat32Real>(bits, &w);
        const uint16_t rec[2] = {(uint16_t)c, (uint16_t)w};
        fwrite(rec, 2, 2, g);
    }
    fclose(f);
    return fclose(g) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 4)
        return convert_file(atoi(argv[1]), argv[2], argv[3]);
    static_assert(format_element_bytes(kFmtInt16Real) == 2 && format_element_bytes(kFmtFloat32Real) == 4 && format_element_bytes(4) == 0, "");
    // every int16 value: floor(x / 16) + 2048, inexact iff x is no multiple of 16
    for (int x = -32768; x <= 32767; x++) {
        uint32_t w;
        const uint32_t c = int16_real_code((uint32_t)(uint16_t)(int16_t)x, &w);
        const int fl = (x >= 0 ? x / 16 : -((-x + 15) / 16)) + 2048;
        if ((int)c != fl || c > 4095 || w != (x % 16 ? kSampleInexact : kSampleExact)) {
            printf("int16 %d: code %u what %u, want %d\n", x, c, w, fl);
            return 1;
        }
    }
    // every code through both formats and back, exact
    for (int code = 0; code < 4096; code++) {
        uint32_t w;
        if (int16_real_code((uint32_t)(uint16_t)(int16_t)((code - 2048) * 16), &w) != (uint32_t)code || w != kSampleExact) {
            printf("int16 round trip of code %d\n", code);
            return 1;
        }
        if (expect_float(bits_of((float)(code - 2048) / 2048.0f), (uint32_t)code, kSampleExact, "grid point"))
            return 1;
        // its neighbours by one ulp: the same code (or its neighbour's, next to 0.0's denormals never), inexact
        const uint32_t b = bits_of((float)(code - 2048) / 2048.0f);
        if (code != 2048) {
            if (check_float(b + 1, "grid point + 1 ulp") || check_float(b - 1, "grid point - 1 ulp"))
                return 1;
            uint32_t wa, wb;
            float32_real_code(b + 1, &wa);
            float32_real_code(b - 1, &wb);
            if (wa == kSampleExact || (wb == kSampleExact))
                return printf("a neighbour of grid point %d counts as exact\n", code), 1;
        }
    }
    // every tie (k + 0.5) / 2048: to the even neighbour
    for (int k = -2049; k <= 2048; k++) {
        const float x = ((float)k + 0.5f) / 2048.0f;
        int even = (k & 1) ? k + 1 : k;
        uint32_t what = kSampleInexact;
        if (even < -2048 || even > 2047)
            what = kSampleClamped, even = even < 0 ? -2048 : 2047;
        if (expect_float(bits_of(x), (uint32_t)(even + 2048), what, "tie"))
            return 1;
    }
    struct { uint32_t bits, code, what; const char *name; } edge[] = {
        {0x00000000u, 2048, kSampleExact, "+0.0"},       {0x80000000u, 2048, kSampleExact, "-0.0"},
        {0x00000001u, 2048, kSampleInexact, "smallest denormal"}, {0x007fffffu, 2048, kSampleInexact, "largest denormal"},
        {0x80000001u, 2048, kSampleInexact, "-smallest denormal"}, {0x807fffffu, 2048, kSampleInexact, "-largest denormal"},
        {0x00800000u, 2048, kSampleInexact, "smallest normal"},
        {bits_of(1.0f), 4095, kSampleClamped, "+1.0"},   {bits_of(-1.0f), 0, kSampleExact, "-1.0"},
        {0x7f800000u, 4095, kSampleClamped, "+Inf"},     {0xff800000u, 0, kSampleClamped, "-Inf"},
        {0x7fc00000u, 2048, kSampleClamped, "NaN"},      {0xffc00001u, 2048, kSampleClamped, "-NaN"},
        {0x7f800001u, 2048, kSampleClamped, "signalling NaN"},
        {bits_of(1e30f), 4095, kSampleClamped, "1e30"},  {bits_of(-1e30f), 0, kSampleClamped, "-1e30"},
        {0x7f7fffffu, 4095, kSampleClamped, "FLT_MAX"},  {bits_of(-1.0f) + 1, 0, kSampleInexact, "-1.0 - 1 ulp"},
        {bits_of(2047.0f / 2048.0f), 4095, kSampleExact, "the largest grid point"},
    };
    for (const auto &e : edge)
        if (expect_float(e.bits, e.code, e.what, e.name))
            return 1;
    // a sweep of bit patterns over all exponents against the binary64 definition
    for (uint64_t b = 0; b < (1ull << 32); b += 65521)
        if (check_float((uint32_t)b, "sweep"))
            return 1;
    printf("sample_formats ok: 65536 int16 values, 4096 codes in both formats, %ld float cases\n", g_float_cases);
    return 0;
}
