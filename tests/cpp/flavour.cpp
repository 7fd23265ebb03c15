// flavour.cpp -- csrc/flavour.hpp on the CPU: for every flavour and the capture lengths the GPU rows use (real: 0, 3, 4, 8, 30, 64;
// IQ and power: 0, 1, 28, 29) and a few thousand more, the power-sample count and the elements the launch in front writes to scratch,
// against the rules written out here per flavour and on their own; the facts a refusal reads (groups of 8, alignment, kinds); and that
// .on_host() / .at() change the alignment alone.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../adsbdec_amd/csrc/flavour.hpp"

using namespace adsb;

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            printf("%s, n = %zu: %s (line %d)\n", name, n, #c, __LINE__);      \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// what the test expects of a flavour, stated without flavour.hpp's accessors
struct Want {
    const char *name;
    Flavour f;
    bool real;      // n counts real samples: two power samples per whole four
    int scale;      // elements in scratch per n where anything is launched in front (0: nothing is)
    bool groups8;
    unsigned align;
    int kind;
    int conv;
};

static size_t checked = 0;

static void check(const Want &w, size_t n)
{
    const char *name = w.name;
    const uint64_t power = w.real ? 2 * (n / 4) : n;
    CHECK(w.f.power_samples(n) == power);
    size_t scratch = 0;
    if (w.scale && w.real && n >= 4)
        scratch = n;
    if (w.scale && !w.real && n >= 1)
        scratch = (size_t)w.scale * n;
    CHECK(w.f.scratch_elements(n) == scratch);
    CHECK((w.f.scratch_elements(n) == 0) == (w.scale == 0 || power == 0));
    CHECK(w.f.real() == w.real && w.f.groups8 == w.groups8 && w.f.in_align == w.align && w.f.kind == w.kind && w.f.conv == w.conv);
    CHECK((w.f.front == Flavour::kNone) == (w.scale == 0));
    const Flavour h = w.f.on_host(), a = w.f.at(16);
    CHECK(h.in_align == 0 && a.in_align == 16);
    CHECK(h.power_samples(n) == power && h.scratch_elements(n) == scratch && a.scratch_elements(n) == scratch);
    CHECK(h.kind == w.kind && h.level_kind == w.f.level_kind && h.front == w.f.front && h.conv == w.conv && h.groups8 == w.groups8);
    checked++;
}

int main()
{
    const Want wants[] = {
        {"uint16", flavour_uint16(), true, 0, false, 16, kKindReal, 0},
        {"packed", flavour_packed(), true, 1, true, 4, kKindReal, 0},
        {"as FLOAT32_REAL", flavour_converted(kFmtFloat32Real), true, 1, false, 4, kKindReal, kFmtFloat32Real},
        {"as INT16_REAL", flavour_converted(kFmtInt16Real), true, 1, false, 2, kKindReal, kFmtInt16Real},
        {"iq FLOAT32_IQ", flavour_of_iq(kFmtFloat32Iq), false, 2, false, 4, kKindIq, kConvFloat32Iq},
        {"iq INT16_IQ", flavour_of_iq(kFmtInt16Iq), false, 0, false, 4, kKindIq, 0},
        {"iq INT8_IQ", flavour_of_iq(kFmtInt8Iq), false, 0, false, 2, kKindIq8, 0},
        {"power", flavour_power(), false, 0, false, 4, kKindPower, 0},
    };
    const size_t real_n[] = {0, 3, 4, 8, 30, 64}, twos_n[] = {0, 1, 28, 29};
    for (const Want &w : wants) {
        if (w.real)
            for (size_t n : real_n)
                check(w, n);
        else
            for (size_t n : twos_n)
                check(w, n);
        for (size_t n = 0; n < 4200; n++)
            check(w, n);
        for (size_t n : {(size_t)1 << 20, ((size_t)1 << 31) - 1, ((size_t)1 << 32) - 4, ((size_t)1 << 32) - 1})
            check(w, n);
    }
    // the kinds: a real capture is the only one with a level kind below zero, and the three others differ
    const char *name = "kinds";
    const size_t n = 0;
    CHECK(flavour_uint16().level_kind == kLevelReal && flavour_packed().level_kind == kLevelReal && flavour_converted(kFmtInt16Real).level_kind == kLevelReal);
    CHECK(flavour_of_iq(kFmtFloat32Iq).level_kind == flavour_of_iq(kFmtInt16Iq).level_kind);
    CHECK(flavour_of_iq(kFmtInt8Iq).level_kind != flavour_of_iq(kFmtInt16Iq).level_kind && flavour_power().level_kind != flavour_of_iq(kFmtInt8Iq).level_kind &&
          flavour_power().level_kind != flavour_of_iq(kFmtInt16Iq).level_kind && flavour_power().level_kind >= 0 && flavour_of_iq(kFmtInt8Iq).level_kind >= 0 &&
          flavour_of_iq(kFmtInt16Iq).level_kind >= 0);
    CHECK(iq_kind(kFmtInt8Iq) == kKindIq8 && iq_kind(kFmtInt16Iq) == kKindIq && iq_kind(kFmtFloat32Iq) == kKindIq);
    printf("ok: %zu checks of %zu flavours\n", checked, sizeof wants / sizeof wants[0]);
    return 0;
}
