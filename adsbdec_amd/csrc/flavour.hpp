// flavour.hpp -- the sample flavours of the capture calls (include/adsbdec_amd.h: uint16 codes, _as, _packed, _iq, _power), each
// described ONCE: how n counts, how many power samples come out, what a device pointer is aligned to, whether n comes in whole
// 8-sample groups, what is launched in front of the kernel and with how many elements, which stream kind and level kind it is.
// The batch decodes, exports, level calls and the 12-bit gather read a capture's facts from here (decoder_stage.hip stages by them);
// the sentences of a refusal stay the operation's, but for the judgement of a format number, which is flavour_as / flavour_iq's.
// Plain host code: tests/cpp/flavour.cpp compiles it without HIP.  (The stream pushes of decoder.hip keep their own order of checks
// and call only the helpers at the end.)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "packed12.h"
#include "sample_format.h"

struct adsb_decoder;

namespace adsb {

constexpr int kKindNone = 0, kKindReal = 1, kKindIq = 2, kKindPower = 3, kKindIq8 = 4; // adsb_decoder::kind
// a PAIR of the stream's units IS a power sample (complex int16 samples, float32 power samples, complex int8 samples): no FIR
// ring, no quads, and the power samples enter the demodulator two at a time (air.c:94-99)
constexpr bool kind_in_twos(int kind) { return kind == kKindIq || kind == kKindPower || kind == kKindIq8; }
// Bytes of one unit of the stream -- what n_samples, stage_first and stage_fill count.  Every kind counts TWO units per pair /
// power sample, so the index arithmetic of the stream machinery (pairs, the carry in twos, compaction, the in-place rule at a
// multiple of 8 units, the EOF horizon) is one for all of them; a unit is 16 bits everywhere except in an int8 IQ stream, whose
// unit is ONE BYTE (I or Q).  Only where the machinery turns units into addresses and byte counts does the kind matter.
constexpr size_t kind_unit_bytes(int kind) { return kind == kKindIq8 ? 1 : 2; }

constexpr uint64_t power_samples_produced(uint64_t n_samples)
{
    return 2 * (n_samples / 4); // air.c:59-92: two power samples per four input samples
}

// Flavour::level_kind: real captures, and the kinds whose units ARE power samples -- level.h's kLevelIq16, kLevelIq8 and kLevelPower under
// names a host program can read (decoder_flavour.hip holds them to level.h)
constexpr int kLevelReal = -1, kLevelKindIq16 = 0, kLevelKindIq8 = 1, kLevelKindPower = 2;

struct Flavour {
    enum Front : uint8_t { kNone, kUnpack, kConvertReal, kConvertIq }; // launched in front, into scratch: nothing | unpack12 | convert, n | convert, 2 n
    int kind;          // kKindReal: n counts real samples, 2 (n / 4) power samples; kKindIq / kKindIq8 / kKindPower: n IS their number
    int level_kind;    // kLevelReal, or level.h's kLevelIq16 / kLevelIq8 / kLevelPower
    Front front;
    int conv;          // what launch_convert* is told (sample_format.h); 0: no conversion
    bool groups8;      // n comes in whole 8-sample groups
    unsigned in_align; // bytes a device input pointer is aligned to (0: host memory, any)

    constexpr bool real() const { return kind == kKindReal; }
    // the power samples of a capture of n
    constexpr uint64_t power_samples(size_t n) const { return real() ? power_samples_produced(n) : (uint64_t)n; }
    // the elements the launch in front writes to scratch: a capture without a power sample is not unpacked or converted (and so not
    // counted in the format report); complex float32 samples are two scalars each
    constexpr size_t scratch_elements(size_t n) const { return front == kNone || power_samples(n) == 0 ? 0 : front == kConvertIq ? 2 * n : n; }
    constexpr Flavour at(unsigned align) const { return Flavour{kind, level_kind, front, conv, groups8, align}; }
    constexpr Flavour on_host() const { return at(0); }
};

// ---- one constructor per family (in device memory; .on_host() for the caller's) ----
constexpr Flavour flavour_uint16() { return Flavour{kKindReal, kLevelReal, Flavour::kNone, 0, false, 16}; }
constexpr Flavour flavour_packed() { return Flavour{kKindReal, kLevelReal, Flavour::kUnpack, 0, true, 4}; }
constexpr Flavour flavour_power() { return Flavour{kKindPower, kLevelKindPower, Flavour::kNone, 0, false, 4}; }
// fmt is a converted real format (format_element_bytes(fmt) != 0) | an IQ format (iq_sample_bytes(fmt) != 0): judged by flavour_as /
// flavour_iq.  fmt 0 goes to fmt 2's int16 grid first; fmt 8 is never converted, a kind of its own whose units are bytes.
constexpr Flavour flavour_converted(int fmt) { return Flavour{kKindReal, kLevelReal, Flavour::kConvertReal, fmt, false, (unsigned)format_element_bytes(fmt)}; }
constexpr Flavour flavour_of_iq(int fmt)
{
    return fmt == kFmtInt8Iq ? Flavour{kKindIq8, kLevelKindIq8, Flavour::kNone, 0, false, 2}
                             : Flavour{kKindIq, kLevelKindIq16, fmt == kFmtFloat32Iq ? Flavour::kConvertIq : Flavour::kNone, fmt == kFmtFloat32Iq ? kConvFloat32Iq : 0, false, 4};
}

// ---- decoder_flavour.hip: the judgement of a format number, and what every _iq and _power call asks of its samples ----
// What every _as call checks first.  0: *f is the converted flavour; 1: fmt is the uint16 code itself (the caller forwards to the
// uint16 entry point); -1: refused.
int flavour_as(adsb_decoder *d, const char *what, int fmt, Flavour *f);
// 0: *f is the IQ flavour; -1: refused, fmt is not an IQ format.
int flavour_iq(adsb_decoder *d, const char *what, int fmt, Flavour *f);
int format_dispatch(adsb_decoder *d, const char *what, int fmt, size_t *elem);
int units_refusal(adsb_decoder *d, const char *what, const Flavour &F, const void *p, size_t n, uint64_t at_units);
int iq_refusal(adsb_decoder *d, const char *what, int fmt, const void *p, size_t n, bool device, uint64_t at_units);
int power_refusal(adsb_decoder *d, const char *what, const void *p, size_t n, bool device, uint64_t at_units);
inline int iq_kind(int fmt) { return flavour_of_iq(fmt).kind; }

} // namespace adsb
