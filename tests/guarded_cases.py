"""The captures, cuts and guards that hold the device calls to the oracle from GUARDED, SEPARATE buffers: what a call is given is
[p, p + n) and nothing else, so everything around it in memory is a decoy -- another capture's frames, louder -- and a kernel or a
launch bound that reads a pair outside its buffer gives CRC-valid wrong records, or other power samples, instead of the right
answer by accident.  No device code here: tests/test_guarded_cpu.py proves from the oracle alone that each guard can be seen,
tests/test_gpu_guarded.py runs the cases on the device.

A stream UNIT is what the library's stream counts (decoder.hip, push_device_impl): a uint16 sample of a real stream, a 16-bit
scalar of an int16 IQ stream (two per complex sample), half a float of a power stream (two per power sample), a byte of an int8
IQ stream (two per complex sample).  A cut at unit c is power sample c / 2 in every kind.

Kinds: "real" (uint16 codes; the int16 and float32 real formats are its exact twins), "real8" (the same with every piece a
multiple of 8: packed input comes in whole groups), "iq" (int16 I, Q; float32 IQ is its exact twin), "iq8" (int8 I, Q) and "power"
(float32 power samples)."""
import functools
import os
import re

import numpy as np

from conftest import ROOT
from test_power_cpu import SCALES, scaled

# ---------------------------------------------------------------- the pieces of section 1
MIN = 1 << 16                                  # kInPlaceMinSamples: below it a device push is staged
SEAM = 4096                                    # kSeamSamples: what an in-place push copies to the staging buffer first
ALIGN = 8                                      # an in-place push starts at a multiple of 8 units (and a 16-byte aligned pointer)
GUARD = 8192                                   # units of decoy on either side of a piece: > a wave's 7 KiB window, > the seam copy
TOTAL = 410_000                                # 205 000 power samples: the reference's last deqframe call visits up to ~203 700
REACH = 1196                                   # offsets in front of a cut whose windows cross it

SIZES = (
    MIN,                                       # exactly the in-place minimum, at the stream's start: in place, no seam
    MIN + ALIGN * 6808,                        # larger, a multiple of 8: in place behind a seam copy
    SEAM + ALIGN,                              # below the minimum: the staged road between two in-place pieces
    MIN + ALIGN // 2,                          # in place, and the next piece starts at 4 mod 8
    MIN + ALIGN * 1536 + ALIGN // 2,           # long but at 4 mod 8: staged; the piece behind it starts at a multiple of 8 again
    TOTAL - (4 * MIN + SEAM + ALIGN * 8346),   # at least the minimum, pushed with _final: in place to the stream's exact end
)
# packed input starts at a multiple of 8 and comes in groups of 8: the two pieces of 4 mod 8 are rounded, nothing is staged for
# its position (the pointer of a packed push is free: it is unpacked into the handle's scratch, which is aligned)
SIZES_PACKED = SIZES[:3] + (MIN + ALIGN, MIN + ALIGN * 1536, SIZES[5])


def header_constants():
    """{name: value} of the constexpr size_t constants of csrc/decoder_state.hpp that are plain numbers or shifts."""
    text = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "decoder_state.hpp")).read()
    out = {}
    for name, a, b in re.findall(r"constexpr\s+size_t\s+(k\w+)\s*=\s*(\d+)u?\s*(?:<<\s*(\d+))?\s*;", text):
        out[name] = int(a) << int(b or 0)
    return out


def cuts(sizes):
    return [int(v) for v in np.cumsum(sizes)[:-1]]


def roads(sizes):
    """[(first unit, units, "in_place" | "staged", final)] of a run of device pushes of these sizes from a 16-byte aligned pointer
    each: push_device_impl's rule."""
    out, at = [], 0
    for i, n in enumerate(sizes):
        out.append((at, n, "in_place" if at % ALIGN == 0 and n >= MIN else "staged", i == len(sizes) - 1))
        at += n
    return out


def check_sizes(sizes, packed=False):
    """The classes section 1 names, in this order and reversed, against the constants of decoder_state.hpp."""
    k = header_constants()
    assert (k["kInPlaceMinSamples"], k["kSeamSamples"]) == (MIN, SEAM)
    assert len(sizes) >= 5 and sum(sizes) == TOTAL and all(n % 2 == 0 for n in sizes)
    for order in (sizes, sizes[::-1]):
        r = roads(order)
        assert r[0][2] == "in_place" and r[-1][2] == "in_place" and r[-1][1] >= MIN and r[-1][3]
        assert any(n == MIN and road == "in_place" for _, n, road, _ in r)
        assert any(n > MIN and n % ALIGN == 0 and road == "in_place" and at > 0 for at, n, road, _ in r)
        short = [i for i, (_, n, road, _) in enumerate(r) if n < MIN]
        assert len(short) == 1 and SEAM < r[short[0]][1] <= SEAM + 2 * ALIGN and r[short[0]][2] == "staged"
        assert r[short[0] + 1][2] == "in_place" and (order is not sizes or r[short[0] - 1][2] == "in_place")
        late = [(at, n) for at, n, road, _ in r if n >= MIN and road == "staged"]
        assert packed or (late and all(at % ALIGN != 0 for at, _ in late))       # long, but staged for where it starts
        assert not packed or all(at % ALIGN == 0 and n % ALIGN == 0 for at, n, _, _ in r)
    both = sorted(set(cuts(sizes)) | set(cuts(sizes[::-1])))
    ends = [(at, at + n) for order in (sizes, sizes[::-1]) for at, n, _, _ in roads(order) if n < MIN]
    # the planted frames of two cuts never meet: 2 x (1200 + 1204) offsets apart, but for the two ends of the short piece
    assert len(both) == 2 * (len(sizes) - 1) and all(b - a >= 2 * 2 * 2404 or (a, b) in ends for a, b in zip(both, both[1:])), both
    return True


# ---------------------------------------------------------------- frames planted relative to the cuts
def plan(sizes, shift=0):
    """[(first candidate offset, DF, "across" | "behind", cut)] for the cuts of both orders.  Across cut c (power sample h = c / 2):
    a frame whose first candidate is the last offset from which the greedy decode still lands on h + 4 -- h - 1196 for a long
    frame (a DF17 or DF18 in turn), h - 636 for a DF11 --, so its preamble lies in the last 1196 offsets and its last data bit lies
    across the cut (an accepted frame carries the decode to its end: one that crossed the cut any further would hide the frame
    behind the cut from the decode, which is all a stream call shows); behind it a frame of the other length whose first
    candidates are h + 3 .. h + 6.  Long and short alternate over the cuts, counted from the short piece: its two ends are 2052
    offsets apart, and take a DF11 each on the inside.
    shift: the weakened plan, every frame moved away from its cut."""
    out = []
    for order in (tuple(sizes), tuple(sizes[::-1])):
        begin_short = [i for i, n in enumerate(order) if n < MIN][0] - 1
        for i, c in enumerate(cuts(order)):
            h = c // 2
            a_long = (i - begin_short) % 2 == 0
            out.append((h + 4 - (1200 if a_long else 640) + shift, (17, 18)[i % 2] if a_long else 11, "across", c))
            out.append((h + 3 + shift, 11 if a_long else (18, 17)[i % 2], "behind", c))
    return out


def _frames(kind, sizes, seed, shift, amp):
    """The generator's frame list: the plan, and background traffic (a frame every 2900 offsets, DF17 / 11 / 18 in turn) wherever no
    planted frame is within reach.  A real frame from sample s on has its first candidate at s / 2 + 3, a complex one at s."""
    from tools import gen_signal as G
    rng = np.random.default_rng(seed)
    fir = kind in ("real", "real8")
    start = (lambda g: 2 * (g - 3)) if fir else (lambda g: g)
    planted = plan(sizes, shift)
    out = []
    for g, df, role, _ in planted:
        fr = G.make_frame(df, rng)
        while role == "across" and not fr[-1] & 1:           # its last bit is a 1: high, then a gap -- the half that lies across the cut
            fr = G.make_frame(df, rng)
        out.append((start(g), fr, float(rng.uniform(*amp)), float(rng.uniform(0, 2 * np.pi))))
    taken = sorted(g for g, _, _, _ in planted)
    for i, g in enumerate(range(1500, TOTAL // 2 - 2600, 2900)):
        if all(abs(g - t) > 2500 for t in taken):
            out.append((start(g), G.make_frame((17, 11, 18)[i % 3], rng), float(rng.uniform(*amp)), float(rng.uniform(0, 2 * np.pi))))
    return out


def _back_to_back(kind, seed, amp):
    """The decoy's frames: back to back, one every 1204 offsets, other bytes, a higher amplitude."""
    from tools import gen_signal as G
    rng = np.random.default_rng(seed)
    start = (lambda g: 2 * (g - 3)) if kind in ("real", "real8") else (lambda g: g)
    return [(start(g), G.make_frame((18, 17, 11)[i % 3], rng), float(rng.uniform(*amp)), float(rng.uniform(0, 2 * np.pi)))
            for i, g in enumerate(range(40, TOTAL // 2 - 1300, 1204))]


def _synth(kind, frames, sigma, seed, bursts=()):
    """The generator's capture of a kind.  bursts: cuts (units) around which the carrier stands for 16 power samples, 8 on either
    side, at 1900 codes -- the decoy's: whatever reads a few pairs of it across a cut reads a pulse where the stream has a gap."""
    from tools import gen_signal as G
    from adsbdec_amd.sample_formats import iq_power, to_int8_iq
    if kind in ("real", "real8"):
        x = G.synth(TOTAL, frames, sigma, seed)
        for c in bursts:
            n = np.arange(c - 16, c + 16)
            x[c - 16:c + 16] = np.clip(np.rint(2048.0 + 1900.0 * np.cos(np.pi * n / 2 + 0.4)), 0, 4095).astype(np.uint16)
        return x
    x = G.iq_synth(TOTAL // 2, frames, sigma, seed)
    for c in bursts:
        x[c // 2 - 8:c // 2 + 8] = (int(16 * 1900 * np.cos(0.4)), int(16 * 1900 * np.sin(0.4)))
    if kind == "iq8":
        return np.ascontiguousarray(to_int8_iq(x)[0])
    return x if kind == "iq" else iq_power(x)


KINDS = ("real", "real8", "iq", "iq8", "power")
_SEED = {k: 8100 + 10 * i for i, k in enumerate(KINDS)}
UPE = {"real": 1, "real8": 1, "iq": 1, "iq8": 1, "power": 2}      # units per element of the flat array


def power_of(kind, flat):
    """The power samples the library defines for a stream of this kind (flat: the stream's elements in one dimension)."""
    from adsbdec_amd.sample_formats import iq_power
    from oracle import oracle as O
    if kind in ("real", "real8"):
        return O.power(np.ascontiguousarray(flat))
    if kind == "power":
        return np.ascontiguousarray(flat)
    return iq_power(flat.reshape(-1, 2), 8 if kind == "iq8" else 2)


class Stream:
    """One capture of section 1.  kind, sizes; x: the capture as one flat array (real: uint16 codes; iq: int16 scalars; iq8: int8
    scalars; power: floats), decoy: the other capture, same shape; a: the capture's power samples; cands, tries: oracle.scan_all
    of every offset (df18 on); frames, stats: the oracle's decode of the whole; decoy_g: the offsets of the decoy's own CRC-valid
    candidates."""

    def sl(self, c0, c1):
        return slice(c0 // UPE[self.kind], c1 // UPE[self.kind])

    def with_guard(self, c0, c1, other):
        """The capture with units [c0, c1) taken from `other` (clipped to the capture)."""
        y = self.x.copy()
        s = self.sl(max(c0, 0), min(c1, TOTAL))
        y[s] = other[s]
        return y


def make_stream(kind, sizes=None, shift=0):
    from oracle import oracle as O
    O.build()
    sizes = tuple(sizes or (SIZES_PACKED if kind == "real8" else SIZES))
    s = Stream()
    s.kind, s.sizes = kind, sizes
    seed = _SEED[kind]
    # (an int8 capture keeps 1 / 256 of the int16 scale: 700 codes are 44 of its steps, the noise is below one)
    x = _synth(kind, _frames(kind, sizes, seed, shift, (700.0, 1100.0)), 5.0, seed)
    decoy = _synth(kind, _back_to_back(kind, seed + 1, (1700.0, 2000.0)), 9.0, seed + 1, sorted(set(cuts(sizes)) | set(cuts(sizes[::-1]))))
    if kind == "power":                                      # general floats: two of test_power_cpu's scales, the decoy's the larger
        x, decoy = scaled(x, SCALES[0]), scaled(decoy, SCALES[2])
    s.x, s.decoy = x.reshape(-1), decoy.reshape(-1)
    assert s.x.size * UPE[kind] == TOTAL and s.decoy.shape == s.x.shape and s.decoy.dtype == s.x.dtype
    s.a = power_of(kind, s.x)
    assert s.a.size == TOTAL // 2
    s.n_off = s.a.size - 1195                                # (TOTAL % 4 == 0: every kind has TOTAL / 2 power samples)
    s.cands, s.tries = O.scan_all(s.a, 0, s.n_off, True)
    s.frames, s.stats = O.decode(s.x, df18=True) if kind in ("real", "real8") else O.demod_power(s.a, df18=True)
    da = power_of(kind, s.decoy)
    s.decoy_g = np.array([c[0] for c in O.scan_all(da, 0, da.size - 1195, True)[0]], dtype=np.int64)
    return s


@functools.lru_cache(maxsize=None)
def stream(kind):
    """The stream of a kind, checked: evaluated once per process."""
    s = make_stream(kind)
    check_sizes(s.sizes, packed=kind == "real8")
    check_stream(s, s.decoy)
    return s


def _span(df):
    return 640 if df == 11 else 1200


def check_planted(s):
    """Every planted frame is where the plan says, as the ORACLE sees the whole capture: a CRC-valid candidate at its first offset,
    and the greedy decode accepts the frame across the cut at that offset and the one behind the cut at one of h .. h + 5."""
    have = {c[0]: c for c in s.cands}
    accepted = {f["g"]: f for f in s.frames}
    for g0, df, role, c in plan(s.sizes):
        h = c // 2
        # (behind the FIR a frame's first candidate is the planned offset or the next one: the carrier's phase decides)
        first = [g for g in (g0, g0 + 1) if g in have and have[g][2][0] >> 3 == df and g - 1 not in have]
        where = (s.kind, role, c, g0)
        assert first, where
        g = first[0]
        if role == "across":
            assert h - REACH <= g < h and g + _span(df) > h, where
            assert g in accepted and accepted[g]["frame"] == have[g][2], where
        else:
            assert h <= g <= h + 5, where
            hit = [k for k in range(h, h + 6) if k in accepted and accepted[k]["frame"] == have[g][2]]
            assert hit, where
    return True


def check_cut(s, c, decoy):
    """Cut c can be seen from both sides with `decoy` as the guards.  Behind the cut: with the decoy as the continuation, a record
    or a try word of the last 1196 offsets before c / 2 changes.  In front of it: with the decoy as the predecessor, a real
    stream's power samples c / 2 .. c / 2 + 5 change (the FIR's six pairs) and nothing behind them, and a record among the first
    offsets behind the cut changes; a stream without a FIR reads nothing in front of an offset, so there the predecessor shows at
    the offsets BEFORE the cut and not one power sample from c / 2 on changes.  And each guard stretch carries CRC-valid
    records of its own: reading it gives wrong frames, not merely none."""
    from oracle import oracle as O
    h = c // 2
    fir = s.kind in ("real", "real8")
    own = O.scan_all(s.a, h - REACH, h, True)
    back = power_of(s.kind, s.with_guard(c, c + GUARD, decoy))
    got = O.scan_all(back, h - REACH, h, True)
    assert np.array_equal(back[:h], s.a[:h]) and (got[0] != own[0] or not np.array_equal(got[1], own[1])), (s.kind, c, "behind")
    front = power_of(s.kind, s.with_guard(c - GUARD, c, decoy))
    changed = np.flatnonzero(front[h:] != s.a[h:])
    if fir:
        assert changed.tolist() == [0, 1, 2, 3, 4, 5], (s.kind, c, changed[:10])
        assert O.scan_all(front, h, h + 7, True)[0] != O.scan_all(s.a, h, h + 7, True)[0], (s.kind, c, "in front")
    else:
        assert changed.size == 0, (s.kind, c, changed[:10])
        assert O.scan_all(front, h - REACH, h, True)[0] != own[0], (s.kind, c, "in front")
    da = power_of(s.kind, decoy)
    g = np.array([r[0] for r in O.scan_all(da, max(0, h - GUARD // 2), min(h + GUARD // 2, da.size) - 1195, True)[0]], dtype=np.int64)
    assert ((g < h - REACH) & (g >= h - GUARD // 2)).any() and (g >= h).any(), (s.kind, c, "the guards carry no record of their own")
    return True


def check_stream(s, decoy):
    check_planted(s)
    for c in sorted(set(cuts(s.sizes)) | set(cuts(s.sizes[::-1]))):
        check_cut(s, c, decoy)
    return True


# ---------------------------------------------------------------- what the fronts push (section 1)
# front: (kind, the call family, fmt)
FRONTS = {
    "u16": ("real", "real", None),
    "s16": ("real", "as", 3),
    "f32": ("real", "as", 1),
    "packed": ("real8", "packed", None),
    "iq16": ("iq", "iq", 2),
    "iqf32": ("iq", "iq", 0),
    "iq8": ("iq8", "iq", 8),
    "power": ("power", "power", None),
}


def unit_bytes(front):
    """Bytes one stream unit takes in the memory a front is given (packed: 1.5, as a fraction of 8 units = 12 bytes)."""
    return {"u16": 2, "s16": 2, "f32": 4, "packed": 1.5, "iq16": 2, "iqf32": 4, "iq8": 1, "power": 2}[front]


def as_front(front, flat):
    """A stretch of a kind's flat array as the bytes the front's calls take: the exact twin of its format."""
    from adsbdec_amd import sample_formats as S
    from adsbdec_amd.packed12 import pack12
    if front == "s16":
        b = S.to_int16_real(flat)
    elif front == "f32":
        b = S.to_float32_real(flat)
    elif front == "packed":
        assert flat.size % 8 == 0
        b = pack12(flat)
    elif front == "iqf32":
        b = S.to_float32_iq(flat)
    else:
        b = flat
    return np.ascontiguousarray(b).view(np.uint8).reshape(-1)


def guarded(front, s, c0, c1):
    """Units [c0, c1) of the stream between GUARD units of the decoy on either side -- the stretch of the decoy in front of c0 and
    the stretch behind c1, wrapped round at the capture's two ends -- as bytes; -> (bytes, byte offset of the piece)."""
    n = TOTAL // UPE[s.kind]
    at = np.arange((c0 - GUARD) // UPE[s.kind], (c1 + GUARD) // UPE[s.kind]) % n
    flat = s.decoy[at]
    lo = GUARD // UPE[s.kind]
    flat[lo:lo + (c1 - c0) // UPE[s.kind]] = s.x[s.sl(c0, c1)]
    lead = int(GUARD * unit_bytes(front))
    b = as_front(front, flat)
    assert lead % 16 == 0 and b.size == int((c1 - c0 + 2 * GUARD) * unit_bytes(front))
    return b, lead


def count_of(front, units):
    """What the front's calls are given as n for a piece of `units` stream units: samples, complex samples or power samples."""
    return units if FRONTS[front][1] in ("real", "as", "packed") else units // 2


# ---------------------------------------------------------------- sections 2 to 4: loud memory
def loud_codes(n, seed, rails=True):
    """n full-range 12-bit codes, never silence (no 0x800), both rails among them."""
    x = np.random.default_rng(seed).integers(0, 4096, n, dtype=np.uint16)
    x[x == 0x800] = 0x801
    if rails and n >= 4:
        x[[1, n // 2]] = 0
        x[[2, n - 2]] = 4095
    return x


def loud_iq(fmt, n, seed):
    """n loud complex samples of an IQ format, never silence, both rails among them (fmt 0: the exact float twin of int16)."""
    from adsbdec_amd.sample_formats import to_float32_iq
    rng = np.random.default_rng(seed)
    if fmt == 8:
        x = rng.integers(-128, 128, (n, 2), dtype=np.int8)
        lo, hi = -128, 127
    else:
        x = rng.integers(-32768, 32768, (n, 2), dtype=np.int16)
        lo, hi = -32768, 32767
    x[x == 0] = 1
    x[1], x[n - 2] = (lo, hi), (hi, lo)
    return to_float32_iq(x) if fmt == 0 else x


def loud_power(n, seed):
    """n loud power samples inside the _power calls' domain, none of them zero."""
    return np.random.default_rng(seed).uniform(1.0, 2.0 ** 28, n).astype(np.float32)


def never_silence(flat):
    """No unit of `flat` is what silence is in its format: code 0x800, a zero float, a zero scalar."""
    flat = np.asarray(flat).reshape(-1)
    if flat.dtype == np.uint16:
        return bool((flat != 0x800).all())
    return bool((flat != 0).all())


def check_first_six(x, guard):
    """A real capture's six first power samples, and no others, change when `guard` (codes) lies in front of it instead of
    silence: tests/test_gpu_batch_records.py's assertion, for any capture and guard."""
    from oracle import oracle as O
    a = O.power(np.ascontiguousarray(x))
    lead = np.full(56, 0x800, np.uint16)
    k = min(16, guard.size)
    lead[56 - k:] = guard[guard.size - k:]
    changed = np.flatnonzero(O.power(np.concatenate([lead, x]))[28:28 + a.size] != a)
    assert changed.tolist() == [0, 1, 2, 3, 4, 5][:a.size], changed[:10]
    return True


def check_rails(guard, kind):
    """The guard holds a code on each rail: a call that read it would count it."""
    from adsbdec_amd.levels import rails
    lo, hi, _ = rails(guard, kind)
    assert lo > 0 and hi > 0, (kind, lo, hi)
    return True


# section 4's lengths: a run, a wave's pass, a workgroup's pass, several workgroups with a ragged end (real codes); below a run,
# odd, a wave's pass and one more, several workgroups with a ragged end (complex and power samples)
REAL_LENGTHS = (56, 3584 + 4, 14336 + 6, 2 * (3 * 7168 + 30) + 3)
IQ_LENGTHS = (1, 27, 1792, 1793, 3 * 7168 + 45)
LOUD_GUARD = 64                                # elements of loud memory on either side of a capture of sections 2 to 4


def inside_loud(payload, guard_front, guard_back):
    """guard | payload | guard as bytes -> (bytes, byte offset of the payload)."""
    f, p, b = (np.ascontiguousarray(v).view(np.uint8).reshape(-1) for v in (guard_front, payload, guard_back))
    return np.concatenate([f, p, b]), f.size


# ---------------------------------------------------------------- section 3, batches: a loud batch, then the targets
N_AROUND = 70_000                              # the targets of section 3 are captures of about this many samples
# road: (family of stale_cases, the form the call takes, fmt, device call?).  The families: "real" (the n % 4 = 1 edge capture and
# 70 000 .. 70 007 samples), "packed" (the three of whole groups), "iq" (the five complex ones); every target batch has an empty capture
# in the middle, and the loud batch in front of it is the loud capture three times, each cut to a different length.
BATCH_ROADS = {
    "decode_batch": ("real", "u16", None, False),
    "decode_batch_as3": ("real", "s16", 3, False),
    "decode_batch_as1": ("real", "f32", 1, False),
    "decode_batch_packed": ("packed", "packed", None, False),
    "decode_batch_iq0": ("iq", "iqf32", 0, False),
    "decode_batch_iq2_one_pointer_4_mod_16": ("iq", "iq16", 2, False),
    "decode_batch_power": ("iq", "power", None, False),
    "decode_batch_device_packed": ("packed", "packed", None, True),
    "decode_batch_device_as3": ("real", "s16", 3, True),
    "decode_batch_device_iq2_one_pointer_4_mod_16": ("iq", "iq16", 2, True),   # (the scratch copy of misaligned captures: device pointers only)
    "power_batch": ("real", "u16", None, False),
    "power_batch_device_packed": ("packed", "packed", None, True),
    "power_batch_device_as1": ("real", "f32", 1, True),
    "power_batch_device_iq0": ("iq", "iqf32", 0, True),
    "level_batch": ("real", "u16", None, False),
    "level_batch_device_packed": ("packed", "packed", None, True),
    "level_batch_device_as3": ("real", "s16", 3, True),
    "level_batch_device_iq0": ("iq", "iqf32", 0, True),
}


def batch_form(form, x):
    """A capture as the oracle knows it (codes, or int16 (I, Q) rows) -> the array a call of this form is given."""
    from adsbdec_amd import sample_formats as S
    from adsbdec_amd.packed12 import pack12
    if form == "packed":
        return pack12(x) if x.size else np.empty(0, np.uint8)
    if form == "power":
        return np.ascontiguousarray(S.iq_power(x), dtype="<f4")
    return np.ascontiguousarray({"s16": S.to_int16_real, "f32": S.to_float32_real, "iqf32": S.to_float32_iq}.get(form, lambda v: v)(x))


LOUD_CUTS = (0, 1, 2)                          # groups of 8 elements cut from the end of the loud capture: three lengths, all of them
                                               # four times a target of N_AROUND samples and, to within 16 elements, the edge capture


def loud_batch(loud):
    """The loud capture three times, each cut to a different length (whole groups of 8 elements: packed input comes in them)."""
    n = len(loud)
    return [np.ascontiguousarray(loud[:n - 8 * k]) for k in LOUD_CUTS]


def with_an_empty_capture(targets):
    """The targets in order with an empty capture in the middle -> (captures, index of the empty one)."""
    mid = len(targets) // 2
    return list(targets[:mid]) + [targets[0][:0]] + list(targets[mid:]), mid


def slots(n_bytes, align):
    """Where a batch's captures lie in one of the handle's batch buffers: capture i at the sum of the sizes before it, each rounded
    up to `align` bytes -> (offsets, total).  The plain statement of csrc/stage_layout.hpp."""
    at, cur = [], 0
    for b in n_bytes:
        at.append(cur)
        cur += -(-int(b) // align) * align
    return at, cur


def check_stale_batch_shows(loud, targets, align):
    """loud, targets: the arrays two batches put into one buffer, captures at multiples of `align` bytes.  Every target of the batch
    that follows the loud one lies wholly inside bytes the loud batch wrote, the buffer shrinks in use, and what the loud batch left
    at the target's place is not the target: a call that read its buffer's past would read other samples."""
    la, lt = slots([np.asarray(x).nbytes for x in loud], align)
    ta, tt = slots([np.asarray(x).nbytes for x in targets], align)
    assert tt < lt and len({np.asarray(x).nbytes for x in loud}) == len(loud) == 3
    flat = np.zeros(lt, np.uint8)                             # (the pad between two captures is nobody's: zeros here)
    for x, a in zip(loud, la):
        b = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        flat[a:a + b.size] = b
    assert all(a % align == 0 for a in la + ta)
    for x, a in zip(targets, ta):
        b = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        assert b.size == 0 or not np.array_equal(flat[a:a + b.size], b)
    return True
