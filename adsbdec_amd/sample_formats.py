"""Signed 16-bit real and float32 real samples (include/adsbdec_amd.h: the formats; airspy_rx -t 3 and -t 1) in plain numpy: the
test-side definition, independent of the library's conversion kernels, and a converter for capture files.

    INT16_REAL    x = (code - 2048) << 4;  code = (x >> 4) + 2048;  inexact iff x & 15
    FLOAT32_REAL  x = (code - 2048) / 2048;  r = rint(2048 x) (ties to even), code = r + 2048 clamped to [0, 4095];
                  clamped iff r + 2048 is outside [0, 4095] or x is +-Inf or NaN (NaN -> 2048), else inexact iff
                  (code - 2048) / 2048 is not x (-0.0 is exact; every non-zero denormal is inexact)

    python -m adsbdec_amd.sample_formats -t 3 in.u16 out.s16          # uint16 capture -> int16 real (-t 1: float32 real)
    python -m adsbdec_amd.sample_formats -t 3 --back in.s16 out.u16   # and back; stderr counts what was off the grid

and the two complex formats (airspy_rx -t 2 and -t 0; the library's _iq calls), which have no uint16 twin -- the converter goes
between the two of them:

    INT16_IQ      int16 (I, Q);  i = I / 16, q = Q / 16;  power sample a = fl(fl(i i) + fl(q q)) in binary32
    FLOAT32_IQ    float32 (I, Q), nominal [-1, 1);  each scalar r = rint(32768 x) (ties to even) clamped to [-32768, 32767];
                  clamped iff r is outside or x is +-Inf or NaN (NaN -> 0), else inexact iff r is not 32768 x; then as INT16_IQ

    python -m adsbdec_amd.sample_formats -t 0 in.s16iq out.f32iq      # int16 IQ capture -> float32 IQ (exact)
    python -m adsbdec_amd.sample_formats -t 0 --back in.f32iq out.s16iq

and float32 POWER samples (the library's _power calls: the reference's ampbuff stream itself, no format of airspy_rx), with the
numpy statement of their input domain (power_domain_ok) and a converter that writes the power file of an IQ capture:

    python -m adsbdec_amd.sample_formats -t 2 --power in.s16iq out.pw   # iq_power of an int16 IQ capture (-t 0: of a float32 one)

and complex int8 captures (the _iq calls' fmt 8 -- the library's own number, not one of airspy_rx: hackrf_transfer's cs8, bladeRF and
USRP sc8), which are decoded as their widened int16 twin is:

    INT8_IQ       int8 (I, Q);  twin = (I << 8, Q << 8) as INT16_IQ;  power sample a = 256 (I^2 + Q^2), an exact integer <= 2^23

    python -m adsbdec_amd.sample_formats -t 8 in.s16iq out.cs8          # int16 IQ capture -> int8 (x >> 8); stderr counts low bits lost
    python -m adsbdec_amd.sample_formats -t 8 --back in.cs8 out.s16iq   # the widened twin (exact)
    python -m adsbdec_amd.sample_formats -t 8 --power in.cs8 out.pw     # its power samples
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

FLOAT32_REAL, INT16_REAL = 1, 3
FLOAT32_IQ, INT16_IQ, INT8_IQ = 0, 2, 8
DTYPES = {FLOAT32_REAL: np.dtype("<f4"), INT16_REAL: np.dtype("<i2")}
IQ_DTYPES = {FLOAT32_IQ: np.dtype("<f4"), INT16_IQ: np.dtype("<i2"), INT8_IQ: np.dtype("i1")}
NAMES = {FLOAT32_REAL: "FLOAT32_REAL", INT16_REAL: "INT16_REAL", FLOAT32_IQ: "FLOAT32_IQ", INT16_IQ: "INT16_IQ", INT8_IQ: "INT8_IQ"}


def _codes(x) -> np.ndarray:
    x = np.asarray(x)
    if x.size and int(x.max()) > 0xFFF:
        raise ValueError("codes above 4095 have no value in this format")
    return x.astype(np.int32)


def to_int16_real(x) -> np.ndarray:
    """uint16 codes 0..4095 -> int16 samples."""
    return ((_codes(x) - 2048) * 16).astype("<i2")


def to_float32_real(x) -> np.ndarray:
    """uint16 codes 0..4095 -> float32 samples in [-1, 1)."""
    return ((_codes(x) - 2048) / 2048.0).astype("<f4")


def flags_int16_real(x) -> tuple[np.ndarray, np.ndarray]:
    """int16 samples -> (codes, inexact mask)."""
    x = np.asarray(x, dtype=np.int16).astype(np.int32)
    return (np.floor_divide(x, 16) + 2048).astype(np.uint16), (x % 16) != 0


def flags_float32_real(x) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """float32 samples -> (codes, inexact mask, clamped mask), in binary64, where 2048 x is exact for every binary32 x."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x.astype(np.float64)                             # (a signalling NaN raises "invalid" in the cast)
        nan = np.isnan(v)
        r = np.rint(np.where(nan, 0.0, v) * 2048.0)          # np.rint: ties to even
        clamped = nan | (r < -2048.0) | (r > 2047.0)         # (+-Inf: r is +-Inf)
        c = np.clip(r, -2048.0, 2047.0)
        inexact = ~clamped & (c / 2048.0 != v)               # (-0.0 == 0.0; a denormal is not 0)
    return (c + 2048.0).astype(np.uint16), inexact, clamped


def from_int16_real(x):
    """int16 samples -> (codes, inexact, clamped = 0)."""
    codes, inexact = flags_int16_real(x)
    return codes, int(inexact.sum()), 0


def from_float32_real(x):
    """float32 samples -> (codes, inexact, clamped): a sample is counted once, clamped wins."""
    codes, inexact, clamped = flags_float32_real(x)
    return codes, int(inexact.sum()), int(clamped.sum())


def to_format(fmt: int, x) -> np.ndarray:
    return to_int16_real(x) if fmt == INT16_REAL else to_float32_real(x)


def from_format(fmt: int, x):
    return from_int16_real(x) if fmt == INT16_REAL else from_float32_real(x)


# ---- complex captures ----
def to_float32_iq(x) -> np.ndarray:
    """int16 IQ scalars -> float32 IQ scalars (x / 32768: exact), same shape."""
    return (np.asarray(x, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).astype("<f4")


def flags_float32_iq(x) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """float32 IQ scalars -> (int16 scalars, inexact mask, clamped mask), in binary64, where 32768 x is exact or overflows to Inf."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x.astype(np.float64)
        nan = np.isnan(v)
        y = np.where(nan, 0.0, v) * 32768.0
        r = np.rint(y)                                       # np.rint: ties to even
        clamped = nan | (r < -32768.0) | (r > 32767.0)       # (+-Inf: r is +-Inf)
        c = np.clip(r, -32768.0, 32767.0)
        inexact = ~clamped & (c != y)                        # (-0.0 == 0.0; a denormal is not 0)
    return c.astype(np.int16), inexact, clamped


def to_int16_iq(x):
    """float32 IQ scalars -> (int16 scalars, inexact, clamped): a scalar is counted once, clamped wins."""
    r, inexact, clamped = flags_float32_iq(x)
    return r, int(inexact.sum()), int(clamped.sum())


def widen_int8_iq(x8) -> np.ndarray:
    """int8 IQ scalars -> the int16 IQ scalars of the widened twin (x << 8: exact), same shape."""
    return (np.asarray(x8, dtype=np.int8).astype(np.int16) * np.int16(256)).astype("<i2")


def to_int8_iq(x16):
    """int16 IQ scalars -> (int8 scalars, inexact): x >> 8, an arithmetic shift; inexact counts the scalars whose low 8 bits are
    not all zero (what the shift drops)."""
    x = np.asarray(x16, dtype=np.int16)
    return (x >> 8).astype(np.int8), int(np.count_nonzero(x & 0xFF))


def iq_power(x, fmt: int = INT16_IQ) -> np.ndarray:
    """The power samples of a complex capture (scalars I, Q, I, Q, ...: any shape with an even number of them) as the library
    defines them: strict binary32, two rounded products and a rounded sum, one power sample per complex sample."""
    if fmt == FLOAT32_IQ:
        x = flags_float32_iq(x)[0]
    elif fmt == INT8_IQ:                                        # the widened twin's samples: 256 (I^2 + Q^2), exact
        x = widen_int8_iq(x)
    elif fmt != INT16_IQ:
        raise ValueError(f"format {fmt} is not an IQ format")
    s = np.asarray(x, dtype=np.int16).reshape(-1, 2).astype(np.float32) * np.float32(0.0625)
    i, q = s[:, 0], s[:, 1]
    return (i * i + q * q).astype(np.float32)               # (numpy rounds every float32 operation on its own)


def power_domain_ok(a) -> bool:
    """The input domain of the _power calls (include/adsbdec_amd.h): every sample finite, its sign bit clear, below 2^29 -- no
    negative, no -0.0, no NaN, no Inf.  Subnormals are inside.  Decided on the bit patterns."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.dtype("<f4"):
        raise ValueError(f"power samples are float32, not {a.dtype}")
    bits = a.view("<u4")
    return bool((bits < np.float32(2.0 ** 29).view("<u4")).all())   # (sign bit set, NaN and Inf are all larger as unsigned words)


def _main_power(a) -> int:
    dt = IQ_DTYPES[a.t]
    b = np.fromfile(a.src, dtype=np.uint8)
    cut = b.size % (2 * dt.itemsize)
    if cut:
        sys.stderr.write(f"{a.src}: {cut} trailing bytes (a partial sample) ignored\n")
    pw = iq_power(b[: b.size - cut].view(dt), a.t)
    assert power_domain_ok(pw)                                       # (|I|, |Q| <= 2048: a power sample is at most 2^23)
    pw.astype("<f4").tofile(a.dst)
    return 0


def _main_iq8(a) -> int:
    dt = IQ_DTYPES[INT8_IQ] if a.back else IQ_DTYPES[INT16_IQ]
    b = np.fromfile(a.src, dtype=np.uint8)
    cut = b.size % (2 * dt.itemsize)
    if cut:
        sys.stderr.write(f"{a.src}: {cut} trailing bytes (a partial sample) ignored\n")
    x = b[: b.size - cut].view(dt)
    if a.back:
        widen_int8_iq(x).tofile(a.dst)
    else:
        r, inexact = to_int8_iq(x)
        if inexact:
            sys.stderr.write(f"{a.src}: {inexact} of {x.size} scalars are not on the int8 grid (low bits dropped)\n")
        r.tofile(a.dst)
    return 0


def _main_iq(a) -> int:
    dt = IQ_DTYPES[FLOAT32_IQ] if a.back else IQ_DTYPES[INT16_IQ]
    b = np.fromfile(a.src, dtype=np.uint8)
    cut = b.size % (2 * dt.itemsize)
    if cut:
        sys.stderr.write(f"{a.src}: {cut} trailing bytes (a partial sample) ignored\n")
    x = b[: b.size - cut].view(dt)
    if a.back:
        r, inexact, clamped = to_int16_iq(x)
        if inexact + clamped:
            sys.stderr.write(f"{a.src}: {inexact + clamped} of {x.size} scalars are not on the int16 grid ({clamped} clamped)\n")
        r.astype("<i2").tofile(a.dst)
    else:
        to_float32_iq(x).tofile(a.dst)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m adsbdec_amd.sample_formats", description=__doc__.split("\n\n")[0])
    ap.add_argument("-t", type=int, choices=sorted(DTYPES) + [FLOAT32_IQ, INT16_IQ, INT8_IQ], required=True,
                    help="1 = FLOAT32_REAL, 3 = INT16_REAL (as airspy_rx -t); 0 = between INT16_IQ and FLOAT32_IQ; 8 = between INT16_IQ and INT8_IQ; "
                         "with --power: 2 / 0 / 8, the format of src")
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--back", action="store_true", help="the format -> uint16 codes instead of uint16 codes -> the format")
    ap.add_argument("--power", action="store_true", help="src is an IQ capture (-t 2 INT16_IQ, -t 0 FLOAT32_IQ): write its float32 power samples")
    a = ap.parse_args(argv)
    if a.power:
        if a.t not in IQ_DTYPES or a.back:
            ap.error("--power takes -t 2, -t 0 or -t 8 and no --back")
        return _main_power(a)
    if a.t == INT16_IQ:
        ap.error("-t 2 goes with --power only (the converter between the IQ formats is -t 0)")
    if a.t == FLOAT32_IQ:
        return _main_iq(a)
    if a.t == INT8_IQ:
        return _main_iq8(a)
    dt = DTYPES[a.t] if a.back else np.dtype("<u2")
    b = np.fromfile(a.src, dtype=np.uint8)
    cut = b.size % dt.itemsize
    if cut:
        sys.stderr.write(f"{a.src}: {cut} trailing bytes (a partial sample) ignored\n")
    x = b[: b.size - cut].view(dt)
    if a.back:
        codes, inexact, clamped = from_format(a.t, x)
        if inexact + clamped:
            sys.stderr.write(f"{a.src}: {inexact + clamped} of {x.size} samples are not {NAMES[a.t]} values ({clamped} clamped)\n")
        codes.astype("<u2").tofile(a.dst)
    else:
        to_format(a.t, x).tofile(a.dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
