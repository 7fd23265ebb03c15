"""Flush (adsb_set_flush; DESIGN.md "Flush"): the silent twin, and the captures the flush tests decode.

The truth of every flush answer is the oracle on the capture's SILENT TWIN: the whole units the call scans, followed by silence
worth P power samples -- code 2048 for real samples, (0, 0) for IQ, +0.0 for power samples.  P = 2 x ADSB_APBUFFSZ in the library's
definition; any even P >= 43 400 gives the same answer (test_flush_cpu.py holds that)."""
import functools

import numpy as np

APBUFFSZ, DECOFFSET, WINDOW = 40980, 1200, 1196
P_DEF = 2 * APBUFFSZ
P_ALL = (43_400, P_DEF, 120_000)


def twin_real(x, P=P_DEF):
    """uint16 codes: the first 4 floor(n / 4) samples, then 2 P codes of 2048."""
    x = np.ascontiguousarray(x)
    return np.concatenate([x[:4 * (x.size // 4)], np.full(2 * P, 2048, np.uint16)])


def twin_power(a, P=P_DEF):
    """float32 power samples: the first 2 floor(n / 2), then P of +0.0 (a trailing odd power sample is never seen: air.c:94-99)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.concatenate([a[:2 * (a.size // 2)], np.zeros(P, np.float32)])


def twin_iq(x, P=P_DEF):
    """int16 (n, 2): the first 2 floor(n / 2) complex samples, then P of (0, 0)."""
    return np.concatenate([x[:2 * (len(x) // 2)], np.zeros((P, 2), x.dtype)])


def recs(frames):
    return [(f["g"], f["ts"], f["pw"], bytes(f["frame"])) for f in frames]


def want_real(oracle, x, df18=True, fix1=False, P=P_DEF):
    fr, st = oracle.decode(twin_real(x, P), df18=df18, fix1=fix1)
    return recs(fr), st


def want_power(oracle, a, df18=True, P=P_DEF):
    fr, st = oracle.demod_power(twin_power(a, P), df18=df18)
    return recs(fr), st


def iq_power(x, fmt=2):
    from adsbdec_amd import sample_formats
    return np.ascontiguousarray(sample_formats.iq_power(x, fmt))


def _frame(rng, df, last_bit=None):
    from tools import gen_signal as G
    while True:
        fr = G.make_frame(df, rng)
        if last_bit is None or (fr[-1] & 1) == last_bit:
            return fr


# ------------------------------------------------------------------ captures with a frame at their end
# `end`: where the frame ENDS, in power samples relative to the capture's M (its power samples): -1, 0, +1, +20 cut the frame, so that
# the slicer reads silence; a frame whose last bit is 1 is high in the first half of its last microsecond only, so it survives a
# cut of up to five power samples and its jump carries the scan past M.
def real_capture(n, seed, end=0, df=17, sigma=4.0, extra=()):
    """uint16 capture of n samples: a frame of `df` ending `end` power samples behind M = 2 floor(n / 4), frames `extra` = [(start
    power sample, df)] in front."""
    from tools import gen_signal as G
    rng = np.random.default_rng([seed, 0xF1])
    M = 2 * (n // 4)
    span = 640 if df == 11 else 1200
    frames = [(2 * s, _frame(rng, d), float(rng.uniform(300, 1500)), float(rng.uniform(0, 6.28))) for s, d in extra]
    start = M + end - span
    if start >= 0:
        frames.append((2 * start, _frame(rng, df, 1), float(rng.uniform(300, 1500)), float(rng.uniform(0, 6.28))))
    return G.synth(n, frames, sigma, seed)


def iq_capture(n, seed, end=0, df=17, sigma=1.0, extra=()):
    """int16 (n, 2) capture of n complex samples, laid out as real_capture (M = 2 floor(n / 2))."""
    from tools import gen_signal as G
    rng = np.random.default_rng([seed, 0xF2])
    M = 2 * (n // 2)
    span = 640 if df == 11 else 1200
    frames = [(s, _frame(rng, d), float(rng.uniform(100, 1500)), float(rng.uniform(0, 6.28))) for s, d in extra]
    start = M + end - span
    if start >= 0:
        frames.append((start, _frame(rng, df, 1), float(rng.uniform(100, 1500)), float(rng.uniform(0, 6.28))))
    return G.iq_synth(n, frames, sigma, seed)


ENDS = (-1, 0, 1, 20, 3, -40)


def seeded(kind, count=200):
    """`count` small captures of a kind ("real": uint16, "iq": int16 pairs): lengths 1 300 .. 6 000 units (every n % 4 and n % 28), a
    long or short frame ending at ENDS around M; every 20th is 84 000 .. 120 000 units long and has frames in front, so that the
    non-flush decode returns some."""
    out = []
    rng = np.random.default_rng([0xF3, len(kind)])
    for i in range(count):
        long_one = i % 20 == 19
        n = int(rng.integers(84_000, 120_000)) if long_one else int(rng.integers(1_300, 6_000))
        df = (17, 11, 18)[i % 3]
        end = ENDS[i % len(ENDS)]
        M = 2 * (n // 4) if kind == "real" else 2 * (n // 2)
        extra = [(int(s), (17, 11)[k % 2]) for k, s in enumerate(range(500, M - 3000, 9_000))] if long_one else []
        out.append((real_capture if kind == "real" else iq_capture)(n, 1000 + i, end, df, extra=extra))
    return out


@functools.lru_cache(maxsize=None)
def seeded_cached(kind, count=200):
    return seeded(kind, count)
