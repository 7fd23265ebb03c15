"""The cases and the expectation that hold the seam kernel (csrc/seam_kernel.hip) sample by sample and offset by offset:
tests/test_wrap_seam_cpu.py pins them on the CPU, tests/test_gpu_wrap_seam.py holds the kernel to them.

A case is a window of N = 65 536 samples centred on a wrap of the reference's sample counter (air.c:34): first_sample =
w * 2^32 - N / 2, power samples [P - 16 384, P + 16 384) with P = w * 2^31.  Its content is one of the nine kinds of
candidate_model.make_captures at one of PLACEMENTS against P; silence lies in front of it (wrap_model.power's history).

Expected power: wrap_model.power(y, first_sample, "true", wrap=w).  Expected lists: oracle.scan_all of that power, moved to
stream offsets.  The wrong models (MODES[1:]) are what a kernel could compute instead; sensitivity() says which expected value
each of them changes."""
import functools

import numpy as np

import candidate_model as M
import wrap_model as W

N = 1 << 16                      # samples of a window
HALF = N // 4                    # power samples on either side of P
E = W.E
WRAPS = (1, 2, 1_000_003)        # the large one: 64-bit index arithmetic only (the ring phase restarts at every wrap)
SEAM_LO, SEAM_HI = -1196, 28     # seam offsets [P - 1196, P + 28) (csrc/seam_kernel.h)
N_POWER = SEAM_HI - SEAM_LO - 1 + 1196   # 2 419 power samples a launch over all of them reads: P - 1196 .. P + 1222
TRANSIENT = range(-1, 6)         # P - 1 .. P + 5
# Where the content sits against P: the window is samples [s, s + N) of make_captures(N + PAD).  Two starts that differ by
# 2 (mod 4) move every preamble and bit cell by an odd number of power samples against P - 1 .. P + 5.  The four were chosen
# (test_wrap_seam_cpu.py asserts it) so that at each of them some kind decodes a candidate AT a transient sample and another
# reads one as the last sample of its frame.  ZERO: make_captures(N) as it is -- no candidate at P - 1 .. P + 5, kept as a case.
PAD = 8192
PLACEMENTS = (1430, 3512, 4790, 6072)
ZERO = None
# The 1-bit repair: the `damaged` kind damages every other long frame, 2 700 offsets apart, so a window holds ONE damaged frame
# start in the 1 224 seam offsets.  damaged_window() cuts the windows out of that kind made longer (the same recipe and seed), at
# starts that bring five DIFFERENT damaged frames into the seam offsets: across P, in the middle, at the first offsets, at the last, in
# the middle again -- five damaged bits, in bytes 10, 1, 13, 6 and 8 of the frame: every one of the slicer's four column words.
DAMAGED_PAD = 7 * 5400
DAMAGED_PLACEMENTS = (2642, 9232, 15792, 18792, 35832)
KINDS = ("sparse", "dense", "noise", "uniform", "saturated", "gate_storm", "back_to_back", "short_frames", "damaged")
# true; the two of wrap_model; the seven products of P - 1 .. P + 5 added in slot order 6 .. 0; the ring rule for P .. P + 6
# (P - 1 by its own epoch's formula, as if the counter had not wrapped one output early)
MODES = ("true", "stale_phase", "no_transient", "reversed_sum", "shifted_transient")


def first_sample(w):
    return w * (1 << 32) - N // 2


def offsets(w):
    """(g0, one past the last offset with a whole window of power samples, P)."""
    g0 = first_sample(w) // 2
    return g0, g0 + N // 2 - 1195, w * E


@functools.lru_cache(maxsize=None)
def _captures(n):
    caps = M.make_captures(n)
    assert tuple(caps) == KINDS
    return caps


def window(kind, placement):
    """The N samples of a case (read-only)."""
    y = _captures(N)[kind] if placement is None else _captures(N + PAD)[kind][placement: placement + N]
    assert y.size == N
    y = y.view()
    y.flags.writeable = False
    return y


@functools.lru_cache(maxsize=None)
def _damaged_capture():
    """candidate_model.make_captures' `damaged` kind, N + DAMAGED_PAD samples long."""
    from tools import gen_signal as G
    n = N + DAMAGED_PAD
    return G.synth(n, M._placed(np.arange(3000, n - 2600, 2700), (17, 18), np.random.default_rng(309), damage=True), 8.0, 309)


def damaged_window(placement):
    y = _damaged_capture()[placement: placement + N]
    assert y.size == N
    y = y.view()
    y.flags.writeable = False
    return y


def blocks_window():
    """Codes 0 / 4095 / 65535 in blocks of 1, 2, 3, 4, 5, 6, 7, 14 and 28 samples: every product of the FIR at its extremes."""
    rng = np.random.default_rng(411)
    out = np.empty(N, np.uint16)
    at = 0
    while at < N:
        k = int(rng.choice((1, 2, 3, 4, 5, 6, 7, 14, 28)))
        out[at: at + k] = rng.choice((0, 4095, 65535))
        at += k
    return out


def uniform_window():
    return np.random.default_rng(412).integers(0, 65536, size=N, dtype=np.uint16)


def ring_sample(y, fs, m, order=range(7)):
    """Power sample m by the ring rule, literally (air.c:59-92 with a 32-bit counter; wrap_model's doc): slot pair i holds the
    latest pair q <= m with (q mod 2^31) mod 7 == i, meets taps T[(2 i - 2 c) mod 14] and the next, c = ((m + 1) mod 2^31) mod 7;
    every product rounded to float32, the products added in `order`."""
    q0 = fs // 2
    c = ((m + 1) % E) % 7
    s = None
    for i in order:
        q = next(q for q in range(m, m - 14, -1) if (q % E) % 7 == i)
        if q >= q0:
            v = y[2 * (q - q0): 2 * (q - q0) + 2].astype(np.float32) - np.float32(2048.0)
            if q % 2:
                v = -v
        else:
            v = np.zeros(2, np.float32)
        t = (2 * i - 2 * c) % 14
        pr = np.array([W.TAPS[t] * v[0], W.TAPS[(t + 1) % 14] * v[1]], np.float32)
        s = pr if s is None else (s + pr).astype(np.float32)
    sq = (s * s).astype(np.float32)
    return np.float32(sq[0] + sq[1])


def power(y, w, mode="true"):
    """a[k] = power sample first_sample(w) / 2 + k of the window under `mode`."""
    fs = first_sample(w)
    if mode in W.MODES:
        return W.power(y, fs, mode, wrap=w)
    a = W.power(y, fs, "true", wrap=w)
    g0, _, P = offsets(w)
    if mode == "reversed_sum":
        for k in TRANSIENT:
            a[P + k - g0] = ring_sample(y, fs, P + k, order=range(6, -1, -1))
    elif mode == "shifted_transient":
        a[P - 1 - g0] = W.power(y, fs, "stale_phase", wrap=w)[P - 1 - g0]
    else:
        raise ValueError(mode)
    return a


def lists(oracle, a, w, df18, lo=None, hi=None):
    """oracle.scan_all over the window's offsets (or [lo, hi) of them) in stream offsets: ([(g, pw, frame)], try words)."""
    g0, g1, _ = offsets(w)
    lo, hi = g0 if lo is None else lo, g1 if hi is None else hi
    assert g0 <= lo <= hi <= g1
    cands, tries = oracle.scan_all(a, lo - g0, hi - g0, df18)
    return [(g + g0, pw, fr) for g, pw, fr in cands], tries + np.uint64(g0 << 2)


def seam_lists(oracle, a, w, df18):
    _, _, P = offsets(w)
    return lists(oracle, a, w, df18, P + SEAM_LO, P + SEAM_HI)


def seam_power(a, w):
    """The N_POWER samples the seam offsets read, P - 1196 .. P + 1222."""
    g0, _, P = offsets(w)
    return a[P + SEAM_LO - g0: P + SEAM_LO - g0 + N_POWER]


def last_read(c):
    """The last power sample the slicer reads for candidate c: bit k compares a[g + 80 + 10 k] with a[g + 85 + 10 k]."""
    return c[0] + 85 + 10 * (8 * len(c[2]) - 1)


def sensitivity(oracle, placement, w=1):
    """{mode: {"lists": kinds whose seam lists (either df18 setting) differ from the true ones, "bits": kinds whose seam power
    differs in a bit}} for the wrong models."""
    out = {m: {"lists": [], "bits": []} for m in MODES[1:]}
    for kind in KINDS:
        y = window(kind, placement)
        true = power(y, w)
        tl = [seam_lists(oracle, true, w, d) for d in (False, True)]
        for mode in MODES[1:]:
            a = power(y, w, mode)
            if not np.array_equal(seam_power(a, w).view(np.uint32), seam_power(true, w).view(np.uint32)):
                out[mode]["bits"].append(kind)
            wl = [seam_lists(oracle, a, w, d) for d in (False, True)]
            if any(x[0] != t[0] or not np.array_equal(x[1], t[1]) for x, t in zip(wl, tl)):
                out[mode]["lists"].append(kind)
    return out


def repairable(oracle, a, w, df18=True):
    """The seam offsets at which a long frame passes the DF gate, misses the CRC and is mended by one flipped bit among bits
    5 .. 111 (what fix_1bit repairs): [(g, pw, mended frame, the bit)] -- the one-bit-damaged long frames that start in the seam."""
    g0, _, P = offsets(w)
    _, tries = seam_lists(oracle, a, w, df18)
    out = []
    for g in sorted({int(t) >> 2 for t in tries}):
        k, fr, pw = oracle.eval_offset(a, g - g0, df18)
        if k != 2 or len(fr) != 14:
            continue
        for b in range(5, 112):
            m = bytearray(fr)
            m[b >> 3] ^= 0x80 >> (b & 7)
            if oracle.crc_residual(bytes(m)) == 0:
                out.append((g, pw, bytes(m), b))
                break
    return out
