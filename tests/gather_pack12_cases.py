"""The cases of the 12-bit burst gather (adsb_gather_pack12_layout, adsb_gather_pack12_device, _as, _packed;
adsbdec_amd/burst_archive.py layout12 and gather12 are the statement), shared by tests/test_gather_pack12_cpu.py and
tests/test_gpu_gather_pack12.py.  No GPU and no reference here: the literal loop over pieces, groups and bits; captures of 12-bit
codes between guards of code 4095; burst tables aimed at the kernel's chunk of C 16-byte words and at its three word phases; the
tables a call refuses.

A run is 28 power samples = 56 samples = 7 groups = 84 packed bytes = 5.25 words, so pieces of 1, 2, 3 and 4 runs end in every
word phase (k % 3) and at every quarter of a word.  A case is (name, M, table)."""
import numpy as np

import gather_cases as GC

RUN = 28
FILL = 2048
GUARD = 2048                  # samples of code 4095 on either side of a capture

table = GC.table


def m_values(runs=400):
    """The capture sizes every shape is run at.  M % 28 in {2, 14, 26}: a last run clipped near its start, in its middle and near its
    end; 28 is a multiple of 4, so each of these has M % 4 == 2 -- the clipped piece ends in a HALF group, completed with code 2048.
    M % 4 == 0 cannot go with those remainders: it is covered at M % 28 in {0, 4, 16, 24}, where a clipped piece ends in a whole
    group (and at 0 nothing is clipped).  -> [M]"""
    return [28 * runs + r for r in (2, 14, 26, 0, 4, 16, 24)]


def words12(lo, hi):
    return -(-12 * -(-(hi - lo) // 4) // 16)


# ------------------------------------------------------------------ the literal loop
def slow_layout12(tab, M):
    off = [0]
    for r in tab:
        lo, hi = RUN * int(r["begin"]), min(RUN * int(r["end"]), M)
        groups = 0
        while 4 * groups < hi - lo:
            groups += 1
        nxt = off[-1] + 12 * groups
        while nxt % 16:
            nxt += 1
        off.append(nxt)
    return off


def slow_gather12(x, tab, M):
    """Bit by bit, from the format's words: a group of 8 samples is ONE 96-bit big-endian number s0 .. s7, 12 bits each, kept as three
    little-endian 32-bit words.  -> (a list of byte values, the offsets, over)."""
    off = slow_layout12(tab, M)
    out = [0] * off[-1]
    over = 0
    for r, at in zip(tab, off):
        lo, hi = RUN * int(r["begin"]), min(RUN * int(r["end"]), M)
        own = [int(v) for v in x[2 * lo:2 * hi]]
        over += sum(v > 4095 for v in own)
        while len(own) % 8:
            own.append(FILL)
        for g in range(len(own) // 8):
            big = 0
            for v in own[8 * g:8 * g + 8]:
                big = (big << 12) | (v & 0xFFF)
            for w in range(3):
                word = (big >> (32 * (2 - w))) & 0xFFFFFFFF
                for b in range(4):
                    out[at + 12 * g + 4 * w + b] = (word >> (8 * b)) & 0xFF
    return out, off, over


# ------------------------------------------------------------------ captures
def codes(n, seed, top=4096):
    """n uint16 codes 1 .. top - 1, never 0 and never a multiple of 4096 in their low bits alone."""
    return np.random.default_rng([seed, n]).integers(1, top, n, dtype=np.uint16)


def guarded(x):
    """4095 ... | capture | 4095 ... -> (samples, sample offset of the capture: a multiple of 8, so 16 bytes)."""
    g = np.full(GUARD, 4095, np.uint16)
    return np.concatenate([g, x, g]), GUARD


def n_for(M, tail=0):
    """A capture length with 2 (n // 4) == M: 2 M + tail, tail in 0 .. 3 (M is even)."""
    assert M % 2 == 0 and 0 <= tail < 4
    return 2 * M + tail


# ------------------------------------------------------------------ the named cases
def named_cases(C, M):
    """The shapes of the issue's list for chunks of C words on a capture of M power samples (about 400 runs or more)."""
    R = -(-M // 28)                                           # runs, the last perhaps clipped
    out = [("no burst", table([]))]
    out.append(("the whole capture", table([(0, R)])))
    # pieces of 1, 2, 3 and 4 runs: 5.25, 10.5, 15.75 and 21 words -- every word phase meets a piece end
    pairs, r = [], 1
    for k in range(60):
        length = 1 + k % 4
        if r + length >= R - 2:
            break
        pairs.append((r, r + length))
        r += length + 1 + k % 2
    out.append(("pieces of 1, 2, 3 and 4 runs", table(pairs)))
    out.append(("... from begin = 0, the last one clipped", table([(0, 1), (2, 4), (5, 8), (9, 13), (R - 1, R)])))
    out.append(("... the last one reaching far beyond M", table([(0, 3), (R - 3, 1 << 30)])))
    # a piece per second run over 3 C + 5 words: every chunk holds many pieces and ends inside one
    n = -(-(3 * C + 5) // 6) + 1
    assert 2 * n < R
    out.append(("every second run a piece, over 3 C + 5 words", table([(2 * i, 2 * i + 1) for i in range(n)])))
    out.append(("every second run a piece, odd begins", table([(2 * i + 1, 2 * i + 2) for i in range(n)])))
    # one long piece between two of one run: chunks that lie inside one piece
    runs = 1
    while words12(0, 28 * runs) < 3 * C + 1:
        runs += 1
    assert runs + 8 < R
    for first in (0, 1):
        out.append((f"a piece of {words12(0, 28 * runs)} >= 3 C + 1 words between two of one run, from run {first + 2}",
                    table([(first, first + 1), (first + 2, first + 2 + runs), (first + 4 + runs, first + 5 + runs)])))
    # a last piece clipped to a half group (M % 4 == 2) or to whole groups (M % 4 == 0), alone and behind others
    out.append(("only a clipped last run", table([(R - 1, R)])))
    out.append(("a long piece up to the clipped end", table([(3, 4), (R - runs - 1, R + 5)])))
    return [(name, M, tab) for name, tab in out]


def random_tables(count, seed):
    """`count` seeded tables on captures of about 400 runs, M even: (M, table)."""
    out = []
    for M, tab in GC.random_tables(count, seed, runs=420):
        M -= M % 2
        tab = tab[28 * tab["begin"].astype(np.int64) < M]
        out.append((M, tab))
    return out


# ------------------------------------------------------------------ what the layout refuses
def refusals(M=28 * 20):
    """[(name, M, table, the record the message names)]: GC.refusals' tables (the gather's own sample_bytes rows left out)."""
    return [(name, M_, tab, word) for name, M_, s, tab, word in GC.refusals(M) if word != "sample_bytes"]
