"""The cases of the burst gather (adsb_gather_layout, adsb_gather_device; adsbdec_amd/burst_archive.py layout and gather are the
statement), shared by tests/test_gather_cpu.py and tests/test_gpu_gather.py.  No GPU and no reference here: burst tables aimed at
the kernel's chunk of C 16-byte output words (C = adsb_gather_chunk_words() is handed in; the CPU test takes a small stand-in, the
statement knows no chunk), the literal loop over pieces and bytes, loud captures, and the tables a call refuses.

A case is (name, M, table): M power samples, a burst table (levels.BURST_DTYPE).  It holds for every s in S_ALL."""
import numpy as np

S_ALL = (2, 4, 8)
RUN = 28
GUARD = 4096                  # bytes of loud decoy on either side of a capture


def table(pairs):
    """[(begin, end)] -> a burst table; hot and peak are whatever (the gather reads neither)."""
    from adsbdec_amd.levels import BURST_DTYPE
    t = np.zeros(len(pairs), dtype=BURST_DTYPE)
    for i, (b, e) in enumerate(pairs):
        t[i] = (b, e, 1 + i % 3, 100.0 + i)
    return t


def words(s, lo, hi):
    return -(-s * (hi - lo) // 16)


# ------------------------------------------------------------------ the literal loop
def slow_layout(tab, M, s):
    off = [0]
    for r in tab:
        lo, hi = RUN * int(r["begin"]), min(RUN * int(r["end"]), M)
        nxt = off[-1] + s * (hi - lo)
        while nxt % 16:
            nxt += 1
        off.append(nxt)
    return off


def slow_gather(capture, tab, M, s):
    """Byte by byte: -> (a list of ints, the offsets)."""
    cap = np.ascontiguousarray(capture).reshape(-1).view(np.uint8)
    off = slow_layout(tab, M, s)
    out = [0] * off[-1]
    for r, at in zip(tab, off):
        lo, hi = RUN * int(r["begin"]), min(RUN * int(r["end"]), M)
        for k in range(s * (hi - lo)):
            out[at + k] = int(cap[s * lo + k])
    return out, off


# ------------------------------------------------------------------ captures
def loud_bytes(n, seed):
    """n bytes, none of them zero: a pad byte that is not zero, or a byte from the wrong place, shows."""
    return np.random.default_rng([seed, n]).integers(1, 256, n, dtype=np.uint8)


def capture_bytes(M, s, seed, extra=0):
    """The s M bytes of a capture of M power samples (+ `extra` bytes of its own behind them: a real capture's trailing n % 4 samples)."""
    return loud_bytes(s * M + extra, seed)


def guarded(cap, seed=99):
    """decoy | capture | decoy -> (bytes, byte offset of the capture: a multiple of 16)."""
    g0, g1 = loud_bytes(GUARD, seed), loud_bytes(GUARD, seed + 1)
    return np.concatenate([g0, cap, g1]), GUARD


# ------------------------------------------------------------------ the named cases
def named_cases(C, s):
    """The shapes of the issue's list, 1 to 7, for chunks of C words and s bytes per power sample."""
    out = [("no burst", 28 * 40 + 5, table([]))]
    for rem in (0, 1, 14, 27):
        M = 28 * 50 + rem
        out.append((f"one burst that is the whole capture, M % 28 = {rem}", M, table([(0, -(-M // 28))])))
    out.append(("a burst with begin = 0, and others", 28 * 60, table([(0, 3), (5, 6), (9, 20), (59, 60)])))
    for rem in (1, 14, 27):
        M = 28 * 37 + rem
        out.append((f"the last burst clipped by M, M % 28 = {rem}", M, table([(1, 2), (4, 9), (30, 38)])))
        out.append((f"the last burst one clipped run, M % 28 = {rem}", M, table([(2, 5), (37, 38)])))
        out.append((f"the last burst reaches far beyond M, M % 28 = {rem}", M, table([(2, 5), (36, 1 << 30)])))
    # 5. every second run a piece: every chunk holds many pieces and ends inside one
    per = words(s, 0, 28)
    n = -(-(3 * C + 5) // per) + 1
    out.append(("every second run a piece, over 3 C + 5 words", 28 * 2 * n, table([(2 * i, 2 * i + 1) for i in range(n)])))
    out.append(("every second run a piece, odd begins", 28 * (2 * n + 1), table([(2 * i + 1, 2 * i + 2) for i in range(n)])))
    # 6. one long piece between two of one run: chunks that lie inside one piece
    runs = 1
    while words(s, 0, 28 * runs) < 3 * C + 1:
        runs += 1
    for first in (0, 1):
        out.append((f"a piece of {words(s, 0, 28 * runs)} >= 3 C + 1 words between two of one run, from run {first + 2}", 28 * (runs + 8),
                    table([(first, first + 1), (first + 2, first + 2 + runs), (first + 4 + runs, first + 5 + runs)])))
    # ... and exactly 3 C + 1 words, the last of them short: the table's last piece, clipped by M
    units = (16 * 3 * C) // s + 1
    out.append(("a last piece of exactly 3 C + 1 words, clipped", 28 * 3 + units, table([(0, 1), (3, 3 + -(-units // 28) + 2)])))
    # 7. both source alignment classes (s = 2: begin even and odd) with run counts even and odd (s = 2: pieces that are no multiple of 16)
    out.append(("begin even / odd x runs even / odd", 28 * 40, table([(0, 1), (3, 4), (6, 8), (11, 13), (14, 17), (19, 22), (24, 25)])))
    out.append(("begin odd first", 28 * 40, table([(1, 4), (7, 8), (10, 12)])))
    return out


def random_tables(count, seed, runs=4000):
    """`count` seeded tables on a capture of about `runs` runs: (M, table) -- densities from a few pieces to every second run, M with
    every remainder mod 28."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        R = int(rng.integers(runs - 200, runs + 200))
        M = 28 * (R - 1) + int(rng.integers(1, 29))
        density = float(rng.choice([0.002, 0.02, 0.2, 0.5]))
        pairs, r = [], int(rng.integers(0, 3))
        while r < R:
            length = int(rng.choice([1, 1, 2, 3, 7, 40])) if rng.random() < 0.9 else int(rng.integers(1, 300))
            pairs.append((r, min(r + length, R) if rng.random() < 0.95 else r + length + 5))
            r = pairs[-1][1] + 1 + int(rng.geometric(density))
        pairs = [(b, e) for b, e in pairs if 28 * b < M]
        out.append((M, table(pairs)))
    return out


# ------------------------------------------------------------------ what a call refuses
def refusals(M=28 * 20):
    """[(name, M, s, table, the record the message names)]"""
    ok = [(1, 3), (5, 8), (10, 12)]
    return [("sample_bytes 3", M, 3, table(ok), "sample_bytes"),
            ("sample_bytes 0", M, 0, table(ok), "sample_bytes"),
            ("sample_bytes 16", M, 16, table(ok), "sample_bytes"),
            ("end == begin", M, 4, table([(1, 3), (5, 5), (10, 12)]), "burst 1"),
            ("end < begin", M, 4, table([(1, 3), (5, 8), (12, 10)]), "burst 2"),
            ("28 begin == M", M, 2, table([(1, 3), (20, 21)]), "burst 1"),
            ("28 begin > M", M, 8, table([(1, 3), (5, 8), (10, 12), (4000, 4001)]), "burst 3"),
            ("first record outside", 10, 4, table([(1, 3)]), "burst 0"),
            ("neighbours touch", M, 4, table([(1, 3), (3, 8)]), "burst 1"),
            ("neighbours overlap", M, 4, table([(1, 3), (5, 8), (7, 12)]), "burst 2"),
            ("descending", M, 4, table([(5, 8), (1, 3)]), "burst 1")]
