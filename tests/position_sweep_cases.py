"""The captures, the sweeps and the coverage accounting that hold every scan kernel to the oracle at EVERY tile-relative offset
of a scan tile: tests/test_position_sweep_cpu.py asserts, from the oracle and candidate_model alone, that the sweeps reach what
they are for; tests/test_gpu_position_sweep.py runs them on the device.  No GPU here.

A scan kernel evaluates an offset at a position inside its tile (the run, and the bit r = g mod 28 inside the run's plane words),
and most special cases of scan_stages.h are special by position.  The oracle's answer for an offset does not depend on where a
launch's tiles begin, so the sweeps keep the samples and move the tiles: a stream scan over [28 j, end) for every j in
[0, owned_runs(K)), a batch whose capture j is the same pattern behind 28 j offsets of exact quiet.  A shift is a multiple of 28:
a record at offset g lands on the tile-relative offset (g -+ 28 j) mod 28 owned_runs(K), and over all j it visits every run at
its own r.  So the sweeps reach every tile-relative offset with a kind of record exactly when that kind occurs at all 28 residues
r -- behind LEAD, where no shift has passed it.  coverage() counts it cell by cell all the same, from the lists and the shifts.

The pattern: LEAD = 28 owned_runs(7) offsets that carry no frame, then 28 DF17 / DF18 frames and 28 DF11 frames 1316 = 47 * 28
offsets apart, frame i nudged by i mod 28 offsets, and one more DF17 frame whose last candidate is the capture's last offset.
The first QUIET offsets are exact quiet (code 2048, IQ 0, power 0.0), so a quiet prefix in front changes no offset's answer."""
import functools
import time
from bisect import bisect_left

import numpy as np

import candidate_model as M
import front_records_cases as F
from test_batch_cpu import offsets_of, power_samples

RUN = M.RUN
LEAD = RUN * M.owned_runs(7)                  # 48 160: every shift of a K <= 7 tile keeps the pattern inside the window
FIRST = 2016                                  # 72 runs behind LEAD
STEP = 1316                                   # 47 runs: a long frame is 1 200 offsets
N_FRAMES = 56                                 # 28 long, then 28 short: i mod 28 takes every value for both
N_SWEEP = 252_936                             # real samples; 126 468 complex or power samples
G_MAX = N_SWEEP // 2 - 1195                   # 125 273 offsets
QUIET = 256                                   # offsets of exact quiet at the pattern's head (a preamble and its DF bits span 130)
WINDOW = 1196
SECONDS = {}

# the stream sweeps of scan_kernel: (id, K, df18, collect_stats).  K = 2 runs with statistics off too: the other Stage B.
SWEEPS = (("k2", 2, True, True), ("k3_df11_17", 3, False, True), ("k7", 7, True, True), ("k2_nostats", 2, True, False))
BATCH_K = 2
BATCH_SHIFTS = M.owned_runs(BATCH_K)          # 460 captures a call
BATCH_FRONTS = ("real", "iq", "iq8", "power")
DIRECT_SHIFTS = (0, 1, 27, 459)               # where the shift-derived expectations are held to the oracle directly

# the damaged capture: 10 * 107 long frames, frame i damaged in bit 5 + i mod 107 and nudged by 3 (i // 107) -- a damaged frame is
# repairable at three consecutive offsets or more, so every bit meets every r
N_DAMAGED = 10 * 107
LEAD_DAMAGED = RUN * M.owned_runs(2)          # swept at K = 2 only
N_DAMAGED_SAMPLES = 2 * (LEAD_DAMAGED + FIRST + STEP * N_DAMAGED + 1200 + 28) // 8 * 8


def shifts(k):
    return range(M.owned_runs(k))


def frame_offsets(n_frames=N_FRAMES, lead=LEAD, nudge=lambda i: i % RUN):
    """The offset each planted frame starts at."""
    return [lead + FIRST + STEP * i + nudge(i) for i in range(n_frames)]


def planted(seed, starts=None, dfs=None, damage=False):
    """[(start offset, frame, amplitude, phase)]: amplitudes 500 .. 1500; long frames alternate DF17 / DF18, the short ones behind
    them are DF11.  damage: long frame i has bit 5 + i mod 107 flipped."""
    from tools import gen_signal as G
    rng = np.random.default_rng(seed)
    starts = frame_offsets() if starts is None else starts
    out = []
    for i, s in enumerate(starts):
        df = dfs(i) if dfs else (11 if i >= 28 else 17 + i % 2)
        fr = bytearray(G.make_frame(df, rng))
        if damage:
            k = 5 + i % 107
            fr[k >> 3] ^= 0x80 >> (k & 7)
        out.append((int(s), bytes(fr), float(rng.uniform(500.0, 1500.0)), float(rng.uniform(0, 2 * np.pi))))
    return out


def _with_end_frame(frames, seed, at):
    """... and a DF17 frame at offset `at` (the end frame: its last candidate is the capture's last offset)."""
    from tools import gen_signal as G
    rng = np.random.default_rng(seed + 1)
    return frames + [(at, G.make_frame(17, rng), 1100.0, 1.1)]


def real_capture(frames, n, sigma, seed):
    """uint16 capture at 20 MS/s: a frame at offset s starts at sample 2 s; the head is exact quiet."""
    from tools import gen_signal as G
    x = G.synth(n, [(2 * s, fr, amp, phi) for s, fr, amp, phi in frames], sigma, seed)
    x[:2 * QUIET] = 2048
    return x


def iq_capture(frames, n, sigma, seed):
    """int16 IQ capture at 10 MS/s, shape (n, 2): a frame at offset s starts at complex sample s; the head is exact quiet."""
    from tools import gen_signal as G
    x = G.iq_synth(n, frames, sigma, seed)
    x[:QUIET] = 0
    return x


def sweep_capture(seed=7001, frames=None):
    """The sweep capture: N_SWEEP real samples."""
    frames = planted(seed) if frames is None else frames
    return real_capture(_with_end_frame(frames, seed, G_MAX - 1 - 6), N_SWEEP, 6.0, seed)


def damaged_capture(seed=7002):
    starts = frame_offsets(N_DAMAGED, LEAD_DAMAGED, lambda i: 3 * (i // 107))
    return real_capture(planted(seed, starts, dfs=lambda i: 17 + i % 2, damage=True), N_DAMAGED_SAMPLES, 6.0, seed)


# ---------------------------------------------------------------- the oracle's lists
class Lists:
    """One capture's exhaustive evaluation: a (its power samples), n_off, raw[df18] = oracle.scan_all's (candidates, tries) -- what
    test_gpu_candidates._window slices --, ev[df18] = the same with reserved = 0 appended to every candidate, g[df18] = the
    candidates' offsets, tg[df18] = the tries' offsets (both ascending)."""

    def __init__(self, oracle, a, n_off):
        self.a, self.n_off = a, n_off
        self.raw, self.ev, self.g, self.tg = {}, {}, {}, {}
        for df18 in (False, True):
            cands, tries = oracle.scan_all(a, 0, n_off, df18)
            self.raw[df18] = (cands, tries)
            self.ev[df18] = ([c + (0,) for c in cands], tries)
            self.g[df18] = [c[0] for c in cands]
            self.tg[df18] = (tries >> np.uint64(2)).astype(np.int64)
            assert self.g[df18] == sorted(self.g[df18]) and np.all(np.diff(self.tg[df18]) > 0)


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def sweep():
    """(the sweep capture, its Lists): evaluated once per process."""
    O = _oracle()
    t0 = time.perf_counter()
    x = sweep_capture()
    a = O.power(x)
    assert a.size - 1195 == G_MAX == offsets_of(x.size)
    out = (x, Lists(O, a, G_MAX))
    SECONDS["sweep"] = time.perf_counter() - t0
    return out


@functools.lru_cache(maxsize=None)
def damaged():
    """(the damaged capture, its Lists, the records fix_1bit adds (front_records_cases.repairable), every record ascending, the
    repaired bit of each added record)."""
    O = _oracle()
    t0 = time.perf_counter()
    x = damaged_capture()
    a = O.power(x)
    L = Lists(O, a, offsets_of(x.size))
    fixed = F.repairable(O, a, *L.ev[True])
    tab = F._syndromes()
    bits = []
    for g, _, fr, _ in fixed:
        _, sliced, _ = O.eval_offset(a, g, True)
        bits.append(tab[O.crc_residual(sliced)])
    out = (x, L, fixed, sorted(L.ev[True][0] + fixed), bits)
    SECONDS["damaged"] = time.perf_counter() - t0
    return out


# ---------------------------------------------------------------- the sweeps of scan_kernel
def first_samples(j):
    """The buffer starts a start-sweep scan rotates over: the highest first_sample adsb_scan_shard accepts for g_begin = 28 j,
    that minus 8, that minus 8 000 (not below 0).  -> the one of shift j; the rule has period 3 * 28, not 2."""
    gb = RUN * j
    top = (2 * (gb - 6)) // 8 * 8 if gb >= 6 else 0
    return max(0, top - (0, 8, 8000)[(j + j // RUN) % 3])


def frame_groups(L, df18=True, lo=LEAD):
    """The runs of consecutive candidate offsets at or behind `lo`: one per planted frame."""
    groups = []
    for g in L.g[df18]:
        if g < lo:
            continue
        if groups and g == groups[-1][-1] + 1:
            groups[-1].append(g)
        else:
            groups.append([g])
    return groups


def end_sweep(L):
    """[(g_begin, g_end, first_sample, n of the exact buffer)] of the end sweep (K = 2): per planted frame with candidates c0 .. cm,
    g_end = c0, c0 + 1, .. cm + 1 (cut at the capture's end) behind g_begin = 28 floor((c0 - 1300) / 28): the frame lies in the
    launch's last tile, the last wave's window leaves [p_lo, p_hi) over the frame's own bits."""
    out = []
    for grp in frame_groups(L):
        gb = RUN * ((grp[0] - 1300) // RUN)
        fs = (2 * (gb - 6)) // 8 * 8
        for ge in range(grp[0], min(grp[-1] + 1, L.n_off) + 1):
            out.append((gb, ge, fs, 2 * (ge - 1 + WINDOW) - fs))
    return out


def head_sweep(L):
    """[(g_begin, first_sample)] of the head sweep (K = 2): per planted frame with candidates c0 .. cm, g_begin = 28 floor(c0 / 28)
    and, where the frame's candidates straddle a multiple of 28, that multiple -- the frame's candidates are the first records of
    tile 0, with the buffer starting at the highest first_sample the call accepts, six pairs in front of them.  (The start sweep
    keeps LEAD in front of the frames: at K = 2 and 3 its tile 0 holds none.)"""
    out = []
    for grp in frame_groups(L):
        for gb in sorted({RUN * (grp[0] // RUN), RUN * (grp[-1] // RUN)}):
            out.append((gb, (2 * (gb - 6)) // 8 * 8))
    return out


def coverage(gs, k, js=None, batch=False):
    """Hits per tile-relative offset of a K tile (-> int array of 28 owned_runs(K)) over the shifts js (default: every j in
    [0, owned_runs(K))) for records at offsets gs.  A stream scan [28 j, end) holds the records at g >= 28 j, at (g - 28 j) mod
    28 owned_runs(K); capture j of a batch holds them all, at (g + 28 j) mod 28 owned_runs(K)."""
    t = RUN * M.owned_runs(k)
    gs = np.asarray(gs, dtype=np.int64)
    hits = np.zeros(t, dtype=np.int64)
    for j in (shifts(k) if js is None else js):
        rel = gs + RUN * j if batch else gs[gs >= RUN * j] - RUN * j
        hits += np.bincount(rel % t, minlength=t)
    return hits


def kinds(L, df18):
    """{kind: offsets} of a capture's records: long and short candidates, DF11 / DF17 / DF18 tries."""
    cands, tries = L.ev[df18]
    out = {"long": [c[0] for c in cands if len(c[2]) == 14], "short": [c[0] for c in cands if len(c[2]) == 7]}
    code = (tries & np.uint64(3)).astype(np.int64)
    for c, df in enumerate((11, 17, 18)):
        if df != 18 or df18:
            out[f"try{df}"] = L.tg[df18][code == c]
    return out


def check_coverage(L, k, df18, js=None, batch=False):
    """Every tile-relative offset of a K tile is the offset of a record of every kind.  -> {kind: fewest hits per offset}."""
    fewest = {}
    for kind, gs in kinds(L, df18).items():
        hits = coverage(gs, k, js, batch)
        fewest[kind] = int(hits.min())
        assert fewest[kind] >= 1, (kind, k, df18, int(np.count_nonzero(hits == 0)), int(np.argmin(hits)))
    return fewest


def tiles_reached(L, k, df18):
    """Which tiles of the start sweep's scans hold candidates: {"first", "interior", "last"} (candidate_model.tile_bounds)."""
    g = np.array(L.g[df18], dtype=np.int64)
    seen = set()
    for j in shifts(k):
        tb = M.tile_bounds(RUN * j, L.n_off, k)
        for t, (t0, t1) in enumerate(tb):
            if np.searchsorted(g, t1) > np.searchsorted(g, t0):
                seen.add("first" if t == 0 else "last" if t == len(tb) - 1 else "interior")
    return seen


@functools.lru_cache(maxsize=None)
def kept_lists(sweep_id):
    """What the never-visited filter leaves of every scan of a start sweep: [candidate_model.filter_model's kept list of the scan
    [28 j, end) for j in shifts(K)], from the oracle's candidates."""
    _, k, df18, _ = next(s for s in SWEEPS if s[0] == sweep_id)
    L = sweep()[1]
    cands, g = L.ev[df18][0], L.g[df18]
    return [M.filter_model(cands[bisect_left(g, RUN * j):], RUN * j, L.n_off, k)[0] for j in shifts(k)]


def where(k, j, g, batch=False):
    """What a failing record's position class is read from: K, the shift, the offset, r = g mod 28 and the tile-relative run."""
    rel = int(g) + RUN * j if batch else int(g) - RUN * j
    return f"K={k} j={j} g={int(g)} r={int(g) % RUN} run={(rel // RUN) % M.owned_runs(k)}"


def first_difference(k, j, got, want, batch=False):
    """where() of the first record that is in one list and not in the other (None: the lists hold the same records)."""
    odd = sorted(set(got) ^ set(want))
    return where(k, j, odd[0][0], batch) if odd else None


def first_try_difference(k, j, got, want, batch=False):
    odd = np.setxor1d(got, want)
    return where(k, j, int(odd[0]) >> 2, batch) if odd.size else None


# ---------------------------------------------------------------- the batch patterns
class Pattern:
    """One front end's pattern: x (what is pushed, the quiet prefix excluded), quiet (one quiet sample), per (samples per offset),
    n (samples), L (its Lists), and dec(j) = (n_j, candidates, tries, frames, stats) expected of capture j."""

    def expected(self, j, df18=True):
        """(sample count, candidates, tries, frames, stats) of capture j -- the pattern behind 28 j offsets of quiet -- derived
        from the unshifted pattern's lists: moved by 28 j, cut at the capture's own n_offsets, decoded by the greedy model."""
        s = RUN * j
        n = self.n + self.per * s
        n_off = self.offsets(n)
        cands = [(c[0] + s,) + c[1:] for c in self.L.ev[df18][0] if c[0] + s < n_off]
        tries = self.L.ev[df18][1] + np.uint64(s << 2)
        tries = tries[(tries >> np.uint64(2)) < np.uint64(n_off)]
        frames, stats, _ = F.greedy(cands, tries, self.power_count(n))
        return n, cands, tries, frames, stats

    def shifted(self, j):
        """Capture j as an array of its own (the CPU test's direct oracle; the device holds overlapping views of one buffer)."""
        s = self.per * RUN * j
        return np.concatenate([np.full((s,) + self.x.shape[1:], self.quiet, self.x.dtype), self.x])


@functools.lru_cache(maxsize=None)
def pattern(front):
    """The pattern of a batch front end: "real" (the sweep capture), "iq" (int16 IQ at 10 MS/s, G.iq_synth of the same geometry),
    "iq8" (int8 IQ: the same at amplitudes that fit, quantised with >> 8), "power" (oracle.power of the real one)."""
    from adsbdec_amd.sample_formats import iq_power, to_int8_iq
    O = _oracle()
    t0 = time.perf_counter()
    p = Pattern()
    p.front = front
    if front == "real":
        p.x, p.L = sweep()
        p.quiet, p.per = 2048, 2
        p.offsets, p.power_count = offsets_of, power_samples
        p.power_of = O.power
    else:
        p.per = 1
        p.offsets = F.n_offsets
        p.power_count = lambda n: n - (n & 1)
        if front == "power":
            p.x = np.ascontiguousarray(sweep()[1].a)
            p.quiet, a = np.float32(0.0), p.x
            p.power_of = lambda x: x
        else:
            seed = 7003 if front == "iq" else 7004
            frames = _with_end_frame(planted(seed), seed, G_MAX - 1 - 4)
            x = iq_capture(frames, N_SWEEP // 2, 6.0 if front == "iq" else 20.0, seed)
            p.quiet = 0
            if front == "iq":
                p.x, p.power_of = x, iq_power
            else:
                p.x, p.power_of = np.ascontiguousarray(to_int8_iq(x)[0]), (lambda x: iq_power(x, 8))
            a = p.power_of(p.x)
        p.L = Lists(O, a, G_MAX)
    p.n = int(len(p.x))
    assert p.offsets(p.n) == G_MAX and p.L.a.size == p.power_count(p.n)
    assert not p.L.a[:QUIET - 16].any()                      # exact quiet is exact 0.0 in power
    SECONDS[front] = time.perf_counter() - t0
    return p
