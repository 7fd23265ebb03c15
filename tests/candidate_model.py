"""Host-only model of what the scan kernel hands over per offset: its tile geometry (scan_kernel.h), the greedy chain the
resolver runs over a candidate list (demod.c:86-143 as resolver.hpp restates it), and the never-visited filter that thins a
tile's CRC-valid candidates (scan_kernel.hip, "Drop candidates the greedy scan ... can never visit").  Plain Python and
numpy; tests/test_candidate_model_cpu.py pins it, tests/test_gpu_candidates.py holds the kernel to it.

A candidate is a tuple whose first element is its offset g and whose third is its frame bytes ((g, pw, frame, ...): the
oracle's scan_all records, or the C-ABI's candidates with their `reserved` flag appended)."""
from bisect import bisect_left

import numpy as np

# scan_kernel.h
RUN = 28
PASS_RUNS = 4 * 63
REACH_RUNS = 44
TAPER_PASSES = 4
CLIST_CAP = 256
DECOFFSET_K = 1200      # longest span an accepted frame jumps: the filter's guard is pg >= DECOFFSET_K - 1
ENTRY_REACH = 1200      # a shard's true entry lies in [g_begin, g_begin + 1200): where the filter must keep every chain


def owned_runs(passes):
    return PASS_RUNS * passes - REACH_RUNS


def tile_passes(tile, big_tiles, k):
    return k if (big_tiles == 0 or tile < big_tiles or k <= TAPER_PASSES) else TAPER_PASSES


def tile_first_run(tile, big_tiles, k):
    if big_tiles == 0 or tile <= big_tiles or k <= TAPER_PASSES:
        return tile * owned_runs(k)
    return big_tiles * owned_runs(k) + (tile - big_tiles) * owned_runs(TAPER_PASSES)


def tile_count(n_offsets, big_tiles, k):
    runs = (n_offsets + RUN - 1) // RUN
    head = big_tiles * owned_runs(k)
    if big_tiles == 0 or k <= TAPER_PASSES or runs <= head:
        return (runs + owned_runs(k) - 1) // owned_runs(k)
    return big_tiles + (runs - head + owned_runs(TAPER_PASSES) - 1) // owned_runs(TAPER_PASSES)


def tile_bounds(g_begin, g_end, passes, big_tiles=0):
    """[(first offset, one past the last)] of every tile of a launch over [g_begin, g_end)."""
    n = tile_count(g_end - g_begin, big_tiles, passes)
    return [(g_begin + RUN * tile_first_run(t, big_tiles, passes),
             min(g_end, g_begin + RUN * tile_first_run(t + 1, big_tiles, passes))) for t in range(n)]


def span(c):
    """Offsets an accepted frame jumps: 80 + 80 * bytes (demod.c:109,120,123): 640 or 1200."""
    return 80 + 80 * len(c[2])


def chain(cands, entry, end):
    """The greedy rule from `entry`: take the first candidate with g >= entry (and g < end), accept it, go on from
    g + span.  -> the accepted candidates."""
    gs = [c[0] for c in cands]
    out, i = [], bisect_left(gs, entry)
    while i < len(cands) and gs[i] < end:
        out.append(cands[i])
        i = bisect_left(gs, gs[i] + span(cands[i]), i + 1)
    return out


def equivalent_from(full, filtered, entries, end):
    """The entries from which the greedy chains over `full` and over `filtered` (both ascending in g) differ, up to `end`.
    A chain depends only on the first candidate at or after its entry, so the answer is memoised per pair of first
    candidates: after an accepted candidate both chains go on from the same offset."""
    fg, hg = [c[0] for c in full], [c[0] for c in filtered]
    memo = {}

    def first(gs, e):
        i = bisect_left(gs, e)
        return i if i < len(gs) and gs[i] < end else None

    def same(e):
        path, ok = [], None
        while True:
            key = (first(fg, e), first(hg, e))
            if key in memo:
                ok = memo[key]
                break
            path.append(key)
            i, j = key
            if i is None or j is None:
                ok = i is None and j is None
                break
            if full[i] != filtered[j]:
                ok = False
                break
            e = fg[i] + span(full[i])
        for key in path:
            memo[key] = ok
        return ok

    return [e for e in entries if not same(e)]


def filter_model(cands, g_begin, g_end, passes, big_tiles=0, clist_cap=CLIST_CAP, *, guard=DECOFFSET_K - 1,
                 spans=(640, 1200), use_complete=True, end_at_pg_counts=False, drop_nothing=False):
    """The never-visited filter of one launch over [g_begin, g_end), applied to its CRC-valid candidates (ascending).
    -> (kept candidates, staged entries per tile).  Per tile: the staged list is the tile's own candidates; with more than
    `clist_cap` of them it is incomplete and nothing is dropped.  Else c goes when c' (the closest staged candidate before
    it) lies at tile-local pg >= guard, c.g < c'.g + span(c'), and no staged candidate's end g + span lies in (c'.g, c.g].
    The keywords after * are the rule's deliberate mutations (tests/test_candidate_model_cpu.py): they must be caught."""
    sp_short, sp_long = spans
    g = np.array([c[0] for c in cands], dtype=np.int64)
    lng = np.array([len(c[2]) == 14 for c in cands], dtype=bool)
    keep = np.ones(len(cands), dtype=bool)
    counts = []
    for t0, t1 in tile_bounds(g_begin, g_end, passes, big_tiles):
        lo, hi = int(np.searchsorted(g, t0)), int(np.searchsorted(g, t1))
        n = hi - lo
        counts.append(n)
        if drop_nothing or (use_complete and n > clist_cap):
            continue
        idx = np.arange(lo, hi)
        if n > clist_cap:   # (mutation use_complete=False: the kernel stages clist_cap of them, in no particular order)
            idx = np.sort(np.random.default_rng(t0).choice(idx, clist_cap, replace=False))
        if idx.size < 2:
            continue
        gi = g[idx] - t0
        sp = np.where(lng[idx], sp_long, sp_short)
        ends = np.sort(gi + sp)
        pg, psp, c = gi[:-1], sp[:-1], gi[1:]     # c' of staged entries 1.. is the entry before
        # no end in (pg, c]  (mutation end_at_pg_counts: in [pg, c])
        e_hi = np.searchsorted(ends, c, side="right")
        e_lo = np.searchsorted(ends, pg, side="left" if end_at_pg_counts else "right")
        drop = (pg >= guard) & (c < pg + psp) & (e_hi == e_lo)
        keep[idx[1:][drop]] = False
    return [c for c, k in zip(cands, keep) if k], counts


def regimes(counts, clist_cap=CLIST_CAP):
    """Tiles per implementation of the filter: (<= 64 staged: readlane path, 65-128: LDS with two threads per entry,
    129-256: LDS with one, more than clist_cap: incomplete list, nothing dropped)."""
    r = [0, 0, 0, 0]
    for n in counts:
        r[3 if n > clist_cap else 0 if n <= 64 else 1 if n <= 128 else 2] += 1
    return r


# ---------------------------------------------------------------- captures (shared by the CPU and the GPU file)
def _placed(starts, dfs, rng, amp=(500.0, 1500.0), damage=False):
    from tools import gen_signal as G
    out = []
    for i, s in enumerate(starts):
        fr = bytearray(G.make_frame(dfs[i % len(dfs)], rng))
        if damage and len(fr) == 14 and i % 2 == 0:
            k = int(rng.integers(5, 112))
            fr[k >> 3] ^= 0x80 >> (k & 7)
        out.append((int(s), bytes(fr), float(rng.uniform(*amp)), float(rng.uniform(0, 2 * np.pi))))
    return out


def make_captures(n=1 << 20):
    """{name: uint16 capture of n samples}: the cases where candidate lists go wrong -- sparse, dense and overlapping,
    noise, uniform full-range codes, saturated and DC stretches under frames, a gate storm, frames back to back, short
    frames back to back, one-bit-damaged long frames.  Deterministic."""
    from tools import gen_signal as G
    assert n % 8 == 0
    caps = {}
    caps["sparse"] = G.sparse_capture(n, n // 6000, seed=301, sigma=8.0, dfs=(17, 18, 11))[0]
    caps["dense"] = G.dense_capture(n, seed=302, sigma=40.0, n_frames=n // 1400, amp=(200, 1800))[0]
    caps["noise"] = G.dense_capture(n, seed=303, sigma=200.0, n_frames=n // 6000)[0]
    caps["uniform"] = np.random.default_rng(304).integers(0, 65536, size=n, dtype=np.uint16)
    rng = np.random.default_rng(305)
    x = G.synth(n, _placed(np.arange(4000, n - 3000, 3100), (17, 11, 18), rng), 10.0, 305)
    q = n // 8
    x[q:2 * q] = 0
    x[3 * q:4 * q] = 4095
    x[5 * q:6 * q] = 65535
    x[6 * q:7 * q] = 2048
    x[q + 5000:q + 7400] = G.synth(2400, _placed([0], (17,), rng), 0.0, 1)   # a frame on top of a flat stretch
    caps["saturated"] = x
    storm = np.tile(G._frame_start_wave(), n // 260 + 1)[:n]
    x = G.synth(n, _placed(np.arange(6000, n - 3000, 9000), (17, 11), rng), 30.0, 306).astype(np.float32)
    x[n // 4:3 * n // 4] += storm[n // 4:3 * n // 4]
    caps["gate_storm"] = np.clip(np.rint(x), 0, 4095).astype(np.uint16)
    caps["back_to_back"] = G.synth(n, _placed(np.arange(3000, n - 2600, 2400), (17, 18, 11), np.random.default_rng(307)),
                                   6.0, 307)
    caps["short_frames"] = G.synth(n, _placed(np.arange(3000, n - 1400, 1280), (11,), np.random.default_rng(308)), 6.0, 308)
    caps["damaged"] = G.synth(n, _placed(np.arange(3000, n - 2600, 2700), (17, 18), np.random.default_rng(309), damage=True),
                              8.0, 309)
    return caps
