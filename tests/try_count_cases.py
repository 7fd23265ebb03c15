"""The try-count pass of a statistics run, try by try: the definition adsb::count_tries_kernel is held to (csrc/scan_kernel.h, the
comment above TryCountArgs) in numpy on uint64, and the cases that reach the kernel's branches.  tests/test_try_count_cpu.py asserts,
from the model and the tile geometry alone, that every case reaches what it says it is for; tests/test_gpu_try_count.py runs the
cases on the device through adsb_count_tries_alone.  Nothing here shares code with the kernel; the tile geometry is
tests/candidate_model.py's.

A PASS is what one launch of the kernel is given (class Pass).  Try words: (g - g_base) << 2 | code in the tile regions and in the
launch-wide list, (g << 2) | code in 64 bits in the carry lists.  Every builder is deterministic and returns (passes or pass,
what): `what` says what the case is for, in figures that measure() computes again from the arrays."""
import numpy as np

import candidate_model as M
from candidate_model import tile_bounds, tile_first_run

U64 = np.uint64
REGION = 4096            # try words per tile region (scan_kernel.h kTryRegion)
COUNT_THREADS = 256      # threads of a block of the count kernel (scan_kernel.hip kCountThreads)
REGION_GRID = 256        # blocks that walk the regions, four tiles each, grid-stride (scan_kernel.hip kCountRegionGrid)
MAX_SPAN = M.DECOFFSET_K
FRAME = np.dtype([("g", "<u8"), ("span", "<u4"), ("pad", "<u4")])          # TryFrame, 16 bytes
SOURCES = ("region", "list", "carry")
COUNTED, SHADOWED, CARRIED, DROPPED = range(4)
FATES = ("counted", "shadowed", "carried", "dropped")
BEYOND = 1 << 40         # a `hi` beyond every launch of the cases


class Pass:
    """g_base, passes, big_tiles, n_tiles, g_end (the launch's tiles cover [g_base, g_end)), frames (FRAME), regions / region_counts
    (uint32, or None / None), tries (uint32: the list), carry_in (uint64), n_carry, hi, final, carry_cap."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Result:
    """acc (three counts), carried (every appended word, sorted), n_carry_out, overflow, and per try: g, code, src, fate."""


def frames_array(g, span):
    f = np.zeros(len(g), FRAME)
    f["g"], f["span"] = np.asarray(g, U64), np.asarray(span, np.uint32)
    return f


def geometry(p):
    """[(t0, t1)] of the launch's tiles."""
    return tile_bounds(p.g_base, p.g_end, p.passes, p.big_tiles) if p.n_tiles else []


def launch_end(g_base, k, big, n_tiles):
    return g_base + M.RUN * tile_first_run(n_tiles, big, k)


def check_contract(p):
    """What the kernel may rely on (scan_kernel.h): frames ascending, not overlapping, spans 1..1200; a region's tries inside its
    tile; list words of 30 bits of offset; every index inside its array."""
    fg, sp = p.frames["g"], p.frames["span"].astype(U64)
    assert ((sp >= 1) & (sp <= MAX_SPAN)).all()
    assert (fg[1:] >= fg[:-1] + sp[:-1]).all()
    assert 2 <= p.passes <= 32 and p.tries.dtype == np.uint32 and p.carry_in.dtype == U64
    assert p.carry_in.size >= min(p.n_carry, p.carry_cap) and (p.carry_cap > 0 or p.final)
    assert (p.tries >> 2 < 1 << 30).all()
    if p.regions is None:
        assert p.region_counts is None and p.n_tiles == 0
        return
    bounds = geometry(p)
    assert len(bounds) == p.n_tiles and p.regions.size == p.n_tiles * REGION and p.region_counts.size == p.n_tiles
    for t, (t0, t1) in enumerate(bounds):
        n = min(int(p.region_counts[t]), REGION)
        g = p.g_base + (p.regions[t * REGION:t * REGION + n].astype(np.int64) >> 2)
        assert n == 0 or (g.min() >= t0 and g.max() < t1), t


def tries_of(p):
    """Every try the pass is given: (g uint64, code, source index into SOURCES)."""
    gs, cs, ss = [], [], []
    if p.regions is not None:
        for t in range(p.n_tiles):
            w = p.regions[t * REGION:t * REGION + min(int(p.region_counts[t]), REGION)].astype(U64)
            gs.append(U64(p.g_base) + (w >> U64(2)))
            cs.append(w & U64(3))
            ss.append(np.zeros(w.size, np.uint8))
    w = p.tries.astype(U64)
    gs.append(U64(p.g_base) + (w >> U64(2)))
    cs.append(w & U64(3))
    ss.append(np.full(w.size, 1, np.uint8))
    w = p.carry_in[:min(p.n_carry, p.carry_cap)]
    gs.append(w >> U64(2))
    cs.append(w & U64(3))
    ss.append(np.full(w.size, 2, np.uint8))
    return np.concatenate(gs).astype(U64), np.concatenate(cs).astype(np.int64), np.concatenate(ss)


def shadowed_by_search(p, g):
    """Shadowed iff the last frame that starts below g reaches beyond it (the frames do not overlap: no other frame can)."""
    fg = p.frames["g"]
    if fg.size == 0:
        return np.zeros(g.size, bool)
    fe = fg + p.frames["span"].astype(U64)
    k = np.searchsorted(fg, g, side="left")                # frames that start below g
    return (k > 0) & (g < fe[np.maximum(k, 1) - 1])


def shadowed_brute(p, g):
    """The definition as it stands: some frame has g_f < g < g_f + span_f."""
    fg = p.frames["g"]
    fe = fg + p.frames["span"].astype(U64)
    out = np.zeros(g.size, bool)
    for i in range(0, g.size, 64):
        x = g[i:i + 64, None]
        out[i:i + 64] = ((fg[None, :] < x) & (x < fe[None, :])).any(axis=1)
    return out


def model(p, brute=None):
    """The definition.  With fewer than 2 000 tries the brute-force form is evaluated too and must agree."""
    g, code, src = tries_of(p)
    late = g >= U64(p.hi)
    sh = shadowed_by_search(p, g)
    if brute is None:
        brute = g.size < 2000
    if brute:
        assert np.array_equal(sh, shadowed_brute(p, g))
    fate = np.where(late, DROPPED if p.final else CARRIED, np.where(sh, SHADOWED, COUNTED))
    r = Result()
    r.g, r.code, r.src, r.fate = g, code, src, fate
    r.acc = [int(np.count_nonzero((fate == COUNTED) & (np.minimum(code, 2) == k))) for k in range(3)]
    c = fate == CARRIED
    r.carried = np.sort((g[c] << U64(2)) | code[c].astype(U64))
    r.n_carry_out = int(r.carried.size)
    r.overflow = r.n_carry_out > p.carry_cap
    return r


def list_grid(p):
    """Blocks of the launch that walk the list and the carry-in, and the trips of their grid-stride loop: launch_count_tries'
    formula (csrc/scan_kernel.hip, `const uint32_t guess = args.n_tries + 65536u` and the three lines below it), restated once."""
    n_tries = int(p.tries.size)
    guess = n_tries + 65536
    cap = min(1024, max(64, n_tries // 2048)) if p.regions is not None else 2048
    blocks = min((guess + COUNT_THREADS - 1) // COUNT_THREADS, cap)
    entries = n_tries + min(p.n_carry, p.carry_cap)
    return blocks, -(-entries // (blocks * COUNT_THREADS))


def measure(p, r=None):
    """What a pass reaches, from the model and the geometry alone.  windows[t]: frames that start in [max(t0 - 1199, 0), t1);
    fits[t]: the wave holds the window -- fewer than 64, or no 65th frame, or the 65th starts at or beyond t1; next_rel[t]: where
    that 65th frame starts, relative to t1 (None: there is none, or the window has fewer than 64); boundary[path][k]: decided tries
    at g_f, g_f + 1, g_f + span - 1, g_f + span of a frame of span >= 3, per look-up path ("window": a region try of a tile that
    fits; "search": everything else); fates[source][fate]."""
    r = r or model(p)
    fg = p.frames["g"].astype(np.int64)        # (the cases that measure windows lie below 2^63)
    sp = p.frames["span"].astype(np.int64)
    out = dict(windows=[], fits=[], next_rel=[], region_blocks=0, region_trips=0)
    bounds = geometry(p)
    for t0, t1 in bounds:
        key = max(t0 - (MAX_SPAN - 1), 0)
        lo, hi = int(np.searchsorted(fg, key)), int(np.searchsorted(fg, t1))
        nxt = int(fg[lo + 64]) - t1 if lo + 64 < fg.size else None
        out["windows"].append(hi - lo)
        out["fits"].append(hi - lo < 64 or nxt is None or nxt >= 0)
        out["next_rel"].append(nxt if hi - lo >= 64 else None)
    if bounds:
        out["region_blocks"] = -(-p.n_tiles // 4)
        out["region_trips"] = -(-out["region_blocks"] // REGION_GRID)
    out["list_blocks"], out["list_trips"] = list_grid(p)
    g = r.g.astype(np.int64)
    path = np.full(g.size, 1)                  # 0 window, 1 search
    if bounds:
        t0s = np.array([b[0] for b in bounds])
        tile = np.clip(np.searchsorted(t0s, g, side="right") - 1, 0, len(bounds) - 1)
        path[(r.src == 0) & np.array(out["fits"])[tile]] = 0
    decided = r.fate <= SHADOWED
    pos = np.full(g.size, -1)
    if fg.size:
        j = np.searchsorted(fg, g, side="right") - 1          # the last frame that starts at or below g
        ok = (j >= 0) & (sp[np.maximum(j, 0)] >= 3)
        d = g - fg[np.maximum(j, 0)]
        pos[ok & (d == 0)] = 0
        pos[ok & (d == 1)] = 1
        pos[ok & (d == sp[np.maximum(j, 0)] - 1)] = 2
        j = np.searchsorted(fg, g, side="left") - 1           # the last frame that starts below g
        ok = (j >= 0) & (sp[np.maximum(j, 0)] >= 3) & (g == fg[np.maximum(j, 0)] + sp[np.maximum(j, 0)])
        pos3 = ok
    else:
        pos3 = np.zeros(g.size, bool)
    out["boundary"] = {name: [int(np.count_nonzero(decided & (path == k) & (pos == q))) for q in range(3)] +
                       [int(np.count_nonzero(decided & (path == k) & pos3))] for k, name in enumerate(("window", "search"))}
    out["fates"] = {name: [int(np.count_nonzero((r.src == s) & (r.fate == f))) for f in range(4)] for s, name in enumerate(SOURCES)}
    out["codes"] = [int(np.count_nonzero((r.fate == COUNTED) & (r.code == c))) for c in range(4)]
    return out


# ---------------------------------------------------------------- building blocks
def place(rng, lo, hi, spans, tight=0.3):
    """Starts of frames with the given spans inside [lo, hi), in order, not overlapping: the free room is shared out at random
    between them, about a share `tight` of the frames directly behind the one before (g + span is the next frame's own offset)."""
    spans = np.asarray(spans, np.int64)
    n = spans.size
    if n == 0:
        return np.zeros(0, np.int64)
    slack = (hi - lo) - int(spans.sum())
    assert slack >= 0, (lo, hi, n, int(spans.sum()))
    w = rng.random(n) + 1e-9
    w[1:][rng.random(n - 1) < tight] = 0.0
    gaps = np.floor(w / w.sum() * slack).astype(np.int64)
    return lo + np.cumsum(gaps) + np.concatenate([[0], np.cumsum(spans[:-1])])


def spans_small(rng, n):
    """{1, 2, 7, 200} in rotation plus one 640 and one 1200, shuffled; one frame alone is a 1200."""
    if n < 2:
        return np.full(n, MAX_SPAN, np.int64)
    return rng.permutation(np.array([640, 1200] + [(1, 2, 7, 200)[i % 4] for i in range(n - 2)], np.int64))


def spans_mix(rng, n, room):
    """n spans out of {1, 2, 7, 200, 640, 1200} that fill at most 70 % of `room`: mostly short ones where room is scarce."""
    rich = room >= 150 * max(n, 1)
    pr = (0.3, 0.3, 0.25, 0.1, 0.03, 0.02) if rich else (0.35, 0.35, 0.28, 0.015, 0.003, 0.002)
    s = rng.choice(np.array([1, 2, 7, 200, 640, 1200], np.int64), size=n, p=pr)
    assert int(s.sum()) <= 0.7 * room or n == 0, (n, room, int(s.sum()))
    return s


def edge_offsets(fg, sp, pick):
    """g_f, g_f + 1, g_f + span - 1 and g_f + span of the picked frames."""
    fg, sp = np.asarray(fg, np.int64)[pick], np.asarray(sp, np.int64)[pick]
    return np.concatenate([fg, fg + 1, fg + sp - 1, fg + sp])


def exactly(rng, first, lo, hi, n):
    """n distinct offsets of [lo, hi): those of `first` that lie inside, in order, then random ones."""
    first = np.asarray(first, np.int64)
    first = first[(first >= lo) & (first < hi)]
    _, at = np.unique(first, return_index=True)
    have = first[np.sort(at)][:n]
    while have.size < n:
        more = rng.integers(lo, hi, size=2 * (n - have.size) + 16)
        both = np.concatenate([have, more])
        _, at = np.unique(both, return_index=True)
        have = both[np.sort(at)][:n]
    return have


def make_pass(rng, g_base, k, big, n_tiles, frames, tg, route, hi, final, carry_cap=None, g_end=None, region_cap=REGION):
    """Deal the tries at the offsets tg (codes 0..3, shuffled) to the three sources.  route: "regions" (every try of a tile into
    that tile's region in shuffled order, what exceeds region_cap words and what lies beyond the tiles onto the list), "list" (n_tiles
    = 0), "carry", "mixed" (60 / 20 / 20 %), or an array of source indices.  A try below g_base can only be carried in."""
    tg = np.asarray(tg, np.int64)
    n = tg.size
    tc = rng.permutation(np.arange(n) % 4)
    if isinstance(route, str):
        want = {"regions": np.zeros(n, int), "list": np.ones(n, int), "carry": np.full(n, 2),
                "mixed": rng.choice(3, size=n, p=(0.6, 0.2, 0.2))}[route]
        if route in ("list", "carry"):
            n_tiles = 0
    else:
        want = np.asarray(route).copy()
    p = Pass(g_base=int(g_base), passes=k, big_tiles=big, n_tiles=n_tiles, frames=frames, hi=int(hi), final=int(final))
    p.g_end = int(g_end) if g_end is not None else launch_end(p.g_base, k, big, n_tiles)
    want[tg < p.g_base] = 2
    want[(want < 2) & (tg - p.g_base >= 1 << 30)] = 2
    word = ((tg - p.g_base) << 2) | tc
    p.regions = p.region_counts = None
    if n_tiles:
        bounds = geometry(p)
        assert len(bounds) == n_tiles
        p.regions = rng.integers(0, 1 << 32, size=n_tiles * REGION, dtype=np.uint32)     # what lies behind a count is never read
        p.region_counts = np.zeros(n_tiles, np.uint32)
        inside = np.flatnonzero((want == 0) & (tg >= p.g_base) & (tg < p.g_end))
        inside = inside[rng.permutation(inside.size)]
        tile = np.searchsorted(np.array([b[0] for b in bounds]), tg[inside], side="right") - 1
        order = np.argsort(tile, kind="stable")
        inside, tile = inside[order], tile[order]
        first = np.searchsorted(tile, np.arange(n_tiles + 1))
        for t in range(n_tiles):
            mine = inside[first[t]:first[t + 1]]
            keep = mine[:region_cap]
            p.regions[t * REGION:t * REGION + keep.size] = word[keep].astype(np.uint32)
            p.region_counts[t] = keep.size
            want[mine[region_cap:]] = 1
        want[(want == 0) & ((tg < p.g_base) | (tg >= p.g_end))] = 1
    else:
        want[want == 0] = 1
    at = np.flatnonzero(want == 1)
    p.tries = word[at[rng.permutation(at.size)]].astype(np.uint32)
    at = np.flatnonzero(want == 2)
    at = at[rng.permutation(at.size)]
    p.carry_in = ((tg[at].astype(U64) << U64(2)) | tc[at].astype(U64)).astype(U64)
    p.n_carry = int(at.size)
    p.carry_cap = int(carry_cap) if carry_cap is not None else n + 16
    check_contract(p)
    return p


ROUTES = ("regions", "list", "carry")


# ---------------------------------------------------------------- 1. window edges
WINDOW_COUNTS = (1, 127, 4095, 4096, 129, 128)          # region words per tile


def window_edges(d, route):
    """K = 2, six tiles whose windows hold 0, 1, 63, 64 (+ the probe), 65 and 64 frames.  The probe frame starts at t1 + d of
    tile 3 (d = -1, 0, 1): the 65th frame behind tile 3's window of 64, and the first of tile 4's window of 65 (which the wave
    cannot hold: the binary search).  Tile 5's 64 frames are the last of the array.  The same frames and tries for every route."""
    rng = np.random.default_rng(7100 + d)
    k, n_tiles, g_base = 2, 6, 28 * 4000
    end = launch_end(g_base, k, 0, n_tiles)
    bounds = tile_bounds(g_base, end, k)
    own = (0, 1, 63, 64, 64, 64)
    fg, sp = [], []
    for t, (t0, t1) in enumerate(bounds):
        s = spans_small(rng, own[t])
        if own[t] >= 4:                                        # the window's first and last frame can shadow a try: 7 and 200
            for at, want in ((0, 7), (-1, 200)):
                j = int(np.flatnonzero(s == want)[1])
                s[at], s[j] = s[j], s[at]
        fg.append(place(rng, t0 + (16 if t == 4 else int(rng.integers(0, 3))), t1 - 1300, s))
        sp.append(s)
        if t == 3:
            fg.append(np.array([t1 + d]))
            sp.append(np.array([7]))
    fg, sp = np.concatenate(fg), np.concatenate(sp)
    tg = []
    for t, (t0, t1) in enumerate(bounds):
        mine = np.flatnonzero((fg >= t0 - 1300) & (fg < t1))
        pick = mine if mine.size <= 16 else np.unique(np.concatenate([mine[:2], mine[-2:], mine[sp[mine] >= 640], rng.choice(mine, 10)]))
        tg.append(exactly(rng, np.concatenate([[t0, t1 - 1], edge_offsets(fg, sp, pick)]), t0, t1, WINDOW_COUNTS[t]))
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), np.concatenate(tg), route, BEYOND, 0)
    what = dict(windows=[0, 1, 63, 64 + (d < 0), 65, 64], fits=[True, True, True, d >= 0, False, True], next_rel_tile3=d,
                counts=list(WINDOW_COUNTS))
    return p, what


# ---------------------------------------------------------------- 2. a frame in front of the tile and of the launch
FRONT_BASES = (0, 28, 1176, 1204, (1 << 32) - 28 * 300, (1 << 33) + 28, 1 << 35)
FRONT_KINDS = ("reaches_t0", "ends_at_t0", "short")


def front_frames(g_base, kind, route, hi=BEYOND):
    """K = 2, three tiles.  In front of t0 of tile 0 and of tile 2: a frame at t0 - 1199 of span 1200 (shadows t0 and nothing else
    of the tile), one at t0 - 1200 of span 1200 (shadows nothing of it) or one at t0 - 1 of span 2 (shadows t0).  Where t0 is
    below that distance the frame starts at offset 0 and ends at the same place; at t0 = 0 there is no offset in front."""
    rng = np.random.default_rng(7200 + FRONT_BASES.index(g_base) * 8 + FRONT_KINDS.index(kind))
    k, n_tiles = 2, 3
    end = launch_end(g_base, k, 0, n_tiles)
    bounds = tile_bounds(g_base, end, k)
    fg, sp, tg, probes = [], [], [], []
    for t in (0, 2):
        b = bounds[t][0]
        if b > 0:
            if kind == "reaches_t0":
                g = max(b - 1199, 0)
                s = b + 1 - g
            elif kind == "ends_at_t0":
                g = max(b - 1200, 0)
                s = b - g
            else:
                g, s = b - 1, 2
            fg.append(g)
            sp.append(s)
            tg += [g - 1, g, g + 1, g + s - 1, g + s]
            probes.append((b, kind != "ends_at_t0"))
        tg += [b - 2, b - 1, b, b + 1, b + 2]
    for t0, t1 in bounds:                                      # and a few frames well inside every tile
        s = spans_small(rng, 5)
        g = place(rng, t0 + 2000, t1 - 2500, s)
        fg += list(g)
        sp += list(s)
        tg += list(edge_offsets(g, s, np.arange(5)))
    order = np.argsort(fg)
    fg, sp = np.array(fg, np.int64)[order], np.array(sp, np.int64)[order]
    tg = np.array(tg, np.int64)
    tg = exactly(rng, tg[tg >= g_base], g_base, end, 120)
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, route, hi, 0)
    return p, dict(probes=probes)


# ---------------------------------------------------------------- 3. hi
HI_KINDS = ("below_base", "at_base", "at_try", "in_span", "beyond")


def _hi_scene(rng, per_tile):
    k, n_tiles, g_base = 2, 4, 28 * 5000
    end = launch_end(g_base, k, 0, n_tiles)
    sp = spans_small(rng, 120)
    fg = place(rng, g_base + 3, end - 3, sp)
    tg = exactly(rng, edge_offsets(fg, sp, rng.choice(120, 40, replace=False)), g_base, end, per_tile * n_tiles)
    return k, n_tiles, g_base, end, fg, sp, tg


def hi_case(kind, final, route):
    """K = 2, four tiles, 120 frames, 2 400 tries.  hi below the launch's base and at it (everything is undecided), equal to the
    offset of a try of tile 1 whose lower neighbour is a try too, inside the span of a 1200 frame with tries on both sides of it, and
    beyond the launch."""
    rng = np.random.default_rng(7300)                          # one scene for every kind, final and route
    k, n_tiles, g_base, end, fg, sp, tg = _hi_scene(rng, 600)
    bounds = tile_bounds(g_base, end, k)
    long_one = int(np.flatnonzero(sp == 1200)[0])
    at_try = bounds[1][0] + 5000
    in_span = int(fg[long_one]) + 600
    tg = np.unique(np.concatenate([tg, [at_try - 1, at_try, in_span - 1, in_span, in_span + 1]]))
    hi = dict(below_base=g_base - 5, at_base=g_base, at_try=at_try, in_span=in_span, beyond=end + 777)[kind]
    rng = np.random.default_rng(7301 + ROUTES.index(route) if route in ROUTES else 7310)
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, route, hi, final)
    return p, dict(hi=hi, at=(hi - 1, hi) if kind in ("at_try", "in_span") else None, all_late=kind in ("below_base", "at_base"),
                   none_late=kind == "beyond")


def carry_overflow(n_late):
    """carry_cap = 100 and exactly n_late undecided tries, from all three sources (60 of the pass's tries come in by the carry)."""
    rng = np.random.default_rng(7400 + n_late)
    k, n_tiles, g_base, end, fg, sp, tg = _hi_scene(rng, 1500)
    want = rng.choice(2, size=tg.size, p=(0.7, 0.3))
    want[rng.choice(tg.size, 60, replace=False)] = 2
    hi = int(np.sort(tg)[-n_late])
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, want, hi, 0, carry_cap=100)
    return p, dict(n_late=n_late, cap=100)


def carry_count_above_cap():
    """*n_carry = 500 on input with carry_cap = 463: the last 37 entries are not read."""
    rng = np.random.default_rng(7450)
    k, n_tiles, g_base, end, fg, sp, tg = _hi_scene(rng, 125)
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, "carry", int(np.sort(tg)[400]), 0, carry_cap=463)
    return p, dict(n_carry=500, cap=463)


# ---------------------------------------------------------------- 4. geometry
GEOMETRIES = ((2, 0, 1), (2, 0, 3), (2, 0, 5), (2, 0, 8), (2, 0, 1030), (7, 0, 5), (7, 1, 5), (7, 3, 6), (32, 0, 3))


def geometry_case(k, big, n_tiles):
    """One frame and a few tries around every tile boundary: at every other boundary b a frame at b - 1199 of span 1200 (a try of
    the tile behind b is shadowed by a frame that starts as far in front of it as a frame can), at the others a frame at b - 3 of
    span 7 (tries of both tiles are shadowed by a frame that starts in the last offsets of the tile in front)."""
    rng = np.random.default_rng(7500 + 100 * k + 10 * big + n_tiles % 7)
    g_base = 28 * 100
    end = launch_end(g_base, k, big, n_tiles)
    bounds = tile_bounds(g_base, end, k, big)
    edges = [b[0] for b in bounds] + [end]
    fg, sp, tg = [], [], []
    for i, b in enumerate(edges):
        if i % 2 == 0:
            fg.append(b - 1199)
            sp.append(1200)
            tg += [b - 1, b, b + 1]
        else:
            fg.append(b - 3)
            sp.append(7)
            tg += [b - 4, b - 2, b - 1, b, b + 3, b + 4]
    tg = np.array(tg, np.int64)
    p = make_pass(rng, g_base, k, big, n_tiles, frames_array(fg, sp), np.unique(tg[tg >= g_base]), "regions", BEYOND, 1)
    return p, dict(tile_offsets=sorted({b[1] - b[0] for b in bounds}, reverse=True), region_blocks=-(-n_tiles // 4),
                   region_trips=-(-(-(-n_tiles // 4)) // REGION_GRID), ragged=n_tiles % 4)


def region_count_above_cap():
    """Tile 0's count says 5 000 with a full region of 4096 words; tile 1's region, the 904 words behind, holds tile 1's tries."""
    rng = np.random.default_rng(7600)
    k, n_tiles, g_base = 2, 3, 28 * 7
    end = launch_end(g_base, k, 0, n_tiles)
    bounds = tile_bounds(g_base, end, k)
    sp = spans_small(rng, 90)
    fg = place(rng, g_base + 1, end - 1, sp)
    tg = np.concatenate([exactly(rng, [], *bounds[0], REGION), exactly(rng, [], *bounds[1], 1000), exactly(rng, [], *bounds[2], 50)])
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, "regions", BEYOND, 1)
    assert list(p.region_counts) == [REGION, 1000, 50]
    p.region_counts[0] = 5000
    check_contract(p)
    return p, dict(count=5000, behind=1000)


# ---------------------------------------------------------------- 5. the list and carry trips, the frame array's size
FRAME_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 300_000)


def _frames_over(rng, n, lo, hi):
    """n frames inside [lo, hi), the first of span 7 and the last of span 200."""
    sp = spans_mix(rng, n, hi - lo)
    if n:
        sp[0], sp[-1] = 7, 200
    return place(rng, lo, hi, sp), sp


def _ends(fg, sp, lo, hi):
    """One try below the first frame, one above the last, one shadowed by the first and one by the last frame."""
    return [lo, hi - 1] + ([int(fg[0]) + 1, int(fg[-1]) + 1] if len(fg) else [])


def list_trips():
    """Regions present (three K = 2 tiles) and a list of 20 000 words, most of them beyond the tiles: 64 blocks of 256 threads, a
    second trip."""
    rng = np.random.default_rng(7700)
    k, n_tiles, g_base = 2, 3, 28 * 11
    end = launch_end(g_base, k, 0, n_tiles)
    far = g_base + 300_000
    fg, sp = _frames_over(rng, 4097, g_base + 50, far - 50)
    tg = exactly(rng, _ends(fg, sp, g_base + 10, far - 10) + list(edge_offsets(fg, sp, rng.choice(4097, 300, replace=False))), g_base, far, 20_300)
    want = np.ones(tg.size, int)
    inside = np.flatnonzero(tg < end)
    want[inside[:300]] = 0
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, want, BEYOND, 1)
    return p, dict(list_words=20_000, list_blocks=64, list_trips=2)


def carry_trips():
    """No regions, no list, 70 000 carried-in tries: 256 blocks of 256 threads, a second trip; a third of them is carried on."""
    rng = np.random.default_rng(7710)
    g_base, far = 28 * 13, 28 * 13 + 400_000
    fg, sp = _frames_over(rng, 4096, g_base + 50, far - 50)
    tg = exactly(rng, _ends(fg, sp, g_base + 10, far - 10) + list(edge_offsets(fg, sp, rng.choice(4096, 300, replace=False))), g_base, far, 70_000)
    p = make_pass(rng, g_base, 2, 0, 0, frames_array(fg, sp), tg, "carry", int(np.sort(tg)[46_000]), 0, carry_cap=70_016)
    return p, dict(carry_words=70_000, list_blocks=256, list_trips=2)


def frame_counts(n_frames):
    """A frame array of n_frames entries under all three sources at once.  Up to 4 097 frames: five K = 7 tiles; about 300 000:
    sixty K = 32 tiles, two of them thinned to 40 frames a window, so that the wave's 64-way search over the whole array ends in a
    window that fits as well as in one that does not."""
    rng = np.random.default_rng(7800 + n_frames % 1000)
    big_array = n_frames > 10_000
    k, n_tiles, g_base = (32, 60, 28 * 17) if big_array else (7, 5, 28 * 17)
    end = launch_end(g_base, k, 0, n_tiles)
    fg, sp = _frames_over(rng, n_frames, g_base + 50, end - 50)
    thin = (3, 17) if big_array else ()
    bounds = tile_bounds(g_base, end, k)
    for t in thin:
        mine = np.flatnonzero((fg >= bounds[t][0] - 1199) & (fg < bounds[t][1]))
        drop = np.setdiff1d(mine, rng.choice(mine, 40, replace=False))
        fg, sp = np.delete(fg, drop), np.delete(sp, drop)
    n = len(fg)
    pick = rng.choice(n, min(n, 200), replace=False) if n else np.zeros(0, int)
    first = _ends(fg, sp, g_base + 10, end - 10) + list(edge_offsets(fg, sp, pick))
    for t in thin:                                             # tries of the thinned tiles: around their own 40 frames
        mine = np.flatnonzero((fg >= bounds[t][0]) & (fg < bounds[t][1]))
        first += list(edge_offsets(fg, sp, mine))
    tg = exactly(rng, first, g_base, end, 6000)
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg, "mixed", end + 1000, 0)
    return p, dict(n_frames=n, thin=list(thin))


# ---------------------------------------------------------------- 6. real traffic
REPLAY_KINDS = ("gate_storm", "back_to_back", "short_frames", "damaged")


def capture_lists(c, df18):
    """(frame offsets, spans, try offsets, try codes, end of the last visited range) of a front_records_cases Case."""
    frames = c.dec[(df18, False)][0]
    fg = np.array([f["g"] for f in frames], np.int64)
    sp = np.array([M.span((f["g"], f["pw"], bytes(f["frame"]))) for f in frames], np.int64)
    w = np.asarray(c.ev[df18][1], U64)
    assert (np.diff((w >> U64(2)).astype(np.int64)) > 0).all()                  # one try word per offset at the most
    return fg, sp, (w >> U64(2)).astype(np.int64), (w & U64(3)).astype(np.int64), int(c.end[df18])


REPLAY_REGION_CAP = {2: REGION, 7: 256}


def _replay_pass(rng, g_base, g_end, k, fg, sp, tg, tc, hi, final, cap):
    """The tries of the launch [g_base, g_end) dealt into its tiles' regions, the overflow onto the list; codes as they are.  No
    tile of these captures has 4096 tries, so at K = 7 a region takes 256 and the rest goes where overflow goes."""
    at = np.flatnonzero((tg >= g_base) & (tg < g_end))
    n_tiles = M.tile_count(g_end - g_base, 0, k) if at.size else 0
    p = make_pass(rng, g_base, k, 0, n_tiles, frames_array(fg, sp), tg[at], "regions" if n_tiles else "list", hi, final, carry_cap=cap,
                  g_end=g_end, region_cap=REPLAY_REGION_CAP[k])
    # make_pass shuffles codes of its own: put the capture's back, word by word
    code = dict(zip(tg[at].tolist(), tc[at].tolist()))

    def recode(words):
        g = g_base + (words.astype(np.int64) >> 2)
        return ((words & ~np.uint32(3)) | np.array([code[x] for x in g.tolist()], np.uint32)).astype(np.uint32) if words.size else words
    p.tries = recode(p.tries)
    for t in range(n_tiles):
        n = int(p.region_counts[t])
        p.regions[t * REGION:t * REGION + n] = recode(p.regions[t * REGION:t * REGION + n])
    check_contract(p)
    return p


def replay_single(c, df18, k):
    fg, sp, tg, tc, end = capture_lists(c, df18)
    rng = np.random.default_rng(7900 + k)
    return [_replay_pass(rng, 0, max(c.n_off, 28), k, fg, sp, tg, tc, end, 1, tg.size + 16)]


def replay_his(fg, sp, end):
    """The two intermediate positions of a three-pass replay: the end of the frame a third of the way, and the middle of the span
    of the frame two thirds of the way (without three frames: a third and two thirds of the way to the end)."""
    n = len(fg)
    if n < 3 or int(fg[n // 3] + sp[n // 3]) >= int(fg[2 * n // 3]):
        return end // 3, 2 * end // 3
    return int(fg[n // 3] + sp[n // 3]), int(fg[2 * n // 3] + sp[2 * n // 3] // 2)


def replay_three(c, df18, k):
    """Three launches and three passes.  Launch j ends 3 000 offsets behind pass j's position hi_j (rounded up to a run), so its
    last tries are carried; pass j is given the frames below hi_j that no earlier pass was given, behind the last one that was.
    The carry-in of passes 1 and 2 is filled in by chain()."""
    fg, sp, tg, tc, end = capture_lists(c, df18)
    rng = np.random.default_rng(7950 + k)
    n_off = max(c.n_off, 28)
    h1, h2 = replay_his(fg, sp, end)
    his = (h1, h2, end)
    cuts = [0] + [min(n_off, -(-(h + 3000) // 28) * 28) for h in (h1, h2)] + [n_off]
    passes, given = [], 0
    for j in range(3):
        upto = int(np.searchsorted(fg, his[j]))                 # frames that start below hi_j
        lo = max(given - 1, 0)
        upto = max(upto, given)
        if cuts[j + 1] > cuts[j]:
            p = _replay_pass(rng, cuts[j], cuts[j + 1], k, fg[lo:upto], sp[lo:upto], tg, tc, his[j], j == 2, tg.size + 16)
        else:
            p = make_pass(rng, cuts[j], k, 0, 0, frames_array(fg[lo:upto], sp[lo:upto]), [], "list", his[j], j == 2, carry_cap=tg.size + 16)
        given = upto
        passes.append(p)
    return passes


def chain(passes, run):
    """Run the passes in order, each one's carry-out the next one's carry-in; run(p) -> an object with .acc (this pass's three
    counts), .carried and .n_carry_out.  -> (summed counts, results)."""
    total, results, carried = [0, 0, 0], [], np.zeros(0, U64)
    for p in passes:
        p.carry_in, p.n_carry = np.asarray(carried, U64), int(len(carried))
        check_contract(p)
        r = run(p)
        assert r.n_carry_out <= p.carry_cap
        carried = r.carried
        total = [a + b for a, b in zip(total, r.acc)]
        results.append(r)
    return total, results
