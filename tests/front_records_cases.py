"""The captures, the oracle's lists and the table of configurations that hold the IQ and the power scan kernels to the oracle
record by record: tests/test_front_records_cpu.py asserts, from the oracle and the layout alone, that the cells reach what they
are for; tests/test_gpu_front_records.py runs them on the device.  Modelled on tests/test_gpu_batch_records.py, whose table,
capture order and helpers are imported, not restated.

A front end is "iq" (int16 I, Q: what adsb_*_iq takes as fmt 2) or "power" (float32 power samples: adsb_*_power).  The reference
is the oracle on the power array the library defines for the input: sample_formats.iq_power(x) for IQ, the array itself for
power.  Sizes count complex / power samples: 2^17 per kind is 129 877 offsets, 11 tiles at K = 2 and 3 at K = 7."""
import functools
import time
from bisect import bisect_left

import numpy as np

import candidate_model as M
from test_batch_cpu import APBUFFSZ, DECOFFSET, check_layout, launch_limit, offsets_of
from test_gpu_batch_records import CONFIGS as BATCH_CONFIGS, EDGES, NAMED_CUTS, _order, _pieces
from test_power_cpu import SCALES, TINY, scaled

FRONTS = ("iq", "power")
N = 1 << 17
N_EDGE = 42_000                               # the edge captures: 40 805 offsets, as the real-sample module's
KINDS = ("sparse", "dense", "noise", "uniform", "saturated", "gate_storm", "back_to_back", "short_frames", "damaged")
STREAM_KINDS = ("gate_storm", "back_to_back", "damaged")
SECONDS = {}                                  # what cases() took per front end: the first test that asks pays it

# (id, Decoder keywords, launch limit of the cut batch run or None: a cell of the stream kernels only).  The batch rows are those
# of tests/test_gpu_batch_records.py; the knobs behind them mean something to the stream kernels alone.
CONFIGS = [c for c in BATCH_CONFIGS] + [
    ("k7_big1", dict(df18=True, collect_stats=True, debug_passes=7, debug_big_tiles=1), None),
    ("k7_big3", dict(df18=True, collect_stats=False, debug_passes=7, debug_big_tiles=3), None),
    ("k7_nostream", dict(df18=False, collect_stats=True, debug_passes=7, debug_no_streaming=1), None),
    ("k7_trycap", dict(df18=True, collect_stats=True, debug_passes=7, debug_try_cap=64), None),
]
IDS = [c[0] for c in CONFIGS]
BATCH_CELLS = [i for i, c in enumerate(CONFIGS) if c[2] is not None]


def units(n):
    """The sample count the batch layout is asked at for a capture of n complex or power samples: 16-bit units, the trailing
    odd sample dropped ("A batch drops a capture's trailing odd sample before the layout")."""
    return 4 * (n // 2)


def n_offsets(n):
    return offsets_of(units(n))


# ---------------------------------------------------------------- captures
def _iq_kinds(n):
    """The nine kinds of candidate_model.make_captures as int16 IQ at 10 MS/s (shape (n, 2)): starts and spacings are half the
    real ones'.  Deterministic."""
    from tools import gen_signal as G
    P = M._placed
    caps = {}
    rng = np.random.default_rng(501)
    caps["sparse"] = G.iq_synth(n, P(np.sort(rng.integers(0, n - 1300, n // 3000)), (17, 18, 11), rng), 4.0, 501)
    rng = np.random.default_rng(502)
    caps["dense"] = G.iq_synth(n, P(np.sort(rng.integers(0, n - 1300, n // 700)), (17, 18, 11), rng, amp=(200.0, 1800.0)), 20.0, 502)
    rng = np.random.default_rng(503)
    caps["noise"] = G.iq_synth(n, P(np.sort(rng.integers(0, n - 1300, n // 3000)), (17, 18, 11), rng), 100.0, 503)
    caps["uniform"] = np.random.default_rng(504).integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    rng = np.random.default_rng(505)
    x = G.iq_synth(n, P(np.arange(2000, n - 1500, 1550), (17, 11, 18), rng), 5.0, 505)
    q = n // 8
    x[q:2 * q] = 0
    x[3 * q:4 * q] = 32767
    x[5 * q:6 * q] = -32768
    x[6 * q:7 * q] = (1000, -700)
    x[q + 2500:q + 3700] = G.iq_synth(1200, P([0], (17,), rng), 0.0, 1)          # a frame on top of a flat stretch
    caps["saturated"] = x
    # preamble and the five DF17 bits at 10 MS/s, 130 samples, back to back over the middle half, under sparse frames
    env = np.zeros(130)
    for s0 in (0, 10, 35, 45):
        env[s0:s0 + 5] = 1.0
    for i, b in enumerate((1, 0, 0, 0, 1)):
        s0 = 80 + 10 * i + (0 if b else 5)
        env[s0:s0 + 5] = 1.0
    storm = np.tile(env, n // 130 + 1)[:n]
    storm[:n // 4] = 0
    storm[3 * n // 4:] = 0
    x = G.iq_synth(n, P(np.arange(3000, n - 1500, 4500), (17, 11), rng), 15.0, 506).astype(np.float64)
    x[:, 0] += 16.0 * 900.0 * np.cos(0.7) * storm
    x[:, 1] += 16.0 * 900.0 * np.sin(0.7) * storm
    caps["gate_storm"] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    caps["back_to_back"] = G.iq_synth(n, P(np.arange(1500, n - 1300, 1200), (17, 18, 11), np.random.default_rng(507)), 3.0, 507)
    caps["short_frames"] = G.iq_synth(n, P(np.arange(1500, n - 700, 640), (11,), np.random.default_rng(508)), 3.0, 508)
    caps["damaged"] = G.iq_synth(n, P(np.arange(1500, n - 1300, 1350), (17, 18), np.random.default_rng(509), damage=True), 4.0, 509)
    assert tuple(caps) == KINDS
    return caps


def _iq_edge(i):
    """42 000 + i complex samples (n % 4 = 0, 1, 2, 3, 0): a DF17 frame from sample 0 on -- candidates at the first offsets -- and
    one whose last candidate is the last offset: its window ends with the capture's last sample that is seen."""
    from tools import gen_signal as G
    rng = np.random.default_rng(5100 + i)
    n = N_EDGE + (i if i < 4 else 8)
    last = n_offsets(n) - 1
    return G.iq_synth(n, [(0, G.make_frame(17, rng), 1200.0, 0.3), (last - 4, G.make_frame(17, rng), 1100.0, 1.1)], 3.0, 5100 + i)


def _power_kinds(oracle, n):
    """The nine kinds as general floats: the FIR's power samples of the real kinds (the two that leave the power domain in
    12-bit versions), the SCALES rotated over them, one stretch of `saturated` tiny or subnormal."""
    real = dict(M.make_captures(2 * n))
    real["uniform"] = np.random.default_rng(604).integers(0, 4096, size=2 * n, dtype=np.uint16)
    x = real["saturated"].copy()
    q = 2 * n // 8
    x[5 * q:6 * q] = np.where((np.arange(q) // 2) % 2, 4095, 0)               # (for the stretch of 65 535: full scale at fs / 4)
    real["saturated"] = x
    assert all(int(v.max()) <= 4095 for v in real.values())
    caps = {}
    for i, name in enumerate(KINDS):
        a = scaled(oracle.power(real[name]), SCALES[(i + 2) % len(SCALES)])
        if name == "saturated":                              # a stretch of frames in noise: every product tiny, thousands subnormal
            tiny = slice(n // 2, n // 2 + n // 16)
            a[tiny] = scaled(a[tiny], TINY)
            assert float(a[tiny].max()) < 1e-30 and np.count_nonzero((a[tiny] > 0) & (a[tiny] < np.finfo(np.float32).tiny)) > 1000
        assert a.size == n
        caps[name] = a
    return caps


def _captures(oracle, front):
    """{name: what is pushed} in the order of the device buffer: an edge capture directly behind `noise` and behind `uniform`
    (a loud tail), the others in a row, the capture without offsets last."""
    from adsbdec_amd.sample_formats import iq_power
    kinds = _iq_kinds(N) if front == "iq" else _power_kinds(oracle, N)
    edges = [_iq_edge(i) for i in range(5)]
    if front == "power":
        edges = [scaled(iq_power(x), SCALES[i % len(SCALES)]) for i, x in enumerate(edges)]
    caps = {}
    edge = iter(zip(EDGES, edges))
    for name, x in kinds.items():
        caps[name] = x
        if name in ("uniform", "noise"):
            e, y = next(edge)
            caps[e] = y
    for e, y in edge:
        caps[e] = y
    if front == "iq":
        caps["short"] = np.random.default_rng(5200).integers(-32768, 32768, size=(2051, 2), dtype=np.int16)
    else:
        caps["short"] = np.random.default_rng(5200).uniform(0, 2.0 ** 28, 2051).astype(np.float32)
    names = list(caps)
    assert names[names.index("edge0") - 1] == "noise" and names[names.index("edge1") - 1] == "uniform"
    assert {len(caps[e]) % 4 for e in EDGES} == {0, 1, 2, 3}
    return caps


# ---------------------------------------------------------------- the oracle's lists
@functools.lru_cache(maxsize=None)
def _syndromes():
    """{CRC residual of a long frame with only bit k set: k} for k in [5, 112): the residual is linear in the frame."""
    from oracle import oracle as O
    tab = {}
    for k in range(5, 112):
        fr = bytearray(14)
        fr[k >> 3] ^= 0x80 >> (k & 7)
        tab[O.crc_residual(bytes(fr))] = k
    assert len(tab) == 107 and 0 not in tab
    return tab


def repairable(oracle, a, cands, tries):
    """What fix_1bit adds to the list of a capture (df18 on): every offset whose try word is long (DF17 / DF18), whose sliced frame
    misses the CRC and has the syndrome of exactly one bit k in [5, 112) -> [(g, pw, the frame with bit k flipped, 1)], from the
    oracle's try words, eval_offset and crc_residual."""
    have = {c[0] for c in cands}
    tab = _syndromes()
    out = []
    for w in tries:
        g = int(w) >> 2
        if int(w) & 3 == 0 or g in have:
            continue
        k, fr, pw = oracle.eval_offset(a, g, True)
        assert k == 2 and len(fr) == 14, (g, k)
        bit = tab.get(oracle.crc_residual(fr))
        if bit is None:
            continue
        m = bytearray(fr)
        m[bit >> 3] ^= 0x80 >> (bit & 7)
        assert oracle.crc_residual(bytes(m)) == 0
        out.append((g, pw, bytes(m), 1))
    return out


def greedy(full, tries, m):
    """The reference's decode of m power samples (m even) from the per-offset lists: air.c:94-99's accumulate / carry around
    demod.c:84-144 -- a deqframe call whenever 40 980 samples or more are buffered, which visits the buffered offsets up to 1 200
    from its end, accepts the first candidate it meets and jumps behind it -- with ts counting the visited offsets and the Try
    row the try words at visited offsets.  `full`: (g, pw, frame, reserved), ascending.  -> (frames, stats with "fixed", the end of
    the last visited range: the position the decode stops at, 0 when it visits nothing).
    cases() holds it to oracle.demod_power on every capture; it is what says which frames a list WITH repaired records gives."""
    gs = [c[0] for c in full]
    frames, seen = [], []
    fed = aidx = gbase = ts = 0
    while True:
        add = (max(0, APBUFFSZ - aidx) + 1) // 2 * 2
        if fed + add > m:
            break
        fed += add
        aidx += add
        limit = gbase + aidx - DECOFFSET
        cur = gbase
        while cur < limit:
            i = bisect_left(gs, cur)
            if i < len(gs) and gs[i] < limit:
                c = full[i]
                ts += c[0] - cur + 1
                seen.append((cur, c[0] + 1))
                frames.append(dict(g=c[0], ts=ts, pw=c[1], frame=c[2], reserved=c[3]))
                cur = c[0] + M.span(c)
            else:
                ts += limit - cur
                seen.append((cur, limit))
                cur = limit
        aidx -= cur - gbase
        gbase = cur
    stats = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}, "fixed": sum(f["reserved"] for f in frames)}
    for f in frames:
        stats["ok"][f["frame"][0] >> 3] += 1
    if seen and tries.size:
        tg = (tries >> np.uint64(2)).astype(np.int64)
        lo, hi = np.array([s[0] for s in seen]), np.array([s[1] for s in seen])
        k = np.searchsorted(lo, tg, side="right") - 1
        vis = (k >= 0) & (tg < hi[np.maximum(k, 0)])
        for code, df in enumerate((11, 17, 18)):
            stats["try"][df] = int(np.count_nonzero(vis & ((tries & np.uint64(3)) == code)))
    return frames, stats, (seen[-1][1] if seen else 0)


def _records(frames):
    return [(f["g"], f["ts"], f["pw"], bytes(f["frame"])) for f in frames]


class Case:
    """One capture: x (what is pushed), a (its power samples), n, n_off, ev[df18] = (candidates with reserved = 0, tries) of every
    offset, dec[(df18, fix1)] = (frames, stats) of the greedy decode, end[df18] = where that decode's last visited range ends, fixed =
    the records fix_1bit adds (df18 on)."""


@functools.lru_cache(maxsize=None)
def cases(front):
    """{name: Case} of a front end in the order of the device buffer; evaluated once per process.  What the edge captures and the
    greedy model are for is asserted here, from the oracle alone."""
    from adsbdec_amd.sample_formats import iq_power, power_domain_ok
    from oracle import oracle as O
    O.build()
    t0 = time.perf_counter()
    out = {}
    for name, x in _captures(O, front).items():
        c = Case()
        c.x = np.ascontiguousarray(x)
        c.a = iq_power(x) if front == "iq" else c.x
        c.n = int(len(x))
        c.n_off = n_offsets(c.n)
        assert c.a.dtype == np.float32 and c.a.size == c.n and power_domain_ok(c.a), name
        assert c.n_off == 0 or c.n_off - 1 + 1195 < c.n
        c.ev, c.dec, c.end = {}, {}, {}
        m = c.n - (c.n & 1)
        for df18 in (False, True):
            cands, tries = O.scan_all(c.a, 0, c.n_off, df18)
            c.ev[df18] = ([r + (0,) for r in cands], tries)
            frames, stats = O.demod_power(c.a, df18=df18)
            c.dec[(df18, False)] = (frames, stats)
            mf, ms, c.end[df18] = greedy(c.ev[df18][0], tries, m)
            assert _records(mf) == _records(frames) and (ms["try"], ms["ok"], ms["fixed"]) == (stats["try"], stats["ok"], 0), (front, name, df18)
        c.fixed = repairable(O, c.a, *c.ev[True]) if c.n_off else []
        c.dec[(True, True)] = greedy(sorted(c.ev[True][0] + c.fixed), c.ev[True][1], m)[:2]
        out[name] = c
        if name in EDGES:
            gs = [r[0] for r in c.ev[True][0]]
            # no FIR in front of these kernels: an in-range offset reads its own capture only, so what loud neighbours can spoil
            # shows at the first and the last offsets -- which carry candidates
            assert gs[:4] == [0, 1, 2, 3] and gs[-4:] == list(range(c.n_off - 4, c.n_off)), (front, name, gs[:6], gs[-6:], c.n_off)
    assert out["short"].n_off == 0 and [n for n in out if n not in EDGES and n != "short"] == list(KINDS)
    SECONDS[front] = time.perf_counter() - t0
    return out


def full_list(c, kw):
    """Every record the device reports for the capture with all_candidates under the cell's keywords, ascending."""
    want = c.ev[kw["df18"]][0]
    return sorted(want + c.fixed) if kw.get("fix_1bit") else want


# ---------------------------------------------------------------- the layout of a cell
def layout(capi, front, cfg_index, cut):
    """(capture order, sample counts, segments, launches) of a batch cell: adsb_batch_layout_ex asked at units(n)."""
    _, kw, limit = CONFIGS[cfg_index]
    host = cases(front)
    order = _order(host, cfg_index)
    ns = [host[name].n for name in order]
    k = kw.get("debug_passes", 0)
    lo = limit if cut else 0
    segs, launches = capi.batch_layout([units(n) for n in ns], passes=k, launch_offsets=lo)
    check_layout([units(n) for n in ns], segs, launches, launch_limit(lo, k))
    return order, ns, segs, launches


def stream_reach(front, cfg_index):
    """(most entries one tile stages, most tries in one tile) over the stream kinds under a forced-K cell's geometry, from
    candidate_model.tile_bounds and the oracle's lists."""
    _, kw, _ = CONFIGS[cfg_index]
    k, big = kw["debug_passes"], kw.get("debug_big_tiles", 0)
    staged = tried = 0
    for name in STREAM_KINDS:
        c = cases(front)[name]
        g = np.array([r[0] for r in full_list(c, kw)], dtype=np.int64)
        tg = (c.ev[kw["df18"]][1] >> np.uint64(2)).astype(np.int64)
        for t0, t1 in M.tile_bounds(0, c.n_off, k, big):
            staged = max(staged, int(np.searchsorted(g, t1) - np.searchsorted(g, t0)))
            tried = max(tried, int(np.searchsorted(tg, t1) - np.searchsorted(tg, t0)))
    return staged, tried


def check_stream_reach(front, cfg_index):
    """A forced-K cell with a shrunken staged list or survivor queue overflows it in at least one tile of the stream kinds (every
    try is a survivor: the tries bound the queue's load from below)."""
    cid, kw, _ = CONFIGS[cfg_index]
    staged, tried = stream_reach(front, cfg_index)
    if "debug_clist_cap" in kw:
        assert staged > kw["debug_clist_cap"], (front, cid, staged)
    if "debug_queue_cap" in kw:
        assert tried > kw["debug_queue_cap"], (front, cid, tried)
    return staged, tried
