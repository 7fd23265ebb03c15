"""The batch kernels' own output, record by record (run with -m gpu on an MI355X): what scan_batch_kernel.hip hands back for
every offset of every capture of a batch -- the records and try words of the last adsb_decode_batch_* call, read through
adsb_batch_records -- against the oracle's exhaustive evaluation of that capture alone (oracle.scan_all) and the host model of the
never-visited filter (tests/candidate_model.py), and what unpack12_batch.hip stores, word for word (adsb_batch_unpacked_copy).
tests/test_gpu_batch.py sees the frames of the greedy chain from offset 0 only; tests/test_gpu_candidates.py sees every offset, but
of scan_kernel.  Here every configuration runs twice: with the default launch limit (one launch), and CUT -- under
adsb_debug_config.batch_launch_offsets a 256 Ki capture is pieces of whole tiles plus a remainder, a launch each, and short
captures roll over into later launches -- the paths of csrc/batch.hpp that are otherwise reached beyond 2^30 offsets only.

The captures lie side by side in ONE device buffer with loud samples in every gap, so whatever a segment reads below its p_lo
or past its p_hi is a neighbour's signal, never silence."""
import numpy as np
import pytest

import candidate_model as M
from conftest import records
from test_batch_cpu import check_layout, launch_limit, offsets_of, power_samples

# measured on an MI355X: 13 s for the module's oracle fixture (charged to the first test), under 0.3 s for every test's own call
pytestmark = [pytest.mark.gpu, pytest.mark.limit(90)]

N = 1 << 18                                    # the nine kinds: 129 877 offsets, 11 tiles at K = 2, 3 at K = 7
N_EDGE = 84_000                                # the edge captures: 40 805 offsets -- two of them fit a cut launch of K = 7, none one of K = 2
TILE = lambda k: M.RUN * M.owned_runs(k)
EDGES = ("edge0", "edge1", "edge2", "edge3", "edge4")

# (id, Decoder keywords, launch limit of the cut run).  The two cuts the suite is about: 2 tiles of K = 7 with no forced K (a
# piece of 96 320 offsets and a remainder), and 3 tiles of K = 2 under debug_passes = 2 (four segments per capture; every capture
# is cut).  The other forced K are cut at tiles of their own: the knob is honoured from one tile of the forced K on.
CUT7, CUT2 = 2 * TILE(7), 3 * TILE(2)
CONFIGS = [
    ("default", dict(df18=True, collect_stats=True), CUT7),
    ("default_df11_17", dict(df18=False, collect_stats=True), CUT7),
    ("default_nostats", dict(df18=True, collect_stats=False), CUT7),
    ("default_df11_17_nostats", dict(df18=False, collect_stats=False), CUT7),
    ("k2", dict(df18=True, collect_stats=True, debug_passes=2), CUT2),
    ("k3_df11_17", dict(df18=False, collect_stats=True, debug_passes=3), 3 * TILE(3)),
    ("k7", dict(df18=True, collect_stats=True, debug_passes=7), CUT7),
    ("k10_nostats", dict(df18=True, collect_stats=False, debug_passes=10), TILE(10)),
    ("k32", dict(df18=True, collect_stats=True, debug_passes=32), TILE(32)),
    ("k7_clist1", dict(df18=True, collect_stats=True, debug_passes=7, debug_clist_cap=1), CUT7),
    ("k2_clist3", dict(df18=True, collect_stats=False, debug_passes=2, debug_clist_cap=3), CUT2),
    ("k7_queue256", dict(df18=True, collect_stats=True, debug_passes=7, debug_queue_cap=256), CUT7),
    ("k7_candcap", dict(df18=True, collect_stats=True, debug_passes=7, debug_cand_cap=64), CUT7),
    ("fix_1bit", dict(df18=True, collect_stats=True, fix_1bit=True), CUT7),
]
NAMED_CUTS = {"default": 7, "default_df11_17": 7, "default_nostats": 7, "default_df11_17_nostats": 7, "fix_1bit": 7, "k2": 2, "k2_clist3": 2}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


def _edge_capture(i):
    """84 000 + i samples (n % 4 = 0, 1, 2, 3, 0): a DF17 frame from sample 0 on and one that ends with the last window."""
    from tools import gen_signal as G
    rng = np.random.default_rng(4100 + i)
    n = N_EDGE + (i if i < 4 else 8)
    last = offsets_of(n) - 1
    return G.synth(n, [(0, G.make_frame(17, rng), 1200.0, 0.3), (2 * last - 12, G.make_frame(17, rng), 1100.0, 1.1)], 6.0, 4100 + i)


@pytest.fixture(scope="module")
def host(oracle):
    """{name: (capture, {df18: (candidates with reserved = 0, tries) of every offset}, {(df18, fix1): oracle.decode})}, in the
    order of the device buffer.  What the edge captures are for is asserted here, from the oracle alone."""
    kinds = M.make_captures(N)
    caps = {}
    edge = iter(EDGES)
    for name, x in kinds.items():
        caps[name] = x
        if name in ("uniform", "noise"):                       # an edge capture directly behind a capture whose tail is loud
            caps[next(edge)] = None
    for name in edge:
        caps[name] = None
    for i, name in enumerate(EDGES):
        caps[name] = _edge_capture(i)
    caps["short"] = np.random.default_rng(4200).integers(0, 4096, size=4099, dtype=np.uint16)     # no offsets: an empty segment
    names = list(caps)
    assert names[names.index("edge0") - 1] == "noise" and names[names.index("edge1") - 1] == "uniform" and float(np.std(caps["uniform"][-64:].astype(np.float64))) > 5000
    assert {caps[e].size % 4 for e in EDGES} == {0, 1, 2, 3}
    out = {}
    rng = np.random.default_rng(4300)
    for name, x in caps.items():
        n = int(x.size)
        a = oracle.power(x)
        n_off = offsets_of(n)
        assert a.size == power_samples(n) and (n_off == 0 or n_off - 1 + 1195 < a.size)
        ev = {}
        for df18 in (False, True):
            c, t = oracle.scan_all(a, 0, n_off, df18)
            ev[df18] = ([r + (0,) for r in c], t)
        dec = {(df18, fix1): oracle.decode(x, df18=df18, fix1=fix1) for df18, fix1 in ((False, False), (True, False), (True, True))}
        out[name] = (x, ev, dec)
        if name in EDGES:
            gs = [r[0] for r in ev[True][0]]
            # the frame at sample 0: candidates at g = 3..6, which read the six power samples that change when the eight pairs in
            # front of the capture are a neighbour's samples instead of silence (the capture's pair 0 at a multiple of 28)
            assert gs[:4] == [3, 4, 5, 6], (name, gs[:6])
            pre = np.concatenate([np.full(40, 2048, np.uint16), rng.integers(0, 4096, 16).astype(np.uint16), x])
            changed = np.nonzero(oracle.power(pre)[28:28 + a.size] != a)[0]
            assert changed.tolist() == [0, 1, 2, 3, 4, 5], (name, changed[:10])
            # the frame at the end: candidates at the last four offsets, the very last one included
            assert gs[-4:] == list(range(n_off - 4, n_off)), (name, gs[-6:], n_off)
            # samples behind the capture's end change only power samples that no offset reads
            post = np.concatenate([x, rng.integers(0, 4096, 64).astype(np.uint16)])
            changed = np.nonzero(oracle.power(post)[:a.size] != a)[0]
            assert (changed.size > 0) == (n % 4 != 0) and (changed.size == 0 or changed.min() > n_off - 1 + 1195), (name, changed)
    # every kind but `uniform` has CRC-valid candidates and tries to compare
    for name in kinds:
        assert name == "uniform" or (len(out[name][1][True][0]) >= 50 and out[name][1][True][1].size >= 500), name
    return out


@pytest.fixture(scope="module")
def device(host, torch_cuda):
    """The captures side by side in one device buffer: 16-byte aligned starts, the up to seven samples between a capture's end and
    the next start filled with loud codes like the guards in front of the first and behind the last.  -> {name: pointer}."""
    rng = np.random.default_rng(4400)
    at, cur = {}, 64
    for name, (x, _, _) in host.items():
        at[name] = cur
        cur = (cur + x.size + 7) // 8 * 8
    buf = rng.integers(0, 4096, size=cur + 64, dtype=np.uint16)          # guards and gaps: never silence
    for name, (x, _, _) in host.items():
        buf[at[name]:at[name] + x.size] = x
    t = torch_cuda.from_numpy(buf.view(np.int16)).cuda()
    assert t.data_ptr() % 16 == 0 and t.numel() * 2 < 64 << 20
    return t, {name: t.data_ptr() + 2 * a for name, a in at.items()}


def _order(host, cfg_index):
    """The batch's capture order of one configuration: the nine kinds rotated, the edge captures in a row behind the fourth of
    them (so that short captures meet a cut launch's remainder and each other), the capture without offsets last."""
    kinds = [n for n in host if n not in EDGES and n != "short"]
    r = cfg_index % len(kinds)
    kinds = kinds[r:] + kinds[:r]
    return kinds[:4] + list(EDGES) + kinds[4:] + ["short"]


def _layout(capi, host, cfg_index, cut):
    _, kw, limit = CONFIGS[cfg_index]
    order = _order(host, cfg_index)
    ns = [int(host[name][0].size) for name in order]
    k = kw.get("debug_passes", 0)
    lo = limit if cut else 0
    segs, launches = capi.batch_layout(ns, passes=k, launch_offsets=lo)
    check_layout(ns, segs, launches, launch_limit(lo, k))
    return order, ns, segs, launches


def _want(host, name, kw):
    return host[name][1][kw["df18"]]


def _pieces(segs, j):
    return [s for s in segs if s["capture"] == j]


def test_cut_layouts_reach_what_they_are_for(capi, host):
    """What keeps the cells below from passing vacuously, from the layout and the oracle's lists alone (nothing here reads the
    device): the cut runs cut, roll over and mix captures in a launch; back-to-back traffic has candidates close to both sides of
    every cut; and the forced-K cells fill tiles beyond 64 staged entries and beyond clist_cap."""
    over64 = over_cap = 0
    for ci, (cid, kw, limit) in enumerate(CONFIGS):
        k = kw.get("debug_passes", 0)
        cap = kw.get("debug_clist_cap", M.CLIST_CAP)
        for cut in (False, True):
            order, ns, segs, launches = _layout(capi, host, ci, cut)
            if k:
                for j, name in enumerate(order):
                    want = _want(host, name, kw)[0]
                    for s in _pieces(segs, j):
                        counts = M.filter_model([c for c in want if s["o_begin"] <= c[0] < s["o_end"]], s["o_begin"], s["o_end"], k, 0, cap)[1]
                        over64 += sum(n >= 65 for n in counts)
                        over_cap += sum(n > cap for n in counts)
            if not cut:
                assert len(launches) == 1 and len(segs) == len(ns), cid
                continue
            n_segs = [len(_pieces(segs, j)) for j in range(len(ns))]
            # (a K = 32 tile is longer than any capture here: that cell rolls over, it cannot cut)
            assert launch_limit(limit, k) == limit and len(launches) >= 4 and (k == 32 or sum(v >= 2 for v in n_segs) >= 6), (cid, n_segs)
            b2b = order.index("back_to_back")
            gs = np.array([c[0] for c in _want(host, "back_to_back", kw)[0]])
            cuts = [s["o_begin"] for s in _pieces(segs, b2b)][1:]
            assert cuts or k == 32, cid
            # a candidate within 1 200 offsets (a frame every 1 200) on both sides of every cut; with DF18 off every third frame
            # is no candidate: within 2 400
            reach = 1200 if kw["df18"] else 2400
            for c in cuts:
                assert ((gs >= c - reach) & (gs < c)).any() and ((gs >= c) & (gs < c + reach)).any(), (cid, c)
            if cid not in NAMED_CUTS:
                continue
            if NAMED_CUTS[cid] == 2:                         # four pieces a capture: at least six captures in three segments or more
                assert sum(v >= 3 for v in n_segs) >= 6, (cid, n_segs)
            else:
                # a launch that holds segments of two captures or more behind a launch that ended on a roll-over (its last segment
                # ends a capture, the next capture did not fit what was left)
                mixed = [li for li in range(1, len(launches))
                         if len({s["capture"] for s in segs[launches[li]["seg_first"]:launches[li]["seg_end"]] if s["o_end"] > s["o_begin"]}) >= 2
                         and segs[launches[li]["seg_first"]]["o_begin"] == 0
                         and segs[launches[li]["seg_first"] - 1]["capture"] != segs[launches[li]["seg_first"]]["capture"]]
                assert mixed, (cid, [(L["seg_first"], L["seg_end"]) for L in launches])
    print("forced-K tiles that stage 65 entries or more:", over64, "; more than clist_cap:", over_cap)
    assert over64 >= 1 and over_cap >= 1


def _rebase(segs, cands, tries, n_captures):
    """The raw virtual lists -> per capture (candidates, tries) at offsets from 0.  Asserts, on the raw lists, that no record and
    no try word lies outside every segment's [base, base + o_end - o_begin)."""
    base = np.array([s["base"] for s in segs], dtype=np.int64)
    span = np.array([s["o_end"] - s["o_begin"] for s in segs], dtype=np.int64)
    shift = np.array([s["o_begin"] - s["base"] for s in segs], dtype=np.int64)
    owner = np.array([s["capture"] for s in segs], dtype=np.int64)
    assert np.all(np.diff(base) > 0)

    def place(g):
        k = np.searchsorted(base, g, side="right") - 1
        assert g.size == 0 or (k.min() >= 0 and np.all(g - base[k] < span[k])), "a record outside every segment"
        return k

    cg = np.array([c[0] for c in cands], dtype=np.int64)
    assert np.all(np.diff(cg) > 0)                           # sorted; one record per offset
    ck = place(cg)
    per_c = [[] for _ in range(n_captures)]
    for c, k in zip(cands, ck):
        per_c[owner[k]].append((c[0] + int(shift[k]),) + c[1:])
    tg = (tries >> np.uint64(2)).astype(np.int64)
    assert np.all(np.diff(tries.astype(np.int64)) > 0)
    tk = place(tg)
    local = ((tg + shift[tk]).astype(np.uint64) << np.uint64(2)) | (tries & np.uint64(3))
    per_t = [local[owner[tk] == j] for j in range(n_captures)]
    return per_c, per_t


def _check_frames(d, order, host, kw, frames, stats):
    key = (kw["df18"], bool(kw.get("fix_1bit")))
    total = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for j, name in enumerate(order):
        wf, ws = host[name][2][key]
        assert records(frames[j]) == records(wf), name
        assert stats[j]["ok"] == ws["ok"] and stats[j].get("fixed", 0) == ws.get("fixed", 0), name
        if kw["collect_stats"]:
            assert stats[j]["try"] == ws["try"], name
        for row in ("try", "ok"):
            for df in (11, 17, 18):
                total[row][df] += stats[j][row][df]
    whole = d.stats()
    assert whole["ok"] == total["ok"] and (not kw["collect_stats"] or whole["try"] == total["try"])


def _run(capi, host, ptrs, cfg_index, cut, all_candidates):
    """One batch call of a cell -> (frames, stats, per-capture candidates, per-capture tries, segments, launches, relaunches)."""
    _, kw, limit = CONFIGS[cfg_index]
    order, ns, segs_want, launches_want = _layout(capi, host, cfg_index, cut)
    d = capi.Decoder(all_candidates=all_candidates, **kw, **(dict(debug_batch_launch_offsets=limit) if cut else {}))
    try:
        before = d.profile()
        frames, stats = d.decode_batch_device([ptrs[name] for name in order], ns, stats=True)
        after = d.profile()
        _check_frames(d, order, host, kw, frames, stats)
        cands, tries, segs, launches = d.batch_records()
    finally:
        d.close()
    # the layout the call used is adsb_batch_layout_ex's for a device of 256 compute units
    assert segs == segs_want and launches == launches_want
    assert after["launches"] - before["launches"] >= sum(1 for L in launches if L["tiles"])
    per_c, per_t = _rebase(segs, cands, tries, len(ns))
    return frames, stats, per_c, per_t, segs, launches, after["relaunches"] - before["relaunches"]


@pytest.mark.parametrize("cfg_index", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
def test_batch_records_equal_the_oracle_offset_by_offset(capi, oracle, host, device, cfg_index):
    cid, kw, _ = CONFIGS[cfg_index]
    _, ptrs = device
    k, cap, fix = kw.get("debug_passes", 0), kw.get("debug_clist_cap", M.CLIST_CAP), bool(kw.get("fix_1bit"))
    uncut = None
    for cut in (False, True):
        order = _order(host, cfg_index)
        frames_a, stats_a, every, tries_a, segs, launches, relaunched_a = _run(capi, host, ptrs, cfg_index, cut, True)
        frames, stats, kept, tries, segs_d, launches_d, relaunched = _run(capi, host, ptrs, cfg_index, cut, False)
        assert segs_d == segs and launches_d == launches
        assert (frames, stats) == (frames_a, stats_a)
        if "debug_cand_cap" in kw:
            assert relaunched_a >= 1 and relaunched >= 1, (cid, cut)
        for j, name in enumerate(order):
            where = (cid, "cut" if cut else "uncut", name)
            x, _, _ = host[name]
            want, wtries = _want(host, name, kw)
            end = offsets_of(x.size)
            # all_candidates = 1: every offset's record, and every try word
            if fix:
                assert [c for c in every[j] if c[3] == 0] == want, where
                wg = {c[0] for c in want}
                for c in every[j]:
                    assert c[3] == 0 or (len(c[2]) == 14 and oracle.crc_residual(c[2]) == 0 and c[0] not in wg), (where, c)
            else:
                assert every[j] == want, (where, len(every[j]), len(want), sorted(set(every[j]) ^ set(want))[:4])
            for t in (tries_a[j], tries[j]):
                assert np.array_equal(t, wtries) if kw["collect_stats"] else t.size == 0, where
            # default: what the never-visited filter leaves
            full = every[j] if fix else want
            assert set(kept[j]) <= set(full) and kept[j] == sorted(kept[j]), where
            parts = _pieces(segs, j)
            entries = [0] + [e for s in parts[1:] for e in range(s["o_begin"], min(s["o_begin"] + M.ENTRY_REACH, end))]
            assert not M.equivalent_from(full, kept[j], entries, end), where
            if k:
                model = [c for s in parts
                         for c in M.filter_model([c for c in full if s["o_begin"] <= c[0] < s["o_end"]], s["o_begin"], s["o_end"], k, 0, cap)[0]]
                assert kept[j] == model, (where, len(kept[j]), len(model), sorted(set(kept[j]) ^ set(model))[:6])
        if fix:
            assert sum(c[3] for name_c in every for c in name_c) > 20, cid
        if uncut is None:
            uncut = (frames, stats, every, None, tries)
        else:                                                # the cut run equals the uncut run, byte for byte
            # (the kept lists may differ where a cut moved a tile boundary: each has been held to its own model above)
            assert (frames, stats) == uncut[:2] and every == uncut[2] and all(np.array_equal(a, b) for a, b in zip(tries, uncut[4]))


# ---------------------------------------------------------------- the batch unpack, word for word
def _group_counts(seed, big_first):
    """~600 captures as numbers of 8-sample groups: 500 of 1 to 40 groups side by side (a 256-group chunk of the unpack kernel
    spans dozens of rows) with captures of 0 groups between them, 255 / 256 / 257 groups, two of 128 Ki samples around a run of
    one-group captures, and one of 256 Ki samples (None: the decodable capture)."""
    rng = np.random.default_rng(seed)
    small = [int(v) for v in rng.integers(1, 41, size=500)]
    for at in range(7, 500, 23):
        small.insert(at, 0)
    edge = [255, 256, 257, 0, 257, 256, 255]
    big = [(128 << 10) // 8] + [1] * 40 + [(128 << 10) // 8]
    # (the first pattern is the larger one: the second call fits the scratch the first one left)
    return (big + [None] + edge + small + [40] * 60) if big_first else (small[:300] + edge + small[300:] + big + [None] + [3, 0, 1] * 10)


def _slots(ns):
    at, cur = [], 0
    for n in ns:
        at.append(cur)
        cur += (2 * n + 127) // 128 * 64
    return at, cur


def test_batch_unpack_word_for_word(capi, oracle, torch_cuda):
    """One adsb_decode_batch_device_packed call over ~600 packed captures of random codes: EVERY capture's unpacked samples in the
    handle's scratch are packed12.unpack12 of its bytes, and the pad behind a capture (up to 126 bytes to the next 128-byte
    boundary) is untouched -- it still holds what a first call with ANOTHER pattern of captures unpacked there."""
    from adsbdec_amd.packed12 import pack12, unpack12
    from test_gpu_batch_packed import PackedOnDevice, packable
    decodable = packable(M.make_captures(N)["dense"])
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        model = known = None
        for call, (seed, big_first) in enumerate(((4500, True), (4501, False))):
            rng = np.random.default_rng(seed + 10)
            caps = [decodable if g is None else rng.integers(0, 4096, size=8 * g, dtype=np.uint16) for g in _group_counts(seed, big_first)]
            packed = [pack12(x) for x in caps]
            ns = [int(x.size) for x in caps]
            assert len(ns) >= 590 and ns.count(0) >= 20 and {8 * 255, 8 * 256, 8 * 257, 128 << 10, N} <= set(ns)
            dev = PackedOnDevice(torch_cuda, packed)
            assert {p % 16 for p in dev.ptrs if p} == {0, 4, 8, 12}
            at, total = _slots(ns)
            if model is None:
                model, known = np.zeros(total, np.uint16), np.zeros(total, bool)
            assert total <= model.size                       # (the second call fits the first one's scratch: it is not reallocated)
            for a, x in zip(at, caps):
                model[a:a + x.size] = x
                known[a:a + x.size] = True
            frames, stats = d.decode_batch_device_packed(dev.ptrs, ns, stats=True)
            n_pad = 0
            for i, (a, x, b) in enumerate(zip(at, caps, packed)):
                slot = (at[i + 1] if i + 1 < len(at) else total) - a
                got = d.batch_unpacked(i, slot)
                assert np.array_equal(got[:x.size], unpack12(b)), (call, i, ns[i])
                pad = slice(a + x.size, a + slot)
                assert np.array_equal(got[x.size:][known[pad]], model[pad][known[pad]]), (call, i, ns[i])
                n_pad += int(np.count_nonzero(known[pad] & (model[pad] != 0)))
                wf, ws = oracle.decode(x, df18=True) if offsets_of(x.size) else ([], {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}})
                assert records(frames[i]) == records(wf) and stats[i] == ws, (call, i, ns[i])
            assert sum(len(f) for f in frames) > 20
            # the second call's pads lie where the first call unpacked random codes: an "untouched" that can be seen
            assert call == 0 or n_pad > 2000, n_pad
            for bad_i, bad_n in ((len(ns), 0), (0, at[1] + 1), (len(ns) - 1, total - at[-1] + 1)):
                with pytest.raises(capi.AdsbError, match="adsb_batch_unpacked_copy"):
                    d.batch_unpacked(bad_i, bad_n)
    finally:
        d.close()
