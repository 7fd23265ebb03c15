"""The try-count pass without a GPU: the numpy definition of tests/try_count_cases.py gives the oracle's Try row on every capture of
the power front end, in one pass and in three chained ones; every case that tests/test_gpu_try_count.py runs on the device reaches
what it says it is for, counted from the model and the tile geometry alone; adsb_count_tries_alone is declared, exported and bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import try_count_cases as T
from conftest import ROOT


def test_entry_point_is_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, diag = strip("adsbdec_amd.h"), strip("adsbdec_amd_diag.h")
    assert re.search(r"\bint\s+adsb_count_tries_alone\s*\(", diag) and "adsb_count_tries" not in main and "adsb_try_frame" not in main
    assert "#define ADSB_ABI_VERSION 5" in main
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    assert "adsb_count_tries_alone" in exported and "adsb_count_tries_alone" in capi.SYMBOLS and hasattr(L, "adsb_count_tries_alone")
    assert len(capi.SYMBOLS["adsb_count_tries_alone"][1]) == 20 and L.adsb_abi_version() == 5
    assert ctypes.sizeof(capi.TryFrame) == 16 and capi.TryFrame.span.offset == 8
    assert capi.TRY_FRAME_DTYPE == T.FRAME and capi.TRY_FRAME_DTYPE.itemsize == 16 and capi.TRY_REGION == T.REGION
    src = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "scan_kernel.h")).read()
    assert "kTryRegion = 4 * kQueueCap" in src and "kQueueCap = 4 * kThreads" in src and "kThreads = 256" in src and T.REGION == 4096


# ------------------------------------------------------------------ (a) the definition equals the oracle
@pytest.fixture(scope="module")
def power_cases():
    import front_records_cases as F
    return F.cases("power")


@pytest.mark.parametrize("df18", [False, True])
def test_definition_gives_the_oracles_try_row(power_cases, df18):
    """Every capture: the oracle's try words against the frames of oracle.demod_power, hi = the end of the last visited range,
    final -> stats["try"], in one pass and in three (hi at a frame's end, then strictly inside a frame's span; a pass is given the
    frames below its hi that no pass before it was given, and the last one that was: one earlier frame suffices)."""
    seen_three = 0
    for name, c in power_cases.items():
        want = c.dec[(df18, False)][1]["try"]
        want = [want[11], want[17], want[18]]
        fg, sp, tg, tc, end = T.capture_lists(c, df18)
        for k in (2, 7):
            total, res = T.chain(T.replay_single(c, df18, k), T.model)
            assert total == want and res[0].n_carry_out == 0, (name, df18, k, total, want)
            passes = T.replay_three(c, df18, k)
            total, res = T.chain(passes, T.model)
            assert total == want and res[2].n_carry_out == 0, (name, df18, k, total, want)
            if len(fg) >= 3:
                h1, h2 = passes[0].hi, passes[1].hi
                assert np.any(fg + sp == h1) and np.any((fg < h2) & (h2 < fg + sp)), (name, h1, h2)
                if name in T.REPLAY_KINDS:
                    # every pass decides something, carries something on, and pass 2 and 3 start with the last frame given before
                    assert res[0].n_carry_out > 0 and res[1].n_carry_out > 0 and all(sum(r.acc) > 0 for r in res), (name, k)
                    assert passes[1].frames["g"][0] == fg[fg < h1][-1] and passes[2].frames["g"][0] == fg[fg < h2][-1]
                    assert sum(len(p.frames) for p in passes) == len(fg) + 2
                    seen_three += 1
    assert seen_three == 2 * (4 if df18 else 3)                 # (without DF18 `damaged` decodes no frame)


def test_replay_kinds_fill_regions_and_shadow_tries(power_cases):
    """What the replay on the device stands on: in each kind some tries are shadowed and some counted, per code that occurs; in the
    K = 7 replay every kind puts tries on the list too (a region takes 256 there)."""
    for name in T.REPLAY_KINDS:
        c = power_cases[name]
        p = T.replay_single(c, True, 7)[0]
        r = T.model(p)
        m = T.measure(p, r)
        assert m["fates"]["region"][T.COUNTED] > 0 and m["fates"]["region"][T.SHADOWED] > 0, (name, m["fates"])
        assert m["fates"]["list"][T.COUNTED] > 0 and int(p.region_counts.max()) == 256, (name, m["fates"])
        assert T.replay_single(c, True, 2)[0].tries.size == 0


# ------------------------------------------------------------------ (b) every case reaches what it claims
def test_window_edge_cases():
    for d in (-1, 0, 1):
        sets = []
        for route in T.ROUTES:
            p, what = T.window_edges(d, route)
            r = T.model(p)
            sets.append(sorted(zip(r.g.tolist(), r.code.tolist())))
            assert len(p.frames) == 0 + 1 + 63 + 64 + 1 + 64 + 64 and set(p.frames["span"].tolist()) == {1, 2, 7, 200, 640, 1200}
            if route != "regions":
                assert p.regions is None and (p.tries.size == 0) != (p.n_carry == 0)
                continue
            m = T.measure(p, r)
            assert m["windows"] == what["windows"] and m["fits"] == what["fits"], (d, m["windows"], m["fits"])
            assert m["next_rel"][3] == what["next_rel_tile3"] == d and m["next_rel"][5] is None and m["next_rel"][4] is not None
            assert list(p.region_counts) == what["counts"] == [1, 127, 4095, 4096, 129, 128] and p.tries.size == 0
            # all four boundary positions under the wave's window and under the binary search of the tile that does not fit
            assert min(m["boundary"]["window"]) >= 8 and min(m["boundary"]["search"]) >= 2, m["boundary"]
            assert min(m["codes"]) > 100
            bounds = T.geometry(p)
            g = set(r.g.tolist())
            assert all(t0 in g and t1 - 1 in g for t0, t1 in bounds[1:]) and bounds[0][0] in g
            # tile 4, which the wave cannot hold: a try shadowed by the 65th frame of its window, the last one
            fg, sp = p.frames["g"].astype(np.int64), p.frames["span"].astype(np.int64)
            last4 = int(np.searchsorted(fg, bounds[4][1])) - 1
            assert sp[last4] == 200 and int(fg[last4]) + 1 in g and int(fg[last4]) + 199 in g
        assert sets[0] == sets[1] == sets[2]                    # the same tries through every source


def test_front_frame_cases():
    clamps = 0
    for g_base in T.FRONT_BASES:
        for kind in T.FRONT_KINDS:
            for route in T.ROUTES:
                p, what = T.front_frames(g_base, kind, route)
                r = T.model(p)
                fate = dict(zip(r.g.tolist(), r.fate.tolist()))
                assert len(what["probes"]) == (1 if g_base == 0 else 2)
                for b, shadowed in what["probes"]:
                    assert fate[b] == (T.SHADOWED if shadowed else T.COUNTED) and fate[b + 1] == T.COUNTED, (g_base, kind, b)
                    if b - 1 >= g_base:                       # (the inner tile: the offset in front of it is the tile before's)
                        assert (b - 1 in fate)
                if route == "regions":
                    bounds = T.geometry(p)
                    assert [b for b, _ in what["probes"]] == [bounds[t][0] for t in (0, 2) if bounds[t][0] > 0]
                    clamps += bounds[0][0] < 1199
    assert clamps == 3 * 3                                      # g_base 0, 28, 1176: key clamps to 0
    p, _ = T.front_frames((1 << 33) + 28, "reaches_t0", "regions", hi=(1 << 33) + 28 + (1 << 32) + 12345)
    assert p.hi - p.g_base > 0xFFFFFFFF and T.model(p).n_carry_out == 0
    p, _ = T.front_frames((1 << 32) - 28 * 300, "short", "regions")
    assert p.g_base < 1 << 32 < T.geometry(p)[0][1]             # tile 0 crosses 2^32


def test_hi_cases():
    for kind in T.HI_KINDS:
        for final in (0, 1):
            for route in T.ROUTES + ("mixed",):
                p, what = T.hi_case(kind, final, route)
                r = T.model(p)
                late = r.fate >= T.CARRIED
                assert set(r.fate[late].tolist()) <= {T.DROPPED if final else T.CARRIED}
                assert (not what["all_late"] or late.all()) and (not what["none_late"] or not late.any())
                if what["at"]:
                    below, at = what["at"]
                    fate = dict(zip(r.g.tolist(), r.fate.tolist()))
                    assert fate[at] >= T.CARRIED and fate[below] <= T.SHADOWED
                    assert 0 < np.count_nonzero(late) < late.size
                if kind == "in_span":
                    fg, sp = p.frames["g"].astype(np.int64), p.frames["span"].astype(np.int64)
                    assert np.any((fg < p.hi) & (p.hi < fg + sp)) and fate[p.hi - 1] == T.SHADOWED
                if route == "regions" and kind in ("at_try", "in_span"):
                    t0, t1 = T.geometry(p)[1 if kind == "at_try" else 0][0], T.geometry(p)[-1][1]
                    assert t0 < p.hi < t1                       # hi inside a region
    for n_late in (101, 5000):
        p, what = T.carry_overflow(n_late)
        r = T.model(p)
        m = T.measure(p, r)
        assert r.n_carry_out == n_late > p.carry_cap == 100 and r.overflow
        assert all(m["fates"][s][T.CARRIED] > 0 for s in T.SOURCES)
        assert sum(m["fates"][s][T.CARRIED] for s in T.SOURCES) == n_late
    p, what = T.carry_count_above_cap()
    assert p.n_carry == 500 > p.carry_cap == 463 and p.carry_in.size == 500
    r = T.model(p)
    assert r.g.size == 463 and 0 < r.n_carry_out < 463
    q = T.Pass(**p.__dict__)
    q.carry_cap = 500
    assert T.model(q).acc != r.acc                              # the 37 entries behind the cap would have been noticed


def test_geometry_cases():
    seen = set()
    for k, big, n_tiles in T.GEOMETRIES:
        p, what = T.geometry_case(k, big, n_tiles)
        r = T.model(p)
        m = T.measure(p, r)
        bounds = T.geometry(p)
        assert len(bounds) == n_tiles and m["region_blocks"] == what["region_blocks"] and m["region_trips"] == what["region_trips"]
        sizes = [28 * (252 * kk - 44) for kk in ((k, 4) if big and k > 4 and n_tiles > big else (k,))]
        assert what["tile_offsets"] == sizes, (k, big, n_tiles, what["tile_offsets"])
        fate = dict(zip(r.g.tolist(), r.fate.tolist()))
        for i, (t0, t1) in enumerate(bounds):                   # the try at every tile's first offset is shadowed, from in front
            assert fate[t0] == T.SHADOWED and p.region_counts[i] >= 3
            assert fate[t0 + 1] == T.COUNTED if i % 2 == 0 else (fate[t0 + 3], fate[t0 + 4]) == (T.SHADOWED, T.COUNTED)
            assert fate[t1 - 1] == T.SHADOWED                   # ... and the one at its last offset
        assert m["fates"]["list"][T.COUNTED] + m["fates"]["list"][T.SHADOWED] >= 2      # behind the last tile
        seen.add((m["region_trips"], what["ragged"] != 0))
    assert (2, True) in seen and (1, False) in seen
    p, what = T.geometry_case(2, 0, 1030)
    assert T.measure(p)["region_blocks"] == 258 > T.REGION_GRID
    p, what = T.region_count_above_cap()
    r = T.model(p)
    assert p.region_counts[0] == 5000 and r.g.size == 4096 + 1000 + 50
    words = p.regions[T.REGION:T.REGION + 904]
    assert np.count_nonzero(~np.isin(words, p.regions[:T.REGION])) == 904       # what an unclamped count would read is other tries


def test_trip_cases():
    p, what = T.list_trips()
    m = T.measure(p)
    assert p.tries.size == what["list_words"] == 20_000 and p.regions is not None and int(p.region_counts.sum()) == 300
    assert (m["list_blocks"], m["list_trips"]) == (what["list_blocks"], what["list_trips"]) == (64, 2)
    assert min(m["boundary"]["search"]) > 50 and m["fates"]["list"][T.SHADOWED] > 1000
    p, what = T.carry_trips()
    r = T.model(p)
    m = T.measure(p, r)
    assert p.n_carry == what["carry_words"] == 70_000 <= p.carry_cap and p.tries.size == 0 and p.regions is None
    assert (m["list_blocks"], m["list_trips"]) == (what["list_blocks"], what["list_trips"]) == (256, 2)
    assert r.n_carry_out == 24_000 and min(m["fates"]["carry"][:3]) > 1000
    sizes = []
    for n in T.FRAME_COUNTS:
        p, what = T.frame_counts(n)
        r = T.model(p)
        m = T.measure(p, r)
        sizes.append(len(p.frames))
        fg, sp = p.frames["g"].astype(np.int64), p.frames["span"].astype(np.int64)
        fate = dict(zip(r.g.tolist(), r.fate.tolist()))
        if len(fg):
            lo, hi = int(r.g.min()), int(r.g.max())
            assert lo < fg[0] and hi >= fg[-1] + sp[-1] and fate[lo] == fate[hi] == T.COUNTED
            assert fate[int(fg[0]) + 1] == fate[int(fg[-1]) + 1] == T.SHADOWED
        assert all(sum(m["fates"][s]) > 500 for s in T.SOURCES) and sum(m["fates"][s][T.CARRIED] for s in T.SOURCES) == 0
        if what["thin"]:
            assert all(m["windows"][t] == 40 and m["fits"][t] for t in what["thin"]) and m["fits"].count(False) == 58
            assert min(m["boundary"]["window"]) >= 10 and min(m["boundary"]["search"]) >= 10, m["boundary"]
    assert sizes[:8] == list(T.FRAME_COUNTS[:8]) and 280_000 < sizes[8] < 300_000


def test_every_source_meets_every_fate_and_every_path_every_boundary():
    """Over the cases of the hi test: a carried, a dropped, a shadowed and a counted try per source."""
    tally = {s: [0, 0, 0, 0] for s in T.SOURCES}
    for kind in ("at_try", "in_span"):
        for final in (0, 1):
            p, _ = T.hi_case(kind, final, "mixed")
            m = T.measure(p)
            for s in T.SOURCES:
                tally[s] = [a + b for a, b in zip(tally[s], m["fates"][s])]
            assert min(m["boundary"]["window"]) > 0 and min(m["boundary"]["search"]) > 0, m["boundary"]
    assert all(min(v) > 10 for v in tally.values()), tally


def test_model_forms_agree_and_contract_is_checked():
    """The brute-force form on every small case is part of model(); here also on a case above its limit, once; and check_contract
    refuses what the kernel may not be given."""
    p, _ = T.hi_case("in_span", 0, "mixed")
    g, _, _ = T.tries_of(p)
    assert g.size > 2000 and np.array_equal(T.shadowed_by_search(p, g), T.shadowed_brute(p, g))
    q = T.Pass(**p.__dict__)
    q.frames = p.frames.copy()
    q.frames["span"][3] = 1201
    with pytest.raises(AssertionError):
        T.check_contract(q)
    q.frames = p.frames.copy()
    q.frames["g"][4] = q.frames["g"][3]
    with pytest.raises(AssertionError):
        T.check_contract(q)
    q.frames = p.frames
    q.regions = p.regions.copy()
    q.regions[0] = np.uint32((13_000 << 2) | 1)                 # a try of tile 1 in tile 0's region
    with pytest.raises(AssertionError):
        T.check_contract(q)
