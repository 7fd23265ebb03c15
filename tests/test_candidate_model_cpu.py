"""The host model of the scan kernel's per-offset output (tests/candidate_model.py), pinned without a GPU: its tile geometry
against scan_kernel.h itself, its never-visited filter as sound (the greedy chain over what it keeps equals the chain over
every CRC-valid candidate from every entry a shard can have), and the checks that tests/test_gpu_candidates.py builds on as
able to fail: every deliberate mutation of the rule is caught, by the check named for it."""
import os
import subprocess

import numpy as np
import pytest

import candidate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launch geometries (passes, big_tiles, clist_cap) and window starts (g_begin: 0 and odd multiples of 28 mid-capture)
GEOMS = ([(k, 0, M.CLIST_CAP) for k in (2, 3, 4, 7, 10, 16, 32)] + [(7, 1, M.CLIST_CAP), (7, 3, M.CLIST_CAP)]
         + [(k, 0, cap) for k in (2, 7, 10) for cap in (1, 3, 64)])
WINDOWS = (0, 28 * 4001, 28 * 9999)


@pytest.fixture(scope="module")
def lists(oracle):
    """{capture: (every CRC-valid candidate of offsets [0, g_end), g_end)} from oracle.scan_all."""
    out = {}
    for name, x in M.make_captures().items():
        a = oracle.power(x)
        g_end = a.size - 1195
        out[name] = (oracle.scan_all(a, 0, g_end, True)[0], g_end)
    return out


def _cells(lists):
    for name, (cands, g_end) in lists.items():
        for gb in WINDOWS:
            mine = [c for c in cands if c[0] >= gb]
            for k, big, cap in GEOMS:
                yield name, mine, gb, g_end, k, big, cap


def _unsound(full, kept, gb, g_end):
    return M.equivalent_from(full, kept, range(gb, min(gb + M.ENTRY_REACH, g_end)), g_end)


def test_geometry_mirror_equals_the_header(tmp_path):
    """tile_count / tile_first_run / tile_passes of the mirror == scan_kernel.h's (hipcc host compile of
    tests/cpp/tile_starts.hip), with and without a taper of kTaperPasses tiles."""
    from adsbdec_amd import _build
    exe = tmp_path / "tile_starts"
    subprocess.run([_build.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "tile_starts.hip"),
                    "-o", str(exe)], check=True, capture_output=True)
    launches = [(n, k, big) for n in (1, 27, 28, 12879, 12880, 12881, 524_093, 1_048_576, 3_000_001)
                for k, big in ((2, 0), (3, 0), (4, 0), (4, 5), (7, 0), (7, 1), (7, 3), (10, 0), (16, 2), (32, 0))]
    out = subprocess.run([str(exe)] + [str(v) for l in launches for v in l], capture_output=True, text=True, check=True)
    lines = out.stdout.split("\n")
    for (n, k, big), line in zip(launches, lines):
        v = [int(w) for w in line.split()]
        tiles = M.tile_count(n, big, k)
        want = [tiles] + [M.tile_first_run(t, big, k) for t in range(tiles + 1)] + [M.tile_passes(t, big, k) for t in range(tiles)]
        assert v == want, (n, k, big)
        # the mirror's tile bounds cover [g_begin, g_end) exactly, in abutting tiles
        b = M.tile_bounds(28, 28 + n, k, big)
        assert b[0][0] == 28 and b[-1][1] == 28 + n and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
    assert len(lines) == len(launches) + 1


def test_chain_and_equivalence_helpers():
    """chain() is the greedy rule; equivalent_from() names exactly the entries whose chains differ."""
    c = [(100, 0, b"\x8d" * 14), (101, 0, b"\x8d" * 14), (1300, 0, b"\x58" * 7), (1302, 0, b"\x58" * 7), (1950, 0, b"\x8d" * 14)]
    assert [x[0] for x in M.chain(c, 0, 10_000)] == [100, 1300, 1950]
    assert [x[0] for x in M.chain(c, 101, 10_000)] == [101, 1302, 1950]
    assert [x[0] for x in M.chain(c, 101, 1302)] == [101]
    assert M.chain(c, 1951, 10_000) == []
    # without 1302, the chain from 101 lands on 1950 instead: entries 101 and 1301..1302 differ, nothing else
    assert M.equivalent_from(c, c[:3] + c[4:], range(0, 2000), 10_000) == [101, 1301, 1302]
    assert M.equivalent_from(c, c, range(0, 2000), 10_000) == []
    assert M.equivalent_from(c, c[:3] + c[4:], range(0, 2000), 1302) == []   # (1302 lies beyond the end)


def test_filter_model_is_sound(lists):
    """Applied per tile to the exhaustive lists, at every geometry and window: the kept list is chain-equivalent to the
    exhaustive one from every entry in [g_begin, g_begin + 1200) -- and it does drop candidates."""
    dropped = 0
    for name, full, gb, g_end, k, big, cap in _cells(lists):
        kept, counts = M.filter_model(full, gb, g_end, k, big, cap)
        assert sum(counts) == len(full)
        assert not _unsound(full, kept, gb, g_end), (name, gb, k, big, cap)
        dropped += len(full) - len(kept)
    assert dropped > 10_000


MUTATIONS = {   # mutation -> (filter_model keywords, the check that must catch it)
    "guard_pg_ge_0": (dict(guard=0), "soundness"),
    "short_span_600": (dict(spans=(600, 1200)), "soundness"),
    "long_span_1199": (dict(spans=(640, 1199)), "soundness"),
    "ignore_complete": (dict(use_complete=False), "soundness"),
    "end_at_pg_counts": (dict(end_at_pg_counts=True), "exactness"),
    "drop_nothing": (dict(drop_nothing=True), "exactness"),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutated_rule_is_caught(lists, mutation):
    """Each mutation of the rule is caught by its named check.  soundness: some cell's kept list has a chain from the
    contract's entries that the exhaustive list does not (what the GPU file asserts in every cell).  exactness: the
    mutation only keeps too much -- it stays sound, so only the GPU file's "kept list == filter_model" can see it."""
    kw, check = MUTATIONS[mutation]
    unsound, differs, cells = [], 0, 0
    for name, full, gb, g_end, k, big, cap in _cells(lists):
        if mutation == "ignore_complete" and cap != 3:
            continue
        cells += 1
        good, _ = M.filter_model(full, gb, g_end, k, big, cap)
        bad, _ = M.filter_model(full, gb, g_end, k, big, cap, **kw)
        if _unsound(full, bad, gb, g_end):
            unsound.append((name, gb, k, big, cap))
        differs += bad != good
    if check == "soundness":
        assert unsound, f"{mutation}: no cell of {cells} is unsound"
    else:
        assert not unsound and differs > 0, (mutation, unsound[:3], differs)
    print(f"{mutation}: caught by the {check} check ({len(unsound)} unsound cells, {differs} differing kept lists of {cells})")


def test_removing_a_reachable_candidate_is_caught(lists):
    """A correct kept list less one candidate that a chain from the contract's entries accepts: equivalent_from names an
    entry (one removal per capture that has candidates, at K = 7)."""
    tried = 0
    for name, (full, g_end) in lists.items():
        kept, _ = M.filter_model(full, 0, g_end, 7)
        ch = M.chain(kept, 0, g_end)
        if len(ch) < 3:
            continue
        victim = ch[len(ch) // 2]
        worse = [c for c in kept if c != victim]
        assert M.equivalent_from(full, worse, range(0, 1200), g_end), name
        tried += 1
    assert tried >= 6


def test_every_regime_of_the_filter_is_reached(lists):
    """Across the capture x geometry x window set, tiles stage <= 64 (the readlane path), 65-128 (LDS, two threads per
    entry), 129-256 (LDS, one thread per entry) and more than clist_cap (incomplete list: nothing dropped) entries."""
    total = np.zeros(4, dtype=np.int64)
    for _, full, gb, g_end, k, big, cap in _cells(lists):
        total += M.regimes(M.filter_model(full, gb, g_end, k, big, cap)[1], cap)
    print("tiles per regime (<=64, 65-128, 129-256, incomplete):", total.tolist())
    assert (total > 0).all(), total.tolist()
