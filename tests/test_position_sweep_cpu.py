"""What keeps tests/test_gpu_position_sweep.py from passing by luck, asserted without a device from the oracle's lists,
candidate_model and the shifts alone (tests/position_sweep_cases.py): every tile-relative offset of a scan tile is the offset of
a long and of a short candidate and of a try of every DF, for every swept K, both Stage B instantiations and every front end;
the end sweep cuts every planted frame's candidates at each of its offsets; the damaged capture has every bit repaired at every
r; the filter comparison is not empty; the shift-derived expectations of the batch calls equal the direct oracle; and a weakened
sweep fails these very assertions."""
import numpy as np
import pytest

import candidate_model as M
import front_records_cases as F
import position_sweep_cases as P


@pytest.fixture(scope="module")
def L():
    return P.sweep()[1]


def test_the_capture_is_what_the_sweeps_need(L):
    """No record's window leaves the capture, no candidate lies in front of LEAD (every shift of a K <= 7 tile keeps all frames
    in its window), every planted frame has its run of consecutive candidates, and the last one ends on the last offset."""
    x, _ = P.sweep()
    assert x.size == P.N_SWEEP and L.n_off == P.G_MAX and P.LEAD == 48_160
    assert max(P.RUN * (M.owned_runs(k) - 1) for _, k, _, _ in P.SWEEPS) < P.LEAD
    for df18 in (False, True):
        assert L.g[df18] and L.g[df18][0] >= P.LEAD + P.FIRST
    groups = P.frame_groups(L)
    assert len(groups) == P.N_FRAMES + 1 and all(3 <= len(g) <= 6 for g in groups), [len(g) for g in groups]
    assert groups[-1][-1] == L.n_off - 1
    by_len = [{len(c[2]) for c in L.ev[True][0] if grp[0] <= c[0] <= grp[-1]} for grp in groups]
    assert by_len[:28] == [{14}] * 28 and by_len[28:56] == [{7}] * 28 and by_len[56] == {14}
    print("candidates:", len(L.g[True]), "(df18 on),", len(L.g[False]), "(off); tries:", L.tg[True].size, L.tg[False].size)


@pytest.mark.parametrize("sweep", P.SWEEPS, ids=[s[0] for s in P.SWEEPS])
def test_the_start_sweep_reaches_every_tile_relative_offset(L, sweep):
    """Per swept K and Stage B instantiation (statistics on / off run the same shifts): every tile-relative offset in
    [0, 28 owned_runs(K)) is the offset of a long candidate, of a short one, and of a DF11, a DF17 and (df18 on) a DF18 try."""
    sid, k, df18, stats = sweep
    fewest = P.check_coverage(L, k, df18)
    print(sid, "fewest hits per tile-relative offset:", fewest)
    assert set(fewest) == ({"long", "short", "try11", "try17", "try18"} if df18 else {"long", "short", "try11", "try17"})
    # ... and the reason: every kind occurs at all 28 residues r behind LEAD
    for kind, gs in P.kinds(L, df18).items():
        gs = np.asarray(gs)
        assert len(set((gs[gs >= P.LEAD] % P.RUN).tolist())) == P.RUN, (sid, kind)
    # the three buffer starts occur at every K, and by a rule that j mod 2 does not decide
    top = lambda j: (2 * (P.RUN * j - 6)) // 8 * 8
    lag = [top(j) - P.first_samples(j) for j in P.shifts(k) if top(j) >= 8000]
    assert set(lag) == {0, 8, 8000}
    for parity in (0, 1):
        assert {top(j) - P.first_samples(j) for j in P.shifts(k) if j % 2 == parity and top(j) >= 8000} == {0, 8, 8000}
    assert all(P.first_samples(j) % 8 == 0 and 0 <= P.first_samples(j) <= max(0, 2 * (P.RUN * j - 6)) for j in P.shifts(k))


def test_candidates_lie_in_first_interior_and_last_tiles(L):
    """Candidates occur in tile 0, in an interior tile and in the last tile of scans of the start sweep; at K = 2 and 3, whose
    tile is shorter than LEAD, tile 0 is the head sweep's: there every r is the tile-relative offset of a candidate in run 0."""
    seen = {sid: P.tiles_reached(L, k, df18) for sid, k, df18, _ in P.SWEEPS}
    print(seen)
    assert all({"interior", "last"} <= s for s in seen.values()) and "first" in seen["k7"]
    g = np.array(L.g[True])
    in_run0 = set()
    for gb, fs in P.head_sweep(L):
        assert gb % P.RUN == 0 and fs % 8 == 0 and 0 <= 2 * (gb - 6) - fs < 8
        first = g[(g >= gb) & (g < gb + P.RUN)]
        assert first.size, gb
        in_run0 |= set((first - gb).tolist())
    assert in_run0 == set(range(P.RUN))


def test_the_end_sweep_cuts_every_frame_at_every_candidate(L):
    """Every scan of the end sweep ends beside a candidate: one at g_end - 1 (the last record the scan owns) or one at g_end (the
    first it must not report) -- both wherever g_end lies inside a frame's run of candidates, and each frame has its first and
    its last cut: g_end = c0 (none of its candidates is in) and g_end = cm + 1 (all are).  The frame at the capture's end is
    among them, the buffer of the exact scan ends with the last owned offset's window, and the frame lies in the last tile."""
    have = set(L.g[True])
    cells = P.end_sweep(L)
    both = 0
    for gb, ge, fs, n in cells:
        assert gb % P.RUN == 0 and fs % 8 == 0 and fs <= 2 * (gb - 6) and fs + n == 2 * (ge - 1 + P.WINDOW) <= P.N_SWEEP
        assert (ge - 1 in have) or (ge in have), (gb, ge)
        both += (ge - 1 in have) and (ge in have)
        assert M.tile_bounds(gb, ge, 2)[-1][0] <= ge - 1 and len(M.tile_bounds(gb, ge, 2)) == 1
    groups = P.frame_groups(L)
    ends = {ge for _, ge, _, _ in cells}
    for grp in groups:
        assert {grp[0], grp[-1] + 1} <= ends | {L.n_off + 1} and all(c in ends for c in grp), grp
    assert L.n_off in ends and L.n_off - 1 in have
    assert both == sum(len(grp) - 1 for grp in groups) and len(cells) >= 5 * len(groups)
    print("end sweep:", len(cells), "cuts,", both, "inside a run of candidates")


def test_the_damaged_capture_repairs_every_bit_at_every_residue():
    """All 107 bit positions 5 .. 111 are repaired at least once per residue class r = g mod 28, every long frame is damaged (the
    oracle finds no CRC-valid candidate), and the K = 2 shifts keep every frame inside the window."""
    x, L, fixed, every, bits = P.damaged()
    assert not L.ev[True][0] and len(fixed) >= 3 * P.N_DAMAGED and every == fixed
    assert fixed[0][0] >= P.LEAD_DAMAGED > P.RUN * (M.owned_runs(2) - 1)
    assert all(r[3] == 1 and len(r[2]) == 14 for r in fixed)
    seen = {(b, r[0] % P.RUN) for b, r in zip(bits, fixed)}
    assert seen == {(b, r) for b in range(5, 112) for r in range(P.RUN)}, len(seen)
    print("damaged capture:", x.size, "samples,", len(fixed), "repairable offsets,", L.tg[True].size, "tries")


@pytest.mark.parametrize("sweep", P.SWEEPS, ids=[s[0] for s in P.SWEEPS])
def test_the_filter_drops_something_and_keeps_something(L, sweep):
    """The default-handle comparison is not empty: at every shift the never-visited filter's model drops candidates and keeps
    candidates; over the sweep the kept lists differ (a tile boundary moves through the frames)."""
    sid, k, df18, _ = sweep
    kept = P.kept_lists(sid)
    assert len(kept) == M.owned_runs(k)
    for j, kl in enumerate(kept):
        full = len([g for g in L.g[df18] if g >= P.RUN * j])
        assert 0 < len(kl) < full, (sid, j, len(kl), full)
    assert len({tuple(c[0] for c in kl) for kl in kept}) > 1


@pytest.mark.parametrize("front", P.BATCH_FRONTS)
def test_batch_expectations_equal_the_direct_oracle(oracle, front):
    """Per front end: the pattern begins with exact quiet, its coverage of a K = 2 tile over the 460 quiet prefixes is complete,
    and the lists, frames and Try/Ok expected of capture j -- the unshifted pattern's moved by 28 j, cut at the capture's own
    n_offsets, decoded by front_records_cases.greedy -- equal oracle.scan_all and oracle.demod_power of that capture, built as an
    array of its own, at j = 0, 1, 27 and 459."""
    p = P.pattern(front)
    quiet = np.full((P.QUIET * p.per,) + p.x.shape[1:], p.quiet, p.x.dtype)
    assert np.array_equal(p.x[:quiet.shape[0]], quiet) and np.any(p.x[quiet.shape[0]:quiet.shape[0] + 64] != p.quiet)
    fewest = P.check_coverage(p.L, P.BATCH_K, True, batch=True)
    print(front, "fewest hits per tile-relative offset:", fewest, "; candidates", len(p.L.g[True]), "tries", p.L.tg[True].size)
    assert P.frame_groups(p.L)[-1][-1] == p.L.n_off - 1
    if front == "iq8":                                       # amplitudes that fit: nothing clips
        assert p.x.dtype == np.int8 and -128 < int(p.x.min()) and int(p.x.max()) < 127 and int(np.abs(p.x).max()) > 60
    for j in P.DIRECT_SHIFTS:
        n, cands, tries, frames, stats = p.expected(j)
        xs = p.shifted(j)
        assert len(xs) == n and p.offsets(n) == p.L.n_off + P.RUN * j
        a = p.power_of(xs)
        cc, tt = oracle.scan_all(a, 0, p.offsets(n), True)
        assert [c + (0,) for c in cc] == cands and np.array_equal(tt, tries), (front, j)
        wf, ws = oracle.decode(xs, df18=True) if front == "real" else oracle.demod_power(a, df18=True)
        assert F._records(wf) == F._records(frames) and len(wf) > 30, (front, j)
        assert ws["try"] == stats["try"] and ws["ok"] == stats["ok"], (front, j)


def test_a_weakened_sweep_fails_the_coverage_assertion(oracle, L):
    """The coverage assertion is no formality: without the nudge i mod 28 every frame sits at one r, with half the shifts half
    of the runs are never reached, without the short frames there is no short candidate -- each fails check_coverage."""
    with pytest.raises(AssertionError):
        P.check_coverage(L, 2, True, js=range(M.owned_runs(2) // 2))
    with pytest.raises(AssertionError):
        P.check_coverage(L, 7, True, js=range(0, M.owned_runs(7), 2))
    with pytest.raises(AssertionError):
        P.check_coverage(P.pattern("iq").L, P.BATCH_K, True, js=range(P.BATCH_SHIFTS // 2), batch=True)
    x = P.sweep_capture(frames=P.planted(7001, P.frame_offsets(nudge=lambda i: 0)))
    flat = P.Lists(oracle, oracle.power(x), P.G_MAX)
    assert len(flat.g[True]) >= 200
    with pytest.raises(AssertionError):
        P.check_coverage(flat, 2, True)
    x = P.sweep_capture(frames=P.planted(7001)[:28])
    longs = P.Lists(oracle, oracle.power(x), P.G_MAX)
    with pytest.raises(AssertionError):
        P.check_coverage(longs, 2, True)
