"""What keeps tests/test_gpu_guarded.py from passing vacuously, from the oracle and numpy alone: every guard of
tests/guarded_cases.py can be SEEN -- reading it instead of what the call was given changes a record, a try word, a power sample or
a counter -- and inputs weakened in the three ways that would blind the device tests fail these checks.  No mutated library is
built or run anywhere: a build with a loosened bound reads memory it was not given; these proofs stand in its place."""
import numpy as np
import pytest

import front_records_cases as F
import guarded_cases as G
import iq8_cases as Q
from test_gpu_batch_records import EDGES, _edge_capture


# ---------------------------------------------------------------- section 1
def test_piece_sizes_hit_every_class():
    """Against kInPlaceMinSamples and kSeamSamples as csrc/decoder_state.hpp states them: a piece exactly at the minimum, a larger
    multiple of 8 in place behind a seam copy, a short one just above the seam copy staged between in-place pieces, a piece that
    leaves the next at 4 mod 8 -- which is then staged although it is long --, a last one in place with _final; in both orders;
    the ten cuts far enough apart for their planted frames."""
    k = G.header_constants()
    assert k["kInPlaceMinSamples"] == G.MIN == 65_536 and k["kSeamSamples"] == G.SEAM == 4096
    assert G.check_sizes(G.SIZES) and G.check_sizes(G.SIZES_PACKED, packed=True)
    assert G.GUARD >= 8192 and G.GUARD > G.SEAM and 2 * G.GUARD > 7 * 1024
    fwd = [road for _, _, road, _ in G.roads(G.SIZES)]
    assert fwd == ["in_place", "in_place", "staged", "in_place", "staged", "in_place"]
    assert [road for _, _, road, _ in G.roads(G.SIZES[::-1])] == ["in_place", "in_place", "staged", "staged", "in_place", "in_place"]
    # sizes that miss a class are refused: no short piece; nothing at 4 mod 8
    with pytest.raises(AssertionError):
        G.check_sizes((G.MIN, G.MIN + 8 * 6808, G.MIN + 8, G.MIN + 4, G.MIN + 8 * 1536 + 4, G.TOTAL - (5 * G.MIN + 8 * 8346 + 16)))
    with pytest.raises(AssertionError):
        G.check_sizes(G.SIZES_PACKED)


@pytest.mark.parametrize("kind", G.KINDS)
def test_every_cut_can_be_seen_from_both_sides(kind):
    """Per kind: the planted frames are where the plan puts them and the oracle's greedy decode accepts them; with the decoy as the
    continuation a record or try word of the last 1196 offsets before each cut changes; with the decoy as the predecessor the six
    power samples behind a real cut change and a record behind it, and each guard stretch carries CRC-valid records of its own."""
    s = G.stream(kind)                                       # (checked when it is made: check_sizes, check_stream)
    assert len(s.frames) > 60 and s.stats["ok"][11] >= 10 and s.stats["ok"][17] >= 10 and s.stats["ok"][18] >= 10
    both = sorted(set(G.cuts(s.sizes)) | set(G.cuts(s.sizes[::-1])))
    assert len(both) == 10 and len(G.plan(s.sizes)) == 20
    long_across = [df != 11 for _, df, role, _ in G.plan(s.sizes) if role == "across"]
    assert sum(long_across) >= 4 and len(long_across) - sum(long_across) >= 4            # long and DF11 alternate over the cuts
    if kind == "power":
        from adsbdec_amd.sample_formats import power_domain_ok
        assert power_domain_ok(s.x) and power_domain_ok(s.decoy) and float(s.decoy.max()) > 4 * float(s.x.max())
    assert s.decoy_g.size > 300                              # the decoy is a frame-carrying capture, back to back


@pytest.mark.parametrize("kind", ("real", "iq", "iq8", "power"))
def test_weakened_inputs_fail_the_checks(kind):
    """The checks are no formality.  Guards of silence carry no record; guards that are the true neighbours change nothing; frames
    moved 2000 offsets away from the cuts leave nothing across or behind them."""
    s = G.stream(kind)
    silence = np.full_like(s.x, 0x800) if s.x.dtype == np.uint16 else np.zeros_like(s.x)
    for c in G.cuts(s.sizes):
        with pytest.raises(AssertionError):
            G.check_cut(s, c, silence)
        with pytest.raises(AssertionError):
            G.check_cut(s, c, s.x)
    moved = G.make_stream(kind, shift=2000)
    with pytest.raises(AssertionError):
        G.check_planted(moved)
    for c in G.cuts(s.sizes)[:2]:
        with pytest.raises(AssertionError):
            G.check_cut(moved, c, moved.decoy)


@pytest.mark.parametrize("front", list(G.FRONTS))
def test_guarded_pieces_are_the_stream_between_the_decoy(front):
    """What a front's tensors hold, read back on the host: every piece starts 16-byte aligned behind 8192 units of the decoy's
    stretch in front of the cut and ends in front of the decoy's stretch behind it; the pieces concatenate to the capture; the
    exact twins convert back to it."""
    from adsbdec_amd import sample_formats as S
    from adsbdec_amd.packed12 import unpack12
    kind, _, fmt = G.FRONTS[front]
    s = G.stream(kind)
    back = {"s16": lambda b: S.from_int16_real(b.view("<i2"))[0], "f32": lambda b: S.from_float32_real(b.view("<f4"))[0],
            "packed": unpack12, "iqf32": lambda b: S.to_int16_iq(b.view("<f4"))[0]}.get(front, lambda b: b.view(s.x.dtype))
    ub = G.unit_bytes(front)
    for sizes in (s.sizes, s.sizes[::-1]):
        whole = []
        for at, n, _, _ in G.roads(sizes):
            b, lead = G.guarded(front, s, at, at + n)
            assert lead % 16 == 0 and lead == int(G.GUARD * ub) and b.size == lead + int(n * ub) + lead
            flat = back(b)
            lo, hi = G.GUARD // G.UPE[kind], (G.GUARD + n) // G.UPE[kind]
            whole.append(flat[lo:hi])
            if at >= G.GUARD:
                assert np.array_equal(flat[:lo], s.decoy[s.sl(at - G.GUARD, at)])
            if at + n + G.GUARD <= G.TOTAL:
                assert np.array_equal(flat[hi:], s.decoy[s.sl(at + n, at + n + G.GUARD)])
            assert not np.array_equal(flat[:lo], s.x[s.sl(max(at, G.GUARD) - G.GUARD, max(at, G.GUARD))])
        assert np.array_equal(np.concatenate(whole), s.x)
        assert sum(G.count_of(front, n) for n in sizes) == G.count_of(front, G.TOTAL)


# ---------------------------------------------------------------- section 2
def test_real_edge_captures_see_a_loud_front_guard(oracle):
    """Each of the five: n % 4 as named, g = 3 .. 6 are candidates of the capture alone, and exactly its six first power samples
    change under loud codes in front -- with silence there (the weakened guard) nothing changes and the check fails."""
    for i, name in enumerate(EDGES):
        x = _edge_capture(i)
        assert x.size % 4 == (0, 1, 2, 3, 0)[i]
        a = oracle.power(x)
        gs = [r[0] for r in oracle.scan_all(a, 0, 2 * (x.size // 4) - 1195, True)[0]]
        assert gs[:4] == [3, 4, 5, 6], (name, gs[:6])
        assert G.check_first_six(x, G.loud_codes(G.LOUD_GUARD, 8300 + i))
        with pytest.raises(AssertionError):
            G.check_first_six(x, np.full(G.LOUD_GUARD, 0x800, np.uint16))


@pytest.mark.parametrize("front", ("iq", "power", "iq8"))
def test_edge_captures_without_a_fir_start_on_their_first_offsets(front):
    """These kernels have no FIR: an offset reads nothing in front of it, so a loud front guard shows only through a scan that
    starts below the capture -- the candidates at g = 0 .. 3 are what such a scan would move or precede."""
    cases = Q.cases() if front == "iq8" else F.cases(front)
    for i, name in enumerate(EDGES):
        c = cases[name]
        gs = [r[0] for r in c.ev[True][0]]
        assert c.n % 4 == (0, 1, 2, 3, 0)[i] and gs[:4] == [0, 1, 2, 3], (front, name, gs[:6])
        assert len(c.dec[(True, False)][0]) >= 1 and c.dec[(True, False)][0][0]["g"] == 0


# ---------------------------------------------------------------- section 3
def test_the_loud_captures_are_longer_and_never_silence():
    edge = max(_edge_capture(i).size for i in range(5))
    loud = G.loud_codes(4 * edge + 8, 8400)
    assert loud.size >= 4 * edge and G.never_silence(loud)
    from adsbdec_amd import sample_formats as S
    assert G.never_silence(S.to_int16_real(loud)) and G.never_silence(S.to_float32_real(loud))
    liq = G.loud_iq(0, 4 * 42_008, 8401)
    assert liq.dtype == np.float32 and len(liq) >= 4 * 42_008 and G.never_silence(liq)
    assert not G.never_silence(np.array([1, 0x800], np.uint16)) and not G.never_silence(np.array([1.0, 0.0], np.float32))


@pytest.mark.parametrize("road", list(G.BATCH_ROADS))
def test_a_batch_behind_the_loud_batch_lies_in_what_it_wrote(road):
    """Per road of test_batches_into_buffers_that_held_a_loud_batch and per buffer the road fills -- what the call is given, landed at
    16 bytes (the _as and packed host batches) or 128, and the 16-bit samples a packed or converted batch leaves in batch_unpacked at
    128: the loud batch is three captures of three lengths, none of them silence; the target batch is shorter in all, so each of its
    captures lies in bytes the loud batch wrote, and those bytes are not its own; the empty capture in the middle takes no room.  A
    loud batch of one length only, or one shorter than the targets, fails the check."""
    family, form, _, on_device = G.BATCH_ROADS[road]
    if family == "iq":
        loud = G.loud_batch(G.loud_iq(2, 4 * len(F._iq_edge(1)), 8401))
        targets = [F._iq_edge(1)] + [np.ascontiguousarray(F._iq_edge(2)[:G.N_AROUND // 2 + j]) for j in range(4)]
    else:
        edge, base = _edge_capture(1), _edge_capture(2)
        loud = G.loud_batch(G.loud_codes(4 * edge.size + 8 - (4 * edge.size) % 8, 8400))
        targets = [edge] + [np.ascontiguousarray(base[:G.N_AROUND + j]) for j in range(8)]
        if family == "packed":
            from test_gpu_batch_packed import packable
            targets = [packable(edge), np.ascontiguousarray(base[:G.N_AROUND]), np.ascontiguousarray(base[:G.N_AROUND + 8])]
    targets, mid = G.with_an_empty_capture(targets)
    assert 0 < mid < len(targets) - 1 and len(targets[mid]) == 0 and all(len(x) for i, x in enumerate(targets) if i != mid)
    assert all(len(x) >= 4 * G.N_AROUND // (2 if family == "iq" else 1) for x in loud) and all(G.never_silence(x) for x in loud)
    given = lambda caps: [G.batch_form(form, x) for x in caps]
    assert form == "packed" or all(G.never_silence(a) for a in given(loud))      # (packed bytes: a zero byte is no silence)
    if not on_device:                                                            # the landing buffer: batch_in or batch_land
        assert G.check_stale_batch_shows(given(loud), given(targets), 16 if form in ("s16", "f32", "packed") else 128)
    if form in ("s16", "f32", "packed", "iqf32"):                                # batch_unpacked: codes, or int16 scalars
        assert G.check_stale_batch_shows(loud, targets, 128)
    at, _ = G.slots([np.asarray(x).nbytes for x in targets], 128)
    assert at[mid] == at[mid + 1]
    with pytest.raises(AssertionError):
        G.check_stale_batch_shows([loud[0]] * 3, targets, 128)
    with pytest.raises(AssertionError):
        G.check_stale_batch_shows([x[:len(targets[0]) // 4] for x in loud], targets, 128)


# ---------------------------------------------------------------- section 4
def test_guards_of_the_exports_can_be_seen(oracle):
    """Real: the first six floats differ between silence and the guard in front, at every length; every kind: the guards hold a code
    on each rail, so reading them would move the counters."""
    for i, n in enumerate(G.REAL_LENGTHS):
        x = np.random.default_rng(8500 + i).integers(0, 4096, n, dtype=np.uint16)
        guard = G.loud_codes(G.LOUD_GUARD, 8510 + i)
        assert G.check_first_six(x, guard) and G.check_rails(guard, "real") and G.check_rails(G.loud_codes(G.LOUD_GUARD, 8511 + i), "real")
        with pytest.raises(AssertionError):
            G.check_first_six(x, np.full(G.LOUD_GUARD, 0x800, np.uint16))
    with pytest.raises(AssertionError):
        G.check_rails(G.loud_codes(G.LOUD_GUARD, 1, rails=False)[3:40] | 1, "real")
    for fmt in (2, 0, 8):
        for skew in (0, 1):
            g = G.loud_iq(fmt, G.LOUD_GUARD + skew, 8610)
            grid = g if fmt != 0 else (g * 32768.0).astype(np.int16)
            assert G.check_rails(grid, "iq8" if fmt == 8 else "iq16") and G.never_silence(g)
    assert G.never_silence(G.loud_power(G.LOUD_GUARD + 1, 8610))
    assert G.REAL_LENGTHS == (56, 3584 + 4, 14336 + 6, 2 * (3 * 7168 + 30) + 3) and G.IQ_LENGTHS == (1, 27, 1792, 1793, 3 * 7168 + 45)
