"""The expectation the seam kernel is held to (tests/wrap_seam_cases.py), on the CPU: the model at the wraps the cases use
against a literal walk of the ring, the conditions that keep the cases from being vacuous, and which expected value each wrong
model changes -- the reason the kernel's power samples are compared bit for bit (adsb_seam_power) and not its lists alone."""
import numpy as np
import pytest

import wrap_model as W
import wrap_seam_cases as S


@pytest.mark.parametrize("w", S.WRAPS)
def test_model_against_a_literal_walk_of_the_ring_at_the_cases_wraps(w):
    """test_wrap_stream_cpu's literal walk (air.c:59-92 word for word, a uint32 counter started below the wrap) at w = 1, 2 and
    1 000 003, whose sample numbers need 52 bits: every power sample bit for bit; ring_sample, which the reversed-sum model is
    built from, gives the same seven transient samples in slot order 0 .. 6, and others in order 6 .. 0."""
    T = np.concatenate([W.TAPS, W.TAPS])
    rng = np.random.default_rng(50 + w % 7)
    fs = w * (1 << 32) - 1200 - 4 * (w % 5)
    y = rng.integers(0, 65536, 2400).astype(np.uint16)
    ring = np.zeros(14, np.float32)
    fidx, out, i = fs % (1 << 32), [], 0
    while i < y.size:
        for sign in (np.float32(1), np.float32(-1)):
            for _ in range(2):
                ring[fidx % 14] = sign * (np.float32(y[i]) - np.float32(2048))
                i += 1
                fidx = (fidx + 1) & 0xFFFFFFFF
            o = 14 - fidx % 14
            si = sq = np.float32(0)
            for k in range(0, 14, 2):
                si = np.float32(si + np.float32(T[k + o] * ring[k]))
                sq = np.float32(sq + np.float32(T[k + 1 + o] * ring[k + 1]))
            out.append(np.float32(np.float32(si * si) + np.float32(sq * sq)))
    lit = np.array(out, np.float32)
    model = W.power(y, fs, "true", wrap=w)
    assert np.array_equal(model.view(np.uint32), lit.view(np.uint32))
    P, g0 = w * W.E, fs // 2
    fwd = np.array([S.ring_sample(y, fs, P + k) for k in S.TRANSIENT], np.float32)
    rev = np.array([S.ring_sample(y, fs, P + k, order=range(6, -1, -1)) for k in S.TRANSIENT], np.float32)
    assert np.array_equal(fwd.view(np.uint32), lit[P - 1 - g0: P + 6 - g0].view(np.uint32))
    assert not np.array_equal(rev.view(np.uint32), fwd.view(np.uint32))


def test_the_ring_phase_is_the_same_at_every_wrap():
    """(q mod 2^31) mod 7 restarts at 0 at every wrap: a window's power does not depend on w, bit for bit.  What the wraps of the
    cases vary is the index arithmetic; what varies the content against P - 1 .. P + 5 is the placement."""
    for kind in ("dense", "uniform"):
        y = S.window(kind, S.PLACEMENTS[0])
        a = [S.power(y, w) for w in S.WRAPS]
        assert all(np.array_equal(a[0].view(np.uint32), b.view(np.uint32)) for b in a[1:]), kind
    assert len({p // 2 % 2 for p in S.PLACEMENTS}) == 2 and len(S.PLACEMENTS) >= 4     # starts an odd number of power samples apart


def _seam_totals(oracle, placement, w=1):
    _, _, P = S.offsets(w)
    cands, n_tries = [], 0
    for kind in S.KINDS:
        c, t = S.seam_lists(oracle, S.power(S.window(kind, placement), w), w, True)
        cands += c
        n_tries += t.size
    return P, cands, n_tries


@pytest.mark.parametrize("placement", S.PLACEMENTS)
def test_the_cases_are_not_vacuous(oracle, placement):
    """At every placement, summed over the nine kinds (df18 on): the seam offsets hold material to compare."""
    P, cands, n_tries = _seam_totals(oracle, placement)
    print(placement, len(cands), n_tries)
    assert len(cands) >= 15 and n_tries >= 150
    assert any(len(c[2]) == 7 for c in cands) and any(len(c[2]) == 14 for c in cands)
    assert any(P - 1 <= c[0] <= P + 5 for c in cands)                    # decoded AT a transient sample
    assert any(P - 1 <= S.last_read(c) <= P + 5 for c in cands)          # the last sample of its window is one


def test_the_capture_as_it_is_holds_what_was_measured(oracle):
    """make_captures(65536) itself centred on the wrap (S.ZERO): 21 candidates and 182 try words in the seam offsets, but none
    decoded at P - 1 .. P + 5 -- which is why the placements are cuts of a longer capture.  It stays a case of the GPU tests."""
    P, cands, n_tries = _seam_totals(oracle, S.ZERO)
    assert (len(cands), n_tries) == (21, 182)
    assert not any(P - 1 <= c[0] <= P + 5 for c in cands)


@pytest.mark.parametrize("placement", S.PLACEMENTS)
def test_what_each_wrong_model_changes(oracle, placement):
    """The sensitivity table.  Every wrong model changes an expected value at every placement; the transient's products added in
    the reverse order change power bits ONLY -- no candidate, no try word of any kind for either df18 setting: lists cannot see a
    rounding-order error, the bit-for-bit comparison of the kernel's power samples can."""
    table = S.sensitivity(oracle, placement)
    print(placement, {m: {k: len(v) for k, v in r.items()} for m, r in table.items()})
    for mode, row in table.items():
        assert row["lists"] or row["bits"], mode
        assert set(row["lists"]) <= set(row["bits"]), mode                # (a list changes only where a sample does)
    assert table["stale_phase"]["lists"] and table["no_transient"]["lists"]
    assert table["reversed_sum"]["lists"] == [] and len(table["reversed_sum"]["bits"]) >= 5
    assert table["shifted_transient"]["bits"]


def test_damaged_long_frames_start_in_the_seam_offsets(oracle):
    """What the 1-bit repair test of the GPU file stands on.  A window holds one damaged frame start in the seam offsets (long
    frames are 1 200 offsets long, the seam 1 224), so the placements of the `damaged` kind bring DIFFERENT damaged frames
    there: at each at least three seam offsets decode a long frame that one flipped bit mends (the half-sample copies of one
    frame), the oracle's list (no repair) has none of them, and over the placements the mended frames are at least three
    distinct ones with distinct damaged bits, in all four column words of the slicer (bytes 0-3, 4-7, 8-11, 12-13)."""
    w = 1
    frames, bits = set(), set()
    for placement in S.DAMAGED_PLACEMENTS:
        a = S.power(S.damaged_window(placement), w)
        fixed = S.repairable(oracle, a, w)
        plain, _ = S.seam_lists(oracle, a, w, True)
        assert len(fixed) >= 3 and not {f[0] for f in fixed} & {c[0] for c in plain}, placement
        assert all(oracle.crc_residual(f[2]) == 0 for f in fixed)
        assert len({f[2] for f in fixed}) == 1 and len({f[3] for f in fixed}) == 1, placement   # one frame start per window
        frames.add(fixed[0][2])
        bits.add(fixed[0][3])
    assert len(frames) == len(bits) == len(S.DAMAGED_PLACEMENTS) >= 3
    assert {b >> 5 for b in bits} == {0, 1, 2, 3}


def test_the_two_diagnostic_calls_are_declared(capi):
    L = capi.load()
    assert L.adsb_scan_wrap_window(None, None, 0, 0, 0, 0, None, 0, None, None, 0, None) == -1
    assert L.adsb_seam_power(None, None, 0, 0, 0, 0, 0, None, 0) == -1
    assert L.adsb_abi_version() == 5
