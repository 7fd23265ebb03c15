"""Decoding past sample 2^31, up to the last sample of the longest stream (2^32 - 4), on the CPU.

* the shift rule (tests/long_stream.py) on the restatement, at FIR phases and deqframe call boundaries, and on the real
  chain where oracle/_ref is built;
* the committed long_stream fixture (the real chain over all 2^32 - 4 samples) against the restatement: b1 and b2 under the
  shift rule, every frame of b3 offset by offset;
* the host resolver and the shard stitcher at a total of 2^32 - 4: the bursts' exhaustive candidates and tries, moved to
  their stream positions, resolved in 8 and 13 shards, stitched -- equal to the fixture, frames and Try/Ok table."""
import numpy as np
import pytest

import long_stream as LS
import shard_helpers
from oracle import oracle as O

FIRST_CALL = 2 * 40980          # input samples at which aidx first reaches APBUFFSZ (air.c:94)


@pytest.fixture(scope="module")
def fixture():
    O.build()
    return LS.load()


def _ts_checked(recs):
    """ts == g + 1 - sum(span - 1) over the frames before (demod.c:86,99,128,134)."""
    skipped = 0
    for g, ts, _, fr in recs:
        assert ts == g + 1 - skipped, (g, ts)
        skipped += LS.SPAN[len(fr)] - 1
    return skipped


def _shift_rule(decode, y, F, **kw):
    """decode(silence(F) ++ y ++ silence) against decode(silence(F mod 28) ++ y ++ silence), moved by the rule."""
    x, shift = LS.padded(F, y, lead=F)
    far, fstats = decode(x, **kw)
    x, shift = LS.padded(F, y)
    near, nstats = decode(x, **kw)
    assert shift == (F - F % 28) // 2
    return far, fstats, near, nstats, shift


@pytest.mark.parametrize("df18", [False, True])
def test_shift_rule_on_the_restatement(fixture, df18):
    """F at every kind of place: multiples of 28, other FIR phases, b2 across the first deqframe call and across later call
    boundaries, and F of tens of millions of samples -- the records move by (F - F mod 28) / 2, the table stays."""
    _, bursts, _ = fixture
    y = bursts["b2"][1]
    n_frames = 0
    for F in (0, 3, 16, 28, 28 * 1001 + 12, FIRST_CALL - y.size // 2, FIRST_CALL - 1200 * 2 + 8, 5 * FIRST_CALL - 2 * 1200 * 5 + 19,
              (1 << 22) + 4, (1 << 24) + 28 * 7, (1 << 25) - 5):
        far, fstats, near, nstats, shift = _shift_rule(O.decode, y, F, df18=df18)
        assert [(f["g"], f["ts"], f["pw"], f["frame"]) for f in far] == \
            [(f["g"] + shift, f["ts"] + shift, f["pw"], f["frame"]) for f in near], F
        assert fstats == nstats, F
        n_frames += len(far)
    assert n_frames > 10 * 11
    # with the 1-bit repair extension too (the GPU tests compare against it through this rule)
    for F in (12, (1 << 23) + 20):
        far, fstats, near, nstats, shift = _shift_rule(O.decode, y, F, df18=df18, fix1=True)
        assert [(f["g"], f["pw"], f["frame"]) for f in far] == [(f["g"] + shift, f["pw"], f["frame"]) for f in near], F
        assert fstats == nstats and fstats["fixed"] > 0, F


@pytest.mark.skipif(not O.ref_available(), reason="the real chain (oracle/_ref) is built only where the reference sources are")
def test_shift_rule_on_the_real_chain(fixture):
    """The same rule on the reference's own decodeiq / deqframe / valid.c, with up to 2^26 samples of silence in front."""
    _, bursts, _ = fixture
    y = bursts["b1"][1][: 1 << 17]
    base = None
    for F in (FIRST_CALL - 20000 + 12, (1 << 20) + 12, (1 << 26) + 12):
        silence = np.full(1 << 22, LS.SILENCE, np.uint16)
        lead = [silence[: min(silence.size, F - k)] for k in range(0, F, silence.size)]
        tail = np.full(LS.SILENCE_AFTER, LS.SILENCE, np.uint16)
        frames, stats = O.ref_decode_pieces(lead + [y, tail], df18=True)
        got = [(f["ts"] - F // 2, f["pw"], f["frame"], f["avr"]) for f in frames]
        if base is None:
            base = (got, stats)
            assert len(got) > 10
        assert (got, stats) == base, F


@pytest.mark.parametrize("df18", [False, True])
def test_the_fixture_follows_the_restatement(fixture, df18):
    """b1 and b2 of the fixture equal the restatement on their stand-ins, moved by the rule (ts also past the frames of the
    bursts before); every frame of b3 is the restatement's evaluation of its offset on power at the stream's phase; b3 holds
    frames beyond the horizon that the reference never reached; the table is b1's + b2's + what b3 reached."""
    rec, bursts, runs = fixture
    run = runs[df18]
    assert rec["n_samples"] == LS.N
    allrec = LS.records(run)
    assert [r[0] for r in allrec] == sorted(r[0] for r in allrec)
    _ts_checked(allrec)
    skipped, stats = 0, {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for name in ("b1", "b2"):
        s, y = bursts[name]
        x, shift = LS.padded(s, y)
        want, wstats = O.decode(x, df18=df18)
        assert LS.records(run, name) == LS.shifted(want, shift, shift - skipped), name
        skipped += sum(LS.SPAN[len(f["frame"])] - 1 for f in want)
        stats = LS.add_stats(stats, wstats)
    assert bursts["b1"][0] < (1 << 31) < bursts["b1"][0] + bursts["b1"][1].size
    assert any(g < (1 << 30) < g + LS.SPAN[len(fr)] for g, _, _, fr in LS.records(run, "b1"))   # a frame across 2^31
    # b3: pw and bytes offset by offset on power samples at the stream's phase
    s, y = bursts["b3"]
    assert s + y.size == LS.N
    x, shift = LS.padded(s, y, after=0)
    a = O.power(x)
    b3 = LS.records(run, "b3")
    for g, _, pw, fr in b3:
        k, got, gpw = O.eval_offset(a, g - shift, df18)
        assert k >= 2 and (got, gpw) == (fr, pw), g
    cands, tries = O.scan_all(a, 0, a.size - 1195, df18)
    last = b3[-1][0] + LS.SPAN[len(b3[-1][3])]
    beyond = [c for c in cands if c[0] + shift >= last]
    assert len(beyond) >= 3, "b3 must hold frames the reference's end-of-file horizon leaves unread"
    assert b3[-1][0] >= LS.N // 2 - LS.TAIL - 1200                          # ... and frames up to it
    three = run["stats"]
    for k in ("try", "ok"):
        for d in (11, 17, 18):
            assert stats[k][d] <= three[k][d], (k, d)
    assert three["ok"][11] + three["ok"][17] + three["ok"][18] == len(allrec)


def _stream_candidates(bursts, df18):
    """The exhaustive candidates and tries of the whole stream: each burst's, at the stream's phase, moved to its place."""
    cands, tries = [], []
    for name in ("b1", "b2", "b3"):
        s, y = bursts[name]
        x, shift = LS.padded(s, y, after=2400 if name != "b3" else 0)
        a = O.power(x)
        c, t = O.scan_all(a, 0, a.size - 1195, df18)
        cands += [(g + shift, pw, fr) for g, pw, fr in c]
        tries.append(t + np.uint64(shift << 2))
    return cands, np.concatenate(tries)


@pytest.mark.parametrize("n_shards", [8, 13])
@pytest.mark.parametrize("df18", [False, True])
def test_stitched_shards_at_the_longest_stream(capi, fixture, df18, n_shards):
    """The host resolver in chain mode per shard and adsb_stitch_shards_stats over a total of 2^32 - 4 samples: seams inside
    b1 (8 shards: the one at sample 2^31) and b2, the end-of-file horizon inside b3 -- frames and table equal the fixture's,
    which come from the reference run over the whole stream."""
    _, bursts, runs = fixture
    cands, tries = _stream_candidates(bursts, df18)
    plan = capi.plan_shards(LS.N, n_shards)
    seams = [p["g_begin"] for p in plan[1:]]
    if n_shards == 8:
        s1, y1 = bursts["b1"]
        s2, y2 = bursts["b2"]
        assert any(s1 // 2 < g < (s1 + y1.size) // 2 for g in seams)
        assert any(s2 // 2 < g < (s2 + y2.size) // 2 for g in seams)
    ss = shard_helpers.from_candidates(capi, cands, LS.N, n_shards, tries=tries)
    rc, out, stats, _, _ = ss.stitch(with_stats=True)
    assert rc == 0
    assert out == LS.records(runs[df18])
    assert stats == runs[df18]["stats"]
