"""The wrap_stream fixture (tests/wrap_model.py, minted by tools/mint_wrap_stream.py through the real reference chain over
7 * 2^32 + 2^21 samples) on the CPU: the model of the front end across a counter wrap, the restatement started just below
a wrap, the conditions that make the fixture able to tell a wrong ring phase or a missing transient from the truth, the
packet formats at ts beyond 2^32, and the seam kernel's build."""
import os
import re
import subprocess

import numpy as np
import pytest

import wrap_model as W
from conftest import ROOT


@pytest.fixture(scope="module")
def fixture():
    return W.load()


def _jumped_before(run, first_g):
    return sum(W.SPAN[len(bytes.fromhex(f["frame"]))] - 1 for f in run["frames"] if f["g"] < first_g)


def test_fixture_shape(fixture):
    rec, bursts, runs = fixture
    assert rec["n_samples"] == W.N == 7 * (1 << 32) + (1 << 21)
    wraps = sorted(w for _, _, w in bursts.values() if w)
    assert wraps == [1, 2, 3, 4, 5, 6, 7]
    assert len({s % 28 for s, _, w in bursts.values() if w}) == 7           # another position against the run grid per wrap
    for name, (s, y, w) in bursts.items():
        assert s % 8 == 0 and y.size % 8 == 0 and y.max() <= 4095, name
        if w:
            assert s < w * (1 << 32) < s + y.size, name                    # across the wrap
    s, y, _ = bursts["mid"]
    assert min(abs(s - k * (1 << 32)) for k in range(9)) >= 1 << 20 and min(abs(s + y.size - k * (1 << 32)) for k in range(9)) >= 1 << 20
    assert s >> 32 >= 1
    s, y, _ = bursts["end"]
    assert s + y.size == W.N
    biggest = max(os.path.getsize(os.path.join(W.DIR, f)) for f in os.listdir(W.DIR))
    assert biggest < 1002053
    for df18 in (False, True):
        for name in bursts:
            assert len(W.records(runs[df18], name)) > 20, name
        g_last = max(f["g"] for f in runs[df18]["frames"])
        assert g_last > W.N // 2 - W.TAIL - 60000                          # frames up to the end-of-file horizon


def test_model_against_a_literal_walk_of_the_ring(fixture):
    """air.c:59-92 word for word with a uint32 counter started below the wrap, against the model's closed form: every power
    sample bit for bit, for the seven wraps; the two wrong modes differ from it, no_transient exactly at P - 1 .. P + 5."""
    T = np.concatenate([W.TAPS, W.TAPS])
    rng = np.random.default_rng(5)
    for w in range(1, 9):
        fs = w * (1 << 32) - 1200 - 4 * w
        y = rng.integers(900, 3200, 2400).astype(np.uint16)
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
        assert np.array_equal(W.power(y, fs, "true").view(np.uint32), lit.view(np.uint32)), w
        P, g0 = w * W.E, fs // 2
        nt = W.power(y, fs, "no_transient", wrap=w)
        assert [int(k) + g0 - P for k in np.nonzero(nt != lit)[0]] == [-1, 0, 1, 2, 3, 4, 5], w
        st = W.power(y, fs, "stale_phase", wrap=w)
        assert np.array_equal(st[: P - g0 - 1], lit[: P - g0 - 1]) and (st != lit).sum() > 100, w


def test_the_restatement_started_below_a_wrap_is_the_restatement_fed_from_sample_zero(oracle):
    """The shortcut that W.standin takes (orc_state_t with fidx, gbase and ts preset instead of 2^32 samples of silence in
    front), pinned once on a stream short enough to feed whole: silence, then a burst, from sample 0."""
    from tools import gen_signal as G
    x, _ = G.sparse_capture(1 << 18, 30, seed=3, dfs=(17, 11, 18))
    lead = 28 * 4000 + 8
    whole = np.concatenate([np.full(lead, W.SILENCE, np.uint16), x, np.full(W.SILENCE_AFTER, W.SILENCE, np.uint16)])
    for df18 in (False, True):
        want, wstats = oracle.decode(whole, df18=df18)
        got, gstats = W.standin(x, lead, df18)
        assert got == [(f["g"], f["ts"], f["pw"], f["frame"]) for f in want] and len(got) > 20
        assert gstats == wstats
        mf, mstats = W.demod(W.power(x, lead, "true"), lead, df18)
        assert [(g, d + g, pw, fr) for g, d, pw, fr in mf] == got and mstats == wstats


@pytest.mark.parametrize("df18", [False, True])
def test_fixture_equals_model_and_restatement_and_is_sensitive(fixture, df18):
    """Every burst but the last (which lies across the end-of-file horizon of the whole stream): the reference's records are
    those of the true model and of the restatement started just below the burst; the Try/Ok table is the sum over the bursts
    plus the last burst's share.  For every wrap burst, stale_phase and no_transient each differ from the reference in a frame
    field or a Try count: no burst is exempt."""
    _, bursts, runs = fixture
    run = runs[df18]
    total = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for name, (s, y, w) in sorted(bursts.items(), key=lambda b: b[1][0]):
        if name == "end":
            continue
        mine = W.records(run, name)
        jumped = _jumped_before(run, s // 2)
        a = W.power(y, s, "true")
        mf, mstats = W.demod(a, s, df18)
        assert [(g, d + g - jumped, pw, fr) for g, d, pw, fr in mf] == mine, name
        sf, sstats = W.standin(y, s, df18)
        assert [(g, ts - jumped, pw, fr) for g, ts, pw, fr in sf] == mine and sstats == mstats, name
        for k in total:
            for d in total[k]:
                total[k][d] += mstats[k][d]
        if w:
            P = w * W.E
            # Y, decoded at P - 635 or one offset earlier: its bit 55 compares a[g + 630] with a[g + 635], a transient sample
            assert any(len(fr) == 7 and P - 1 <= g + 635 <= P + 5 for g, _, _, fr in mine), name
            assert not any(P - 635 < g < P + 1204 for g, _, _, _ in mine), name          # D at P + 5 is a Try and no Ok
            assert any(g < P - 1196 for g, _, _, _ in mine) and any(g > P + 1200 for g, _, _, _ in mine)
            for mode in W.MODES[1:]:
                wf, wstats = W.demod(W.power(y, s, mode, wrap=w), s, df18)
                assert (wf, wstats) != (mf, mstats), f"{name}: {mode} gives the reference's records: the burst cannot tell"
    rest = {k: {d: run["stats"][k][d] - total[k][d] for d in total[k]} for k in total}
    assert all(v >= 0 for k in rest for v in rest[k].values())
    assert sum(rest["ok"].values()) == len(W.records(run, "end"))


def test_format_frame_at_the_largest_ts(capi, oracle, fixture):
    """adsb_format_frame against formatpkt (output.c:204-262) where ts * 12 / 10 is far beyond 32 bits: all three formats."""
    _, _, runs = fixture
    f = max(runs[True]["frames"], key=lambda f: f["ts"])
    assert f["ts"] > 6 * W.E + (1 << 30)                                   # (ts = g + 1 - the offsets jumped: 34 bits)
    fr = dict(ts=f["ts"], pw=f["pw"], frame=bytes.fromhex(f["frame"]))
    for fmt in (0, 1, 2):
        assert capi.format_frame(fr, fmt) == oracle.formatpkt(fr["frame"], fr["ts"], fr["pw"], fmt), fmt
    assert capi.format_frame(fr, 1).decode() == f["mlat"]                # ... and the reference's own MLAT line
    short = next(g for g in reversed(runs[True]["frames"]) if len(g["frame"]) == 14)
    fr = dict(ts=short["ts"], pw=short["pw"], frame=bytes.fromhex(short["frame"]))
    assert capi.format_frame(fr, 1).decode() == short["mlat"]


def test_seam_kernel_build():
    """seam_kernel.hip for gfx950: no scratch, and NO fused multiply-add at all -- its power samples come from power_ordered<>
    (power_ordered.h, shared with the scan kernel's pw_at, which has none either: tests/test_build_flags.py counts the scan
    kernel's fused forms, all of them in the FIR of a run and the sign tests) and from the ring rule, written as separate
    products and sums."""
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "seam_kernel.hip")
    assert "seam_kernel.hip" in _build.HIP_SOURCES
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    isa = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and "seam_kernel" in next(iter(sizes)) and int(next(iter(sizes.values()))) == 0
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)", isa, flags=re.M)   # (the pattern of test_build_flags.py)
    assert fused == []
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", isa).group(1))
    assert lds < 16 * 1024
    assert len(re.findall(r"^\s*v_pk_mul_f32|^\s*v_mul_f32", isa, flags=re.M)) >= 8      # products and squares stay products
    # the scan kernel's shared power code moved to a header, nothing else: the two kernels include the same file
    for f in ("scan_kernel.hip", "seam_kernel.hip"):
        assert '#include "power_ordered.h"' in open(os.path.join(ROOT, "adsbdec_amd", "csrc", f)).read(), f


def test_switch_is_declared_and_default_is_off(capi):
    L = capi.load()
    for name in ("adsb_set_long_stream", "adsb_get_wraps", "adsb_multi_set_long_streams"):
        assert hasattr(L, name), name
    assert L.adsb_set_long_stream(None, 1) == -1 and L.adsb_get_wraps(None, None, None) == -1
    assert L.adsb_multi_set_long_streams(None, 1) == -1
    assert L.adsb_abi_version() == 5
