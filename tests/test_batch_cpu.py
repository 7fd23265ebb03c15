"""A batch of independent captures in one launch (adsb_decode_batch_*), as far as it goes without a GPU: the entry points
exist, the layout in virtual offsets (csrc/batch.hpp through adsb_batch_layout) keeps its promises for any mix of capture
lengths, and the per-capture resolve (adsb_batch_resolve) turns the records of a batch -- here the oracle's, shifted to the
layout's virtual offsets -- into exactly the frames and Try/Ok tables the oracle decodes from every capture alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from candidate_model import RUN, owned_runs
from conftest import ROOT, records

WINDOW, DECOFFSET, APBUFFSZ = 1196, 1200, 40980
GAP = WINDOW + DECOFFSET                                # free virtual offsets behind a capture's last power sample
MAX_LAUNCH = (1 << 30) - RUN * owned_runs(32)           # scan_kernel.h kMaxLaunchOffsets: g_rel has 30 bits


def power_samples(n):
    return 2 * ((n + 3) // 4)                           # air.c:59-92 at end of file


def offsets_of(n):
    """Offsets the reference can visit in a file of n samples: none before its first deqframe call (air.c:94)."""
    m = 2 * (n // 4)
    return m - WINDOW + 1 if power_samples(n) >= APBUFFSZ and m >= WINDOW else 0


def test_entry_points_are_declared_exported_and_bound(capi):
    inc = os.path.join(ROOT, "include")
    strip = lambda h: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
    main, diag = strip("adsbdec_amd.h"), strip("adsbdec_amd_diag.h")
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.load()
    for name, header in (("adsb_decode_batch_device", main), ("adsb_decode_batch_host", main),
                         ("adsb_batch_layout", diag), ("adsb_batch_resolve", diag), ("adsb_batch_layout_ex", diag),
                         ("adsb_batch_resolve_ex", diag), ("adsb_batch_records", diag), ("adsb_batch_unpacked_copy", diag)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\b%s\b" % name, exported) and name in capi.SYMBOLS and hasattr(L, name), name
    assert hasattr(capi.Decoder, "decode_batch") and hasattr(capi.Decoder, "decode_batch_device")
    assert hasattr(capi.Decoder, "batch_records") and hasattr(capi.Decoder, "batch_unpacked")
    assert L.adsb_abi_version() == 5
    # the hooks are the diag header's, and the knob that cuts captures at test sizes is the last member of the knob struct
    assert "adsb_batch_records" not in main and "adsb_batch_unpacked_copy" not in main and "batch_launch_offsets" not in main
    assert re.search(r"int32_t\s+batch_launch_offsets\s*;\s*}\s*adsb_debug_config\s*;", diag)
    assert capi.DebugConfig._fields_[-1][0] == "batch_launch_offsets" == capi.DEBUG_KNOBS[-1]
    assert [f for f, _ in capi.DebugConfig._fields_[1:]] == list(capi.DEBUG_KNOBS)
    assert L.adsb_batch_records(None, None, None, None, None, None, None, None, None) == -1
    assert L.adsb_batch_unpacked_copy(None, 0, None, 0) == -1
    # NULL handle: -1, nothing touched
    assert L.adsb_decode_batch_device(None, 0, None, None, None, None, None) == -1
    assert L.adsb_decode_batch_host(None, 0, None, None, None, None, None) == -1


def launch_limit(launch_offsets, passes):
    """batch.hpp batch_launch_limit: the knob is honoured from one tile of a split launch (K = 7, or the forced K) up to the
    default."""
    return launch_offsets if RUN * owned_runs(passes or 7) <= launch_offsets <= MAX_LAUNCH else MAX_LAUNCH


def check_layout(ns, segs, launches, limit=MAX_LAUNCH):
    assert [s["capture"] for s in segs] == sorted(s["capture"] for s in segs)
    assert sorted(set(s["capture"] for s in segs)) == list(range(len(ns)))          # every capture has a segment
    by_capture = {}
    for s in segs:
        by_capture.setdefault(s["capture"], []).append(s)
    prev_end = None
    for i, n in enumerate(ns):
        parts = by_capture[i]
        # every capture's offsets are covered exactly once, in order
        assert parts[0]["o_begin"] == 0 and parts[-1]["o_end"] == offsets_of(n), (i, n)
        for a, b in zip(parts, parts[1:]):
            assert a["o_end"] == b["o_begin"] and a["o_end"] > a["o_begin"]
        for s in parts:
            assert s["base"] % RUN == 0 and s["o_begin"] % RUN == 0
            if prev_end is not None:
                assert s["base"] >= prev_end + GAP, (i, s, prev_end)              # ascending, at least the stated gap
            # what the segment's offsets read ends a window behind its last one; a capture's last segment, at its last power sample
            reach = s["o_end"] - s["o_begin"] + (WINDOW - 1 if s["o_end"] > s["o_begin"] else 0)
            if s is parts[-1]:
                reach = max(reach, power_samples(n) - s["o_begin"])
            prev_end = s["base"] + reach
    seen = 0
    for li, L in enumerate(launches):
        mine = segs[L["seg_first"]:L["seg_end"]]
        assert L["seg_first"] == seen and mine
        seen = L["seg_end"]
        assert 2 <= L["passes"] <= 32
        tile = RUN * owned_runs(L["passes"])
        assert L["g_end"] - L["g_begin"] <= limit and L["g_begin"] % RUN == 0
        t = 0
        for s in mine:
            assert s["launch"] == li and s["first_tile"] == t
            n_off = s["o_end"] - s["o_begin"]
            assert s["tiles"] == -(-n_off // tile)                                  # its own tiles: the last one partly filled
            # every tile lies inside the segment: tile k owns [base + k tile, min(base + (k + 1) tile, base + n_off))
            assert n_off == 0 or (s["tiles"] - 1) * tile < n_off
            assert n_off == 0 or (L["g_begin"] <= s["base"] and s["base"] + n_off <= L["g_end"])
            if s is not by_capture[s["capture"]][-1]:
                assert n_off % tile == 0                                            # a cut capture is cut between tiles
                assert len(mine) == 1 and n_off == limit // tile * tile             # ... into launches of their own, as full as whole tiles go
            else:
                assert n_off <= limit                                               # what fits a launch is not cut
            t += s["tiles"]
        assert t == L["tiles"]
    assert seen == len(segs)


def test_layout_properties(capi):
    rng = np.random.default_rng(20261)
    special = [0, 3, 2391, 81956, 81957, 81960, (1 << 32) - 4, 2392, 4 * 1196, 1 << 16, (1 << 20) + 1, (1 << 20) + 3]
    cases = [special, [1 << 20] * 256, [(1 << 28)] * 9, [1 << 16] * 2000, [(1 << 32) - 4] * 2 + [5], []]
    for _ in range(12):
        k = int(rng.integers(1, 60))
        ns = [int(v) for v in np.concatenate([rng.integers(0, 1 << int(rng.integers(4, 27)), size=k), rng.choice(special, 3)])]
        rng.shuffle(ns)
        cases.append(ns)
    for ns in cases:
        for passes in (0, 2, 7):
            segs, launches = capi.batch_layout(ns, passes=passes)
            check_layout(ns, segs, launches)
            assert passes == 0 or all(L["passes"] == passes for L in launches)
    # the same under a lowered launch limit (adsb_debug_config.batch_launch_offsets): tile multiples at K = 2, 7 and 32, with and
    # without forced passes -- honoured or not, by batch_launch_limit's rule.  Pieces and roll-overs in almost every case.
    t2, t7, t32 = (RUN * owned_runs(k) for k in (2, 7, 32))
    small = [v for v in special if v < 1 << 31]
    mixes = [[1 << 18] * 9 + [81960 + 8 * k for k in range(6)], [1 << 20] * 3 + [90_000] * 40]
    for _ in range(10):
        k = int(rng.integers(3, 40))
        ns = [int(v) for v in np.concatenate([rng.integers(0, 1 << int(rng.integers(18, 25)), size=k), rng.choice(small, 3)])]
        rng.shuffle(ns)
        mixes.append(ns)
    honoured = cut = rolled = 0
    for ns in mixes:
        for launch_offsets, passes in ((3 * t2, 2), (3 * t2, 0), (t2, 2), (2 * t7, 0), (2 * t7, 7), (t7, 0), (5 * t7 + 28, 2), (t32, 32),
                                       (t32, 0), (3 * t32, 7), (t7 - 28, 0), (MAX_LAUNCH + 28, 0)):
            limit = launch_limit(launch_offsets, passes)
            assert (limit == launch_offsets) == (launch_offsets not in (t7 - 28, MAX_LAUNCH + 28) and (launch_offsets, passes) != (3 * t2, 0))
            segs, launches = capi.batch_layout(ns, passes=passes, launch_offsets=launch_offsets)
            check_layout(ns, segs, launches, limit)
            assert passes == 0 or all(L["passes"] == passes for L in launches)
            if limit == MAX_LAUNCH:
                assert (segs, launches) == capi.batch_layout(ns, passes=passes)
                continue
            honoured += 1
            cut += len(segs) > len(ns)
            # a roll-over: a launch that ended because the next capture did not fit what was left of it, not on a cut
            rolled += any(segs[L["seg_first"]]["capture"] != segs[L["seg_first"] - 1]["capture"] for L in launches[1:])
    assert honoured == 9 * len(mixes) and 10 * cut >= 8 * honoured and 10 * rolled >= 8 * honoured, (honoured, cut, rolled)
    # nine buffers of 256 Mi samples are more than 2^30 offsets: two launches or more
    assert len(capi.batch_layout([1 << 28] * 9)[1]) >= 2
    # 256 captures of 1 Mi samples are one launch of seven passes, eleven tiles a capture (the quantisation loss: 1.3 %)
    segs, launches = capi.batch_layout([1 << 20] * 256)
    assert len(launches) == 1 and launches[0]["passes"] == 7 and {s["tiles"] for s in segs} == {11}
    # a batch has no long-stream mode
    assert capi.batch_layout([1 << 32]) is None and capi.batch_layout([5, (1 << 32) + 8, 5]) is None


def seeded_capture(i):
    from tools import gen_signal as G
    rng = np.random.default_rng(7000 + i)
    kind = i % 4
    n = int(rng.integers(90_000, 400_000)) + (i % 5)                    # lengths with n % 4 != 0 among them
    if i in (3, 11):
        return np.full([0, 3][i == 11], 2048, np.uint16)               # empty; three samples
    if i in (7, 15):                                                   # below one window; a window and more, but deqframe never fires
        return np.clip(np.rint(2048 + rng.normal(0, 30, [2391, 81956][i == 15])), 0, 4095).astype(np.uint16)
    if kind == 0:
        return G.sparse_capture(n, max(1, n // 6000), seed=7000 + i, sigma=8.0, dfs=(17, 18, 11))[0]
    if kind == 1:
        return G.dense_capture(n, seed=7000 + i, sigma=40.0, n_frames=max(1, n // 1400), amp=(200, 1800))[0]
    if kind == 2:
        return G.dense_capture(n, seed=7000 + i, sigma=200.0, n_frames=max(1, n // 6000))[0]
    starts = np.arange(3000, max(3001, n - 2600), 2400)
    return G.synth(n, [(int(s), G.make_frame((17, 18, 11)[k % 3], rng), float(rng.uniform(500, 1500)), 0.0)
                       for k, s in enumerate(starts)], 6.0, 7000 + i)


def _resolve_equals_the_oracle(capi, oracle, df18, launch_offsets):
    caps = [seeded_capture(i) for i in range(20)]
    ns = [int(x.size) for x in caps]
    segs, launches = capi.batch_layout(ns, launch_offsets=launch_offsets)
    check_layout(ns, segs, launches, launch_limit(launch_offsets, 0))
    cands, tries = [], []
    n_cut = 0
    for s in segs:
        n_cut += s["o_begin"] != 0
        x = caps[s["capture"]]
        if s["o_end"] == s["o_begin"]:
            continue
        c, t = oracle.scan_all(oracle.power(x), s["o_begin"], s["o_end"], df18)
        shift = s["base"] - s["o_begin"]
        cands += [(g + shift, pw, fr) for g, pw, fr in c]
        tries.append(t + np.uint64(shift << 2))
    if launch_offsets == 0:
        assert n_cut == 0                                              # (none of these is cut)
    else:                                                              # most are, and the launches are many: records on both sides of every cut
        assert n_cut >= 14 and len(launches) > n_cut and len({s["capture"] for s in segs if s["o_begin"]}) >= 12
    assert cands == sorted(cands, key=lambda c: c[0])
    tries = np.concatenate(tries) if tries else np.empty(0, np.uint64)
    assert np.all(np.diff(tries.astype(np.int64)) >= 0)
    frames, stats = capi.batch_resolve(ns, cands, tries, launch_offsets=launch_offsets)
    visited, with_frames = 0, 0
    for i, x in enumerate(caps):
        want, wstats = oracle.decode(x, df18=df18)
        assert records(frames[i]) == records(want), (i, ns[i])
        assert stats[i] == wstats, (i, ns[i])
        if offsets_of(ns[i]):
            visited += 1
            with_frames += bool(want)
    assert visited >= 15 and 4 * with_frames >= 3 * visited, (visited, with_frames)
    # a record that lies in no capture's offsets is an error, not a frame of the neighbour
    g_gap = segs[0]["base"] + segs[0]["o_end"] + 5
    bad = sorted(cands + [(g_gap, 1, bytes(14))], key=lambda c: c[0])
    with pytest.raises(capi.AdsbError):
        capi.batch_resolve(ns, bad, tries, launch_offsets=launch_offsets)
    return frames


@pytest.mark.parametrize("df18", [False, True])
def test_resolve_per_capture_equals_the_oracle(capi, oracle, df18):
    """Every CRC-valid candidate and every try of 20 seeded captures, shifted to the layout's virtual offsets, concatenated
    and sorted: per capture, frames (g, ts, pw, bytes) and Try/Ok table are oracle.decode's of that capture alone."""
    _resolve_equals_the_oracle(capi, oracle, df18, 0)


@pytest.mark.parametrize("df18", [False, True])
def test_resolve_of_cut_captures_equals_the_oracle(capi, oracle, df18):
    """The same through a layout whose launches hold one K = 7 tile (adsb_debug_config.batch_launch_offsets): the captures
    are cut into pieces and remainders, a launch each -- the oracle's real records on both sides of every cut, where
    test_resolve_rebases_records_on_both_sides_of_a_cut has hand-made ones.  Same frames, same tables."""
    _resolve_equals_the_oracle(capi, oracle, df18, RUN * owned_runs(7))


def test_resolve_rebases_records_on_both_sides_of_a_cut(capi):
    """A capture of more than 2^30 offsets is cut into segments, a launch each; the host half of that path without a device.
    Hand-made records (valid DF17 frames; a try word beside each) lie on the last offset of a piece, on the first of the next,
    around the second cut, and in a short capture before and behind the long one.  Shifted to the layout's virtual offsets they
    must come back per capture at their own offsets from 0, and frames, ts and Try/Ok must be those of ONE adsb::Resolver pass
    that is fed the same records unshifted: the code that has parity with the reference for an uncut capture."""
    from tools import gen_signal as G
    rng = np.random.default_rng(99)
    ns = [100_000, (1 << 32) - 4, 200_000]
    segs, launches = capi.batch_layout(ns)
    check_layout(ns, segs, launches)
    parts = [s for s in segs if s["capture"] == 1]
    assert len(parts) >= 3 and len(launches) >= 3 and [s["o_begin"] for s in parts][1:] == [s["o_end"] for s in parts][:-1]
    cut1, cut2 = parts[1]["o_begin"], parts[2]["o_begin"]
    own = {0: [5000, 20_000], 1: [7, cut1 - 5000, cut1 - 1, cut1, cut1 + 5000, cut2 - 5000, cut2, cut2 + 1, cut2 + 5000,
                                  offsets_of(ns[1]) - 1], 2: [0, 30_000]}
    recs = {i: [(g, 1000 + k, bytes(G.make_frame(17, rng))) for k, g in enumerate(gs)] for i, gs in own.items()}
    assert len({fr for v in recs.values() for _, _, fr in v}) == sum(map(len, own.values()))       # all frames differ
    def virtual(i, g):
        s = [s for s in segs if s["capture"] == i and s["o_begin"] <= g < s["o_end"]]
        assert len(s) == 1
        return s[0]["base"] + g - s[0]["o_begin"]
    cands = [(virtual(i, g), pw, fr) for i in sorted(recs) for g, pw, fr in recs[i]]
    assert cands == sorted(cands, key=lambda c: c[0])
    tries = np.array([(c[0] << 2) | 1 for c in cands], np.uint64)
    frames, stats = capi.batch_resolve(ns, cands, tries)
    for i in sorted(recs):
        r = capi.Resolver()
        try:
            r.feed(recs[i], np.array([(g << 2) | 1 for g, _, _ in recs[i]], np.uint64))
            r.advance(power_samples(ns[i]), offsets_of(ns[i]))
            want, wstats = r.drain(), r.stats()
        finally:
            r.close()
        assert records(frames[i]) == records(want) and stats[i] == wstats, i
        got = [f["g"] for f in frames[i]]
        assert set(got) <= set(own[i]) and got == sorted(got)
    # nothing lies within a frame's length in front of these: the greedy scan reaches and accepts them
    g1 = [f["g"] for f in frames[1]]
    assert {7, cut1 - 5000, cut1 - 1, cut1 + 5000, cut2 - 5000, cut2, cut2 + 5000} <= set(g1)
    assert [f["g"] for f in frames[0]] == own[0] and [f["g"] for f in frames[2]] == own[2]
    by_g = {f["g"]: f for f in frames[1]}
    assert bytes(by_g[cut2]["frame"]) == recs[1][6][2] and by_g[cut1 - 1]["pw"] == recs[1][2][1]


def test_batch_kernel_build(capi):
    """scan_batch_kernel.hip for gfx950, by the rules tests/test_build_flags.py holds scan_kernel.hip to: two kernels
    (statistics on / off), no scratch, at most 96 VGPRs (five waves per SIMD), and per kernel exactly the fused operations of
    scan_kernel -- the stages are the same text (scan_stages.h).  The sample pointer comes from memory here, and taking it
    from there must add no flat traffic: exactly the flat instructions of scan_kernel.hip's unit.  (Both units have some: the
    28-pair sample loads of the non-inlined pw_at go through a generic pointer in either.  What is asserted is "no more than
    scan_kernel", not "every sample load is global"; Stage A's typed loads go through a buffer resource in both.)"""
    from adsbdec_amd import _build
    assert "scan_batch_kernel.hip" in _build.HIP_SOURCES
    isa = {}
    for f in ("scan_batch_kernel.hip", "scan_kernel.hip"):
        cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, f), "-o", "-"]
        isa[f] = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    b = isa["scan_batch_kernel.hip"]
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in b
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", b, flags=re.M))
    assert len(sizes) == 2 and all("scan_batch_kernel" in k for k in sizes) and set(sizes.values()) == {"0"}, sizes
    vgprs = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", b)
    assert len(vgprs) == 2 and all(int(v) <= 96 for _, v in vgprs), vgprs
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)", b, flags=re.M)
    assert set(fused) == {"v_fma_f32", "v_pk_fma_f32"}
    assert fused.count("v_fma_f32") == 12 * 2 and fused.count("v_pk_fma_f32") == (22 + 184 + 24) * 2
    flat = lambda s: sorted(re.findall(r"^\s*(flat_\w+)", s, flags=re.M))
    assert flat(b) == flat(isa["scan_kernel.hip"])
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", b, flags=re.M)) == 17 * 2      # Stage A's typed loads, through a resource
    assert len(re.findall(r"^\s*s_load_dword", b, flags=re.M)) >= 4                       # the segment: scalar LOADS
    for f in ("scan_batch_kernel.hip", "scan_stages.h"):                                   # no build knob, as scan_kernel.hip
        src = open(os.path.join(_build.CSRC, f)).read()
        assert "#if" not in src, f
