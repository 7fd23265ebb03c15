"""The gate behind the envelope without a GPU: the numpy statement (adsbdec_amd/levels.py bursts, burst_samples) against the slow
paint-and-merge wording of the same definition, on thousands of small random cases and on the named cases the GPU test runs;
adsb_level_percentile against levels.percentile; the three calls are declared, exported and bound, the two new units are built, the
ABI version stays 5; the host program refuses -U where it cannot be meant, before any GPU call; and the pipeline fixture's condition
-- every planted frame is in the decode of some burst, the bursts cover less than burst_cases.COVER of the capture -- with the
frames per burst recorded for tests/test_gpu_bursts.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import burst_cases as BC
from conftest import ROOT

T_FOR_CPU = 2048   # (the statement knows no tile: any T gives valid cases; this is the kernels' own)


def LV():
    from adsbdec_amd import levels
    return levels


def agree(name, env, threshold, lead, hang):
    got = LV().bursts(env, threshold, lead, hang)
    assert got.dtype == LV().BURST_DTYPE
    assert BC.as_tuples(got) == BC.paint_and_merge(env, threshold, lead, hang), name
    return got


# ------------------------------------------------------------------ the statement
def test_statement_against_paint_and_merge_on_random_small_cases():
    rng = np.random.default_rng(3001)
    specials = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0, 1, 0x7F7FFFFF], dtype="<u4").view("<f4")
    thresholds = (0.0, 1.0e-40, 1.0, 2.5, float("inf"), 3.4028234663852886e38)
    for i in range(3000):
        R = int(rng.integers(0, 90))
        env = rng.uniform(0.0, 4.0, R).astype("<f4")
        env[rng.random(R) < 0.15] *= np.float32(-1.0)
        k = rng.random(R) < 0.1
        env[k] = rng.choice(specials, size=int(k.sum()))
        agree(i, env, float(rng.choice(thresholds)), int(rng.integers(0, 8)), int(rng.integers(0, 8)))


def test_statement_on_the_named_cases():
    T = 64                                                   # (paint-and-merge is slow: the same patterns around a smaller seam)
    for case in BC.named_cases(T) + [BC.alternating(T)]:
        name, env, threshold, lead, hang = case
        if lead > 10 * env.size:                             # (painting 2^30 runs per hot run: the clipped equivalent)
            assert np.array_equal(LV().bursts(env, threshold, lead, hang), LV().bursts(env, threshold, env.size, env.size)), name
            lead = hang = env.size
        got = agree(name, env, threshold, lead, hang)
        # ascending, at least one run apart, inside the envelope
        assert (got["begin"] < got["end"]).all() and (got["end"] <= env.size).all() and (got["end"][:-1] < got["begin"][1:]).all(), name
    name, env, threshold, lead, hang = BC.alternating(T)
    assert LV().bursts(env, threshold, lead, hang).size == (env.size + 1) // 2
    for t in BC.VALUE_THRESHOLDS:
        agree(t, BC.value_env(), t, 1, 2)
    every = LV().bursts(BC.value_env(), 0.0, 0, 0)
    assert every.size == 1 and every[0]["hot"] == BC.value_env().size and np.isnan(every[0]["peak"])   # +0.0: every run hot; NaN tops


def test_statement_refuses_what_the_call_refuses():
    env = np.ones(10, dtype="<f4")
    for bad in (dict(threshold=float("nan")), dict(threshold=-0.0), dict(threshold=-1.0), dict(lead=(1 << 30) + 1), dict(hang=(1 << 30) + 1),
                dict(lead=-1)):
        kw = dict(threshold=1.0, lead=1, hang=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            LV().bursts(env, **kw)
    with pytest.raises(ValueError):
        LV().bursts(env.astype(np.float64), 1.0, 1, 1)
    assert LV().bursts(np.zeros(0, "<f4"), 1.0, 1, 1).size == 0


def test_burst_samples():
    b = np.array([(0, 3, 1, 5.0), (5, 10, 2, 7.0)], dtype=LV().BURST_DTYPE)
    assert LV().burst_samples(b, 270).tolist() == [[0, 84], [140, 270]]
    assert LV().burst_samples(b, 280).tolist() == [[0, 84], [140, 280]]
    assert LV().burst_samples(b[:0], 280).shape == (0, 2)
    big = np.array([((1 << 31) - 10, (1 << 31) - 1, 1, 1.0)], dtype=LV().BURST_DTYPE)
    assert LV().burst_samples(big, 1 << 40).tolist() == [[28 * ((1 << 31) - 10), 28 * ((1 << 31) - 1)]]   # (no 32-bit product)


# ------------------------------------------------------------------ adsb_level_percentile
def test_level_percentile_is_the_statements(capi):
    L = capi.load()
    rng = np.random.default_rng(3002)
    qs = (0.0, 1.0e-9, 0.25, 0.5, 0.999, 1.0)

    def same(hist, q):
        got, want = np.float32(capi.level_percentile(hist, q)), np.float32(LV().percentile(hist, q))
        assert got.view(np.uint32) == want.view(np.uint32), (np.flatnonzero(hist)[:4], q, got, want)
    for k in range(2048):                                    # every single-bin histogram: the bin's lower edge (NaN from 2041 on)
        hist = np.zeros(2048, np.uint64)
        hist[k] = 1 + k % 3
        same(hist, qs[k % len(qs)])
    for _ in range(200):
        hist = np.zeros(2048, np.uint64)
        where = rng.choice(2040, size=int(rng.integers(1, 60)), replace=False)
        hist[where] = rng.integers(1, 1 << int(rng.integers(1, 40)), size=where.size).astype(np.uint64)
        for q in qs + (float(rng.random()),):
            same(hist, q)
    one = np.zeros(2048, np.uint64)
    one[1016] = 5
    assert capi.level_percentile(one, 0.5) == 1.0
    for q in (-0.001, 1.001, float("nan"), float("inf")):    # the refusals: -1
        assert capi.level_percentile(one, q) == -1.0
    assert capi.level_percentile(np.zeros(2048, np.uint64), 0.5) == -1.0
    assert L.adsb_level_percentile(None, 0.5) == -1.0


# ------------------------------------------------------------------ interface and build
def test_entry_points_are_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    text = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    main = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adsbdec_amd_diag.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name, res, n_args in (("adsb_bursts_device", "long", 8), ("adsb_bursts_host", "long", 8), ("adsb_level_percentile", "float", 2)):
        assert re.search(rf"\b{res}\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == n_args and capi.SYMBOLS[name][0] is (C.c_long if res == "long" else C.c_float), name
    assert re.search(r"\buint32_t\s+adsb_burst_tile_runs\s*\(\s*void\s*\)", diag) and "adsb_burst_tile_runs" in exported
    assert "typedef struct adsb_burst { uint32_t begin, end, hot; float peak; } adsb_burst;" in main
    assert LV().BURST_DTYPE.itemsize == 16 and [LV().BURST_DTYPE.fields[k][1] for k in ("begin", "end", "hot", "peak")] == [0, 4, 8, 12]
    for m in ("bursts_device", "bursts_host", "bursts"):
        assert callable(getattr(capi.Decoder, m)), m
    assert callable(capi.level_percentile)
    T = capi.burst_tile_runs()
    assert T >= 256 and T % 256 == 0
    assert "burst_kernel.hip" in _build.HIP_SOURCES and "decoder_bursts.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "burst_kernel.hip.o" in mk and "decoder_bursts.hip.o" in mk
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main
    assert len(text.splitlines()) <= 250
    # NULL handle: -1, nothing touched
    tab = np.full(4 * 16, 0x5A, dtype=np.uint8)
    assert L.adsb_bursts_device(None, None, 0, 1.0, 0, 0, tab.ctypes.data, 4) == -1
    assert L.adsb_bursts_host(None, None, 0, 1.0, 0, 0, tab.ctypes.data, 4) == -1
    assert (tab == 0x5A).all()


def test_the_gate_has_three_kernels_without_scratch():
    """gfx950 only; three kernels, none with scratch; hot and peak are vector atomics that return nothing, and no kernel of the unit
    reads a flag in a loop: the only loads of the emit and summary kernels are of the envelope and of their own rows."""
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "burst_kernel.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True,
                         check=True).stdout
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 3 and all(int(v) == 0 for v in sizes.values()), sizes
    for k in ("burst_summary_kernel", "burst_combine_kernel", "burst_emit_kernel"):
        assert any(k in name for name in sizes), (k, sorted(sizes))
    assert re.search(r"^\s*global_atomic_add\s", isa, flags=re.M) and re.search(r"^\s*global_atomic_umax\s", isa, flags=re.M)
    assert not re.search(r"^\s*(global|flat)_atomic_\w+\s.*\bsc0\b", isa, flags=re.M)        # (none returns a value)
    assert not re.search(r"^\s*flat_(load|store|atomic)", isa, flags=re.M)
    assert re.search(r"^\s*global_load_dwordx4", isa, flags=re.M)                              # 16 bytes per lane
    assert not re.search(r"^\s*s_sleep", isa, flags=re.M)                                      # nothing waits


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_gate_refusals_and_usage(capi, tmp_path):
    """-U without -L, with -I, -B, -G or -W, or with a factor that is no finite number above 0 (or a lead / hang that is no whole number
    up to 2^30): exit 1 with a message before any GPU call (the file does not even exist, and nothing is created)."""
    capi.load()
    p = _cli(capi, tmp_path, "-U", "8", "-f", "nothing.bin")
    assert p.returncode == 1 and "-U is not supported without -L" in p.stderr and not p.stdout, p.stderr
    p = _cli(capi, tmp_path, "-L", "-I", "1", "-U", "8", "-f", "nothing.bin")
    assert p.returncode == 1 and "-U is not supported with -I: " in p.stderr and not p.stdout, p.stderr
    for extra, word in ((["-G", "2"], "-G"), (["-B", "list.txt"], "-B"), (["-W", "out.pw"], "-W")):
        p = _cli(capi, tmp_path, "-L", "-U", "8", *extra, "-f", "nothing.bin")          # (-L's own refusal stands in front)
        assert p.returncode == 1 and "is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
        p = _cli(capi, tmp_path, "-U", "8", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and "-U is not supported" in p.stderr and not p.stdout, (extra, p.stderr)
    for bad in ("0", "-1", "abc", "nan", "inf", "1e999", "", "8,", "8,x", "8,-1", "8,1.5", "8,1,", "8,1,2,3", "8,1073741825", "8,1,1073741825"):
        p = _cli(capi, tmp_path, "-L", "-U", bad, "-f", "nothing.bin")
        assert p.returncode == 1 and "a finite factor above 0" in p.stderr and not p.stdout, (bad, p.stderr)
    assert not os.listdir(tmp_path)
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "-L -U factor[,lead[,hang]] -f filename" in u.stdout and "\t-U factor[,lead[,hang]] :" in u.stdout
    assert "-L -I ms -f filename" in u.stdout and "\t-L :" in u.stdout                   # (what the level tests pin stays)
    # a well-formed -U gets as far as the file
    p = _cli(capi, tmp_path, "-L", "-U", "8,0,1073741824", "-f", "nothing.bin")
    assert p.returncode == 255 and "nothing.bin" in p.stderr


# ------------------------------------------------------------------ the pipeline fixture's condition
def test_pipeline_fixture_keeps_every_planted_frame(oracle):
    p = BC.pipeline()
    M = p["a"].size
    assert M == BC.PIPE_N and len(p["truth"]) == BC.PIPE_FRAMES
    assert {len(f) for _, f in p["truth"]} == {7, 14}                                    # short and long
    b, slices = p["bursts"], p["slices"]
    assert 1 <= b.size <= BC.PIPE_FRAMES
    per = BC.frames_per_burst(oracle)
    assert len(per) == b.size
    found = {f[3] for frames in per for f in frames}
    lost = [(s, f.hex()) for s, f in p["truth"] if f not in found]
    assert not lost, lost
    # every frame lies inside the burst that decodes it, and a burst decodes nothing but planted frames
    planted = {f: s for s, f in p["truth"]}
    for (lo, hi), frames in zip(slices, per):
        assert frames, (lo, hi)
        for g, ts, pw, f in frames:
            assert f in planted and lo <= planted[f] < hi and abs(lo + g - planted[f]) <= 2
    cover = int((slices[:, 1] - slices[:, 0]).sum()) / M
    assert cover < BC.COVER, cover
    assert (slices[:, 0] % 28 == 0).all() and (slices[:-1, 1] < slices[1:, 0]).all()
    # with the hang first meant (4 runs) nothing at all decodes: why the default is 1468
    short = LV().burst_samples(LV().bursts(p["env"], p["threshold"], 2, 4), M)
    assert not any(oracle.demod_power(np.ascontiguousarray(p["a"][lo:hi]), df18=True)[0] for lo, hi in short)
