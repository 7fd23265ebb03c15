"""The level report without a GPU: the adsb_level_* calls are declared, exported and bound; the gfx950 code of level_kernel.hip has
no scratch and carries Stage A's loads and the FIR's own fused operations once; adsbdec_amd.levels.level_report -- the numpy
statement the GPU tests hold the kernels to -- puts the landmark values in the bins the header names, obeys the sum rule, gives the
float maximum as envelope on every committed fixture, is safe with NaN and negative samples, and agrees with
sample_formats.power_domain_ok; percentile; the C host program's -L refuses what it cannot combine with before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_cases, load_golden

ENTRY_POINTS = ("adsb_level_device", "adsb_level_device_as", "adsb_level_device_packed", "adsb_level_device_iq", "adsb_level_device_power",
                "adsb_level_host")


def LV():
    from adsbdec_amd import levels
    return levels


def SF():
    from adsbdec_amd import sample_formats
    return sample_formats


def f32(*vals):
    return np.array(vals, dtype=np.float32)


def from_bits(*words):
    return np.array(words, dtype="<u4").view("<f4")


def test_entry_points_are_declared_exported_and_bound(capi):
    import ctypes as C
    from adsbdec_amd import _build
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
    for m in ("level_device", "level_device_as", "level_device_packed", "level_device_iq", "level_device_power", "level"):
        assert callable(getattr(capi.Decoder, m)), m
    assert "typedef struct adsb_level_report { uint64_t samples, negative, rail_lo, rail_hi, over; uint64_t hist[2048]; } adsb_level_report;" in main
    assert C.sizeof(capi.LevelReport) == 8 * (5 + 2048) and capi.LevelReport.hist.offset == 40
    assert "level_kernel.hip" in _build.HIP_SOURCES and "decoder_level.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "level_kernel.hip.o" in mk and "decoder_level.hip.o" in mk
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main


@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "level_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


FUSED = r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)"


def test_isa_of_the_level_unit(isa):
    """gfx950 only; no kernel of the unit has scratch; the FIR is there once, with Stage A's 17 typed loads in front of it and the
    fused operations tests/test_power_export_cpu.py pins for the export's copy (184 products and 24 accumulations, nothing else
    fused: the IQ kernels' squares and sums stay separate); the histogram is LDS adds that return nothing, and the 64-bit totals
    take vector atomics."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert sum("level_units_kernel" in k for k in sizes) == 3 and any(re.search(r"\d+level_kernel", k) for k in sizes), sorted(sizes)
    for name, size in sizes.items():
        assert int(size) == 0, f"{name} spills to scratch"
    fused = re.findall(FUSED, isa, flags=re.M)
    assert set(fused) <= {"v_pk_fma_f32"}, f"contracted arithmetic in the ISA: {sorted(set(fused))}"
    assert len(re.findall(r"^\s*v_pk_fma_f32", isa, flags=re.M)) == 184 + 24
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", isa, flags=re.M)) == 17
    assert re.search(r"^\s*ds_add_u32", isa, flags=re.M) and not re.search(r"^\s*ds_add_rtn", isa, flags=re.M)
    assert re.search(r"^\s*global_atomic_add_x2", isa, flags=re.M)
    lds = [int(v) for v in re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", isa, flags=re.M)]
    assert max(lds) <= 4 * 8192 + 64                                      # at most a histogram per wave: 5 workgroups a CU


# ------------------------------------------------------------------ the definition
def test_landmark_bins():
    """0.0 -> bin 0, the smallest subnormal -> 0, the largest -> 7, 1.0 -> 1016, 2^29 -> 1248 and the float below it -> 1247, Inf -> 2040,
    NaNs above it; the constants of the module say the same."""
    L = LV()
    top = from_bits(0x4E000000 - 1)[0]
    a = np.concatenate([f32(0.0, 1.0, 2.0 ** 29, np.inf), from_bits(0x00000001, 0x007FFFFF, 0x7FC00000, 0x7F800001, 0x7FFFFFFF), [top]]).astype("<f4")
    r = L.level_report(a)
    want = {0: 2, 7: 1, 1016: 1, 1247: 1, 1248: 1, 2040: 2, 2044: 1, 2047: 1}
    assert {int(k): int(v) for k, v in enumerate(r["hist"]) if v} == want
    assert (L.BIN_ONE, L.BIN_DOMAIN_END, L.BIN_NONFINITE, L.BINS, L.RUN) == (1016, 1248, 2040, 2048, 28)
    assert r["hist"].dtype == np.uint64 and r["hist"].shape == (2048,) and r["samples"] == a.size and r["negative"] == 0
    assert L.bin_lower_edge(1016) == 1.0 and L.bin_lower_edge(1248) == 2.0 ** 29 and L.bin_lower_edge(1024) == 2.0 and L.bin_lower_edge(0) == 0.0
    assert abs(10 * np.log10(L.bin_lower_edge(1017) / L.bin_lower_edge(1016)) - 0.51) < 0.01     # the widest bin of an octave
    assert abs(10 * np.log10(L.bin_lower_edge(1024) / L.bin_lower_edge(1016)) - 3.0103) < 1e-3   # eight bins: an octave
    with pytest.raises(ValueError):
        L.level_report(np.zeros(4, np.float64))


def test_sum_rule_and_negatives():
    """hist.sum() + negative == samples on random bit patterns; -0.0 counts as negative and sits in no bin."""
    L = LV()
    b = np.random.default_rng(23).integers(0, 1 << 32, 100_003, dtype=np.uint64).astype("<u4")
    r = L.level_report(b.view("<f4"))
    assert int(r["hist"].sum()) + r["negative"] == r["samples"] == b.size
    assert r["negative"] == int((b >> 31).sum()) and 0 < r["negative"] < b.size
    z = L.level_report(f32(-0.0, 0.0, -1.0))
    assert z["negative"] == 2 and int(z["hist"][0]) == 1 and int(z["hist"].sum()) == 1
    assert z["env"].view("<u4").tolist() == [0]
    e = L.level_report(np.zeros(0, np.float32))
    assert e["samples"] == 0 and e["env"].size == 0 and not e["hist"].any()


@pytest.mark.parametrize("name", golden_cases())
def test_env_is_the_float_maximum_on_the_fixtures(oracle, name):
    L = LV()
    x, rec = load_golden(name)
    a = oracle.power(x)[: 2 * (x.size // 4)]
    r = L.level_report(a)
    m = a.size
    runs = -(-m // 28)
    assert r["env"].dtype == np.float32 and r["env"].size == runs
    pad = np.zeros(runs * 28, np.float32)
    pad[:m] = a
    assert np.array_equal(r["env"].view("<u4"), pad.reshape(runs, 28).max(axis=1).view("<u4"))
    assert SF().power_domain_ok(a) and L.domain_ok(r)
    assert int(r["hist"].sum()) == m and r["negative"] == 0


def test_env_with_nan_and_negative_samples_planted():
    """A NaN wins its run (its bit pattern is the largest sign-clear word), a NaN with the sign bit set and a negative count for
    nothing, a run of negatives only has envelope +0 -- whatever the order inside the run."""
    L = LV()
    rng = np.random.default_rng(5)
    a = rng.uniform(1.0, 1000.0, 28 * 5 + 3).astype("<f4")
    b = a.view("<u4").copy()
    b[3] = 0x7FC00001                       # run 0: a quiet NaN
    b[28 + 4] = 0xFFC00000                  # run 1: a NaN with the sign set
    b[28 + 9] = np.float32(-5e6).view("<u4")
    b[56: 84] |= 0x80000000                 # run 2: every sample negative
    b[84 + 27] = 0x7F800000                 # run 3: +Inf
    want = []
    for r in range(6):
        w = b[28 * r: 28 * r + 28]
        want.append(int(np.where(w >> 31, 0, w).max()))
    got = L.level_report(b.view("<f4"))
    assert got["env"].view("<u4").tolist() == want
    assert want[0] == 0x7FC00001 and want[2] == 0 and want[3] == 0x7F800000 and got["env"].size == 6
    assert got["negative"] == 30
    perm = np.concatenate([rng.permutation(28) + 28 * r for r in range(5)] + [np.arange(140, 143)])
    again = L.level_report(b[perm].view("<f4"))
    assert again["env"].view("<u4").tolist() == want and np.array_equal(again["hist"], got["hist"])


def test_equivalence_with_power_domain_ok():
    """power_domain_ok(a) <=> negative == 0 and hist[1248:].sum() == 0, on an array inside the domain and on arrays that break each
    clause in turn."""
    L, S = LV(), SF()
    base = np.random.default_rng(9).uniform(0.0, 2.0 ** 28, 4099).astype("<f4")
    base[:4] = from_bits(0, 1, 0x007FFFFF, 0x4E000000 - 1)              # +0, subnormals, the largest value below 2^29
    assert S.power_domain_ok(base) and L.domain_ok(L.level_report(base))
    breakers = {"negative": f32(-1.0), "-0.0": f32(-0.0), "2^29": f32(2.0 ** 29), "large": f32(3e38), "+Inf": f32(np.inf), "-Inf": f32(-np.inf),
                "NaN": from_bits(0x7FC00000), "-NaN": from_bits(0xFFC00000)}
    for how, v in breakers.items():
        a = base.copy()
        a[1234] = v[0]
        r = L.level_report(a)
        by_report = r["negative"] == 0 and int(r["hist"][1248:].sum()) == 0
        assert S.power_domain_ok(a) is False and by_report is False and L.domain_ok(r) is False, how
        assert (r["negative"] == 1) != (int(r["hist"][1248:].sum()) == 1), how                 # exactly one clause each


def test_percentile():
    L = LV()
    h = np.zeros(2048, np.uint64)
    h[1016], h[1024], h[1100] = 50, 49, 1
    assert L.percentile(h, 0.0) == 1.0 and L.percentile(h, 0.5) == 1.0 and L.percentile(h, 0.51) == 2.0
    assert L.percentile(h, 0.99) == 2.0 and L.percentile(h, 0.999) == L.bin_lower_edge(1100) == L.percentile(h, 1.0)
    a = np.random.default_rng(4).uniform(0.5, 4096.0, 20_001).astype("<f4")
    r = L.level_report(a)
    for q in (0.1, 0.5, 0.9, 0.999):
        exact = np.sort(a)[int(np.ceil(q * a.size)) - 1]
        edge = L.percentile(r["hist"], q)
        assert edge <= exact < edge * (1 + 1 / 8) + 1e-3, q             # the bin that holds the q-quantile
    with pytest.raises(ValueError):
        L.percentile(np.zeros(2048, np.uint64), 0.5)
    with pytest.raises(ValueError):
        L.percentile(h, 1.5)


def test_rails_of_the_input_codes():
    L = LV()
    x = np.array([0, 4095, 4096, 65535, 2048, 0, 0, 4095, 0, 4097], dtype=np.uint16)   # (the last two, n % 4, count too)
    assert L.rails(x, "real") == (4, 2, 3)
    assert L.rails(x[:3], "real") == (0, 0, 0)                                          # (no power sample: an all-zero report)
    assert L.rails(np.array([[-32768, 32767], [0, -32768]], np.int16), "iq16") == (2, 1, 0)
    assert L.rails(np.array([[-128, 127], [127, 5]], np.int8), "iq8") == (1, 2, 0)


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_level_refusals_and_usage(capi, tmp_path):
    """-L with -G, -B, -W, -s, -l or several -f: exit 1 with both names before any GPU call (the files do not even exist, and nothing
    is created); the usage text names -L."""
    capi.load()
    for extra, word in ((["-G", "2"], "-G"), (["-W", "out.pw"], "-W"), (["-s", "127.0.0.1:9"], "-s"), (["-l", "127.0.0.1:9"], "-l"),
                        (["-f", "other.bin"], "several -f")):
        p = _cli(capi, tmp_path, "-L", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and "-L is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
    p = _cli(capi, tmp_path, "-L", "-B", "list.txt")
    assert p.returncode == 1 and "-L is not supported with -B: " in p.stderr and not p.stdout
    assert not os.listdir(tmp_path)
    p = _cli(capi, tmp_path, "-L")                                       # no input: the usage text
    assert p.returncode == 1 and "usage" in p.stdout
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "-L -f filename" in u.stdout and "\t-L :" in u.stdout and "invalid option" in u.stderr
    assert "dBFS" not in u.stdout
