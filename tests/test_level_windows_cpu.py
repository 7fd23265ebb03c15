"""The window form of the level report without a GPU: adsb_level_windows, adsb_level_windows_host and adsb_level_add are declared,
exported and bound; the numpy statement (adsbdec_amd/levels.py level_windows, add) is the level report of the slices, and the
reports of any partition add up to the one-window report; the table the host side builds, the row search and the per-wave
accumulate-and-flush hold on the CPU, under the sanitizers, in a program of their own; the gfx950 code of
level_windows_kernel.hip has one kernel, no scratch, the FIR once and Stage A's 17 typed loads; the host program refuses -I
where it cannot be meant, before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FUSED = r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)"
COUNTERS = ("samples", "negative", "rail_lo", "rail_hi", "over")


def LV():
    from adsbdec_amd import levels
    return levels


def same(r, s):
    return all(int(r[k]) == int(s[k]) for k in COUNTERS) and np.array_equal(np.asarray(r["hist"], np.uint64), np.asarray(s["hist"], np.uint64))


# ------------------------------------------------------------------ interface and build
def test_entry_points_are_declared_exported_and_bound(capi):
    import ctypes as C
    from adsbdec_amd import _build
    text = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    main = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name, res, n_args in (("adsb_level_windows", "long", 9), ("adsb_level_windows_host", "long", 9), ("adsb_level_add", "void", 2)):
        assert re.search(rf"\b{res}\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == n_args and capi.SYMBOLS[name][0] is (C.c_long if res == "long" else None), name
    assert callable(capi.Decoder.level_windows) and callable(capi.Decoder.level_windows_host) and callable(capi.level_add)
    # the header keeps its size and both pinned sentences, and says where one window differs from the single call
    assert len(text.splitlines()) <= 250
    assert "adsb_level_batch_*: a BATCH of captures" in text and "No multi-GPU or stream-window form" in text
    assert "adsb_level_windows: ONE stream" in text and "trailing n % 4 codes belong to no window" in text
    # symbols are added, no struct changes
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main
    assert C.sizeof(capi.LevelReport) == 8 * (5 + 2048)
    assert "level_windows_kernel.hip" in _build.HIP_SOURCES and "decoder_level_windows.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "level_windows_kernel.hip.o" in mk and "decoder_level_windows.hip.o" in mk
    # NULL handle: -1, nothing touched
    e = (C.c_uint64 * 2)(0, 0)
    r = capi.LevelReport()
    assert L.adsb_level_windows(None, None, 0, 0, 1, e, C.byref(r), None, 0) == -1
    assert L.adsb_level_windows_host(None, None, 0, 0, 1, e, C.byref(r), None, 0) == -1
    L.adsb_level_add(None, C.byref(r))
    L.adsb_level_add(C.byref(r), None)
    assert r.samples == 0


# ------------------------------------------------------------------ the numpy statement
def stream(rng, n):
    """uint16 codes with rail codes sprinkled in, and float32 "power samples" of any bit pattern that is not negative, plus a few
    that are: level_windows takes `a` as given, so the statement is checked on more than a front end can produce."""
    x = rng.integers(1, 4095, size=n, dtype=np.uint16)
    x[rng.integers(0, n, size=n // 50)] = 0
    x[rng.integers(0, n, size=n // 60)] = 4095
    x[rng.integers(0, n, size=n // 70)] = rng.integers(4096, 65536, size=n // 70)
    m = 2 * (n // 4)
    a = (rng.integers(0, 1 << 31, size=m, dtype=np.int64).astype(np.uint32) >> rng.integers(0, 12, size=m).astype(np.uint32)).view(np.float32)
    neg = rng.integers(0, m, size=m // 40)
    a[neg] = -np.abs(a[neg])
    return x, a


def partition(rng, lo, hi, k):
    """k windows over [lo, hi): inner edges multiples of 28, some of them equal (empty windows)"""
    inner = 28 * np.sort(rng.integers(-(-lo // 28), hi // 28 + 1, size=k - 1))
    return [lo] + [int(v) for v in inner] + [hi]


def test_level_windows_is_the_level_report_of_the_slices():
    L, rng = LV(), np.random.default_rng(2701)
    x, a = stream(rng, 20002)
    for edges in ([0, a.size], [28, 56, 84], [280, 280, 2072, 2072, 2100, 9999], partition(rng, 56, a.size - 5, 40)):
        reports, env = L.level_windows(a, x, edges)
        assert len(reports) == len(edges) - 1
        for lo, hi, r in zip(edges, edges[1:], reports):
            want = L.level_report(a[lo:hi])
            own = x[2 * lo:2 * hi]
            want["rail_lo"], want["rail_hi"], want["over"] = int((own == 0).sum()), int((own == 4095).sum()), int((own > 4095).sum())
            assert same(r, want) and "env" not in r and r["samples"] == hi - lo
            if lo == hi:
                assert same(r, L.zero_report())
        want_env = L.level_report(a[edges[0]:edges[-1]])["env"]
        assert env.dtype == np.float32 and env.size == -(-(edges[-1] - edges[0]) // 28)
        assert np.array_equal(env.view(np.uint32), want_env.view(np.uint32))
        # one envelope serves all windows: a window's own envelope is its stretch of it
        for lo, hi in zip(edges, edges[1:]):
            own = L.level_report(a[lo:hi])["env"]
            at = (lo - edges[0]) // 28
            assert np.array_equal(own.view(np.uint32), env[at:at + own.size].view(np.uint32))
    for bad in ([0, 27, 56], [56, 28], [], [0, a.size + 1]):
        with pytest.raises(ValueError):
            L.level_windows(a, x, bad)


def test_add_is_associative_with_the_zero_report_as_identity(capi):
    L, rng = LV(), np.random.default_rng(2702)
    capi.load()

    def random_report():
        r = {k: int(rng.integers(0, 1 << 40)) for k in COUNTERS}
        r["hist"] = rng.integers(0, 1 << 40, size=2048, dtype=np.uint64)
        return r
    for _ in range(8):
        r, s, t = random_report(), random_report(), random_report()
        assert same(L.add(L.add(r, s), t), L.add(r, L.add(s, t)))
        assert same(L.add(r, s), L.add(s, r))
        assert same(L.add(r, L.zero_report()), r) and same(L.add(L.zero_report(), r), r)
        assert "env" not in L.add(r, s)
        # adsb_level_add is that sum
        assert same(capi.level_add(r, s), L.add(r, s))
        assert same(capi.level_add(r, L.zero_report()), r)
    assert L.add(r, s)["hist"].dtype == np.uint64


def test_the_reports_of_a_partition_add_up():
    L, rng = LV(), np.random.default_rng(2703)
    for n in (20000, 20002, 20003):
        x, a = stream(rng, n)
        whole, env = L.level_windows(a, x, [0, a.size])
        for k in (2, 7, 300):
            reports, env_k = L.level_windows(a, x, partition(rng, 0, a.size, k))
            total = L.zero_report()
            for r in reports:
                total = L.add(total, r)
            assert same(total, whole[0]), (n, k)
            assert np.array_equal(env_k.view(np.uint32), env.view(np.uint32))
        # one window over a whole capture against the single call's report: equal when no code trails, else short of exactly them
        single = L.with_rails(L.level_report(a), x, "real")
        if n % 4 == 0:
            assert same(whole[0], single)
        else:
            trail = x[4 * (n // 4):]
            assert trail.size == n % 4
            for key, hit in (("rail_lo", trail == 0), ("rail_hi", trail == 4095), ("over", trail > 4095)):
                assert whole[0][key] == single[key] - int(hit.sum())
            assert np.array_equal(whole[0]["hist"], single["hist"]) and whole[0]["samples"] == single["samples"]
        assert np.array_equal(env.view(np.uint32), L.level_report(a)["env"].view(np.uint32))


# ------------------------------------------------------------------ the table
def test_table_rows_ranges_and_flush_under_the_sanitizers(tmp_path):
    """csrc/level_windows.hpp compiled for the host with -fsanitize=address,undefined, a program of its own
    (tests/cpp/level_windows_rows.cpp): seeded edge lists with empty windows and windows of 28, up to 1100 windows; every pass
    belongs to exactly one window, rows are found from any starting row, the waves' ranges cover every pass once, the per-wave
    accumulate-and-flush leaves what a direct count leaves and writes every float of the shared envelope once."""
    exe = tmp_path / "level_windows_rows"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "level_windows_rows.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 63 lists"), p.stdout + p.stderr


# ------------------------------------------------------------------ the ISA of the new unit
@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "level_windows_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def test_isa_of_the_windows_unit(isa):
    """What tests/test_level_batch_cpu.py asks of the batch unit, asked of this one: gfx950 only; ONE kernel, no scratch; the FIR once
    (184 products and 24 accumulations, nothing else fused -- a 64-bit division in the kernel would show here as v_fmamk_f32) behind
    Stage A's 17 typed loads; the histogram is LDS adds that return nothing, a histogram per wave and 16 bytes beside it; the 64-bit
    totals take vector atomics; ONE workgroup barrier (the waves meet at their end, never per pass); the row of a pass is found by
    scalar loads from the table."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and "level_windows_kernel" in next(iter(sizes)), sorted(sizes)
    assert all(int(v) == 0 for v in sizes.values()), "the kernel spills to scratch"
    fused = re.findall(FUSED, isa, flags=re.M)
    assert set(fused) <= {"v_pk_fma_f32"}, f"contracted arithmetic in the ISA: {sorted(set(fused))}"
    assert len(re.findall(r"^\s*v_pk_fma_f32", isa, flags=re.M)) == 184 + 24
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", isa, flags=re.M)) == 17
    assert re.search(r"^\s*ds_add_u32", isa, flags=re.M) and not re.search(r"^\s*ds_add_rtn", isa, flags=re.M)
    assert re.search(r"^\s*global_atomic_add_x2", isa, flags=re.M) and not re.search(r"^\s*flat_atomic", isa, flags=re.M)
    assert len(re.findall(r"^\s*s_barrier", isa, flags=re.M)) == 1
    lds = [int(v) for v in re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", isa, flags=re.M)]
    assert lds == [4 * 8192 + 16]                                            # a histogram per wave: 5 workgroups a CU
    table_loads = [b for b in re.findall(r"^\s*s_load_dword(?:x\d+)?\s+s\[?[\d:]+\]?,\s*(s\[\d+:\d+\])", isa, flags=re.M) if b != "s[0:1]"]
    assert len(table_loads) >= 1, table_loads


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_interval_refusals_and_usage(capi, tmp_path):
    """-I without -L, with -t, -p, -q or -w, or with a length that is no number above 0: exit 1 with a message before any GPU call (the
    file does not even exist, and nothing is created); the usage text names -I."""
    capi.load()
    p = _cli(capi, tmp_path, "-I", "1", "-f", "nothing.bin")
    assert p.returncode == 1 and "-I is not supported without -L" in p.stderr and not p.stdout, p.stderr
    for extra, word in ((["-t", "3"], "-t"), (["-p"], "-p"), (["-q", "2"], "-q"), (["-w"], "-w")):
        p = _cli(capi, tmp_path, "-L", "-I", "1", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and "-I is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
    for bad in ("0", "-1", "abc", "1ms", "nan", ""):
        p = _cli(capi, tmp_path, "-L", "-I", bad, "-f", "nothing.bin")
        assert p.returncode == 1 and "a number above 0" in p.stderr and not p.stdout, (bad, p.stderr)
    p = _cli(capi, tmp_path, "-L", "-I", "1", "-G", "2", "-f", "nothing.bin")      # -L's own refusals stay in front
    assert p.returncode == 1 and "-L is not supported with -G: " in p.stderr and not p.stdout
    assert not os.listdir(tmp_path)
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "-L -I ms -f filename" in u.stdout and "\t-I ms :" in u.stdout
    assert "-L -f filename" in u.stdout and "\t-L :" in u.stdout                   # (what tests/test_level_cpu.py pins stays)
