"""Signed 16-bit real and float32 real input without a GPU: the two sample functions the conversion kernels run
(csrc/sample_format.h, compiled for the host by tests/cpp/sample_formats.cpp) against the formats' definitions and against the
numpy definition (adsbdec_amd/sample_formats.py), the C-ABI's new entry points, adsb_format_bytes, and the C host program's -t."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ENTRY_POINTS = ("adsb_format_bytes", "adsb_push_as", "adsb_push_async_as", "adsb_push_device_as", "adsb_push_device_final_as",
                "adsb_decode_device_as", "adsb_decode_batch_device_as", "adsb_decode_batch_host_as", "adsb_get_format_report",
                "adsb_convert_samples")
EXACT, INEXACT, CLAMPED = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sample_formats") / "sample_formats"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "sample_formats.cpp"), "-o", str(out)],
                   check=True)
    return str(out)


def header(exe, fmt, x, tmp_path):
    """(codes, what) of the header's function for every sample of x."""
    x.tofile(tmp_path / "in.bin")
    subprocess.run([exe, str(fmt), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    r = np.fromfile(tmp_path / "out.bin", dtype=np.uint16).reshape(-1, 2)
    assert r.shape[0] == x.size
    return r[:, 0], r[:, 1]


def numpy_what(fmt, x):
    from adsbdec_amd import sample_formats as S
    if fmt == S.INT16_REAL:
        codes, inexact = S.flags_int16_real(x)
        return codes, inexact.astype(np.uint16) * INEXACT
    codes, inexact, clamped = S.flags_float32_real(x)
    assert not (inexact & clamped).any()                    # counted at most once
    return codes, inexact.astype(np.uint16) * INEXACT + clamped.astype(np.uint16) * CLAMPED


def test_header_against_the_definition_on_the_host(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "65536 int16 values, 4096 codes in both formats" in p.stdout


def test_every_int16_value(exe, tmp_path):
    from adsbdec_amd import sample_formats as S
    x = np.arange(-32768, 32768, dtype=np.int32).astype("<i2")
    codes, what = header(exe, S.INT16_REAL, x, tmp_path)
    want = [((int(v) >> 4) + 2048, int((int(v) & 15) != 0)) for v in x]        # the definition, in Python integers
    assert list(zip(codes.tolist(), what.tolist())) == want
    ncodes, nwhat = numpy_what(S.INT16_REAL, x)
    assert np.array_equal(ncodes, codes) and np.array_equal(nwhat, what)
    assert codes.min() == 0 and codes.max() == 4095
    assert S.from_int16_real(x)[1:] == (65536 - 4096, 0)


@pytest.mark.parametrize("fmt", [1, 3])
def test_every_code_round_trips(exe, tmp_path, fmt):
    from adsbdec_amd import sample_formats as S
    c = np.arange(4096, dtype=np.uint16)
    x = S.to_format(fmt, c)
    assert x.dtype == S.DTYPES[fmt]
    if fmt == 3:
        assert x[0] == -32768 and x[2048] == 0 and x[4095] == 2047 * 16
    else:
        assert x[0] == -1.0 and x[2048] == 0.0 and x[4095] == np.float32(2047 / 2048) and x.max() < 1.0
    codes, inexact, clamped = S.from_format(fmt, x)
    assert np.array_equal(codes, c) and (inexact, clamped) == (0, 0)
    hcodes, hwhat = header(exe, fmt, x, tmp_path)
    assert np.array_equal(hcodes, c) and not hwhat.any()
    with pytest.raises(ValueError, match="4095"):
        S.to_format(fmt, np.array([4096], np.uint16))


def f32(bits):
    return np.array(bits, dtype="<u4").view("<f4")


def test_float_edge_cases(exe, tmp_path):
    from adsbdec_amd import sample_formats as S
    grid = S.to_float32_real(np.arange(4096, dtype=np.uint16))
    ties = ((np.arange(-2049, 2049, dtype=np.float64) + 0.5) / 2048.0).astype("<f4")
    gb = grid.view("<u4")
    near = np.concatenate([gb[gb != 0] + 1, gb[gb != 0] - 1]).astype("<u4").view("<f4")     # one ulp either side (not of 0.0)
    named = {
        "+0.0": (0x00000000, 2048, EXACT), "-0.0": (0x80000000, 2048, EXACT),
        "smallest denormal": (0x00000001, 2048, INEXACT), "largest denormal": (0x007FFFFF, 2048, INEXACT),
        "-smallest denormal": (0x80000001, 2048, INEXACT), "-largest denormal": (0x807FFFFF, 2048, INEXACT),
        "+1.0": (0x3F800000, 4095, CLAMPED), "-1.0": (0xBF800000, 0, EXACT),
        "+Inf": (0x7F800000, 4095, CLAMPED), "-Inf": (0xFF800000, 0, CLAMPED),
        "NaN": (0x7FC00000, 2048, CLAMPED), "-NaN": (0xFFC00000, 2048, CLAMPED), "signalling NaN": (0x7F800001, 2048, CLAMPED),
        "1e30": (int(np.array(1e30, "<f4").view("<u4")), 4095, CLAMPED), "-1e30": (int(np.array(-1e30, "<f4").view("<u4")), 0, CLAMPED),
    }
    edge = f32([v[0] for v in named.values()])
    x = np.concatenate([grid, ties, near, edge])
    codes, what = header(exe, 1, x, tmp_path)
    ncodes, nwhat = numpy_what(1, x)
    assert np.array_equal(codes, ncodes) and np.array_equal(what, nwhat)
    # the grid: exact, every code
    assert np.array_equal(codes[:4096], np.arange(4096)) and not what[:4096].any()
    # ties go to the even neighbour; beyond the ends they clamp
    t_codes, t_what = codes[4096:4096 + ties.size], what[4096:4096 + ties.size]
    for k, c, w in zip(range(-2049, 2049), t_codes.tolist(), t_what.tolist()):
        even = k + 1 if k & 1 else k
        assert (c, w) == ((min(max(even, -2048), 2047) + 2048), CLAMPED if not -2048 <= even <= 2047 else INEXACT), k
    # one ulp off a grid point is never exact
    n_what = what[4096 + ties.size:4096 + ties.size + near.size]
    assert (n_what != EXACT).all()
    e_codes, e_what = codes[-edge.size:], what[-edge.size:]
    for (name, (_, c, w)), gc, gw in zip(named.items(), e_codes.tolist(), e_what.tolist()):
        assert (gc, gw) == (c, w), name
    # the counts: once per sample, clamped wins
    _, inexact, clamped = S.from_float32_real(x)
    assert inexact == int((what == INEXACT).sum()) and clamped == int((what == CLAMPED).sum())


def test_random_bits_header_equals_numpy(exe, tmp_path):
    """Random bit patterns -- off-grid values, NaN, Inf, denormals, huge values -- through both definitions."""
    rng = np.random.default_rng(20261018)
    bits = rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype("<u4")
    bits[:20_000] &= 0x807FFFFF                                  # denormals and zeros
    bits[20_000:40_000] = (bits[20_000:40_000] & 0x80FFFFFF) | 0x3F000000    # |x| in [0.5, 1): near the grid's range
    x = bits.view("<f4")
    codes, what = header(exe, 1, x, tmp_path)
    ncodes, nwhat = numpy_what(1, x)
    assert np.array_equal(codes, ncodes) and np.array_equal(what, nwhat)
    assert {EXACT, INEXACT, CLAMPED} == set(np.unique(what).tolist())


def test_file_converter_round_trips(tmp_path):
    x = np.random.default_rng(5).integers(0, 4096, 10_001, dtype=np.uint16)
    x.tofile(tmp_path / "a.u16")
    run = lambda *a: subprocess.run([sys.executable, "-m", "adsbdec_amd.sample_formats", *a], cwd=ROOT, capture_output=True, text=True, check=True)
    for t, ext, size in ((3, "s16", 2), (1, "f32", 4)):
        run("-t", str(t), str(tmp_path / "a.u16"), str(tmp_path / f"a.{ext}"))
        assert os.path.getsize(tmp_path / f"a.{ext}") == size * x.size
        p = run("-t", str(t), "--back", str(tmp_path / f"a.{ext}"), str(tmp_path / "b.u16"))
        assert p.stderr == "" and np.array_equal(np.fromfile(tmp_path / "b.u16", np.uint16), x)
    p = run("-t", "3", "--back", str(tmp_path / "a.u16"), str(tmp_path / "c.u16"))      # a raw file read as int16: off the grid
    assert "samples are not INT16_REAL values" in p.stderr


def test_entry_points_are_declared_and_exported(capi):
    inc = os.path.join(ROOT, "include")
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd_diag.h")).read(), flags=re.S)
    for name in ENTRY_POINTS[:-1]:
        assert re.search(rf"\b{name}\s*\(", main), name
    assert re.search(r"\badsb_convert_samples\s*\(", diag) and "adsb_convert_samples" not in main
    assert "adsb_format_report" in main and "#define ADSB_ABI_VERSION 5" in main
    from adsbdec_amd import _build
    assert "convert_samples.hip" in _build.HIP_SOURCES
    assert "convert_samples.hip.o" in open(os.path.join(ROOT, "Makefile")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS:
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name


def test_format_bytes(capi, tmp_path):
    L = capi.load()
    for fmt, size in ((1, 4), (3, 2), (4, 2), (5, 2), (0, 0), (2, 0), (7, 0), (-1, 0)):
        for n in (0, 1, 7, 1 << 24, (1 << 32) + 3):
            assert L.adsb_format_bytes(fmt, n) == size * n, (fmt, n)
    # and from C, through the main header alone
    src = tmp_path / "m.c"
    src.write_text('#include "adsbdec_amd.h"\n#include <stdio.h>\nint main(void) { adsb_format_report r = {0, 0, 0}; (void)r;\n'
                   'printf("%zu %zu %zu\\n", adsb_format_bytes(ADSB_FMT_FLOAT32_REAL, 3), adsb_format_bytes(ADSB_FMT_INT16_REAL, 3), '
                   'adsb_format_bytes(ADSB_FMT_RAW, 3) + adsb_format_bytes(ADSB_FMT_UINT16_REAL, 0)); return 0; }\n')
    from adsbdec_amd import _build
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "m"),
                    "-L", _build.LIBDIR, "-ladsbdec_amd", f"-Wl,-rpath,{_build.LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(tmp_path / "m")], capture_output=True, text=True).stdout.split() == ["12", "6", "6"]


@pytest.mark.parametrize("args,words", [
    (["-t", "0"], ["-t 0", "IQ", "raw twin"]),
    (["-t", "2"], ["-t 2", "IQ", "raw twin"]),
    (["-t", "9"], ["-t 9"]),
    (["-t", "3", "-p"], ["-t 3", "-p"]),
    (["-t", "3", "-G", "2"], ["-t 3", "-G"]),
    (["-t", "1", "-B", "list"], ["-t 1", "-B"]),
])
def test_cli_refusals_come_before_any_gpu_call(capi, tmp_path, args, words):
    """Each is refused with a message and exit status 1 before the GPU runtime is touched: the files need not exist, and no
    device is needed (this box has none)."""
    extra = [] if "-B" in args else ["-f", str(tmp_path / "x")]
    p = subprocess.run([capi.CLI_PATH, *args, *extra], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and p.stdout == "", (p.returncode, p.stdout, p.stderr)
    for w in words:
        assert w in p.stderr, (w, p.stderr)


def test_cli_usage_names_the_flag(capi):
    u = subprocess.run([capi.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert u.returncode == 1 and "[-t type]" in u.stdout and "\t-t type :" in u.stdout
    assert "[-p]" in u.stdout and "\t-p :" in u.stdout        # what the packed test looks for is still there
