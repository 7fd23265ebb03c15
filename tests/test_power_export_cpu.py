"""The power export without a GPU: the adsb_power_* calls are declared, exported and bound; the gfx950 code of
power_export_kernel.hip has no scratch, contracts nothing and carries the FIR's own fused operations once per copy; the properties
of the reference's power samples that the GPU tests stand on (prefix, 28-sample shift, silence in front) hold under the oracle; the
C host program's -W refuses what it cannot combine with before any GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ENTRY_POINTS = ("adsb_power_window", "adsb_power_window_host", "adsb_power_device", "adsb_power_device_as", "adsb_power_device_packed",
                "adsb_power_device_iq")
# FIR copies in power_export_kernel.hip: ONE.  The unit has one kernel with a FIR (power_export_kernel; iq_power_export_kernel has
# none), the kernel is not a template, and its two load paths (typed buffer loads inside the buffer, plain loads at its edges) join
# in front of the FIR, as they do in stage_a.
FIR_COPIES = 1


def test_entry_points_are_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
    for m in ("power_window", "power_window_host", "power_device", "power_device_as", "power_device_packed", "power_device_iq", "power"):
        assert callable(getattr(capi.Decoder, m)), m
    assert "power_export_kernel.hip" in _build.HIP_SOURCES and "decoder_export.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "power_export_kernel.hip.o" in mk and "decoder_export.hip.o" in mk
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main
    assert not re.search(r"^\s*(import|from)\s+torch", open(os.path.join(ROOT, "adsbdec_amd", "capi.py")).read(), flags=re.M)


@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "power_export_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


FUSED = r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)"


def kernel_bodies(isa):
    """name -> the instructions between the kernel's label and its s_endpgm-terminated body's .amdhsa_kernel block."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", isa, flags=re.M)
    bodies = {}
    for n in names:
        m = re.search(rf"^{re.escape(n)}:[^\n]*\n(.*?)^\s*\.amdhsa_kernel\s+{re.escape(n)}", isa, flags=re.M | re.S)
        assert m, n
        bodies[n] = m.group(1)
    return bodies


def test_isa_of_the_export_unit(isa):
    """gfx950 only; two kernels, neither with scratch; the fused operations are the FIR's own and nothing else: per FIR copy the 184
    products t (x - 2048) = fma(t, x, -2048 t) (packed, scalar tap pair, vector constant pair) and the 24 accumulations of a shared
    product fma(M, (2, 1) | (1, 2), s) that tests/test_build_flags.py pins for scan_kernel.hip's FIR -- and none of its sign tests
    (2 c' - c, the factor 2.0), which belong to the planes this kernel does not build.  The IQ kernel fuses nothing."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 2 and any("iq_power_export_kernel" in k for k in sizes) and any(re.search(r"\d+power_export_kernel", k) for k in sizes)
    for name, size in sizes.items():
        assert int(size) == 0, f"{name} spills to scratch"
    fused = re.findall(FUSED, isa, flags=re.M)
    assert set(fused) <= {"v_fma_f32", "v_pk_fma_f32"}, f"contracted arithmetic in the ISA: {sorted(set(fused))}"
    lines = re.findall(r"^\s*v_pk_fma_f32.*$", isa, flags=re.M)
    by_two = [ln for ln in lines if re.search(r"\b2\.0\b", ln)]
    products = [ln for ln in lines if re.search(r",\s*s\[\d+:\d+\],\s*v\[\d+:\d+\]", ln) and ln not in by_two]
    assert not by_two and "v_fma_f32" not in fused                      # no sign test, packed or scalar
    assert len(lines) == (184 + 24) * FIR_COPIES, len(lines)
    assert len(products) >= 184 * FIR_COPIES, len(products)
    # the sums and the squares stay separate: 28 outputs x 6 additions, less the 24 that are the shared products' accumulations
    assert len(re.findall(r"^\s*v_pk_add_f32", isa, flags=re.M)) >= (168 - 24) * FIR_COPIES
    assert len(re.findall(r"^\s*v_pk_mul_f32", isa, flags=re.M)) >= 28 * FIR_COPIES
    bodies = kernel_bodies(isa)
    iq = [b for n, b in bodies.items() if "iq_power_export_kernel" in n][0]
    assert not re.findall(FUSED, iq, flags=re.M)
    assert len(re.findall(r"^\s*v_mul_f32|^\s*v_pk_mul_f32", iq, flags=re.M)) >= 1 and "global_store_dwordx4" in iq
    fir = [b for n, b in bodies.items() if "iq_power_export_kernel" not in n][0]
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", fir, flags=re.M)) == 17                          # Stage A's loads
    # a whole wave's samples turn through LDS (7 writes, 7 reads of 16 bytes) and leave in 7 stores of contiguous lines; the
    # window's ragged last wave stores 7 x 16 bytes per lane; no workgroup barrier anywhere
    assert len(re.findall(r"^\s*ds_write_b128|^\s*ds_store_b128", fir, flags=re.M)) == 7
    assert len(re.findall(r"^\s*ds_read_b128|^\s*ds_load_b128", fir, flags=re.M)) == 7
    assert len(re.findall(r"^\s*global_store_dwordx4", fir, flags=re.M)) == 14 and "s_barrier" not in fir


# ------------------------------------------------------------------ the oracle properties the GPU tests stand on
N_ORACLE = 1 << 14


@pytest.fixture(scope="module")
def full_range():
    return np.random.default_rng(1717).integers(0, 65536, N_ORACLE, dtype=np.uint16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_oracle_prefix_property(oracle, full_range):
    """power(x[:n])[:2 (n // 4)] == power(x)[:2 (n // 4)] for ragged n: a power sample depends on no later pair."""
    x = full_range
    a = oracle.power(x)
    for n in list(range(0, 13)) + [57, 58, 59, 3583, 3585, 3586, 3587, N_ORACLE - 1]:
        k = 2 * (n // 4)
        assert np.array_equal(bits(oracle.power(x[:n].copy())[:k]), bits(a[:k])), n


def test_oracle_shift_property(oracle, full_range):
    """power(x[f:])[6:] == power(x)[f // 2 + 6:] for f a multiple of 28 samples -- and for no smaller shift tried: the phase is
    m mod 7 together with the fs/4 sign, so the stream's period is 28 samples."""
    x = full_range
    a = oracle.power(x)
    for f in (28, 56, 196, 364):
        assert np.array_equal(bits(oracle.power(x[f:].copy())[6:]), bits(a[f // 2 + 6:])), f
    for f in (4, 8, 14):
        assert not np.array_equal(bits(oracle.power(x[f:].copy())[6:]), bits(a[f // 2 + 6:])), f


def test_oracle_silence_property(oracle, full_range):
    """28 samples of 0x800 in front of a capture give the capture's own array behind them: a pair that is not held reads as silence,
    which is the reference's zeroed ring (air.c:33)."""
    x = full_range
    a = oracle.power(x)
    b = oracle.power(np.concatenate([np.full(28, 0x800, np.uint16), x]))
    assert np.array_equal(bits(b[14:]), bits(a)) and not b[:14].any()


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_export_refusals_and_usage(capi, tmp_path):
    """-W with -w, -t, -p, -G, -B, -s, -l or several -f: exit 1 with a reason before any GPU call (the files do not even exist, and
    nothing is created); -e stays unknown; the usage text names -W."""
    capi.load()
    for extra, word in ((["-w"], "-w"), (["-t", "3"], "-t"), (["-p"], "-p"), (["-G", "2"], "-G"), (["-s", "127.0.0.1:9"], "-s"),
                        (["-l", "127.0.0.1:9"], "-l"), (["-f", "other.bin"], "several -f")):
        p = _cli(capi, tmp_path, "-W", "out.pw", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and "-W is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
    p = _cli(capi, tmp_path, "-W", "out.pw", "-B", "list.txt")
    assert p.returncode == 1 and "-W is not supported with -B: " in p.stderr
    assert not os.path.exists(tmp_path / "out.pw")
    p = _cli(capi, tmp_path, "-W", "out.pw")                             # no input: the usage text
    assert p.returncode == 1 and "usage" in p.stdout
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "-W out.pw -f filename" in u.stdout and "\t-W out.pw :" in u.stdout and "invalid option" in u.stderr
