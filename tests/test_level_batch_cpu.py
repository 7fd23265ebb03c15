"""The batch level report without a GPU: the adsb_level_batch_* calls are declared, exported and bound; the gfx950 code of
level_batch_kernel.hip has no scratch, one real kernel and three unit kernels, the FIR's own fused operations once and Stage A's 17
typed loads, a histogram per wave in LDS and nothing more; the table the host side builds, the row search, the split of the passes
over the waves and the per-wave accumulate-and-flush hold on the CPU, under the sanitizers, in a program of their own."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

ENTRY_POINTS = ("adsb_level_batch_device", "adsb_level_batch_device_as", "adsb_level_batch_device_packed", "adsb_level_batch_device_iq",
                "adsb_level_batch_device_power", "adsb_level_batch_host")
FUSED = r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)"


def test_entry_points_are_declared_exported_and_bound(capi):
    import ctypes as C
    from adsbdec_amd import _build
    inc = os.path.join(ROOT, "include")
    strip = lambda h: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
    main, diag = strip("adsbdec_amd.h"), strip("adsbdec_amd_diag.h")
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        n_args = 8 if name.endswith(("_as", "_iq")) else 7
        assert len(capi.SYMBOLS[name][1]) == n_args and capi.SYMBOLS[name][0] is C.c_long, name
    for m in ("level_batch_device", "level_batch_device_as", "level_batch_device_packed", "level_batch_device_iq", "level_batch_device_power",
              "level_batch"):
        assert callable(getattr(capi.Decoder, m)), m
    assert "level_batch_kernel.hip" in _build.HIP_SOURCES and "decoder_level_batch.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "level_batch_kernel.hip.o" in mk and "decoder_level_batch.hip.o" in mk
    # symbols are added, no struct changes: the ABI stays 5, the report is the single calls', and the knob that lets a small batch
    # exercise the flush is a call of the diag header's, not of the drop-in one
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main
    assert C.sizeof(capi.LevelReport) == 8 * (5 + 2048)
    assert re.search(r"\bint\s+adsb_debug_set_level_batch_blocks\s*\(", diag) and "adsb_debug_set_level_batch_blocks" not in main
    assert "adsb_debug_set_level_batch_blocks" in exported and callable(capi.Decoder.set_level_batch_blocks)
    # NULL handle: -1, nothing touched
    assert L.adsb_level_batch_device(None, 0, None, None, None, None, None) == -1
    assert L.adsb_level_batch_host(None, 0, None, None, None, None, None) == -1
    assert L.adsb_debug_set_level_batch_blocks(None, 1) == -1


def test_the_header_says_what_is_in_and_what_is_out():
    main = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    assert "No batch, multi-GPU or stream-window form" not in main
    assert "adsb_level_batch_*: a BATCH of captures" in main and "No multi-GPU or stream-window form" in main


@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "level_batch_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def test_isa_of_the_batch_level_unit(isa):
    """What tests/test_level_cpu.py asks of level_kernel.hip, asked of the batch unit: gfx950 only; one real kernel and three unit
    kernels, none with scratch; the FIR once (184 products and 24 accumulations, nothing else fused -- a 64-bit division in a kernel
    would show here as v_fmamk_f32: the split of the passes over the waves is divided on the host) behind Stage A's 17 typed loads;
    the histogram is LDS adds that return nothing, a histogram per wave and 16 bytes beside it; the 64-bit totals take vector atomics;
    ONE workgroup barrier per kernel (the waves meet at their end, never per pass); the row of a pass is found by scalar loads from
    the table."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 4, sorted(sizes)
    assert sum("level_units_batch_kernel" in k for k in sizes) == 3 and sum(bool(re.search(r"\d+level_batch_kernel", k)) for k in sizes) == 1
    for name, size in sizes.items():
        assert int(size) == 0, f"{name} spills to scratch"
    fused = re.findall(FUSED, isa, flags=re.M)
    assert set(fused) <= {"v_pk_fma_f32"}, f"contracted arithmetic in the ISA: {sorted(set(fused))}"
    assert len(re.findall(r"^\s*v_pk_fma_f32", isa, flags=re.M)) == 184 + 24
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", isa, flags=re.M)) == 17
    assert re.search(r"^\s*ds_add_u32", isa, flags=re.M) and not re.search(r"^\s*ds_add_rtn", isa, flags=re.M)
    assert re.search(r"^\s*global_atomic_add_x2", isa, flags=re.M) and not re.search(r"^\s*flat_atomic", isa, flags=re.M)
    assert len(re.findall(r"^\s*s_barrier", isa, flags=re.M)) == 4       # one per kernel: block_finish
    lds = [int(v) for v in re.findall(r"^\s*\.amdhsa_group_segment_fixed_size\s+(\d+)", isa, flags=re.M)]
    assert len(lds) == 4 and max(lds) <= 4 * 8192 + 64                     # a histogram per wave: 5 workgroups a CU
    table_loads = [b for b in re.findall(r"^\s*s_load_dword(?:x\d+)?\s+s\[?[\d:]+\]?,\s*(s\[\d+:\d+\])", isa, flags=re.M) if b != "s[0:1]"]
    assert len(table_loads) >= 4, table_loads                              # (each of the four kernels reads its rows so, in wide loads)


def test_table_ranges_and_flush_under_the_sanitizers(tmp_path):
    """csrc/level_batch.hpp compiled for the host with -fsanitize=address,undefined, a program of its own (tests/cpp/level_batch_rows.cpp):
    seeded lists with lengths around 0, one run, one pass and several passes and empty captures between them, up to 700 captures;
    every unit maps to the right capture and pass; the ranges of 1, 4 and 8192 waves cover every unit exactly once; the per-wave
    accumulate-and-flush on small counters leaves in every capture's totals what a direct count leaves, and writes every run's
    envelope once."""
    exe = tmp_path / "level_batch_rows"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "level_batch_rows.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 62 lists"), p.stdout + p.stderr
