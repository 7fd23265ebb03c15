"""The batch power export without a GPU: the adsb_power_batch_* calls are declared, exported and bound; the gfx950 code of
power_export_batch_kernel.hip has no scratch, contracts nothing, carries the FIR's own fused operations once per copy and Stage A's
17 typed loads; the table the host side builds and the row search the kernels make hold on the CPU, under the sanitizers, for
randomised lists of capture lengths."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_power_export_cpu import FUSED, kernel_bodies

ENTRY_POINTS = ("adsb_power_batch_device", "adsb_power_batch_device_as", "adsb_power_batch_device_packed", "adsb_power_batch_device_iq",
                "adsb_power_batch_host")
# FIR copies in power_export_batch_kernel.hip: ONE.  The unit has one kernel with a FIR (power_export_batch_kernel;
# iq_power_export_batch_kernel has none), the kernel is not a template, the row look-up in front of the body is scalar code that
# duplicates nothing behind it, and the two load paths (typed buffer loads inside a capture, plain loads at its edges) join in front
# of the FIR, as they do in power_export_kernel.
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
    for m in ("power_batch_device", "power_batch_device_as", "power_batch_device_packed", "power_batch_device_iq", "power_batch"):
        assert callable(getattr(capi.Decoder, m)), m
    assert "power_export_batch_kernel.hip" in _build.HIP_SOURCES and "decoder_export_batch.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "power_export_batch_kernel.hip.o" in mk and "decoder_export_batch.hip.o" in mk
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main
    assert not re.search(r"^\s*(import|from)\s+torch", open(os.path.join(ROOT, "adsbdec_amd", "capi.py")).read(), flags=re.M)


@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "power_export_batch_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def test_isa_of_the_batch_export_unit(isa):
    """What tests/test_power_export_cpu.py asks of power_export_kernel.hip, asked of the batch unit: gfx950 only; two kernels, neither
    with scratch; the fused operations are the FIR's own (184 products and 24 shared-product accumulations per copy, packed) and none
    of the planes' sign tests; Stage A's 17 typed loads; a whole wave turns through LDS (7 + 7 accesses of 16 bytes) and leaves in 7
    stores, a ragged wave in 7 more; no workgroup barrier.  The IQ kernel fuses nothing.  The row of a pass is found by scalar loads
    from the table: the kernel's only other scalar loads are its three arguments'."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 2 and any("iq_power_export_batch_kernel" in k for k in sizes)
    assert any(re.search(r"\d+power_export_batch_kernel", k) for k in sizes)
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
    assert len(re.findall(r"^\s*v_pk_add_f32", isa, flags=re.M)) >= (168 - 24) * FIR_COPIES
    assert len(re.findall(r"^\s*v_pk_mul_f32", isa, flags=re.M)) >= 28 * FIR_COPIES
    bodies = kernel_bodies(isa)
    iq = [b for n, b in bodies.items() if "iq_power_export_batch_kernel" in n][0]
    assert not re.findall(FUSED, iq, flags=re.M)
    assert len(re.findall(r"^\s*v_mul_f32|^\s*v_pk_mul_f32", iq, flags=re.M)) >= 1 and "global_store_dwordx4" in iq
    fir = [b for n, b in bodies.items() if "iq_power_export_batch_kernel" not in n][0]
    assert len(re.findall(r"^\s*buffer_load_format_xyzw", fir, flags=re.M)) == 17 * FIR_COPIES
    assert len(re.findall(r"^\s*ds_write_b128|^\s*ds_store_b128", fir, flags=re.M)) == 7
    assert len(re.findall(r"^\s*ds_read_b128|^\s*ds_load_b128", fir, flags=re.M)) == 7
    assert len(re.findall(r"^\s*global_store_dwordx4", fir, flags=re.M)) == 14 and "s_barrier" not in fir
    # the row search and the row itself: scalar loads whose base is not the kernarg pointer s[0:1]
    table_loads = [b for b in re.findall(r"^\s*s_load_dword(?:x\d+)?\s+s\[?[\d:]+\]?,\s*(s\[\d+:\d+\])", fir, flags=re.M) if b != "s[0:1]"]
    assert len(table_loads) >= 2, table_loads
    # and no lane loads from the table: the kernel's vector loads are the capture's samples, 34 pairs of the plain-load road
    assert len(re.findall(r"^\s*global_load_dword\b", fir, flags=re.M)) == 34
    assert not re.findall(r"^\s*global_load_dwordx[234]", fir, flags=re.M)


def test_table_and_row_search_under_the_sanitizers(tmp_path):
    """csrc/power_export_batch.hpp compiled for the host with -fsanitize=address,undefined, a program of its own: lists with zeros,
    lengths 1 .. 7, lengths at 3584 k and 3584 k +- 1 .. 4, a capture of 2^32 - 4 samples, up to 2048 captures; every pass maps to the
    right capture and in-capture pass, the closing row holds the total, captures without power samples have no row."""
    exe = tmp_path / "power_export_batch_rows"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "power_export_batch_rows.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 302 lists"), p.stdout + p.stderr
