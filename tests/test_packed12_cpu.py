"""Airspy packed 12-bit input without a GPU: the format's known answers through the numpy definition (adsbdec_amd/packed12.py)
and through the group arithmetic the unpack kernel runs (csrc/packed12.h, compiled for the host), pack/unpack round trips,
the kernel's build (gfx950, no scratch), the C-ABI's new entry points, and the C host program's -p flag."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

KAT = [
    ("78 56 34 12 f0 de bc 9a 78 56 34 12", [0x123, 0x456, 0x789, 0xABC, 0xDEF, 0x012, 0x345, 0x678]),
    ("ff 02 18 00 00 80 ff f7 0f 0f 5a a5", [0x001, 0x802, 0xFFF, 0x7FF, 0x800, 0x0A5, 0x5A0, 0xF0F]),
]
ENTRY_POINTS = ("adsb_push_packed", "adsb_push_packed_async", "adsb_push_device_packed", "adsb_push_device_packed_final",
                "adsb_decode_device_packed", "adsb_unpack_packed12")


@pytest.mark.parametrize("hexbytes,samples", KAT)
def test_known_answers_numpy(hexbytes, samples):
    from adsbdec_amd import packed12 as P
    b = bytes.fromhex(hexbytes.replace(" ", ""))
    assert P.unpack12(b).tolist() == samples
    assert P.pack12(np.array(samples, np.uint16)).tobytes() == b
    assert P.packed_bytes(8) == 12


def test_every_code_at_every_position_round_trips():
    from adsbdec_amd import packed12 as P
    rng = np.random.default_rng(20261015)
    x = rng.integers(0, 4096, size=(8, 4096, 8), dtype=np.uint16)   # [position, code, group]
    for pos in range(8):
        x[pos, :, pos] = np.arange(4096)
    x = x.reshape(-1)
    b = P.pack12(x)
    assert b.dtype == np.uint8 and b.size == x.size // 8 * 12
    assert np.array_equal(P.unpack12(b), x)
    assert np.array_equal(P.pack12(P.unpack12(b)), b)
    # the definition, independently: field k of the 96-bit big-endian number w0:w1:w2
    g = b.reshape(-1, 12).view("<u4").astype(object)
    big = (g[:, 0] << 64) | (g[:, 1] << 32) | g[:, 2]
    for k in range(8):
        assert [int(v) for v in (big >> (84 - 12 * k)) & 0xFFF] == x.reshape(-1, 8)[:, k].tolist()


def test_pack_refuses_what_the_format_cannot_hold():
    from adsbdec_amd import packed12 as P
    with pytest.raises(ValueError, match="8-sample groups"):
        P.pack12(np.zeros(7, np.uint16))
    with pytest.raises(ValueError, match="4095"):
        P.pack12(np.full(8, 4096, np.uint16))
    with pytest.raises(ValueError, match="12-byte groups"):
        P.unpack12(b"\0" * 13)


def test_file_converter_round_trips(tmp_path):
    import sys
    x = np.random.default_rng(3).integers(0, 4096, 8 * 1000 + 5, dtype=np.uint16)
    x.tofile(tmp_path / "a.u16")
    run = lambda *a: subprocess.run([sys.executable, "-m", "adsbdec_amd.packed12", *a], cwd=ROOT, capture_output=True, text=True, check=True)
    p = run(str(tmp_path / "a.u16"), str(tmp_path / "a.p12"))
    assert "5 trailing samples" in p.stderr
    assert os.path.getsize(tmp_path / "a.p12") == 12000
    run("--unpack", str(tmp_path / "a.p12"), str(tmp_path / "b.u16"))
    assert np.array_equal(np.fromfile(tmp_path / "b.u16", np.uint16), x[:8000])


def test_header_group_arithmetic_on_the_host(tmp_path):
    """csrc/packed12.h -- the function unpack12_kernel runs -- compiled for the host: both known answers, and every 12-bit
    code at each of the 8 positions of a group with random neighbours, against the definition bit by bit."""
    exe = tmp_path / "packed12"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "packed12.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "2 known answers, 32768 groups" in p.stdout


def test_unpack_kernel_builds_for_gfx950_without_scratch():
    from adsbdec_amd import _build
    assert "unpack12.hip" in _build.HIP_SOURCES
    assert "unpack12.hip.o" in open(os.path.join(ROOT, "Makefile")).read()
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "unpack12.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert '.amdgcn_target "amdgcn-amd-amdhsa--gfx950"' in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and "unpack12_kernel" in next(iter(sizes))
    assert all(int(v) == 0 for v in sizes.values()), sizes
    assert re.search(r"^\s*global_load_dwordx3\b", isa, flags=re.M)      # 12 bytes in per group ...
    assert re.search(r"^\s*global_store_dwordx4\b", isa, flags=re.M)     # ... 16 bytes out
    assert not re.search(r"^\s*ds_", isa, flags=re.M)                    # no LDS


def test_entry_points_are_declared_and_exported(capi):
    inc = os.path.join(ROOT, "include")
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd_diag.h")).read(), flags=re.S)
    for name in ENTRY_POINTS[:5]:
        assert re.search(rf"\b{name}\s*\(", main), name
    assert re.search(r"\badsb_unpack_packed12\s*\(", diag)
    assert "#define ADSB_PACKED12_BYTES(n)" in main
    from adsbdec_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS:
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name


def test_packed_bytes_macro_in_c(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include "adsbdec_amd.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu\\n", (size_t)ADSB_PACKED12_BYTES((size_t)8), '
                   '(size_t)ADSB_PACKED12_BYTES((size_t)1 << 20)); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "m")], check=True)
    assert subprocess.run([str(tmp_path / "m")], capture_output=True, text=True).stdout.split() == ["12", str(3 << 19)]


def test_cli_refuses_packed_with_multi_gpu_before_any_gpu_call(capi, tmp_path):
    """-p -G is refused with a message and exit status 1, before the GPU runtime is touched: the file need not even exist, and
    no device is needed (this box has none)."""
    p = subprocess.run([capi.CLI_PATH, "-p", "-G", "2", "-f", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stdout == ""
    assert "-p" in p.stderr and "-G" in p.stderr
    u = subprocess.run([capi.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert u.returncode == 1 and "[-p]" in u.stdout and "\t-p :" in u.stdout
    assert subprocess.run([capi.CLI_PATH, "-e"], capture_output=True).returncode == 1     # -e stays unknown
