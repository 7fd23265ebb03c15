"""Batches of packed captures without a GPU: the batched unpack kernel's build (gfx950: one kernel, no scratch, 12 bytes in and
16 bytes out per lane), the new entry points in the headers, the library and the bindings, and the C host program's -B flag
as far as it goes before the GPU runtime is touched."""
import os
import re
import subprocess

from conftest import ROOT

ENTRY_POINTS = ("adsb_decode_batch_device_packed", "adsb_decode_batch_host_packed", "adsb_multi_decode_batch_host",
                "adsb_multi_decode_batch_files")
DIAG_ENTRY_POINTS = ("adsb_multi_batch_plan", "adsb_multi_set_batch_bytes")


def test_batched_unpack_kernel_builds_for_gfx950_without_scratch():
    from adsbdec_amd import _build
    assert "unpack12_batch.hip" in _build.HIP_SOURCES
    assert "unpack12_batch.hip.o" in open(os.path.join(ROOT, "Makefile")).read()
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "unpack12_batch.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert '.amdgcn_target "amdgcn-amd-amdhsa--gfx950"' in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and "unpack12_batch_kernel" in next(iter(sizes))
    assert all(int(v) == 0 for v in sizes.values()), sizes
    assert re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", isa, flags=re.M) == ["0"]
    assert re.search(r"^\s*global_load_dwordx3\b", isa, flags=re.M)      # 12 bytes in per group ...
    assert re.search(r"^\s*global_store_dwordx4\b", isa, flags=re.M)     # ... 16 bytes out
    assert not re.search(r"^\s*(ds_|scratch_|flat_)", isa, flags=re.M)   # no LDS, no scratch, no generic-address access
    # the rows of a chunk's first and last group are looked up by the scalar unit (once per wave, not per lane): two bisections,
    # each a loop around a 64-bit scalar load of a row's running group count.  The kernel's own arguments are scalar loads too,
    # off s[0:1] (the kernarg pointer is the only user SGPR pair), so those do not count.
    assert re.search(r"^\s*\.amdhsa_user_sgpr_count\s+2\s*$", isa, flags=re.M)
    assert re.search(r"^\s*\.amdhsa_user_sgpr_kernarg_segment_ptr\s+1\s*$", isa, flags=re.M)
    table_loads = [base for base in re.findall(r"^\s*s_load_dwordx2\s+s\[\d+:\d+\],\s*(s\[\d+:\d+\])", isa, flags=re.M) if base != "s[0:1]"]
    assert len(table_loads) >= 2, table_loads
    assert int(re.search(r"^\s*\.vgpr_count:\s*(\d+)", isa, flags=re.M).group(1)) <= 32


def test_row_lookup_on_the_host(tmp_path):
    """csrc/packed12.h unpack12_row -- what the kernel finds a group's capture with -- compiled for the host: captures of 1
    group and of 2^29 groups side by side, every group around every capture boundary and random ones, looked up chunk-wise as
    the kernel does."""
    exe = tmp_path / "unpack12_rows"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "unpack12_rows.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 200 tables"), p.stdout + p.stderr


def test_the_bit_layout_is_written_once():
    """The batched kernel goes through packed12.h's unpack12_group_pairs, the function the CPU test checks: no second copy."""
    text = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "unpack12_batch.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert "unpack12_group_pairs(" in code and '#include "packed12.h"' in code
    assert "0xfff" not in code.lower() and ">> 20" not in code and "__shared__" not in code


def test_entry_points_are_declared_and_exported(capi):
    inc = os.path.join(ROOT, "include")
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "adsbdec_amd_diag.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", main), name
    for name in DIAG_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", diag) and not re.search(rf"\b{name}\s*\(", main), name
    from adsbdec_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ENTRY_POINTS + DIAG_ENTRY_POINTS:
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
    assert "#define ADSB_ABI_VERSION 5" in main                         # nothing that exists changed meaning or place


def test_python_bindings_exist(capi):
    from adsbdec_amd import sharding
    for name in ("decode_batch_device_packed_raw", "decode_batch_device_packed", "decode_batch_packed"):
        assert callable(getattr(capi.Decoder, name)), name
    for name in ("decode_batch_host", "decode_batch_files", "set_batch_bytes"):
        assert callable(getattr(sharding.MultiDecoder, name)), name


def _cli(capi, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60)


def test_cli_batch_list_usage_errors_before_any_gpu_call(capi, tmp_path):
    """-B with -f, -s or -l: the usage text and exit status 1; a list file that is not there: a message and a non-zero status.
    All of it before the GPU runtime is touched (this box has no device)."""
    lst = tmp_path / "list.txt"
    lst.write_text(str(tmp_path / "a.u16") + "\n")
    for extra in (["-f", str(tmp_path / "a.u16")], ["-s", "127.0.0.1:1"], ["-l", "127.0.0.1:1"], ["-d", "0", "-G", "2"]):
        p = _cli(capi, "-a", "-B", str(lst), *extra)
        assert p.returncode == 1 and p.stdout.startswith("adsbdec_amd :") and "-B listfile" in p.stdout, (extra, p.stdout, p.stderr)
    p = _cli(capi, "-B", str(tmp_path / "no_such_list"))
    assert p.returncode != 0 and p.stdout == ""
    assert "no_such_list" in p.stderr and "list of captures" in p.stderr
    u = _cli(capi)
    assert u.returncode == 1 and "-B listfile" in u.stdout and "\t-B listfile :" in u.stdout


def test_cli_keeps_what_it_refused_before(capi, tmp_path):
    f = str(tmp_path / "x")
    assert _cli(capi, "-f", f, "-f", f).returncode == 1                                   # several -f without -G
    assert _cli(capi, "-G", "2", "-s", "127.0.0.1:1", "-f", f, "-f", f).returncode == 1   # -G with -s and several captures
    many = [a for _ in range(65) for a in ("-f", f)]
    assert _cli(capi, "-G", "2", *many).returncode == 1                                   # the 65th -f
    p = _cli(capi, "-p", "-G", "2", "-f", f)
    assert p.returncode == 1 and "-p" in p.stderr and "-G" in p.stderr                    # -p with -G -f
