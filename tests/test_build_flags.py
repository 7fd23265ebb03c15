"""The kernel's arithmetic must round like binary32 multiply-THEN-add: check that the gfx950 ISA hipcc emits
for the scan kernel contains exactly the fused operations the source writes (each exact by construction), no scratch
(spills), and that it is built for gfx950 only."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "scan_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def test_fused_operations_of_the_scan_kernel_are_the_exact_ones(isa):
    """The signal arithmetic is binary32 multiply, THEN binary32 add.  The compiler contracts nothing
    (-ffp-contract=off); the fused multiply-adds in the ISA are the ones scan_kernel.hip writes itself, each of which rounds
    the same real number the reference's separate operation rounds:
      * 56 sign tests per instantiation (2 c' - c on truncated integers: 22 packed + 12 scalar, the factor is the literal 2.0);
      * the FIR's products  t (x - 2048) = fma(t, x, -2048 t)  (2048 t is exact): 196 per run of 28 outputs, 12 of them
        shared by two outputs -> 184 packed instructions with a scalar tap pair and a vector constant pair;
      * the 24 accumulations of a shared product  s + 2 M = fma(M, (2, 1) | (1, 2), s)  (doubling is exact).
    Anything else fused, or another count, is a contraction bug or a change of the FIR that has to come here too."""
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*)", isa, flags=re.M)
    kernels = len(re.findall(r"^\s*\.amdhsa_kernel\s.*scan_kernel", isa, flags=re.M))
    assert kernels == 2  # scan_kernel<true|false> (count_tries_kernel has no float math)
    assert set(fused) <= {"v_fma_f32", "v_pk_fma_f32"}, f"contracted arithmetic in the ISA: {sorted(set(fused))}"
    packed = sum(1 for f in fused if f.startswith("v_pk_"))
    scalar = len(fused) - packed
    assert scalar == 12 * kernels, f"{scalar} scalar fused operations, expected {12 * kernels} (sign tests of the odd columns)"
    assert packed == (22 + 184 + 24) * kernels, f"{packed} packed fused operations, expected {(22 + 184 + 24) * kernels}"
    lines = re.findall(r"^\s*v_pk_fma_f32.*$", isa, flags=re.M)
    by_two = [ln for ln in lines if re.search(r"\b2\.0\b", ln)]          # the sign tests multiply by the literal 2.0 ...
    products = [ln for ln in lines if re.search(r",\s*s\[\d+:\d+\],\s*v\[\d+:\d+\]", ln) and ln not in by_two]
    assert len(by_two) == 22 * kernels, len(by_two)                       # (demod.c:83's SN)
    assert len(products) >= 184 * kernels, len(products)                  # ... a product reads scalar taps and a vector constant
    for ln in re.findall(r"^\s*v_fma_f32.*$", isa, flags=re.M):
        assert re.search(r"\b2\.0\b", ln), ln
    assert "-ffp-contract=off" in __import__("adsbdec_amd._build", fromlist=["HIP_FLAGS"]).HIP_FLAGS
    # the sums and the squares stay separate operations: 168 FIR additions + the pair sums, 28 squares per run
    assert len(re.findall(r"^\s*v_pk_add_f32", isa, flags=re.M)) >= 168 * kernels
    assert len(re.findall(r"^\s*v_pk_mul_f32", isa, flags=re.M)) >= 28 * kernels


def test_no_scratch_and_gfx950_only(isa):
    """No kernel of the library spills: 0 bytes of scratch each, at most 96 VGPRs (five waves per SIMD: scan_kernel.h kMinWaves)."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    # scan_kernel<true|false>, count_tries_kernel, report_kernel, copy_samples_kernel (the staging tail: round 6)
    assert len(sizes) == 5 and not any("pipe" in k for k in sizes) and any("copy_samples_kernel" in k for k in sizes)
    for name, size in sizes.items():
        assert int(size) == 0, f"{name} spills to scratch"
    for name, vgprs in re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", isa):
        assert int(vgprs) <= 96, (name, vgprs)
        # the try-count pass runs BESIDE the next scan: five scan waves of 96 VGPRs leave 32 of a SIMD's 512 free (round 6's
        # first four-words-per-lane version took 40 and did not fit: +36 % pass time, +3 % on the scan beside it)
        if "count_tries_kernel" in name:
            assert int(vgprs) <= 32, (name, vgprs)


def test_shipped_library_reads_no_environment():
    """Round 3 shipped its tuning laboratory (19 ADSB_* environment knobs, one of which switched an ordering rule off).
    The library in adsbdec_amd/lib carries no such name and does not import getenv; the kernel source has no build knob."""
    from adsbdec_amd import _build
    lib = _build.build()
    names = subprocess.run(["strings", lib], capture_output=True, text=True, check=True).stdout.splitlines()
    assert not [n for n in names if n.startswith("ADSB_")]
    dyn = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in dyn
    for f in ("scan_kernel.hip", "scan_kernel.h", "scan_tile.h"):
        src = open(os.path.join(ROOT, "adsbdec_amd", "csrc", f)).read()
        assert "#if" not in src.replace("#ifndef ADSBDEC", ""), f
    # The ONE knob the kernel source has lives in a header of its own: the per-phase tile clocks of a measurement build
    # (scan_stamps.h, -DADSB_PHASE_STAMPS, round 6).  The shipped build defines every macro of it empty and exports no reader.
    stamps = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "scan_stamps.h")).read()
    assert set(re.findall(r"#\s*if\w*\s+(\w+)", stamps)) == {"ADSB_PHASE_STAMPS"}
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "adsb_debug_phase_read" not in exported and "g_phase" not in exported


def test_atomic_optimizer_off_and_bitop3_gate(isa):
    """Two build properties the measured kernel time depends on: the compiler's atomic
    optimizer is off (it turns the survivor queue's per-lane LDS adds, which 13 % of the lanes execute, into a
    wave-wide DPP scan: +3.9 % kernel time), and the gate words are formed by gfx950's v_bitop3_b32."""
    from adsbdec_amd import _build
    assert "-amdgpu-atomic-optimizer-strategy=None" in _build.HIP_FLAGS
    assert len(re.findall(r"^\s*v_bitop3_b32", isa, flags=re.M)) >= 24   # 6 per chunk, 4 chunks per batch, two paths, two kernels
    assert re.search(r"^\s*ds_add_rtn_u32", isa, flags=re.M)


def test_host_side_is_built_for_avx2_and_the_refusal_is_not():
    """The host side of the decoder*.hip units (hand-off check, resolver, frame writer) is built with -mavx2 (adsbdec_amd/_build.py: 2 % of a
    call); the function that tells adsb_create whether the host can run that, and the rest of host_abi.cpp, are not."""
    from adsbdec_amd import _build, capi
    lib = _build.build()
    assert "-mavx2" in _build.HIP_FLAGS and _build.HIP_FLAGS[_build.HIP_FLAGS.index("-mavx2") - 1] == "-Xarch_host"
    dis = subprocess.run(["objdump", "-d", "--no-show-raw-insn", lib], capture_output=True, text=True, check=True).stdout
    assert "%ymm" in dis                                             # the flag reached the host compile
    body = dis.split("<adsb_host_cpu_refusal>:")[1].split("\n\n")[0]
    assert "ymm" not in body and "ret" in body                       # ... and not this function
    assert capi.load().adsb_host_cpu_refusal() is None               # (every host these tests run on has AVX2)
