"""Build driver: hipcc cross-compiles the gfx950 code object without a GPU.

    python -m adsbdec_amd._build            # build lib/libadsbdec_amd.so + the C CLI
    python -m adsbdec_amd._build --force

Outputs stay in-tree (adsbdec_amd/lib/), are git-ignored, and travel to the GPU
box with the gpurun snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libadsbdec_amd.so")
CLI = os.path.join(LIBDIR, "adsbdec_amd_cli")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROCM = os.environ.get("ROCM", "/opt/rocm")  # the HIP runtime's headers and library for the host program, as the Makefile's ROCM

HIP_SOURCES = ["scan_kernel.hip", "scan_batch_kernel.hip", "scan_iq_kernel.hip", "scan_iq8_kernel.hip", "scan_power_kernel.hip", "seam_kernel.hip", "decoder.hip", "decoder_collect.hip",
               "decoder_lifecycle.hip", "decoder_batch.hip", "decoder_shard.hip", "unpack12.hip", "unpack12_batch.hip",
               "convert_samples.hip", "power_export_kernel.hip", "decoder_export.hip",
               "power_export_batch_kernel.hip", "decoder_export_batch.hip", "level_kernel.hip", "decoder_level.hip",
               "level_batch_kernel.hip", "decoder_level_batch.hip", "level_windows_kernel.hip", "decoder_level_windows.hip", "decoder_stage.hip", "decoder_flavour.hip",
               "burst_kernel.hip", "burst_slice_kernel.hip", "decoder_bursts.hip", "gather_kernel.hip", "decoder_gather.hip",
               "gather_pack12_kernel.hip", "decoder_gather_pack12.hip"]
C_SOURCES = ["format.c"]
# host-only C++ (no HIP): the multi-GPU driver over the C-ABI, and the part of the C-ABI that needs no device
CXX_SOURCES = ["multi.cpp", "host_abi.cpp", "numa.cpp"]
# the host program (csrc/cli/): one gcc line over all of them; it is rebuilt when any of them or any header beside them changes
CLI_DIR = os.path.join(CSRC, "cli")
CLI_SOURCES = ["adsbdec_amd_cli.c", "options.c", "common.c", "stream.c", "batch.c", "export.c", "level.c", "bursts.c", "record.c", "sink.c", "burst_archive.c"]
# What an object depends on is what the compiler says it read: every compile writes <object>.d (-MMD) and the next build
# reads it.  (Until round 6 this was a hand-kept list of headers, and gang.hpp -- included by resolver.hpp -- was not on
# it: editing it alone left stale objects.  tests/test_host_logic.py touches a header and watches the rebuild.)
# -ffp-contract=off: the reference arithmetic is binary32 multiply THEN add
# (SURVEY Q3); a fused multiply-add would change rounding.
# -amdgpu-atomic-optimizer-strategy=None: the compiler otherwise turns the survivor queue's per-lane LDS
# atomicAdd(qcount, n) into a scalar loop over the active lanes (readlane / writelane prefix sum, one iteration per
# lane) -- a fine trade for contended global atomics, a bad one for an LDS counter: kernel -3.9 % without it.
# -Xarch_host -mavx2: the HOST side of decoder.hip and the units beside it (the hand-off stream's check, the resolver's two loops, the frame writer) is
# what a call of the benchmark capture ends on; with 256-bit moves it is 2 % shorter (adsb_decode_device 0.1544 -> 0.1510 ms,
# profiles/r6_ab_runs.txt section 15; BMI / POPCNT alone: nothing).  Every x86-64 host an MI355X ships in has AVX2; one that has
# not is refused by adsb_create with a message (host_abi.cpp adsb_host_cpu_refusal, built without the flag).
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wall",
             "-Wno-unused-function", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-Xarch_host", "-mavx2"]


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any((not os.path.exists(d)) or os.path.getmtime(d) > t for d in deps)


def _recorded_deps(obj: str) -> list[str] | None:
    """The files the compiler read for `obj` last time (its -MMD depfile), or None when there is no record."""
    path = obj + ".d"
    if not os.path.exists(path):
        return None
    with open(path) as f:
        text = f.read().replace("\\\n", " ")
    _, _, rest = text.partition(":")
    return [os.path.normpath(w) for w in rest.split()]


def _stale(obj: str, src: str) -> bool:
    deps = _recorded_deps(obj)
    # An object compiled in another copy of the tree (a checkout moved or copied together with its lib/) records that copy's
    # files: their times say nothing about this tree's sources, so it is rebuilt.  (-MMD leaves system headers out: every
    # file a compile here reads lies under ROOT.)
    return deps is None or any(not d.startswith(ROOT + os.sep) for d in deps) or _newer(obj, [src] + deps)


def _run(cmd: list[str]) -> None:
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + p.stdout + p.stderr)
        raise RuntimeError(f"build step failed: {cmd[0]} ... {cmd[-1]}")


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    objs = []
    for s in HIP_SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s + ".o")
        if force or _stale(obj, src):
            if verbose:
                print("hipcc", s)
            _run([HIPCC] + HIP_FLAGS + os.environ.get("ADSB_EXTRA_HIPFLAGS", "").split() + ["-MMD", "-MF", obj + ".d", "-c", src, "-o", obj])
        objs.append(obj)
    for s in C_SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s + ".o")
        if force or _stale(obj, src):
            _run(["gcc", "-O2", "-fPIC", "-Wall", "-MMD", "-MF", obj + ".d", "-c", src, "-o", obj])
        objs.append(obj)
    for s in CXX_SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s + ".o")
        if force or _stale(obj, src):
            if verbose:
                print("g++", s)
            _run(["g++", "-O2", "-fPIC", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-MMD", "-MF", obj + ".d", "-c", src, "-o", obj])
        objs.append(obj)
    if force or _newer(LIB, objs):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lm", "-lpthread"])
    cli_srcs = [os.path.join(CLI_DIR, s) for s in CLI_SOURCES]
    cli_headers = [os.path.join(CLI_DIR, h) for h in sorted(os.listdir(CLI_DIR)) if h.endswith(".h")] if os.path.isdir(CLI_DIR) else []
    if cli_headers and (force or _newer(CLI, cli_srcs + cli_headers + [LIB, os.path.join(ROOT, "include", "adsbdec_amd.h")])):
        _run(cli_command(CLI, cli_srcs))
    return LIB


def cli_command(out: str, srcs: list[str], extra: list[str] | None = None) -> list[str]:
    """The one gcc line of the host program: `srcs` against this tree's library and public header.
    (The HIP runtime's C API: the device buffers of the program's own that -W -q, -L and -K | -P work through.)"""
    return (["gcc", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__"] + (extra or []) + ["-o", out] + srcs +
            ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROCM, "include"), "-L", LIBDIR, "-ladsbdec_amd",
             "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-lpthread", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(ROCM, "lib")])


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
