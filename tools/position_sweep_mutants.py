"""Builds of the library with ONE value of scan_stages.h changed at ONE position of a scan tile, for the question "would
tests/test_gpu_position_sweep.py notice, and would the older offset-by-offset files?" (profiles/r22_position_sweep_tests.txt).
Each build goes to adsbdec_amd/lib_ab/ (git-ignored) and is loaded through ADSB_LIB_PATH; nothing here is part of the library
or of the suite.

    python -m adsbdec_amd._build                 # the objects the mutants are linked with
    python tools/position_sweep_mutants.py [name ...]
    ADSB_LIB_PATH=$PWD/adsbdec_amd/lib_ab/libadsbdec_p1_next_lane_slot.so python -m pytest -m gpu tests/test_gpu_position_sweep.py

A mutation changes a value that feeds the sign planes or a gate word, never an address, a loop bound or the set of offsets a
launch may evaluate beyond its own: every build reads and writes what the shipped kernels read and write."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd import _build as B  # noqa: E402

UNITS = ["scan_kernel.hip", "scan_batch_kernel.hip", "scan_iq_kernel.hip", "scan_iq8_kernel.hip", "scan_power_kernel.hip"]
NEXT = "            a[28 + k] = from_next_lane(a[k]);"
# name: (text of scan_stages.h, its replacement, occurrences of the text, the occurrence that is replaced or None: all)
MUTANTS = {
    # Stage A of the real-sample kernels: the last sample of the next lane that a plane bit depends on comes from the wrong slot
    # (a[42] feeds c[32] and so bit 27 of E1 and E2; slot 15, a[43], feeds c[33] only, which nothing reads)
    "p1_next_lane_slot": (NEXT, "            a[28 + k] = from_next_lane(a[k == 14 ? 13 : k]);", 4, 0),
    # ... lane 63's duplicate of the next wave's first run differs from the original in one sample
    "p2_lane63_duplicate": (NEXT, "            a[28 + k] = from_next_lane(lane == 63 && k == 3 ? 0.0f : a[k]);", 4, 0),
    # ... one bit of the E2 plane of the first run of the second pass (the seam between two passes)
    "p3_seam_run_e2_bit": ("            pl_e2[v] = e2;", "            pl_e2[v] = v == kWaveRuns * kWaves ? e2 & ~(1u << 5) : e2;", 4, 0),
    # Stage B, every front end: the ragged batch's mask loses the last offset that exists
    "p4_ragged_mask": ("nvalid > 0 ? (1u << nvalid) - 1u : 0u;", "nvalid > 0 ? (1u << (nvalid - 1)) - 1u : 0u;", 1, None),
    # ... the full batch of four chunks loses one offset of its last thread's last word (K >= 5 only: K = 2, 3 have no full batch)
    "p5_full_batch_bit": ("                gt[u] = gate, gb1[u] = b1, gb4[u] = b4;",
                          "                gt[u] = (decltype(is_full)::value && u == kGateBatch - 1 && tid == NT - 1) ? gate & ~(1u << 27) : gate, gb1[u] = b1, gb4[u] = b4;", 1, None),
}
OUT = os.path.join(B.PKG, "lib_ab")


def mutate(text, name):
    old, new, count, which = MUTANTS[name]
    assert text.count(old) == count, (name, text.count(old))
    if which is None:
        return text.replace(old, new)
    parts = text.split(old)
    return old.join(parts[:which + 1]) + new + old.join(parts[which + 1:])


def build(name):
    header = mutate(open(os.path.join(B.CSRC, "scan_stages.h")).read(), name)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "scan_stages.h"), "w") as f:       # (found first: the units lie beside it)
            f.write(header)
        objs = {}
        for unit in UNITS:
            src, objs[unit] = os.path.join(tmp, unit), os.path.join(tmp, unit + ".o")
            with open(src, "w") as f:
                f.write(open(os.path.join(B.CSRC, unit)).read())
            subprocess.run([B.HIPCC] + B.HIP_FLAGS + ["-I", B.CSRC, "-c", src, "-o", objs[unit]], check=True)
        link = [objs.get(s, os.path.join(B.LIBDIR, s + ".o")) for s in B.HIP_SOURCES]
        link += [os.path.join(B.LIBDIR, s + ".o") for s in B.C_SOURCES + B.CXX_SOURCES]
        lib = os.path.join(OUT, f"libadsbdec_{name}.so")
        subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + link + ["-lm", "-lpthread"], check=True)
    return lib


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(4) as pool:
        for lib in pool.map(build, sys.argv[1:] or list(MUTANTS)):
            print(lib, flush=True)
