"""Builds of the library with ONE comparison or constant of adsb::count_tries_kernel changed, for the question "would
tests/test_gpu_try_count.py notice?" (profiles/r21_try_count_tests.txt).  Each build goes to adsbdec_amd/lib_ab/ (git-ignored) and
is loaded through ADSB_LIB_PATH; nothing here is part of the library or of the suite.

    python -m adsbdec_amd._build                 # the objects the mutants are linked with
    python tools/try_count_mutants.py [name ...]
    ADSB_LIB_PATH=$PWD/adsbdec_amd/lib_ab/libadsbdec_m1_w_le_64.so python -m pytest -m gpu tests/test_gpu_try_count.py

A mutation changes a comparison or a constant, never an address or the bound of a loop over memory: every build reads and writes
what the shipped kernel reads and writes."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd import _build as B  # noqa: E402

KEY = "t0 >= (uint64_t)(ADSB_DECOFFSET_K - 1) ? t0 - (ADSB_DECOFFSET_K - 1) : 0;"
# name: (text of scan_kernel.hip, its replacement, occurrences)
MUTANTS = {
    "m1_w_le_64": ("const bool fits = w < 64u ||", "const bool fits = w <= 64u ||", 1),
    "m2_gt_t1": ("a.frames[lo + 64u].g >= t1;", "a.frames[lo + 64u].g > t1;", 1),
    "m3_fj_le_rt": ("shadowed[u] |= fj < rt[u] &&", "shadowed[u] |= fj <= rt[u] &&", 1),
    "m4_rt_le_ej": ("&& rt[u] < ej;", "&& rt[u] <= ej;", 1),
    "m5_key_k": (KEY, "t0 >= (uint64_t)(ADSB_DECOFFSET_K) ? t0 - (ADSB_DECOFFSET_K) : 0;", 1),
    "m6_hi_rel_gt": ("if (live[u] && gr >= hi_rel) {", "if (live[u] && gr > hi_rel) {", 1),
    "m7_code_mod3": ("cnt[code < 3 ? code : 2]++;", "cnt[code % 3]++;", 2),
    "m8_key_k_minus_2": (KEY, "t0 >= (uint64_t)(ADSB_DECOFFSET_K - 2) ? t0 - (ADSB_DECOFFSET_K - 2) : 0;", 1),
    "m9_search_le_end": ("return lo > 0 && g < a.frames[lo - 1].g + a.frames[lo - 1].span;",
                         "return lo > 0 && g <= a.frames[lo - 1].g + a.frames[lo - 1].span;", 1),
    "m10_list_hi_gt": ("            if (g >= a.hi) {", "            if (g > a.hi) {", 1),
}
OUT = os.path.join(B.PKG, "lib_ab")


def build(name):
    old, new, count = MUTANTS[name]
    text = open(os.path.join(B.CSRC, "scan_kernel.hip")).read()
    assert text.count(old) == count, (name, text.count(old))
    with tempfile.TemporaryDirectory() as tmp:
        src, obj = os.path.join(tmp, "scan_kernel.hip"), os.path.join(tmp, "scan_kernel.hip.o")
        with open(src, "w") as f:
            f.write(text.replace(old, new))
        subprocess.run([B.HIPCC] + B.HIP_FLAGS + ["-I", B.CSRC, "-c", src, "-o", obj], check=True)
        objs = [obj if s == "scan_kernel.hip" else os.path.join(B.LIBDIR, s + ".o") for s in B.HIP_SOURCES]
        objs += [os.path.join(B.LIBDIR, s + ".o") for s in B.C_SOURCES + B.CXX_SOURCES]
        lib = os.path.join(OUT, f"libadsbdec_{name}.so")
        subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + ["-lm", "-lpthread"], check=True)
    return lib


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(4) as pool:
        for lib in pool.map(build, sys.argv[1:] or list(MUTANTS)):
            print(lib, flush=True)
