"""Complex int8 (IQ) captures without a GPU -- fmt 8 of the _iq calls: adsb_iq_bytes and the enum, the header's scalar power
function against numpy for every (I, Q), the numpy definitions and the converter, the committed fixtures against the oracle, the
new kernel unit's gfx950 resource report, the C host program's -q 8 refusals, and what the GPU module's captures are for."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import iq8_cases as Q
from conftest import ROOT

INT8_IQ, S16_IQ, F32_IQ = 8, 2, 0


# ------------------------------------------------------------------ 1. symbols and enum
def test_iq_bytes_enum_and_exports(capi, tmp_path):
    L = capi.load()
    assert L.adsb_iq_bytes(INT8_IQ, 3) == 6 and L.adsb_iq_bytes(INT8_IQ, 0) == 0
    assert [L.adsb_iq_bytes(f, 3) for f in (0, 2)] == [24, 12]
    assert [L.adsb_iq_bytes(f, 3) for f in (1, 3, 4, 5, 7, -1)] == [0] * 6           # the pinned zeros
    assert L.adsb_format_bytes(INT8_IQ, 3) == 0                                      # the _as family has no IQ format
    assert L.adsb_abi_version() == 5
    assert capi.FMT_INT8_IQ == 8 and capi.IQ_DTYPES[8] == np.dtype(np.int8)
    from adsbdec_amd import _build
    src = tmp_path / "m.c"
    src.write_text('#include "adsbdec_amd.h"\n#include <stdio.h>\nint main(void) { printf("%zu %d\\n", adsb_iq_bytes(ADSB_FMT_INT8_IQ, 3), '
                   'ADSB_FMT_INT8_IQ); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "m"),
                    "-L", _build.LIBDIR, "-ladsbdec_amd", "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(tmp_path / "m")], capture_output=True, text=True).stdout.split() == ["6", "8"]
    # fmt 8 goes through the existing _iq entry points: nothing is exported beyond the headers' declarations
    declared = set()
    for h in ("adsbdec_amd.h", "adsbdec_amd_diag.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        declared |= set(re.findall(r"\b(adsb_[a-z0-9_]+)\s*\(", text))
    declared -= {"adsb_get_profile", "adsb_multi_worker_profile"}
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    assert declared == set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    assert "scan_iq8_kernel.hip" in _build.HIP_SOURCES


# ------------------------------------------------------------------ 2. the header's scalar power function
def test_iq8_power_of_every_sample_equals_numpy(tmp_path):
    """sample_format.h's iq8_power -- what pw_at_iq8 runs on the device -- compiled into a host program of its own: all 65 536
    (I, Q) pairs against 256 (I^2 + Q^2) and against the widened twin's iq_power."""
    from adsbdec_amd.sample_formats import iq_power
    src = tmp_path / "p.cpp"
    src.write_text('#include "sample_format.h"\n#include <stdio.h>\nint main() { for (uint32_t d = 0; d < 65536; d++) { float a = adsb::iq8_power(d); '
                   'uint32_t b; __builtin_memcpy(&b, &a, 4); fwrite(&b, 4, 1, stdout); } return 0; }\n')
    exe = tmp_path / "p"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "adsbdec_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    got = np.frombuffer(subprocess.run([str(exe)], capture_output=True, check=True).stdout, dtype="<u4")
    d = np.arange(65536, dtype=np.uint32)
    x8 = np.stack([(d & 0xFF).astype(np.uint8).view(np.int8), (d >> 8).astype(np.uint8).view(np.int8)], axis=1)   # I is the low byte
    w = x8.astype(np.int64)
    want = (256 * (w[:, 0] ** 2 + w[:, 1] ** 2))
    assert int(want.max()) == 1 << 23
    assert np.array_equal(got, want.astype(np.float32).view("<u4"))
    assert np.array_equal(got, iq_power(Q.twin(x8), S16_IQ).view("<u4"))


# ------------------------------------------------------------------ 3. sample_formats, the fixtures, the digests
def test_numpy_definitions():
    from adsbdec_amd import sample_formats as S
    rng = np.random.default_rng(81)
    x8 = rng.integers(-128, 128, size=(50_000, 2), dtype=np.int8)
    x8[:3] = [[-128, -128], [127, -128], [0, 0]]
    w = x8.astype(np.int64)
    a = S.iq_power(x8, INT8_IQ)
    assert a.dtype == np.float32 and np.array_equal(a, S.iq_power(S.widen_int8_iq(x8), S16_IQ))
    assert np.array_equal(a.astype(np.int64), 256 * (w[:, 0] ** 2 + w[:, 1] ** 2)) and a[0] == 2.0 ** 23
    assert S.widen_int8_iq(x8).dtype == np.dtype("<i2") and np.array_equal(S.widen_int8_iq(x8).astype(np.int64), w * 256)
    back, lost = S.to_int8_iq(S.widen_int8_iq(x8))
    assert back.dtype == np.int8 and np.array_equal(back, x8) and lost == 0
    x16 = rng.integers(-32768, 32768, size=(50_000, 2), dtype=np.int16)
    q, lost = S.to_int8_iq(x16)
    assert np.array_equal(q.astype(np.int64), np.floor_divide(x16.astype(np.int64), 256))      # an arithmetic shift: towards -inf
    assert lost == int(np.count_nonzero(x16.astype(np.int64) % 256))
    assert S.INT8_IQ == 8 and S.IQ_DTYPES[8] == np.dtype(np.int8)
    with pytest.raises(ValueError):
        S.iq_power(x8, 7)


def test_converter_round_trips(tmp_path):
    from adsbdec_amd import sample_formats as S
    sys.path.insert(0, ROOT)
    from tools import gen_signal as G
    x16 = G.make_iq_workload(20_000, seed=4)[0]
    x16.tofile(tmp_path / "a.s16iq")
    (tmp_path / "a.s16iq").open("ab").write(b"\x01\x02\x03")               # a partial sample at the end
    run = lambda *a, check=True: subprocess.run([sys.executable, "-m", "adsbdec_amd.sample_formats", *a], cwd=ROOT, capture_output=True, text=True,
                                                check=check)
    p = run("-t", "8", str(tmp_path / "a.s16iq"), str(tmp_path / "a.cs8"))
    q, lost = S.to_int8_iq(x16)
    assert "3 trailing bytes" in p.stderr and f"{lost} of {x16.size} scalars are not on the int8 grid" in p.stderr and lost > 0
    got = np.fromfile(tmp_path / "a.cs8", dtype=np.int8).reshape(-1, 2)
    assert np.array_equal(got, q)
    p = run("-t", "8", "--back", str(tmp_path / "a.cs8"), str(tmp_path / "b.s16iq"))
    w = np.fromfile(tmp_path / "b.s16iq", dtype="<i2").reshape(-1, 2)
    assert p.stderr == "" and np.array_equal(w, S.widen_int8_iq(q))
    p = run("-t", "8", str(tmp_path / "b.s16iq"), str(tmp_path / "c.cs8"))                     # the twin is on the grid: nothing lost
    assert p.stderr == "" and np.array_equal(np.fromfile(tmp_path / "c.cs8", dtype=np.int8).reshape(-1, 2), q)
    run("-t", "8", "--power", str(tmp_path / "a.cs8"), str(tmp_path / "a.pw"))
    assert np.array_equal(np.fromfile(tmp_path / "a.pw", dtype="<f4"), S.iq_power(q, INT8_IQ))
    assert run("-t", "8", "--power", "--back", str(tmp_path / "a.cs8"), str(tmp_path / "d.pw"), check=False).returncode == 2
    assert run("-t", "9", str(tmp_path / "a.cs8"), str(tmp_path / "d.pw"), check=False).returncode == 2


def test_the_fixture_set_is_the_one_the_tests_expect():
    from adsbdec_amd.sample_formats import iq_power
    assert Q.iq8_fixtures() == Q.FIXTURES
    for f in os.listdir(Q.IQ8_DIR):
        assert os.path.getsize(os.path.join(Q.IQ8_DIR, f)) <= 400_000, f
    for name in Q.FIXTURES:
        assert len(Q.load_iq8(name)[0]) <= 120_000
    full, rec = Q.load_iq8("full_scale")
    assert int(full.min()) == -128 and max(f["pw"] for f in rec["frames"]) == 1 << 23 and len(rec["frames"]) == 8
    x, rec = Q.load_iq8("ragged")
    assert len(x) % 2 == 1 and len(x) > 40_980 and 0 < len(rec["frames"]) < 6            # six planted: the horizon cuts the rest
    assert len(Q.load_iq8("too_short")[0]) == 40_978 and not Q.load_iq8("too_short")[1]["frames"]
    x, rec = Q.load_iq8("noise")
    assert not rec["frames"] and sum(rec["stats"]["try"].values()) > 100 and int(np.abs(x.astype(np.int16)).max()) > 60
    # the quantised workload: ordinary input whose noise falls below one int8 step, so the D plane's tie rule is exercised
    x, rec = Q.load_iq8("workload_a")
    a = iq_power(x, INT8_IQ)
    assert len(rec["frames"]) >= 8 and {len(f["frame"]) for f in rec["frames"]} == {14, 28}
    assert float(np.mean(a[:-5] == a[5:])) >= 0.2
    assert len(Q.load_iq8("workload_noa")[1]["frames"]) < len(rec["frames"])


@pytest.mark.parametrize("name", Q.FIXTURES)
def test_fixture_equals_the_oracle_on_iq_power(oracle, name):
    """Every record of a fixture is what the restatement of demod.c / valid.c gives on iq_power(x, 8) -- the widened twin's power
    samples -- and, where the compiled reference is at hand, what the reference's own demodulator prints for it."""
    from adsbdec_amd.sample_formats import iq_power
    x, rec = Q.load_iq8(name)
    a = iq_power(x, INT8_IQ)
    assert np.array_equal(a, iq_power(Q.twin(x), S16_IQ))
    frames, stats = oracle.demod_power(a, df18=rec["df18"])
    assert stats == rec["stats"]
    assert [(f["g"], f["ts"], f["pw"], f["frame"].hex().upper()) for f in frames] == [(f["g"], f["ts"], f["pw"], f["frame"]) for f in rec["frames"]]
    for f in rec["frames"]:
        fr = bytes.fromhex(f["frame"])
        assert oracle.formatpkt(fr, f["ts"], f["pw"], 0) == f["avr"].encode()
        assert oracle.formatpkt(fr, f["ts"], f["pw"], 1) == f["mlat"].encode()
        assert oracle.formatpkt(fr, f["ts"], f["pw"], 2) == bytes.fromhex(f["beast"])
    if oracle.ref_available():
        rf, rstats = oracle.ref_demod(a, df18=rec["df18"])
        assert rstats == rec["stats"]
        assert [(r["ts"], r["pw"], r["avr"].decode(), r["mlat"].decode(), r["beast"].hex().upper()) for r in rf] == \
            [(f["ts"], f["pw"], f["avr"], f["mlat"], f["beast"]) for f in rec["frames"]]


def test_generator_digests():
    sys.path.insert(0, ROOT)
    from tools.make_golden_iq8 import cases, generator_digests
    with open(os.path.join(Q.IQ8_DIR, "generator_digests.json")) as f:
        assert generator_digests() == json.load(f)
    for name, input_name, x, df18 in cases():                             # the committed inputs are what the generator makes today
        assert np.array_equal(x, Q.load_iq8(name)[0]) and Q.load_iq8(name)[1]["df18"] == df18, name
    x = Q.load_iq8("workload_a")[0]
    assert hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() == generator_digests()["to_int8_iq(make_iq_workload(100000, seed=2))"]


# ------------------------------------------------------------------ 4. the new unit's ISA
@pytest.fixture(scope="module")
def isa():
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "scan_iq8_kernel.hip")
    cmd = [_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def test_scan_iq8_kernel_resources_and_fused_operations(isa):
    """scan_iq8_kernel.hip by the rules tests/test_build_flags.py holds scan_kernel.hip to: gfx950 only, four kernels, no scratch,
    at most 96 VGPRs (five waves per SIMD), and no fused float operation but the plane arithmetic's sign tests by the literal 2.0
    -- the power samples are exact integers, formed without one."""
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa and len(re.findall(r"\.amdgcn_target", isa)) == 1
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 4 and sum("scan_iq8_kernel" in k for k in sizes) == 2 and sum("scan_iq8_batch_kernel" in k for k in sizes) == 2
    for name, size in sizes.items():
        assert int(size) == 0, f"{name} spills to scratch"
    vgprs = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", isa)
    assert len(vgprs) == 4
    for name, v in vgprs:
        assert int(v) <= 96, (name, v)
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|mac|mad|fmac|dot)\w*f(?:32|16)\w*.*)$", isa, flags=re.M)
    assert fused and {f.split()[0] for f in fused} <= {"v_fma_f32", "v_pk_fma_f32"}, sorted({f.split()[0] for f in fused})
    for ln in fused:
        assert re.search(r"\b2\.0\b", ln), ln
    assert len(fused) == (22 + 12) * 4                                     # the sign tests of test_build_flags.py, per kernel


# ------------------------------------------------------------------ 5. the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_q8_refusals_and_usage(capi, tmp_path):
    """-q 8 with -t, -p, -G, -B, -w or -W: the "-q N is not supported with X" message and status 1 before any GPU call (the file
    does not even exist); the usage text names -q 8; -t 8 and -t 9 stay refused."""
    capi.load()
    for extra, word in ((["-t", "3"], "-t"), (["-p"], "-p"), (["-G", "2"], "-G"), (["-w"], "-w"), (["-W", "out.pw"], "-W")):
        p = _cli(capi, tmp_path, "-q", "8", *extra, "-f", "nothing.cs8")
        assert p.returncode == 1 and "-q 8 is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
        assert not os.path.exists(tmp_path / "out.pw")
    p = _cli(capi, tmp_path, "-q", "8", "-B", "list.txt")
    assert p.returncode == 1 and "-q 8 is not supported with -B: " in p.stderr
    for bad in ("6", "9", "16"):
        p = _cli(capi, tmp_path, "-q", bad, "-f", "nothing.cs8")
        assert p.returncode == 1 and "not an IQ sample type" in p.stderr and "8 (int8 IQ)" in p.stderr, (bad, p.stderr)
    for t in ("8", "9"):
        p = _cli(capi, tmp_path, "-t", t, "-f", "nothing.cs8")
        assert p.returncode == 1 and "unknown sample type" in p.stderr, (t, p.stderr)
    u = subprocess.run([capi.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert u.returncode == 1 and "[-q type]" in u.stdout and "-q 8" in u.stdout and "signed 8 bits IQ" in u.stdout


# ------------------------------------------------------------------ 6. what the GPU module's captures are for
def test_the_captures_reach_what_they_are_for(capi):
    """From the oracle and the layout alone: the edge captures carry candidates at their first and last offsets (no FIR in front
    of this kernel: what a segment's clipping can spoil shows there), every kind keeps frames after the quantisation, the stream
    kinds overflow the shrunken lists of the forced-K cells, and the layout at units(n) is well-formed, cut and uncut."""
    import front_records_cases as F
    host = Q.cases()
    assert len(host) == 15 and {len(host[e].x) % 4 for e in Q.EDGES} == {0, 1, 2, 3}
    for e in Q.EDGES:
        c = host[e]
        gs = [r[0] for r in c.ev[True][0]]
        assert gs[:4] == [0, 1, 2, 3] and gs[-4:] == list(range(c.n_off - 4, c.n_off)), (e, gs[:6], gs[-6:], c.n_off)
    for name in Q.KINDS:
        c = host[name]
        assert c.x.dtype == np.int8 and c.n == Q.N and c.n_off == 129_877
        if name not in ("uniform", "noise"):
            assert len(c.dec[(True, False)][0]) >= 5, name
    assert len(host["damaged"].fixed) > 20
    assert int(host["uniform"].x.min()) == -128 and int(host["uniform"].x.max()) == 127
    for ci in range(len(Q.CONFIGS)):
        _, kw, limit = Q.CONFIGS[ci]
        if kw.get("debug_passes"):
            k, big = kw["debug_passes"], kw.get("debug_big_tiles", 0)
            staged = tried = 0
            for name in Q.STREAM_KINDS:
                c = host[name]
                g = np.array([r[0] for r in Q.full_list(c, kw)], dtype=np.int64)
                tg = (c.ev[kw["df18"]][1] >> np.uint64(2)).astype(np.int64)
                for t0, t1 in F.M.tile_bounds(0, c.n_off, k, big):
                    staged = max(staged, int(np.searchsorted(g, t1) - np.searchsorted(g, t0)))
                    tried = max(tried, int(np.searchsorted(tg, t1) - np.searchsorted(tg, t0)))
            if "debug_clist_cap" in kw:
                assert staged > kw["debug_clist_cap"], (Q.IDS[ci], staged)
            if "debug_queue_cap" in kw:
                assert tried > kw["debug_queue_cap"], (Q.IDS[ci], tried)
        if ci in Q.BATCH_CELLS:
            for cut in (False, True):
                order, ns, segs, launches = Q.layout(capi, ci, cut)
                assert len(order) == 15 and (not cut or len(launches) > 1), (Q.IDS[ci], cut, len(launches))
