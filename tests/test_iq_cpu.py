"""Complex (IQ) captures without a GPU: the committed fixtures against the oracle on the library's power-sample definition, the
float32 scalar function against numpy, adsb_iq_bytes, the generator's digests, the C host program's -q refusals and the converter."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

IQ_DIR = os.path.join(GOLDEN, "iq")
F32_IQ, S16_IQ = 0, 2


def iq_cases():
    return sorted(f[:-5] for f in os.listdir(IQ_DIR) if f.endswith(".json") and f != "generator_digests.json")


def load_iq(name):
    with open(os.path.join(IQ_DIR, name + ".json")) as f:
        rec = json.load(f)
    x = np.load(os.path.join(IQ_DIR, rec["input"]))["x"]
    assert x.dtype == np.int16 and x.shape == (rec["n_samples"], 2)
    rec["stats"] = {k: {int(d): v for d, v in rec["stats"][k].items()} for k in rec["stats"]}
    return x, rec


def edge_bits():
    """float32 bit patterns: +-Inf, NaNs, denormals, +-0.0, +-1, the ends of the int16 range, ties at 2^-16, and 10^6 random ones."""
    f = lambda v: np.array(v, dtype="<f4").view("<u4")
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x80000000,
                        0x00000000, 0x3F800000, 0xBF800000], dtype="<u4")
    near = f([32767 / 32768, 32767.5 / 32768, 32767.49 / 32768, -32768.5 / 32768, -32768.51 / 32768, -1.0 - 2.0 ** -16,
              2.0 ** -16, 3 * 2.0 ** -16, -2.0 ** -16, 2.0 ** -17, 2.0 ** -15, 5 * 2.0 ** -16, 0.5, 0.25 + 2.0 ** -16, 1e-30, 3e38, -3e38])
    rng = np.random.default_rng(20)
    rnd = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype("<u4")
    grid = (rng.integers(-32768, 32768, 4096).astype(np.float32) / np.float32(32768)).view("<u4")
    half = ((rng.integers(-32768, 32767, 4096).astype(np.float64) + 0.5) / 32768).astype("<f4").view("<u4")   # exact ties
    return np.concatenate([special, near, grid, half, rnd])


def test_the_fixture_set_is_the_one_the_tests_expect():
    assert iq_cases() == ["full_scale", "mixed_df_a", "mixed_df_noa", "ragged", "ties_noise", "too_short", "wide_noise"]
    for f in os.listdir(IQ_DIR):
        assert os.path.getsize(os.path.join(IQ_DIR, f)) < 600_000, f
    full, rec = load_iq("full_scale")
    assert int(full.min()) == -32768 and max(f["pw"] for f in rec["frames"]) > 4_000_000
    assert len(load_iq("too_short")[0]) == 40978 and not load_iq("too_short")[1]["frames"]
    assert len(load_iq("ragged")[0]) % 2 == 1
    x, rec = load_iq("ties_noise")
    from adsbdec_amd.sample_formats import iq_power
    a = iq_power(x)
    assert 0.15 < float(np.mean(a[:-5] == a[5:])) < 0.35 and sum(rec["stats"]["try"].values()) > 100
    assert 25 <= len(load_iq("mixed_df_a")[1]["frames"]) <= 35 and {len(f["frame"]) for f in load_iq("mixed_df_a")[1]["frames"]} == {14, 28}


@pytest.mark.parametrize("name", iq_cases())
def test_fixture_equals_the_oracle_on_iq_power(oracle, name):
    """Every record of a fixture is what the restatement of demod.c / valid.c gives on iq_power(x), and -- where the compiled
    reference is at hand -- what the reference's own demodulator prints for it, byte for byte in the three framings."""
    from adsbdec_amd.sample_formats import iq_power, to_float32_iq
    x, rec = load_iq(name)
    a = iq_power(x)
    assert np.array_equal(a, iq_power(to_float32_iq(x), F32_IQ))          # the float twin is exact
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


def test_iq_power_is_strict_binary32():
    """iq_power against exact integer arithmetic rounded once per operation: products of int16 fit 31 bits, so the two rounded
    products and the rounded sum can be restated with Python integers and float32 conversions."""
    from adsbdec_amd.sample_formats import iq_power
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, size=(20000, 2), dtype=np.int64)
    x[:4] = [[-32768, -32768], [32767, -32768], [0, 0], [-1, 1]]
    ii = (x[:, 0] * x[:, 0]).astype(np.float64).astype(np.float32)   # fl(I^2): int64 -> binary64 is exact, -> binary32 rounds once
    qq = (x[:, 1] * x[:, 1]).astype(np.float64).astype(np.float32)
    want = ((ii.astype(np.float64) + qq.astype(np.float64)).astype(np.float32) * np.float32(2.0 ** -8))
    assert np.array_equal(iq_power(x.astype(np.int16)), want)
    assert iq_power(x[:1].astype(np.int16))[0] == 2.0 ** 23


def test_float32_iq_code_equals_numpy(tmp_path):
    from adsbdec_amd.sample_formats import flags_float32_iq
    exe = tmp_path / "sample_formats_iq"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "sample_formats_iq.cpp"), "-o", str(exe)],
                   check=True)
    bits = edge_bits()
    bits.tofile(tmp_path / "in.bin")
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", dtype="<u2").reshape(-1, 2)
    r, inexact, clamped = flags_float32_iq(bits.view("<f4"))
    assert np.array_equal(got[:, 0].view(np.int16), r)
    assert np.array_equal(got[:, 1], np.where(clamped, 2, np.where(inexact, 1, 0)))
    assert inexact.sum() > 1000 and clamped.sum() > 1000 and (~inexact & ~clamped).sum() > 4096
    # the named cases: NaN -> 0 clamped, +-Inf clamped to the ends, denormals inexact 0, -0.0 exact, +1 clamped to 32767, -1 exact
    named = {0x7FC00000: (0, 2), 0x7F800000: (32767, 2), 0xFF800000: (-32768, 2), 0x00000001: (0, 1), 0x807FFFFF: (0, 1),
             0x80000000: (0, 0), 0x3F800000: (32767, 2), 0xBF800000: (-32768, 0)}
    for b, (code, what) in named.items():
        i = int(np.nonzero(bits == b)[0][0])
        assert (int(got[i, 0].view(np.int16) if hasattr(got[i, 0], "view") else got[i, 0]), int(got[i, 1])) == (code, what), hex(b)
    # ties at 2^-16 go to the even neighbour
    t = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768], dtype="<f4")
    assert flags_float32_iq(t)[0].tolist() == [0, 2, 2, 0, -2] and flags_float32_iq(t)[1].all()


def test_iq_bytes_from_python_and_from_c99(capi, tmp_path):
    L = capi.load()
    assert [L.adsb_iq_bytes(f, 3) for f in (0, 2)] == [24, 12]
    assert [L.adsb_iq_bytes(f, 3) for f in (1, 3, 4, 5, 7, -1)] == [0] * 6
    assert L.adsb_iq_bytes(2, 0) == 0
    assert [L.adsb_format_bytes(f, 3) for f in (0, 2)] == [0, 0]          # the _as family still has no IQ format
    assert L.adsb_abi_version() == 5
    from adsbdec_amd import _build
    src = tmp_path / "m.c"
    src.write_text('#include "adsbdec_amd.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %d %d\\n", adsb_iq_bytes(ADSB_FMT_FLOAT32_IQ, 3), '
                   'adsb_iq_bytes(ADSB_FMT_INT16_IQ, 3), adsb_iq_bytes(ADSB_FMT_INT16_REAL, 3), ADSB_FMT_FLOAT32_IQ, ADSB_FMT_INT16_IQ); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "m"),
                    "-L", _build.LIBDIR, "-ladsbdec_amd", "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(tmp_path / "m")], capture_output=True, text=True).stdout.split() == ["24", "12", "0", "0", "2"]


def test_iq_generator_digests():
    sys.path.insert(0, ROOT)
    from tools import gen_signal as G
    from tools.make_golden_iq import generator_digests
    with open(os.path.join(IQ_DIR, "generator_digests.json")) as f:
        assert generator_digests() == json.load(f)
    x, truth = G.make_iq_workload(100_000, seed=2)
    assert x.dtype == np.int16 and x.shape == (100_000, 2) and len(truth) == 10
    assert len(np.unique(x & 15)) == 16 and {len(fr) for _, fr in truth} <= {7, 14}     # all 16 bits in use
    with open(os.path.join(GOLDEN, "generator_digests.json")) as f:                      # the uint16 generators are where they were
        assert "make_workload" in f.read()


def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_q_refusals_and_usage(capi, tmp_path):
    """-q with -t, -p, -G or -B, or with a number that is no IQ type: a message and status 1 before any GPU call (the file does not
    even exist); -t 0 | 2 keeps its refusal; the usage text names -q."""
    capi.load()
    for extra, word in ((["-t", "3"], "-t"), (["-p"], "-p"), (["-G", "2"], "-G")):
        p = _cli(capi, tmp_path, "-q", "2", *extra, "-f", "nothing.iq")
        assert p.returncode == 1 and "-q 2 is not supported with " + word in p.stderr and not p.stdout, (extra, p.stderr)
    p = _cli(capi, tmp_path, "-q", "0", "-B", "list.txt")
    assert p.returncode == 1 and "-q 0 is not supported with -B" in p.stderr
    for bad in ("1", "3", "4", "5", "7", "x", "-1"):
        p = _cli(capi, tmp_path, "-q", bad, "-f", "nothing.iq")
        assert p.returncode == 1 and "not an IQ sample type" in p.stderr, (bad, p.stderr)
    for t in ("0", "2"):
        p = _cli(capi, tmp_path, "-t", t, "-f", "nothing.iq")
        assert p.returncode == 1 and "IQ" in p.stderr and "raw twin" in p.stderr
    u = subprocess.run([capi.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert u.returncode == 1 and "[-q type]" in u.stdout and "\t-q type :" in u.stdout and "[-t type]" in u.stdout and "\t-t type :" in u.stdout


def test_converter_round_trips(tmp_path):
    from adsbdec_amd import sample_formats as S
    x, _ = load_iq("mixed_df_a")
    assert np.array_equal(S.to_int16_iq(S.to_float32_iq(x))[0], x) and S.to_int16_iq(S.to_float32_iq(x))[1:] == (0, 0)
    x.tofile(tmp_path / "a.s16iq")
    (tmp_path / "a.s16iq").open("ab").write(b"\x01\x02\x03")               # a partial sample at the end
    run = lambda *a: subprocess.run([sys.executable, "-m", "adsbdec_amd.sample_formats", *a], cwd=ROOT, capture_output=True, text=True, check=True)
    p = run("-t", "0", str(tmp_path / "a.s16iq"), str(tmp_path / "a.f32iq"))
    assert "3 trailing bytes" in p.stderr
    f = np.fromfile(tmp_path / "a.f32iq", dtype="<f4")
    assert f.size == x.size and np.abs(f).max() < 1.0
    p = run("-t", "0", "--back", str(tmp_path / "a.f32iq"), str(tmp_path / "b.s16iq"))
    assert p.stderr == "" and np.array_equal(np.fromfile(tmp_path / "b.s16iq", dtype="<i2").reshape(-1, 2), x)
    (f + np.float32(1e-6)).astype("<f4").tofile(tmp_path / "off.f32iq")
    p = run("-t", "0", "--back", str(tmp_path / "off.f32iq"), str(tmp_path / "c.s16iq"))
    assert "not on the int16 grid" in p.stderr
    with pytest.raises(ValueError):
        S.iq_power(x, 3)
