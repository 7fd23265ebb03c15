"""float32 power-sample streams without a GPU: the door at the reference's own boundary (adsbdec.h:5, deqframe(ampbuff, len)).
The uint16 fixtures are valid expectations through it -- the oracle's demodulator on the oracle's power samples reproduces the
committed records -- the stream rule for a trailing odd sample, the numpy statement of the input domain, the captures of
general floats the GPU tests use, the converter and the C host program's -w refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_cases, golden_records, load_golden, records

SCALES = (0.37, 0.0031, 17.3)          # arbitrary mantissas; 1234.567 would leave the domain (2.3e6 x 1234 > 2^29)
TINY = 1e-38                           # below the smallest normal binary32 number: every product is tiny or subnormal
_general = {}


def scaled(a, s):
    """fl(a s): one rounded binary32 multiplication per sample."""
    return (a * np.float32(s)).astype(np.float32)


def general_capture(n, seed=78):
    """Power samples of a complex capture full of frames: one every 1201 + k samples (k = 0 .. 28 in turn: every offset mod 28),
    DF17 / DF18 / DF11 in turn, amplitudes 300 .. 1500 in noise of sigma 4 -- the kind of test_gpu_iq.big_capture, at any length."""
    if (n, seed) not in _general:
        from adsbdec_amd.sample_formats import iq_power
        from tools import gen_signal as G
        rng = np.random.default_rng(seed)
        starts, s, k = [], 0, 0
        while s + 1201 + 28 < n - 1300:
            starts.append(s)
            s += 1201 + k % 29
            k += 1
        frames = [(st, G.make_frame((17, 18, 11)[i % 3], rng), float(rng.uniform(300, 1500)), float(rng.uniform(0, 2 * np.pi)))
                  for i, st in enumerate(starts)]
        _general[(n, seed)] = iq_power(G.iq_synth(n, frames, 4.0, seed))
    return _general[(n, seed)]


@pytest.mark.parametrize("name", golden_cases())
def test_uint16_fixtures_are_expectations_through_the_power_door(oracle, name):
    """demod_power(power(x)) is the committed record set and Try/Ok table of every uint16 fixture, and its power samples lie in
    the domain of the _power calls."""
    from adsbdec_amd.sample_formats import power_domain_ok
    x, rec = load_golden(name)
    a = oracle.power(x)
    assert power_domain_ok(a) and float(a.max()) < 3.0e7
    frames, stats = oracle.demod_power(a, df18=rec["df18"])
    assert records(frames) == golden_records(rec)
    assert stats == rec["stats"]


@pytest.mark.parametrize("name", golden_cases())
def test_a_trailing_odd_power_sample_changes_nothing(oracle, name):
    """Power samples enter in twos (air.c:94-99): the stream of an odd number of them decodes as the stream without the last."""
    x, rec = load_golden(name)
    a = oracle.power(x)
    assert len(a) % 2 == 0
    assert oracle.demod_power(a[:-1].copy(), df18=rec["df18"]) == oracle.demod_power(a[:-2].copy(), df18=rec["df18"])


def test_the_fixture_set_is_the_one_the_issue_counted():
    assert len(golden_cases()) == 8


def test_power_domain_ok():
    from adsbdec_amd.sample_formats import power_domain_ok
    f = lambda *v: np.array(v, dtype="<f4")
    good = f(0.0, 1.0, 2.9e7, 2.0 ** 29 * (1 - 2.0 ** -24), 1e-38, 1e-45)
    assert good[-1] > 0 and good[-2] < np.finfo(np.float32).tiny        # two subnormals
    assert power_domain_ok(good) and power_domain_ok(f())
    for bad in (-0.0, -1.0, -1e-45, np.nan, np.inf, -np.inf, 2.0 ** 29, 3e38):
        assert not power_domain_ok(np.concatenate([good, f(bad)])), bad
        assert not power_domain_ok(f(bad))
    nan_with_sign = np.array([0xFFC00000], dtype="<u4").view("<f4")
    assert not power_domain_ok(nan_with_sign)
    with pytest.raises(ValueError):
        power_domain_ok(np.zeros(4, np.float64))


def test_general_float_captures_decode_at_every_scale(oracle):
    """The 256 Ki capture of general floats: inside the domain at every scale of the GPU tests, at least 190 frames under the
    oracle at each of them, and none at 1e-38, where every sum truncates to 0."""
    from adsbdec_amd.sample_formats import power_domain_ok
    a = general_capture(1 << 18)
    assert power_domain_ok(a)
    for s in (1.0,) + SCALES:
        b = scaled(a, s)
        assert power_domain_ok(b), s
        assert len(np.unique(b.view(np.uint32) & 0xFF)) == 256 or s == 1.0     # general mantissas, not a grid
        frames, stats = oracle.demod_power(b, df18=True)
        assert len(frames) >= 190, (s, len(frames))
    assert not power_domain_ok(scaled(a, 1234.567))
    t = scaled(a, TINY)
    assert power_domain_ok(t) and 0 < float(t.max()) < 1e-30 and ((t > 0) & (t < np.finfo(np.float32).tiny)).sum() > 1000
    frames, stats = oracle.demod_power(t, df18=True)
    assert frames == [] and sum(stats["try"].values()) == 0


def test_converter_writes_the_power_file(tmp_path):
    from adsbdec_amd import sample_formats as S
    from test_iq_cpu import load_iq
    x, _ = load_iq("mixed_df_a")
    x.tofile(tmp_path / "a.s16iq")
    (tmp_path / "a.s16iq").open("ab").write(b"\x01\x02\x03")               # a partial sample at the end
    run = lambda *a, check=True: subprocess.run([sys.executable, "-m", "adsbdec_amd.sample_formats", *a], cwd=ROOT, capture_output=True,
                                                text=True, check=check)
    p = run("-t", "2", "--power", str(tmp_path / "a.s16iq"), str(tmp_path / "a.pw"))
    assert "3 trailing bytes" in p.stderr
    assert np.array_equal(np.fromfile(tmp_path / "a.pw", dtype="<f4"), S.iq_power(x))
    S.to_float32_iq(x).tofile(tmp_path / "a.f32iq")
    run("-t", "0", "--power", str(tmp_path / "a.f32iq"), str(tmp_path / "b.pw"))
    assert np.array_equal(np.fromfile(tmp_path / "b.pw", dtype="<f4"), S.iq_power(x))
    assert run("-t", "3", "--power", str(tmp_path / "a.s16iq"), str(tmp_path / "c.pw"), check=False).returncode == 2
    assert run("-t", "2", str(tmp_path / "a.s16iq"), str(tmp_path / "c.pw"), check=False).returncode == 2


def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_w_refusals_and_usage(capi, tmp_path):
    """-w with -q, -t, -p, -G or -B: exit 1 with a reason before any GPU call (the file does not even exist); the usage text names
    -w and the domain."""
    capi.load()
    for extra, word in ((["-q", "2"], "-q"), (["-t", "1"], "-t"), (["-p"], "-p"), (["-G", "2"], "-G")):
        p = _cli(capi, tmp_path, "-w", *extra, "-f", "nothing.pw")
        assert p.returncode == 1 and "-w is not supported with " + word + ": " in p.stderr and not p.stdout, (extra, p.stderr)
    p = _cli(capi, tmp_path, "-w", "-B", "list.txt")
    assert p.returncode == 1 and "-w is not supported with -B: " in p.stderr
    u = subprocess.run([capi.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert u.returncode == 1 and "[-w]" in u.stdout and "\t-w :" in u.stdout and "2^29" in u.stdout and "[-q type]" in u.stdout


def test_power_symbols_are_declared_and_bound(capi):
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    for name in ("adsb_push_power", "adsb_push_power_async", "adsb_push_device_power", "adsb_push_device_power_final",
                 "adsb_decode_device_power", "adsb_decode_batch_device_power", "adsb_decode_batch_host_power"):
        assert hasattr(L, name) and name + "(" in header, name
    for m in ("push_power", "decode_power", "push_device_power", "decode_device_power", "decode_batch_power", "decode_batch_device_power"):
        assert callable(getattr(capi.Decoder, m)), m
    assert "2^29" in header and "subnormals" in header
