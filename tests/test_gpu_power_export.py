"""The power export on the MI355X (run with -m gpu): power_export_kernel / iq_power_export_kernel and every adsb_power_* call, held
bit for bit (floats compared as uint32) to oracle.power -- the restatement of air.c:54-91 that tests/test_oracle_vs_ref.py holds to the
reference's decodeiq -- and to sample_formats.iq_power: the committed fixtures, every length around a run, a wave and a block on
full-range codes, windows of a stream with and without overlap, the round trip through decode_device_power without leaving HBM, the
converted and packed twins, a stream in progress beside it, the refusals, and the C host program's -W."""
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records
from test_gpu_iq import to_dev
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)
from test_iq_cpu import iq_cases, load_iq

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF          # a NaN no power sample is: what an unwritten float of `out` holds
GUARD = 64
N_WIN = 1 << 16


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev_out(torch, n_floats, lead=0):
    """n_floats + GUARD sentinels on the device: (tensor, pointer)."""
    return to_dev(torch, np.full(n_floats + GUARD, SENT, np.uint32), lead=lead)


def read_out(t, lead=0):
    return t.cpu().numpy()[lead:].view(np.uint32)


def check_out(t, want, how):
    """The first len(want) floats are `want` bit for bit, and everything behind them -- the guard included -- is untouched."""
    got = read_out(t)
    k = len(want)
    assert np.array_equal(got[:k], bits(want)), (how, np.flatnonzero(got[:k] != bits(want))[:8])
    assert (got[k:] == SENT).all(), how


_full = {}


def full_range(oracle):
    """Seeded full-range uint16 codes (0 .. 65535), 65 539 of them, and the oracle's power samples of the whole."""
    if not _full:
        x = np.random.default_rng(355).integers(0, 65536, N_WIN + 3, dtype=np.uint16)
        _full["x"], _full["a"] = x, oracle.power(x)
        _full["a64"] = oracle.power(x[:N_WIN].copy())
    return _full


# ------------------------------------------------------------------ 1. the fixtures
@pytest.mark.limit(60)
@pytest.mark.parametrize("name", golden_cases())
def test_uint16_fixtures(capi, oracle, dec_factory, torch_cuda, name):
    x, rec = load_golden(name)
    n, k = x.size, 2 * (x.size // 4)
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, k)
    assert d.power_device(ptr, n, po, k) == k
    check_out(to, oracle.power(x)[:k], name)


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (2, 0))
@pytest.mark.parametrize("name", iq_cases())
def test_iq_fixtures(capi, dec_factory, torch_cuda, name, fmt):
    x, rec = load_iq(name)
    n = len(x)
    d = dec_factory()
    d.reset()
    t, ptr = to_dev(torch_cuda, x if fmt == 2 else S().to_float32_iq(x))
    to, po = dev_out(torch_cuda, n)
    assert d.power_device_iq(fmt, ptr, n, po, n) == n
    check_out(to, S().iq_power(x), (name, fmt))
    assert d.format_report() == ((2 * n, 0, 0) if fmt == 0 else (0, 0, 0))


# ------------------------------------------------------------------ 2. lengths and edges
LENGTHS = (list(range(0, 9)) + list(range(24, 33)) + list(range(52, 61)) + list(range(3580, 3589)) + list(range(14332, 14341))
           + [N_WIN, N_WIN + 3])


@pytest.mark.limit(120)
def test_lengths_and_edges(capi, oracle, dec_factory, torch_cuda):
    """Full-range codes; every n around nothing, half a run, a run (56 samples), a wave (3584) and a block's pass (14 336), and two at
    which the typed-load path and the plain-load path both run: the oracle's prefix, 2 (n // 4) floats and not one more."""
    f = full_range(oracle)
    x, a = f["x"], f["a"]
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    for n in LENGTHS:
        k = 2 * (n // 4)
        to, po = dev_out(torch_cuda, k)
        assert d.power_device(ptr, n, po, k) == k, n
        check_out(to, a[:k], n)


# ------------------------------------------------------------------ 3. windows
def walk(rng_seed=28):
    """(m_begin, m_end) of a walk over [0, 32768) in windows of 28 k power samples: k below a wave (64 runs), below a block (256) and
    of several blocks, a seeded list beside the sizes next to those thresholds.  The last window ends ragged, at 32768."""
    rng = np.random.default_rng(rng_seed)
    small, mid = [int(v) for v in rng.integers(1, 64, 3)], [int(v) for v in rng.integers(66, 255, 2)]
    ks = [1, 63, 257, 64, small[0], 65, mid[0], small[1], 300, 255, mid[1], small[2], 256]
    out, m, i = [], 0, 0
    while m < N_WIN // 2:
        e = min(m + 28 * ks[i % len(ks)], N_WIN // 2)
        out.append((m, e))
        m, i = e, i + 1
    sizes = [(e - b) // 28 for b, e in out]
    assert min(sizes) < 64 and [k for k in sizes if 64 <= k < 256] and max(sizes) > 256 and out[-1][1] % 28 != 0
    return out


@pytest.mark.limit(120)
def test_windows_with_overlap_concatenate_to_the_stream(capi, oracle, dec_factory, torch_cuda):
    f = full_range(oracle)
    x, a = f["x"][:N_WIN], f["a64"]
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    pieces, pieces_host = [], []
    for i, (mb, me) in enumerate(walk()):
        first = max(0, 2 * mb - 16)
        to, po = dev_out(torch_cuda, me - mb)
        assert d.power_window(ptr + 2 * first, first, 2 * me - first, mb, me, po, me - mb) == me - mb
        check_out(to, a[mb:me], (mb, me))
        pieces.append(read_out(to)[: me - mb])
        if i % 3 == 0:
            pieces_host.append((mb, d.power_window_host(x[first: 2 * me], first, mb, me)))
    assert np.array_equal(np.concatenate(pieces), bits(a))
    for mb, p in pieces_host:
        assert np.array_equal(bits(p), bits(a[mb: mb + len(p)])), mb


@pytest.mark.limit(60)
def test_a_window_without_overlap_reads_silence(capi, oracle, dec_factory, torch_cuda):
    """The buffer starts exactly at 2 m_begin > 0: the first six samples are those of the capture with 0x800 in front of that point --
    and not the stream's --, everything behind them is the stream's.  Device call and host call."""
    f = full_range(oracle)
    x, a = f["x"][:N_WIN], f["a64"]
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    for mb, me in ((2800, 2800 + 28 * 5), (28 * 64 * 5, 28 * 64 * 5 + 28 * 300 + 11)):
        first = 2 * mb
        y = x.copy()
        y[:first] = 0x800
        want = oracle.power(y)[mb:me]
        assert np.array_equal(bits(want[6:]), bits(a[mb + 6: me])) and (bits(want[:6]) != bits(a[mb: mb + 6])).any()
        to, po = dev_out(torch_cuda, me - mb)
        assert d.power_window(ptr + 2 * first, first, N_WIN - first, mb, me, po, me - mb) == me - mb
        check_out(to, want, (mb, me))
        assert (read_out(to)[:6] != bits(a[mb: mb + 6])).any()
        got = d.power_window_host(x[first:], first, mb, me)
        assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ 4. the round trip
@pytest.mark.limit(60)
@pytest.mark.parametrize("name", golden_cases())
def test_round_trip_in_hbm(capi, oracle, dec_factory, torch_cuda, name):
    """Export, then decode_device_power on the exported device buffer: the fixture's committed records and Try/Ok table.  The float
    array is read back only to be held to the domain of the _power calls."""
    x, rec = load_golden(name)
    n, k = x.size, 2 * (x.size // 4)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, k)
    assert d.power_device(ptr, n, po, k) == k
    assert S().power_domain_ok(read_out(to)[:k].view("<f4"))
    assert records(d.decode_device_power(po, k)) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 5. formats
@pytest.mark.limit(60)
def test_converted_and_packed_twins_export_the_raw_samples(capi, oracle, dec_factory, torch_cuda):
    from adsbdec_amd.packed12 import pack12
    x, rec = load_golden("mixed_df_a_384Ki")
    n, k = x.size, 2 * (x.size // 4)
    want = oracle.power(x)[:k]
    d = dec_factory()
    d.reset()
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, k)
    assert d.power_device(ptr, n, po, k) == k
    check_out(to, want, "raw")
    for fmt, twin in ((3, S().to_int16_real(x)), (1, S().to_float32_real(x)), (4, x), (5, x)):
        tt, pt = to_dev(torch_cuda, twin)
        to, po = dev_out(torch_cuda, k)
        assert d.power_device_as(fmt, pt, n, po, k) == k
        check_out(to, want, fmt)
    assert d.format_report() == (2 * n, 0, 0)
    tp, pp = to_dev(torch_cuda, pack12(x))
    to, po = dev_out(torch_cuda, k)
    assert d.power_device_packed(pp, n, po, k) == k
    check_out(to, want, "packed")


# ------------------------------------------------------------------ 6. a stream in progress is not touched
@pytest.mark.limit(60)
def test_a_stream_in_progress_is_untouched(capi, oracle, dec_factory, torch_cuda):
    x, rec = load_golden("config1_1Mi_100xDF17")
    f = full_range(oracle)
    y, a = f["x"][:N_WIN], f["a64"]
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptr = to_dev(torch_cuda, y)
    d.reset()
    chunk = 100_003
    for i, lo in enumerate(range(0, x.size, chunk)):
        d.push(x[lo: lo + chunk])
        mb = 28 * 64 * i
        me = mb + 28 * 70 + 5
        first = max(0, 2 * mb - 16)
        to, po = dev_out(torch_cuda, me - mb)
        assert d.power_window(ptr + 2 * first, first, N_WIN - first, mb, me, po, me - mb) == me - mb
        check_out(to, a[mb:me], mb)
        assert np.array_equal(bits(d.power(y[:4096])), bits(a[:2048]))
    d.finish()
    assert records(d.drain()) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 7. refusals
@pytest.mark.limit(60)
def test_refusals_write_nothing(capi, oracle, dec_factory, torch_cuda):
    f = full_range(oracle)
    x = f["x"][:N_WIN]
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, 4096)
    W = lambda *a: (lambda: d.power_window(*a))
    top = 1 << 32
    mb_top = -(-(top // 2 - N_WIN // 2) // 28) * 28
    cases = [
        ("16-byte", W(ptr + 8, 0, N_WIN - 8, 0, 280, po, 4096)),                       # misaligned sample pointer
        ("16-byte", W(ptr, 0, N_WIN, 0, 280, po + 4, 4095)),                           # misaligned device_power
        ("multiple of 8", W(ptr + 8, 4, N_WIN - 4, 28, 280, po, 4096)),                # first_sample % 8
        ("multiple of 28", W(ptr, 0, N_WIN, 14, 280, po, 4096)),                       # m_begin % 28
        ("own pair", W(ptr, 0, 560, 0, 281, po, 4096)),                                # the window reaches behind the buffer
        ("own pair", W(ptr + 1024, 512, N_WIN - 512, 252, 560, po, 4096)),             # ... in front of it (2 x 252 < 512)
        ("below m_begin", W(ptr, 0, N_WIN, 280, 252, po, 4096)),                       # m_end < m_begin
        ("the array holds", W(ptr, 0, N_WIN, 0, 4097, po, 4096)),                      # power_cap one too small
        ("2^32", W(ptr, top - N_WIN, N_WIN, mb_top, mb_top + 28, po, 4096)),           # first_sample + n = 2^32
        ("not a real format", lambda: d.power_device_as(0, ptr, 4096, po, 4096)),
        ("not a real format", lambda: d.power_device_as(2, ptr, 4096, po, 4096)),
        ("unknown sample format", lambda: d.power_device_as(7, ptr, 4096, po, 4096)),
        ("the array holds", lambda: d.power_device(ptr, 8196, po, 4096)),
        ("not an IQ format", lambda: d.power_device_iq(3, ptr, 4096, po, 4096)),
        ("multiple of 8", lambda: d.power_device_packed(ptr, 4100, po, 4096)),
    ]
    for word, call in cases:
        with pytest.raises(capi.AdsbError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        assert (read_out(to) == SENT).all(), word
    with pytest.raises(capi.AdsbError) as e:                                          # the host call: the same window rules
        d.power_window_host(x[:560], 0, 0, 281)
    assert "own pair" in str(e.value)
    # the long-stream handle is held to the same 2^32, and an empty window is no error
    dl = dec_factory(fresh=True)
    dl.set_long_stream(True)
    with pytest.raises(capi.AdsbError) as e:
        dl.power_window(ptr, top - N_WIN, N_WIN, mb_top, mb_top + 28, po, 4096)
    assert "2^32" in str(e.value)
    assert d.power_window(ptr, 0, N_WIN, 280, 280, po, 0) == 0 and (read_out(to) == SENT).all()
    assert d.power_window(ptr, 0, N_WIN, 0, 4096, po, 4096) == 4096                   # and the handle still works
    check_out(to, f["a64"][:4096], "after the refusals")


# ------------------------------------------------------------------ 8. the C host program
@pytest.mark.limit(120)
def test_cli_export_and_round_trip(capi, oracle, tmp_path):
    """-W on a 5 Mi-sample file (config1 tiled: a piece seam falls inside, and the file ends ragged) writes oracle.power's bytes, and
    -a -w on that output prints what -a on the capture prints."""
    x, rec = load_golden("config1_1Mi_100xDF17")
    big = np.concatenate([np.tile(x, 5), x[:3]])
    assert big.size > 2 * 28 * 74898 + 10_000
    cap, pw = tmp_path / "capture.bin", tmp_path / "out.pw"
    big.tofile(cap)
    p = subprocess.run([capi.CLI_PATH, "-W", str(pw), "-f", str(cap)], capture_output=True, timeout=100)
    assert p.returncode == 0 and not p.stdout, p.stderr
    assert b"6 trailing bytes ignored" in p.stderr
    want = oracle.power(big)[: 2 * (big.size // 4)]
    assert np.array_equal(np.fromfile(pw, dtype="<u4"), bits(want))
    assert S().power_domain_ok(want)
    a = subprocess.run([capi.CLI_PATH, "-a", "-f", str(cap)], capture_output=True, timeout=100)
    b = subprocess.run([capi.CLI_PATH, "-a", "-w", "-f", str(pw)], capture_output=True, timeout=100)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and len(a.stdout.splitlines()) >= 400
    table = lambda err: [ln for ln in err.decode().splitlines() if ln.startswith(("Try", "Ok", "Total"))]
    assert table(a.stderr) == table(b.stderr) and len(table(a.stderr)) == 3


@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", (2, 0))
def test_cli_export_iq(capi, tmp_path, fmt):
    x, rec = load_iq("mixed_df_a")
    src, pw = tmp_path / "capture.iq", tmp_path / "out.pw"
    with open(src, "wb") as f:
        f.write((x if fmt == 2 else S().to_float32_iq(x)).tobytes() + b"\x01\x02\x03")
    p = subprocess.run([capi.CLI_PATH, "-q", str(fmt), "-W", str(pw), "-f", str(src)], capture_output=True, timeout=100)
    assert p.returncode == 0 and not p.stdout, p.stderr
    assert b"3 trailing bytes ignored" in p.stderr
    assert np.array_equal(np.fromfile(pw, dtype="<u4"), bits(S().iq_power(x)))


# ------------------------------------------------------------------ 9. round the kernels' grid-stride loops
@pytest.mark.limit(120)
def test_real_export_second_trip_of_the_grid(capi, oracle, dec_factory, torch_cuda):
    """32 Mi + 5 full-range samples: 9363 wave passes over a grid that is capped at 2048 workgroups x 4 waves = 8192, so the waves of
    the first 293 workgroups go round the loop a second time -- FirConsts written again, the wave's LDS slice used again behind the
    first trip's stores, and the window's ragged last wave, which takes the direct-store road, on a wave whose first trip went
    through LDS -- while their neighbours in the same workgroup do not.  The whole array against the oracle, the guard behind it."""
    n = (1 << 25) + 5
    k = 2 * (n // 4)
    assert (k + 1791) // 1792 > 2048 * 4 and k % 1792 and k % 28
    x = np.random.default_rng(950).integers(0, 65536, n, dtype=np.uint16)
    want = oracle.power(x)[:k]
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, k)
    assert d.power_device(ptr, n, po, k) == k
    check_out(to, want, "32 Mi + 5 samples")


@pytest.mark.limit(120)
def test_iq_export_third_trip_of_the_grid(capi, dec_factory, torch_cuda):
    """4 Mi + 1027 complex samples: a trip of the IQ kernel's grid (2048 workgroups x 256 lanes x 4 samples) covers 2 Mi, so every lane
    goes round twice, the first 256 a third time, and 3 samples are the tail.  The whole array against iq_power, the guard behind it."""
    n = 2 * 2048 * 256 * 4 + 1027
    x = np.random.default_rng(951).integers(-32768, 32768, (n, 2), dtype=np.int16)
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    to, po = dev_out(torch_cuda, n)
    assert d.power_device_iq(2, ptr, n, po, n) == n
    check_out(to, S().iq_power(x), "4 Mi + 1027 complex samples")
