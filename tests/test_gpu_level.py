"""The level report on the MI355X (run with -m gpu): level_kernel / level_units_kernel and every adsb_level_* call, held for EQUALITY --
counters, the 2048 bins and the envelope's bits -- to adsbdec_amd.levels.level_report of the power samples the export of the same
flavour is defined to write: oracle.power(x) for real captures, sample_formats.iq_power for complex ones, the caller's floats for
power input; never the library's own export.  The committed fixtures; content that loads the accumulation (silence, the two rails
in turn, two bins); every length around a run, a wave's pass (1792 power samples) and a workgroup's (7168), and one capture long
enough that waves go round the grid-stride loop; totals zeroed per call; the converted and packed twins; the three IQ formats with
rails planted; floats outside the _power domain; a stream in progress beside it; the refusals; the host call and the C host
program's -L."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records
from iq8_cases import iq8_fixtures, load_iq8
from test_gpu_iq import to_dev
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)
from test_iq_cpu import iq_cases, load_iq

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF          # a NaN no envelope float of these tests is: what an unwritten float holds
SENT64 = 0xA5A5A5A5A5A5A5A5
GUARD = 64
COUNTERS = ("samples", "negative", "rail_lo", "rail_hi", "over")


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def LV():
    from adsbdec_amd import levels
    return levels


def dev_env(torch, m, lead=0):
    """ceil(m / 28) + GUARD sentinels on the device: (tensor, pointer, floats of the envelope)."""
    k = -(-m // 28)
    t, p = to_dev(torch, np.full(k + GUARD, SENT, np.uint32), lead=lead)
    return t, p, k


def want_real(oracle, x, a=None):
    """The report of a real capture: level_report of the oracle's power samples, the rails of its codes."""
    k = 2 * (x.size // 4)
    a = oracle.power(x) if a is None else a
    return LV().with_rails(LV().level_report(np.ascontiguousarray(a[:k])), x, "real")


def check(got, env_t, want, how):
    """Counters, bins and envelope bits are `want`'s, and the envelope array behind its last float is untouched."""
    for key in COUNTERS:
        assert got[key] == want[key], (how, key, got[key], want[key])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), (how, np.flatnonzero(got["hist"] != want["hist"])[:8])
    assert int(got["hist"].sum()) + got["negative"] == got["samples"], how
    if env_t is not None:
        e = env_t.cpu().numpy().view(np.uint32)
        k = want["env"].size
        assert np.array_equal(e[:k], want["env"].view(np.uint32)), (how, np.flatnonzero(e[:k] != want["env"].view(np.uint32))[:8])
        assert (e[k:] == SENT).all(), how


# ------------------------------------------------------------------ 1. the fixtures
@pytest.mark.limit(60)
@pytest.mark.parametrize("name", golden_cases())
def test_uint16_fixtures(capi, oracle, dec_factory, torch_cuda, name):
    x, rec = load_golden(name)
    want = want_real(oracle, x)
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    te, pe, k = dev_env(torch_cuda, want["samples"])
    got = d.level_device(ptr, x.size, pe, k)
    check(got, te, want, name)
    if name == "wide_codes_noise":                                      # (n % 4 == 2: the last two codes, both above 4095, count)
        assert got["over"] == 212_323 == int((x > 4095).sum())
    if name == "dense_noise_256Ki":
        assert got["rail_lo"] > 0 and got["rail_hi"] > 0
    check(d.level_device(ptr, x.size), None, want, name + " without an envelope")


# ------------------------------------------------------------------ 2. content that loads the accumulation
@pytest.mark.limit(60)
def test_silence_rails_and_two_bins(capi, oracle, dec_factory, torch_cuda):
    """Silence puts every increment of every pass on bin 0 (the wave-uniform road, 64 lanes on one counter); a capture alternating
    0 and 4095 puts every code on a rail; power samples drawn from two bins, in stretches where a whole wave agrees and in stretches
    where it does not, take both roads of one increment."""
    d = dec_factory()
    n = 2 * (3 * 7168 + 30) + 3
    for how, x in (("silence", np.full(n, 0x800, np.uint16)), ("rails", np.tile(np.array([0, 4095], np.uint16), n // 2 + 1)[:n])):
        want = want_real(oracle, x)
        t, ptr = to_dev(torch_cuda, x)
        te, pe, k = dev_env(torch_cuda, want["samples"])
        got = d.level_device(ptr, n, pe, k)
        check(got, te, want, how)
        if how == "silence":
            assert int(got["hist"][0]) == got["samples"] == 2 * (n // 4) and got["rail_lo"] == got["rail_hi"] == 0
        else:
            assert got["rail_lo"] == (n + 1) // 2 and got["rail_hi"] == n // 2 and got["over"] == 0   # (all n codes, the last three too)
    rng = np.random.default_rng(2)
    m = 5 * 7168 + 13
    a = np.where(rng.integers(0, 2, m) == 1, np.float32(3.0), np.float32(1.0)).astype("<f4")
    a[1792: 3 * 1792] = np.float32(3.125)                                 # two passes of a wave that agree on bin 1028 ...
    a[7168 + 28 * 5: 7168 + 28 * 6] = np.float32(1.0)                    # ... and one lane's run that agrees with itself only
    want = LV().level_report(a)
    assert np.count_nonzero(want["hist"]) == 2
    t, ptr = to_dev(torch_cuda, a)
    te, pe, k = dev_env(torch_cuda, m)
    check(d.level_device_power(ptr, m, pe, k), te, want, "two bins")


# ------------------------------------------------------------------ 3. lengths around every seam of the pass structure
M_SEAMS = (0, 2, 26, 28, 30, 1790, 1792, 1794, 7166, 7170, 3 * 7168 + 30)


@pytest.mark.limit(120)
def test_lengths_around_run_wave_and_workgroup(capi, oracle, dec_factory, torch_cuda):
    """Full-range codes; n = 2 M + (0 .. 3) for every M of the list: the oracle's prefix (power(x[:n]) is power(x)'s first 2 (n // 4)
    floats: tests/test_power_export_cpu.py), M power samples and not one more; the rail counters run over all n codes, the
    trailing n % 4 included, unless the capture has no power sample at all."""
    x = np.random.default_rng(355).integers(0, 65536, 2 * M_SEAMS[-1] + 3, dtype=np.uint16)
    a = oracle.power(x)
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    for i, m in enumerate(M_SEAMS):
        n = 2 * m + i % 4
        want = want_real(oracle, x[:n], a)
        assert want["samples"] == m
        te, pe, k = dev_env(torch_cuda, m)
        got = d.level_device(ptr, n, pe if m else 0, k)
        check(got, te, want, n)


@pytest.mark.limit(120)
def test_second_trip_of_the_grid(capi, oracle, dec_factory, torch_cuda):
    """32 Mi + 5 full-range samples, the size of the export's own test, and the export's grid: 9363 wave passes over at most 2048
    workgroups x 4 waves = 8192, so the waves of the first 293 workgroups go round the loop a second time -- their LDS histograms
    and scalar counters carried from trip to trip, the FIR's constants written again -- while their neighbours do not, and the
    capture's ragged last wave is the second trip of a wave whose first was whole."""
    n = (1 << 25) + 5
    k = 2 * (n // 4)
    assert (k + 1791) // 1792 > 2048 * 4 and k % 1792 and k % 28
    x = np.random.default_rng(950).integers(0, 65536, n, dtype=np.uint16)
    want = want_real(oracle, x)
    d = dec_factory()
    t, ptr = to_dev(torch_cuda, x)
    te, pe, ke = dev_env(torch_cuda, k)
    check(d.level_device(ptr, n, pe, ke), te, want, "32 Mi + 5 samples")


# ------------------------------------------------------------------ 4. the totals are zeroed per call
@pytest.mark.limit(60)
def test_calling_twice_gives_the_same_report(capi, oracle, dec_factory, torch_cuda):
    x, _ = load_golden("dense_noise_256Ki")
    y, _ = load_golden("wide_codes_noise")
    wx, wy = want_real(oracle, x), want_real(oracle, y)
    d = dec_factory()
    tx, px = to_dev(torch_cuda, x)
    ty, py = to_dev(torch_cuda, y)
    check(d.level_device(px, x.size), None, wx, "first")
    check(d.level_device(px, x.size), None, wx, "again")
    check(d.level_device(py, y.size), None, wy, "another capture")
    check(d.level_device(px, x.size), None, wx, "behind another capture")


# ------------------------------------------------------------------ 5. the converted and packed twins
@pytest.mark.limit(60)
def test_converted_and_packed_twins(capi, oracle, dec_factory, torch_cuda):
    """fmt 3, fmt 1 and packed 12-bit: the report of the uint16 twin, rails counted on the converted codes; the format report
    moves as the export's does (n per converting call, nothing for fmt 4 / 5 and packed)."""
    from adsbdec_amd.packed12 import pack12
    x, rec = load_golden("dense_noise_256Ki")
    n = x.size
    want = want_real(oracle, x)
    assert want["rail_lo"] > 0 and want["rail_hi"] > 0
    d = dec_factory()
    d.reset()
    for fmt, twin in ((3, S().to_int16_real(x)), (1, S().to_float32_real(x)), (4, x), (5, x)):
        tt, pt = to_dev(torch_cuda, twin)
        te, pe, k = dev_env(torch_cuda, want["samples"])
        check(d.level_device_as(fmt, pt, n, pe, k), te, want, fmt)
    assert d.format_report() == (2 * n, 0, 0)
    tp, pp = to_dev(torch_cuda, pack12(x[: n - n % 8]))
    wp = want_real(oracle, x[: n - n % 8])
    te, pe, k = dev_env(torch_cuda, wp["samples"])
    check(d.level_device_packed(pp, n - n % 8, pe, k), te, wp, "packed")
    assert d.format_report() == (2 * n, 0, 0)


# ------------------------------------------------------------------ 6. complex captures
def want_iq(x, fmt):
    """x: the capture as the call is given it.  The power samples are sample_formats.iq_power's; the rails are those of the int16
    grid (fmt 0: behind the conversion, so a clamped float shows) or of the bytes (fmt 8)."""
    a = S().iq_power(x, fmt)
    grid = S().flags_float32_iq(x)[0] if fmt == 0 else x
    return LV().with_rails(LV().level_report(a), grid, "iq8" if fmt == 8 else "iq16")


def planted_iq(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == 8:
        x = rng.integers(-100, 100, (n, 2), dtype=np.int8)
        lo, hi = -128, 127
    else:
        x = rng.integers(-20000, 20000, (n, 2), dtype=np.int16)
        lo, hi = -32768, 32767
    where = rng.choice(n, size=min(n, 7), replace=False)
    for j, i in enumerate(where):
        x[i, j % 2] = lo if j % 3 else hi
    x[where[0]] = (hi, lo)                                               # (n = 1 too: both rails)
    if fmt != 0:
        return x
    f = S().to_float32_iq(x)
    f[where[0], 0], f[where[-1], 1] = np.float32(1.5), np.float32(-7.0)     # out of range: clamped onto the rails
    if n > 3:
        f[where[1], 1] = np.float32(np.inf)
    return f


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (2, 0, 8))
def test_iq_formats_with_rails_planted(capi, dec_factory, torch_cuda, fmt):
    """Every length class: below a run, odd, a wave's pass and one more, several workgroups with a ragged end; from an array that is
    16-byte aligned (the 16-byte loads) and from one that is not (unit by unit)."""
    d = dec_factory()
    d.reset()
    converted = 0
    for i, n in enumerate((1, 27, 1792, 1793, 3 * 7168 + 45)):
        x = planted_iq(fmt, n, 60 + i)
        want = want_iq(x, fmt)
        assert want["rail_lo"] > 0 and want["rail_hi"] > 0 and want["over"] == 0 and want["samples"] == n
        for lead in (0, 4 if fmt != 8 else 2):
            t, ptr = to_dev(torch_cuda, x, lead=lead)
            te, pe, k = dev_env(torch_cuda, n)
            check(d.level_device_iq(fmt, ptr, n, pe, k), te, want, (fmt, n, lead))
            converted += 2 * n if fmt == 0 else 0
    rep = d.format_report()
    assert rep[0] == converted and (fmt != 0 or rep[2] > 0)


@pytest.mark.limit(60)
def test_iq_fixtures(capi, dec_factory, torch_cuda):
    d = dec_factory()
    for fmt, names, load in ((2, iq_cases(), load_iq), (8, iq8_fixtures(), load_iq8)):
        for name in names:
            x, rec = load(name)
            want = want_iq(x, fmt)
            t, ptr = to_dev(torch_cuda, x)
            te, pe, k = dev_env(torch_cuda, len(x))
            check(d.level_device_iq(fmt, ptr, len(x), pe, k), te, want, (fmt, name))


# ------------------------------------------------------------------ 7. power input, inside and outside its domain
@pytest.mark.limit(60)
def test_power_input_outside_its_domain(capi, dec_factory, torch_cuda):
    """NaN, +-Inf, -0.0, a negative, 2^29 and the largest value below it, planted one kind at a time and all together: the report is
    level_report's, and its verdict (negative == 0 and hist[1248:] empty) is power_domain_ok's."""
    d = dec_factory()
    m = 2 * 7168 + 17
    base = np.random.default_rng(77).uniform(0.0, 1.0e6, m).astype("<f4")
    below = np.array([0x4E000000 - 1], "<u4").view("<f4")[0]
    plants = {"inside": [], "below 2^29": [below], "NaN": [np.float32(np.nan)], "+Inf": [np.float32(np.inf)], "-Inf": [np.float32(-np.inf)],
              "-0.0": [np.float32(-0.0)], "negative": [np.float32(-3.0)], "2^29": [np.float32(2.0 ** 29)]}
    plants["all"] = [v[0] for v in plants.values() if v]
    for how, vals in plants.items():
        a = base.copy()
        at = np.random.default_rng(len(how)).choice(m, size=len(vals), replace=False)
        a[at] = vals
        want = LV().level_report(a)
        for lead in (0, 4):
            t, ptr = to_dev(torch_cuda, a, lead=lead)
            te, pe, k = dev_env(torch_cuda, m)
            got = d.level_device_power(ptr, m, pe, k)
            check(got, te, want, (how, lead))
            assert got["rail_lo"] == got["rail_hi"] == got["over"] == 0
            assert LV().domain_ok(got) == S().power_domain_ok(a) == (how in ("inside", "below 2^29")), how


# ------------------------------------------------------------------ 8. a stream in progress is not touched
@pytest.mark.limit(60)
def test_a_stream_in_progress_is_untouched(capi, oracle, dec_factory, torch_cuda):
    x, rec = load_golden("config1_1Mi_100xDF17")
    y, _ = load_golden("dense_noise_256Ki")
    want = want_real(oracle, y)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptr = to_dev(torch_cuda, y)
    d.reset()
    half = x.size // 2 + 1
    d.push(x[:half])
    te, pe, k = dev_env(torch_cuda, want["samples"])
    check(d.level_device(ptr, y.size, pe, k), te, want, "between the pushes")
    got = d.level(y)
    check(got, None, want, "the host call between the pushes")
    assert np.array_equal(got["env"].view(np.uint32), want["env"].view(np.uint32))
    d.push(x[half:])
    d.finish()
    assert records(d.drain()) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 9. refusals
@pytest.mark.limit(60)
def test_refusals_write_nothing(capi, dec_factory, torch_cuda):
    """Each refusal leaves a sentinel-filled report and envelope as they were and the format report unmoved."""
    d = dec_factory()
    d.reset()
    n = 1 << 16
    x = np.random.default_rng(9).integers(0, 4096, n, dtype=np.uint16)
    t, ptr = to_dev(torch_cuda, x)
    te, pe, k = dev_env(torch_cuda, n)                                     # room for every flavour's M
    out = capi.LevelReport()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    before = d.format_report()
    km = -(-(n // 2) // 28)
    big = 1 << 32
    cases = [
        ("NULL buffer", lambda: d.level_device(0, n, pe, k, out=out)),
        ("NULL buffer", lambda: d.level_device_as(3, 0, n, pe, k, out=out)),
        ("NULL buffer", lambda: d.level_device_packed(0, n, pe, k, out=out)),
        ("NULL samples", lambda: d.level_device_iq(2, 0, n, pe, k, out=out)),
        ("NULL samples", lambda: d.level_device_power(0, n, pe, k, out=out)),
        ("16-byte", lambda: d.level_device(ptr + 8, n - 8, pe, k, out=out)),
        ("2-byte aligned", lambda: d.level_device_as(3, ptr + 1, n - 8, pe, k, out=out)),
        ("4-byte aligned", lambda: d.level_device_as(1, ptr + 2, n // 2 - 8, pe, k, out=out)),
        ("4-byte aligned", lambda: d.level_device_packed(ptr + 2, 4096, pe, k, out=out)),
        ("4-byte aligned", lambda: d.level_device_iq(2, ptr + 2, 4096, pe, k, out=out)),
        ("4-byte aligned", lambda: d.level_device_iq(0, ptr + 2, 4096, pe, k, out=out)),
        ("2-byte aligned", lambda: d.level_device_iq(8, ptr + 1, 4096, pe, k, out=out)),
        ("4-byte aligned", lambda: d.level_device_power(ptr + 2, 4096, pe, k, out=out)),
        ("the array holds", lambda: d.level_device(ptr, n, pe, km - 1, out=out)),              # env_cap one too small
        ("the array holds", lambda: d.level_device_iq(2, ptr, n // 2, pe, km - 1, out=out)),   # (M = n / 2 complex samples here)
        ("the array holds", lambda: d.level_device_power(ptr, n // 2, pe, km - 1, out=out)),
        ("the array holds", lambda: d.level_device(ptr, n, pe, 0, out=out)),                   # a non-NULL envelope with cap 0
        ("NULL envelope", lambda: d.level_device(ptr, n, 0, km, out=out)),
        ("the envelope must be 4-byte aligned", lambda: d.level_device(ptr, n, pe + 2, k - 1, out=out)),
        ("not a real format", lambda: d.level_device_as(0, ptr, 4096, pe, k, out=out)),
        ("not a real format", lambda: d.level_device_as(2, ptr, 4096, pe, k, out=out)),
        ("unknown sample format", lambda: d.level_device_as(7, ptr, 4096, pe, k, out=out)),
        ("not an IQ format", lambda: d.level_device_iq(3, ptr, 4096, pe, k, out=out)),
        ("not an IQ format", lambda: d.level_device_iq(1, ptr, 4096, pe, k, out=out)),
        ("multiple of 8", lambda: d.level_device_packed(ptr, 4100, pe, k, out=out)),
        ("2^32", lambda: d.level_device(ptr, big, 0, 0, out=out)),                             # n at the flavour's limit
        ("2^32", lambda: d.level_device_as(3, ptr, big, 0, 0, out=out)),
        ("2^32", lambda: d.level_device_packed(ptr, big, 0, 0, out=out)),
        ("2^31", lambda: d.level_device_iq(2, ptr, 1 << 31, 0, 0, out=out)),
        ("2^31", lambda: d.level_device_iq(8, ptr, 1 << 31, 0, 0, out=out)),
        ("2^31", lambda: d.level_device_power(ptr, 1 << 31, 0, 0, out=out)),
    ]
    words = np.ctypeslib.as_array((C.c_uint64 * (5 + 2048)).from_buffer(out))
    for word, call in cases:
        with pytest.raises(capi.AdsbError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
        assert (words == SENT64).all(), word
        assert (te.cpu().numpy().view(np.uint32) == SENT).all(), word
        assert d.format_report() == before, word
    with pytest.raises(capi.AdsbError) as e:                                # the host call: the same rules
        L = capi.load()
        if L.adsb_level_host(d._h, x.ctypes.data, big, C.byref(out), None, 0) < 0:
            d._check(-1, "adsb_level_host")
    assert "2^32" in str(e.value) and (words == SENT64).all()
    # no power samples: a zeroed report, NULL pointers allowed, nothing launched; and the handle still works
    for got in (d.level_device(0, 3, out=out), d.level_device_iq(8, 0, 0), d.level_device_power(0, 0), d.level_device_packed(0, 0),
                d.level_device_as(1, 0, 2)):
        assert all(got[key] == 0 for key in COUNTERS) and not got["hist"].any()
    assert not words.any()
    got = d.level_device(ptr, n, pe, k)
    assert got["samples"] == n // 2 and got["over"] == 0


# ------------------------------------------------------------------ 10. the host call and the C host program
def parse_cli(text):
    lines = text.splitlines()
    head = lines[0].split()
    assert head[0::2] == list(COUNTERS), head
    out = dict(zip(head[0::2], (int(v) for v in head[1::2])))
    hist = np.zeros(2048, np.uint64)
    for ln in lines[1:-1]:
        w = ln.split()
        assert w[0] == "bin" and len(w) == 4, ln
        hist[int(w[1])] = int(w[3])
        assert float(w[2]) == LV().bin_lower_edge(int(w[1])), ln
    out["hist"] = hist
    tail = lines[-1].split()
    assert tail[0::3] == ["median", "p99.9", "peak"] and tail[2::3] == ["dB"] * 3, lines[-1]
    return out, [float(v) for v in tail[1::3]]


@pytest.mark.limit(120)
def test_host_call_and_cli(capi, oracle, dec_factory, tmp_path):
    """adsb_level_host on a fixture, with and without an envelope; -L on the same file prints the same counters and bins and the
    summary's three bins in dB of raw power units; -L -q 8 on an int8 fixture likewise, trailing bytes named on stderr."""
    x, rec = load_golden("wide_codes_noise")
    want = want_real(oracle, x)
    d = dec_factory()
    got = d.level(x)
    check(got, None, want, "adsb_level_host")
    assert np.array_equal(got["env"].view(np.uint32), want["env"].view(np.uint32))
    check(d.level(x, env=False), None, want, "adsb_level_host without an envelope")
    x8, _ = load_iq8("noise")
    files = ((tmp_path / "capture.bin", x.tobytes() + b"\x01", [], want, b"1 trailing bytes ignored" if x.size % 4 == 0 else b"trailing bytes ignored"),
             (tmp_path / "capture.cs8", x8.tobytes() + b"\x01", ["-q", "8"], want_iq(x8, 8), b"1 trailing bytes ignored"))
    for path, data, sel, w, note in files:
        path.write_bytes(data)
        p = subprocess.run([capi.CLI_PATH, *sel, "-L", "-f", str(path)], capture_output=True, timeout=100)
        assert p.returncode == 0, p.stderr
        assert note in p.stderr, p.stderr
        text = p.stdout.decode()
        assert "dBFS" not in text
        r, db = parse_cli(text)
        for key in COUNTERS:
            assert r[key] == w[key], (path.name, key)
        assert np.array_equal(r["hist"], w["hist"]), path.name
        edges = [LV().percentile(w["hist"], 0.5), LV().percentile(w["hist"], 0.999), LV().bin_lower_edge(int(np.flatnonzero(w["hist"])[-1]))]
        for have, edge in zip(db, edges):
            assert abs(have - 10 * np.log10(edge)) <= 0.006, (path.name, have, edge)    # (printed with two decimals)
