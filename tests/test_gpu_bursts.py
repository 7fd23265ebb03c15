"""The gate behind the envelope on the MI355X (run with -m gpu): burst_kernel.hip's three launches and the adsb_bursts_* calls, held
for EQUALITY -- begin, end, hot and the peak's bits, record for record, and B -- to adsbdec_amd.levels.bursts.  Every length around a
wave, a tile (T = adsb_burst_tile_runs()) and many tiles; the named patterns at a tile's seam; a table shorter than B against
poison; floats of every kind at five thresholds; envelopes 1, 2 and 3 floats behind a 16-byte boundary; a few hundred random cases;
the envelope as three level calls write it; a stream in progress beside it; the refusals; and the pipeline -- export, level, gate,
one batch decode of the pieces -- against the record tests/test_bursts_cpu.py checks, with the host program's -L -U beside it."""
import subprocess

import numpy as np
import pytest

import burst_cases as BC
from test_gpu_iq import to_dev
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

POISON = 0xA5


def LV():
    from adsbdec_amd import levels
    return levels


def same(got, want, how):
    """Two burst tables are equal field by field, the peak by its bits."""
    assert got.size == want.size, (how, got.size, want.size)
    for key in ("begin", "end", "hot"):
        assert np.array_equal(got[key], want[key]), (how, key, np.flatnonzero(got[key] != want[key])[:8])
    assert np.array_equal(got["peak"].view(np.uint32), want["peak"].view(np.uint32)), (how, "peak")


def run_case(d, torch, case, lead_floats=0):
    """One case through adsb_bursts_device with room for every burst and 8 records of poison behind them -> the statement's table."""
    name, env, threshold, lead, hang = case
    want = LV().bursts(env, threshold, lead, hang)
    t, ptr = to_dev(torch, env, lead=4 * lead_floats)
    table = np.frombuffer(bytearray([POISON]) * (16 * (want.size + 8)), dtype=LV().BURST_DTYPE)
    got, b = d.bursts_device(ptr, env.size, threshold, lead, hang, want.size + 8, table=table)
    assert b == want.size, (name, b, want.size)
    same(got, want, name)
    assert (table[want.size:].view(np.uint8) == POISON).all(), name
    return want


@pytest.fixture(scope="module")
def T(capi):
    return capi.burst_tile_runs()


# ------------------------------------------------------------------ 1. lengths and named patterns
@pytest.mark.limit(60)
def test_lengths_around_a_wave_a_tile_and_many_tiles(capi, dec_factory, torch_cuda, T):
    d = dec_factory()
    assert BC.LENGTHS(T) == (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 5, 40 * T + 3)
    for case in BC.length_cases(T):
        run_case(d, torch_cuda, case)


@pytest.mark.limit(60)
def test_named_patterns_at_the_seam(capi, dec_factory, torch_cuda, T):
    d = dec_factory()
    sizes = {}
    for case in BC.named_cases(T):
        sizes[case[0]] = run_case(d, torch_cuda, case).size
    # the cases are what their names say
    assert sizes["no hot run"] == 0 and sizes["every run hot"] == 1
    assert sizes["hot at T - 1 and T: one burst across the seam"] == 1
    assert sizes["hot at T - 1 and T - 1 + join: joined"] == 1 and sizes["hot at T - 1 and T + join: split"] == 2
    joined = sizes["two hot tiles, three empty between, join spans the three empty tiles: joined"]
    assert sizes["two hot tiles, three empty between, join one smaller: split"] == joined + 1


@pytest.mark.limit(60)
def test_most_bursts_and_a_table_shorter_than_b(capi, dec_factory, torch_cuda, T):
    """Every second run hot with lead = hang = 0: B = ceil(R / 2).  cap = B; cap = B / 3 against poison -- the records from cap on stay
    poison, the return value is still B, the records below cap are complete; cap = 0 with NULL only counts."""
    d = dec_factory()
    name, env, threshold, lead, hang = BC.alternating(T)
    want = LV().bursts(env, threshold, lead, hang)
    B = want.size
    assert B == (env.size + 1) // 2 and (want["hot"] == 1).all()
    t, ptr = to_dev(torch_cuda, env)
    got, b = d.bursts_device(ptr, env.size, threshold, lead, hang, B)
    assert b == B
    same(got, want, "cap = B")
    cap = B // 3
    table = np.frombuffer(bytearray([POISON]) * (16 * B), dtype=LV().BURST_DTYPE)
    got, b = d.bursts_device(ptr, env.size, threshold, lead, hang, cap, table=table)
    assert b == B and got.size == cap
    same(got, want[:cap], "cap = B / 3")
    assert (table[cap:].view(np.uint8) == POISON).all()
    got, b = d.bursts_device(ptr, env.size, threshold, lead, hang, 0)
    assert b == B and got.size == 0
    # the same with bursts of several tiles each: the table ends inside a burst that the tiles behind it would add to
    env2 = BC.envelope(7 * T, np.arange(7 * T))
    env2[[T // 2, 3 * T + 1]] = np.float32(0.0)
    want2 = LV().bursts(env2, threshold, 0, 0)
    assert want2.size == 3
    t2, ptr2 = to_dev(torch_cuda, env2)
    table = np.frombuffer(bytearray([POISON]) * (16 * 3), dtype=LV().BURST_DTYPE)
    got, b = d.bursts_device(ptr2, env2.size, threshold, 0, 0, 2, table=table)
    assert b == 3
    same(got, want2[:2], "cap inside")
    assert (table[2:].view(np.uint8) == POISON).all()


# ------------------------------------------------------------------ 2. values and alignment
@pytest.mark.limit(60)
def test_floats_of_every_kind_at_five_thresholds(capi, dec_factory, torch_cuda):
    d = dec_factory()
    env = BC.value_env()
    counts = []
    for threshold in BC.VALUE_THRESHOLDS:
        for lead, hang in ((0, 0), (1, 2)):
            want = run_case(d, torch_cuda, (threshold, env, threshold, lead, hang))
        counts.append(int(want["hot"].sum()))
    assert counts[0] == env.size                                    # +0.0: every run hot, the negative ones too (u = 0)
    assert counts[0] > counts[1] > counts[2] > counts[4] > counts[3] > 0      # ... the largest finite float is hot at itself; Inf: Inf and NaN


@pytest.mark.limit(60)
def test_envelopes_off_the_16_byte_grid(capi, dec_factory, torch_cuda, T):
    """The envelope 1, 2 and 3 floats behind a 16-byte boundary, with the floats in front of it and behind it hot: the head and the
    tail are read float by float, and nothing outside the envelope counts."""
    d = dec_factory()
    rng = np.random.default_rng(14)
    for R in (1, 2, 3, 5, 64, T - 1, T, T + 2, 3 * T + 5):
        inner = BC.envelope(R, np.flatnonzero(rng.random(R) < 0.2), R)
        inner[[0, R - 1]] = np.float32(5.0e5)
        padded = np.concatenate([np.full(8, 9.0e9, "<f4"), inner, np.full(8, 9.0e9, "<f4")])
        want = LV().bursts(inner, BC.THRESHOLD, 2, 3)
        for off in (0, 1, 2, 3):
            t, ptr = to_dev(torch_cuda, padded, lead=4 * off)          # inner starts 8 + off floats behind a 256-byte boundary
            got, b = d.bursts_device(ptr + 4 * 8, R, BC.THRESHOLD, 2, 3, want.size + 1)
            assert b == want.size
            same(got, want, (R, off))
    for case in BC.named_cases(T):
        for off in (1, 3):
            run_case(d, torch_cuda, case, lead_floats=off)


# ------------------------------------------------------------------ 3. random
@pytest.mark.limit(120)
def test_random_cases(capi, dec_factory, torch_cuda, T):
    d = dec_factory()
    nonempty = 0
    for i, case in enumerate(BC.random_cases(T, 300, 3003)):
        nonempty += run_case(d, torch_cuda, case, lead_floats=i % 4 if i % 5 == 0 else 0).size > 0
    assert nonempty > 200


# ------------------------------------------------------------------ 4. where the envelope comes from
@pytest.mark.limit(60)
def test_the_envelope_of_three_level_calls(capi, oracle, dec_factory, torch_cuda):
    """A uint16 capture, an int16 IQ capture and an int8 IQ capture: level_device* with the envelope followed by bursts_device,
    Decoder.bursts (uint16) and bursts_host equal the statement on levels.level_report(...)["env"]."""
    from adsbdec_amd import sample_formats
    d = dec_factory()
    rng = np.random.default_rng(15)
    n = 3 * 7168 * 4 + 6

    def loud(x, lo, hi, scale):
        for s in rng.integers(0, len(x) - 400, 25):
            x[s:s + int(rng.integers(30, 400))] = rng.integers(lo, hi, dtype=x.dtype) if scale else hi
        return x
    x16 = rng.integers(2040, 2056, n).astype(np.uint16)
    for s in rng.integers(0, n - 800, 25):
        x16[s:s + 600:2] = 3500
    iq16 = loud(rng.integers(-40, 40, (n // 2, 2)).astype(np.int16), 0, 9000, False)
    iq8 = loud(rng.integers(-3, 4, (n // 2, 2)).astype(np.int8), 0, 100, False)
    for kind, x, a in (("real", x16, None), ("iq16", iq16, sample_formats.iq_power(iq16, 2)), ("iq8", iq8, sample_formats.iq_power(iq8, 8))):
        if a is None:
            a = np.ascontiguousarray(oracle.power(x)[:2 * (x.size // 4)])
        rep = LV().level_report(np.ascontiguousarray(a))
        env = rep["env"]
        threshold = float(np.float32(8.0 * LV().percentile(rep["hist"], 0.5)))
        want = LV().bursts(env, threshold, 2, 4)
        assert want.size >= 3, (kind, want.size)
        t, ptr = to_dev(torch_cuda, x)
        te, pe = to_dev(torch_cuda, np.zeros(env.size, np.float32))
        if kind == "real":
            d.level_device(ptr, x.size, pe, env.size)
        else:
            d.level_device_iq(2 if kind == "iq16" else 8, ptr, len(x), pe, env.size)
        got, b = d.bursts_device(pe, env.size, threshold, 2, 4, want.size)
        assert b == want.size
        same(got, want, kind + " device")
        got, b = d.bursts_host(env, threshold, 2, 4)
        assert b == want.size
        same(got, want, kind + " host")
        if kind == "real":
            got, b = d.bursts(x, q=0.5, factor=8.0, lead=2, hang=4)
            assert b == want.size
            same(got, want, "Decoder.bursts")
    got, b = d.bursts(np.zeros(3, np.uint16))
    assert b == 0 and got.size == 0                                  # no power sample: no run, nothing launched
    got, b = d.bursts_host(np.zeros(0, np.float32), 1.0, 1, 1, cap=4)
    assert b == 0 and got.size == 0


# ------------------------------------------------------------------ 5. state
@pytest.mark.limit(60)
def test_a_call_between_two_pushes_and_the_refusals(capi, dec_factory, torch_cuda, T):
    import ctypes as C
    from conftest import golden_cases, load_golden
    x, rec = load_golden(golden_cases()[0])
    plain = dec_factory(fresh=True, df18=rec["df18"])
    want_frames = plain.decode(x)
    d = dec_factory(fresh=True, df18=rec["df18"])
    case = BC.named_cases(T)[7]
    half = x.size // 2 // 8 * 8
    d.push(x[:half])
    run_case(d, torch_cuda, case)
    d.push(x[half:])
    d.finish()
    assert d.drain() == want_frames
    # every refusal: -1 with its message, the table untouched, the handle usable afterwards
    name, env, threshold, lead, hang = case
    t, ptr = to_dev(torch_cuda, env)
    L, h = d._L, d._h
    table = np.full(16 * 8, POISON, np.uint8)
    tp = table.ctypes.data
    refusals = ((0, 5, threshold, lead, hang, tp, 8, "NULL envelope"),
                (ptr + 2, 5, threshold, lead, hang, tp, 8, "4-byte aligned"),
                (ptr, 1 << 31, threshold, lead, hang, tp, 8, "2^31"),
                (ptr, env.size, float("nan"), lead, hang, tp, 8, "threshold"),
                (ptr, env.size, -0.0, lead, hang, tp, 8, "threshold"),
                (ptr, env.size, -1.0, lead, hang, tp, 8, "threshold"),
                (ptr, env.size, threshold, (1 << 30) + 1, hang, tp, 8, "2^30"),
                (ptr, env.size, threshold, lead, (1 << 30) + 1, tp, 8, "2^30"),
                (ptr, env.size, threshold, lead, hang, 0, 8, "NULL table"))
    for fn in (L.adsb_bursts_device, L.adsb_bursts_host):
        host = fn is L.adsb_bursts_host
        for p, n, th, le, ha, tab, cap, word in refusals:
            if host and p:
                p = env.ctypes.data + (p - ptr)
            assert fn(h, p or None, n, th, le, ha, tab or None, cap) == -1, (host, word)
            assert word in L.adsb_last_error(h).decode(), (word, L.adsb_last_error(h))
            assert (table == POISON).all(), word
    assert L.adsb_bursts_device(h, None, 0, threshold, lead, hang, None, 0) == 0      # no run: 0, nothing launched
    run_case(d, torch_cuda, case)


# ------------------------------------------------------------------ 6. the pipeline
@pytest.mark.limit(120)
def test_pipeline_export_level_gate_decode(capi, oracle, dec_factory, torch_cuda, tmp_path):
    """power_device_iq -> level_device_power with the envelope -> bursts_device -> ONE decode_batch_device_power on the pieces (the
    pointers out_ptr + 112 begin are 16-byte aligned); the frames per burst are the oracle's, record for record -- the record
    tests/test_bursts_cpu.py holds to the planted frames.  The host program's -L -U lines for the same file are the statement's."""
    p = BC.pipeline()
    record = BC.frames_per_burst(oracle)
    x, M = p["x"], p["a"].size
    d = dec_factory(fresh=True, df18=True)
    t, ptr = to_dev(torch_cuda, x)
    ta, pa = to_dev(torch_cuda, np.zeros(M, np.float32))
    assert d.power_device_iq(2, ptr, len(x), pa, M) == M
    n_env = -(-M // 28)
    te, pe = to_dev(torch_cuda, np.zeros(n_env, np.float32))
    rep = d.level_device_power(pa, M, pe, n_env)
    threshold = float(np.float32(BC.FACTOR * capi.level_percentile(rep["hist"], 0.5)))
    assert threshold == p["threshold"]
    got, b = d.bursts_device(pe, n_env, threshold, BC.LEAD, BC.HANG, 64)
    assert b == p["bursts"].size
    same(got, p["bursts"], "pipeline")
    slices = LV().burst_samples(got, M)
    assert np.array_equal(slices, p["slices"])
    assert all((pa + 112 * int(r["begin"])) % 16 == 0 for r in got)
    frames = d.decode_batch_device_power([pa + 112 * int(r["begin"]) for r in got], [int(hi - lo) for lo, hi in slices])
    assert len(frames) == len(record)
    for k, (mine, want) in enumerate(zip(frames, record)):
        assert [(f["g"], f["ts"], f["pw"], f["frame"]) for f in mine] == want, k
    # the host program
    path = tmp_path / "pipeline.iq16"
    x.tofile(path)
    out = subprocess.run([capi.CLI_PATH, "-L", "-q", "2", "-U", "%g" % BC.FACTOR, "-f", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("bursts "))
    assert lines[at] == "bursts %d threshold %.9g lead %d hang %d" % (b, threshold, BC.LEAD, BC.HANG)
    assert lines[at - 1].startswith("median ") and len(lines) == at + 1 + b
    for ln, (lo, hi), r in zip(lines[at + 1:], slices, p["bursts"]):
        assert ln == "%d %d %d %.9g" % (lo, hi, r["hot"], r["peak"]), ln
    plain = subprocess.run([capi.CLI_PATH, "-L", "-q", "2", "-f", str(path)], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0 and plain.stdout.splitlines() == lines[:at]           # -L's own report is what it was
