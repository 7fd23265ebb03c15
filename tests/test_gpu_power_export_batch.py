"""The batch power export on the MI355X (run with -m gpu): power_export_batch_kernel / iq_power_export_batch_kernel and every
adsb_power_batch_* call.  Capture i of a batch is held bit for bit (floats compared as uint32) to what the single call of the same
flavour writes for it alone, and to the definition: oracle.power -- the restatement of air.c:54-91 that tests/test_oracle_vs_ref.py
holds to the reference's decodeiq -- or sample_formats.iq_power.  The captures of a batch lie back to back in ONE device allocation
of full-range codes, so that a neighbour's samples lie where a capture's silence must be read, and the outputs lie in ONE buffer
with 64 sentinel floats between them, so that a float written past a capture's count shows."""
import numpy as np
import pytest

from conftest import golden_records, load_golden, records
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF          # a NaN no power sample is: what an unwritten float of an output holds
GUARD = 64
W = 3584                   # samples of a pass: one wave, 64 runs of 28 power samples
# the edges of a run (56 samples) and of a wave (3584), around one, two, four and eight waves
EDGES = [0, 1, 3, 4, 7, 8, 55, 56, 57, 60, 3583, 3584, 3585, 3587, 3588, 3640, 7167, 7168, 7172, 4 * W - 4, 4 * W + 4, 8 * W + 56]
IQ_LENGTHS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4099]
PACKED_LENGTHS = [0, 8, 56, 64, 3584, 3592, 7168, 7176, 4 * W + 8]
AS_LENGTHS = [0, 3, 4, 7, 57, 3585, 3588, 7172, 4 * W + 4]


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def carve(torch, arrays, align, seed=7):
    """The arrays back to back in ONE device allocation, each at the next multiple of `align` bytes; every byte between and behind
    them is noise.  -> (tensor that keeps the memory alive, pointers; None for an empty array)."""
    blobs = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]
    at, off = [], 0
    for b in blobs:
        off = -(-off // align) * align
        at.append(off)
        off += b.size
    buf = np.random.default_rng(seed).integers(0, 256, off + 256, dtype=np.uint8)
    for o, b in zip(at, blobs):
        buf[o: o + b.size] = b
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0
    return t, [t.data_ptr() + o if b.size else None for o, b in zip(at, blobs)]


class Outputs:
    """One device buffer of sentinels: GUARD floats, capture 0's floats (a multiple of 4, so that every array is 16-byte aligned),
    GUARD floats, capture 1's ... and GUARD floats behind the last."""

    def __init__(self, torch, counts):
        self.counts, self.at, off = list(counts), [], GUARD
        for k in self.counts:
            self.at.append(off)
            off += -(-k // 4) * 4 + GUARD
        self.floats = off
        self.t = torch.from_numpy(np.full(off, SENT, np.uint32).view(np.uint8)).cuda()
        self.ptrs = [self.t.data_ptr() + 4 * o for o in self.at]
        self.caps = list(self.counts)

    def read(self):
        return self.t.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.read() == SENT).all())

    def check(self, wants, how):
        """Every capture's floats are `wants[i]` bit for bit, and every other float of the buffer still holds the sentinel."""
        want = np.full(self.floats, SENT, np.uint32)
        for o, k, w in zip(self.at, self.counts, wants):
            assert len(w) == k, how
            want[o: o + k] = bits(w)
        got = self.read()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (how, bad[:8], [i for i, o in enumerate(self.at) if o <= bad[0]][-1:])

    def piece(self, got, i):
        return got[self.at[i]: self.at[i] + self.counts[i]]


def real_power(oracle, x):
    k = 2 * (x.size // 4)
    return oracle.power(x)[:k] if k else np.zeros(0, np.float32)


def single_calls(torch, call, ptrs, ns, counts):
    """What the single call writes for every capture alone: call(ptr, n, out_ptr, cap) -> list of uint32 arrays."""
    out = []
    for p, n, k in zip(ptrs, ns, counts):
        t = torch.from_numpy(np.full(k + GUARD, SENT, np.uint32).view(np.uint8)).cuda()
        assert call(p or 0, n, t.data_ptr(), k) == k
        got = t.cpu().numpy().view(np.uint32)
        assert (got[k:] == SENT).all()
        out.append(got[:k])
    return out


_edges = {}


def edge_batch(oracle):
    """The edge lengths in a seeded shuffled order with a zero-length capture between every two, full-range codes, and the oracle's
    power samples of every capture: computed once, shared by the tests below and never changed."""
    if not _edges:
        rng = np.random.default_rng(1792)
        order = list(EDGES)
        rng.shuffle(order)
        ns = []
        for n in order:
            ns += [n, 0]
        xs = [rng.integers(0, 65536, n, dtype=np.uint16) for n in ns]
        _edges.update(ns=ns, xs=xs, want=[real_power(oracle, x) for x in xs])
    return _edges


# ------------------------------------------------------------------ 1. the edges of a wave and of a run
@pytest.mark.limit(60)
def test_edges_back_to_back(capi, oracle, dec_factory, torch_cuda):
    e = edge_batch(oracle)
    ns, xs, want = e["ns"], e["xs"], e["want"]
    counts = [2 * (n // 4) for n in ns]
    d = dec_factory()
    t, ptrs = carve(torch_cuda, xs, 16)
    # a neighbour's samples lie right in front of a capture: where its silence is read
    assert any(p and p % 128 for p in ptrs)
    out = Outputs(torch_cuda, counts)
    assert d.power_batch_device(ptrs, ns, out.ptrs, out.caps) == sum(counts)
    out.check(want, "edges against the oracle")
    got = out.read()
    alone = single_calls(torch_cuda, d.power_device, ptrs, ns, counts)
    for i in range(len(ns)):
        assert np.array_equal(out.piece(got, i), alone[i]), (i, ns[i])


# ------------------------------------------------------------------ 2. batch sizes
@pytest.mark.limit(60)
def test_batch_sizes(capi, oracle, dec_factory, torch_cuda):
    """A batch of one; 300 captures of one pass each -- more rows than a bisection's first steps tell apart, whole waves and ragged
    ones mixed --; and a batch whose captures all have no power sample (NULL pointers and all): 0, nothing launched."""
    d = dec_factory()
    rng = np.random.default_rng(300)
    for ns in ([7172], [W - 4 * (i % 5) for i in range(300)]):
        xs = [rng.integers(0, 65536, n, dtype=np.uint16) for n in ns]
        counts = [2 * (n // 4) for n in ns]
        t, ptrs = carve(torch_cuda, xs, 16)
        out = Outputs(torch_cuda, counts)
        assert d.power_batch_device(ptrs, ns, out.ptrs, out.caps) == sum(counts)
        out.check([real_power(oracle, x) for x in xs], len(ns))
    out = Outputs(torch_cuda, [0, 0, 0, 0])
    assert d.power_batch_device([None, None, out.ptrs[2], None], [0, 1, 2, 3], [None, None, out.ptrs[2], None], [0, 0, 0, 0]) == 0
    assert out.untouched()
    assert d.power_batch_device([], [], [], []) == 0


# ------------------------------------------------------------------ 3. round the grid-stride loop
@pytest.mark.limit(120)
def test_second_trip_of_the_grid(capi, dec_factory, torch_cuda):
    """The grid is capped at 2048 workgroups of kWaves = 4 waves: 8192 passes a trip.  40 captures of about 768 Ki samples, ragged,
    are 40 x 220 = 8800 passes, so the first waves go round a second time, into other captures than their first trip's.  On the
    device against the loop of power_device; the oracle is not run at this size."""
    torch = torch_cuda
    rng = np.random.default_rng(40)
    ns = [768 * 1024 + int(v) for v in rng.integers(-2000, 2000, 40)]
    counts = [2 * (n // 4) for n in ns]
    assert sum(-(-k // 1792) for k in counts) > 2048 * 4 and any(k % 1792 for k in counts) and any(n % 4 for n in ns)
    xs = [rng.integers(0, 65536, n, dtype=np.uint16) for n in ns]
    d = dec_factory()
    t, ptrs = carve(torch, xs, 16)
    out = Outputs(torch, counts)
    assert d.power_batch_device(ptrs, ns, out.ptrs, out.caps) == sum(counts)
    want = torch.from_numpy(np.full(out.floats, SENT, np.uint32).view(np.uint8)).cuda()
    for p, n, k, o in zip(ptrs, ns, counts, out.at):
        assert d.power_device(p, n, want.data_ptr() + 4 * o, k) == k
    assert torch.equal(out.t.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ 4. the formats
def check_flavour(torch, d, batch_call, single_call, ptrs, ns, counts, wants, report):
    """One flavour: the batch call against the definition and against the loop of single calls, and the format report of each --
    `report` = (converted, inexact, clamped) of ONE pass over the captures."""
    d.reset()
    out = Outputs(torch, counts)
    assert batch_call(ptrs, ns, out.ptrs, out.caps) == sum(counts)
    out.check(wants, "against the definition")
    assert d.format_report() == report
    got = out.read()
    alone = single_calls(torch, single_call, ptrs, ns, counts)
    for i in range(len(ns)):
        assert np.array_equal(out.piece(got, i), alone[i]), (i, ns[i])
    assert d.format_report() == tuple(2 * v for v in report)        # the loop has counted exactly what the batch counted


@pytest.mark.limit(60)
def test_packed(capi, oracle, dec_factory, torch_cuda):
    from adsbdec_amd.packed12 import pack12
    rng = np.random.default_rng(12)
    ns = list(PACKED_LENGTHS)
    rng.shuffle(ns)
    xs = [rng.integers(0, 4096, n, dtype=np.uint16) for n in ns]
    d = dec_factory()
    t, ptrs = carve(torch_cuda, [pack12(x) if x.size else np.zeros(0, np.uint8) for x in xs], 4)
    check_flavour(torch_cuda, d, d.power_batch_device_packed, d.power_device_packed, ptrs, ns, [2 * (n // 4) for n in ns],
                  [real_power(oracle, x) for x in xs], (0, 0, 0))


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (3, 1, 4))
def test_converted(capi, oracle, dec_factory, torch_cuda, fmt):
    """fmt 3: every int16 value is legal, most are off the grid.  fmt 1: codes' own floats, floats off the grid, floats outside
    [-1, 1), NaN and Inf.  fmt 4: the uint16 call.  The report counts the samples of the captures that have power samples."""
    rng = np.random.default_rng(fmt)
    ns = list(AS_LENGTHS)
    rng.shuffle(ns)
    if fmt == 3:
        raw = [rng.integers(-32768, 32768, n).astype("<i2") for n in ns]
        conv = [S().from_int16_real(r) for r in raw]
    elif fmt == 1:
        raw = []
        for n in ns:
            r = S().to_float32_real(rng.integers(0, 4096, n, dtype=np.uint16))
            kind = rng.integers(0, 8, n)
            r[kind == 1] += np.float32(1e-4)
            r[kind == 2] *= np.float32(1.7)
            r[kind == 3] = np.float32("nan")
            r[(kind == 4) & (np.arange(n) % 2 == 0)] = np.float32("inf")
            raw.append(r.astype("<f4"))
        conv = [S().from_float32_real(r) for r in raw]
    else:
        raw = [rng.integers(0, 65536, n, dtype=np.uint16) for n in ns]
        conv = [(r, 0, 0) for r in raw]
    live = [n >= 4 for n in ns]
    report = (0, 0, 0) if fmt == 4 else tuple(sum(v for v, on in zip(col, live) if on)
                                              for col in (ns, [c[1] for c in conv], [c[2] for c in conv]))
    assert fmt == 4 or (report[1] > 0 and (fmt == 3 or report[2] > 0))
    d = dec_factory()
    t, ptrs = carve(torch_cuda, raw, 16 if fmt == 4 else raw[0].itemsize)
    assert fmt == 4 or any(p and p % 16 for p in ptrs)
    check_flavour(torch_cuda, d, lambda *a: d.power_batch_device_as(fmt, *a), lambda *a: d.power_device_as(fmt, *a), ptrs, ns,
                  [2 * (n // 4) for n in ns], [real_power(oracle, np.asarray(c[0], dtype=np.uint16)) for c in conv], report)


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (2, 0))
def test_iq(capi, dec_factory, torch_cuda, fmt):
    rng = np.random.default_rng(20 + fmt)
    ns = list(IQ_LENGTHS)
    rng.shuffle(ns)
    if fmt == 2:
        raw = [rng.integers(-32768, 32768, (n, 2)).astype("<i2") for n in ns]
        x16, report = raw, (0, 0, 0)
    else:
        raw = [(rng.random((n, 2)) * 2.4 - 1.2).astype("<f4") for n in ns]
        conv = [S().to_int16_iq(r) for r in raw]
        x16 = [c[0] for c in conv]
        report = (2 * sum(ns), sum(c[1] for c in conv), sum(c[2] for c in conv))
        assert report[1] > 0 and report[2] > 0
    wants = [S().iq_power(np.asarray(x, dtype="<i2").reshape(-1, 2)) if n else np.zeros(0, np.float32) for x, n in zip(x16, ns)]
    d = dec_factory()
    t, ptrs = carve(torch_cuda, raw, 4)
    assert any(p and p % 16 for p in ptrs)
    check_flavour(torch_cuda, d, lambda *a: d.power_batch_device_iq(fmt, *a), lambda *a: d.power_device_iq(fmt, *a), ptrs, ns, list(ns),
                  wants, report)


# ------------------------------------------------------------------ 5. the host flavour
@pytest.mark.limit(60)
def test_host_equals_device(capi, oracle, dec_factory, torch_cuda):
    e = edge_batch(oracle)
    d = dec_factory()
    got = d.power_batch(e["xs"])
    assert len(got) == len(e["xs"])
    for i, (g, w) in enumerate(zip(got, e["want"])):
        assert g.dtype == np.float32 and np.array_equal(bits(g), bits(w)), (i, e["ns"][i])


# ------------------------------------------------------------------ 6. composition: export a batch, decode the batch, in HBM
# every committed fixture, by the -a setting its records were made with; all inside the _power calls' domain (checked below)
COMPOSED = {True: ("dense_noise_256Ki", "mixed_df_a_384Ki", "odd_carry_base_a", "ragged_tail", "wide_codes_noise"),
            False: ("config1_1Mi_100xDF17", "mixed_df_noa_384Ki", "too_short")}


@pytest.mark.limit(60)
@pytest.mark.parametrize("df18", (True, False))
def test_export_then_decode_batch(capi, oracle, dec_factory, torch_cuda, df18):
    loaded = [load_golden(name) for name in COMPOSED[df18]]
    xs, recs = [x for x, _ in loaded], [rec for _, rec in loaded]
    for name, x, rec in zip(COMPOSED[df18], xs, recs):                   # on the CPU first
        assert rec["df18"] == df18 and S().power_domain_ok(real_power(oracle, x)), name
    ns = [x.size for x in xs]
    counts = [2 * (n // 4) for n in ns]
    d = dec_factory(df18=df18, collect_stats=True)
    t, ptrs = carve(torch_cuda, xs, 16)
    out = Outputs(torch_cuda, counts)
    assert d.power_batch_device(ptrs, ns, out.ptrs, out.caps) == sum(counts)
    frames, stats = d.decode_batch_device_power(out.ptrs, counts, stats=True)
    for i, (name, rec) in enumerate(zip(COMPOSED[df18], recs)):
        assert records(frames[i]) == golden_records(rec), name
        assert stats[i] == rec["stats"], name


# ------------------------------------------------------------------ 7. a stream in progress is not touched
@pytest.mark.limit(60)
def test_a_stream_in_progress_is_untouched(capi, oracle, dec_factory, torch_cuda):
    x, rec = load_golden("config1_1Mi_100xDF17")
    e = edge_batch(oracle)
    ns, xs = e["ns"][:12], e["xs"][:12]
    counts = [2 * (n // 4) for n in ns]
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptrs = carve(torch_cuda, xs, 16)
    d.reset()
    half = x.size // 2 + 3
    d.push(x[:half])
    out = Outputs(torch_cuda, counts)
    assert d.power_batch_device(ptrs, ns, out.ptrs, out.caps) == sum(counts)
    out.check(e["want"][:12], "between two pushes")
    got = d.power_batch(xs)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, e["want"][:12]))
    d.push(x[half:])
    d.finish()
    assert records(d.drain()) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 8. refusals
@pytest.mark.limit(60)
def test_refusals_write_nothing(capi, oracle, dec_factory, torch_cuda):
    """Every refusal once, by capture index: -1, a message that names the capture and the reason, every output float still the
    sentinel, the format report as it was -- and the next valid call succeeds.  None of these reaches a launch: every pointer that
    is passed is a valid one or is refused for its value alone."""
    rng = np.random.default_rng(8)
    ns = [64, 4096, 64]
    counts = [2 * (n // 4) for n in ns]
    xs = [rng.integers(0, 4096, n, dtype=np.uint16) for n in ns]
    d = dec_factory()
    d.reset()
    t, ptrs = carve(torch_cuda, xs, 16)
    out = Outputs(torch_cuda, counts)
    po, caps = out.ptrs, out.caps
    assert d.power_batch_device_as(3, ptrs, ns, po, caps) == sum(counts)  # (the report is not empty when the refusals begin)
    out = Outputs(torch_cuda, counts)
    po = out.ptrs
    before = d.format_report()
    assert before[0] == sum(ns)

    def sub(lst, i, v):
        return [v if k == i else a for k, a in enumerate(lst)]

    cases = [
        ("capture 1", "NULL", lambda: d.power_batch_device(sub(ptrs, 1, None), ns, po, caps)),
        ("capture 2", "NULL", lambda: d.power_batch_device(ptrs, ns, sub(po, 2, None), caps)),
        ("capture 1", "16-byte aligned", lambda: d.power_batch_device(sub(ptrs, 1, ptrs[1] + 8), sub(ns, 1, 4000), po, caps)),
        ("capture 2", "4-byte aligned", lambda: d.power_batch_device_iq(2, sub(ptrs, 2, ptrs[2] + 2), [8, 8, 8], po, caps)),
        ("capture 1", "power array must be 16-byte aligned", lambda: d.power_batch_device(ptrs, ns, sub(po, 1, po[1] + 4), sub(caps, 1, caps[1] - 1))),
        ("capture 1", "2^32", lambda: d.power_batch_device(ptrs, sub(ns, 1, 1 << 32), po, sub(caps, 1, 1 << 32))),
        ("capture 0", "2^31", lambda: d.power_batch_device_iq(2, ptrs, sub([8, 8, 8], 0, 1 << 31), po, sub(caps, 0, 1 << 32))),
        ("capture 1", "the array holds", lambda: d.power_batch_device(ptrs, ns, po, sub(caps, 1, caps[1] - 1))),
        ("capture 2", "the array holds", lambda: d.power_batch_device_iq(2, ptrs, [8, 8, 33], po, caps)),
        ("capture 1", "multiple of 8", lambda: d.power_batch_device_packed(ptrs, sub(ns, 1, 4092), po, caps)),
        ("capture 1", "4-byte aligned", lambda: d.power_batch_device_as(1, sub(ptrs, 1, ptrs[1] + 2), [16, 16, 16], po, caps)),
        ("capture 2", "2-byte aligned", lambda: d.power_batch_device_as(3, sub(ptrs, 2, ptrs[2] + 1), [16, 16, 16], po, caps)),
        ("", "not a real format", lambda: d.power_batch_device_as(0, ptrs, ns, po, caps)),
        ("", "not a real format", lambda: d.power_batch_device_as(2, ptrs, ns, po, caps)),
        ("", "unknown sample format", lambda: d.power_batch_device_as(7, ptrs, ns, po, caps)),
        ("", "not an IQ format", lambda: d.power_batch_device_iq(3, ptrs, [8, 8, 8], po, caps)),
        ("format 8", "not exported", lambda: d.power_batch_device_iq(8, ptrs, [8, 8, 8], po, caps)),
        ("captures", "32 bits", lambda: d._power_call("adsb_power_batch_device", (1 << 32) - 1, *d._power_batch_args(ptrs, ns, po, caps)[1:])),
    ]
    for who, why, call in cases:
        with pytest.raises(capi.AdsbError) as e:
            call()
        assert who in str(e.value) and why in str(e.value), (who, why, str(e.value))
        assert out.untouched(), (who, why)
        assert d.format_report() == before, (who, why)
    with pytest.raises(capi.AdsbError) as e:                               # the host flavour: the same rules but the alignments
        d._power_call("adsb_power_batch_host", *d._power_batch_args([x.ctypes.data for x in xs], ns, [None, None, None], caps))
    assert "capture 0" in str(e.value) and "NULL" in str(e.value)
    # and the handle still works
    assert d.power_batch_device(ptrs, ns, po, caps) == sum(counts)
    out.check([real_power(oracle, x) for x in xs], "after the refusals")
    assert d.format_report() == before
