"""The batch level report on the MI355X (run with -m gpu): level_batch_kernel / level_units_batch_kernel and every
adsb_level_batch_* call.  Capture i of a batch is held -- counts compared as integers, envelopes as uint32 -- to the report and the
envelope the single call of the same flavour gives for it alone, and to the definition: levels.level_report of oracle.power (the
restatement of air.c:54-91) or of sample_formats.iq_power, with levels.rails of the input codes.  The captures of a batch lie back to
back in ONE device allocation of full-range noise, so that a neighbour's samples lie where a capture's silence must be read, and the
envelopes lie in ONE sentinel-filled buffer with 64 guard floats between them, so that a float written past a capture's count
shows.  Every batch runs with the default grid and with adsb_debug_set_level_batch_blocks(1): four waves then share the batch and
each changes capture -- and flushes its histogram to the totals of the capture it held -- many times."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_records, load_golden, records
from test_gpu_level import COUNTERS, GUARD, SENT, LV, S, dev_env, planted_iq, want_iq, want_real
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)
from test_gpu_power_export_batch import AS_LENGTHS, IQ_LENGTHS, PACKED_LENGTHS, W, carve, edge_batch

pytestmark = pytest.mark.gpu

SENT64 = 0xA5A5A5A5A5A5A5A5


def runs(m):
    return -(-m // 28)


class Envs:
    """One device buffer of sentinels: GUARD floats, capture 0's envelope, GUARD floats, capture 1's ... and GUARD floats behind the
    last.  A capture with on[i] False, or without power samples, has no envelope: NULL and 0."""

    def __init__(self, torch, ms, on=None):
        on = [True] * len(ms) if on is None else list(on)
        self.counts = [runs(m) if o else 0 for m, o in zip(ms, on)]
        self.at, off = [], GUARD
        for k in self.counts:
            self.at.append(off)
            off += k + GUARD
        self.floats = off
        self.t = torch.from_numpy(np.full(off, SENT, np.uint32).view(np.uint8)).cuda()
        self.ptrs = [self.t.data_ptr() + 4 * o if k else None for o, k in zip(self.at, self.counts)]
        self.caps = list(self.counts)

    def read(self):
        return self.t.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.read() == SENT).all())

    def check(self, wants, how):
        """Every envelope is wants[i]["env"] bit for bit, and every other float of the buffer still holds the sentinel."""
        want = np.full(self.floats, SENT, np.uint32)
        for o, k, w in zip(self.at, self.counts, wants):
            if k:
                assert w["env"].size == k, how
                want[o: o + k] = w["env"].view(np.uint32)
        bad = np.flatnonzero(self.read() != want)
        assert bad.size == 0, (how, bad[:8], [i for i, o in enumerate(self.at) if o <= bad[0]][-1:])


def same(got, want, how):
    for key in COUNTERS:
        assert got[key] == want[key], (how, key, got[key], want[key])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), (how, np.flatnonzero(got["hist"] != want["hist"])[:8])
    assert int(got["hist"].sum()) + got["negative"] == got["samples"], how


def hold_batch(torch, d, batch_call, single_call, ptrs, ns, wants, on=None, report=None, how=""):
    """One flavour on one batch: the batch call against the definition (`wants`), against the loop of single calls -- reports,
    envelope bits, and where `report` = (converted, inexact, clamped) of ONE pass over the captures is given, the format report of
    each --, and against itself on one workgroup: four waves that change capture, and flush, many times."""
    ms = [w["samples"] for w in wants]
    envs = Envs(torch, ms, on)
    got = batch_call(ptrs, ns, envs.ptrs, envs.caps)
    assert len(got) == len(ns)
    for i, (g, w) in enumerate(zip(got, wants)):
        same(g, w, (how, "against the definition", i, ns[i]))
    envs.check(wants, (how, "against the definition"))
    counted = d.format_report()
    if report is not None:                                                # (None in a place: whatever the device counted there)
        assert all(r is None or r == c for r, c in zip(report, counted)), (how, report, counted)
    for i, (p, n, m) in enumerate(zip(ptrs, ns, ms)):
        te, pe, k = dev_env(torch, m if envs.counts[i] else 0)
        alone = single_call(p or 0, n, pe if k else 0, k)
        same(got[i], alone, (how, "against the single call", i, n))
        e = te.cpu().numpy().view(np.uint32)
        assert np.array_equal(e[:k], wants[i]["env"].view(np.uint32)[:k]) and (e[k:] == SENT).all(), (how, i, n)
    if report is not None:
        assert d.format_report() == tuple(2 * v for v in counted), how   # the loop has counted exactly what the batch counted
    d.set_level_batch_blocks(1)
    try:
        few = Envs(torch, ms, on)
        again = batch_call(ptrs, ns, few.ptrs, few.caps)
    finally:
        d.set_level_batch_blocks(0)
    for i, (g, a) in enumerate(zip(got, again)):
        same(a, g, (how, "one workgroup against the default grid", i, ns[i]))
    few.check(wants, (how, "one workgroup"))
    return got


# ------------------------------------------------------------------ 1. the edges of a wave and of a run, uint16
@pytest.mark.limit(60)
def test_edges_back_to_back(capi, oracle, dec_factory, torch_cuda):
    """The export batch test's EDGES in its seeded shuffled order with a zero-length capture between every two (its batch and its
    oracle power samples, computed once per session)."""
    e = edge_batch(oracle)
    ns, xs = e["ns"], e["xs"]
    wants = [want_real(oracle, x, a) for x, a in zip(xs, e["want"])]
    for x, w in zip(xs, wants):                                            # the statement of the issue, word for word
        ref = LV().with_rails(LV().level_report(oracle.power(x)[:2 * (x.size // 4)] if x.size >= 4 else np.zeros(0, np.float32)), x, "real")
        same(w, ref, "the definition")
    d = dec_factory()
    t, ptrs = carve(torch_cuda, xs, 16)
    assert any(p and p % 128 for p in ptrs)                                # a neighbour's samples lie right in front of a capture
    got = hold_batch(torch_cuda, d, d.level_batch_device, d.level_device, ptrs, ns, wants, how="edges")
    assert any(g["over"] for g in got) and sum(g["samples"] for g in got) == sum(2 * (n // 4) for n in ns)
    # no envelope at all: both arrays NULL
    for g, w in zip(d.level_batch_device(ptrs, ns), wants):
        same(g, w, "device_env == NULL")
    # a batch of one: three passes leave a wave of the workgroup without work; nine fill two workgroups whose four waves hold the
    # same capture at their end and leave as one sum -- on one workgroup, all nine passes
    for i in (ns.index(7172), ns.index(8 * W + 56)):
        hold_batch(torch_cuda, d, d.level_batch_device, d.level_device, ptrs[i: i + 1], ns[i: i + 1], wants[i: i + 1], how=("a batch of one", ns[i]))


# ------------------------------------------------------------------ 2. content that shows a leak between neighbours
def leak_batch():
    """About 40 captures of one to three passes side by side: silence (every increment of a pass on one bin: the run-uniform
    shortcut), clipped noise, all-4095, codes above 4095, and captures with n % 4 of 1, 2 and 3 whose trailing codes are 0, 4095 and
    65535 -- on the rails only if the batch counts them, and for the right capture."""
    rng = np.random.default_rng(2053)
    xs = []
    for i in range(8):
        n = (1 + i % 3) * W - 4 * (i % 4) + (0, 1, 2, 3, 0, 2, 1, 3)[i]
        silence = np.full(n, 0x800, np.uint16)
        clipped = np.clip(rng.normal(2048, 1500, n), 0, 4095).astype(np.uint16)
        top = np.full(n, 4095, np.uint16)
        wide = rng.integers(4000, 65536, n, dtype=np.uint16)
        tails = rng.integers(1, 4095, n + 4 - n % 4 + 1 + i % 3, dtype=np.uint16)       # n % 4 of 1, 2, 3 in turn
        tails[4 * (tails.size // 4):] = (0, 4095, 65535)[: tails.size % 4]
        xs += [silence, clipped, top, wide, tails]
    return xs


@pytest.mark.limit(60)
def test_neighbours_do_not_leak(capi, oracle, dec_factory, torch_cuda):
    xs = leak_batch()
    ns = [x.size for x in xs]
    assert len(xs) == 40 and {n % 4 for n in ns} == {0, 1, 2, 3} and all(1 <= -(-(2 * (n // 4)) // 1792) <= 3 for n in ns)
    wants = [want_real(oracle, x) for x in xs]
    # what a leak would change: silence is one bin and no rail; all-4095 is all rail_hi; the trailing codes count once each
    assert int(wants[0]["hist"][0]) == wants[0]["samples"] and wants[0]["rail_lo"] == wants[0]["rail_hi"] == 0
    assert wants[2]["rail_hi"] == ns[2] and wants[3]["over"] > 0 and wants[3]["rail_lo"] == 0
    assert (wants[4]["rail_lo"], wants[4]["rail_hi"], wants[4]["over"]) == (1, 0, 0)
    assert (wants[9]["rail_lo"], wants[9]["rail_hi"], wants[9]["over"]) == (1, 1, 0)
    assert (wants[14]["rail_lo"], wants[14]["rail_hi"], wants[14]["over"]) == (1, 1, 1)
    d = dec_factory()
    t, ptrs = carve(torch_cuda, xs, 16)
    on = [i % 3 != 1 for i in range(len(xs))]                              # captures with and without an envelope in one batch
    hold_batch(torch_cuda, d, d.level_batch_device, d.level_device, ptrs, ns, wants, on=on, how="content")
    for blocks in (1, 0):                                                  # and with device_env == NULL, on both grids
        d.set_level_batch_blocks(blocks)
        for g, w in zip(d.level_batch_device(ptrs, ns), wants):
            same(g, w, ("device_env == NULL", blocks))


# ------------------------------------------------------------------ 3. more captures than a launch takes
@pytest.mark.limit(60)
def test_sub_batches(capi, oracle, dec_factory, torch_cuda):
    """1100 captures of 0 .. 130 samples: a sub-batch of 1024 and one of 76, each its own table, totals and launch; the reports land
    at the right index of out[] across the seam."""
    rng = np.random.default_rng(1100)
    ns = [int(v) for v in rng.integers(0, 131, 1100)]
    xs = [rng.integers(0, 65536, n, dtype=np.uint16) for n in ns]
    wants = [want_real(oracle, x) for x in xs]
    d = dec_factory()
    t, ptrs = carve(torch_cuda, xs, 16)
    ms = [w["samples"] for w in wants]
    envs = Envs(torch_cuda, ms)
    got = d.level_batch_device(ptrs, ns, envs.ptrs, envs.caps)
    for i, (g, w) in enumerate(zip(got, wants)):
        same(g, w, ("sub-batches", i, ns[i]))
    envs.check(wants, "sub-batches")
    for i in (0, 1023, 1024, 1099):
        same(got[i], d.level_device(ptrs[i] or 0, ns[i]), ("against the single call", i))


# ------------------------------------------------------------------ 4. the other flavours
@pytest.mark.limit(60)
def test_packed(capi, oracle, dec_factory, torch_cuda):
    from adsbdec_amd.packed12 import pack12
    rng = np.random.default_rng(12)
    ns = list(PACKED_LENGTHS) + [W + 8, 2 * W]
    rng.shuffle(ns)
    xs = [np.clip(rng.normal(2048, 1200, n), 0, 4095).astype(np.uint16) for n in ns]
    d = dec_factory()
    d.reset()
    t, ptrs = carve(torch_cuda, [pack12(x) if x.size else np.zeros(0, np.uint8) for x in xs], 4)
    assert any(p and p % 16 for p in ptrs)
    got = hold_batch(torch_cuda, d, d.level_batch_device_packed, d.level_device_packed, ptrs, ns, [want_real(oracle, x) for x in xs],
                     report=(0, 0, 0), how="packed")
    assert sum(g["rail_lo"] for g in got) > 0 and sum(g["rail_hi"] for g in got) > 0


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (3, 1, 4))
def test_converted(capi, oracle, dec_factory, torch_cuda, fmt):
    """fmt 3: every int16 value is legal, most are off the grid.  fmt 1: codes' own floats, floats off the grid, floats outside
    [-1, 1), NaN and Inf.  fmt 4: forwarded to the uint16 call.  The rails are those of the CONVERTED codes, the trailing n % 4 too;
    the format report counts the samples of the captures that have power samples, as the loop of single calls leaves it."""
    rng = np.random.default_rng(fmt)
    ns = list(AS_LENGTHS) + [W + 1, W + 2, 2 * W + 3]
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
    d.reset()
    t, ptrs = carve(torch_cuda, raw, 16 if fmt == 4 else raw[0].itemsize)
    assert fmt == 4 or any(p and p % 16 for p in ptrs)
    wants = [want_real(oracle, np.asarray(c[0], dtype=np.uint16)) for c in conv]
    hold_batch(torch_cuda, d, lambda *a: d.level_batch_device_as(fmt, *a), lambda *a: d.level_device_as(fmt, *a), ptrs, ns, wants,
               report=report, how=("as", fmt))


IQ_NS = IQ_LENGTHS + [27, 28, 29, 1791, 1792, 1793, 2 * 1792 + 5]


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (2, 0, 8))
def test_iq(capi, dec_factory, torch_cuda, fmt):
    """Lengths around a run (28) and a pass (1792), rails planted (fmt 0: floats clamped onto them); pointers aligned to the sample
    and no more -- fmt 8: 2 bytes, not 8, so the unit-by-unit road and the 8-byte road are both taken in one batch."""
    rng = np.random.default_rng(20 + fmt)
    ns = list(IQ_NS)
    rng.shuffle(ns)
    raw = [planted_iq(fmt, n, 80 + i) if n else np.zeros((0, 2), {8: np.int8, 2: np.int16, 0: np.float32}[fmt]) for i, n in enumerate(ns)]
    wants = [want_iq(x, fmt) if n else LV().level_report(np.zeros(0, np.float32)) for x, n in zip(raw, ns)]
    report = (0, 0, 0)
    if fmt == 0:
        report = (2 * sum(ns), None, None)                                   # (the planted floats hold Inf: the counts are the loop's)
    d = dec_factory()
    d.reset()
    align = 2 if fmt == 8 else 4
    t, ptrs = carve(torch_cuda, raw, align)
    assert any(p and p % (4 * align) for p in ptrs) and any(p and p % (4 * align) == 0 for p in ptrs)
    got = hold_batch(torch_cuda, d, lambda *a: d.level_batch_device_iq(fmt, *a), lambda *a: d.level_device_iq(fmt, *a), ptrs, ns, wants,
                     report=report, how=("iq", fmt))
    assert sum(g["rail_lo"] for g in got) > 0 and sum(g["rail_hi"] for g in got) > 0 and not any(g["over"] for g in got)


@pytest.mark.limit(60)
def test_power_input(capi, dec_factory, torch_cuda):
    """float32 power samples inside and outside the _power domain: negatives, -0.0, NaN, Inf and subnormals planted capture by
    capture, so that a count in a neighbour's report shows; a capture that holds only negatives has a zero envelope."""
    rng = np.random.default_rng(77)
    ns = list(IQ_NS)
    rng.shuffle(ns)
    plants = ([np.float32(-3.0)], [np.float32(-0.0)], [np.float32(np.nan)], [np.float32(np.inf), np.float32(-np.inf)],
              list(np.array([1, 0x007FFFFF], "<u4").view("<f4")), [])
    raw = []
    for i, n in enumerate(ns):
        a = rng.uniform(0.0, 1.0e6, n).astype("<f4")
        vals = plants[i % len(plants)][:n]
        if vals:
            a[rng.choice(n, size=len(vals), replace=False)] = vals
        raw.append(a)
    whole = max(range(len(ns)), key=lambda i: ns[i])
    raw[whole] = -np.abs(raw[whole]) - np.float32(1.0)                     # every sample negative
    wants = [LV().level_report(a) for a in raw]
    assert wants[whole]["negative"] == ns[whole] and not wants[whole]["env"].view(np.uint32).any()
    assert sum(w["negative"] for w in wants) > ns[whole] and any(w["hist"][2040:].any() for w in wants) and any(w["hist"][:8].sum() > 0 for w in wants)
    d = dec_factory()
    t, ptrs = carve(torch_cuda, raw, 4)
    assert any(p and p % 16 for p in ptrs)
    got = hold_batch(torch_cuda, d, d.level_batch_device_power, d.level_device_power, ptrs, ns, wants, how="power")
    assert all(g["rail_lo"] == g["rail_hi"] == g["over"] == 0 for g in got)
    assert [LV().domain_ok(g) for g in got] == [bool(S().power_domain_ok(a)) for a in raw]


@pytest.mark.limit(60)
def test_host_equals_device(capi, oracle, dec_factory, torch_cuda):
    """adsb_level_batch_host on the edge batch and on the content batch (whose trailing codes the call counts from the caller's
    memory): reports and envelopes are the definition's and adsb_level_host's."""
    e = edge_batch(oracle)
    xs = e["xs"] + leak_batch()[:10]
    wants = [want_real(oracle, x, a) for x, a in zip(e["xs"], e["want"])] + [want_real(oracle, x) for x in xs[len(e["xs"]):]]
    d = dec_factory()
    got = d.level_batch(xs)
    assert len(got) == len(xs)
    for i, (g, w) in enumerate(zip(got, wants)):
        same(g, w, ("host", i, xs[i].size))
        assert g["env"].dtype == np.float32 and np.array_equal(g["env"].view(np.uint32), w["env"].view(np.uint32)), i
    for i in (0, 2, len(e["xs"]) + 4, len(e["xs"]) + 9):
        alone = d.level(xs[i])
        same(got[i], alone, ("against adsb_level_host", i))
        assert np.array_equal(got[i]["env"].view(np.uint32), alone["env"].view(np.uint32))
    for g, w in zip(d.level_batch(xs, env=False), wants):
        same(g, w, "host, no envelope")
        assert "env" not in g


# ------------------------------------------------------------------ 5. a stream in progress is not touched
@pytest.mark.limit(60)
def test_a_stream_in_progress_is_untouched(capi, oracle, dec_factory, torch_cuda):
    x, rec = load_golden("config1_1Mi_100xDF17")
    e = edge_batch(oracle)
    ns, xs = e["ns"][:12], e["xs"][:12]
    wants = [want_real(oracle, y, a) for y, a in zip(xs, e["want"][:12])]
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptrs = carve(torch_cuda, xs, 16)
    d.reset()
    half = x.size // 2 + 3
    d.push(x[:half])
    envs = Envs(torch_cuda, [w["samples"] for w in wants])
    for g, w in zip(d.level_batch_device(ptrs, ns, envs.ptrs, envs.caps), wants):
        same(g, w, "between two pushes")
    envs.check(wants, "between two pushes")
    for g, w in zip(d.level_batch(xs), wants):
        same(g, w, "the host call between two pushes")
    d.push(x[half:])
    d.finish()
    assert records(d.drain()) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.limit(60)
def test_refusals_write_nothing(capi, oracle, dec_factory, torch_cuda):
    """Every refusal once, by capture index: -1, a message that names the capture and the reason, every word of out[] and every
    envelope float as it was, the format report as it was -- and the next valid call succeeds.  None of these reaches a launch: every
    pointer that is passed is a valid one or is refused for its value alone."""
    rng = np.random.default_rng(8)
    ns = [64, 4096, 64]
    xs = [rng.integers(0, 4096, n, dtype=np.uint16) for n in ns]
    ms = [2 * (n // 4) for n in ns]
    d = dec_factory()
    d.reset()
    t, ptrs = carve(torch_cuda, xs, 16)
    first = Envs(torch_cuda, ms)
    assert len(d.level_batch_device_as(3, ptrs, ns, first.ptrs, first.caps)) == 3   # (the report is not empty when the refusals begin)
    before = d.format_report()
    assert before[0] == sum(ns)
    envs = Envs(torch_cuda, ns)                                                        # room for every flavour's M
    pe, caps = envs.ptrs, envs.caps
    out = (capi.LevelReport * 3)()
    C.memset(C.addressof(out), 0xA5, C.sizeof(out))
    words = np.ctypeslib.as_array((C.c_uint64 * (3 * (5 + 2048))).from_buffer(out))

    def sub(lst, i, v):
        return [v if k == i else a for k, a in enumerate(lst)]

    def raw(name, *args):
        if getattr(capi.load(), name)(d._h, *args) < 0:
            d._check(-1, name)

    arr = lambda typ, vals: (typ * len(vals))(*vals)
    P, N = arr(C.c_void_p, ptrs), arr(C.c_size_t, ns)
    B = d.level_batch_device
    cases = [
        ("capture 1", "NULL buffer", lambda: B(sub(ptrs, 1, None), ns, pe, caps, out=out)),
        ("capture 1", "16-byte aligned", lambda: B(sub(ptrs, 1, ptrs[1] + 8), sub(ns, 1, 4000), pe, caps, out=out)),
        ("capture 2", "4-byte aligned", lambda: d.level_batch_device_iq(2, sub(ptrs, 2, ptrs[2] + 2), [8, 8, 8], pe, caps, out=out)),
        ("capture 2", "4-byte aligned", lambda: d.level_batch_device_iq(0, sub(ptrs, 2, ptrs[2] + 2), [8, 8, 4], pe, caps, out=out)),
        ("capture 0", "2-byte aligned", lambda: d.level_batch_device_iq(8, sub(ptrs, 0, ptrs[0] + 1), [8, 8, 8], pe, caps, out=out)),
        ("capture 1", "4-byte aligned", lambda: d.level_batch_device_power(sub(ptrs, 1, ptrs[1] + 2), [8, 8, 8], pe, caps, out=out)),
        ("capture 1", "4-byte aligned", lambda: d.level_batch_device_packed(sub(ptrs, 1, ptrs[1] + 2), [8, 8, 8], pe, caps, out=out)),
        ("capture 1", "4-byte aligned", lambda: d.level_batch_device_as(1, sub(ptrs, 1, ptrs[1] + 2), [16, 16, 16], pe, caps, out=out)),
        ("capture 2", "2-byte aligned", lambda: d.level_batch_device_as(3, sub(ptrs, 2, ptrs[2] + 1), [16, 16, 16], pe, caps, out=out)),
        ("capture 1", "2^32", lambda: B(ptrs, sub(ns, 1, 1 << 32), None, None, out=out)),
        ("capture 1", "2^32", lambda: d.level_batch_device_packed(ptrs, sub(ns, 1, 1 << 32), None, None, out=out)),
        ("capture 0", "2^31", lambda: d.level_batch_device_iq(2, ptrs, sub([8, 8, 8], 0, 1 << 31), None, None, out=out)),
        ("capture 0", "2^31", lambda: d.level_batch_device_iq(8, ptrs, sub([8, 8, 8], 0, 1 << 31), None, None, out=out)),
        ("capture 2", "2^31", lambda: d.level_batch_device_power(ptrs, sub([8, 8, 8], 2, 1 << 31), None, None, out=out)),
        ("capture 1", "multiple of 8", lambda: d.level_batch_device_packed(ptrs, sub(ns, 1, 4092), pe, caps, out=out)),
        ("capture 1", "the array holds", lambda: B(ptrs, ns, pe, sub(caps, 1, runs(ms[1]) - 1), out=out)),
        ("capture 2", "the array holds", lambda: d.level_batch_device_iq(2, ptrs, [8, 8, 33], pe, sub(caps, 2, 1), out=out)),
        ("capture 0", "the array holds", lambda: raw("adsb_level_batch_device", 3, P, N, out, arr(C.c_void_p, pe), arr(C.c_size_t, sub(caps, 0, 0)))),
        ("capture 2", "NULL envelope", lambda: raw("adsb_level_batch_device", 3, P, N, out, arr(C.c_void_p, sub(pe, 2, None)), arr(C.c_size_t, caps))),
        ("capture 1", "envelope must be 4-byte aligned", lambda: B(ptrs, ns, sub(pe, 1, pe[1] + 2), caps, out=out)),
        ("", "both NULL", lambda: raw("adsb_level_batch_device", 3, P, N, out, arr(C.c_void_p, pe), None)),
        ("", "NULL capture arrays", lambda: raw("adsb_level_batch_device", 3, None, N, out, None, None)),
        ("", "NULL capture arrays", lambda: raw("adsb_level_batch_device_power", 3, P, None, out, None, None)),
        ("", "NULL reports", lambda: raw("adsb_level_batch_device", 3, P, N, None, arr(C.c_void_p, pe), arr(C.c_size_t, caps))),
        ("", "not a real format", lambda: d.level_batch_device_as(0, ptrs, ns, pe, caps, out=out)),
        ("", "not a real format", lambda: d.level_batch_device_as(2, ptrs, ns, pe, caps, out=out)),
        ("", "unknown sample format", lambda: d.level_batch_device_as(7, ptrs, ns, pe, caps, out=out)),
        ("", "not an IQ format", lambda: d.level_batch_device_iq(3, ptrs, [8, 8, 8], pe, caps, out=out)),
        ("captures", "32 bits", lambda: raw("adsb_level_batch_device", (1 << 32) - 1, P, N, out, None, None)),
        ("capture 0", "NULL buffer", lambda: raw("adsb_level_batch_host", 3, arr(C.c_void_p, [None, None, None]), N, out, None, None)),
        ("capture 1", "2^32", lambda: raw("adsb_level_batch_host", 3, arr(C.c_void_p, [x.ctypes.data for x in xs]),
                                         arr(C.c_size_t, sub(ns, 1, 1 << 32)), out, None, None)),
    ]
    for who, why, call in cases:
        with pytest.raises(capi.AdsbError) as e:
            call()
        assert who in str(e.value) and why in str(e.value), (who, why, str(e.value))
        assert (words == SENT64).all(), (who, why)
        assert envs.untouched(), (who, why)
        assert d.format_report() == before, (who, why)
    # no power samples: zeroed reports, NULL pointers allowed, nothing launched; an empty batch; and the handle still works
    got = B([None, None, ptrs[2]], [0, 3, 2], [None, None, None], [0, 0, 0], out=out)
    assert all(g[key] == 0 for g in got for key in COUNTERS) and not any(g["hist"].any() for g in got) and not words.any()
    assert d.level_batch_device_iq(8, [None], [0])[0]["samples"] == 0 and d.level_batch_device_power([None], [0])[0]["samples"] == 0
    assert B([], []) == [] and d.level_batch([]) == []
    assert envs.untouched() and d.format_report() == before
    wants = [want_real(oracle, x) for x in xs]
    for g, w in zip(B(ptrs, ns, pe, [runs(m) for m in ms]), wants):
        same(g, w, "after the refusals")
    assert d.format_report() == before
