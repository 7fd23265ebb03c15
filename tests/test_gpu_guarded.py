"""Device calls held to the oracle from guarded, separate buffers (run with -m gpu on an MI355X).  Everywhere else in the suite the
memory around what a call is given is the stream's true continuation, the allocator's quiet pages or the same capture again, so a
kernel or a launch bound that read a few pairs outside [p, p + n) would read the right data or silence.  Here it reads a decoy:

1. pieces of one stream, each in a tensor of its own between 8192 units of ANOTHER frame-carrying capture, with frames planted
   across and directly behind every cut (tests/guarded_cases.py), in place and staged, through all eight fronts and two handles;
2. the edge captures of the neighbouring modules (a frame from sample 0 on), decoded as a stream from their loud buffers;
3. a handle whose scratch, staging and landing buffers hold a louder, four times longer capture when the target arrives -- and
   whose batch buffers, tables and totals hold a loud batch when a batch of targets arrives;
4. whole-capture exports and level reports of captures that lie inside loud memory with both rails planted in the guards.

Every comparison is equality with the oracle.  tests/test_guarded_cpu.py proves without a device that each guard can be seen.
Every test allocates all the memory it lets a kernel touch: the guards are part of the tensors."""
import numpy as np
import pytest

import front_records_cases as F
import guarded_cases as G
import iq8_cases as Q
from conftest import records
from test_gpu_batch_records import EDGES, _edge_capture, device, host, torch_cuda  # noqa: F401  (fixtures)
from test_gpu_candidates import _scan
from test_gpu_level import check as check_level, dev_env, want_iq, want_real, planted_iq
from test_gpu_batch_packed import packable
from test_gpu_power_export import check_out, dev_out

# measured on an MI355X (profiles/r25_guarded_tests.txt): no call above 0.35 s; the limit of 60 s each is that ten times over, rounded up to
# 30 s, and a step further for whichever test runs first and pays the build of the library from source (28 s)
pytestmark = pytest.mark.gpu

HANDLES = {
    "stats": dict(df18=True, collect_stats=True),
    "k2_nostats": dict(df18=True, collect_stats=False, debug_passes=2),     # the other Stage B: small tiles, many tile starts a piece
}


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def LV():
    from adsbdec_amd import levels
    return levels


def to_dev(torch, b, lead):
    """Bytes on the device -> (the tensor that keeps them, the pointer `lead` bytes in)."""
    t = torch.from_numpy(np.ascontiguousarray(b).view(np.uint8).reshape(-1)).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + lead


def check_stats(got, want, collect, where):
    assert got["ok"] == want["ok"], where
    if collect:
        assert got["try"] == want["try"], where


# ---------------------------------------------------------------- the calls of a front
def push(d, front, ptr, n, final):
    _, family, fmt = G.FRONTS[front]
    if family == "real":
        (d.push_device_final if final else d.push_device)(ptr, n)
    elif family == "as":
        d.push_device_as(fmt, ptr, n, final)
    elif family == "packed":
        (d.push_device_packed_final if final else d.push_device_packed)(ptr, n)
    elif family == "iq":
        d.push_device_iq(fmt, ptr, n, final)
    else:
        d.push_device_power(ptr, n, final)


def decode_whole(capi, d, front, ptr, n):
    _, family, fmt = G.FRONTS[front]
    if family == "real":
        return capi._frames_to_dicts(*d.decode_device_raw(ptr, n))
    if family == "as":
        return d.decode_device_as(fmt, ptr, n)
    if family == "packed":
        return capi._frames_to_dicts(*d.decode_device_packed_raw(ptr, n))
    if family == "iq":
        return d.decode_device_iq(fmt, ptr, n)
    return d.decode_device_power(ptr, n)


def converts(front):
    return front in ("s16", "f32", "iqf32")


# ---------------------------------------------------------------- 1. pieces of one stream, each in a buffer of its own
_pieces = {}


def pieces(torch, front):
    """{"forward" | "reversed": [(tensor, pointer, n, final)], "whole": (tensor, pointer, n)} of a front, made once: every piece
    and the whole capture between GUARD units of the decoy on either side, the piece 16-byte aligned."""
    if front not in _pieces:
        s = G.stream(G.FRONTS[front][0])
        out = {}
        for order, sizes in (("forward", s.sizes), ("reversed", s.sizes[::-1])):
            out[order] = []
            for at, n, _, final in G.roads(sizes):
                b, lead = G.guarded(front, s, at, at + n)
                t, ptr = to_dev(torch, b, lead)
                assert ptr % 16 == 0
                out[order].append((t, ptr, G.count_of(front, n), final))
        b, lead = G.guarded(front, s, 0, G.TOTAL)
        t, ptr = to_dev(torch, b, lead)
        out["whole"] = (t, ptr, G.count_of(front, G.TOTAL))
        _pieces[front] = out
    return _pieces[front]


@pytest.mark.limit(60)
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("front", list(G.FRONTS))
def test_pieces_in_buffers_of_their_own(capi, torch_cuda, front, handle):
    """Six device pushes of one stream -- in place at the minimum, in place behind a seam copy, staged because short, staged because
    it starts at 4 mod 8, in place to the exact end with _final -- in this order and reversed, each piece in a tensor of its own
    between stretches of a decoy capture: the frames and the Try/Ok table are the oracle's of the whole capture, every piece took
    the road guarded_cases.roads names, the launches evaluated every offset exactly once, the format report counts what was
    converted, and the same handle then decodes the whole capture in one call to the same answer."""
    s = G.stream(G.FRONTS[front][0])
    want, kw = records(s.frames), HANDLES[handle]
    assert len(want) > 60
    report = (G.TOTAL, 0, 0) if converts(front) else (0, 0, 0)
    p = pieces(torch_cuda, front)
    d = capi.Decoder(**kw)
    try:
        for order in ("forward", "reversed"):
            d.reset()
            got, before = [], d.profile()
            sizes = s.sizes if order == "forward" else s.sizes[::-1]
            for (_, ptr, n, final), (at, _, road, _) in zip(p[order], G.roads(sizes)):
                launches = d.profile()["launches"]
                push(d, front, ptr, n, final)
                got += d.drain()
                # the road the piece took: an in-place push behind earlier data scans the seam from the staging buffer and the
                # bulk where it lies, a staged push and the stream's first one scan once
                assert d.profile()["launches"] - launches == (2 if road == "in_place" and at else 1), (front, handle, order, at, road)
            where = (front, handle, order)
            after = d.profile()
            # every offset of the stream was evaluated, by exactly one launch: no piece reported offsets beyond what it could scan
            assert after["offsets"] - before["offsets"] == s.n_off and after["relaunches"] == before["relaunches"], where
            assert records(got) == want, (where, len(got), len(want), sorted(set(records(got)) ^ set(want))[:4])
            check_stats(d.stats(), s.stats, kw["collect_stats"], where)
            assert d.format_report() == report, where
        _, ptr, n = p["whole"]
        where = (front, handle, "whole")
        assert records(decode_whole(capi, d, front, ptr, n)) == want, where
        check_stats(d.stats(), s.stats, kw["collect_stats"], where)
        assert d.format_report() == report, where
    finally:
        d.close()


# ---------------------------------------------------------------- 2. a stream that starts behind a loud guard
def _loud_twin(torch, front, x, seed):
    """A real capture's twin of a front between 64 loud codes on either side -> (tensor, pointer)."""
    flat = np.concatenate([G.loud_codes(G.LOUD_GUARD, seed), x, G.loud_codes(G.LOUD_GUARD, seed + 1)])
    t, ptr = to_dev(torch, G.as_front(front, flat), int(G.LOUD_GUARD * G.unit_bytes(front)))
    assert ptr % 16 == 0
    return t, ptr


def _stream_both_ways(capi, d, front, ptr, n, want, where):
    """decode_device* and one push_device*_final of the same memory: the frames and the table."""
    wf, ws = want
    assert records(decode_whole(capi, d, front, ptr, n)) == records(wf), (where, "decode_device")
    check_stats(d.stats(), ws, True, (where, "decode_device"))
    d.reset()
    push(d, front, ptr, n, True)
    assert records(d.drain()) == records(wf), (where, "push_device_final")
    check_stats(d.stats(), ws, True, (where, "push_device_final"))


@pytest.mark.limit(60)
@pytest.mark.parametrize("all_candidates", (True, False), ids=("all_candidates", "default"))
def test_real_edge_captures_decoded_behind_a_loud_guard(capi, oracle, host, device, torch_cuda, all_candidates):
    """The five real edge captures (n % 4 = 0, 1, 2, 3, 0; a frame from sample 0 on, whose candidates at g = 3 .. 6 read the six power
    samples the pre-halo makes) through scan_kernel as a STREAM, from the buffer in which loud codes lie directly in front of
    them: silence is what the call must read there.  The int16, float32 and packed twins from loud buffers of their own."""
    _, ptrs = device
    d = capi.Decoder(df18=True, collect_stats=True, all_candidates=all_candidates)
    try:
        for i, name in enumerate(EDGES):
            x, _, dec = host[name]
            want = dec[(True, False)]
            assert len(want[0]) >= 1 and want[0][0]["g"] == 3
            _stream_both_ways(capi, d, "u16", ptrs[name], x.size, want, name)
            for front in ("s16", "f32"):
                t, ptr = _loud_twin(torch_cuda, front, x, 8300 + i)
                _stream_both_ways(capi, d, front, ptr, x.size, want, (name, front))
                assert d.format_report() == (x.size, 0, 0)
            x8 = packable(x)
            t, ptr = _loud_twin(torch_cuda, "packed", x8, 8300 + i)
            _stream_both_ways(capi, d, "packed", ptr, x8.size, oracle.decode(x8, df18=True), (name, "packed"))
    finally:
        d.close()


@pytest.mark.limit(60)
@pytest.mark.parametrize("all_candidates", (True, False), ids=("all_candidates", "default"))
@pytest.mark.parametrize("front", ("iq16", "iqf32", "iq8", "power"))
def test_edge_captures_of_the_other_fronts_behind_a_loud_guard(capi, torch_cuda, front, all_candidates):
    """The five edge captures of the IQ, int8 IQ and power front ends through their stream kernels, in place from the loud buffers of
    tests/test_gpu_front_records.py and tests/test_gpu_iq8.py: candidates at the very first offsets, loud samples right in front."""
    import test_gpu_front_records as R
    import test_gpu_iq8 as R8
    if front == "iq8":
        cases, (_, ptrs) = Q.cases(), R8.device(torch_cuda)
    else:
        cases = F.cases("power" if front == "power" else "iq")
        _, ptrs = R.device(torch_cuda, {"iq16": "iq", "iqf32": "iq_f32", "power": "power"}[front])
    d = capi.Decoder(df18=True, collect_stats=True, all_candidates=all_candidates)
    try:
        for name in EDGES:
            c = cases[name]
            want = c.dec[(True, False)]
            assert len(want[0]) >= 1 and want[0][0]["g"] == 0
            _stream_both_ways(capi, d, front, ptrs[name], c.n, want, (front, name))
            assert d.format_report() == ((2 * c.n, 0, 0) if front == "iqf32" else (0, 0, 0))
    finally:
        d.close()


# ---------------------------------------------------------------- 3. a handle whose buffers hold a louder, longer capture
N_AROUND = G.N_AROUND                             # 70 000: the lengths n .. n + 7 of the packed and quad classes: above the in-place minimum
_stale = {}


def stale_cases(oracle):
    """Real: the loud capture (full-range codes, never 0x800, four times the longest target) and the targets -- the edge capture of
    n % 4 = 1 and eight captures of 70 000 .. 70 007 samples -- with the oracle's answers.  Complex: the same for float32 IQ."""
    if not _stale:
        edge = _edge_capture(1)
        base = _edge_capture(2)
        targets = [edge] + [np.ascontiguousarray(base[:N_AROUND + j]) for j in range(8)]
        _stale["loud"] = G.loud_codes(4 * edge.size + 8 - (4 * edge.size) % 8, 8400)
        _stale["real"] = [(x, oracle.decode(x, df18=True), oracle.power(x)) for x in targets]
        # (packed input comes in whole groups: the edge capture cut to one, and the two lengths around 70 000 that are multiples of 8)
        _stale["packed"] = [(x, oracle.decode(x, df18=True), oracle.power(x))
                            for x in (packable(edge), np.ascontiguousarray(base[:N_AROUND]), np.ascontiguousarray(base[:N_AROUND + 8]))]
        iq_edge = F._iq_edge(1)
        iq_targets = [iq_edge] + [np.ascontiguousarray(F._iq_edge(2)[:N_AROUND // 2 + j]) for j in range(4)]
        _stale["loud_iq"] = G.loud_iq(0, 4 * len(iq_edge), 8401)
        _stale["iq"] = [(x, oracle.demod_power(S().iq_power(x), df18=True), S().iq_power(x)) for x in iq_targets]
        assert all(_stale["loud"].size >= 4 * x.size for x, _, _ in _stale["real"]) and G.never_silence(_stale["loud"])
        assert all(len(_stale["loud_iq"]) >= 4 * len(x) for x, _, _ in _stale["iq"]) and G.never_silence(_stale["loud_iq"])
        assert len(_stale["real"][0][1][0]) >= 1 and len(_stale["iq"][0][1][0]) >= 1
    return _stale


def _fresh_and_used(capi, kw, dirty, run, targets, where):
    """One handle per road: `dirty` fills its buffers with the loud capture, then every target through `run` gives the oracle's
    answer -- and what a fresh handle gives."""
    used = capi.Decoder(**kw)
    try:
        dirty(used)
        for j, (x, want, _) in enumerate(targets):
            got = run(used, x)
            assert records(got[0]) == records(want[0]), (where, j, "behind the loud capture")
            check_stats(got[1], want[1], True, (where, j))
            fresh = capi.Decoder(**kw)
            try:
                again = run(fresh, x)
            finally:
                fresh.close()
            assert (records(again[0]), again[1]) == (records(got[0]), got[1]), (where, j, "a fresh handle")
    finally:
        used.close()


@pytest.mark.limit(60)
@pytest.mark.parametrize("mode", ("sync", "async"))
def test_host_pushes_into_staging_that_held_a_loud_capture(capi, oracle, torch_cuda, mode):
    """stage[] and land[] of a handle with a 64 Ki staging buffer: the loud capture goes through (compacting at every piece), the
    stream is reset, and the targets follow in chunks of 30 001 -- as uint16 and, for land[], as int16 real."""
    c = stale_cases(oracle)
    kw = dict(df18=True, collect_stats=True, stage_samples=1 << 16)

    def run_u16(d, x):
        return d.decode(x, chunk=30_001, mode=mode), d.stats()

    def run_s16(d, x):
        return d.decode_as(3, S().to_int16_real(x), chunk=30_001, mode=mode), d.stats()

    _fresh_and_used(capi, kw, lambda d: d.decode(c["loud"], chunk=50_000, mode=mode), run_u16, c["real"], ("push", mode))
    _fresh_and_used(capi, kw, lambda d: d.decode_as(3, S().to_int16_real(c["loud"]), chunk=50_000, mode=mode), run_s16, c["real"][:3],
                    ("push_as", mode))


@pytest.mark.limit(60)
@pytest.mark.parametrize("front", ("u16_unaligned", "s16", "f32", "packed", "iqf32"))
def test_device_pushes_into_scratch_that_held_a_loud_capture(capi, oracle, torch_cuda, front):
    """The staged copy of an unaligned device push, and `unpacked` of the converted, packed and float-IQ device pushes: one final
    push of the loud capture, a reset, then one final push of each target, every target between loud guards of its own."""
    c = stale_cases(oracle)
    kw = dict(df18=True, collect_stats=True)
    complex_ = front == "iqf32"
    fr = "u16" if front == "u16_unaligned" else front
    skew = 1 if front == "u16_unaligned" else 0           # one more loud code in front: the pointer is 2 mod 16, the push is staged
    loud = c["loud_iq"] if complex_ else c["loud"]
    keep = []

    def place(x):
        if complex_:
            g = lambda seed: G.loud_iq(0, G.LOUD_GUARD, seed)
            b, lead = G.inside_loud(S().to_float32_iq(x), g(8410), g(8411))
            return to_dev(torch_cuda, b, lead) + (len(x),)
        flat = np.concatenate([G.loud_codes(G.LOUD_GUARD + skew, 8412), x, G.loud_codes(G.LOUD_GUARD, 8413)])
        return to_dev(torch_cuda, G.as_front(fr, flat), int((G.LOUD_GUARD + skew) * G.unit_bytes(fr))) + (x.size,)

    def run(d, x):
        t, ptr, n = place(x)
        assert (ptr % 16 != 0) == (skew == 1)
        keep.append(t)
        d.reset()
        push(d, fr, ptr, n, True)
        return d.drain(), d.stats()

    def dirty(d):
        t, ptr = to_dev(torch_cuda, loud if complex_ else G.as_front(fr, loud), 2 * skew)
        push(d, fr, ptr, len(loud) - skew, True)
        d.drain()

    targets = c["iq"] if complex_ else c["packed"] if front == "packed" else c["real"]
    _fresh_and_used(capi, kw, dirty, run, targets, front)


@pytest.mark.limit(60)
def test_exports_and_levels_from_scratch_that_held_a_loud_capture(capi, oracle, torch_cuda):
    """power_device_as / _packed / _iq(fmt 0) and their level_device twins convert into `unpacked` first: behind the loud capture the
    floats are the oracle's bit for bit, the reports levels.level_report's, and nothing is written behind either output."""
    c = stale_cases(oracle)
    d = capi.Decoder(df18=True, collect_stats=True)
    n_calls = 0
    try:
        for what in ("s16", "f32", "packed", "iqf32"):
            complex_ = what == "iqf32"
            fmt = G.FRONTS[what][2]
            loud = c["loud_iq"] if complex_ else c["loud"]
            tl, pl = to_dev(torch_cuda, loud if complex_ else G.as_front(what, loud), 0)
            nl = len(loud)
            to, po = dev_out(torch_cuda, nl)

            def export(ptr, n, po, cap):
                if complex_:
                    return d.power_device_iq(0, ptr, n, po, cap)
                return d.power_device_packed(ptr, n, po, cap) if what == "packed" else d.power_device_as(fmt, ptr, n, po, cap)

            def level(ptr, n, pe, k):
                if complex_:
                    return d.level_device_iq(0, ptr, n, pe, k)
                return d.level_device_packed(ptr, n, pe, k) if what == "packed" else d.level_device_as(fmt, ptr, n, pe, k)

            for call in ("power", "level"):
                for x, _, a in (c["iq"] if complex_ else c["packed"] if what == "packed" else c["real"]):
                    # the loud capture goes through the call first and is discarded
                    assert export(pl, nl, po, nl) > 0 if call == "power" else level(pl, nl, 0, 0)["samples"] > 0
                    n = len(x)
                    k = n if complex_ else 2 * (n // 4)
                    if complex_:
                        g = lambda seed: G.loud_iq(0, G.LOUD_GUARD, seed)
                        b, lead = G.inside_loud(S().to_float32_iq(x), g(8420), g(8421))
                    else:
                        flat = np.concatenate([G.loud_codes(G.LOUD_GUARD, 8422), x, G.loud_codes(G.LOUD_GUARD, 8423)])
                        b, lead = G.as_front(what, flat), int(G.LOUD_GUARD * G.unit_bytes(what))
                    t, ptr = to_dev(torch_cuda, b, lead)
                    if call == "power":
                        tt, pt = dev_out(torch_cuda, k)
                        assert export(ptr, n, pt, k) == k
                        check_out(tt, a[:k], (what, n))
                    else:
                        want = want_iq(S().to_float32_iq(x), 0) if complex_ else want_real(oracle, x, a)
                        te, pe, ke = dev_env(torch_cuda, want["samples"])
                        check_level(level(ptr, n, pe, ke), te, want, (what, n))
                    n_calls += 1
    finally:
        d.close()
    assert n_calls == 2 * (9 + 9 + 3 + 5)


@pytest.mark.limit(60)
def test_host_calls_from_windows_that_held_a_loud_capture(capi, oracle, torch_cuda):
    """adsb_scan_shard_host, adsb_power_window_host and adsb_level_host copy the caller's samples into win_buf and write pow_buf:
    behind the loud capture every record and try word, every float and every counter of the targets are the oracle's."""
    c = stale_cases(oracle)
    loud = c["loud"]
    d = capi.Decoder(df18=True, collect_stats=True, all_candidates=True)
    try:
        for j, (x, _, a) in enumerate(c["real"][:5]):
            n_off = (2 * (x.size // 4)) - 1195
            k = 2 * (x.size // 4)
            _scan(capi, d, (loud, None, None), True, 0, loud.size, 0, 2 * (loud.size // 4) - 1195)
            cands, tries = _scan(capi, d, (x, None, None), True, 0, x.size, 0, n_off)
            wc, wt = oracle.scan_all(a, 0, n_off, True)
            assert cands == [r + (0,) for r in wc] and np.array_equal(tries, wt), ("scan_shard_host", j)
            assert d.power_window_host(loud, 0, 0, 2 * (loud.size // 4)).size == 2 * (loud.size // 4)
            got = d.power_window_host(x, 0, 0, k)
            assert np.array_equal(got.view(np.uint32), a[:k].view(np.uint32)), ("power_window_host", j)
            assert d.level(loud)["samples"] == 2 * (loud.size // 4)
            got, want = d.level(x), want_real(oracle, x, a)
            check_level(got, None, want, ("level", j))
            assert np.array_equal(got["env"].view(np.uint32), want["env"].view(np.uint32)), ("level", j)
    finally:
        d.close()


# ---------------------------------------------------------------- 3b. batches into buffers that held a loud batch
BATCH_ROADS, batch_form = G.BATCH_ROADS, G.batch_form    # (tests/guarded_cases.py: shared with the CPU proof)
_batch_want = {}


def batch_cases(oracle, family):
    """-> (the loud batch, the target batch with an empty capture in the middle, that capture's index, the targets' oracle answers
    with None for the empty one), all as the oracle knows them."""
    c = stale_cases(oracle)
    loud = G.loud_batch(G.loud_iq(2, len(c["loud_iq"]), 8401) if family == "iq" else c["loud"])
    targets, mid = G.with_an_empty_capture([x for x, _, _ in c[family]])
    answers = list(c[family])
    answers.insert(mid, None)
    return loud, targets, mid, answers


def _host_at_4_mod_16(a):
    """A copy of the array whose first byte lies at an address that is 4 mod 16."""
    raw = np.empty(a.nbytes + 32, np.uint8)
    lead = (4 - raw.ctypes.data) % 16
    out = raw[lead:lead + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 4
    return out


def _count(form, a):
    """What the calls are given as n: samples, complex samples or power samples."""
    return a.size // 12 * 8 if form == "packed" else a.size // 2 if form in ("iq16", "iqf32") else a.size


def _run_batch(capi, torch, d, road, caps, skew_one, floats=None):
    """One batch call of a road -> what it gave, in a form that compares with ==: decodes ([records], [stats]); exports [the floats'
    bytes] (checked: nothing behind cap; device calls with `floats`: check_out against them); levels ([(counters, bins' bytes,
    envelope's bytes)], the reports with "env"), nothing behind an envelope."""
    from test_gpu_power_export import GUARD as OUT_GUARD, SENT
    family, form, fmt, on_device = BATCH_ROADS[road]
    arrs = [batch_form(form, x) for x in caps]
    biggest = max(range(len(arrs)), key=lambda i: arrs[i].size)
    ns = [_count(form, a) for a in arrs]
    keep, ptrs = [], []
    if on_device:
        for i, a in enumerate(arrs):
            if skew_one and i == biggest:                         # one complex sample of loud memory in front: 4 mod 16
                t, p = to_dev(torch, np.concatenate([np.full(4, 0x7F, np.uint8), a.reshape(-1).view(np.uint8)]), 4)
            else:
                t, p = to_dev(torch, a, 0) if a.size else (None, 0)
            keep.append(t)
            ptrs.append(p)
    elif skew_one:
        arrs[biggest] = _host_at_4_mod_16(arrs[biggest])
    # the power samples a capture gives: two per four real samples, one per complex sample
    ks = [len(x) if family == "iq" else 2 * (len(x) // 4) for x in caps]
    if road.startswith("decode"):
        if on_device:
            call = {"packed": lambda: d.decode_batch_device_packed(ptrs, ns, stats=True), "s16": lambda: d.decode_batch_device_as(fmt, ptrs, ns, stats=True),
                    "iq16": lambda: d.decode_batch_device_iq(fmt, ptrs, ns, stats=True)}[form]
        else:
            call = {"u16": lambda: d.decode_batch(arrs, stats=True), "s16": lambda: d.decode_batch_as(fmt, arrs, stats=True),
                    "f32": lambda: d.decode_batch_as(fmt, arrs, stats=True), "packed": lambda: d.decode_batch_packed(arrs, stats=True),
                    "iq16": lambda: d.decode_batch_iq(fmt, arrs, stats=True), "iqf32": lambda: d.decode_batch_iq(fmt, arrs, stats=True),
                    "power": lambda: d.decode_batch_power(arrs, stats=True)}[form]
        frames, st = call()
        return [records(f) for f in frames], st
    if road.startswith("power"):
        if on_device:
            outs = [dev_out(torch, k) for k in ks]
            args = d._power_batch_args(ptrs, ns, [p if k else 0 for (_, p), k in zip(outs, ks)], ks)
            name = {"packed": "adsb_power_batch_device_packed", "f32": "adsb_power_batch_device_as", "iqf32": "adsb_power_batch_device_iq"}[form]
            assert d._power_call(name, *(() if form == "packed" else (fmt,)), *args) == sum(ks)
            for j, (t, _) in enumerate(outs):
                if floats is not None and floats[j] is not None:
                    check_out(t, floats[j][:ks[j]], (road, j))
            got = [t.cpu().numpy().view(np.uint32) for t, _ in outs]
        else:
            got = [np.full(k + OUT_GUARD, SENT, np.uint32) for k in ks]
            args = d._power_batch_args([a.ctypes.data if a.size else None for a in arrs], ns, [o.ctypes.data if k else None for o, k in zip(got, ks)], ks)
            assert d._power_call("adsb_power_batch_host", *args) == sum(ks)
        assert all((o[k:] == SENT).all() for o, k in zip(got, ks)), (road, "floats behind cap")
        return [o[:k].tobytes() for o, k in zip(got, ks)]
    if on_device:
        envs = [dev_env(torch, k) if k else (None, 0, 0) for k in ks]
        call = {"packed": lambda **kw: d.level_batch_device_packed(ptrs, ns, **kw), "s16": lambda **kw: d.level_batch_device_as(fmt, ptrs, ns, **kw),
                "iqf32": lambda **kw: d.level_batch_device_iq(fmt, ptrs, ns, **kw)}[form]
        out = call(env_ptrs=[p for _, p, _ in envs], env_caps=[k for _, _, k in envs])
        for r, (t, _, k) in zip(out, envs):
            e = t.cpu().numpy().view(np.uint32) if t is not None else np.empty(0, np.uint32)
            assert (e[k:] == SENT).all(), (road, "floats behind the envelope")
            r["env"] = e[:k].view(np.float32).copy()
    else:
        out = d.level_batch(arrs, env=True)
    return [({k: v for k, v in r.items() if k not in ("hist", "env")}, r["hist"].tobytes(), r["env"].view(np.uint32).tobytes()) for r in out], out


@pytest.mark.limit(60)
@pytest.mark.parametrize("road", list(BATCH_ROADS))
def test_batches_into_buffers_that_held_a_loud_batch(capi, oracle, torch_cuda, road):
    """batch_in, batch_land and batch_unpacked, the unpack, export and level tables and the level totals of a handle whose first batch
    call was the loud capture three times, each cut to a different length: the targets of stale_cases with an empty capture in the
    middle then give the oracle's answers -- records and Ok/Try, floats bit for bit with nothing behind cap, reports and envelopes
    word for word -- and what a fresh handle gives."""
    family, form, fmt, on_device = BATCH_ROADS[road]
    loud, targets, mid, answers = batch_cases(oracle, family)
    skew_one = "4_mod_16" in road
    kw = dict(df18=True, collect_stats=True)
    floats = [None if w is None else w[2] for w in answers]
    used, fresh = capi.Decoder(**kw), capi.Decoder(**kw)
    try:
        _run_batch(capi, torch_cuda, used, road, loud, skew_one)              # the loud batch goes through the call first and is discarded
        got = _run_batch(capi, torch_cuda, used, road, targets, skew_one, floats)
        again = _run_batch(capi, torch_cuda, fresh, road, targets, skew_one)
    finally:
        used.close()
        fresh.close()
    if road.startswith("decode"):
        assert got[0][mid] == [] and not any(got[1][mid]["ok"].values()) and not any(got[1][mid]["try"].values()), (road, "the empty capture")
        for j, w in enumerate(answers):
            if w is not None:
                assert got[0][j] == records(w[1][0]), (road, j, "behind the loud batch")
                check_stats(got[1][j], w[1][1], True, (road, j))
        assert again == got, (road, "a fresh handle")
    elif road.startswith("power"):
        assert got[mid] == b"", (road, "the empty capture")
        for j, w in enumerate(answers):
            if w is not None:
                k = len(got[j]) // 4
                assert k > 0 and got[j] == np.ascontiguousarray(w[2][:k], dtype=np.float32).tobytes(), (road, j, "behind the loud batch")
        assert again == got, (road, "a fresh handle")
    else:
        assert got[1][mid]["samples"] == 0 and not got[1][mid]["hist"].any() and got[1][mid]["env"].size == 0, (road, "the empty capture")
        for j, w in enumerate(answers):
            if w is not None:
                if (family, j) not in _batch_want:
                    _batch_want[family, j] = want_iq(S().to_float32_iq(w[0]), 0) if family == "iq" else want_real(oracle, w[0], w[2])
                want = _batch_want[family, j]
                check_level(got[1][j], None, want, (road, j))
                assert np.array_equal(got[1][j]["env"].view(np.uint32), want["env"].view(np.uint32)), (road, j, "the envelope")
        assert again[0] == got[0], (road, "a fresh handle")


# ---------------------------------------------------------------- 4. whole-capture exports and level reports inside loud memory
@pytest.mark.limit(60)
def test_real_exports_and_levels_inside_loud_memory(capi, oracle, torch_cuda):
    """A run, a wave's pass, a workgroup's pass and several workgroups with a ragged end, 16-byte aligned between loud codes with both
    rails among them: the floats are oracle.power(x)'s -- the first six those with silence in front --, the report level_report's of
    them with the rails of the capture's own n codes; uint16 and the int16, float32 and packed twins."""
    d = capi.Decoder(df18=True)
    n_calls = 0
    try:
        for i, n in enumerate(G.REAL_LENGTHS):
            x = np.random.default_rng(8500 + i).integers(0, 4096, n, dtype=np.uint16)
            x[[0, n // 3]], x[[n // 2, n - 1]] = 0, 4095
            for front in ("u16", "s16", "f32", "packed"):
                y = packable(x) if front == "packed" else x
                a = oracle.power(y)
                k = 2 * (y.size // 4)
                want = want_real(oracle, y, a)
                assert want["rail_lo"] == int((y == 0).sum()) > 0 and want["rail_hi"] == int((y == 4095).sum()) > 0
                t, ptr = _loud_twin(torch_cuda, front, y, 8510 + i)
                fmt = G.FRONTS[front][2]
                tt, pt = dev_out(torch_cuda, k)
                te, pe, ke = dev_env(torch_cuda, k)
                if front == "u16":
                    assert d.power_device(ptr, y.size, pt, k) == k
                    rep = d.level_device(ptr, y.size, pe, ke)
                elif front == "packed":
                    assert d.power_device_packed(ptr, y.size, pt, k) == k
                    rep = d.level_device_packed(ptr, y.size, pe, ke)
                else:
                    assert d.power_device_as(fmt, ptr, y.size, pt, k) == k
                    rep = d.level_device_as(fmt, ptr, y.size, pe, ke)
                check_out(tt, a[:k], (front, n))
                check_level(rep, te, want, (front, n))
                n_calls += 2
    finally:
        d.close()
    assert n_calls == 2 * 4 * len(G.REAL_LENGTHS)


@pytest.mark.limit(60)
@pytest.mark.parametrize("fmt", (2, 0, 8, "power"))
def test_complex_and_power_exports_and_levels_inside_loud_memory(capi, torch_cuda, fmt):
    """power_device_iq (fmt 2 and 0: what the export takes) and level_device_iq / level_device_power of
    1, 27, 1792, 1793 and 3 x 7168 + 45 samples between loud guards with rails planted, from a 16-byte aligned pointer and from
    the unaligned one that takes the unit-by-unit road: samples, every counter, every bin and every float are exact, and not one of
    the guards' rails is counted."""
    d = capi.Decoder(df18=True)
    n_calls = 0
    try:
        for i, n in enumerate(G.IQ_LENGTHS):
            if fmt == "power":
                x = np.random.default_rng(8600 + i).uniform(0.0, 2.0 ** 28, n).astype(np.float32)
                a, want = x, LV().level_report(x)
            else:
                x = planted_iq(fmt, n, 8600 + i)
                a, want = S().iq_power(x, fmt), want_iq(x, fmt)
                assert want["rail_lo"] > 0 and want["rail_hi"] > 0
            for skew in (0, 1):                              # one more element of guard in front: 4 bytes (fmt 8: 2) off the alignment
                if fmt == "power":
                    gf, gb = G.loud_power(G.LOUD_GUARD + skew, 8610), G.loud_power(G.LOUD_GUARD, 8611)
                else:
                    gf, gb = G.loud_iq(fmt, G.LOUD_GUARD + skew, 8610), G.loud_iq(fmt, G.LOUD_GUARD, 8611)
                    if fmt == 0 and skew:                    # (a float pair is 8 bytes: one scalar more, not one pair)
                        gf = gf.reshape(-1)[1:]
                b, lead = G.inside_loud(x, gf, gb)
                t, ptr = to_dev(torch_cuda, b, lead)
                assert (ptr % 16 != 0) == bool(skew)
                te, pe, ke = dev_env(torch_cuda, n)
                if fmt == "power":
                    rep = d.level_device_power(ptr, n, pe, ke)
                elif fmt == 8:                               # (int8 IQ has a level report and no export)
                    rep = d.level_device_iq(fmt, ptr, n, pe, ke)
                else:
                    tt, pt = dev_out(torch_cuda, n)
                    assert d.power_device_iq(fmt, ptr, n, pt, n) == n
                    check_out(tt, a, (fmt, n, skew))
                    rep = d.level_device_iq(fmt, ptr, n, pe, ke)
                    n_calls += 1
                check_level(rep, te, want, (fmt, n, skew))
                n_calls += 1
    finally:
        d.close()
    assert n_calls == (1 if fmt in ("power", 8) else 2) * 2 * len(G.IQ_LENGTHS)
