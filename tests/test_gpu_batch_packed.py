"""adsb_decode_batch_device_packed / _host_packed: a batch of Airspy packed 12-bit captures, unpacked by ONE launch
(unpack12_batch.hip) and scanned as a batch.  The packed inputs are built with adsbdec_amd.packed12.pack12; every capture's
expected result is oracle.decode(unpack12(packed)) of that capture alone -- g, ts, pw, frame bytes and the Try/Ok table where it
is collected -- and the same handle's adsb_decode_device_packed on that capture alone must agree."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records
from test_batch_cpu import seeded_capture

pytestmark = pytest.mark.gpu

# tools/batch_probe.py --packed, 256 captures of 1 Mi samples on an MI355X (profiles/r10_batch_packed.txt): one
# adsb_decode_batch_device_packed call against the loop of adsb_decode_device_packed.  Asserted below: half of it, rounded down,
# never less than 1.  Measured: 0.777 ms against 7.624 ms.
MEASURED_LOOP_OVER_BATCH = 9.81
ASSERTED_LOOP_OVER_BATCH = max(1, int(MEASURED_LOOP_OVER_BATCH / 2))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


def packable(x):
    """The capture cut to whole 8-sample groups, codes clipped to what 12 bits hold."""
    x = np.asarray(x, np.uint16)
    return np.ascontiguousarray(np.minimum(x[: x.size // 8 * 8], 4095).astype(np.uint16))


class PackedOnDevice:
    """Packed captures side by side in ONE device buffer, every capture at a 4-byte aligned address; `skew` bytes (a multiple
    of 4) in front of each capture move the addresses off the 16-byte boundaries."""

    def __init__(self, torch, packed, skew=(4, 8, 12, 0)):
        at, cur = [], 0
        for i, b in enumerate(packed):
            cur = (cur + 15) // 16 * 16 + skew[i % len(skew)]
            at.append(cur)
            cur += b.size
        host = np.zeros(cur + 16, np.uint8)
        for a, b in zip(at, packed):
            host[a:a + b.size] = b
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + a if b.size else 0 for a, b in zip(at, packed)]


def build_mixed():
    from candidate_model import make_captures
    from tools import gen_signal as G
    caps = [seeded_capture(i) for i in range(28)]
    rng = np.random.default_rng(10_000)
    for n in (0, 8, 2392, 81952, 81960):                     # 81 952: below the reference's first deqframe call; 81 960: the first length with offsets
        caps.append(np.clip(np.rint(2048 + rng.normal(0, 30, n)), 0, 4095).astype(np.uint16))
    caps.append(G.sparse_capture(1 << 20, 170, seed=811, sigma=8.0, dfs=(17, 18, 11))[0])
    caps.append(G.dense_capture(1 << 20, seed=812, sigma=40.0, n_frames=700, amp=(200, 1800))[0])
    quarter = make_captures(1 << 20)
    caps.append(quarter["gate_storm"][(1 << 18) - 40_000:(1 << 19) + 2])
    caps.append(quarter["back_to_back"][: (1 << 19) + 3])
    caps.append(quarter["damaged"][: 300_001])
    caps.append(G.dense_capture(9 << 20, seed=813, sigma=60.0, n_frames=6000, amp=(200, 1800))[0])
    caps.append(quarter["short_frames"][: 1 << 19])
    caps = [packable(x) for x in caps]
    assert all(x.size % 8 == 0 and (x.size == 0 or int(x.max()) <= 4095) for x in caps)
    return caps


@pytest.fixture(scope="module")
def mixed(torch_cuda):
    """40 packed captures: the seeded ones of tests/test_batch_cpu.py (sparse, dense, noisy, back-to-back), the lengths 0, 8,
    2 392, 81 952 and 81 960, 1 Mi sparse and dense, a piece of the gate storm, back-to-back and damaged traffic, a 9 Mi dense
    capture; two of them a second time through the same pointer.  -> (unpacked twins, packed bytes, pointers, lengths)."""
    from adsbdec_amd.packed12 import pack12, unpack12
    caps = build_mixed()
    packed = [pack12(x) for x in caps]
    for x, b in zip(caps, packed):
        assert b.size == x.size // 8 * 12 and np.array_equal(unpack12(b), x)
    dev = PackedOnDevice(torch_cuda, packed)
    ptrs, ns = list(dev.ptrs), [int(x.size) for x in caps]
    for twice in (33, 38):                                   # the same pointer twice
        caps.append(caps[twice]), packed.append(packed[twice]), ptrs.append(ptrs[twice]), ns.append(ns[twice])
    assert len(caps) >= 30 and {0, 8, 2392, 81952, 81960} <= set(ns)
    assert {p % 16 for p in ptrs if p} >= {4, 8, 12} and all(p % 4 == 0 for p in ptrs)
    return caps, packed, ptrs, ns, dev


_want = {}


def _oracle(oracle, packed, df18, fix1=False):
    from adsbdec_amd.packed12 import unpack12
    key = (id(packed), df18, fix1)
    if key not in _want:
        _want[key] = [oracle.decode(unpack12(b), df18=df18, fix1=fix1) for b in packed]
    return _want[key]


def _alone(capi, d, ptr, n):
    out, k = d.decode_device_packed_raw(ptr, n)
    return capi._frames_to_dicts(out, k)


def _check_batch(d, ns, want, with_stats, got):
    frames, stats = got
    assert len(frames) == len(stats) == len(want) == len(ns)
    total = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for i, (wf, ws) in enumerate(want):
        assert records(frames[i]) == records(wf), (i, ns[i])
        assert stats[i]["ok"] == ws["ok"], (i, ns[i])
        if with_stats:
            assert {k: v for k, v in stats[i].items() if k != "fixed"} == {k: v for k, v in ws.items() if k != "fixed"}, (i, ns[i])
        assert stats[i].get("fixed", 0) == ws.get("fixed", 0)
        for row in ("try", "ok"):
            for df in (11, 17, 18):
                total[row][df] += stats[i][row][df]
    whole = d.stats()                                        # adsb_get_stats after a batch: the sum over its captures
    assert whole["ok"] == total["ok"] and (not with_stats or whole["try"] == total["try"])
    return frames


@pytest.mark.limit(120)
def test_golden_fixtures_packed_in_one_call(capi, torch_cuda):
    from adsbdec_amd.packed12 import pack12
    used = 0
    for df18 in (False, True):
        loaded = [(n,) + load_golden(n) for n in golden_cases()]
        loaded = [(n, x, rec) for n, x, rec in loaded if rec["df18"] == df18 and x.size % 8 == 0 and int(x.max()) <= 4095]
        if not loaded:
            continue
        dev = PackedOnDevice(torch_cuda, [pack12(x) for _, x, _ in loaded])
        ns = [int(x.size) for _, x, _ in loaded]
        d = capi.Decoder(df18=df18, collect_stats=True)
        try:
            frames, stats = d.decode_batch_device_packed(dev.ptrs, ns, stats=True)
            for i, (name, x, rec) in enumerate(loaded):
                assert records(frames[i]) == golden_records(rec), name
                assert stats[i] == rec["stats"], name
                assert records(_alone(capi, d, dev.ptrs[i], ns[i])) == golden_records(rec), name
                used += 1
        finally:
            d.close()
    assert used >= 5


@pytest.mark.limit(300)
@pytest.mark.parametrize("df18", [False, True])
@pytest.mark.parametrize("collect_stats", [False, True])
def test_mixed_batch(capi, oracle, mixed, df18, collect_stats):
    caps, packed, ptrs, ns, _ = mixed
    want = _oracle(oracle, packed, df18)
    assert sum(bool(f) for f, _ in want) >= 25
    d = capi.Decoder(df18=df18, collect_stats=collect_stats)
    try:
        before = d.profile()
        frames = _check_batch(d, ns, want, collect_stats, d.decode_batch_device_packed(ptrs, ns, stats=True))
        after = d.profile()
        assert after["launches"] - before["launches"] == 1              # one scan launch behind the one unpack launch
        for i in range(len(ns)):                                        # ... and the same handle, every capture alone
            assert records(_alone(capi, d, ptrs[i], ns[i])) == records(frames[i]), (i, ns[i])
        frames2 = d.decode_batch_device_packed(ptrs, ns)                # again, behind single decodes
        assert [records(f) for f in frames2] == [records(f) for f in frames]
    finally:
        d.close()


@pytest.mark.limit(300)
def test_mixed_batch_with_one_bit_repair(capi, oracle, mixed):
    caps, packed, ptrs, ns, _ = mixed
    want = _oracle(oracle, packed, True, fix1=True)
    assert sum(ws["fixed"] for _, ws in want) > 20
    d = capi.Decoder(df18=True, collect_stats=True, fix_1bit=True)
    try:
        _check_batch(d, ns, want, True, d.decode_batch_device_packed(ptrs, ns, stats=True))
    finally:
        d.close()


@pytest.mark.limit(300)
def test_packed_batch_equals_the_batch_of_the_unpacked_twins(capi, torch_cuda, mixed):
    caps, packed, ptrs, ns, _ = mixed
    tens = [torch_cuda.from_numpy(x.view(np.int16)).cuda() if x.size else None for x in caps]
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        twins = d.decode_batch_device([t.data_ptr() if t is not None else 0 for t in tens], ns, stats=True)
        got = d.decode_batch_device_packed(ptrs, ns, stats=True)
        assert [records(f) for f in got[0]] == [records(f) for f in twins[0]] and got[1] == twins[1]
    finally:
        d.close()


@pytest.mark.limit(300)
def test_mixed_batch_from_host_memory(capi, oracle, mixed):
    caps, packed, ptrs, ns, _ = mixed
    want = _oracle(oracle, packed, True)
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        _check_batch(d, ns, want, True, d.decode_batch_packed(packed, stats=True))
        assert [records(f) for f in d.decode_batch_packed(packed[:3])] == [records(f) for f, _ in want[:3]]   # (a smaller one, same buffers)
        _check_batch(d, ns, want, True, d.decode_batch_device_packed(ptrs, ns, stats=True))                   # device after host, same handle
        for kw in (dict(collect_stats=False), dict(df18=False, collect_stats=True), dict(collect_stats=True, fix_1bit=True)):
            d2 = capi.Decoder(**{"df18": True, **kw})
            try:
                _check_batch(d2, ns, _oracle(oracle, packed, kw.get("df18", True), fix1=kw.get("fix_1bit", False)), kw["collect_stats"],
                             d2.decode_batch_packed(packed, stats=True))
            finally:
                d2.close()
    finally:
        d.close()


@pytest.mark.limit(300)
def test_relaunch_with_regrown_buffers(capi, oracle, mixed):
    caps, packed, ptrs, ns, _ = mixed
    want = _oracle(oracle, packed, True)
    d = capi.Decoder(df18=True, collect_stats=True, debug_cand_cap=8, debug_try_cap=64)
    try:
        before = d.profile()
        _check_batch(d, ns, want, True, d.decode_batch_device_packed(ptrs, ns, stats=True))
        after = d.profile()
        assert after["relaunches"] - before["relaunches"] >= 1
        assert after["launches"] - before["launches"] >= 2
    finally:
        d.close()


@pytest.mark.limit(600)
@pytest.mark.parametrize("n_each", [1 << 16, 1 << 20])
def test_two_thousand_captures_in_one_call(capi, oracle, torch_cuda, n_each):
    """2 048 packed captures of 64 Ki samples (below the reference's first deqframe call: no frames, and no scan launch) and of
    1 Mi samples (3 GiB packed, 4 GiB of scratch), each in one call: 64 distinct captures, 32 copies of each at addresses of
    their own.  Every capture is compared with the oracle's answer for its content."""
    from adsbdec_amd.packed12 import pack12, unpack12
    from tools.gen_signal import make_workload
    B, distinct = 2048, 64
    t, _ = make_workload(torch_cuda, distinct * n_each, seed=5)
    x = packable(t.cpu().numpy().view(np.uint16))
    del t
    assert x.size == distinct * n_each
    one = pack12(x)
    assert np.array_equal(unpack12(one), x)              # the whole buffer round-trips: oracle.decode(x[...]) below is decode(unpack12(packed))
    per = n_each // 8 * 12
    buf = torch_cuda.from_numpy(one).cuda().repeat(B // distinct)
    assert buf.numel() == B * per
    ptrs = [buf.data_ptr() + per * i for i in range(B)]
    want = [oracle.decode(x[k * n_each:(k + 1) * n_each], df18=False) for k in range(distinct)]
    d = capi.Decoder(df18=False, collect_stats=True)
    try:
        before = d.profile()["launches"]
        frames, stats = d.decode_batch_device_packed(ptrs, [n_each] * B, stats=True)
        # (2 048 x 1 Mi samples are more than 2^30 offsets: the layout says how many launches that takes)
        assert d.profile()["launches"] - before == sum(1 for launch in capi.batch_layout([n_each] * B)[1] if launch["tiles"])
        for i in range(B):
            wf, ws = want[i % distinct]
            assert records(frames[i]) == records(wf) and stats[i] == ws, i
        assert (sum(len(f) for f in frames) > B) == (n_each > 81960)
        for i in (0, 7, B - 1):
            assert records(_alone(capi, d, ptrs[i], n_each)) == records(frames[i])
    finally:
        d.close()


@pytest.mark.limit(120)
def test_refusals_leave_a_usable_handle(capi, oracle, mixed):
    caps, packed, ptrs, ns, dev = mixed
    want = _oracle(oracle, packed, True)
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        k = 34                                               # the 1 Mi dense capture
        assert ns[k] == 1 << 20
        half = 1 << 19
        d.reset()
        d.push_device_packed(ptrs[k], half)                  # a stream in progress: a refusal leaves it as it is
        host = [packed[33], packed[k]]
        for call, bad_ptrs, bad_ns, word in (
                (d.decode_batch_device_packed, [ptrs[33], ptrs[k]], [ns[33], ns[k] - 4], "capture 1.*multiple of 8"),
                (d.decode_batch_device_packed, [ptrs[33], ptrs[k] + 2], [ns[33], ns[k] - 8], "capture 1.*4-byte aligned"),
                (d.decode_batch_device_packed, [ptrs[33], ptrs[k], 0], [ns[33], ns[k], 8], "capture 2.*NULL"),
                (d.decode_batch_device_packed, [ptrs[k]], [1 << 32], "capture 0.*2\\^32")):
            with pytest.raises(capi.AdsbError, match=word):
                call(bad_ptrs, bad_ns)
        L = capi.load()
        hp = (C.c_void_p * 3)(host[0].ctypes.data, host[1].ctypes.data, None)
        first = (C.c_uint64 * 4)()
        out = C.POINTER(capi.Frame)()
        for bad_ns, word in (([ns[33], ns[k] - 4, 0], b"capture 1"), ([ns[33], ns[k], 8], b"capture 2"), ([1 << 32, 0, 0], b"capture 0")):
            assert L.adsb_decode_batch_host_packed(d._h, 3, hp, (C.c_size_t * 3)(*bad_ns), C.byref(out), first, None) == -1
            assert word in L.adsb_last_error(d._h), L.adsb_last_error(d._h)
        d.push_device_packed_final(ptrs[k] + half // 8 * 12, ns[k] - half)
        assert records(d.drain()) == records(want[k][0]) and d.stats() == want[k][1]
        _check_batch(d, ns, want, True, d.decode_batch_device_packed(ptrs, ns, stats=True))
        _check_batch(d, ns, want, True, d.decode_batch_packed(packed, stats=True))
        assert d.decode_batch_device_packed([], []) == [] and d.decode_batch_packed([]) == []
    finally:
        d.close()


@pytest.mark.limit(120)
def test_the_handle_is_an_ordinary_one_after_a_reset(capi, oracle, mixed):
    """A packed batch leaves the handle finished, as adsb_decode_batch_device does: a push without adsb_reset is refused and
    adsb_get_stats goes on answering the batch's sum; after adsb_reset the handle streams as any other."""
    from adsbdec_amd.packed12 import unpack12
    caps, packed, ptrs, ns, _ = mixed
    want = _oracle(oracle, packed, True)
    k = 38                                                   # the 9 Mi dense capture
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        frames, _ = d.decode_batch_device_packed(ptrs, ns, stats=True)
        batch_sum = d.stats()
        assert sum(batch_sum["ok"].values()) == sum(len(f) for f in frames) > 0
        for push in (lambda: d.push(caps[k][:4096]), lambda: d.push_packed(packed[k][:12 * 512]),
                     lambda: d.push_device_packed(ptrs[k], ns[k]), lambda: d.push_device_packed_final(ptrs[k], ns[k])):
            with pytest.raises(capi.AdsbError, match="after adsb_finish"):
                push()
        assert d.pending() == 0 and d.stats() == batch_sum
        d.reset()
        assert d.pending() == 0 and d.stats() == {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
        assert records(d.decode_packed(packed[k], chunk=1 << 20)) == records(want[k][0])      # a packed push stream
        assert d.stats() == want[k][1]
        assert records(d.decode(unpack12(packed[k]), chunk=1 << 20)) == records(want[k][0])   # a uint16 push stream
        assert records(_alone(capi, d, ptrs[k], ns[k])) == records(want[k][0]) and d.stats() == want[k][1]
        d.decode_batch_packed(packed[:5])
        d.reset()
        assert d.pending() == 0
    finally:
        d.close()


@pytest.mark.limit(600)
def test_packed_batch_call_against_the_loop_of_single_calls(capi, oracle, torch_cuda):
    """256 device-resident packed captures of 1 Mi samples (sparse traffic): one adsb_decode_batch_device_packed against the
    loop of adsb_decode_device_packed over the same captures -- the call the library offered for a packed archive before, an
    unpack launch, a scan launch and a host round trip per capture.  Same process, a handle per side, frames compared first,
    a warm-up, medians of 7 repetitions.  Measured with tools/batch_probe.py --packed (profiles/r10_batch_packed.txt);
    asserted: half the measured ratio, rounded down.  Printed, not asserted: adsb_decode_batch_device on the unpacked twins --
    the difference is the price of the extra pass of 3.5 B per sample."""
    from adsbdec_amd.packed12 import pack12, unpack12
    from tools.gen_signal import make_workload
    B, n = 256, 1 << 20
    t, _ = make_workload(torch_cuda, B * n, seed=1)
    x = packable(t.cpu().numpy().view(np.uint16))
    assert x.size == B * n
    twins = torch_cuda.from_numpy(x.view(np.int16)).cuda()
    del t
    per = n // 8 * 12
    pk = torch_cuda.from_numpy(pack12(x)).cuda()
    ptrs = [pk.data_ptr() + per * i for i in range(B)]
    uptrs = [twins.data_ptr() + 2 * n * i for i in range(B)]
    d_batch, d_loop, d_twin = capi.Decoder(df18=False), capi.Decoder(df18=False), capi.Decoder(df18=False)
    try:
        L = capi.load()
        p, up = (C.c_void_p * B)(*ptrs), (C.c_void_p * B)(*uptrs)
        nn = (C.c_size_t * B)(*([n] * B))
        first = (C.c_uint64 * (B + 1))()
        out = C.POINTER(capi.Frame)()

        def batch(fn=L.adsb_decode_batch_device_packed, d=d_batch, pp=p):
            t0 = time.perf_counter()
            k = fn(d._h, B, pp, nn, C.byref(out), first, None)
            dt = time.perf_counter() - t0
            assert k > 12_000
            return dt

        def loop():
            total = 0
            t0 = time.perf_counter()
            for i in range(B):
                total += L.adsb_decode_device_packed(d_loop._h, ptrs[i], n, d_loop._out_ref)
            return time.perf_counter() - t0, total

        got = d_batch.decode_batch_device_packed(ptrs, [n] * B)
        alone = [_alone(capi, d_loop, ptrs[i], n) for i in range(B)]
        assert [records(f) for f in got] == [records(f) for f in alone]
        assert [records(f) for f in d_twin.decode_batch_device(uptrs, [n] * B)] == [records(f) for f in got]
        for i in (0, 1, 100, 255):
            assert records(got[i]) == records(oracle.decode(unpack12(pack12(x[i * n:(i + 1) * n])), df18=False)[0]), i
        for _ in range(3):
            batch(), loop(), batch(L.adsb_decode_batch_device, d_twin, up)
        tb = sorted(batch() for _ in range(7))
        tl = sorted(loop()[0] for _ in range(7))
        tu = sorted(batch(L.adsb_decode_batch_device, d_twin, up) for _ in range(7))
        assert loop()[1] == sum(len(f) for f in got)
        print(f"\npacked batch call: median {tb[3] * 1e3:.3f} ms (min {tb[0] * 1e3:.3f}); loop of {B} packed calls: median {tl[3] * 1e3:.3f} ms "
              f"(min {tl[0] * 1e3:.3f}); ratio {tl[3] / tb[3]:.2f}; batch of the unpacked twins: median {tu[3] * 1e3:.3f} ms "
              f"(packed / unpacked {tb[3] / tu[3]:.2f})")
        assert tb[3] * ASSERTED_LOOP_OVER_BATCH <= tl[3], (tb, tl)
    finally:
        d_batch.close()
        d_loop.close()
        d_twin.close()
