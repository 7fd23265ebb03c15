"""A handle that has allocated EVERY optional resource, destroyed and created again (run with -m gpu on an MI355X).

One handle per cycle -- long-stream, statistics, one-bit repair, a reader thread and a gang, the smallest staging buffers --
goes through the asynchronous stream path (both staging buffers, the tail copy, both copy streams, the count passes), the
packed stream path (the landing buffers), both host batch calls (the batch scratch, the landing scratch, both tables) and
a shard scan from host memory (the window buffer), and is closed.  Every result is the oracle's, the cycles agree, and a
handle created after the last close decodes like the first.  No assertion on free device memory: the machines are
shared."""
import ctypes as C

import numpy as np
import pytest

from conftest import records
from test_batch_cpu import seeded_capture
from test_gpu_batch_packed import packable

pytestmark = pytest.mark.gpu

N = 1 << 20
KW = dict(long_stream=True, collect_stats=True, fix_1bit=True, host_threads=3, stage_samples=1 << 16)


def _table(stats):
    return stats["try"], stats["ok"], stats.get("fixed", 0)


@pytest.fixture(scope="module")
def work(oracle, capi):
    """The inputs and the oracle's answers, computed once: x, its packable twin, four seeded captures and theirs, and the
    first owned range of a two-shard plan with the oracle's exhaustive evaluation of it."""
    from adsbdec_amd.packed12 import pack12
    from tools import gen_signal as G
    x = G.sparse_capture(N, 170, seed=4242, sigma=8.0, dfs=(17, 18, 11))[0]
    caps = [seeded_capture(i) for i in range(4)]
    shard = capi.plan_shards(x.size, 2)[0]
    assert shard["first_sample"] == 0 and 0 == shard["g_begin"] < shard["g_end"]
    decode = lambda y: oracle.decode(y, df18=False, fix1=True)
    w = dict(x=x, px=pack12(packable(x)), caps=caps, pcaps=[pack12(packable(c)) for c in caps], shard=shard,
             want_x=decode(x), want_px=decode(packable(x)), want_caps=[decode(c) for c in caps],
             want_pcaps=[decode(packable(c)) for c in caps],
             want_shard=oracle.scan_all(oracle.power(x), shard["g_begin"], shard["g_end"], False))
    assert len(w["want_x"][0]) >= 50 and sum(bool(f) for f, _ in w["want_caps"]) >= 2
    return w


def _scan_shard_host(capi, d, x, shard):
    L = capi.load()
    n = shard["n_samples"]
    buf = np.ascontiguousarray(x[:n])
    cands, tries = (capi.Candidate * (1 << 16))(), np.empty(1 << 20, dtype=np.uint64)
    nc, nt = C.c_size_t(0), C.c_size_t(0)
    rc = L.adsb_scan_shard_host(d._h, buf.ctypes.data, 0, n, shard["g_begin"], shard["g_end"], cands, len(cands), C.byref(nc),
                                tries.ctypes.data_as(C.POINTER(C.c_uint64)), tries.size, C.byref(nt))
    assert rc == 0, (L.adsb_last_error(d._h) or b"").decode()
    return ([(int(c.g), int(c.pw), bytes(c.frame[: c.len]), int(c.reserved)) for c in cands[: nc.value]],
            tries[: nt.value].copy())


def _cycle(capi, w):
    """One handle through every path; what it gave, after each answer has been checked against the oracle's."""
    d = capi.Decoder(**KW)
    try:
        got = [records(d.decode(w["x"], mode="async")), _table(d.stats())]
        assert got[0] == records(w["want_x"][0]) and got[1] == _table(w["want_x"][1])
        d.reset()
        got += [records(d.decode_packed(w["px"])), _table(d.stats())]
        assert got[2] == records(w["want_px"][0]) and got[3] == _table(w["want_px"][1])
        d.reset()
        for bufs, want, call in ((w["pcaps"], w["want_pcaps"], d.decode_batch_packed), (w["caps"], w["want_caps"], d.decode_batch)):
            frames, stats = call(bufs, stats=True)
            got += [[records(f) for f in frames], [_table(s) for s in stats]]
            assert got[-2] == [records(f) for f, _ in want] and got[-1] == [_table(s) for _, s in want]
        kept, tries = _scan_shard_host(capi, d, w["x"], w["shard"])
        wc, wt = w["want_shard"]
        # the try words are the oracle's; the records are what the device's never-visited filter leaves of the oracle's
        # exhaustive list (tests/test_gpu_candidates.py), plus repaired frames (reserved = 1)
        assert np.array_equal(tries, wt)
        assert kept == sorted(kept) and {c[:3] for c in kept if c[3] == 0} <= set(wc) and len(kept) >= 20
        got += [kept, tries.tolist()]
    finally:
        d.close()
    return got


@pytest.mark.limit(120)
def test_a_handle_with_every_resource_closed_and_created_again(capi, work):
    cycles = [_cycle(capi, work) for _ in range(3)]
    assert cycles[1] == cycles[0] and cycles[2] == cycles[0]
    d = capi.Decoder(**KW)
    try:
        assert records(d.decode(work["x"], mode="async")) == records(work["want_x"][0])
        assert _table(d.stats()) == _table(work["want_x"][1])
    finally:
        d.close()
