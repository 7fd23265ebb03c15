"""adsb_decode_batch_*: a batch of independent captures in as few launches as they fit (scan_batch_kernel.hip, batch.hpp).
Every capture's result is compared bit for bit -- g, ts, pw, frame bytes, and the Try/Ok table where it is collected -- with
oracle.decode of that capture alone and with the same handle's adsb_decode_device on that capture alone."""
import time

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records
from test_batch_cpu import seeded_capture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).cuda()


def _alone(capi, d, ptr, n):
    out, k = d.decode_device_raw(ptr, n)
    return capi._frames_to_dicts(out, k)


@pytest.fixture(scope="module")
def mixed(torch_cuda, oracle):
    """~40 captures: empty, 3 samples, below one window, 81 956 samples (a window and more, but the reference's first deqframe
    call never fires), 1 Mi sparse and dense, a piece of the gate storm, a 9 Mi dense capture, lengths with n % 4 != 0, and the
    same buffer twice.  -> (host arrays, device tensors, pointers, lengths)."""
    from candidate_model import make_captures
    from tools import gen_signal as G
    caps = [seeded_capture(i) for i in range(28)]          # holds the four degenerate lengths and n % 4 = 1, 2, 3
    caps.append(G.sparse_capture(1 << 20, 170, seed=811, sigma=8.0, dfs=(17, 18, 11))[0])
    caps.append(G.dense_capture(1 << 20, seed=812, sigma=40.0, n_frames=700, amp=(200, 1800))[0])
    quarter = make_captures(1 << 20)
    caps.append(quarter["gate_storm"][(1 << 18) - 40_000:(1 << 19) + 2])      # mostly storm: every tile overflows its queue
    caps.append(quarter["back_to_back"][: (1 << 19) + 3])
    caps.append(quarter["damaged"][: 300_001])
    caps.append(G.dense_capture(9 << 20, seed=813, sigma=60.0, n_frames=6000, amp=(200, 1800))[0])
    caps.append(quarter["saturated"])
    caps.append(quarter["short_frames"][: 1 << 19])
    caps.append(quarter["uniform"][: 200_002])
    tens = [_dev(torch_cuda, x) if x.size else None for x in caps]
    ptrs = [t.data_ptr() if t is not None else 0 for t in tens]
    ns = [int(x.size) for x in caps]
    for twice in (28, 33):                                  # the same pointer twice
        caps.append(caps[twice]), tens.append(tens[twice]), ptrs.append(ptrs[twice]), ns.append(ns[twice])
    assert len(caps) >= 39 and {n % 4 for n in ns} == {0, 1, 2, 3} and {0, 3, 2391, 81956} <= set(ns)
    return caps, tens, ptrs, ns


_want = {}


def _oracle(oracle, caps, df18, fix1=False):
    key = (id(caps), df18, fix1)
    if key not in _want:
        _want[key] = [oracle.decode(x, df18=df18, fix1=fix1) for x in caps]
    return _want[key]


def _check_batch(capi, d, caps, ptrs, ns, want, with_stats, got=None):
    frames, stats = got if got is not None else d.decode_batch_device(ptrs, ns, stats=True)
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
    whole = d.stats()                                       # adsb_get_stats after a batch: the sum over its captures
    assert whole["ok"] == total["ok"] and (not with_stats or whole["try"] == total["try"])
    assert d.profile()["host_threads_running"] == 0
    return frames


@pytest.mark.limit(120)
def test_golden_fixtures_in_one_call(capi, torch_cuda):
    for df18 in (False, True):
        names = [n for n in golden_cases() if load_golden(n)[1]["df18"] == df18]
        if not names:
            continue
        loaded = [load_golden(n) for n in names]
        tens = [_dev(torch_cuda, x) for x, _ in loaded]
        d = capi.Decoder(df18=df18, collect_stats=True)
        try:
            frames, stats = d.decode_batch_device([t.data_ptr() for t in tens], [t.numel() for t in tens], stats=True)
            for i, (x, rec) in enumerate(loaded):
                assert records(frames[i]) == golden_records(rec), names[i]
                assert stats[i] == rec["stats"], names[i]
                assert records(_alone(capi, d, tens[i].data_ptr(), tens[i].numel())) == golden_records(rec)
        finally:
            d.close()


@pytest.mark.limit(300)
@pytest.mark.parametrize("df18", [False, True])
@pytest.mark.parametrize("collect_stats", [False, True])
def test_mixed_batch(capi, oracle, mixed, df18, collect_stats):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, df18)
    assert sum(bool(f) for f, _ in want) >= 25
    d = capi.Decoder(df18=df18, collect_stats=collect_stats)
    try:
        before = d.profile()
        frames = _check_batch(capi, d, caps, ptrs, ns, want, collect_stats)
        after = d.profile()
        assert after["launches"] - before["launches"] == 1          # 11.6 Mi offsets: one launch
        assert after["offsets"] - before["offsets"] == sum(max(0, 2 * (n // 4) - 1195) for n in ns if n >= 81960 - 3)
        for i in range(len(ns)):                                    # ... and the same handle, every capture alone
            assert records(_alone(capi, d, ptrs[i], ns[i])) == records(frames[i]), (i, ns[i])
        frames2 = d.decode_batch_device(ptrs, ns)                   # again, behind single decodes
        assert [records(f) for f in frames2] == [records(f) for f in frames]
    finally:
        d.close()


@pytest.mark.limit(300)
def test_mixed_batch_with_one_bit_repair(capi, oracle, mixed):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True, fix1=True)
    assert sum(ws["fixed"] for _, ws in want) > 20
    d = capi.Decoder(df18=True, collect_stats=True, fix_1bit=True)
    try:
        _check_batch(capi, d, caps, ptrs, ns, want, True)
    finally:
        d.close()


@pytest.mark.limit(300)
def test_mixed_batch_from_host_memory(capi, oracle, mixed):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        _check_batch(capi, d, caps, ptrs, ns, want, True, got=d.decode_batch(caps, stats=True))
        assert [records(f) for f in d.decode_batch(caps[:3])] == [records(f) for f, _ in want[:3]]   # (a smaller one, same scratch)
    finally:
        d.close()


@pytest.mark.limit(300)
def test_all_candidates_and_small_tiles(capi, oracle, mixed):
    """cfg.all_candidates (no never-visited filter) and a forced K = 2 (four times the tiles): the same frames."""
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    for kw in (dict(all_candidates=True), dict(debug_passes=2), dict(debug_passes=9)):
        d = capi.Decoder(df18=True, collect_stats=True, **kw)
        try:
            _check_batch(capi, d, caps, ptrs, ns, want, True)
        finally:
            d.close()


@pytest.mark.limit(300)
def test_relaunch_with_regrown_buffers(capi, oracle, mixed):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    d = capi.Decoder(df18=True, collect_stats=True, debug_cand_cap=8, debug_try_cap=64)
    try:
        before = d.profile()
        _check_batch(capi, d, caps, ptrs, ns, want, True)
        after = d.profile()
        assert after["relaunches"] - before["relaunches"] >= 1
        assert after["launches"] - before["launches"] >= 2
    finally:
        d.close()


@pytest.mark.limit(300)
def test_two_thousand_short_captures(capi, oracle, torch_cuda):
    """2 000 captures of 64 Ki samples in one call.  (By the reference's own rule such a file decodes to nothing: its first
    deqframe call needs 81 960 samples, air.c:94 -- the batch says so without a launch.)  And 2 000 of 96 Ki, which do decode."""
    from tools.gen_signal import make_workload
    for n_each, launches in ((1 << 16, 0), (96 << 10, 1)):
        t, _ = make_workload(torch_cuda, 2000 * n_each, seed=5)
        x = t.cpu().numpy().view(np.uint16)
        ptrs = [t.data_ptr() + 2 * n_each * i for i in range(2000)]
        ns = [n_each] * 2000
        d = capi.Decoder(df18=False, collect_stats=True)
        try:
            before = d.profile()["launches"]
            frames, stats = d.decode_batch_device(ptrs, ns, stats=True)
            assert d.profile()["launches"] - before == launches
            n_frames = 0
            for i in range(0, 2000, 1 if n_each > 81960 else 50):
                wf, ws = oracle.decode(x[i * n_each:(i + 1) * n_each], df18=False)
                assert records(frames[i]) == records(wf) and stats[i] == ws, i
                n_frames += len(wf)
            assert (n_frames > 2000) == (n_each > 81960)
            for i in (0, 7, 1999):
                assert records(_alone(capi, d, ptrs[i], ns[i])) == records(frames[i])
        finally:
            d.close()


@pytest.mark.limit(900)
def test_one_256Mi_buffer_nine_times(capi, oracle, torch_cuda):
    """More than 2^30 offsets: two launches or more.  512 MiB of HBM."""
    from tools.gen_signal import make_workload
    n = 1 << 28
    t, _ = make_workload(torch_cuda, n, seed=3)
    want, wstats = oracle.decode(t.cpu().numpy().view(np.uint16), df18=False)
    assert len(want) > 12_000
    d = capi.Decoder(df18=False, collect_stats=True)
    try:
        before = d.profile()
        frames, stats = d.decode_batch_device([t.data_ptr()] * 9, [n] * 9, stats=True)
        after = d.profile()
        assert after["launches"] - before["launches"] >= 2
        assert after["offsets"] - before["offsets"] == 9 * (n // 2 - 1195)
        for i in range(9):
            assert records(frames[i]) == records(want), i
            assert stats[i] == wstats, i
        assert records(_alone(capi, d, t.data_ptr(), n)) == records(want)
    finally:
        d.close()


@pytest.mark.limit(120)
def test_refusals_leave_a_usable_handle(capi, oracle, mixed):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    d = capi.Decoder(df18=True)
    try:
        k = 29                                               # the 1 Mi dense capture
        d.reset()
        d.push_device(ptrs[k], 1 << 19)                      # a stream in progress: a refusal leaves it as it is
        for bad_ptrs, bad_ns, word in (([ptrs[28], ptrs[k] + 2], [ns[28], ns[k] - 8], "capture 1.*16-byte aligned"),
                                       ([ptrs[28], ptrs[k], 0], [ns[28], ns[k], 5], "capture 2.*NULL"),
                                       ([ptrs[k]], [1 << 32], "capture 0.*2\\^32")):
            with pytest.raises(capi.AdsbError, match=word):
                d.decode_batch_device(bad_ptrs, bad_ns)
        d.push_device_final(ptrs[k] + 2 * (1 << 19), ns[k] - (1 << 19))
        assert records(d.drain()) == records(want[k][0])
        got = d.decode_batch_device([ptrs[k], 0, ptrs[28]], [ns[k], 0, ns[28]])
        assert [records(f) for f in got] == [records(want[k][0]), [], records(want[28][0])]
        assert d.decode_batch_device([], []) == [] and d.decode_batch([]) == []
    finally:
        d.close()


@pytest.mark.limit(120)
def test_the_handle_is_an_ordinary_one_after_a_batch(capi, oracle, mixed):
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        d.decode_batch_device(ptrs, ns)
        k = 33                                               # the 9 Mi dense capture
        assert records(_alone(capi, d, ptrs[k], ns[k])) == records(want[k][0])
        assert d.stats() == want[k][1]
        assert records(d.decode(caps[k], chunk=1 << 20)) == records(want[k][0])      # a push stream
        assert d.stats() == want[k][1]
        d.decode_batch_device(ptrs[:5], ns[:5])
        d.reset()
        assert d.pending() == 0 and d.stats() == {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    finally:
        d.close()


@pytest.mark.limit(120)
def test_a_push_right_after_a_batch_is_refused_until_a_reset(capi, oracle, mixed):
    """A batch leaves the handle finished, as adsb_decode_device does: every kind of push without adsb_reset is refused, and
    adsb_get_stats goes on answering the batch's sum -- never the batch's numbers for a later stream.  After adsb_reset the
    same pushes are an ordinary stream with its own table."""
    caps, tens, ptrs, ns = mixed
    want = _oracle(oracle, caps, True)
    k = 29                                               # 1 Mi dense
    d = capi.Decoder(df18=True, collect_stats=True)
    try:
        frames, _ = d.decode_batch_device(ptrs[:30], ns[:30], stats=True)
        batch_sum = d.stats()
        assert sum(batch_sum["ok"].values()) == sum(len(f) for f in frames) > 0
        for push in (lambda: d.push(caps[k][:4096]), lambda: d.push_async(caps[k][:4096]),
                     lambda: d.push_device(ptrs[k], ns[k]), lambda: d.push_device_final(ptrs[k], ns[k])):
            with pytest.raises(capi.AdsbError, match="after adsb_finish"):
                push()
        d.finish()                                           # (no-op on a finished handle)
        assert d.pending() == 0 and d.stats() == batch_sum
        d.reset()
        d.push_device(ptrs[k], ns[k])
        d.finish()
        assert records(d.drain()) == records(want[k][0]) and d.stats() == want[k][1] != batch_sum
        d.decode_batch_device(ptrs[:5], ns[:5])              # a second batch, then a host push stream
        d.reset()
        d.push(caps[k])
        d.finish()
        assert records(d.drain()) == records(want[k][0]) and d.stats() == want[k][1]
    finally:
        d.close()


@pytest.mark.limit(600)
def test_batch_call_is_at_least_twice_as_fast_as_the_loop(capi, oracle, torch_cuda):
    """256 sparse captures of 1 Mi samples: one adsb_decode_batch_device against a loop of adsb_decode_device over the same
    captures -- same process, same handle configuration, warm-up first, median of 7 repetitions each.  The loop is what the
    library offered before, and pays a launch (10.7 us by scan_kernel.h's own constant) and a host round trip per capture;
    the batch is one launch of 256 x 11 tiles, one sort and 256 resolver passes.  Asserted: batch <= loop / 2."""
    import ctypes as C
    from tools.gen_signal import make_workload
    B, n = 256, 1 << 20
    t, _ = make_workload(torch_cuda, B * n, seed=1)
    ptrs = [t.data_ptr() + 2 * n * i for i in range(B)]
    d_batch, d_loop = capi.Decoder(df18=False), capi.Decoder(df18=False)
    try:
        L = capi.load()
        p = (C.c_void_p * B)(*ptrs)
        nn = (C.c_size_t * B)(*([n] * B))
        first = (C.c_uint64 * (B + 1))()
        out = C.POINTER(capi.Frame)()

        def batch():
            t0 = time.perf_counter()
            k = L.adsb_decode_batch_device(d_batch._h, B, p, nn, C.byref(out), first, None)
            dt = time.perf_counter() - t0
            assert k > 12_000
            return dt

        def loop():
            total = 0
            t0 = time.perf_counter()
            for i in range(B):
                total += d_loop._decode_device(d_loop._h, ptrs[i], n, d_loop._out_ref)
            return time.perf_counter() - t0, total

        got = d_batch.decode_batch_device(ptrs, [n] * B)
        alone = [_alone(capi, d_loop, ptrs[i], n) for i in range(B)]
        assert [records(f) for f in got] == [records(f) for f in alone]
        x = t.cpu().numpy().view(np.uint16)
        for i in (0, 1, 100, 255):
            assert records(got[i]) == records(oracle.decode(x[i * n:(i + 1) * n], df18=False)[0]), i
        for _ in range(3):
            batch(), loop()
        tb = sorted(batch() for _ in range(7))
        tl = sorted(loop()[0] for _ in range(7))
        assert loop()[1] == sum(len(f) for f in got)
        print(f"\nbatch call: median {tb[3] * 1e3:.3f} ms (min {tb[0] * 1e3:.3f}); loop of {B} calls: median {tl[3] * 1e3:.3f} ms "
              f"(min {tl[0] * 1e3:.3f}); ratio {tl[3] / tb[3]:.2f}")
        assert tb[3] <= 0.5 * tl[3], (tb, tl)
    finally:
        d_batch.close()
        d_loop.close()
