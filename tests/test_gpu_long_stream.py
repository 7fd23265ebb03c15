"""Decoding past sample 2^31, up to 2^32 - 4, on the device, against the long_stream fixture (tests/long_stream.py): the real
reference chain's records and Try/Ok table over a whole stream of 2^32 - 4 samples that is silence but for three bursts.
The silence is one device buffer pushed again and again, so a full-length stream costs a few GiB of HBM and no host work.

* one handle over the whole stream, the bursts pushed from the device, from the host (sync, async, push_overlap) and as
  packed 12-bit samples; with the 1-bit repair against the restatement under the shift rule; then a sample more is refused;
* the multi-GPU driver, 8 handles on this device: seams inside b1 (at sample 2^31) and b2, the horizon inside b3;
* adsb_scan_shard / adsb_scan_shard_host offset by offset at windows across sample 2^31 and up to sample 2^32 - 4;
* the 2^32 limit of the shard primitives, on both sides."""
import ctypes as C

import numpy as np
import pytest

import candidate_model as M
import long_stream as LS
from test_gpu_candidates import CONFIGS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def fixture():
    return LS.load()


@pytest.fixture(scope="module")
def silence(torch_cuda, capi):
    """One device buffer of silence, as long as the longest shard of an 8-way plan (a little over 2^29 samples, 1 GiB)."""
    n = max(p["n_samples"] for p in capi.plan_shards(LS.N, 8))
    t = torch_cuda.full((n,), LS.SILENCE, dtype=torch_cuda.int16, device="cuda")
    yield t
    del t
    torch_cuda.cuda.empty_cache()


def _dev(torch, y):
    return torch.from_numpy(np.ascontiguousarray(y).view(np.int16)).cuda()


def _packed_dev(torch, y):
    from adsbdec_amd.packed12 import pack12
    return torch.from_numpy(pack12(y)).cuda()


def _records(raw):
    from adsbdec_amd import capi
    return [(f["g"], f["ts"], f["pw"], bytes(f["frame"])) for f in capi._frames_to_dicts(*raw)]


def _push_stream(capi, torch, d, silence, bursts, how):
    """The whole stream into handle d: silence from the device buffer, the bursts as `how` says."""
    keep = []
    pinned = capi.PinnedBuffers(2, max(y.size for _, y in bursts.values()))
    bufs = pinned.__enter__()
    try:
        k = 0
        for at, y in LS.pieces(bursts, silence):
            if isinstance(y, np.ndarray) and y.dtype == np.uint16:
                if how == "device":
                    t = _dev(torch, y)
                    keep.append(t)
                    d.push_device(t.data_ptr(), y.size)
                elif how == "sync":
                    d.push(y)
                elif how in ("async", "overlap"):
                    b = bufs[k % 2][: y.size]
                    k += 1
                    b[:] = y
                    if how == "async":
                        d.push_async(b)                   # borrowed until the next push returns
                    else:
                        d.push(b)                         # push_overlap: the copy is complete on return
                        b[:] = 0xFFFF
                elif how == "packed":
                    m = y.size - y.size % 8
                    t = _packed_dev(torch, y[:m])
                    keep.append(t)
                    d.push_device_packed(t.data_ptr(), m)
                    if m < y.size:                        # b3 ends at 2^32 - 4, not a multiple of 8: its last samples unpacked
                        t = _dev(torch, y[m:])
                        keep.append(t)
                        d.push_device(t.data_ptr(), y.size - m)
                else:
                    raise ValueError(how)
            else:
                d.push_device(y.data_ptr(), y.numel())
        d.sync()
    finally:
        pinned.__exit__(None, None, None)
    return keep


class _Silence:
    """The device silence buffer, sliced like an ndarray by LS.pieces."""

    def __init__(self, t):
        self.t = t
        self.size = t.numel()

    def __getitem__(self, sl):
        return self.t[sl]


@pytest.mark.limit(240)
@pytest.mark.parametrize("how,df18", [("device", False), ("device", True), ("sync", True), ("async", False),
                                      ("overlap", True), ("packed", True)])
def test_one_handle_decodes_the_whole_stream(capi, torch_cuda, fixture, silence, how, df18):
    _, bursts, runs = fixture
    d = capi.Decoder(df18=df18, collect_stats=True, push_overlap=(how == "overlap"))
    try:
        keep = _push_stream(capi, torch_cuda, d, _Silence(silence), bursts, how)
        # one sample more than the reference can count: refused, before anything is read; the stream goes on
        with pytest.raises(capi.AdsbError, match="2\\^32"):
            d.push_device(silence.data_ptr(), 4)
        d.finish()
        assert _records(d.take_raw()) == LS.records(runs[df18])
        assert d.stats() == runs[df18]["stats"]
        del keep
        # ... and the handle decodes the next stream
        d.reset()
        s, y = bursts["b2"]
        x, shift = LS.padded(s, y)
        t = _dev(torch_cuda, x)
        d.push_device_final(t.data_ptr(), x.size)
        from oracle import oracle as O
        want, wstats = O.decode(x, df18=df18)
        assert _records(d.take_raw()) == [(f["g"], f["ts"], f["pw"], f["frame"]) for f in want]
        assert d.stats() == wstats
    finally:
        d.close()


@pytest.mark.limit(240)
def test_one_bit_repair_over_the_whole_stream(capi, oracle, torch_cuda, fixture, silence):
    """fix_1bit: b1 and b2 equal the restatement's 1-bit repair on their stand-ins under the shift rule (frames, and the
    repaired count of those two bursts at least); b2 holds the damaged long frames."""
    _, bursts, runs = fixture
    d = capi.Decoder(df18=True, collect_stats=True, fix_1bit=True)
    try:
        keep = _push_stream(capi, torch_cuda, d, _Silence(silence), bursts, "device")
        d.finish()
        got = _records(d.take_raw())
        stats = d.stats()
        del keep
    finally:
        d.close()
    fixed = 0
    for name in ("b1", "b2"):
        s, y = bursts[name]
        x, shift = LS.padded(s, y)
        want, wstats = oracle.decode(x, df18=True, fix1=True)
        lo, hi = s // 2, (s + y.size) // 2
        assert [(g, pw, fr) for g, _, pw, fr in got if lo <= g < hi] == [(f["g"] + shift, f["pw"], f["frame"]) for f in want], name
        fixed += wstats["fixed"]
    assert fixed > 10 and stats["fixed"] >= fixed
    assert len(got) > len(runs[True]["frames"])


@pytest.mark.limit(240)
def test_multi_gpu_driver_over_the_whole_stream(capi, torch_cuda, fixture, silence):
    """adsb_multi_decode_device, 8 handles on device 0: a shard of nothing but silence reads the shared silence buffer, a
    shard that holds a burst has a buffer of its own."""
    from adsbdec_amd import sharding
    _, bursts, runs = fixture
    for df18 in (True, False):
        md = sharding.MultiDecoder(8, [0] * 8, df18=df18, collect_stats=True)
        own = []
        try:
            plan = md.plan(LS.N)
            assert len(plan) == 8
            s1, y1 = bursts["b1"]
            assert s1 < 2 * plan[4]["g_begin"] < s1 + y1.size                # the seam near sample 2^31 falls inside b1
            ptrs = []
            for p in plan:
                a, e = p["first_sample"], p["first_sample"] + p["n_samples"]
                mine = [(s, y) for s, y in bursts.values() if s < e and s + y.size > a]
                if not mine:
                    ptrs.append(silence.data_ptr())
                    continue
                t = silence[: p["n_samples"]].clone()
                for s, y in mine:
                    lo, hi = max(s, a), min(s + y.size, e)
                    t[lo - a: hi - a] = _dev(torch_cuda, y[lo - s: hi - s])
                own.append(t)
                ptrs.append(t.data_ptr())
            assert 3 <= len(own) <= 5
            got = _records(md.decode_device(LS.N, ptrs))
            assert got == LS.records(runs[df18]), df18
            assert md.stats() == runs[df18]["stats"], df18
            assert md.info()["fallback"] == 0
        finally:
            md.close()
            del own
            torch_cuda.cuda.empty_cache()


# ---- the scan kernel offset by offset at high stream positions ----------------------------------------------------------
# (first sample, samples): a window across sample 2^31 (power sample 2^30), and one that ends at the stream's last sample
HIGH = (((1 << 31) - (1 << 19) + 8), 1 << 20), (((1 << 32) - (1 << 20) + 16), (1 << 20) - 20)
HIGH_CONFIGS = [c for c in CONFIGS if c[0] in ("default", "k2", "k7_big1", "k7_clist1", "k7_nostream")]


@pytest.fixture(scope="module")
def high_cells(oracle, torch_cuda):
    """[(capture name, first_sample, samples on the device, window, {df18: exhaustive (cands, tries) moved to the stream})]"""
    out = []
    for i, (name, x) in enumerate(M.make_captures(1 << 20).items()):
        fs, n = HIGH[i % 2]
        x = np.ascontiguousarray(x[:n])
        pad = fs % 28
        a = oracle.power(np.concatenate([np.full(pad, LS.SILENCE, np.uint16), x]))
        off = (fs - pad) // 2                    # a[k] is the stream's power sample k + off
        gb = -(-(fs // 2 + 6) // 28) * 28
        ge = (fs + n) // 2 - 1195
        ev = {}
        for df18 in (False, True):
            cands, tries = oracle.scan_all(a, gb - off, ge - off, df18)
            ev[df18] = ([(g + off, pw, fr, 0) for g, pw, fr in cands], tries + np.uint64(off << 2))
        out.append((name, fs, x, torch_cuda.from_numpy(x.view(np.int16)).cuda(), gb, ge, ev))
    assert HIGH[1][0] + HIGH[1][1] == LS.N and HIGH[0][0] < (1 << 31) < HIGH[0][0] + HIGH[0][1]
    return out


def _scan(capi, dec, x, t, host, fs, gb, ge):
    if not host:
        cands, nc, tries = dec.scan_shard(t.data_ptr(), fs, x.size, gb, ge)
    else:
        L = capi.load()
        cands, tries = (capi.Candidate * (1 << 16))(), np.empty(1 << 20, dtype=np.uint64)
        ncv, ntv = C.c_size_t(0), C.c_size_t(0)
        rc = L.adsb_scan_shard_host(dec._h, x.ctypes.data, fs, x.size, gb, ge, cands, len(cands), C.byref(ncv),
                                    tries.ctypes.data_as(C.POINTER(C.c_uint64)), tries.size, C.byref(ntv))
        assert rc == 0, (L.adsb_last_error(dec._h) or b"").decode()
        nc, tries = ncv.value, tries[: ntv.value].copy()
    return [(int(c.g), int(c.pw), bytes(c.frame[: c.len]), int(c.reserved)) for c in cands[:nc]], tries


@pytest.mark.limit(120)
@pytest.mark.parametrize("cfg", HIGH_CONFIGS, ids=[c[0] for c in HIGH_CONFIGS])
def test_candidates_offset_by_offset_past_sample_2p31(capi, high_cells, cfg):
    kw = dict(cfg[1])
    df18, stats = kw["df18"], kw["collect_stats"]
    d_all = capi.Decoder(all_candidates=True, **kw)
    d = capi.Decoder(**kw)
    seen = 0
    try:
        for j, (name, fs, x, t, gb, ge, ev) in enumerate(high_cells):
            host = j % 3 == 1
            where = (name, fs, gb, ge, host)
            want, wtries = ev[df18]
            seen += len(want)
            got, tries = _scan(capi, d_all, x, t, host, fs, gb, ge)
            assert got == want, where
            assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
            kept, tries = _scan(capi, d, x, t, host, fs, gb, ge)
            assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
            assert set(kept) <= set(want) and kept == sorted(kept), where
            assert not M.equivalent_from(want, kept, range(gb, min(gb + M.ENTRY_REACH, ge)), ge), where
    finally:
        d_all.close()
        d.close()
    assert seen > 1000


@pytest.mark.limit(120)
def test_shard_primitives_refuse_a_window_that_reaches_2p32(capi, torch_cuda, high_cells):
    """adsb_scan_shard, adsb_scan_shard_host, adsb_scan_shard_resolved[_walk] and adsb_shard_begin: a window up to sample
    2^32 - 4 and a stream of 2^32 - 4 samples go; a window that reaches 2^32 or a stream of 2^32 samples is refused, by a
    message that names the limit, and the handle works on."""
    L = capi.load()
    name, fs, x, _, gb, ge, ev = high_cells[1]
    assert fs + x.size == LS.N
    y = np.concatenate([x, np.full(4, LS.SILENCE, np.uint16)])         # ... up to sample 2^32
    t = torch_cuda.from_numpy(y.view(np.int16)).cuda()
    d = capi.Decoder(df18=True, collect_stats=True, all_candidates=True)
    d2 = capi.Decoder(df18=True, collect_stats=True)

    def refused(rc, h=d):
        msg = (L.adsb_last_error(h._h) or b"").decode()
        assert rc == -1 and "2^32" in msg, (rc, msg)

    try:
        cands = (capi.Candidate * (1 << 16))()
        tries = np.empty(1 << 20, dtype=np.uint64)
        ncv, ntv = C.c_size_t(0), C.c_size_t(0)
        tp = tries.ctypes.data_as(C.POINTER(C.c_uint64))
        for k, ok in ((x.size, True), (y.size, False)):
            rc = L.adsb_scan_shard(d._h, t.data_ptr(), fs, k, gb, ge, cands, len(cands), C.byref(ncv), tp, tries.size, C.byref(ntv))
            assert rc == 0 if ok else refused(rc) is None
            if ok:
                assert [(int(c.g), int(c.pw), bytes(c.frame[: c.len]), 0) for c in cands[: ncv.value]] == ev[True][0]
            rc = L.adsb_scan_shard_host(d._h, y.ctypes.data, fs, k, gb, ge, cands, len(cands), C.byref(ncv), tp, tries.size,
                                        C.byref(ntv))
            assert rc == 0 if ok else refused(rc) is None
        # (no frame is kept by anyone here: the resolved calls are asked for the limit only)
        head = capi.ShardHead()
        frames = (capi.Frame * 4096)()
        hc = (capi.Candidate * 4096)()
        bases = (C.c_uint64 * 64)()
        for k, total, ok in ((x.size, LS.N, True), (y.size, LS.N, False), (x.size, LS.N + 4, False)):
            rc = L.adsb_scan_shard_resolved_walk(d2._h, t.data_ptr(), fs, k, gb, ge, total, C.byref(head), frames, len(frames),
                                                 hc, len(hc), bases, len(bases))
            assert rc == 0 if ok else refused(rc, d2) is None, (k, total)
            if ok:
                assert head.n_frames > 10 and head.g_end == ge
        refused(L.adsb_scan_shard_resolved(d2._h, t.data_ptr(), fs, y.size, gb, ge, C.byref(head), frames, len(frames), hc,
                                           len(hc)), d2)
        for first, total, ok in ((fs, LS.N, True), (fs, LS.N + 4, False), (1 << 32, LS.N + 8, False)):
            rc = L.adsb_shard_begin(d2._h, first, gb, ge, total, None, 0)
            assert rc == 0 if ok else refused(rc, d2) is None, (first, total)
            d2.reset()
        # the handle still scans
        got, _ = _scan(capi, d, x, t, False, fs, gb, ge)
        assert got == ev[True][0]
    finally:
        d.close()
        d2.close()
