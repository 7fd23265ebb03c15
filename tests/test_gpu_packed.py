"""Airspy packed 12-bit input on the MI355X: the unpack kernel alone, every packed ingress of one handle (host pushes in the
three modes, mixed streams, device-resident captures), the golden fixtures, and the C host program's -p against the real
reference on the unpacked twin.  The definition every result is checked against is the numpy one (adsbdec_amd/packed12.py)
and the uint16 path: a packed capture must decode exactly like its unpacked twin."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def dec_factory(capi, torch_cuda):
    made = []

    def make(**kw):
        d = capi.Decoder(**kw)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


def _pack(x):
    from adsbdec_amd.packed12 import pack12
    return pack12(x)


def _table(stderr: bytes):
    """The Try/Ok rows of the stderr table (valid.c:84-100), wherever they are in the output."""
    text = stderr.decode()
    tr = re.search(r"^Try :(.*)$", text, flags=re.M).group(1).split()
    ok = re.search(r"^Ok :(.*)$", text, flags=re.M).group(1).split()
    return [int(v) for v in tr], [int(v) for v in ok]


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.limit(120)
@pytest.mark.parametrize("groups", [1, 7, (1 << 20) + 3])
def test_unpack_kernel_alone(capi, torch_cuda, groups):
    """adsb_unpack_packed12 == packed12.unpack12, at destination offsets that are multiples of 8 samples; nothing outside
    the destination range is written.  Misaligned pointers and n % 8 != 0 are refused with a message."""
    torch = torch_cuda
    L = capi.load()
    n = 8 * groups
    x = np.random.default_rng(groups).integers(0, 4096, n, dtype=np.uint16)
    src = torch.from_numpy(_pack(x)).cuda()
    for off in (0, 8, 64, 4104):
        dst = torch.full((off + n + 64,), 0x7777, dtype=torch.int16, device="cuda")
        assert L.adsb_unpack_packed12(dst.data_ptr() + 2 * off, src.data_ptr(), n, None) == 0, L.adsb_last_error(None)
        torch.cuda.synchronize()
        got = dst.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[off: off + n], x), off
        assert (got[:off] == 0x7777).all() and (got[off + n:] == 0x7777).all(), off
    dst = torch.zeros(n + 64, dtype=torch.int16, device="cuda")
    assert L.adsb_unpack_packed12(dst.data_ptr(), src.data_ptr(), 7, None) == -1 and b"multiple of 8" in L.adsb_last_error(None)
    assert L.adsb_unpack_packed12(dst.data_ptr() + 8, src.data_ptr(), 8, None) == -1 and b"aligned" in L.adsb_last_error(None)
    assert L.adsb_unpack_packed12(dst.data_ptr(), src.data_ptr() + 2, 8, None) == -1 and b"aligned" in L.adsb_last_error(None)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all()


# ------------------------------------------------------------------ host pushes
N_HOST = (9 << 20) + 8 * 37     # > 2 x (4 Mi + 8): the largest chunk is pushed more than once
_captures = {}


def _capture(oracle, kind, df18):
    key = (kind, df18)
    if key not in _captures:
        from tools import gen_signal as G
        if kind == "sparse":
            x, _ = G.sparse_capture(N_HOST, n_frames=1500, seed=61 + df18, sigma=8.0, dfs=(17, 18, 11))
        else:
            x, _ = G.dense_capture(N_HOST, seed=71 + df18, sigma=300.0, n_frames=3000, amp=(150, 1900))
        assert x.max() <= 4095
        subsets = {}
        for n in (64 << 10, 1 << 20, N_HOST):       # prefixes the small chunks run on (8-sample pushes of 9 Mi would take minutes)
            subsets[n] = (x[:n], _pack(x[:n])) + tuple(oracle.decode(x[:n], df18=df18))
        _captures[key] = subsets
    return _captures[key]


# (chunk in samples, prefix of the capture, stage_samples); each in the sync, async and push_overlap modes
PATHS = [(8, 64 << 10, 0), (8 * 131, 1 << 20, 0), (1 << 20, N_HOST, 0), ((4 << 20) + 8, N_HOST, 0),
         (8 * 131, 1 << 20, 64 << 10), (1 << 20, N_HOST, 64 << 10)]


@pytest.mark.limit(900)
@pytest.mark.parametrize("kind,df18", [("sparse", False), ("sparse", True), ("dense", False), ("dense", True)])
def test_host_pushes_equal_the_unpacked_twin(capi, oracle, dec_factory, kind, df18):
    """push_packed in chunks of 8, 8*131, 1 Mi (the reference's call size) and 4 Mi + 8 samples, in sync, async and push_overlap
    modes, and with a 64 Ki-sample staging buffer (every piece compacts): frames (g, ts, pw, bytes) and Try/Ok equal the
    oracle on the unpacked twin and the same decoder's uint16 path."""
    cap = _capture(oracle, kind, df18)
    for chunk, n, stage in PATHS:
        x, p, want, wstats = cap[n]
        assert len(want) > 0 or n == 64 << 10
        for mode in ("sync", "async", "overlap"):
            d = dec_factory(df18=df18, collect_stats=True, stage_samples=stage, push_overlap=(mode == "overlap"))
            what = f"{kind} df18={df18} chunk={chunk} n={n} stage={stage} mode={mode}"
            got = d.decode_packed(p, chunk=chunk, mode=mode)
            assert records(got) == records(want), what
            assert d.stats() == wstats, what
            u16 = d.decode(x, chunk=chunk, mode=mode)
            assert records(u16) == records(got), what
            assert d.stats() == wstats, what
            d.close()


@pytest.mark.limit(300)
@pytest.mark.parametrize("asynchronous", [False, True])
def test_mixed_stream_and_refusals(capi, oracle, dec_factory, asynchronous):
    """uint16 and packed pushes interleaved at 8-aligned positions decode like the whole capture.  A packed push at a position
    that is not a multiple of 8, or of a sample count that is not, fails with a message and leaves the handle as it was: the
    stream then goes on (as uint16) and decodes correctly."""
    from tools import gen_signal as G
    x, _ = G.dense_capture(3 << 20, seed=91, sigma=40.0, n_frames=600, amp=(150, 1800))
    want, wstats = oracle.decode(x, df18=True)
    assert len(want) > 100
    cuts = [0, 8 * 1000, 8 * 9000, 8 * 9003, 8 * 100_000, 8 * 100_001, 1 << 20, (1 << 20) + 8 * 5, x.size]
    assert cuts == sorted(cuts)
    d = dec_factory(df18=True, collect_stats=True)
    push_u16 = d.push_async if asynchronous else d.push
    push_p12 = d.push_packed_async if asynchronous else d.push_packed
    keep = []                                         # (async: the pieces stay borrowed until the next call)
    out = []
    d.reset()
    for k in range(len(cuts) - 1):
        piece = np.ascontiguousarray(x[cuts[k]:cuts[k + 1]])
        if k % 2:
            piece = _pack(piece)
        keep.append(piece)
        (push_p12 if k % 2 else push_u16)(piece)
        out += d.drain()
    d.finish()
    out += d.drain()
    assert records(out) == records(want)
    assert d.stats() == wstats

    d.reset()
    head = np.ascontiguousarray(x[:13])
    push_u16(head)
    p = _pack(x[16:16 + 8 * 100])
    with pytest.raises(capi.AdsbError, match="stream position 13: packed input must start at a multiple of 8"):
        push_p12(p)
    with pytest.raises(capi.AdsbError, match="n = 12 is not a multiple of 8"):
        push_p12((p.ctypes.data, 12))
    rest = np.ascontiguousarray(x[13:])
    push_u16(rest)
    d.finish()
    assert records(d.drain()) == records(want)
    assert d.stats() == wstats


# ------------------------------------------------------------------ device-resident captures
def _pack_on_device(torch, t):
    """The uint16 capture t (int16 view) packed on the device with torch integer ops -> uint8 tensor (12 bytes per 8 samples)."""
    s = t.view(-1, 8).to(torch.int64) & 0xFFF
    w = [(s[:, 0] << 20) | (s[:, 1] << 8) | (s[:, 2] >> 4),
         ((s[:, 2] & 0xF) << 28) | (s[:, 3] << 16) | (s[:, 4] << 4) | (s[:, 5] >> 8),
         ((s[:, 5] & 0xFF) << 24) | (s[:, 6] << 12) | s[:, 7]]
    del s
    out = torch.empty((t.numel() // 8, 12), dtype=torch.uint8, device=t.device)
    for q in range(3):
        for j in range(4):
            out[:, 4 * q + j] = ((w[q] >> (8 * j)) & 0xFF).to(torch.uint8)
    return out.view(-1)


def _frames(capi, res):
    ptr, k = res
    return [(f["g"], f["ts"], f["pw"], f["frame"]) for f in capi._frames_to_dicts(ptr, k)]


def _counters(d):
    p = d.profile()
    return {k: p[k] for k in ("launches", "relaunches", "offsets", "candidates", "big_offsets")}


@pytest.mark.limit(900)
def test_device_resident_configs1(capi, dec_factory, torch_cuda):
    """BASELINE configs[1] (256 Mi samples, make_workload), packed on the device: decode_device_packed equals decode_device on
    the uint16 capture -- frames, ts checksum, Try/Ok and the launch counters -- and so does push_device_packed in three
    unequal pieces (the first one small enough to be staged) plus _final.  A pointer not aligned to 4 bytes is refused."""
    torch = torch_cuda
    from tools.gen_signal import make_workload
    n = 256 << 20
    t, truth = make_workload(torch, n, seed=1)
    p = _pack_on_device(torch, t)
    torch.cuda.synchronize()
    assert p.numel() == n // 8 * 12
    # the device packing agrees with the numpy definition on a slice
    from adsbdec_amd.packed12 import unpack12
    assert np.array_equal(unpack12(p[: 12 * 4096].cpu().numpy()), t[: 8 * 4096].cpu().numpy().view(np.uint16))

    d = dec_factory(collect_stats=True)
    c0 = _counters(d)
    want = _frames(capi, d.decode_device_raw(t.data_ptr(), n))
    wstats = d.stats()
    c1 = _counters(d)
    got = _frames(capi, d.decode_device_packed_raw(p.data_ptr(), n))
    assert d.stats() == wstats
    c2 = _counters(d)
    assert len(want) > 0.9 * len(truth)
    assert got == want
    assert sum(f[1] for f in got) == sum(f[1] for f in want)          # ts checksum
    assert {k: c1[k] - c0[k] for k in c0} == {k: c2[k] - c1[k] for k in c0}

    cuts = [0, 8 * 5000, 8 * 11_000_017, n]
    d.reset()
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        (d.push_device_packed_final if k == 2 else d.push_device_packed)(p.data_ptr() + a // 8 * 12, b - a)
    assert [(f["g"], f["ts"], f["pw"], f["frame"]) for f in d.drain()] == want
    assert d.stats() == wstats

    d.reset()
    with pytest.raises(capi.AdsbError, match="not 4-byte aligned"):
        d.push_device_packed(p.data_ptr() + 2, 8 * 1000)
    with pytest.raises(capi.AdsbError, match="not 4-byte aligned"):
        d.decode_device_packed_raw(p.data_ptr() + 1, n - 8)
    with pytest.raises(capi.AdsbError, match="not a multiple of 8"):
        d.push_device_packed(p.data_ptr(), 8 * 1000 + 4)
    d.push_device_packed_final(p.data_ptr(), 8 * 100_000)           # the handle was left as it was: a fresh stream decodes
    head, _ = torch.split(t, [8 * 100_000, n - 8 * 100_000])
    e = dec_factory(collect_stats=True)
    e.push_device_final(head.data_ptr(), head.numel())
    assert records(d.drain()) == records(e.drain())
    assert d.stats() == e.stats()
    del p, t
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ golden fixtures
@pytest.mark.limit(120)
@pytest.mark.parametrize("name", golden_cases())
def test_golden_packed(capi, dec_factory, torch_cuda, name):
    """Every committed fixture whose codes fit 12 bits and whose length is a whole number of groups, pushed packed (host and
    device), gives its records and Try/Ok table."""
    x, rec = load_golden(name)
    if x.size and int(x.max()) > 4095:
        pytest.skip(f"{name}: codes up to {int(x.max())} (> 4095) have no packed 12-bit form")
    if x.size % 8:
        pytest.skip(f"{name}: {x.size} samples is not a whole number of 8-sample groups")
    p = _pack(x)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    assert records(d.decode_packed(p, chunk=1 << 20)) == golden_records(rec)
    assert d.stats() == rec["stats"]
    t = torch_cuda.from_numpy(p).cuda()
    assert records(capi._frames_to_dicts(*d.decode_device_packed_raw(t.data_ptr(), x.size))) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ the C host program against the real reference
@pytest.mark.limit(900)
def test_cli_packed_equals_real_reference_on_the_unpacked_twin(capi, oracle, tmp_path):
    """adsbdec_amd_cli -p on a packed file larger than two ring buffers: the same stdout bytes (AVR, AVR-MLAT, Beast) and Try/Ok
    table as the real reference chain on the unpacked uint16 file; the same with 7 trailing bytes (ignored, and stderr says so)
    and through a pipe."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref (the compiled reference) did not travel with this snapshot")
    from tools import gen_signal as G
    x, _ = G.dense_capture((40 << 20) + 8 * 3, seed=307, sigma=25.0, n_frames=4000, amp=(150, 1800))
    assert x.max() <= 4095
    u16, p12, cut = str(tmp_path / "x.u16"), str(tmp_path / "x.p12"), str(tmp_path / "cut.p12")
    x.tofile(u16)
    p = _pack(x)
    p.tofile(p12)
    with open(cut, "wb") as f:
        f.write(p.tobytes() + bytes(range(7)))
    assert os.path.getsize(cut) % 12 == 7
    rf, rstats = oracle.ref_decode(None, True, path=u16)
    assert len(rf) > 1000
    table = ([rstats["try"][k] for k in (11, 17, 18)], [rstats["ok"][k] for k in (11, 17, 18)])
    for flag, key in (([], "avr"), (["-m"], "mlat"), (["-b"], "beast")):
        for path, ignored in ((p12, None), (cut, 7)):
            r = subprocess.run([capi.CLI_PATH, "-p", "-a"] + flag + ["-f", path], capture_output=True, timeout=600)
            assert r.returncode == 0, r.stderr
            assert r.stdout == b"".join(f[key] for f in rf), (flag, path)
            assert _table(r.stderr) == table
            if ignored:
                assert b"7 trailing bytes ignored" in r.stderr
            else:
                assert b"ignored" not in r.stderr
    with open(cut, "rb") as f:
        r = subprocess.run([capi.CLI_PATH, "-p", "-a", "-f", "/dev/stdin"], stdin=f, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"".join(f["avr"] for f in rf)
    assert _table(r.stderr) == table and b"7 trailing bytes ignored" in r.stderr
