"""The burst gather on the MI355X (run with -m gpu): adsb_gather_device against the numpy statement (adsbdec_amd/burst_archive.py
gather) for equality, byte for byte.  The output array is filled with poison first and compared WHOLE: the bytes of the pieces, the
zero pad between them, and the poison at and behind `total`.  The capture lies between two stretches of loud decoy, none of whose
bytes is zero: a lane that reads past a piece's end, or past the capture's, puts decoy where a zero belongs.

The shapes are the smallest at which the kernel can still go wrong, C = adsb_gather_chunk_words() 16-byte words a chunk
(tests/gather_cases.py names them); then the call between two pushes of a stream, every refusal, the pipeline (level -> gate ->
gather -> archive -> decode on a flush handle, against the oracle and against the batch decode of the pieces where they lie in the
capture), and the host program's -K and -k."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import burst_cases as BC
import flush_cases as FC
import gather_cases as GC

pytestmark = pytest.mark.gpu

POISON = 0xA5
TAIL = 4096                   # poison bytes behind `total` that are compared too


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def dec_factory(capi, torch_cuda):
    made = {}

    def make(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = capi.Decoder(**kw)
        return made[key]
    yield make
    for d in made.values():
        d.close()


def BA():
    from adsbdec_amd import burst_archive
    return burst_archive


def LV():
    from adsbdec_amd import levels
    return levels


def to_dev(torch, b):
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    t = torch.from_numpy(b if b.flags.writeable else b.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


class Device:
    """A capture between its decoys in HBM, and a poisoned output array."""

    def __init__(self, torch, cap):
        self.torch, self.cap = torch, cap
        both, self.lead = GC.guarded(cap)
        self.t, base = to_dev(torch, both)
        self.ptr = base + self.lead
        self.out = None

    def gather(self, d, tab, M, s, capture_bytes=None, slack=TAIL, out_cap=None):
        """One call, held to the statement: -> (the output's bytes, offsets)."""
        want, woff = BA().gather(self.cap, tab, M, s)
        room = want.size + slack
        if self.out is None or self.out.numel() < room:
            self.out = self.torch.empty(max(room, 1 << 16), dtype=self.torch.uint8, device="cuda")
        self.out.fill_(POISON)
        off = d.gather_device(self.ptr, self.cap.size if capture_bytes is None else capture_bytes, s, M, tab, self.out.data_ptr(),
                              want.size if out_cap is None else out_cap)
        got = self.out[:room].cpu().numpy()
        assert np.array_equal(off, woff), (M, s, tab.size)
        assert np.array_equal(got[:want.size], want), (M, s, tab.size, int(np.flatnonzero(got[:want.size] != want)[0]))
        assert (got[want.size:] == POISON).all(), (M, s, tab.size)
        return got[:want.size], off


# ------------------------------------------------------------------ 1 to 7: the named shapes
@pytest.mark.limit(60)
@pytest.mark.parametrize("s", GC.S_ALL)
def test_named_shapes(capi, dec_factory, torch_cuda, s):
    d = dec_factory()
    Cw = capi.gather_chunk_words()
    cases = GC.named_cases(Cw, s)
    assert cases[0][2].size == 0
    for name, M, tab in cases:
        dev = Device(torch_cuda, GC.capture_bytes(M, s, 21))
        out, off = dev.gather(d, tab, M, s)
        if tab.size == 0:                                    # no burst: 0, nothing launched, nothing written
            assert off.tolist() == [0] and out.size == 0
    # the shapes are what they are meant to be
    for M, tab in [(M, tab) for name, M, tab in cases if name.startswith("every second run a piece")]:
        assert int(BA().layout(tab, M, s)[-1]) // 16 >= 3 * Cw + 5 and tab.size > 3 * Cw // 14
    long_ones = [(M, tab) for name, M, tab in cases if "3 C + 1" in name]
    assert len(long_ones) == 3
    for M, tab in long_ones:
        off = BA().layout(tab, M, s)
        assert int(off[2] - off[1]) // 16 >= 3 * Cw + 1
    M, tab = long_ones[-1]
    assert int(BA().layout(tab, M, s)[2] - BA().layout(tab, M, s)[1]) // 16 == 3 * Cw + 1


@pytest.mark.limit(30)
def test_real_capture_with_trailing_samples(dec_factory, torch_cuda):
    """A uint16 real capture with n % 4 != 0: M = 2 floor(n / 4), the capture's bytes reach beyond 4 M, and the last burst is clipped."""
    d = dec_factory()
    for n in (28 * 2 * 37 + 28 + 1, 28 * 2 * 37 + 28 + 3, 28 * 2 * 37 + 4 + 2):       # M % 28 = 14, 14, 2; n % 4 = 1, 3, 2
        M = 2 * (n // 4)
        assert n % 4 and M % 28
        dev = Device(torch_cuda, GC.loud_bytes(2 * n, 31))
        dev.gather(d, GC.table([(0, 2), (5, 9), (36, 40)]), M, 4)
        # ... and with capture_bytes exactly 4 M
        dev.gather(d, GC.table([(0, 2), (5, 9), (36, 40)]), M, 4, capture_bytes=4 * M)


# ------------------------------------------------------------------ 8: seeded random tables
@pytest.mark.limit(120)
@pytest.mark.parametrize("s", GC.S_ALL)
def test_random_tables(dec_factory, torch_cuda, s):
    d = dec_factory()
    tables = GC.random_tables(300, 5000 + s)
    dev = Device(torch_cuda, GC.capture_bytes(max(M for M, _ in tables), s, 22))
    seen = set()
    for i, (M, tab) in enumerate(tables):
        dev.gather(d, tab, M, s, capture_bytes=s * M)
        seen.add(M % 28)
    assert len(seen) == 28


# ------------------------------------------------------------------ 9: between two pushes of a stream
@pytest.mark.limit(60)
def test_between_two_pushes_of_a_stream(capi, dec_factory, torch_cuda):
    x = FC.real_capture(400_000, 77, extra=tuple((s, (17, 11)[k % 2]) for k, s in enumerate(range(500, 150_000, 9_000))))
    d = dec_factory(df18=True, collect_stats=True)
    want = d.decode(x)
    want_stats = d.stats()
    assert len(want) >= 10
    t, ptr = to_dev(torch_cuda, x)
    M, s = 28 * 500, 4
    dev = Device(torch_cuda, GC.capture_bytes(M, s, 23))
    tab = GC.table([(1, 40), (60, 61), (200, 499)])
    d.reset()
    cut = 8 * 20_000
    d.push_device(ptr, cut)
    dev.gather(d, tab, M, s)
    d.push_device_final(ptr + 2 * cut, x.size - cut)
    d.finish()
    assert d.drain() == want and d.stats() == want_stats
    # ... and on the capture the stream itself is being pushed from
    d.reset()
    d.push_device(ptr, cut)
    got = torch_cuda.full((4096,), POISON, dtype=torch_cuda.uint8, device="cuda")
    off = d.gather_device(ptr, 2 * x.size, 4, 2 * (x.size // 4), GC.table([(3, 5)]), got.data_ptr(), 4096)
    assert off.tolist() == [0, 224] and np.array_equal(got.cpu().numpy()[:224], x.view(np.uint8)[4 * 84:4 * 140])
    d.push_device_final(ptr + 2 * cut, x.size - cut)
    d.finish()
    assert d.drain() == want


# ------------------------------------------------------------------ 10: refusals
@pytest.mark.limit(60)
def test_refusals_leave_the_poison(capi, dec_factory, torch_cuda):
    d = dec_factory()
    L, h = d._L, d._h
    err = lambda: L.adsb_last_error(h).decode()
    M, s = 28 * 20, 4
    cap = GC.capture_bytes(M, s, 24)
    t, ptr = to_dev(torch_cuda, cap)
    out = torch_cuda.full((1 << 16,), POISON, dtype=torch_cuda.uint8, device="cuda")
    ok = GC.table([(1, 3), (5, 8), (10, 12)])
    total = int(BA().layout(ok, M, s)[-1])

    def call(cap_ptr=ptr, capture_bytes=cap.size, s_=s, M_=M, tab=ok, out_ptr=out.data_ptr(), out_cap=1 << 16):
        off = np.full(tab.size + 1, 0x5A5A5A5A, np.uint64)
        rc = L.adsb_gather_device(h, cap_ptr or None, capture_bytes, s_, M_, tab.ctypes.data if tab.size else None, tab.size, out_ptr or None,
                                  out_cap, off.ctypes.data)
        return rc, off

    def refused(word, **kw):
        rc, off = call(**kw)
        assert rc == -1 and word in err(), (word, kw, rc, err())
        assert (off == 0x5A5A5A5A).all()
        assert bool((out == POISON).all()), word

    for name, M_, s_, tab, word in GC.refusals():
        refused(word, s_=s_, M_=M_, tab=tab, capture_bytes=1 << 20)
    refused("capture_bytes", capture_bytes=s * M - 1)
    refused("16-byte aligned", cap_ptr=ptr + 8)
    refused("16-byte aligned", out_ptr=out.data_ptr() + 4)
    refused("NULL capture", cap_ptr=0)
    refused("NULL output", out_ptr=0)
    refused("burst 2", out_cap=total - 16)
    refused("burst 0", out_cap=0)
    refused("burst 1", out_cap=int(BA().layout(ok, M, s)[1]))
    assert "adsb_gather_device" in err()
    assert L.adsb_gather_device(None, ptr, cap.size, s, M, ok.ctypes.data, ok.size, out.data_ptr(), 1 << 16, None) == -1
    # no burst: 0, with NULL pointers too; then the call that works, offsets optional
    empty = GC.table([])
    assert L.adsb_gather_device(h, None, 0, 4, 0, None, 0, None, 0, None) == 0
    rc, off = call(tab=empty)
    assert rc == 0 and off.tolist() == [0] and bool((out == POISON).all())
    assert L.adsb_gather_device(h, ptr, cap.size, s, M, ok.ctypes.data, ok.size, out.data_ptr(), total, None) == total
    got = out.cpu().numpy()
    assert np.array_equal(got[:total], BA().gather(cap, ok, M, s)[0]) and (got[total:] == POISON).all()


# ------------------------------------------------------------------ 11: the pipeline
def shifted(want, begin):
    return [(g + 28 * begin, ts + 28 * begin, pw, fr) for g, ts, pw, fr in want]


@pytest.fixture(scope="module")
def pipe(capi, dec_factory, torch_cuda, tmp_path_factory):
    """The pipeline on the fixture, run once: level -> gate (2, 4) -> gather_device -> archive written and read back -> decode."""
    p = BC.pipeline()
    x, M = p["x"], p["a"].size
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    t, ptr = to_dev(torch_cuda, x)
    n_env = -(-M // 28)
    te, pe = to_dev(torch_cuda, np.zeros(n_env, np.float32))
    rep = d.level_device_iq(2, ptr, len(x), pe, n_env)
    threshold = float(np.float32(BC.FACTOR * capi.level_percentile(rep["hist"], 0.5)))
    tab, b = d.bursts_device(pe, n_env, threshold, 2, 4, 64)
    want_bytes, want_off = BA().gather(x, tab, M, 4)
    out = torch_cuda.full((want_bytes.size + TAIL,), POISON, dtype=torch_cuda.uint8, device="cuda")
    off = d.gather_device(ptr, x.nbytes, 4, M, tab, out.data_ptr(), want_bytes.size)
    got = out.cpu().numpy()
    path = tmp_path_factory.mktemp("pipe") / "pipe.brs"
    BA().write(path, 2, len(x), M, threshold, 2, 4, tab, got[:want_bytes.size])
    frames, stats = BA().decode(d, BA().read(path))
    return dict(d=d, rep=rep, threshold=threshold, tab=tab, b=b, want_bytes=want_bytes, want_off=want_off, off=off, got=got, frames=frames,
                stats=stats, archive=path.read_bytes(), ptr=ptr, out=out, keep=(t, te))


@pytest.mark.limit(120)
def test_pipeline(oracle, pipe):
    """The oracle on each piece's silent twin with g and ts shifted by 28 begin, and what decode_batch_device_iq returns for pointers
    into the original capture -- gathering changes nothing.  All 36 planted frames are found, in under 1 % of the capture's bytes."""
    p = BC.pipeline()
    x, M = p["x"], p["a"].size
    d, tab, want_bytes, got, off, ptr = (pipe[k] for k in ("d", "tab", "want_bytes", "got", "off", "ptr"))
    assert pipe["rep"]["samples"] == M and pipe["threshold"] == p["threshold"]
    assert pipe["b"] == 36 and np.array_equal(tab, LV().bursts(p["env"], p["threshold"], 2, 4))
    assert np.array_equal(off, pipe["want_off"]) and np.array_equal(got[:want_bytes.size], want_bytes) and (got[want_bytes.size:] == POISON).all()
    assert want_bytes.size < 0.01 * x.nbytes
    sl = LV().burst_samples(tab, M)
    want, want_stats = [], {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for r, (lo, hi) in zip(tab, sl):
        w, st = FC.want_power(oracle, np.ascontiguousarray(p["a"][lo:hi]))
        want += shifted(w, int(r["begin"]))
        for k in ("try", "ok"):
            for df in (11, 17, 18):
                want_stats[k][df] += st[k][df]
    assert FC.recs(pipe["frames"]) == want
    assert {k: pipe["stats"][k] for k in ("try", "ok")} == want_stats
    found = {f["frame"] for f in pipe["frames"]}
    assert len(p["truth"]) == 36 and all(fr in found for _, fr in p["truth"])
    # pointers into the original capture: the same records
    ptrs, ns = [ptr + 4 * int(lo) for lo, _ in sl], [int(hi - lo) for lo, hi in sl]
    direct = d.decode_batch_device_iq(2, ptrs, ns)
    assert [rec for r, mine in zip(tab, direct) for rec in shifted(FC.recs(mine), int(r["begin"]))] == want
    # ... and pointers into the gathered array on the device
    inplace = d.decode_batch_device_iq(2, [pipe["out"].data_ptr() + int(o) for o in off[:-1]], ns)
    assert [rec for r, mine in zip(tab, inplace) for rec in shifted(FC.recs(mine), int(r["begin"]))] == want


@pytest.mark.limit(60)
def test_pipeline_on_a_real_capture(capi, oracle, dec_factory, torch_cuda, tmp_path):
    """The same equality on a small uint16 real capture, against flush_cases' real twin of each piece.  (Nothing is claimed about
    which frames the gate keeps here.)"""
    from tools import gen_signal as G
    x, _ = G.sparse_capture(600_002, 12, seed=5)
    M = 2 * (x.size // 4)
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    t, ptr = to_dev(torch_cuda, x)
    n_env = -(-M // 28)
    te, pe = to_dev(torch_cuda, np.zeros(n_env, np.float32))
    rep = d.level_device(ptr, x.size, pe, n_env)
    threshold = float(np.float32(48.0 * capi.level_percentile(rep["hist"], 0.5)))
    tab, b = d.bursts_device(pe, n_env, threshold, 2, 4, 4096)
    assert 1 <= b <= 4096
    want_bytes, want_off = BA().gather(x, tab, M, 4)
    out = torch_cuda.full((want_bytes.size + TAIL,), POISON, dtype=torch_cuda.uint8, device="cuda")
    off = d.gather_device(ptr, x.nbytes, 4, M, tab, out.data_ptr(), want_bytes.size)
    got = out.cpu().numpy()
    assert np.array_equal(off, want_off) and np.array_equal(got[:want_bytes.size], want_bytes) and (got[want_bytes.size:] == POISON).all()
    BA().write(tmp_path / "real.brs", 4, x.size, M, threshold, 2, 4, tab, got[:want_bytes.size])
    frames, stats = BA().decode(d, BA().read(tmp_path / "real.brs"))
    sl = LV().burst_samples(tab, M)
    want = []
    for r, (lo, hi) in zip(tab, sl):
        want += shifted(FC.want_real(oracle, x[2 * lo:2 * hi])[0], int(r["begin"]))
    assert FC.recs(frames) == want
    direct = d.decode_batch_device([ptr + 4 * int(lo) for lo, _ in sl], [2 * int(hi - lo) for lo, hi in sl])
    assert [rec for r, mine in zip(tab, direct) for rec in shifted(FC.recs(mine), int(r["begin"]))] == want


# ------------------------------------------------------------------ 12: the host program
@pytest.mark.limit(120)
def test_host_program_keeps_and_decodes(capi, oracle, pipe, tmp_path):
    """-L -U 48,2,4 -K out.brs -q 2 -f capture, then -k -a -f out.brs: the .brs is Python's byte for byte, the packets are the
    pipeline's."""
    p = BC.pipeline()
    (tmp_path / "c.iq16").write_bytes(p["x"].tobytes())
    q = subprocess.run([capi.CLI_PATH, "-L", "-U", "48,2,4", "-K", str(tmp_path / "out.brs"), "-q", "2", "-f", str(tmp_path / "c.iq16")],
                       capture_output=True, timeout=100)
    err = q.stderr.decode()
    assert q.returncode == 0, err
    arch = BA().unpack(pipe["archive"])
    whole = 4 * arch["M"]
    assert f"kept 36 bursts, {arch['payload'].size} of {whole} bytes" in err
    assert b"bursts 36 threshold" in q.stdout
    assert (tmp_path / "out.brs").read_bytes() == pipe["archive"]
    for flags, fmt in ((["-a"], 0), (["-a", "-m"], 1)):
        k = subprocess.run([capi.CLI_PATH, "-k", *flags, "-f", str(tmp_path / "out.brs")], capture_output=True, timeout=100)
        assert k.returncode == 0, k.stderr.decode()
        assert k.stdout == oracle.avr_lines(pipe["frames"], fmt), flags
        assert b"Try :" in k.stderr and b"Ok :" in k.stderr
    # without -a the DF18 frames are not decoded: fewer packets, not more
    k = subprocess.run([capi.CLI_PATH, "-k", "-f", str(tmp_path / "out.brs")], capture_output=True, timeout=100)
    assert k.returncode == 0 and 0 < len(k.stdout) < len(oracle.avr_lines(pipe["frames"], 0))


@pytest.mark.limit(60)
def test_host_program_writes_no_archive_without_a_threshold(capi, torch_cuda, tmp_path):
    """-K on a capture with no sign-clear power sample: the gate has no median to take a threshold from, so the run says so, ends with
    status 255 and writes no archive (and not an empty one with threshold 0)."""
    (tmp_path / "neg.pw").write_bytes(np.full(28 * 100, -1.0, dtype="<f4").tobytes())
    q = subprocess.run([capi.CLI_PATH, "-L", "-U", "48,2,4", "-K", str(tmp_path / "out.brs"), "-w", "-f", str(tmp_path / "neg.pw")],
                       capture_output=True, timeout=50)
    assert q.returncode == 255 and b"no archive is written" in q.stderr, q.stderr.decode()
    assert b"bursts 0 threshold none" in q.stdout and not (tmp_path / "out.brs").exists()
