"""Decoding through the wraps of the reference's 32-bit sample counter, on the device, against the wrap_stream fixture
(tests/wrap_model.py): the real reference chain's records and Try/Ok table over a stream of 7 * 2^32 + 2^21 samples that is
silence but for nine bursts -- one across each wrap (all seven ring phases), one inside an epoch, one across the end-of-file
horizon.  The silence is one device buffer pushed again and again.

Push boundaries: the stream is cut ON a wrap, 4 samples before it or 4 after it (8 for packed input, whose pushes are whole
groups); the bursts across wraps 4 and 6 go in as ONE push that spans the wrap."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import wrap_model as W

pytestmark = pytest.mark.gpu

SILENCE_SAMPLES = 1 << 29
PREFIX = (1 << 32) + (1 << 21)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def fixture():
    return W.load()


@pytest.fixture(scope="module")
def silence(torch_cuda):
    t = torch_cuda.full((SILENCE_SAMPLES,), W.SILENCE, dtype=torch_cuda.int16, device="cuda")
    yield t
    del t
    torch_cuda.cuda.empty_cache()


class _Silence:
    def __init__(self, t):
        self.t = t
        self.size = t.numel()

    def __getitem__(self, sl):
        return self.t[sl]


def _dev(torch, y):
    return torch.from_numpy(np.ascontiguousarray(y).view(np.int16)).cuda()


def _records(raw):
    from adsbdec_amd import capi
    return [(f["g"], f["ts"], f["pw"], bytes(f["frame"])) for f in capi._frames_to_dicts(*raw)]


def cuts(step):
    """Stream positions at which a push must end: wrap w cut on it, `step` before, `step` after, or not at all."""
    out = set()
    for w in range(1, 8):
        d = (0, -step, step, None, 0, None, step)[w - 1]
        if d is not None:
            out.add(w * (1 << 32) + d)
    return out


def cut_pieces(bursts, silence, step, total=W.N):
    """W.pieces with every piece that holds a cut position split there."""
    cs = sorted(cuts(step))
    for at, y in W.pieces(bursts, silence, total):
        n = y.size if isinstance(y, np.ndarray) else y.numel()
        inner = [c - at for c in cs if at < c < at + n]
        for lo, hi in zip([0] + inner, inner + [n]):
            yield at + lo, y[lo:hi]


def push_stream(capi, torch, d, silence, bursts, how, total=W.N):
    keep = []
    longest = max(y.size for _, y, _ in bursts.values())
    pinned = capi.PinnedBuffers(2, longest)
    bufs = pinned.__enter__()
    spans, on_cut = 0, 0
    try:
        k = 0
        step = 8 if how == "packed" else 4
        for at, y in cut_pieces(bursts, _Silence(silence), step, total):
            n = y.size if isinstance(y, np.ndarray) else y.numel()
            if n == 0:
                continue
            spans += at >> 32 != (at + n - 1) >> 32
            on_cut += at in cuts(step)
            if not isinstance(y, np.ndarray):
                d.push_device(y.data_ptr(), n)
            elif how == "device":
                t = _dev(torch, y)
                keep.append(t)
                d.push_device(t.data_ptr(), n)
            elif how == "sync":
                d.push(np.ascontiguousarray(y))
            elif how in ("async", "overlap"):
                b = bufs[k % 2][:n]
                k += 1
                b[:] = y
                if how == "async":
                    d.push_async(b)
                else:
                    d.push(b)
                    b[:] = 0xFFFF
            elif how == "packed":
                from adsbdec_amd.packed12 import pack12
                assert at % 8 == 0 and n % 8 == 0
                t = torch.from_numpy(pack12(np.ascontiguousarray(y))).cuda()
                keep.append(t)
                d.push_device_packed(t.data_ptr(), n)
            else:
                raise ValueError(how)
        d.sync()
    finally:
        pinned.__exit__(None, None, None)
    if total == W.N:
        assert on_cut == 5 and spans >= 2      # pushes that start on / beside a wrap, and pushes that span one
    return keep


@pytest.mark.limit(240)
@pytest.mark.parametrize("how", ["device", "sync", "async", "overlap", "packed"])
@pytest.mark.parametrize("df18", [False, True])
def test_whole_stream_equals_the_reference(capi, torch_cuda, fixture, silence, how, df18):
    _, bursts, runs = fixture
    d = capi.Decoder(long_stream=True, df18=df18, collect_stats=True, push_overlap=(how == "overlap"))
    try:
        keep = push_stream(capi, torch_cuda, d, silence, bursts, how)
        d.finish()
        got = _records(d.take_raw())
        want = W.records(runs[df18])
        assert len(got) == len(want) and got == want
        assert d.stats() == runs[df18]["stats"]
        wraps, seam = d.wraps()
        assert wraps == 7 and seam == 7 * 1224
        del keep
    finally:
        d.close()


@pytest.mark.limit(240)
@pytest.mark.parametrize("kw", [dict(host_threads=1), dict(), dict(all_candidates=True), dict(host_threads=3)])
def test_whole_stream_with_other_configurations(capi, torch_cuda, fixture, silence, kw):
    _, bursts, runs = fixture
    d = capi.Decoder(long_stream=True, df18=True, collect_stats=True, **kw)
    try:
        keep = push_stream(capi, torch_cuda, d, silence, bursts, "device")
        d.finish()
        assert _records(d.take_raw()) == W.records(runs[True])
        assert d.stats() == runs[True]["stats"]
        assert d.wraps()[0] == 7
        del keep
        # the switch is sticky across a reset: the handle decodes the stream's prefix next, as the reference did
        d.reset()
        keep = push_stream(capi, torch_cuda, d, silence, bursts, "device", total=PREFIX)
        d.finish()
        rec = fixture[0]["prefix"]
        frames = capi._frames_to_dicts(*d.take_raw())
        assert b"".join(capi.format_frame(f, 1) for f in frames).decode() == rec["mlat"]
        assert d.wraps()[0] == 1
    finally:
        d.close()


@pytest.mark.limit(240)
def test_one_bit_repair_against_the_restatement(capi, torch_cuda, fixture, silence):
    """fix_1bit has no reference: every burst but the last equals the restatement's 1-bit repair started just below the burst
    (W.standin); each wrap burst holds a damaged DF17 decoded at P + 5, the last of the seam offsets [P - 1196, P + 5]."""
    _, bursts, runs = fixture
    d = capi.Decoder(long_stream=True, df18=True, collect_stats=True, fix_1bit=True)
    try:
        keep = push_stream(capi, torch_cuda, d, silence, bursts, "device")
        d.finish()
        raw = capi._frames_to_dicts(*d.take_raw())
        stats = d.stats()
        del keep
    finally:
        d.close()
    got = [(f["g"], f["pw"], bytes(f["frame"])) for f in raw]
    fixed = 0
    for name, (s, y, w) in bursts.items():
        if name == "end":
            continue
        want, wstats = W.standin(y, s, True, fix1=True)
        lo, hi = s // 2, (s + y.size) // 2
        assert [r for r in got if lo <= r[0] < hi] == [(g, pw, fr) for g, _, pw, fr in want], name
        if w:
            P = w * W.E
            assert any(g == P + 5 and len(fr) == 14 for g, _, _, fr in want), name   # the repaired frame in the seam offsets
        fixed += wstats["fixed"]
    assert fixed >= 7 and stats["fixed"] >= fixed


@pytest.mark.limit(240)
def test_multi_streams_host_with_two_long_captures(capi, fixture):
    """adsb_multi_decode_streams_host: two captures of 2^32 + 2^21 samples side by side on one device (the same host array
    twice): each equals the reference's run over that prefix; without the switch the call refuses."""
    from adsbdec_amd import sharding
    rec, bursts, _ = fixture
    x = np.full(PREFIX, W.SILENCE, np.uint16)
    for s, y, _ in bursts.values():
        if s < PREFIX:
            x[s: s + y.size] = y
    md = sharding.MultiDecoder(2, [0, 0], df18=True, collect_stats=True)
    try:
        with pytest.raises(sharding.ShardError, match="2\\^32"):
            md.decode_streams_host([x, x])
        md.set_long_streams(True)
        md.decode_streams_host([x, x])
        for k in range(2):
            frames = capi._frames_to_dicts(*md.stream_frames(k))
            assert b"".join(capi.format_frame(f, 1) for f in frames).decode() == rec["prefix"]["mlat"], k
            st = md.stream_stats(k)
            assert {a: {str(b): v for b, v in st[a].items()} for a in ("try", "ok")} == rec["prefix"]["stats"], k
        with pytest.raises(sharding.ShardError, match="2\\^32"):      # one capture sharded over devices keeps its limit
            md.decode_host(x)
    finally:
        md.close()


@pytest.mark.limit(240)
def test_cli_decodes_a_file_of_more_than_8_gib(capi, fixture, tmp_path):
    """adsbdec_amd_cli -a -m -f on the stream's first 2^32 + 2^21 samples: the AVR-MLAT bytes of the reference's own run over
    that prefix.  Zero bytes are not silence, so the file is code 2048 throughout: 8.6 GB really written."""
    rec, bursts, _ = fixture
    need = 2 * PREFIX + (1 << 28)
    if shutil.disk_usage(tmp_path).free < need:
        pytest.skip(f"the temporary directory has less than {need >> 20} MiB free: no room for the 8.6 GB capture")
    path = os.path.join(tmp_path, "prefix.u16")
    try:
        silence = np.full(1 << 26, W.SILENCE, np.uint16)
        with open(path, "wb") as f:
            for _, y in W.pieces(bursts, silence, PREFIX):
                f.write(memoryview(np.ascontiguousarray(y)).cast("B"))
        assert os.path.getsize(path) == 2 * PREFIX
        p = subprocess.run([capi.CLI_PATH, "-a", "-m", "-f", path], capture_output=True, timeout=200)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout.decode() == rec["prefix"]["mlat"]
        tables = [[int(v) for v in ln.split(":")[1].split()] for ln in p.stderr.decode().splitlines()
                  if ":" in ln and len(ln.split(":")[1].split()) == 3 and all(v.isdigit() for v in ln.split(":")[1].split())]
        want = rec["prefix"]["stats"]
        assert [want[k][d] for k in ("try", "ok") for d in ("11", "17", "18")] == tables[0] + tables[1]   # valid.c:84-100
    finally:
        if os.path.exists(path):
            os.remove(path)


@pytest.mark.limit(240)
def test_the_limit_stays_where_the_switch_is_off_and_for_shards(capi, torch_cuda, silence):
    d = capi.Decoder(df18=True)
    try:
        for _ in range(7):
            d.push_device(silence.data_ptr(), SILENCE_SAMPLES)
        d.push_device(silence.data_ptr(), SILENCE_SAMPLES - 4)
        with pytest.raises(capi.AdsbError, match="2\\^32"):
            d.push_device(silence.data_ptr(), 4)
        with pytest.raises(capi.AdsbError, match="fresh or reset"):      # not in the middle of a stream
            d.set_long_stream(True)
        d.reset()
        d.set_long_stream(True)
        for _ in range(8):
            d.push_device(silence.data_ptr(), SILENCE_SAMPLES)
        d.push_device(silence.data_ptr(), 1 << 20)
        assert d.wraps() == (1, 1224)
        d.reset()
        assert d.wraps() == (0, 0)
        # the shard primitives refuse at 2^32 with the switch on, as before
        L = capi.load()
        assert L.adsb_shard_begin(d._h, 0, 0, 1 << 20, 1 << 32, None, 0) != 0
        assert b"2^32" in L.adsb_last_error(d._h)
    finally:
        d.close()
