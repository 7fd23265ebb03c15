"""Complex (IQ) captures on the MI355X (run with -m gpu): the scan kernels' IQ front end and every _iq call of the library, held
to the reference's demodulator on the numpy definition of the power samples (adsbdec_amd/sample_formats.py iq_power): the
committed fixtures (tests/golden/iq, minted through oracle/_ref/ref_adsbdec -p), the kernel's candidates offset by offset,
chunked and staged streams, batches, the float32 conversion, the refusals, the 1-bit repair and the C host program's -q."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import golden_records, records
from test_iq_cpu import edge_bits, iq_cases, load_iq

pytestmark = pytest.mark.gpu

F32_IQ, S16_IQ = 0, 2
FMTS = [S16_IQ, F32_IQ]


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


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def to_dev(torch, a, lead=0):
    """A numpy array as bytes on the device behind `lead` bytes of padding: (tensor that keeps the memory alive, pointer)."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), b])).cuda()
    assert t.data_ptr() % 256 == 0 or t.numel() == 0
    return t, t.data_ptr() + lead


def as_fmt(fmt, x):
    """The int16 capture x in format fmt (the float twin is exact: x / 32768)."""
    return x if fmt == S16_IQ else S().to_float32_iq(x)


# ------------------------------------------------------------------ 1. the fixtures through every call
@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", iq_cases())
def test_fixtures_through_every_call(capi, dec_factory, torch_cuda, name, fmt):
    """Frames (g, ts, pw, bytes) and Try/Ok of every fixture through push_iq + finish, push_iq_async, push_device_iq_final and
    decode_device_iq, as int16 and as its exact float twin (whose report says: every scalar converted, none off the grid)."""
    x, rec = load_iq(name)
    want, n = golden_records(rec), len(x)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    src = as_fmt(fmt, x)
    t, ptr = to_dev(torch_cuda, src)
    report = (2 * n, 0, 0) if fmt == F32_IQ else (0, 0, 0)

    def check(frames, how):
        assert records(frames) == want, (how, len(frames), len(want))
        assert d.stats() == rec["stats"], how
        assert d.format_report() == report, how

    check(d.decode_iq(fmt, src), "push_iq + finish")
    check(d.decode_iq(fmt, src, chunk=30_001, mode="async"), "push_iq_async")
    d.reset()
    d.push_device_iq(fmt, ptr, n, final=True)
    check(d.drain(), "push_device_iq_final")
    check(d.decode_device_iq(fmt, ptr, n), "decode_device_iq")


# ------------------------------------------------------------------ 2. offset by offset
N_BIG = 1 << 20
K_BIG = 2                                   # passes per tile of the launches below: tile_offsets(2) = 28 * (252 * 2 - 44)
TILE = 28 * (252 * K_BIG - 44)
_big = {}


def big_capture(oracle):
    """One capture of 1 Mi complex samples: frames at -1195, -600, -1 and 0 around the first twelve tile boundaries of a K = 2
    launch (each placement at three of them), then ~700 frames 1201 + k samples apart (k = 0 .. 28 in turn: every offset mod 28, every lane of a wave -- 62 and 63
    and the wave and pass boundaries included -- many times over), one frame at g = 0, one that ends on the last sample.  With
    the oracle's exhaustive evaluation of every offset and its greedy decode."""
    if not _big:
        from tools import gen_signal as G
        rng = np.random.default_rng(77)
        starts = [0] + [b * TILE + (-1195, -600, -1, 0)[(b - 1) % 4] for b in range(1, 13)]   # (one per boundary: closer, they would overlap)
        s = 13 * TILE
        k = 0
        while s + 1201 + 28 + 1200 < N_BIG - 1300:
            starts.append(s)
            s += 1201 + k % 29
            k += 1
        starts.append(N_BIG - 1200)
        assert len(starts) > 700 and len({st % 28 for st in starts}) == 28
        frames = [(st, G.make_frame((17, 18, 11)[i % 3] if st != N_BIG - 1200 else 17, rng), float(rng.uniform(300, 1500)),
                   float(rng.uniform(0, 2 * np.pi))) for i, st in enumerate(starts)]
        x = G.iq_synth(N_BIG, frames, 4.0, 77)
        a = S().iq_power(x)
        _big.update(x=x, a=a, starts=starts, all=oracle.scan_all(a, 0, N_BIG - 1195, True), dec=oracle.demod_power(a, df18=True))
        assert len(_big["dec"][0]) > 690
    return _big


@pytest.mark.limit(180)
def test_candidates_offset_by_offset(capi, oracle, dec_factory, torch_cuda):
    """all_candidates = 1: every CRC-valid offset the device reports -- (g, pw, bytes) -- and, with collect_stats, every DF-gate
    pass equal the oracle's exhaustive evaluation of all n - 1195 offsets of iq_power(x).  The list is read back through the
    batch call (adsb_batch_records: scan_iq_batch_kernel); the stream calls (scan_iq_kernel) have no such read-out and are held
    to the greedy decode of the same capture here, with and without the never-visited filter, at K = 2 and the default K."""
    big = big_capture(oracle)
    x = big["x"]
    t, ptr = to_dev(torch_cuda, x)
    want_c, want_t = big["all"]
    d = dec_factory(df18=True, collect_stats=True, all_candidates=True, debug_passes=K_BIG)
    frames, stats = d.decode_batch_device_iq(S16_IQ, [ptr], [N_BIG], stats=True)
    cands, tries, segs, launches = d.batch_records()
    assert all(l["passes"] == K_BIG for l in launches)
    base = segs[0]["base"]
    assert [(g - base, pw, fr) for g, pw, fr, _ in cands] == want_c
    assert np.array_equal(np.sort(tries - np.uint64(base << 2)), np.sort(want_t))    # words (g << 2) | DF code
    got_g = {c[0] for c in want_c}
    for st in big["starts"]:                               # every planted frame is a candidate at its own offset
        assert st in got_g, st
    wf, ws = big["dec"]
    assert records(frames[0]) == records(wf) and stats[0] == ws
    for kw in (dict(all_candidates=True, debug_passes=K_BIG), dict(debug_passes=K_BIG), dict(), dict(debug_passes=7)):
        ds = dec_factory(df18=True, collect_stats=True, **kw)
        assert records(ds.decode_device_iq(S16_IQ, ptr, N_BIG)) == records(wf), kw
        assert ds.stats() == ws, kw


# ------------------------------------------------------------------ 3. chunking
@pytest.mark.limit(180)
@pytest.mark.parametrize("fmt", FMTS)
def test_chunked_and_staged_streams_equal_one_aligned_push(capi, oracle, dec_factory, torch_cuda, fmt):
    """The capture of test 2 pushed in pieces of 1, 3, 7, 4 099, 65 537 and the rest, from the host and from the device, and
    in one piece from a device pointer one complex sample past a 16-byte boundary (the staged path): the frames and the Try/Ok
    table of one aligned push, which are the oracle's."""
    big = big_capture(oracle)
    src = as_fmt(fmt, big["x"])
    wf, ws = big["dec"]
    elem = src.dtype.itemsize * 2
    d = dec_factory(df18=True, collect_stats=True)
    t, ptr = to_dev(torch_cuda, src)
    assert records(d.decode_device_iq(fmt, ptr, N_BIG)) == records(wf) and d.stats() == ws
    cuts = np.cumsum([0, 1, 3, 7, 4099, 65537]).tolist() + [N_BIG]
    d.reset()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.push_iq(fmt, src[lo:hi])
    d.finish()
    assert records(d.drain()) == records(wf) and d.stats() == ws
    d.reset()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.push_device_iq(fmt, ptr + elem * lo, hi - lo)
    d.finish()
    assert records(d.drain()) == records(wf) and d.stats() == ws
    t1, p1 = to_dev(torch_cuda, src, lead=4 if fmt == S16_IQ else 8)
    assert p1 % 16 != 0
    assert records(d.decode_device_iq(fmt, p1, N_BIG)) == records(wf) and d.stats() == ws
    d.reset()
    d.push_device_iq(fmt, p1, N_BIG // 2)
    d.push_device_iq(fmt, p1 + elem * (N_BIG // 2), N_BIG // 2, final=True)
    assert records(d.drain()) == records(wf) and d.stats() == ws


# ------------------------------------------------------------------ 4. batches
@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
def test_batches_equal_the_single_calls(capi, dec_factory, torch_cuda, fmt):
    """Six captures -- 0, 1, 40 979 and 40 982 samples and two fixtures -- through the device call and the host call: every
    capture's frames and Try/Ok table are those of its own decode_device_iq."""
    mixed, _ = load_iq("mixed_df_a")
    full, _ = load_iq("full_scale")
    ragged, _ = load_iq("ragged")
    caps = [as_fmt(fmt, c) for c in (mixed[:0], mixed[:1], ragged[:40979], ragged[:40982], mixed, full)]
    d = dec_factory(df18=True, collect_stats=True)
    held = [to_dev(torch_cuda, c) for c in caps]
    single = []
    for c, (_, p) in zip(caps, held):
        single.append((records(d.decode_device_iq(fmt, p, len(c))), d.stats()))
    assert single[3][0] and single[4][0] and single[5][0] and not single[0][0] and not single[2][0]
    frames, stats = d.decode_batch_device_iq(fmt, [p if len(c) else 0 for c, (_, p) in zip(caps, held)], [len(c) for c in caps], stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    if fmt == F32_IQ:
        assert d.format_report() == (2 * sum(len(c) for c in caps), 0, 0)
    frames, stats = d.decode_batch_iq(fmt, caps, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    if fmt == S16_IQ:      # device captures that are only 4-byte aligned take the copy
        held4 = [to_dev(torch_cuda, c, lead=4) for c in caps]
        frames, stats = d.decode_batch_device_iq(fmt, [p for _, p in held4], [len(c) for c in caps], stats=True)
        assert [(records(f), s) for f, s in zip(frames, stats)] == single


# ------------------------------------------------------------------ 5. the float32 conversion
@pytest.mark.limit(120)
def test_float32_conversion_on_the_device(capi, dec_factory, torch_cuda):
    """The CPU test's edge vector through the conversion kernel: codes and the two counts are numpy's.  An off-grid capture
    reports inexact scalars and decodes as its quantised twin."""
    torch = torch_cuda
    L = capi.load()
    bits = edge_bits()
    r, inexact, clamped = S().flags_float32_iq(bits.view("<f4"))
    t, p = to_dev(torch, bits)
    for doff in (0, 1, 5):
        dst = torch.full((64 + doff + bits.size + 64,), 0x7777, dtype=torch.int16, device="cuda")
        counters = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
        assert L.adsb_convert_iq_float32(dst.data_ptr() + 2 * (64 + doff), p, bits.size, counters.data_ptr(), None) == 0, L.adsb_last_error(None)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got[64 + doff: 64 + doff + bits.size], r), doff
        assert (got[:64 + doff] == 0x7777).all() and (got[64 + doff + bits.size:] == 0x7777).all()
        assert counters.cpu().tolist() == [5 + int(inexact.sum()), 7 + int(clamped.sum())]
    x, rec = load_iq("mixed_df_a")
    rng = np.random.default_rng(5)
    off = (S().to_float32_iq(x).astype(np.float64) + rng.uniform(-0.45, 0.45, x.shape) / 32768.0).astype("<f4")
    off[100] = [np.nan, 7.0]
    q, wi, wc = S().to_int16_iq(off)
    assert wi > x.size // 2 and wc == 2
    d = dec_factory(df18=True, collect_stats=True)
    tq, pq = to_dev(torch, q)
    want = records(d.decode_device_iq(S16_IQ, pq, len(q)))
    to, po = to_dev(torch, off)
    assert records(d.decode_device_iq(F32_IQ, po, len(off))) == want and len(want) > 20
    assert d.format_report() == (off.size, wi, wc)
    assert records(d.decode_iq(F32_IQ, off, chunk=10_007)) == want
    assert d.format_report() == (off.size, wi, wc)


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.limit(120)
def test_refusals_leave_the_stream_as_it_was(capi, dec_factory, torch_cuda):
    """Mixing kinds both ways, a long-stream handle, formats that are not IQ, a pointer 2 bytes off, 2^31 samples: -1 with a
    message, and the stream that was in progress still finishes with its own frames."""
    L = capi.load()
    x, rec = load_iq("mixed_df_a")
    want = golden_records(rec)
    t, ptr = to_dev(torch_cuda, x)
    n, half = len(x), len(x) // 2
    d = dec_factory(df18=True, collect_stats=True)
    real = np.full(4096, 2048, np.uint16)
    tr, pr = to_dev(torch_cuda, real)

    def refused(call, *words):
        with pytest.raises(capi.AdsbError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    d.reset()
    d.push_iq(S16_IQ, x[:half])
    refused(lambda: d.push(real), "IQ", "real")                                    # a real push into an IQ stream
    refused(lambda: d.push_as(3, real.view(np.int16)), "IQ", "real")
    refused(lambda: d.push_device(pr, real.size), "IQ", "real")
    refused(lambda: d.push_packed(np.zeros(12, np.uint8)), "IQ", "real")
    for fmt in (1, 3, 4, 5, 7):
        refused(lambda: d.push_iq(fmt, (x.ctypes.data, 8)), f"format {fmt}", "IQ")
        refused(lambda: d.push_device_iq(fmt, ptr, 8), f"format {fmt}")
    refused(lambda: d.push_device_iq(S16_IQ, ptr + 2, 8), "4-byte aligned")
    refused(lambda: d.push_device_iq(F32_IQ, ptr + 2, 8), "4-byte aligned")
    refused(lambda: d.push_iq(S16_IQ, (x.ctypes.data, 1 << 31)), "2^31")
    refused(lambda: d.push_device_iq(S16_IQ, ptr, 1 << 31), "2^31")
    refused(lambda: d.push_iq(S16_IQ, (None, 8)), "NULL")
    d.push_device_iq(S16_IQ, ptr + 4 * half, n - half)
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    # decode_device_iq refuses before its reset: the finished stream's statistics are still there
    for call, word in ((lambda: d.decode_device_iq(S16_IQ, ptr + 2, n), "4-byte aligned"), (lambda: d.decode_device_iq(5, ptr, n), "format 5"),
                       (lambda: d.decode_device_iq(S16_IQ, ptr, 1 << 31), "2^31"),
                       (lambda: d.decode_batch_device_iq(S16_IQ, [ptr, ptr + 2], [n, n]), "capture 1"),
                       (lambda: d.decode_batch_device_iq(3, [ptr], [n]), "format 3")):
        refused(call, word)
        assert d.stats() == rec["stats"]
    # an IQ push into a real stream
    d.reset()
    d.push(real)
    refused(lambda: d.push_iq(S16_IQ, x[:half]), "real", "IQ")
    refused(lambda: d.push_device_iq(F32_IQ, ptr, 8), "real", "IQ")
    d.push(real)
    d.finish()
    assert d.drain() == []
    # the _as calls keep refusing the IQ numbers
    d.reset()
    for fmt in (0, 2):
        refused(lambda: d.push_as(fmt, (x.ctypes.data, 8)), "IQ", "raw twin")
    # a long-stream handle takes no IQ samples, and stays usable for real ones
    dl = dec_factory(df18=True)
    dl.set_long_stream(True)
    refused(lambda: dl.push_iq(S16_IQ, x[:half]), "long-stream", "IQ")
    refused(lambda: dl.decode_device_iq(S16_IQ, ptr, n), "long-stream")
    refused(lambda: dl.decode_batch_device_iq(S16_IQ, [ptr], [n]), "long-stream")
    dl.push(real)
    dl.finish()
    assert dl.drain() == []


# ------------------------------------------------------------------ 7. the 1-bit repair
@pytest.mark.limit(60)
def test_one_bit_repair(capi, dec_factory, torch_cuda):
    """cfg.fix_1bit: a DF17 frame with one payload bit flipped decodes to the original bytes, marked in `reserved` and counted in
    stats.fixed; with the knob off it does not decode."""
    from tools import gen_signal as G
    rng = np.random.default_rng(9)
    good, hit = G.make_frame(17, rng), bytearray(G.make_frame(17, rng))
    orig = bytes(hit)
    hit[5] ^= 0x10                                              # bit 43 of the frame: inside [5, 112)
    x = G.iq_synth(60_000, [(5000, good, 800.0, 0.4), (20_000, bytes(hit), 900.0, 2.1)], 2.0, 9)
    d_on, d_off = dec_factory(df18=True, fix_1bit=True), dec_factory(df18=True)
    for fmt in FMTS:
        src = as_fmt(fmt, x)
        d_on.reset()
        d_on.push_iq(fmt, src)
        d_on.finish()
        buf, k = d_on.drain_raw()
        got = [(bytes(f.frame[: f.len]), int(f.reserved) & 1) for f in buf[:k]]
        assert got == [(good, 0), (orig, 1)], fmt
        assert [abs(int(f.g) - at) <= 1 for f, at in zip(buf[:k], (5000, 20_000))] == [True, True]   # (a half-sample copy may come first)
        assert d_on.stats()["fixed"] == 1 and d_on.stats()["ok"][17] == 2
        assert [f["frame"] for f in d_off.decode_iq(fmt, src)] == [good], fmt


# ------------------------------------------------------------------ 8. the C host program
@pytest.mark.limit(120)
def test_cli_q(capi, tmp_path):
    """adsbdec_amd_cli -q 2 -a -m -f and -b through a loopback peer: the fixture's AVR-MLAT and Beast bytes and its Try/Ok table;
    -q 0 on the float twin prints the same packets."""
    from test_cli_sink import Listener
    x, rec = load_iq("mixed_df_a")
    path = tmp_path / "mixed.s16iq"
    x.tofile(path)
    mlat = "".join(f["mlat"] for f in rec["frames"]).encode()
    beast = b"".join(bytes.fromhex(f["beast"]) for f in rec["frames"])
    p = subprocess.run([capi.CLI_PATH, "-q", "2", "-a", "-m", "-f", str(path)], capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr
    assert p.stdout == mlat
    table = p.stderr.decode().splitlines()
    tr = [ln for ln in table if ln.startswith("Try")][0].split()[2:]
    ok = [ln for ln in table if ln.startswith("Ok")][0].split()[2:]
    assert [int(v) for v in tr] == [rec["stats"]["try"][k] for k in (11, 17, 18)]
    assert [int(v) for v in ok] == [rec["stats"]["ok"][k] for k in (11, 17, 18)]
    lis = Listener()
    p = subprocess.run([capi.CLI_PATH, "-q", "2", "-a", "-b", "-s", f"127.0.0.1:{lis.port}", "-f", str(path)], capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr
    assert lis.join() == beast
    fpath = tmp_path / "mixed.f32iq"
    S().to_float32_iq(x).tofile(fpath)
    p = subprocess.run([capi.CLI_PATH, "-q", "0", "-a", "-m", "-f", str(fpath)], capture_output=True, timeout=100)
    assert p.returncode == 0 and p.stdout == mlat, p.stderr
