"""Signed 16-bit real and float32 real input on the MI355X: the conversion kernel alone, every ingress of one handle that takes
a format (host pushes in the three modes, mixed streams, device pushes, batches), the golden fixtures, off-grid input and its
report, the refusals, and the C host program's -t.  The definition every conversion is held to is the numpy one
(adsbdec_amd/sample_formats.py); frames are those of the raw uint16 twin, bit for bit."""
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records

pytestmark = pytest.mark.gpu

F32, S16, U16, RAW = 1, 3, 4, 5
FMTS = [S16, F32]
ELEM = {S16: 2, F32: 4}


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


def to_dev(torch, a):
    """A numpy array of any dtype as bytes on the device (the tensor keeps the memory alive; its pointer is 256-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    assert t.data_ptr() % 256 == 0 or t.numel() == 0
    return t


# ------------------------------------------------------------------ the kernel alone
def _random_source(fmt, n, seed):
    """n samples of random bits -- off-grid values, NaN, Inf, denormals, huge values -- with the special values planted too."""
    rng = np.random.default_rng(seed)
    if fmt == S16:
        return rng.integers(0, 1 << 16, n, dtype=np.uint32).astype("<u2").view("<i2")
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    k = n // 4
    bits[:k] = (bits[:k] & 0x80FFFFFF) | 0x3F000000            # |x| in [0.5, 1): inside the grid's range, off the grid
    bits[k:2 * k] = S().to_float32_real(rng.integers(0, 4096, k, dtype=np.uint16)).view("<u4")     # on the grid
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x807FFFFF, 0x80000000, 0x3F800000, 0xBF800000,
                        0x3A000000, 0x39800000], dtype="<u4")  # +-Inf, NaN, denormals, -0.0, +-1.0, 2^-11 (grid), 2^-12 (a tie)
    if n:
        at = rng.integers(0, n, min(n, 64))
        bits[at] = special[rng.integers(0, special.size, at.size)]
    rng.shuffle(bits)
    return bits.view("<f4")


KERNEL_N = [0, 1, 7, 8, 9, 15, 63, 64, 65, 511, 513, 2048 * 8 + 3, (1 << 20) + 5]   # the last: more groups than lanes (grid stride)


@pytest.mark.limit(120)
@pytest.mark.parametrize("n", KERNEL_N)
@pytest.mark.parametrize("fmt", FMTS)
def test_convert_kernel_alone(capi, torch_cuda, fmt, n):
    """adsb_convert_samples == the numpy definition for dst at 0..7 samples past a 16-byte boundary and src 0, 1 and 3 elements
    past an aligned base; 64 canary samples either side of dst stay; the two counters grow by numpy's counts, and a second call
    without counters writes the same samples and leaves them alone."""
    torch = torch_cuda
    L = capi.load()
    src_h = _random_source(fmt, n + 3, 1000 * fmt + n % 997)
    if fmt == S16:
        codes, inexact = S().flags_int16_real(src_h)
        clamped = np.zeros(n + 3, bool)
    else:
        codes, inexact, clamped = S().flags_float32_real(src_h)
    if n >= 511 and fmt == F32:
        assert inexact.any() and clamped.any() and (~inexact & ~clamped).any()
    src = to_dev(torch, src_h)
    for soff in (0, 1, 3):
        want = codes[soff:soff + n]
        wi, wc = int(inexact[soff:soff + n].sum()), int(clamped[soff:soff + n].sum())
        for doff in range(8):
            dst = torch.full((64 + doff + n + 64 + 8,), 0x7777, dtype=torch.int16, device="cuda")
            assert dst.data_ptr() % 16 == 0
            counters = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
            p_dst, p_src = dst.data_ptr() + 2 * (64 + doff), src.data_ptr() + ELEM[fmt] * soff
            assert L.adsb_convert_samples(p_dst, p_src, fmt, n, counters.data_ptr(), None) == 0, L.adsb_last_error(None)
            torch.cuda.synchronize()
            got = dst.cpu().numpy().view(np.uint16)
            what = (fmt, n, soff, doff)
            assert np.array_equal(got[64 + doff: 64 + doff + n], want), what
            assert (got[:64 + doff] == 0x7777).all() and (got[64 + doff + n:] == 0x7777).all(), what
            assert counters.cpu().tolist() == [5 + wi, 7 + wc], what
            if doff in (0, 3):                              # again, without counters
                dst.fill_(0x7777)
                assert L.adsb_convert_samples(p_dst, p_src, fmt, n, None, None) == 0
                torch.cuda.synchronize()
                assert np.array_equal(dst.cpu().numpy().view(np.uint16), got), what
                assert counters.cpu().tolist() == [5 + wi, 7 + wc], what


@pytest.mark.limit(60)
def test_convert_kernel_refusals_write_nothing(capi, torch_cuda):
    torch = torch_cuda
    L = capi.load()
    src = to_dev(torch, _random_source(F32, 1024, 3))
    dst = torch.zeros(4096, dtype=torch.int16, device="cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    for fmt, args, word in ((S16, (dst.data_ptr(), src.data_ptr() + 1), b"aligned"), (F32, (dst.data_ptr(), src.data_ptr() + 2), b"aligned"),
                            (S16, (dst.data_ptr() + 1, src.data_ptr()), b"aligned"), (U16, (dst.data_ptr(), src.data_ptr()), b"format 4"),
                            (0, (dst.data_ptr(), src.data_ptr()), b"format 0"), (7, (dst.data_ptr(), src.data_ptr()), b"format 7"),
                            (S16, (None, src.data_ptr()), b"NULL")):
        assert L.adsb_convert_samples(args[0], args[1], fmt, 512, counters.data_ptr(), None) == -1, (fmt, args)
        msg = L.adsb_last_error(None)
        assert b"adsb_convert_samples" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0).all() and counters.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------ golden twins
def _has_twin(x):
    return x.size == 0 or int(x.max()) <= 4095


def test_seven_of_the_eight_fixtures_have_twins():
    names = golden_cases()
    twins = [n for n in names if _has_twin(load_golden(n)[0])]
    assert len(names) == 8 and len(twins) == 7 and set(names) - set(twins) == {"wide_codes_noise"}


@pytest.mark.limit(120)
@pytest.mark.parametrize("name", golden_cases())
def test_golden_twins(capi, dec_factory, torch_cuda, name):
    """Every committed fixture whose codes fit 12 bits, converted to both formats: decode_device_as equals decode_device of the
    raw capture and the fixture's records (g, ts, pw, bytes) and Try/Ok table; nothing is off the grid."""
    x, rec = load_golden(name)
    if not _has_twin(x):                                       # codes up to 29 999: no value in either format
        for fmt in FMTS:
            with pytest.raises(ValueError, match="4095"):
                S().to_format(fmt, x)
        return
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    raw = to_dev(torch_cuda, x)
    want = records(capi._frames_to_dicts(*d.decode_device_raw(raw.data_ptr(), x.size)))
    assert want == golden_records(rec)
    assert d.format_report() == (0, 0, 0)
    for fmt in FMTS:
        t = to_dev(torch_cuda, S().to_format(fmt, x))
        assert records(d.decode_device_as(fmt, t.data_ptr(), x.size)) == want, fmt
        assert d.stats() == rec["stats"], fmt
        assert d.format_report() == (x.size, 0, 0), fmt
    for fmt in (U16, RAW):                                     # the pass-through formats: the uint16 call itself
        assert records(d.decode_device_as(fmt, raw.data_ptr(), x.size)) == want, fmt
        assert d.format_report() == (0, 0, 0), fmt


# ------------------------------------------------------------------ streams
N_STREAM = (1 << 20) + 37
_stream = {}


def _stream_capture(oracle):
    """One sparse capture of ~1 Mi samples and what the oracle decodes from it and from its 96 Ki prefix."""
    if not _stream:
        from tools import gen_signal as G
        x, _ = G.sparse_capture(N_STREAM, n_frames=180, seed=1811, sigma=8.0, dfs=(17, 18, 11))
        assert x.max() <= 4095
        _stream["x"] = x
        for n in (96 << 10, N_STREAM):
            _stream[n] = oracle.decode(x[:n], df18=True)
        assert len(_stream[N_STREAM][0]) > 100 and len(_stream[96 << 10][0]) > 3
    return _stream


# (chunk in samples, prefix of the capture): pushes of 4 samples run on the 96 Ki prefix (the reference hands out no frame
# before sample 81 960, air.c:94) -- 24 Ki pushes; a quarter of a million of them on the whole capture would take a minute
# per mode and show nothing else
STREAM_PATHS = [(4, 96 << 10), (1000, N_STREAM), (4099, N_STREAM), (65536, N_STREAM)]


@pytest.mark.limit(300)
@pytest.mark.parametrize("mode", ["sync", "async", "overlap"])
@pytest.mark.parametrize("fmt", FMTS)
def test_host_pushes_equal_the_one_shot_decode(capi, oracle, dec_factory, torch_cuda, fmt, mode):
    """push_as in chunks of 4, 1 000, 4 099 (odd: every destination alignment) and 65 536 samples, with the default staging
    buffer and one of 64 Ki samples (every piece compacts): frames and Try/Ok equal the oracle's on the raw twin, which is what
    the one-shot decode_device_as gives."""
    cap = _stream_capture(oracle)
    for chunk, n in STREAM_PATHS:
        x = cap["x"][:n]
        want, wstats = cap[n]
        xf = S().to_format(fmt, x)
        for stage in (0, 64 << 10):
            d = dec_factory(df18=True, collect_stats=True, stage_samples=stage, push_overlap=(mode == "overlap"))
            what = f"fmt={fmt} chunk={chunk} n={n} stage={stage} mode={mode}"
            t = to_dev(torch_cuda, xf)
            one_shot = records(d.decode_device_as(fmt, t.data_ptr(), n))
            assert one_shot == records(want), what
            got = d.decode_as(fmt, xf, chunk=chunk, mode=mode)
            assert records(got) == one_shot, what
            assert d.stats() == wstats, what
            assert d.format_report() == (n, 0, 0), what
            d.close()


@pytest.mark.limit(120)
@pytest.mark.parametrize("asynchronous", [False, True])
def test_a_stream_that_switches_formats(capi, oracle, dec_factory, asynchronous):
    """uint16, int16, float32 and packed pushes (the packed ones at multiples of 8) in one stream decode like the whole capture."""
    from adsbdec_amd.packed12 import pack12
    cap = _stream_capture(oracle)
    x = cap["x"]
    want, wstats = cap[N_STREAM]
    cuts = [0, 1001, 70_002, 70_005, 8 * 20_000, 8 * 30_000, 8 * 30_000 + 13, 500_001, 8 * 80_000, 8 * 90_001, 900_000, x.size]
    kinds = ["u16", "s16", "f32", "s16", "p12", "f32", "u16", "s16", "p12", "f32", "s16"]
    assert cuts == sorted(cuts) and len(kinds) == len(cuts) - 1
    d = dec_factory(df18=True, collect_stats=True)
    m = "async" if asynchronous else "sync"
    keep, out, converted = [], [], 0
    d.reset()
    for k, kind in enumerate(kinds):
        piece = np.ascontiguousarray(x[cuts[k]:cuts[k + 1]])
        if kind == "p12":
            assert cuts[k] % 8 == 0 and piece.size % 8 == 0
            piece = pack12(piece)
            (d.push_packed_async if asynchronous else d.push_packed)(piece)
        elif kind == "u16":
            d.push_as(RAW if k else U16, piece, m)
        else:
            fmt = S16 if kind == "s16" else F32
            converted += piece.size
            piece = S().to_format(fmt, piece)
            d.push_as(fmt, piece, m)
        keep.append(piece)                                  # (async: the pieces stay borrowed until the next call)
        out += d.drain()
    d.finish()
    out += d.drain()
    assert records(out) == records(want)
    assert d.stats() == wstats
    assert d.format_report() == (converted, 0, 0)


@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
def test_device_pushes_in_pieces(capi, oracle, dec_factory, torch_cuda, fmt):
    """push_device_as in unequal pieces -- small ones that are staged, one at a multiple of 8 that is scanned in place, odd
    ones -- ending with _final, equals the one-shot decode."""
    cap = _stream_capture(oracle)
    x = cap["x"]
    want, wstats = cap[N_STREAM]
    t = to_dev(torch_cuda, S().to_format(fmt, x))
    d = dec_factory(df18=True, collect_stats=True)
    cuts = [0, 5600, 5600 + 300_008, 700_003, 700_004, x.size]
    d.reset()
    for k in range(len(cuts) - 1):
        a, b = cuts[k], cuts[k + 1]
        d.push_device_as(fmt, t.data_ptr() + ELEM[fmt] * a, b - a, final=(k == len(cuts) - 2))
    assert records(d.drain()) == records(want)
    assert d.stats() == wstats
    assert d.format_report() == (x.size, 0, 0)
    # a stream that ends with an empty final push
    d.reset()
    d.push_device_as(fmt, t.data_ptr(), x.size)
    d.push_device_as(fmt, None, 0, final=True)
    assert records(d.drain()) == records(want)


# ------------------------------------------------------------------ batches
BATCH_N = [0, 2000, 70_001, 131_072, 33_333, 262_144]     # empty, below one window (< 2 392 samples), two odd lengths


def _batch_captures(x):
    out, at = [], 0
    for n in BATCH_N:
        out.append(np.ascontiguousarray(x[at:at + n]))
        at += n
    assert at <= x.size
    return out


@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
def test_batches_equal_the_single_decodes(capi, oracle, dec_factory, torch_cuda, fmt):
    """Six captures in one conversion launch and the batch scan: frames and per-capture Try/Ok equal decode_device_as of each
    capture alone (which equals the oracle on its raw twin), from device and from host memory."""
    caps = _batch_captures(_stream_capture(oracle)["x"])
    conv = [S().to_format(fmt, c) for c in caps]
    dev = [to_dev(torch_cuda, c) for c in conv]
    d = dec_factory(df18=True, collect_stats=True)
    single, sstats = [], []
    for c, t in zip(caps, dev):
        single.append(records(d.decode_device_as(fmt, t.data_ptr() if c.size else None, c.size)))
        sstats.append(d.stats())
        if c.size:
            want, wstats = oracle.decode(c, df18=True)
            assert single[-1] == records(want) and sstats[-1] == wstats
    assert sum(len(s) for s in single) > 40 and single[0] == [] and single[1] == []
    frames, stats = d.decode_batch_device_as(fmt, [t.data_ptr() if t.numel() else None for t in dev], BATCH_N, stats=True)
    assert [records(f) for f in frames] == single and stats == sstats
    assert d.format_report() == (sum(BATCH_N), 0, 0)
    frames, stats = d.decode_batch_as(fmt, conv, stats=True)
    assert [records(f) for f in frames] == single and stats == sstats
    assert d.format_report() == (sum(BATCH_N), 0, 0)
    # the pass-through formats: the uint16 batch call
    raw = [to_dev(torch_cuda, c) for c in caps]
    frames = d.decode_batch_device_as(RAW, [t.data_ptr() if t.numel() else None for t in raw], BATCH_N)
    assert [records(f) for f in frames] == single and d.format_report() == (0, 0, 0)


def _off_grid(fmt, x, seed):
    """The capture x in format fmt with samples pushed off the grid: (samples, codes numpy decodes, inexact, clamped)."""
    rng = np.random.default_rng(seed)
    if fmt == S16:
        y = (S().to_int16_real(x).astype(np.int32) + rng.integers(0, 16, x.size)).astype("<i2")   # random low nibbles: the same codes
    else:
        y = S().to_float32_real(x).copy()
        bad = rng.random(x.size) < 0.01
        y[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1.0, 1.5, -1.25, 3e38, -7.0], "<f4"), int(bad.sum()))
        off = (rng.random(x.size) < 0.01) & ~bad
        y[off] += rng.uniform(-2e-4, 2e-4, int(off.sum())).astype("<f4")                    # up to 0.4 of a grid step
        y[rng.integers(0, x.size, 50)] = np.array([1e-40], "<f4")[0]                            # denormals
    codes, inexact, clamped = S().from_format(fmt, y)
    return y, codes, inexact, clamped


@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
def test_off_grid_input_and_its_report(capi, oracle, dec_factory, torch_cuda, fmt):
    """int16 with random low nibbles, float32 with 1 % NaN / +-Inf / |x| > 1 and 1 % values off the grid: the frames are those of
    the codes the numpy definition gives, and the report equals numpy's counts exactly -- one shot, pushed from the host, and
    summed over a batch."""
    x = _stream_capture(oracle)["x"]
    y, codes, inexact, clamped = _off_grid(fmt, x, 77 + fmt)
    assert inexact > 5000 and (fmt == S16 or clamped > 5000)
    if fmt == S16:
        assert np.array_equal(codes, x) and clamped == 0
    d = dec_factory(df18=True, collect_stats=True)
    raw = to_dev(torch_cuda, codes)
    want = records(capi._frames_to_dicts(*d.decode_device_raw(raw.data_ptr(), codes.size)))
    wstats = d.stats()
    assert len(want) > 50
    t = to_dev(torch_cuda, y)
    assert records(d.decode_device_as(fmt, t.data_ptr(), y.size)) == want
    assert d.stats() == wstats
    assert d.format_report() == (y.size, inexact, clamped)
    assert records(d.decode_as(fmt, y, chunk=100_003, mode="async")) == want
    assert d.format_report() == (y.size, inexact, clamped)
    d.reset()
    assert d.format_report() == (0, 0, 0)                      # since adsb_reset
    caps = _batch_captures(y)
    ccodes = _batch_captures(codes)
    per = [S().from_format(fmt, c) for c in caps]
    for c, (k, _, _) in zip(ccodes, per):
        assert np.array_equal(c, k)
    frames = d.decode_batch_as(fmt, caps)
    assert [records(f) for f in frames] == [records(f) for f in d.decode_batch(ccodes)]
    d.decode_batch_as(fmt, caps)
    assert d.format_report() == (sum(BATCH_N), sum(p[1] for p in per), sum(p[2] for p in per))


# ------------------------------------------------------------------ refusals
@pytest.mark.limit(120)
@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_leave_the_handle_as_it_was(capi, oracle, dec_factory, torch_cuda, fmt):
    """A bad fmt (0, 2: IQ has no raw twin; 7), a device pointer off by half an element, NULL with n > 0 -- through every _as
    call, in batches by capture index: -1 with a message that names the call, and the stream that was pending goes on and ends
    with the right frames."""
    cap = _stream_capture(oracle)
    x = cap["x"]
    want, wstats = cap[N_STREAM]
    y = S().to_format(fmt, x)
    t = to_dev(torch_cuda, y)
    half = ELEM[fmt] // 2
    d = dec_factory(df18=True, collect_stats=True)
    d.reset()
    cut = 400_003
    d.push_as(fmt, y[:cut])
    out = d.drain()
    E = capi.AdsbError
    for bad, why in ((0, "IQ"), (2, "IQ"), (7, "unknown sample format 7")):
        with pytest.raises(E, match=f"adsb_push_as.*{why}"):
            d.push_as(bad, y[cut:])
        with pytest.raises(E, match=f"adsb_push_async_as.*{why}"):
            d.push_as(bad, (y.ctypes.data, 100), "async")
        with pytest.raises(E, match=f"adsb_push_device_as.*{why}"):
            d.push_device_as(bad, t.data_ptr(), 1000)
        with pytest.raises(E, match=f"adsb_push_device_final_as.*{why}"):
            d.push_device_as(bad, t.data_ptr(), 1000, final=True)
        with pytest.raises(E, match=f"adsb_decode_device_as.*{why}"):
            d.decode_device_as(bad, t.data_ptr(), 1000)
        with pytest.raises(E, match=f"adsb_decode_batch_device_as.*{why}"):
            d.decode_batch_device_as(bad, [t.data_ptr()], [1000])
        with pytest.raises(E, match=f"adsb_decode_batch_host_as.*{why}"):
            d.decode_batch_as(bad, [y[:1000]])
    with pytest.raises(E, match="adsb_push_as.*raw twin"):
        d.push_as(0, y[cut:])
    with pytest.raises(E, match=f"adsb_push_device_as: device pointer .* is not {ELEM[fmt]}-byte aligned"):
        d.push_device_as(fmt, t.data_ptr() + half, 1000)
    with pytest.raises(E, match=f"adsb_push_device_final_as: device pointer .* is not {ELEM[fmt]}-byte aligned"):
        d.push_device_as(fmt, t.data_ptr() + half, 1000, final=True)
    with pytest.raises(E, match=f"adsb_decode_device_as: device pointer .* is not {ELEM[fmt]}-byte aligned"):
        d.decode_device_as(fmt, t.data_ptr() + half, 1000)
    with pytest.raises(E, match="adsb_decode_batch_device_as: capture 2: device pointer"):
        d.decode_batch_device_as(fmt, [t.data_ptr(), None, t.data_ptr() + 4096 + half], [1000, 0, 1000])
    with pytest.raises(E, match="adsb_push_device_as: NULL samples"):
        d.push_device_as(fmt, None, 1000)
    with pytest.raises(E, match="adsb_decode_device_as: NULL samples"):
        d.decode_device_as(fmt, None, 1000)
    with pytest.raises(E, match="adsb_push_as: NULL samples"):
        d.push_as(fmt, (None, 1000))
    with pytest.raises(E, match="adsb_decode_batch_device_as: capture 1: NULL samples"):
        d.decode_batch_device_as(fmt, [t.data_ptr(), None], [1000, 1000])
    with pytest.raises(E, match="adsb_decode_batch_host_as: capture 1: NULL samples"):
        import ctypes as C                                     # (the wrapper of the host flavour takes arrays: the raw call)
        L = capi.load()
        p = (C.c_void_p * 2)(y.ctypes.data, None)
        n = (C.c_size_t * 2)(1000, 1000)
        first = (C.c_uint64 * 3)()
        if L.adsb_decode_batch_host_as(d._h, fmt, 2, p, n, d._out_ref, first, None) < 0:
            d._check(-1, "adsb_decode_batch_host_as")
    with pytest.raises(E, match=r"adsb_decode_batch_device_as: capture 0 has .* samples: 2\^32 or more"):
        d.decode_batch_device_as(fmt, [t.data_ptr()], [1 << 32])
    with pytest.raises(E, match=r"2\^32 samples"):
        d.push_device_as(fmt, t.data_ptr(), (1 << 32) - 5)     # the stream would reach 2^32 samples (it is not a long stream)
    with pytest.raises(E, match=r"2\^32 samples"):
        d.decode_device_as(fmt, t.data_ptr(), 1 << 32)
    # the pending stream goes on
    assert d.format_report() == (cut, 0, 0)
    d.push_as(fmt, y[cut:])
    d.finish()
    out += d.drain()
    assert records(out) == records(want)
    assert d.stats() == wstats
    assert d.format_report() == (x.size, 0, 0)


# ------------------------------------------------------------------ the C host program
@pytest.mark.limit(300)
def test_cli_type_flag_equals_the_raw_file(capi, oracle, tmp_path):
    """-t 3 on the int16 file and -t 1 on the float32 file write the stdout bytes and the stderr of the run on the raw file, in
    the three output formats; -t 4 and -t 5 are that run; a trailing partial sample is dropped with a line on stderr; a raw file
    read as int16 ends with the line that asks whether -t is right."""
    cap = _stream_capture(oracle)
    x = cap["x"]
    want, wstats = cap[N_STREAM]
    paths = {U16: str(tmp_path / "x.u16"), S16: str(tmp_path / "x.s16"), F32: str(tmp_path / "x.f32")}
    x.tofile(paths[U16])
    for fmt in FMTS:
        S().to_format(fmt, x).tofile(paths[fmt])
    run = lambda *a: subprocess.run([capi.CLI_PATH, *a], capture_output=True, timeout=120)
    for flags in (["-a", "-m"], ["-a", "-b"], ["-a"]):
        base = run(*flags, "-f", paths[U16])
        assert base.returncode == 0 and len(base.stdout) > 16 * len(want), base.stderr
        if flags == ["-a", "-m"]:
            assert base.stdout == b"".join(capi.format_frame(f, 1) for f in want)
        for fmt in FMTS:
            r = run(*flags, "-t", str(fmt), "-f", paths[fmt])
            assert r.returncode == 0, r.stderr
            assert r.stdout == base.stdout, (flags, fmt)
            assert r.stderr == base.stderr, (flags, fmt)              # the Try/Ok table, and nothing else
        for fmt in (U16, RAW):
            r = run(*flags, "-t", str(fmt), "-f", paths[U16])
            assert (r.returncode, r.stdout, r.stderr) == (0, base.stdout, base.stderr), (flags, fmt)
    assert b"Try :" in base.stderr
    # a trailing partial element
    cut = str(tmp_path / "cut.f32")
    with open(cut, "wb") as f:
        f.write(S().to_float32_real(x).tobytes() + b"\x01\x02\x03")
    r = run("-a", "-t", "1", "-f", cut)
    assert r.returncode == 0 and r.stdout == base.stdout and b"3 trailing bytes ignored" in r.stderr
    # the wrong type: a raw file read as int16
    r = run("-a", "-t", "3", "-f", paths[U16])
    _, inexact, clamped = S().from_int16_real(x.view("<i2"))
    assert r.returncode == 0
    assert f"{inexact} of {x.size} samples are not INT16_REAL values (0 clamped): is -t right?\n".encode() in r.stderr
