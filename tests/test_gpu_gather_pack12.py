"""The 12-bit burst gather on the MI355X (run with -m gpu): adsb_gather_pack12_device, _as and _packed against the numpy statement
(adsbdec_amd/burst_archive.py gather12) for equality, byte for byte.  The output array is filled with poison first and compared
WHOLE: the bytes of the pieces, the zero pad between them, and the poison at and behind `total`.  The capture lies between two
stretches of code 4095: a lane that reads past a piece's end where the fill belongs, or past the capture's, packs 0xfff where 0x800
belongs.

Shapes (tests/gather_pack12_cases.py names them): every one at M % 28 in {2, 14, 26} -- 28 is a multiple of 4, so these all have
M % 4 == 2 and end in a half group -- and, for M % 4 == 0, at M % 28 in {0, 4, 16, 24}.  Then seeded random tables, codes above 4095,
the converted and packed flavours, every refusal, the call between two pushes of a stream, the pipeline (level -> gate -> gather ->
decode where the pieces lie, on a flush handle, against the uint16 gather's pieces and against the oracle) and the host program's -P."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import flush_cases as FC
import gather_cases as GC
import gather_pack12_cases as PC

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
    """A uint16 capture between its guards of code 4095 in HBM, and a poisoned output array."""

    def __init__(self, torch, x):
        self.torch, self.x = torch, x
        both, lead = PC.guarded(x)
        self.t, base = to_dev(torch, both)
        self.ptr = base + 2 * lead
        assert self.ptr % 16 == 0
        self.out = None

    def gather(self, d, tab, n=None, call=None, slack=TAIL):
        """One call, held to the statement: -> (the output's bytes, offsets, over)."""
        n = self.x.size if n is None else n
        M = 2 * (n // 4)
        want, woff, wover = BA().gather12(self.x, tab, M)
        room = want.size + slack
        if self.out is None or self.out.numel() < room:
            self.out = self.torch.empty(max(room, 1 << 16), dtype=self.torch.uint8, device="cuda")
        self.out.fill_(POISON)
        off, over = (call or (lambda *a: d.gather_pack12_device(self.ptr, *a)))(n, tab, self.out.data_ptr(), want.size)
        got = self.out[:room].cpu().numpy()
        assert np.array_equal(off, woff), (M, tab.size)
        assert np.array_equal(got[:want.size], want), (M, tab.size, int(np.flatnonzero(got[:want.size] != want)[0]))
        assert (got[want.size:] == POISON).all(), (M, tab.size)
        assert over == wover, (M, tab.size, over, wover)
        return got[:want.size], off, over


# ------------------------------------------------------------------ 1: the shapes aimed at the kernel
@pytest.mark.limit(60)
@pytest.mark.parametrize("M", PC.m_values())
def test_named_shapes(capi, dec_factory, torch_cuda, M):
    d = dec_factory()
    Cw = capi.gather_chunk_words()
    cases = PC.named_cases(Cw, M)
    for tail in (0, 3):                                      # n % 4: samples behind the last power sample belong to no piece
        dev = Device(torch_cuda, PC.codes(PC.n_for(M, tail), 21 + tail))
        for name, M_, tab in cases:
            out, off, over = dev.gather(d, tab)
            if tab.size == 0:                                # no burst: 0, nothing launched, nothing written
                assert off.tolist() == [0] and out.size == 0
    # the shapes are what they are meant to be
    by_name = {name: tab for name, _, tab in cases}
    assert len(by_name) == len(cases) == 11
    tab = by_name["every second run a piece, over 3 C + 5 words"]
    assert int(BA().layout12(tab, M)[-1]) // 16 >= 3 * Cw + 5 and tab.size > 3 * Cw // 6
    long_ones = [tab for name, tab in by_name.items() if "3 C + 1" in name]
    assert len(long_ones) == 2
    for tab in long_ones:
        off = BA().layout12(tab, M)
        assert int(off[2] - off[1]) // 16 >= 3 * Cw + 1 and int(off[1]) == 96 and int(off[3] - off[2]) == 96
    lens = {int(e - b) for b, e in zip(by_name["pieces of 1, 2, 3 and 4 runs"]["begin"], by_name["pieces of 1, 2, 3 and 4 runs"]["end"])}
    assert lens == {1, 2, 3, 4}
    last = LV().burst_samples(by_name["only a clipped last run"], M)[0]
    assert int(last[1]) == M and (2 * int(last[1] - last[0])) % 8 == (4 if M % 4 == 2 else 0)


# ------------------------------------------------------------------ 2: seeded random tables
@pytest.mark.limit(120)
def test_random_tables(dec_factory, torch_cuda):
    d = dec_factory()
    tables = PC.random_tables(300, 5012)
    x = PC.codes(2 * max(M for M, _ in tables) + 3, 22)
    dev = Device(torch_cuda, x)
    seen = set()
    for i, (M, tab) in enumerate(tables):
        dev.gather(d, tab, n=2 * M + i % 4)
        seen.add((M % 28, M % 4))
    assert len(seen) == 14                                   # every even remainder mod 28 (M % 4 follows from it)


# ------------------------------------------------------------------ 3: codes above 4095
@pytest.mark.limit(60)
def test_codes_above_4095_are_counted_once_and_stored_by_their_low_bits(dec_factory, torch_cuda):
    d = dec_factory()
    M = 28 * 400 + 14
    x = PC.codes(PC.n_for(M, 3), 23)
    loud = x.copy()
    loud[::37] |= 0x1000                                     # inside and outside the pieces, the trailing samples among them
    loud[5::101] |= 0xF000
    total_over = 0
    for name, M_, tab in PC.named_cases(256, M):
        out, off, over = Device(torch_cuda, loud).gather(d, tab)
        clean, _, zero = BA().gather12(x, tab, M)
        assert zero == 0 and np.array_equal(out, clean), name                 # the low 12 bits are what is stored
        sl = LV().burst_samples(tab, M)
        assert over == sum(int(np.count_nonzero(loud[2 * lo:2 * hi] > 4095)) for lo, hi in sl), name
        total_over += over
    assert total_over > 1000
    # every sample above 4095: a dense count, one atomic per lane that has any
    every = (x | 0x1000).astype(np.uint16)
    out, off, over = Device(torch_cuda, every).gather(d, GC.table([(0, 401)]))
    assert over == 2 * M
    # *over may be NULL
    dev = Device(torch_cuda, loud)
    tab = GC.table([(1, 3), (5, 8)])
    want, woff, _ = BA().gather12(loud, tab, M)
    o = torch_cuda.full((want.size + 64,), POISON, dtype=torch_cuda.uint8, device="cuda")
    assert d._L.adsb_gather_pack12_device(d._h, dev.ptr, loud.size, tab.ctypes.data, tab.size, o.data_ptr(), want.size, None, None) == want.size
    got = o.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == POISON).all()


# ------------------------------------------------------------------ 4: the converted and the packed flavours
@pytest.mark.limit(60)
def test_as_and_packed_equal_the_statement_on_the_converted_twin(dec_factory, torch_cuda):
    from adsbdec_amd import packed12, sample_formats
    d = dec_factory()
    for M in (28 * 400 + 14, 28 * 400 + 16):
        cases = PC.named_cases(256, M)
        for tail in (0, 3):
            x = PC.codes(PC.n_for(M, tail), 24 + tail)
            dev = Device(torch_cuda, x)
            for fmt in (3, 1):
                twin = sample_formats.to_format(fmt, x)
                codes, inexact, clamped = sample_formats.from_format(fmt, twin)
                assert np.array_equal(codes, x) and inexact == clamped == 0
                t, ptr = to_dev(torch_cuda, twin)
                d.reset()
                calls = 0
                for name, M_, tab in cases:
                    dev.gather(d, tab, call=lambda *a: d.gather_pack12_device_as(fmt, ptr, *a))
                    calls += tab.size > 0
                assert d.format_report() == (calls * x.size, 0, 0)      # rule 6: every call that converts adds its samples
        # packed: whole groups of 8 samples
        n = PC.n_for(M, 0) // 8 * 8
        x = PC.codes(n, 26)
        dev = Device(torch_cuda, x)
        t, ptr = to_dev(torch_cuda, packed12.pack12(x))
        d.reset()
        for name, M_, tab in PC.named_cases(256, 2 * (n // 4)):
            dev.gather(d, tab, call=lambda *a: d.gather_pack12_device_packed(ptr, *a))
        assert d.format_report() == (0, 0, 0)                           # an unpack counts nothing
    # an inexact int16 sample is converted as the decode calls convert it, and the report says so
    x = PC.codes(PC.n_for(28 * 40, 0), 27)
    twin = sample_formats.to_format(3, x)
    twin[100] += 5
    codes, inexact, clamped = sample_formats.from_format(3, twin)
    t, ptr = to_dev(torch_cuda, twin)
    d.reset()
    Device(torch_cuda, codes).gather(d, GC.table([(0, 40)]), call=lambda *a: d.gather_pack12_device_as(3, ptr, *a))
    assert d.format_report() == (x.size, 1, 0) and inexact == 1


# ------------------------------------------------------------------ 5: refusals, and the call between two pushes
@pytest.mark.limit(60)
def test_refusals_leave_the_poison(capi, dec_factory, torch_cuda):
    from adsbdec_amd import packed12, sample_formats
    d = dec_factory()
    L, h = d._L, d._h
    err = lambda: L.adsb_last_error(h).decode()
    M = 28 * 20
    x = PC.codes(2 * M, 28)
    t, ptr = to_dev(torch_cuda, x)
    t3, ptr3 = to_dev(torch_cuda, sample_formats.to_format(3, x))
    tp, ptrp = to_dev(torch_cuda, packed12.pack12(x))
    out = torch_cuda.full((1 << 16,), POISON, dtype=torch_cuda.uint8, device="cuda")
    ok = GC.table([(1, 3), (5, 8), (10, 12)])
    total = int(BA().layout12(ok, M)[-1])
    d.reset()

    def call(flavour="device", cap_ptr=None, n=x.size, tab=ok, out_ptr=out.data_ptr(), out_cap=1 << 16, fmt=3):
        off = np.full(tab.size + 1, 0x5A5A5A5A, np.uint64)
        over = C.c_uint64(0x5A)
        args = (n, tab.ctypes.data if tab.size else None, tab.size, out_ptr or None, out_cap, off.ctypes.data, C.byref(over))
        if flavour == "device":
            rc = L.adsb_gather_pack12_device(h, (ptr if cap_ptr is None else cap_ptr) or None, *args)
        elif flavour == "as":
            rc = L.adsb_gather_pack12_device_as(h, fmt, (ptr3 if cap_ptr is None else cap_ptr) or None, *args)
        else:
            rc = L.adsb_gather_pack12_device_packed(h, (ptrp if cap_ptr is None else cap_ptr) or None, *args)
        return rc, off, over.value

    def refused(word, **kw):
        rc, off, over = call(**kw)
        assert rc == -1 and word in err(), (word, kw, rc, err())
        assert (off == 0x5A5A5A5A).all() and over == 0x5A
        assert bool((out == POISON).all()), word
        assert d.format_report() == (0, 0, 0), word                     # nothing counted

    for flavour, p0 in (("device", ptr), ("as", ptr3), ("packed", ptrp)):
        for name, M_, tab, word in PC.refusals(M):
            refused(word, flavour=flavour, n=(2 * M_ + 7) // 8 * 8 if flavour == "packed" else 2 * M_, tab=tab)   # (20 -> 24: m = 12, as far outside)
        refused("2^32", flavour=flavour, n=1 << 32)
        refused("aligned", flavour=flavour, cap_ptr=p0 + (2 if flavour == "packed" else 8))
        refused("16-byte aligned", flavour=flavour, out_ptr=out.data_ptr() + 4)
        refused("NULL capture", flavour=flavour, cap_ptr=0)
        refused("NULL output", flavour=flavour, out_ptr=0)
        refused("burst 2", flavour=flavour, out_cap=total - 16)
        refused("burst 0", flavour=flavour, out_cap=0)
        refused("burst 1", flavour=flavour, out_cap=int(BA().layout12(ok, M)[1]))
        assert "adsb_gather_pack12_device" in err()
    for fmt in (0, 2, 4, 5, 8, 16, -1):
        refused(f"format {fmt}", flavour="as", fmt=fmt)
    refused("multiple of 8", flavour="packed", n=x.size - 4)
    # _packed takes a pointer that is 4-byte and not 16-byte aligned
    tq = torch_cuda.zeros((tp.numel() + 16,), dtype=torch_cuda.uint8, device="cuda")
    tq[4:4 + tp.numel()] = tp
    rc, off, over = call(flavour="packed", cap_ptr=tq.data_ptr() + 4, out_cap=total)
    assert rc == total and over == 0 and np.array_equal(out.cpu().numpy()[:total], BA().gather12(x, ok, M)[0])
    out.fill_(POISON)
    # no burst: 0, with NULL pointers too; then the call that works, offsets and over optional
    empty = GC.table([])
    assert L.adsb_gather_pack12_device(h, None, 0, None, 0, None, 0, None, None) == 0
    for flavour in ("device", "as", "packed"):
        rc, off, over = call(flavour=flavour, tab=empty)
        assert rc == 0 and off.tolist() == [0] and over == 0 and bool((out == POISON).all())
    assert d.format_report() == (0, 0, 0)
    assert L.adsb_gather_pack12_device(h, ptr, x.size, ok.ctypes.data, ok.size, out.data_ptr(), total, None, None) == total
    got = out.cpu().numpy()
    assert np.array_equal(got[:total], BA().gather12(x, ok, M)[0]) and (got[total:] == POISON).all()


@pytest.mark.limit(60)
def test_between_two_pushes_of_a_stream(capi, dec_factory, torch_cuda):
    from adsbdec_amd import packed12
    x = FC.real_capture(400_000, 77, extra=tuple((s, (17, 11)[k % 2]) for k, s in enumerate(range(500, 150_000, 9_000))))
    d = dec_factory(df18=True, collect_stats=True)
    want = d.decode(x)
    want_stats = d.stats()
    assert len(want) >= 10
    t, ptr = to_dev(torch_cuda, x)
    M = 28 * 500
    y = PC.codes(2 * M, 29)
    dev = Device(torch_cuda, y)
    tp, ptrp = to_dev(torch_cuda, packed12.pack12(y))
    tab = GC.table([(1, 40), (60, 61), (200, 499)])
    cut = 8 * 20_000
    for call in (None, lambda *a: d.gather_pack12_device_packed(ptrp, *a)):
        d.reset()
        d.push_device(ptr, cut)
        dev.gather(d, tab, call=call)
        d.push_device_final(ptr + 2 * cut, x.size - cut)
        d.finish()
        assert d.drain() == want and d.stats() == want_stats
    # ... and on the capture the stream itself is being pushed from
    d.reset()
    d.push_device(ptr, cut)
    got = torch_cuda.full((4096,), POISON, dtype=torch_cuda.uint8, device="cuda")
    off, over = d.gather_pack12_device(ptr, x.size, GC.table([(3, 5)]), got.data_ptr(), 4096)
    assert off.tolist() == [0, 176] and over == 0
    assert np.array_equal(got.cpu().numpy()[:168], packed12.pack12(x[2 * 84:2 * 140])) and not got.cpu().numpy()[168:176].any()
    d.push_device_final(ptr + 2 * cut, x.size - cut)
    d.finish()
    assert d.drain() == want


# ------------------------------------------------------------------ 6: the pipeline
def shifted(want, begin):
    return [(g + 28 * begin, ts + 28 * begin, pw, fr) for g, ts, pw, fr in want]


PIPE_N, PIPE_FRAMES, PIPE_SEED = 600_000, 12, 5               # the real capture of test_gpu_gather.py's pipeline, cut to whole groups of 8


def pipe_capture():
    from tools import gen_signal as G
    return G.sparse_capture(PIPE_N, PIPE_FRAMES, seed=PIPE_SEED)


@pytest.fixture(scope="module")
def pipe(capi, dec_factory, torch_cuda):
    """level -> gate (lead 2, hang 4) -> both gathers, run once."""
    x, truth = pipe_capture()
    M = 2 * (x.size // 4)
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    t, ptr = to_dev(torch_cuda, x)
    n_env = -(-M // 28)
    te, pe = to_dev(torch_cuda, np.zeros(n_env, np.float32))
    rep = d.level_device(ptr, x.size, pe, n_env)
    threshold = float(np.float32(48.0 * capi.level_percentile(rep["hist"], 0.5)))
    tab, b = d.bursts_device(pe, n_env, threshold, 2, 4, 4096)
    assert 1 <= b <= 4096 and rep["over"] == 0
    want16, off16 = BA().gather(x, tab, M, 4)
    want12, off12, over = BA().gather12(x, tab, M)
    out16 = torch_cuda.full((want16.size + TAIL,), POISON, dtype=torch_cuda.uint8, device="cuda")
    out12 = torch_cuda.full((want12.size + TAIL,), POISON, dtype=torch_cuda.uint8, device="cuda")
    assert np.array_equal(d.gather_device(ptr, x.nbytes, 4, M, tab, out16.data_ptr(), want16.size), off16)
    got_off, got_over = d.gather_pack12_device(ptr, x.size, tab, out12.data_ptr(), want12.size)
    got12 = out12.cpu().numpy()
    assert np.array_equal(got_off, off12) and got_over == over == 0
    assert np.array_equal(got12[:want12.size], want12) and (got12[want12.size:] == POISON).all()
    return dict(x=x, truth=truth, M=M, d=d, tab=tab, threshold=threshold, off16=off16, off12=off12, out16=out16, out12=out12,
                payload12=got12[:want12.size].copy(), keep=(t, te))


@pytest.mark.limit(120)
def test_pipeline(oracle, pipe):
    """decode_batch_device_packed over the packed pieces where they lie == decode_batch_device over adsb_gather_device's pieces,
    record for record and with the same Try/Ok tables, == the oracle on each piece's silent twin; all planted frames are found; the
    archive of kind 12 decodes to the same records."""
    x, M, d, tab = (pipe[k] for k in ("x", "M", "d", "tab"))
    sl = LV().burst_samples(tab, M)
    units12 = [8 * -(-int(hi - lo) // 4) for lo, hi in sl]
    f12, s12 = d.decode_batch_device_packed([pipe["out12"].data_ptr() + int(o) for o in pipe["off12"][:-1]], units12, stats=True)
    f16, s16 = d.decode_batch_device([pipe["out16"].data_ptr() + int(o) for o in pipe["off16"][:-1]], [2 * int(hi - lo) for lo, hi in sl], stats=True)
    assert len(f12) == len(f16) == tab.size
    want = []
    for i, (r, (lo, hi)) in enumerate(zip(tab, sl)):
        assert FC.recs(f12[i]) == FC.recs(f16[i]), i
        assert {k: s12[i][k] for k in ("try", "ok")} == {k: s16[i][k] for k in ("try", "ok")}, i
        w, st = FC.want_real(oracle, x[2 * lo:2 * hi])
        assert FC.recs(f12[i]) == w and {k: s12[i][k] for k in ("try", "ok")} == {k: st[k] for k in ("try", "ok")}, i
        want += shifted(w, int(r["begin"]))
    found = {bytes(f["frame"]) for mine in f12 for f in mine}
    assert len(pipe["truth"]) == PIPE_FRAMES and all(bytes(fr) in found for _, fr in pipe["truth"])
    # three quarters of the uint16 gather's bytes, up to the pad of each piece to a multiple of 16
    assert 3 * int(pipe["off16"][-1]) - 48 * tab.size <= 4 * pipe["payload12"].size <= 3 * int(pipe["off16"][-1]) + 64 * tab.size
    # the archive, through burst_archive.decode: ONE packed batch call, g and ts rebased
    arch = BA().unpack(BA().pack(12, x.size, M, pipe["threshold"], 2, 4, tab, pipe["payload12"]))
    frames, stats = BA().decode(d, arch)
    assert FC.recs(frames) == want
    assert stats["try"] == {df: sum(s[("try")][df] for s in s16) for df in (11, 17, 18)}


@pytest.mark.limit(60)
def test_a_piece_with_a_fill_decodes_as_the_uint16_piece(oracle, dec_factory, torch_cuda):
    """A capture with n % 8 == 4 and a frame at its very end, the whole of it one burst: its packed piece ends in four codes 2048, and
    decodes -- where it lies -- as the uint16 piece and as the oracle's silent twin."""
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    got_frames = 0
    for i, (n, end) in enumerate(((28 * 2 * 90 + 4, 0), (28 * 2 * 171 + 20, 1), (28 * 2 * 120 + 52, -1))):
        x = FC.real_capture(n, 600 + i, end, (17, 18, 11)[i])
        M = 2 * (n // 4)
        assert n % 8 == 4 and M % 4 == 2
        tab = GC.table([(0, -(-M // 28))])
        dev = Device(torch_cuda, x)
        out, off, over = dev.gather(d, tab)
        assert over == 0 and out.size == int(off[1]) and (8 * -(-M // 4)) - 2 * M == 4
        f12, s12 = d.decode_batch_device_packed([dev.out.data_ptr()], [8 * -(-M // 4)], stats=True)
        f16, s16 = d.decode_batch_device([dev.ptr], [n], stats=True)
        w, st = FC.want_real(oracle, x)
        assert FC.recs(f12[0]) == FC.recs(f16[0]) == w, i
        assert {k: s12[0][k] for k in ("try", "ok")} == {k: s16[0][k] for k in ("try", "ok")} == {k: st[k] for k in ("try", "ok")}, i
        got_frames += len(w)
    assert got_frames >= 2


# ------------------------------------------------------------------ 7: the host program
@pytest.mark.limit(180)
def test_host_program_packs_and_decodes(capi, pipe, tmp_path):
    """-L -U 48,2,4 -P out.brs on the uint16 file, its -p twin and its -t 3 twin: the same file, byte for byte
    burst_archive.pack(kind 12, ...); -k prints from it the packets it prints from -K's archive."""
    from adsbdec_amd import packed12, sample_formats
    x, M, tab = pipe["x"], pipe["M"], pipe["tab"]
    assert x.size % 8 == 0
    (tmp_path / "c.u16").write_bytes(x.tobytes())
    (tmp_path / "c.p12").write_bytes(packed12.pack12(x).tobytes())
    (tmp_path / "c.i16").write_bytes(sample_formats.to_format(3, x).tobytes())
    want = BA().pack(12, x.size, M, pipe["threshold"], 2, 4, tab, pipe["payload12"])
    gate = ["-L", "-U", "48,2,4"]
    for name, extra in (("c.u16", []), ("c.p12", ["-p"]), ("c.i16", ["-t", "3"])):
        dst = tmp_path / (name + ".brs")
        q = subprocess.run([capi.CLI_PATH, *gate, "-P", str(dst), *extra, "-f", str(tmp_path / name)], capture_output=True, timeout=100)
        err = q.stderr.decode()
        assert q.returncode == 0, err
        assert f"kept {tab.size} bursts, {pipe['payload12'].size} of {3 * M} bytes" in err, err
        assert f"bursts {tab.size} threshold".encode() in q.stdout
        assert dst.read_bytes() == want, name
    q = subprocess.run([capi.CLI_PATH, *gate, "-K", str(tmp_path / "k.brs"), "-f", str(tmp_path / "c.u16")], capture_output=True, timeout=100)
    assert q.returncode == 0, q.stderr.decode()
    assert (tmp_path / "k.brs").stat().st_size > (tmp_path / "c.u16.brs").stat().st_size
    for flags in (["-a"], ["-a", "-m"]):
        k12 = subprocess.run([capi.CLI_PATH, "-k", *flags, "-f", str(tmp_path / "c.u16.brs")], capture_output=True, timeout=100)
        k16 = subprocess.run([capi.CLI_PATH, "-k", *flags, "-f", str(tmp_path / "k.brs")], capture_output=True, timeout=100)
        assert k12.returncode == 0 and k16.returncode == 0, k12.stderr.decode() + k16.stderr.decode()
        assert k12.stdout == k16.stdout and k12.stdout.count(b"\n") >= PIPE_FRAMES, flags
        assert b"Try :" in k12.stderr and k12.stderr == k16.stderr


@pytest.mark.limit(60)
def test_host_program_writes_no_archive_over_a_code_that_does_not_fit(capi, pipe, tmp_path):
    """A code 4096 inside a burst: status 255, the count and a pointer to -K on stderr, no archive."""
    x, M, tab = pipe["x"].copy(), pipe["M"], pipe["tab"]
    lo, hi = LV().burst_samples(tab, M)[tab.size // 2]
    x[int(lo + hi)] = 4096                                   # sample lo + hi is the middle of [2 lo, 2 hi)
    (tmp_path / "c.u16").write_bytes(x.tobytes())
    q = subprocess.run([capi.CLI_PATH, "-L", "-U", "48,2,4", "-P", str(tmp_path / "o.brs"), "-f", str(tmp_path / "c.u16")],
                       capture_output=True, timeout=100)
    err = q.stderr.decode()
    assert q.returncode == 255 and "-P: 1 samples inside the bursts are above 4095" in err and "-K" in err, err
    assert not (tmp_path / "o.brs").exists()
