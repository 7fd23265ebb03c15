"""Flush (adsb_set_flush; DESIGN.md "Flush") on the MI355X (run with -m gpu): every flush answer -- single calls, streams and batches of
all five front ends in every flavour -- equals the oracle on the capture's silent twin, record for record and with the same Try/Ok
table.  These are the first launches that OWN offsets whose windows cross the end of the buffer: Stage A's edge path, the slicer's
reads, the try words and the count pass are all held at the top end here."""
import functools
import subprocess

import numpy as np
import pytest

import burst_cases as BC
import flush_cases as FC

pytestmark = pytest.mark.gpu

KINDS = ["u16", "as3", "as1", "packed", "iq2", "iq0", "iq8", "power"]
REAL = ("u16", "as3", "as1", "packed")
UNIT_BYTES = {"u16": 2, "as3": 2, "as1": 4, "packed": 1.5, "iq2": 4, "iq0": 8, "iq8": 2, "power": 4}   # per sample the call counts
TILE = lambda k: 28 * (252 * k - 44)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def dec_factory(capi, torch_cuda):
    made, extra = {}, []

    def make(fresh=False, **kw):
        key = tuple(sorted(kw.items()))
        if fresh:
            extra.append(capi.Decoder(**kw))
            return extra[-1]
        if key not in made:
            made[key] = capi.Decoder(**kw)
        return made[key]
    yield make
    for d in list(made.values()) + extra:
        d.close()


def SF():
    from adsbdec_amd import sample_formats
    return sample_formats


def to_dev(torch, a, tail=None):
    """The array's bytes on the device, `tail` (bytes of a decoy) DIRECTLY behind them: (tensor, pointer)."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if tail is not None:
        b = np.concatenate([b, np.ascontiguousarray(tail).view(np.uint8).reshape(-1)])
    if b.size == 0:
        b = np.zeros(16, np.uint8)
    t = torch.from_numpy(b if b.flags.writeable else b.copy()).cuda()
    return t, t.data_ptr()


# ------------------------------------------------------------------ a capture in a kind's format, and its truth
def as_kind(kind, base):
    """base: uint16 codes (real kinds) or int16 (n, 2) (the others) -> (the array the call is given, n as the call counts it)."""
    if kind == "u16":
        return base, base.size
    if kind == "as3":
        return SF().to_int16_real(base), base.size
    if kind == "as1":
        return SF().to_float32_real(base), base.size
    if kind == "packed":
        from adsbdec_amd import packed12
        n = base.size // 8 * 8
        return packed12.pack12(base[:n]), n
    if kind == "iq2":
        return base, len(base)
    if kind == "iq0":
        return SF().to_float32_iq(base), len(base)
    if kind == "iq8":
        return SF().to_int8_iq(base)[0], len(base)
    return FC.iq_power(base), len(base)


def truth(oracle, kind, base, fix1=False):
    if kind in REAL:
        x = base[:base.size // 8 * 8] if kind == "packed" else base
        return FC.want_real(oracle, x, fix1=fix1)
    a = FC.iq_power(SF().to_int8_iq(base)[0], 8) if kind == "iq8" else FC.iq_power(base)
    return FC.want_power(oracle, a)


@functools.lru_cache(maxsize=None)
def base_capture(family, n, seed, end, df):
    f = FC.real_capture if family == "real" else FC.iq_capture
    extra = tuple((s, (17, 11)[k % 2]) for k, s in enumerate(range(200, (n // 2 if family == "real" else n) - 3000, 11_000)))
    # (int8 keeps 8 of the 16 bits: the frames are loud enough to survive that)
    x = f(n, seed, end, df, extra=extra) if family == "real" else f(n, seed, end, df, sigma=1.0, extra=extra)
    x.setflags(write=False)
    return x


def family(kind):
    return "real" if kind in REAL else "iq"


def single(d, capi, kind, ptr, n):
    if kind == "u16":
        out, k = d.decode_device_raw(ptr, n)
        return capi._frames_to_dicts(out, k)
    if kind in ("as3", "as1"):
        return d.decode_device_as(3 if kind == "as3" else 1, ptr, n)
    if kind == "packed":
        out, k = d.decode_device_packed_raw(ptr, n)
        return capi._frames_to_dicts(out, k)
    if kind == "power":
        return d.decode_device_power(ptr, n)
    return d.decode_device_iq(int(kind[2:]), ptr, n)


def decoy(kind, units=4096):
    """Loud memory of the kind's dtype, never silence: what lies directly behind every buffer."""
    rng = np.random.default_rng(5)
    if kind in ("u16", "packed"):
        x = rng.integers(0, 4096, units, dtype=np.uint16)
        x[x == 0x800] = 0x801
        return x if kind == "u16" else __import__("adsbdec_amd.packed12", fromlist=["pack12"]).pack12(x[:units // 8 * 8])
    if kind == "as3":
        return rng.integers(-32768, 32767, units).astype("<i2") | 16
    if kind == "as1":
        return rng.uniform(0.5, 0.99, units).astype("<f4")
    if kind == "iq2":
        return rng.integers(-32768, 32767, (units, 2)).astype("<i2") | 1
    if kind == "iq0":
        return rng.uniform(0.5, 0.99, (units, 2)).astype("<f4")
    if kind == "iq8":
        return rng.integers(-128, 127, (units, 2)).astype(np.int8) | 1
    return rng.uniform(1.0, 2.0 ** 28, units).astype("<f4")


def single_cases(kind):
    """(n, end, df, passes): the sizes of the statement with a long and a short frame cut at M - 1 .. M + 20; every even M mod 28
    (M is even by definition) with every n % 4; M at a tile seam - 2 / + 0 / + 2 for K = 2 and the forced K = 3."""
    per = 4 if kind in REAL else 2                  # units per two power samples
    out = []
    for n in (2_048, 4_096, 81_956, 81_960):
        for i, end in enumerate((-1, 0, 1, 20)):
            out.append((n, end, (17, 11)[(i + n // 4) % 2], 0))
    for k in range(14):
        out.append((3_000 + per * k + k % per, (3, 0, 1, 5)[k % 4], (17, 11, 18)[k % 3], 0))
    for K in (2, 3):
        for dm in (-2, 0, 2):
            out.append(((TILE(K) + dm) * per // 2, 3, 17, K))
            out.append(((TILE(K) + dm) * per // 2 + 1, 0, 11, K))
    return out


# ------------------------------------------------------------------ 1. single calls
@pytest.mark.limit(120)
@pytest.mark.parametrize("kind", KINDS)
def test_single_calls(capi, oracle, dec_factory, torch_cuda, kind):
    """adsb_decode_device* on a flush handle, with a loud decoy directly behind every buffer: frames and Try/Ok (the device count
    pass) are the twin's; a handle without flush returns none of the frames of the captures below 81 960 samples."""
    n_frames = n_cut = 0
    plain = dec_factory(df18=True, collect_stats=True)
    for n, end, df, passes in single_cases(kind):
        base = base_capture(family(kind), n, 300 + n % 89 + end, end, df)
        arr, cnt = as_kind(kind, base)
        want, want_stats = truth(oracle, kind, base)
        kw = dict(debug_passes=passes) if passes else {}
        d = dec_factory(flush=True, df18=True, collect_stats=True, **kw)
        assert d.flush
        t, ptr = to_dev(torch_cuda, arr, decoy(kind))
        got = single(d, capi, kind, ptr, cnt)
        assert FC.recs(got) == want, (kind, n, end, passes, len(got), len(want))
        assert d.stats() == want_stats, (kind, n, end, passes)
        M = 2 * (cnt // 4) if kind in REAL else 2 * (cnt // 2)
        n_frames += len(want)
        n_cut += sum(g + (640 if len(fr) == 7 else 1200) > M for g, _, _, fr in want)
        if 2 * ((cnt + 3) // 4 if kind in REAL else cnt // 2) < FC.APBUFFSZ:
            assert single(plain, capi, kind, ptr, cnt) == []              # today's behaviour: below the horizon, nothing
    assert n_frames >= 30 and n_cut >= 8, (n_frames, n_cut)


@pytest.mark.limit(60)
@pytest.mark.parametrize("kind", ["u16", "iq2", "power"])
def test_host_stats_and_fix_1bit(capi, oracle, dec_factory, torch_cuda, kind):
    """collect_stats through the host-side count (no_streaming: the try words come back on the launch-wide list) and fix_1bit: a
    capture whose last frame has one damaged bit, with tries in the last 1 196 offsets."""
    base = base_capture(family(kind), 9_000, 41, 2, 17)
    arr, cnt = as_kind(kind, base)
    want = truth(oracle, kind, base)
    t, ptr = to_dev(torch_cuda, arr, decoy(kind))
    d = dec_factory(flush=True, df18=True, collect_stats=True, debug_no_streaming=1)
    assert (FC.recs(single(d, capi, kind, ptr, cnt)), d.stats()) == want
    if kind == "u16":
        from tools import gen_signal as G
        rng = np.random.default_rng(3)
        fr = bytearray(FC._frame(rng, 17, 1))
        good = bytes(fr)
        fr[6] ^= 0x10                                                       # one bit of the payload
        n = 7_001
        M = 2 * (n // 4)
        x = G.synth(n, [(2 * (M + 2 - 1200), bytes(fr), 900.0, 0.4)], 4.0, 12)
        fw, sw = oracle.decode(FC.twin_real(x), df18=True, fix1=True)
        assert any(f["frame"] == good for f in fw) and sw["fixed"] >= 1
        assert sum(sw["try"].values()) > 0
        df = dec_factory(flush=True, df18=True, collect_stats=True, fix_1bit=True)
        t2, p2 = to_dev(torch_cuda, x, decoy(kind))
        out, k = df.decode_device_raw(p2, n)
        assert FC.recs(capi._frames_to_dicts(out, k)) == FC.recs(fw)
        st = df.stats()
        assert {"try": st["try"], "ok": st["ok"]} == {"try": sw["try"], "ok": sw["ok"]}


# ------------------------------------------------------------------ 2. streams
def host_slice(kind, arr, lo, hi):
    if kind == "packed":
        return arr[lo // 8 * 12: hi // 8 * 12]
    return arr[lo:hi]


def push_host(d, kind, piece, mode):
    if kind == "u16":
        return d.push(piece) if mode == "sync" else d.push_async(piece)
    if kind in ("as3", "as1"):
        return d.push_as(3 if kind == "as3" else 1, piece, mode)
    if kind == "packed":
        return d.push_packed(piece) if mode == "sync" else d.push_packed_async(piece)
    if kind == "power":
        return d.push_power(np.ascontiguousarray(piece), mode)
    return d.push_iq(int(kind[2:]), np.ascontiguousarray(piece), mode)


def push_dev(d, kind, ptr, n, final):
    if kind == "u16":
        return d.push_device_final(ptr, n) if final else d.push_device(ptr, n)
    if kind in ("as3", "as1"):
        return d.push_device_as(3 if kind == "as3" else 1, ptr, n, final)
    if kind == "packed":
        return d.push_device_packed_final(ptr, n) if final else d.push_device_packed(ptr, n)
    if kind == "power":
        return d.push_device_power(ptr, n, final)
    return d.push_device_iq(int(kind[2:]), ptr, n, final)


def pieces_of(total, sizes):
    out, at = [], 0
    for s in sizes:
        s = min(s, total - at)
        out.append((at, at + s))
        at += s
    if at < total:
        out.append((at, total))
    return out


@pytest.mark.limit(120)
@pytest.mark.parametrize("kind", KINDS)
def test_streams(capi, oracle, dec_factory, torch_cuda, kind):
    """The same capture pushed in ragged pieces -- 1 sample, 7, empty pushes, a run, a tile + 1 and - 1 -- through host pushes, async
    pushes, device pushes staged and in place, and a _final push: always the single call's answer, which is the twin's.  A second
    adsb_finish returns nothing new, and adsb_reset keeps the flag."""
    base = base_capture(family(kind), 119_996 if kind in REAL else 119_998, 77, 3, 17)
    arr, cnt = as_kind(kind, base)
    want = truth(oracle, kind, base)
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    t, ptr = to_dev(torch_cuda, arr, decoy(kind))
    assert (FC.recs(single(d, capi, kind, ptr, cnt)), d.stats()) == want
    q = 8 if kind == "packed" else 1
    ragged = [1 * q, 7 * q, 0, 28 * q, 0, 12_881 // q * q + (q if q > 1 else 0), 12_879 // q * q, 4_093 // q * q, 50_000 // q * q]
    for mode in ("sync", "async"):
        d.reset()
        assert d.flush                                                    # sticky across adsb_reset
        got = []
        keep = []
        for lo, hi in pieces_of(cnt, ragged):
            piece = np.ascontiguousarray(host_slice(kind, arr, lo, hi))
            keep.append(piece)
            push_host(d, kind, piece, mode)          # (async: the piece stays borrowed, and alive in `keep`, until the stream ends)
            got += d.drain()
        d.finish()
        got += d.drain()
        assert (FC.recs(got), d.stats()) == want, (kind, mode)
        d.finish()
        assert d.drain() == []                                            # a second adsb_finish: nothing new
    ub = UNIT_BYTES[kind]
    for sizes, last_final in (([16, 65_560], True), ([16, 40_000], True), ([8, 0, 7 * q, 30_000 // q * q, 0], False)):
        d.reset()
        got = []
        ps = pieces_of(cnt, sizes)
        for i, (lo, hi) in enumerate(ps):
            final = last_final and i == len(ps) - 1
            push_dev(d, kind, ptr + int(lo * ub), hi - lo, final)
            got += d.drain()
        if not last_final:
            d.finish()
            got += d.drain()
        assert (FC.recs(got), d.stats()) == want, (kind, sizes)


# ------------------------------------------------------------------ 3. batches
def batch_call(d, kind, ptrs, ns):
    if kind == "u16":
        return d.decode_batch_device(ptrs, ns, stats=True)
    if kind in ("as3", "as1"):
        return d.decode_batch_device_as(3 if kind == "as3" else 1, ptrs, ns, stats=True)
    if kind == "packed":
        return d.decode_batch_device_packed(ptrs, ns, stats=True)
    if kind == "power":
        return d.decode_batch_device_power(ptrs, ns, stats=True)
    return d.decode_batch_device_iq(int(kind[2:]), ptrs, ns, stats=True)


def lay_out(torch, kind, arrays):
    """The captures in ONE device buffer, each at a 16-byte boundary, every byte between and behind them LOUD: a read of the
    neighbour where silence is meant changes a bit.  -> (tensor, pointers)."""
    loud = np.ascontiguousarray(decoy(kind, 1 << 16)).view(np.uint8).reshape(-1)
    parts, ptrs, at = [], [], 0
    for a in arrays:
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        ptrs.append(at)
        parts.append(b)
        at += b.size
        pad = (-at) % 16 + 16
        parts.append(loud[at % 4096: at % 4096 + pad])
        at += pad
    parts.append(loud[:8192])
    t = torch.from_numpy(np.concatenate(parts)).cuda()
    return t, [t.data_ptr() + p for p in ptrs]


def check_batch(capi, oracle, d, torch_cuda, kind, bases, singles_every=8):
    arrs = [as_kind(kind, b) for b in bases]
    t, ptrs = lay_out(torch_cuda, kind, [a for a, _ in arrs])
    ns = [c for _, c in arrs]
    frames, stats = batch_call(d, kind, ptrs, ns)
    assert len(frames) == len(bases)
    wants = [truth(oracle, kind, b) for b in bases]
    for i, (w, ws) in enumerate(wants):
        assert (FC.recs(frames[i]), stats[i]) == (w, ws), (kind, i, ns[i])
    for i in range(0, len(bases), singles_every):
        assert FC.recs(single(d, capi, kind, ptrs[i], ns[i])) == wants[i][0], (kind, i)
    return sum(len(w) for w, _ in wants)


@pytest.mark.limit(120)
@pytest.mark.parametrize("kind", KINDS)
def test_batch_of_short_captures_between_loud_neighbours(capi, oracle, dec_factory, torch_cuda, kind):
    rng = np.random.default_rng(11)
    ns = [0, 3, 5, 1_199] + [int(v) for v in rng.integers(1_300, 6_001, size=60)]
    bases = [base_capture(family(kind), n, 500 + i, FC.ENDS[i % 6], (17, 11, 18)[i % 3]) for i, n in enumerate(ns)]
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    assert check_batch(capi, oracle, d, torch_cuda, kind, bases) >= 40
    frames, _ = batch_call(dec_factory(df18=True, collect_stats=True), kind, *_ptrs_ns(torch_cuda, kind, bases))
    assert all(f == [] for f in frames)                                   # without flush: nothing, by construction


def _ptrs_ns(torch, kind, bases, _keep=[]):
    arrs = [as_kind(kind, b) for b in bases]
    t, ptrs = lay_out(torch, kind, [a for a, _ in arrs])
    _keep[:] = [t]
    return ptrs, [c for _, c in arrs]


@pytest.mark.limit(120)
@pytest.mark.parametrize("kind", ["u16", "iq2", "power", "iq8"])
def test_batch_with_roll_overs_and_cut_captures(capi, oracle, dec_factory, torch_cuda, kind):
    """adsb_debug_config.batch_launch_offsets = two tiles of K = 2: captures longer than that are cut into segments, the others roll
    over into later launches."""
    per = 4 if kind in REAL else 2
    ms = [30_000, 2_000, 12_880, 12_882, 25_760, 25_762, 700, 40_000, 12_878, 5_000]
    bases = [base_capture(family(kind), m * per // 2 + i % per, 900 + i, FC.ENDS[i % 6], (17, 11)[i % 2]) for i, m in enumerate(ms)]
    d = dec_factory(flush=True, df18=True, collect_stats=True, debug_passes=2, debug_batch_launch_offsets=2 * TILE(2))
    assert check_batch(capi, oracle, d, torch_cuda, kind, bases, singles_every=3) >= 10
    _, _, segs, launches = d.batch_records()
    assert len(launches) >= 4 and len(segs) > len(ms)


@pytest.mark.limit(180)
def test_batch_of_4096_short_captures(capi, oracle, dec_factory, torch_cuda):
    """The README's batch: 4 096 captures of 2 048 samples, a frame in every 16th."""
    noise = [base_capture("real", 2_048, 2000 + i, -5000, 17) for i in range(4)]      # (end far below 0: no frame fits)
    with_frame = [base_capture("real", 2_048, 3000 + i, FC.ENDS[i % 6], 11) for i in range(256)]   # (a long frame is longer than the capture)
    bases = [with_frame[i // 16] if i % 16 == 7 else noise[i % 4] for i in range(4096)]
    x = np.concatenate(bases)
    t, ptr = to_dev(torch_cuda, x, decoy("u16"))
    d = dec_factory(flush=True, df18=True, collect_stats=True)
    frames, stats = d.decode_batch_device([ptr + 4096 * i for i in range(4096)], [2048] * 4096, stats=True)
    cache = {}
    total = 0
    for i, b in enumerate(bases):
        if id(b) not in cache:
            cache[id(b)] = FC.want_real(oracle, b)
        assert (FC.recs(frames[i]), stats[i]) == cache[id(b)], i
        total += len(frames[i])
    assert total >= 150


# ------------------------------------------------------------------ 4. the pipeline
@pytest.mark.limit(120)
def test_pipeline_with_short_pieces(capi, oracle, dec_factory, torch_cuda):
    """export -> level with the envelope -> the gate at lead 2, hang 4 -> ONE batch decode of the pieces on a flush handle: 36
    bursts that cover under 1 % of the capture hold all 36 planted frames; the same call without flush returns nothing."""
    from adsbdec_amd import levels
    p = BC.pipeline()
    x, M = p["x"], p["a"].size
    d = dec_factory(flush=True, df18=True)
    t, ptr = to_dev(torch_cuda, x)
    ta, pa = to_dev(torch_cuda, np.zeros(M, np.float32))
    assert d.power_device_iq(2, ptr, len(x), pa, M) == M
    n_env = -(-M // 28)
    te, pe = to_dev(torch_cuda, np.zeros(n_env, np.float32))
    rep = d.level_device_power(pa, M, pe, n_env)
    threshold = float(np.float32(BC.FACTOR * capi.level_percentile(rep["hist"], 0.5)))
    assert threshold == p["threshold"]
    want_b = levels.bursts(p["env"], threshold, 2, 4)
    got, b = d.bursts_device(pe, n_env, threshold, 2, 4, 64)
    assert b == 36 == want_b.size
    assert [(int(r["begin"]), int(r["end"])) for r in got] == [(int(r["begin"]), int(r["end"])) for r in want_b]
    slices = levels.burst_samples(got, M)
    covered = sum(int(hi - lo) for lo, hi in slices)
    assert covered < 0.01 * M, covered / M
    ptrs, ns = [pa + 112 * int(r["begin"]) for r in got], [int(hi - lo) for lo, hi in slices]
    frames = d.decode_batch_device_power(ptrs, ns)
    found = set()
    for (lo, hi), mine in zip(slices, frames):
        want = FC.want_power(oracle, np.ascontiguousarray(p["a"][lo:hi]))[0]
        assert FC.recs(mine) == want, (lo, hi)
        found |= {f["frame"] for f in mine}
    assert len(p["truth"]) == 36 and all(fr in found for _, fr in p["truth"])
    plain = dec_factory(df18=True)
    assert sum(len(f) for f in plain.decode_batch_device_power(ptrs, ns)) == 0      # today's behaviour: every piece is below the horizon


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.limit(60)
def test_refusals(capi, dec_factory, torch_cuda):
    import ctypes as C
    x = base_capture("real", 4_096, 1, 0, 17)
    t, ptr = to_dev(torch_cuda, x)
    want = None
    d = dec_factory(fresh=True, df18=True)
    L, h = d._L, d._h
    err = lambda: L.adsb_last_error(h).decode()
    d.push(x[:100])
    assert L.adsb_set_flush(h, 1) == -1 and "before the first push" in err() and not d.flush
    d.reset()
    d.set_flush(True)
    assert L.adsb_set_long_stream(h, 1) == -1 and "adsb_set_flush" in err()
    out, k = d.decode_device_raw(ptr, x.size)                              # the handle stays usable
    want = capi._frames_to_dicts(out, k)
    nc, nt = C.c_size_t(0), C.c_size_t(0)
    cands = (capi.Candidate * 16)()
    for fn in (L.adsb_scan_shard, L.adsb_scan_wrap_window):
        assert fn(h, C.c_void_p(ptr), 0, x.size, 0, 28, cands, 16, C.byref(nc), None, 0, C.byref(nt)) == -1
        assert "adsb_set_flush" in err(), err()
    out, k = d.decode_device_raw(ptr, x.size)
    assert capi._frames_to_dicts(out, k) == want
    d.reset()
    d.set_flush(False)
    d.set_long_stream(True)
    assert L.adsb_set_flush(h, 1) == -1 and "adsb_set_long_stream" in err() and not d.flush
    d.set_long_stream(False)
    d.set_flush(True)
    out, k = d.decode_device_raw(ptr, x.size)
    assert capi._frames_to_dicts(out, k) == want


# ------------------------------------------------------------------ 6. the host program
def _run(capi, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, timeout=120)


@pytest.mark.limit(120)
def test_cli_flush(capi, oracle, torch_cuda, tmp_path):
    """-E -a -f, and -E with -q 2, -w and -B: the bytes are oracle.avr_lines of the twin's frames and the table is the twin's; without
    -E the bytes are what they are today (nothing, for files this short)."""
    xr = base_capture("real", 30_001, 8, 3, 17)
    xi = base_capture("iq", 20_001, 9, 1, 17)
    fr, st = oracle.decode(FC.twin_real(xr), df18=True)
    fp, sp = oracle.demod_power(FC.twin_power(FC.iq_power(xi)), df18=True)
    assert len(fr) >= 3 and len(fp) >= 2
    (tmp_path / "r.u16").write_bytes(xr.tobytes())
    (tmp_path / "c.iq16").write_bytes(xi.tobytes())
    (tmp_path / "c.pw").write_bytes(FC.iq_power(xi).tobytes())
    for args, frames in ((["-E", "-a", "-f", str(tmp_path / "r.u16")], fr), (["-E", "-a", "-q", "2", "-f", str(tmp_path / "c.iq16")], fp),
                         (["-E", "-a", "-w", "-f", str(tmp_path / "c.pw")], fp)):
        p = _run(capi, *args)
        err = p.stderr.decode()
        assert p.returncode == 0, err
        assert p.stdout == oracle.avr_lines(frames), args
        q = _run(capi, *[a for a in args if a != "-E"])
        assert q.returncode == 0 and q.stdout == b""
    x2 = base_capture("real", 5_000, 10, 0, 11)
    (tmp_path / "s.u16").write_bytes(x2.tobytes())
    (tmp_path / "list.txt").write_text(f"{tmp_path / 'r.u16'}\n{tmp_path / 's.u16'}\n")
    p = _run(capi, "-E", "-a", "-B", str(tmp_path / "list.txt"))
    assert p.returncode == 0, p.stderr.decode()
    assert (tmp_path / "r.u16.avr").read_bytes() == oracle.avr_lines(fr)
    assert (tmp_path / "s.u16.avr").read_bytes() == oracle.avr_lines(oracle.decode(FC.twin_real(x2), df18=True)[0])
    p = _run(capi, "-a", "-B", str(tmp_path / "list.txt"))
    assert p.returncode == 0 and (tmp_path / "r.u16.avr").read_bytes() == b""
