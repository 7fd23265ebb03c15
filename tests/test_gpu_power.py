"""float32 power-sample streams on the MI355X (run with -m gpu): the scan kernels' power front end (scan_power_kernel.hip) and
every _power call of the library, held to the reference's demodulator on the very array that is pushed: the committed fixtures
(uint16 ones through oracle.power, IQ ones through iq_power), the kernel's candidates offset by offset on general floats, edge
values (subnormals, ties, sums one ulp around an integer, c == 2 c'), lengths, chunked and staged streams, batches, the refusals,
the 1-bit repair and the C host program's -w."""
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, golden_records, load_golden, records
from test_gpu_iq import K_BIG, N_BIG, TILE, big_capture, to_dev
from test_iq_cpu import iq_cases, load_iq
from test_power_cpu import SCALES, TINY, general_capture, scaled

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
    made, by_cfg = [], {}

    def make(fresh=False, **kw):
        """A handle with this configuration: one per configuration and module (every decode call resets it) unless `fresh`."""
        key = tuple(sorted(kw.items()))
        if fresh or key not in by_cfg:
            d = capi.Decoder(**kw)
            made.append(d)
            if fresh:
                return d
            by_cfg[key] = d
        return by_cfg[key]
    yield make
    for d in made:
        d.close()


def S():
    from adsbdec_amd import sample_formats
    return sample_formats


def fixture_power(oracle, name):
    """(power samples, record) of a committed fixture: "iq/<name>" through iq_power, the uint16 ones through the oracle's FIR."""
    if name.startswith("iq/"):
        x, rec = load_iq(name[3:])
        return S().iq_power(x), rec
    x, rec = load_golden(name)
    return oracle.power(x), rec


ALL_FIXTURES = golden_cases() + ["iq/" + n for n in iq_cases()]


# ------------------------------------------------------------------ 1. the fixtures through every call
@pytest.mark.limit(120)
@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_fixtures_through_every_call(capi, oracle, dec_factory, torch_cuda, name):
    """Frames (g, ts, pw, bytes) and Try/Ok of every fixture through push_power + finish, push_power_async (chunk 30 001),
    push_device_power_final and decode_device_power."""
    a, rec = fixture_power(oracle, name)
    assert S().power_domain_ok(a)
    want, n = golden_records(rec), len(a)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptr = to_dev(torch_cuda, a)

    def check(frames, how):
        assert records(frames) == want, (how, len(frames), len(want))
        assert d.stats() == rec["stats"], how

    check(d.decode_power(a), "push_power + finish")
    check(d.decode_power(a, chunk=30_001, mode="async"), "push_power_async")
    d.reset()
    d.push_device_power(ptr, n, final=True)
    check(d.drain(), "push_device_power_final")
    check(d.decode_device_power(ptr, n), "decode_device_power")


# ------------------------------------------------------------------ 2. offset by offset
_scaled = {}


def big_scaled(oracle, s):
    """test_gpu_iq.big_capture's power samples times s (1.0: as they are), with the oracle's exhaustive evaluation and greedy decode."""
    if s not in _scaled:
        big = big_capture(oracle)
        if s == 1.0:
            _scaled[s] = dict(a=big["a"], all=big["all"], dec=big["dec"])
        else:
            b = scaled(big["a"], s)
            assert S().power_domain_ok(b)
            _scaled[s] = dict(a=b, all=oracle.scan_all(b, 0, N_BIG - 1195, True), dec=oracle.demod_power(b, df18=True))
            assert len(_scaled[s]["dec"][0]) > 690
    return _scaled[s]


def check_candidates(d, ptr, n, want_c, want_t, passes=K_BIG):
    """One capture through the batch call of a handle made with all_candidates + collect_stats: its records and try words."""
    frames, stats = d.decode_batch_device_power([ptr], [n], stats=True)
    cands, tries, segs, launches = d.batch_records()
    assert all(l["passes"] == passes for l in launches)
    base = segs[0]["base"]
    got = [(g - base, pw, fr) for g, pw, fr, _ in cands]
    if got != want_c:
        gg, ww = {c[0]: c for c in got}, {c[0]: c for c in want_c}
        raise AssertionError(("candidates", len(got), len(want_c), sorted(set(gg) ^ set(ww))[:8],
                              [(gg[g], ww[g]) for g in sorted(set(gg) & set(ww)) if gg[g] != ww[g]][:4]))
    assert np.array_equal(np.sort(tries - np.uint64(base << 2)), np.sort(want_t))    # words (g << 2) | DF code
    return frames[0], stats[0]


@pytest.mark.limit(180)
@pytest.mark.parametrize("s", (1.0,) + SCALES)
def test_candidates_offset_by_offset(capi, oracle, dec_factory, torch_cuda, s):
    """all_candidates = 1: every CRC-valid offset the device reports -- (g, pw, bytes) -- and, with collect_stats, every DF-gate
    pass equal the oracle's exhaustive evaluation of all n - 1195 offsets of the pushed array: the capture of test_gpu_iq (frames
    at -1195 / -600 / -1 / 0 around twelve K = 2 tile boundaries, at every offset mod 28, at g = 0 and ending on the last sample) as
    it is and as general floats fl(a s).  The list is read back through the batch call (scan_power_batch_kernel); the stream
    kernel (scan_power_kernel) is held to the greedy decode, with and without the never-visited filter, at K = 2 and the default K."""
    big = big_scaled(oracle, s)
    a = big["a"]
    t, ptr = to_dev(torch_cuda, a)
    want_c, want_t = big["all"]
    wf, ws = big["dec"]
    d = dec_factory(df18=True, collect_stats=True, all_candidates=True, debug_passes=K_BIG)
    frames, stats = check_candidates(d, ptr, N_BIG, want_c, want_t)
    got_g = {c[0] for c in want_c}
    for st in big_capture(oracle)["starts"]:               # every planted frame is a candidate at its own offset
        assert st in got_g, st
    assert records(frames) == records(wf) and stats == ws
    for kw in (dict(all_candidates=True, debug_passes=K_BIG), dict(debug_passes=K_BIG), dict(), dict(debug_passes=7)):
        ds = dec_factory(df18=True, collect_stats=True, **kw)
        assert records(ds.decode_device_power(ptr, N_BIG)) == records(wf), kw
        assert ds.stats() == ws, kw


# ------------------------------------------------------------------ 3. edge values
N_EDGE = 1 << 16


def fl_sum(x, y):
    return np.float32(np.float32(x) + np.float32(y))


def partner_for_sum(x, target):
    """y >= 0 with fl(x + y) == target exactly (binary32), found by walking from target - x."""
    y = np.float32(np.float32(target) - np.float32(x))
    for _ in range(64):
        r = fl_sum(x, y)
        if r == target:
            assert y >= 0
            return y
        y = np.nextafter(y, np.float32(np.inf) if r < target else np.float32(0), dtype=np.float32)
    raise AssertionError((x, target))


def edge_capture(oracle):
    """64 Ki power samples cut from the dense part of the capture of test 2, then: [20000, 30000) scaled by 1e-38; [34000, 38000)
    period 5, so a[m] == a[m+5] for whole runs; at six frames below 20000 the first preamble sum a[g] + a[g+10] one ulp below, at and one
    ulp above an integer, c[g] == 2 c[g+5] and c[g+35] == 2 c[g+30] exactly, and one frame whose DATA samples are all subnormal."""
    big = big_capture(oracle)
    a = big["a"][13 * TILE: 13 * TILE + N_EDGE].copy()
    frames0, _ = oracle.demod_power(a, df18=True)
    a[20000:30000] = scaled(a[20000:30000], TINY)
    a[34000:38000] = np.tile(a[34000:34005], 800)
    fr = [f for f in frames0 if 1201 <= f["g"] and f["g"] + 1300 < 20000][::2]    # (inside the first buffer: the greedy decode sees them too)
    assert len(fr) >= 6
    notes = {}
    for f, how in zip(fr, ("below", "at", "above", "c_eq_2c1", "c_eq_2c2", "subnormal_data")):
        g = f["g"]
        if how in ("below", "at", "above"):
            n_int = np.float32(np.trunc(fl_sum(a[g], a[g + 10])))
            target = {"below": np.nextafter(n_int, np.float32(0), dtype=np.float32), "at": n_int,
                      "above": np.nextafter(n_int, np.float32(np.inf), dtype=np.float32)}[how]
            a[g + 10] = partner_for_sum(a[g], target)
            assert fl_sum(a[g], a[g + 10]) == target and int(target) == int(n_int) - (how == "below")
        elif how == "c_eq_2c1":      # p1 = c[g] against s1 = c[g+5] (demod.c:102-107): exactly twice, so NOT greater
            c = int(fl_sum(a[g], a[g + 10]))
            if c % 2:
                a[g] += np.float32(1.0)
                c = int(fl_sum(a[g], a[g + 10]))
            assert c % 2 == 0
            a[g + 5], a[g + 15] = np.float32(c // 2), np.float32(0.0)
            assert int(fl_sum(a[g], a[g + 10])) == 2 * int(fl_sum(a[g + 5], a[g + 15]))
        elif how == "c_eq_2c2":      # p2 = c[g+35] against s2 = c[g+30]
            c = int(fl_sum(a[g + 35], a[g + 45]))
            if c % 2:
                a[g + 35] += np.float32(1.0)
                c = int(fl_sum(a[g + 35], a[g + 45]))
            a[g + 30], a[g + 40] = np.float32(c // 2), np.float32(0.0)
            assert int(fl_sum(a[g + 35], a[g + 45])) == 2 * int(fl_sum(a[g + 30], a[g + 40]))
        else:                        # every sample behind the preamble is subnormal: the bits are comparisons of subnormals
            seg = scaled(scaled(a[g + 80: g + 1200], 2.0 ** -100), 2.0 ** -48)
            assert float(seg.max()) < np.finfo(np.float32).tiny and (seg > 0).sum() > 1000
            a[g + 80: g + 1200] = seg
        notes[how] = g
    assert S().power_domain_ok(a)
    return a, notes


@pytest.mark.limit(120)
def test_edge_values(capi, oracle, dec_factory, torch_cuda):
    """The edge capture's candidates and tries equal the oracle's, offset by offset, and its greedy decode the oracle's.  What the
    oracle says about the planted values is asserted too, so that the comparison is not between two empty lists."""
    a, notes = edge_capture(oracle)
    want_c, want_t = oracle.scan_all(a, 0, N_EDGE - 1195, True)
    wf, ws = oracle.demod_power(a, df18=True)
    cand_g = {c[0] for c in want_c}
    try_g = {int(w) >> 2 for w in want_t}
    assert not [g for g in cand_g | try_g if 20000 <= g < 30000 - 1196]            # the tiny stretch: no candidate, no try
    assert [f for f in wf if f["g"] < 20000 - 1200] and [f for f in wf if 30000 <= f["g"] < 34000 - 1200]   # frames on either side
    assert not [g for g in cand_g if 34000 <= g < 38000 - 1196]                      # ties: never "greater"
    for how in ("below", "at", "above", "subnormal_data"):
        assert notes[how] in cand_g, how
    assert notes["c_eq_2c1"] not in cand_g and notes["c_eq_2c2"] not in cand_g and notes["c_eq_2c1"] not in try_g
    t, ptr = to_dev(torch_cuda, a)
    for passes in (K_BIG, 7):
        d = dec_factory(df18=True, collect_stats=True, all_candidates=True, debug_passes=passes)
        frames, stats = check_candidates(d, ptr, N_EDGE, want_c, want_t, passes)
        assert records(frames) == records(wf) and stats == ws
    ds = dec_factory(df18=True, collect_stats=True)
    assert records(ds.decode_device_power(ptr, N_EDGE)) == records(wf) and ds.stats() == ws
    assert records(ds.decode_power(a, chunk=10_007)) == records(wf) and ds.stats() == ws


# ------------------------------------------------------------------ 4. lengths, chunks, staging
LENGTHS = [0, 1, 2, 1195, 1196, 1197, 1200, 1201] + list(range(40978, 40984)) + list(range(42179, 42184)) + list(range(81958, 81963))


@pytest.mark.limit(120)
def test_prefixes_of_one_capture(capi, oracle, dec_factory, torch_cuda):
    """Every length around the window (1196), the reference's buffer (40 980), buffer + 1200 and two buffers: the prefix decodes
    as the oracle decodes it, from the device and from the host; a trailing odd sample is never seen."""
    a = general_capture(1 << 17)[:82000]
    t, ptr = to_dev(torch_cuda, a)
    d = dec_factory(df18=True, collect_stats=True)
    seen = set()
    for n in LENGTHS:
        wf, ws = oracle.demod_power(a[:n].copy(), df18=True)
        assert records(d.decode_device_power(ptr, n)) == records(wf), n
        assert d.stats() == ws, n
        assert records(d.decode_power(a[:n])) == records(wf) and d.stats() == ws, n
        seen.add(len(wf))
    assert seen == {0, 33, 66}         # (nothing decodes below one buffer of the reference's, 40 980 samples: the end-of-file horizon)


@pytest.mark.limit(180)
def test_chunked_and_staged_streams_equal_one_aligned_push(capi, oracle, dec_factory, torch_cuda):
    """The capture of test 2 in pieces of 1, 3, 4 and 30 001 samples and the rest, and in uniform chunks of 30 001, from the host
    (sync, async, overlap) and from the device; a short capture sample by sample and in threes and fours; device pointers 4 and 8
    bytes off a 16-byte boundary (the staged path): the frames and Try/Ok of one aligned push, which are the oracle's."""
    big = big_scaled(oracle, 1.0)
    a = big["a"]
    wf, ws = big["dec"]
    d = dec_factory(df18=True, collect_stats=True)
    dov = dec_factory(df18=True, collect_stats=True, push_overlap=True)
    t, ptr = to_dev(torch_cuda, a)
    assert records(d.decode_device_power(ptr, N_BIG)) == records(wf) and d.stats() == ws
    cuts = np.cumsum([0, 1, 3, 4, 30001]).tolist() + [N_BIG]
    for dec in (d, dov):
        dec.reset()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.push_power(a[lo:hi])
        dec.finish()
        assert records(dec.drain()) == records(wf) and dec.stats() == ws
        assert records(dec.decode_power(a, chunk=30_001)) == records(wf) and dec.stats() == ws
    assert records(d.decode_power(a, chunk=30_001, mode="async")) == records(wf) and d.stats() == ws
    d.reset()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.push_device_power(ptr + 4 * lo, hi - lo)
    d.finish()
    assert records(d.drain()) == records(wf) and d.stats() == ws
    for lead in (4, 8):
        t1, p1 = to_dev(torch_cuda, a, lead=lead)
        assert p1 % 16 == lead
        assert records(d.decode_device_power(p1, N_BIG)) == records(wf) and d.stats() == ws
        d.reset()
        d.push_device_power(p1, N_BIG // 2)
        d.push_device_power(p1 + 4 * (N_BIG // 2), N_BIG // 2, final=True)
        assert records(d.drain()) == records(wf) and d.stats() == ws
    short = np.ascontiguousarray(general_capture(1 << 17)[:42_201])
    sf, ss = oracle.demod_power(short, df18=True)
    assert len(sf) >= 30
    for chunk in (1, 3, 4):            # 2 001 pushes of `chunk` samples -- every stream position mod 4, odd ones included -- then the rest
        head = 2001 * chunk
        for dec, mode in ((d, "sync"), (d, "async"), (dov, "sync")):
            dec.reset()
            for lo in range(0, head, chunk):
                dec.push_power(short[lo:lo + chunk], mode)
            dec.push_power(short[head:], mode)
            dec.finish()
            assert records(dec.drain()) == records(sf) and dec.stats() == ss, (chunk, mode)


# ------------------------------------------------------------------ 5. batches
@pytest.mark.limit(120)
def test_batches_equal_the_single_calls(capi, oracle, dec_factory, torch_cuda):
    """Nine captures -- empty, one sample, shorter than a window, odd lengths around the reference's buffer, two fixtures and two of
    general floats -- through the device call and the host call: every capture's frames and Try/Ok table are those of its own
    decode_device_power, which are the oracle's."""
    mixed, _ = fixture_power(oracle, "iq/mixed_df_a")
    u16, _ = fixture_power(oracle, golden_cases()[0])
    gen = general_capture(1 << 17)
    caps = [gen[:0], gen[:1], gen[:1195], gen[:40979], gen[:40982], mixed, u16, gen[:100_001], scaled(gen, SCALES[0])]
    caps = [np.ascontiguousarray(c) for c in caps]
    d = dec_factory(df18=True, collect_stats=True)
    held = [to_dev(torch_cuda, c) for c in caps]
    single = []
    for c, (_, p) in zip(caps, held):
        single.append((records(d.decode_device_power(p, len(c))), d.stats()))
        wf, ws = oracle.demod_power(c, df18=True)
        assert single[-1] == (records(wf), ws), len(c)
    assert not single[0][0] and not single[2][0] and not single[3][0] and all(s[0] for s in single[4:])   # (40 979: below one buffer)
    ns = [len(c) for c in caps]
    frames, stats = d.decode_batch_device_power([p if len(c) else 0 for c, (_, p) in zip(caps, held)], ns, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    frames, stats = d.decode_batch_power(caps, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    held4 = [to_dev(torch_cuda, c, lead=4) for c in caps]      # device captures that are only 4-byte aligned take the copy
    frames, stats = d.decode_batch_device_power([p for _, p in held4], ns, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.limit(120)
def test_refusals_leave_the_stream_as_it_was(capi, oracle, dec_factory, torch_cuda):
    """Power into a real and into an IQ stream and both the other way, a long-stream handle, a pointer 2 bytes off, NULL, 2^31
    samples: -1 with a message that names both kinds, and the stream that was in progress still finishes with its own frames."""
    a, rec = fixture_power(oracle, "iq/mixed_df_a")
    x, _ = load_iq("mixed_df_a")
    want = golden_records(rec)
    t, ptr = to_dev(torch_cuda, a)
    tx, px = to_dev(torch_cuda, x)
    n, half = len(a), len(a) // 2
    d = dec_factory(df18=True, collect_stats=True)
    real = np.full(4096, 2048, np.uint16)
    tr, pr = to_dev(torch_cuda, real)

    def refused(call, *words):
        with pytest.raises(capi.AdsbError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    d.reset()
    d.push_power(a[:half])
    refused(lambda: d.push(real), "power", "real")                                  # other kinds into a power stream
    refused(lambda: d.push_as(3, real.view(np.int16)), "power", "real")
    refused(lambda: d.push_device(pr, real.size), "power", "real")
    refused(lambda: d.push_packed(np.zeros(12, np.uint8)), "power", "real")
    refused(lambda: d.push_iq(2, x[:8]), "power", "IQ")
    refused(lambda: d.push_device_iq(0, px, 8), "power", "IQ")
    refused(lambda: d.push_device_power(ptr + 2, 8), "4-byte aligned")
    refused(lambda: d.push_power((a.ctypes.data, 1 << 31)), "2^31")
    refused(lambda: d.push_power((a.ctypes.data, (1 << 31) - half)), "2^31")       # the STREAM would reach it
    refused(lambda: d.push_device_power(ptr, 1 << 31), "2^31")
    refused(lambda: d.push_power((None, 8)), "NULL")
    refused(lambda: d.push_device_power(0, 8), "NULL")
    d.push_device_power(ptr + 4 * half, n - half)
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    # decode_device_power and the batch calls refuse before their reset: the finished stream's statistics are still there
    for call, word in ((lambda: d.decode_device_power(ptr + 2, n), "4-byte aligned"), (lambda: d.decode_device_power(ptr, 1 << 31), "2^31"),
                       (lambda: d.decode_device_power(0, n), "NULL"),
                       (lambda: d.decode_batch_device_power([ptr, ptr + 2], [n, n]), "capture 1"),
                       (lambda: d.decode_batch_device_power([ptr, 0], [n, 5]), "capture 1")):
        refused(call, word)
        assert d.stats() == rec["stats"]
    # power pushes into a real stream and into an IQ stream
    d.reset()
    d.push(real)
    refused(lambda: d.push_power(a[:half]), "real", "power")
    refused(lambda: d.push_device_power(ptr, 8), "real", "power")
    d.push(real)
    d.finish()
    assert d.drain() == []
    d.reset()
    d.push_iq(2, x[:half])
    refused(lambda: d.push_power(a[:half]), "IQ", "power")
    refused(lambda: d.push_device_power(ptr, 8, final=True), "IQ", "power")
    d.push_iq(2, x[half:])
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    # a long-stream handle takes no power samples, and stays usable for real ones
    dl = dec_factory(fresh=True, df18=True)
    dl.set_long_stream(True)
    refused(lambda: dl.push_power(a[:half]), "long-stream", "power")
    refused(lambda: dl.push_device_power(ptr, n), "long-stream", "power")
    refused(lambda: dl.decode_device_power(ptr, n), "long-stream")
    refused(lambda: dl.decode_batch_device_power([ptr], [n]), "long-stream")
    refused(lambda: dl.decode_batch_power([a]), "long-stream")
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
    a = S().iq_power(x)
    d_on, d_off = dec_factory(df18=True, fix_1bit=True), dec_factory(df18=True)
    d_on.reset()
    d_on.push_power(a)
    d_on.finish()
    buf, k = d_on.drain_raw()
    got = [(bytes(f.frame[: f.len]), int(f.reserved) & 1) for f in buf[:k]]
    assert got == [(good, 0), (orig, 1)]
    assert [abs(int(f.g) - at) <= 1 for f, at in zip(buf[:k], (5000, 20_000))] == [True, True]   # (a half-sample copy may come first)
    assert d_on.stats()["fixed"] == 1 and d_on.stats()["ok"][17] == 2
    assert [f["frame"] for f in d_off.decode_power(a)] == [good]


# ------------------------------------------------------------------ 8. the C host program
@pytest.mark.limit(120)
def test_cli_w(capi, oracle, tmp_path):
    """adsbdec_amd_cli -w -a -m -f and -b through a loopback peer: mixed_df_a's committed AVR-MLAT and Beast bytes and its Try/Ok
    table; trailing bytes that make no sample are named on stderr.  Where the compiled reference is at hand, the same file through
    its own deqframe (ref_adsbdec -a -p) gives the bytes the program writes, in all three framings."""
    from test_cli_sink import Listener
    a, rec = fixture_power(oracle, "iq/mixed_df_a")
    path = tmp_path / "mixed.pw"
    a.astype("<f4").tofile(path)
    with open(path, "ab") as f:
        f.write(b"\x01\x02\x03")
    avr = "".join(f["avr"] for f in rec["frames"]).encode()
    mlat = "".join(f["mlat"] for f in rec["frames"]).encode()
    beast = b"".join(bytes.fromhex(f["beast"]) for f in rec["frames"])
    p = subprocess.run([capi.CLI_PATH, "-w", "-a", "-m", "-f", str(path)], capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr
    assert p.stdout == mlat
    table = p.stderr.decode().splitlines()
    assert any("3 trailing bytes ignored" in ln for ln in table)
    tr = [ln for ln in table if ln.startswith("Try")][0].split()[2:]
    ok = [ln for ln in table if ln.startswith("Ok")][0].split()[2:]
    assert [int(v) for v in tr] == [rec["stats"]["try"][k] for k in (11, 17, 18)]
    assert [int(v) for v in ok] == [rec["stats"]["ok"][k] for k in (11, 17, 18)]
    lis = Listener()
    p = subprocess.run([capi.CLI_PATH, "-w", "-a", "-b", "-s", f"127.0.0.1:{lis.port}", "-f", str(path)], capture_output=True, timeout=100)
    assert p.returncode == 0, p.stderr
    assert lis.join() == beast
    p = subprocess.run([capi.CLI_PATH, "-w", "-a", "-f", str(path)], capture_output=True, timeout=100)
    assert p.returncode == 0 and p.stdout == avr, p.stderr
    for extra in (["-q", "2"], ["-t", "1"], ["-p"], ["-G", "2"], ["-B", str(tmp_path / "list.txt")]):
        r = subprocess.run([capi.CLI_PATH, "-w", *extra, "-a", "-f", str(path)], capture_output=True, timeout=100)
        assert r.returncode == 1 and b"-w is not supported with " + extra[0].encode() + b": " in r.stderr and not r.stdout, extra
    if oracle.ref_available():
        rf, rstats = oracle.ref_demod(a, df18=True)
        assert b"".join(r["avr"] for r in rf) == avr and b"".join(r["mlat"] for r in rf) == mlat and b"".join(r["beast"] for r in rf) == beast
        assert rstats == rec["stats"]
