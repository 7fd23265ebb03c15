"""The window form of the level report on the MI355X (run with -m gpu): level_windows_kernel, adsb_level_windows,
adsb_level_windows_host and the host program's -L -I.  Everything is held for EQUALITY -- counters and the 2048 bins as integers, the
envelope as uint32 -- to adsbdec_amd.levels.level_windows of the power samples Decoder.power() gives for the stream (that export is
held to the reference bit for bit elsewhere): window i is the level report of a[e[i]:e[i + 1]] with the rails of x[2 e[i] : 2 e[i + 1]],
and one envelope serves all windows.

The stream is 200 740 samples of noise: 100 370 power samples, 56 whole passes of 1792 and a last run of 18.  Codes 0, 4095 and 5000
stand at the last sample of windows and the first of the next, and one very large sample on each side of an edge: a window that
counted a neighbour's code, or took silence where the stream has samples, shows.  A second stream has n % 4 == 2 and the trailing
codes 0 and 4095, which belong to no window."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, golden_records, load_golden, records
from test_gpu_iq import to_dev
from test_gpu_level import COUNTERS, GUARD, SENT, LV, dev_env, parse_cli
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT64 = 0xA5A5A5A5A5A5A5A5
N = 200_740
M = 100_370
PASS = 1792


def same(got, want, how):
    for key in COUNTERS:
        assert got[key] == want[key], (how, key, got[key], want[key])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), (how, np.flatnonzero(got["hist"] != want["hist"])[:8])
    assert int(got["hist"].sum()) + got["negative"] == got["samples"], how


def total(reports):
    t = LV().zero_report()
    for r in reports:
        t = LV().add(t, r)
    return t


@pytest.fixture(scope="module")
def work(capi, dec_factory, torch_cuda):
    """The two streams, their power samples (computed once, never changed) and the first stream on the device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_signal
    x, _ = gen_signal.dense_capture(N, seed=27)
    assert x.size == N and N % 4 == 0 and 2 * (N // 4) == M == 56 * PASS + 18
    codes = (0, 4095, 5000)
    for j, e in enumerate(range(PASS, M, PASS)):                            # the edges of the windows of 1792: multiples of 28 too
        if j % 3 != 2:
            x[2 * e - 1], x[2 * e] = codes[j % 3], codes[(j + 1) % 3]        # the last sample of a window, the first of the next
    x[2 * (7 * PASS) - 1] = 65535                                           # one very large sample on each side of an edge:
    x[2 * (9 * PASS)] = 65535                                               # ... each reaches six power samples further
    x[2 * (28 * 1201) - 1], x[2 * (28 * 1201)] = 0, 65000                   # an edge of the windows of 28 that is no pass's
    n2 = 4 * 3593 + 2
    y, _ = gen_signal.dense_capture(n2, seed=28)
    y[1], y[n2 // 2] = 0, 4095
    y[-2:] = (0, 4095)                                                      # the trailing n % 4 codes
    d = dec_factory()
    a, b = d.power(x), d.power(y)
    assert a.size == M and b.size == 2 * (n2 // 4) and a.dtype == np.float32
    a.setflags(write=False), b.setflags(write=False), x.setflags(write=False), y.setflags(write=False)
    t, ptr = to_dev(torch_cuda, x)
    return dict(x=x, a=a, y=y, b=b, t=t, ptr=ptr)


WANT = {}   # the statement of a partition of the first stream, computed once


def hold(torch, d, ptr, first_sample, n, edges, a, x, how, host=None, key=None):
    """One device call (and, with host = the buffer's samples, one host call) against the statement: every report, their sum, the
    shared envelope bit for bit, and the floats behind the envelope untouched.  key: a name under which the statement is kept."""
    if key is None or key not in WANT:
        WANT[key] = LV().level_windows(a, x, edges)
    want, want_env = WANT[key]
    te, pe, k = dev_env(torch, edges[-1] - edges[0])
    assert k == want_env.size
    got = d.level_windows(ptr, first_sample, n, edges, pe if k else 0, k)
    assert len(got) == len(edges) - 1
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, (how, "window", i, edges[i], edges[i + 1]))
    same(total(got), LV().level_windows(a, x, [edges[0], edges[-1]])[0][0], (how, "the sum"))
    e = te.cpu().numpy().view(np.uint32)
    assert np.array_equal(e[:k], want_env.view(np.uint32)), (how, "envelope", np.flatnonzero(e[:k] != want_env.view(np.uint32))[:8])
    assert (e[k:] == SENT).all(), (how, "behind the envelope")
    for g, w in zip(d.level_windows(ptr, first_sample, n, edges), want):     # device_env == NULL
        same(g, w, (how, "no envelope"))
    if host is not None:
        reports, env = d.level_windows_host(host, first_sample, edges)
        for i, (g, w) in enumerate(zip(reports, want)):
            same(g, w, (how, "host, window", i))
        assert env.dtype == np.float32 and np.array_equal(env.view(np.uint32), want_env.view(np.uint32)), (how, "host envelope")
    return got


# ------------------------------------------------------------------ 1. one window over the whole stream
@pytest.mark.limit(60)
def test_one_window_over_the_whole_stream(capi, dec_factory, torch_cuda, work):
    d = dec_factory()
    x, a = work["x"], work["a"]
    te, pe, k = dev_env(torch_cuda, M)
    single = d.level_device(work["ptr"], N, pe, k)
    env_single = te.cpu().numpy().view(np.uint32)[:k]
    got = hold(torch_cuda, d, work["ptr"], 0, N, [0, M], a, x, "n % 4 == 0", host=x)
    same(got[0], single, "against adsb_level_device")
    te2, pe2, _ = dev_env(torch_cuda, M)
    same(d.level_windows(work["ptr"], 0, N, [0, M], pe2, k)[0], single, "again")
    assert np.array_equal(te2.cpu().numpy().view(np.uint32)[:k], env_single)
    reports, env = d.level_windows_host(x, 0, [0, M])
    same(reports[0], single, "the host call against adsb_level_device")
    assert np.array_equal(env.view(np.uint32), env_single)
    # trailing codes: everything the single call reports but the two codes no window owns
    y, b = work["y"], work["b"]
    t, ptr = to_dev(torch_cuda, y)
    alone = d.level_device(ptr, y.size)
    got = hold(torch_cuda, d, ptr, 0, y.size, [0, b.size], b, y, "n % 4 == 2", host=y)[0]
    assert (got["rail_lo"], got["rail_hi"], got["over"]) == (alone["rail_lo"] - 1, alone["rail_hi"] - 1, alone["over"])
    assert got["rail_lo"] >= 1 and got["rail_hi"] >= 1
    assert got["samples"] == alone["samples"] and got["negative"] == alone["negative"] and np.array_equal(got["hist"], alone["hist"])


# ------------------------------------------------------------------ 2. partitions
def partitions():
    rng = np.random.default_rng(2700)
    inner = 28 * np.sort(rng.integers(10, M // 28 + 1, size=299))
    inner[40:44] = inner[40]                                                # empty windows among them, for certain
    ragged = [28 * 100] + [28 * 100 + PASS * k + 28 * (k % 3) for k in range(1, 20)] + [28 * 100 + PASS * 20 + 13]
    return {"28": list(range(0, M, 28)) + [M], "1792": list(range(0, M, PASS)) + [M],
            "random": [280] + [int(v) for v in inner] + [M], "ragged": ragged,
            "1025 of 28": [56 + 28 * i for i in range(1026)]}


@pytest.mark.limit(60)
@pytest.mark.parametrize("blocks", (0, 1, 2))
def test_partitions(capi, dec_factory, torch_cuda, work, blocks):
    """All windows of 28 (3585 of them: four sub-launches), windows of 1792, 300 random multiples of 28 with empty windows among them, a
    last edge that is no multiple of 28, and 1025 windows of 28 over 28 700 power samples (a sub-launch of 1024 and one of one) -- on
    the default grid and on one and two workgroups, where one wave crosses many windows and flushes at each."""
    d = dec_factory()
    x, a = work["x"], work["a"]
    parts = partitions()
    assert len(parts["28"]) - 1 == 3585 and parts["28"][-1] % 28 == 18 and len(parts["random"]) - 1 == 300 and parts["ragged"][-1] % 28 == 13
    assert len(parts["1025 of 28"]) - 1 == 1025 and parts["1025 of 28"][-1] - parts["1025 of 28"][0] == 28_700
    assert any(p == q for p, q in zip(parts["random"], parts["random"][1:]))
    d.set_level_batch_blocks(blocks)
    try:
        for name, edges in parts.items():
            got = hold(torch_cuda, d, work["ptr"], 0, N, edges, a, x, (name, blocks), host=x if blocks == 0 and name != "28" else None, key=name)
            if name == "1792":                                              # the planted codes count for the window that owns them
                assert got[0]["rail_lo"] >= 1 and got[1]["rail_hi"] >= 1 and sum(g["over"] for g in got) >= 20
    finally:
        d.set_level_batch_blocks(0)


# ------------------------------------------------------------------ 3. history: the six older pairs
@pytest.mark.limit(60)
def test_a_buffer_that_starts_mid_stream(capi, dec_factory, torch_cuda, work):
    """first_sample = 2 e[0] - 16 (all six older pairs held), - 8 (four) and - 0 (none): the statement with x[:first_sample] = 2048.  The
    buffer lies inside the stream's own allocation, so the samples in front of it are the stream's: read, they would not be silence."""
    d = dec_factory()
    x, a = work["x"], work["a"]
    e0 = 7 * PASS                                                           # (the very large sample stands right in front of it)
    edges = [e0, e0 + 28, e0 + 56, e0 + 2 * PASS, e0 + 2 * PASS, e0 + 5 * PASS + 28 * 3 + 5]
    n_end = 2 * edges[-1]                                                   # the buffer ends with the last window's last pair
    whole = LV().level_windows(a, x, edges)[0]
    for back in (16, 8, 0):
        fs = 2 * e0 - back
        xx = x.copy()
        xx[:fs] = 2048
        aa = d.power(xx)
        assert np.array_equal(aa[e0 + 6:].view(np.uint32), a[e0 + 6:].view(np.uint32))
        assert (back == 16) == np.array_equal(aa[e0:e0 + 6].view(np.uint32), a[e0:e0 + 6].view(np.uint32))   # (silence there shows)
        got = hold(torch_cuda, d, work["ptr"] + 2 * fs, fs, n_end - fs, edges, aa, xx, ("history", back), host=x[fs:n_end])
        if back == 16:
            for g, w in zip(got, whole):
                same(g, w, "all six pairs held: the whole stream's slices")


# ------------------------------------------------------------------ 4. nothing outside the buffer is read
@pytest.mark.limit(60)
@pytest.mark.parametrize("blocks", (0, 1))
def test_guarded_by_a_decoy(capi, dec_factory, torch_cuda, work, blocks):
    """The buffer between stretches of a loud decoy capture (both rails and codes above them), as tests/test_gpu_guarded.py places its
    pieces: nothing outside [first_sample, first_sample + n) may change a report, in front of the buffer or behind it."""
    d = dec_factory()
    x, a = work["x"], work["a"]
    rng = np.random.default_rng(2704)
    guard = 4096
    d.set_level_batch_blocks(blocks)
    try:
        for e0, eK, back in ((3 * PASS, 6 * PASS + 28 * 2 + 7, 0), (28 * 65, 28 * 65 + 28 * 300, 8), (PASS, 4 * PASS, 16), (0, 2 * PASS + 3, 0)):
            fs, n_end = 2 * e0 - back, 2 * eK
            decoy = rng.choice(np.array([0, 4095, 65535, 5000, 1], np.uint16), size=2 * guard + n_end - fs)
            decoy[guard:guard + n_end - fs] = x[fs:n_end]
            t, p = to_dev(torch_cuda, decoy)
            xx = x.copy()
            xx[:fs] = 2048
            aa = d.power(xx)
            step = 28 * 23
            edges = list(range(e0, eK, step)) + [eK]
            hold(torch_cuda, d, p + 2 * guard, fs, n_end - fs, edges, aa, xx, ("decoy", e0, eK, back, blocks))
    finally:
        d.set_level_batch_blocks(0)


# ------------------------------------------------------------------ 5. between the pushes of a stream
@pytest.mark.limit(60)
def test_between_two_pushes(capi, dec_factory, torch_cuda, work):
    x, rec = load_golden("config1_1Mi_100xDF17")
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    d.reset()
    half = x.size // 2 + 3
    d.push(x[:half])
    edges = [PASS * k for k in range(0, 30, 3)]
    hold(torch_cuda, d, work["ptr"], 0, N, edges, work["a"], work["x"], "between two pushes", host=work["x"])
    d.push(x[half:])
    d.finish()
    assert records(d.drain()) == golden_records(rec)
    assert d.stats() == rec["stats"]


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.limit(60)
def test_refusals_write_nothing(capi, dec_factory, torch_cuda, work):
    """Every refusal once: -1, a message that names the reason and, where one is at fault, the window; every word of out[] and every
    envelope float as it was, the format report as it was -- and the next valid call succeeds.  None of these reaches a launch."""
    d = dec_factory()
    d.reset()
    x, a, ptr = work["x"], work["a"], work["ptr"]
    before = d.format_report()
    te, pe, k = dev_env(torch_cuda, 3 * PASS)
    out = (capi.LevelReport * 3)()
    C.memset(C.addressof(out), 0xA5, C.sizeof(out))
    words = np.ctypeslib.as_array((C.c_uint64 * (3 * (5 + 2048))).from_buffer(out))
    henv = np.full(k, SENT, np.uint32)
    E = [PASS, 2 * PASS, 3 * PASS, 4 * PASS]
    fs, n = 2 * PASS - 16, 2 * 3 * PASS + 16
    p = ptr + 2 * fs
    arr = lambda vals: (C.c_uint64 * len(vals))(*vals)
    W = lambda *args, **kw: d.level_windows(*args, out=out, **kw)

    def raw(name, *args):
        if getattr(capi.load(), name)(d._h, *args) < 0:
            d._check(-1, name)

    def host(edges, first=fs, buf=x[fs:fs + n], env=henv, cap=None):
        raw("adsb_level_windows_host", buf.ctypes.data if buf is not None else None, first, n, len(edges) - 1, arr(edges), out,
            env.ctypes.data if env is not None else None, k if cap is None else cap)

    long_d = dec_factory(fresh=True)
    long_d.set_long_stream(True)
    cases = [
        ("", "multiple of 8 samples", lambda: W(p + 8, fs + 4, n - 4, E, pe, k)),
        ("", "16-byte aligned", lambda: W(p + 8, fs, n, E, pe, k)),
        ("window 2", "multiple of 28", lambda: W(p, fs, n, [PASS, 2 * PASS, 2 * PASS + 14, 4 * PASS], pe, k)),
        ("window 0", "multiple of 28", lambda: W(p, fs, n, [PASS + 1, 2 * PASS, 3 * PASS, 4 * PASS], pe, k)),
        ("window 1", "ascend", lambda: W(p, fs, n, [2 * PASS, 3 * PASS, 2 * PASS, 4 * PASS], pe, k)),
        ("window 0", "own pair", lambda: W(p, fs, n, [PASS - 28] + E[1:], pe, k)),
        ("last window", "own pair", lambda: W(p, fs, n, E[:3] + [4 * PASS + 1], pe, k)),
        ("last window", "own pair", lambda: W(p, fs, n, E[:3] + [(1 << 31) + 1], pe, k)),
        ("", "2^32", lambda: W(p, (1 << 32) - 64, 64, E, pe, k)),
        ("", "2^32", lambda: W(p, fs, 1 << 32, E, pe, k)),
        ("", "2^32", lambda: long_d.level_windows(p, (1 << 32) - 64, 64, E, pe, k, out=out)),
        ("", "NULL edges", lambda: raw("adsb_level_windows", p, fs, n, 3, None, out, pe, k)),
        ("", "NULL reports", lambda: raw("adsb_level_windows", p, fs, n, 3, arr(E), None, pe, k)),
        ("", "NULL buffer", lambda: W(0, fs, n, E, pe, k)),
        ("", "envelope must be 4-byte aligned", lambda: W(p, fs, n, E, pe + 2, k)),
        ("", "the array holds", lambda: W(p, fs, n, E, pe, 3 * 64 - 1)),
        ("", "NULL envelope", lambda: raw("adsb_level_windows", p, fs, n, 3, arr(E), out, None, k)),
        ("windows", "32 bits", lambda: raw("adsb_level_windows", p, fs, n, (1 << 32) - 1, arr(E), out, pe, k)),
        ("", "multiple of 8 samples", lambda: host(E, first=fs + 4)),
        ("window 1", "multiple of 28", lambda: host([PASS, PASS + 5, 3 * PASS, 4 * PASS])),
        ("window 2", "ascend", lambda: host([PASS, 3 * PASS, 3 * PASS, 2 * PASS])),
        ("window 0", "own pair", lambda: host([PASS - 28] + E[1:])),
        ("last window", "own pair", lambda: host(E[:3] + [4 * PASS + 28])),
        ("", "2^32", lambda: host(E, first=(1 << 32) - 8)),
        ("", "NULL buffer", lambda: host(E, buf=None)),
        ("", "the array holds", lambda: host(E, cap=k - 1)),
        ("", "NULL envelope", lambda: host(E, env=None)),
        ("", "NULL edges", lambda: raw("adsb_level_windows_host", x[fs:].ctypes.data, fs, n, 3, None, out, None, 0)),
        ("", "NULL reports", lambda: raw("adsb_level_windows_host", x[fs:].ctypes.data, fs, n, 3, arr(E), None, None, 0)),
        ("windows", "32 bits", lambda: raw("adsb_level_windows_host", x[fs:].ctypes.data, fs, n, (1 << 32) - 1, arr(E), out, None, 0)),
    ]
    for who, why, call in cases:
        with pytest.raises(capi.AdsbError) as e:
            call()
        assert who in str(e.value) and why in str(e.value), (who, why, str(e.value))
        assert (words == SENT64).all(), (who, why)
        assert (te.cpu().numpy().view(np.uint32) == SENT).all() and (henv == SENT).all(), (who, why)
        assert d.format_report() == before, (who, why)
    long_d.close()
    # no windows: 0, nothing launched or written; empty windows: zeroed reports, NULL samples allowed; and the handle still works
    assert capi.load().adsb_level_windows(d._h, None, 0, 0, 0, arr([0]), out, None, 0) == 0 and (words == SENT64).all()
    assert capi.load().adsb_level_windows_host(d._h, None, 0, 0, 0, arr([0]), out, None, 0) == 0 and (words == SENT64).all()
    got = W(0, 0, 0, [0, 0, 0, 0])
    assert all(g[key] == 0 for g in got for key in COUNTERS) and not any(g["hist"].any() for g in got) and not words.any()
    C.memset(C.addressof(out), 0xA5, C.sizeof(out))
    raw("adsb_level_windows_host", None, fs, n, 3, arr([PASS, PASS, PASS, PASS]), out, None, 0)
    assert not words.any() and (te.cpu().numpy().view(np.uint32) == SENT).all()
    xx = x.copy()
    xx[:fs] = 2048
    hold(torch_cuda, d, p, fs, n, E, d.power(xx), xx, "after the refusals", host=x[fs:fs + n])
    assert d.format_report() == before


# ------------------------------------------------------------------ 7. the host program
def parse_windows(text):
    """-L -I's output -> ([(start seconds, [median, p99.9, peak] in dB, (rail_lo, rail_hi, over))], the closing report's text)"""
    lines = text.splitlines()
    rows = []
    while lines and lines[0].startswith("t "):
        w = lines.pop(0).split()
        assert w[2] == "s" and w[3::3][:3] == ["median", "p99.9", "peak"] and w[5::3][:3] == ["dB"] * 3 and w[12::2] == ["rail_lo", "rail_hi", "over"], w
        rows.append((float(w[1]), [float(v) for v in w[4::3][:3]], tuple(int(v) for v in w[13::2])))
    return rows, "\n".join(lines) + "\n"


@pytest.mark.limit(120)
def test_host_program(capi, work, tmp_path):
    """-L -I 1 on the stream as a file and as a FIFO fed with the same bytes, whole and in pieces of three windows: a line per window
    of 9996 power samples (10 000 rounded down to a multiple of 28) -- start, the three bins in dB of raw power units, the window's
    rails -- and -L's own report of the sum, which for this stream (n % 4 == 0) is plain -L's output byte for byte."""
    x, a = work["x"], work["a"]
    path, fifo = tmp_path / "capture.bin", tmp_path / "capture.fifo"
    data = x.tobytes() + b"\x07"
    path.write_bytes(data)
    plain = subprocess.run([capi.CLI_PATH, "-L", "-f", str(path)], capture_output=True, timeout=100)
    assert plain.returncode == 0, plain.stderr
    whole, _ = parse_cli(plain.stdout.decode())
    want_whole = LV().with_rails(LV().level_report(a), x, "real")
    same(dict(whole, hist=whole["hist"].astype(np.uint64)), want_whole, "plain -L")
    win = 9996
    edges = list(range(0, M, win)) + [M]
    want, _ = LV().level_windows(a, x, edges)
    assert len(want) == 11
    os.mkfifo(fifo)

    def feed():
        with open(fifo, "wb") as f:
            for at in range(0, len(data), 50_001):                          # (pieces that are no multiple of anything)
                f.write(data[at:at + 50_001])

    for source, piece in ((path, None), (path, "3"), (fifo, None), (fifo, "3")):
        env = dict(os.environ)
        if piece:
            env["ADSB_CLI_LEVEL_PIECE"] = piece
        th = threading.Thread(target=feed) if source is fifo else None
        if th:
            th.start()
        p = subprocess.run([capi.CLI_PATH, "-L", "-I", "1", "-f", str(source)], capture_output=True, timeout=100, env=env)
        if th:
            th.join()
        assert p.returncode == 0, p.stderr
        assert b"1 trailing bytes ignored" in p.stderr, p.stderr
        rows, closing = parse_windows(p.stdout.decode())
        assert len(rows) == len(want), (source.name, piece, len(rows))
        for i, ((t0, db, rails), w) in enumerate(zip(rows, want)):
            assert abs(t0 - edges[i] / 1e7) < 1e-6, (i, t0)
            assert rails == (w["rail_lo"], w["rail_hi"], w["over"]), (source.name, piece, i)
            bins = [LV().percentile(w["hist"], 0.5), LV().percentile(w["hist"], 0.999), LV().bin_lower_edge(int(np.flatnonzero(w["hist"])[-1]))]
            for have, edge in zip(db, bins):
                assert abs(have - 10 * np.log10(edge)) <= 0.006, (source.name, piece, i, have, edge)   # (printed with two decimals)
        assert closing == plain.stdout.decode(), (source.name, piece)
