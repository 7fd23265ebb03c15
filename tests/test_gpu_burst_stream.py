"""The gate of a slice of a stream on the MI355X (run with -m gpu): burst_slice_kernel.hip's launches and adsb_bursts_slice_*, held for
EQUALITY to the numpy statements: the records of consecutive calls, concatenated, are adsbdec_amd.levels.bursts of the whole envelope
-- begin, end, hot and the peak's bits, record for record -- and every call's table and carry are levels.bursts_slice's.  One
envelope of R = 2 T + 300 runs (two tile seams, a wave's tail) with tests/burst_cases.py's seam patterns, cut in two at EVERY run;
300 random cases in 1 to 5 slices; cuts aimed at a lead zone, a cluster's inside, a hang zone and the two sides of e + join; a table
shorter than B against poison and the repeat; in == out; empty slices; every refusal; adsb_level_windows at two bases;
adsb_bursts_device, whose tables must not have moved; and the host program's record mode, -S -O, whose archive is
burst_archive.record_statement's and -L -U -K's byte for byte at every piece, from a file and from a FIFO."""
import os
import subprocess
import threading

import numpy as np
import pytest

import burst_cases as BC
from test_gpu_bursts import POISON, same
from test_gpu_iq import to_dev
from test_gpu_power import dec_factory, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LEAD, HANG = 2, 4
JOIN = LEAD + HANG + 1


def LV():
    from adsbdec_amd import levels
    return levels


@pytest.fixture(scope="module")
def T(capi):
    return capi.burst_tile_runs()


def seam_envelope(T):
    """R = 2 T + 300 runs with burst_cases.named_cases' patterns at both seams (lead 2, hang 4): run 0 and run R - 1 hot; T - 1 and T,
    one burst across the seam; T - 1 + join, joined; then one more than join further on, split; 2 T - 1 and 2 T + join, split; a dense
    stretch and a sprinkle."""
    R = 2 * T + 300
    hot = {0, 3, 40, T - 5, T - 1, T, T - 1 + JOIN, T + 2 * JOIN, 2 * T - 1, 2 * T + JOIN, 2 * T + 100, R - 1}
    hot |= set(range(T + 500, T + 640))                                            # more than a wave's lanes of one burst
    rng = np.random.default_rng(21)
    hot |= {int(v) for v in np.flatnonzero(rng.random(R) < 0.01)}
    return BC.envelope(R, sorted(hot), 5)


@pytest.fixture(scope="module")
def seam(torch_cuda, T):
    env = seam_envelope(T)
    want = LV().bursts(env, BC.THRESHOLD, LEAD, HANG)
    assert env.size == 2 * T + 300 and want.size > 20 and want["begin"][0] == 0 and want["end"][-1] == env.size
    t, ptr = to_dev(torch_cuda, env)
    return dict(env=env, want=want, t=t, ptr=ptr)


def stream(d, ptr, env, edges, threshold, lead, hang, check_each=True, room=8):
    """The envelope at ptr through adsb_bursts_slice_device slice by slice, slice i the runs [edges[i], edges[i + 1]) -- views into the
    one device array -- the last call final -> the concatenated records.  Every call's table, B and carry are the statement's."""
    carry, want_carry = LV().burst_carry(), LV().burst_carry()
    recs = []
    for i in range(len(edges) - 1):
        lo, hi = int(edges[i]), int(edges[i + 1])
        final = i == len(edges) - 2
        want, want_carry = LV().bursts_slice(env[lo:hi], threshold, lead, hang, want_carry, final)
        got, b, carry = d.bursts_slice_device(ptr + 4 * lo if hi > lo else 0, hi - lo, threshold, lead, hang, carry, final, want.size + room)
        if check_each:
            assert b == want.size, (edges, i, b, want.size)
            same(got, want, (edges, i))
            assert carry.tobytes() == want_carry.tobytes(), (edges, i, carry, want_carry)
        recs.append(got.copy())
    assert not carry["open"][0] and carry["runs"][0] == env.size
    return np.concatenate(recs)


# ------------------------------------------------------------------ 1. every cut
@pytest.mark.limit(60)
def test_two_slices_at_every_cut(capi, dec_factory, seam):
    """The seam envelope as two slices, cut at every run 0 .. R: the second slice starts 0, 1, 2 and 3 floats behind a 16-byte boundary
    in turn.  Each cut's records are levels.bursts of the whole, compared as bytes."""
    d = dec_factory()
    env, ptr, whole = seam["env"], seam["ptr"], seam["want"].tobytes()
    R = env.size
    table, carry = np.zeros(seam["want"].size + 8, dtype=LV().BURST_DTYPE), LV().burst_carry()
    bad = []
    for cut in range(R + 1):
        carry[:] = 0
        a, b1, _ = d.bursts_slice_device(ptr if cut else 0, cut, BC.THRESHOLD, LEAD, HANG, carry, False, table.size, table=table, out=carry)
        first = a.tobytes()
        assert carry["runs"][0] == cut
        c, b2, _ = d.bursts_slice_device(ptr + 4 * cut if cut < R else 0, R - cut, BC.THRESHOLD, LEAD, HANG, carry, True, table.size, table=table, out=carry)
        if first + c.tobytes() != whole or b1 + b2 != seam["want"].size or carry["open"][0]:
            bad.append(cut)
    assert not bad, bad[:20]
    # three of the cuts call by call against the statement, carry included
    for cut in (seam["env"].size // 2, capi.burst_tile_runs() - 1 + 3, 1):
        same(stream(d, ptr, env, [0, cut, R], BC.THRESHOLD, LEAD, HANG), seam["want"], cut)


# ------------------------------------------------------------------ 2. random cases and aimed cuts
def aimed_cuts(want, lead, hang, R, rng):
    """Cuts inside a burst's lead zone, between two hot runs of a cluster, inside the hang zone, at e + join and e + join + 1, where the
    table has such places (s and e from a table that is not clipped there)."""
    join, cuts = lead + hang + 1, []
    for b in want[rng.permutation(want.size)[:3]]:
        s, e = int(b["begin"]) + lead, int(b["end"]) - hang - 1
        cuts += [s - lead + 1, (s + e) // 2 + 1, e + 2, e + join, e + join + 1]
    return sorted({c for c in cuts if 0 <= c <= R})


@pytest.mark.limit(60)
def test_random_cases_in_one_to_five_slices(capi, dec_factory, torch_cuda, T):
    d = dec_factory()
    rng = np.random.default_rng(22)
    for i in range(300):
        R = int(rng.integers(0, 3 * T)) if i % 3 else int(rng.integers(0, 200))
        density = float(rng.choice([0.0, 0.002, 0.02, 0.2, 0.9]))
        lead, hang = (1468, 1468) if i == 7 else (int(rng.integers(0, 7)), int(rng.integers(0, 7)))
        env = BC.envelope(R, np.flatnonzero(rng.random(R) < density), i)
        want = LV().bursts(env, BC.THRESHOLD, lead, hang)
        k = int(rng.integers(1, 6))
        cuts = sorted(int(v) for v in rng.integers(0, R + 1, k - 1))
        if i % 2 and want.size:
            cuts = aimed_cuts(want, lead, hang, R, rng)[:4]
        t, ptr = to_dev(torch_cuda, env, lead=4 * (i % 4))
        same(stream(d, ptr, env, [0, *cuts, R], BC.THRESHOLD, lead, hang), want, (i, R, lead, hang, cuts))


@pytest.mark.limit(60)
def test_cuts_aimed_at_the_zones_of_a_burst(capi, dec_factory, seam):
    """Around one cluster of the seam envelope: every cut from its lead zone to two runs past e + join + 1, as the middle of three
    slices; and lead / hang that change from call to call, against the statement call by call."""
    d = dec_factory()
    env, ptr, want = seam["env"], seam["ptr"], seam["want"]
    R = env.size
    k = int(np.flatnonzero(want["hot"] > 100)[0])                                    # the dense stretch: s = T + 500
    s, e = int(want["begin"][k]) + LEAD, int(want["end"][k]) - HANG - 1
    for cut in [*range(s - LEAD - 2, s + 3), (s + e) // 2, *range(e, e + JOIN + 4)]:
        same(stream(d, ptr, env, [0, s - 40, cut, R], BC.THRESHOLD, LEAD, HANG), want, cut)
    rng = np.random.default_rng(23)
    carry, want_carry = LV().burst_carry(), LV().burst_carry()
    edges = [0, *sorted(int(v) for v in rng.integers(0, R + 1, 11)), R]
    for i in range(12):
        lo, hi, lead, hang = edges[i], edges[i + 1], int(rng.integers(0, 7)), int(rng.integers(0, 7))
        w, want_carry = LV().bursts_slice(env[lo:hi], BC.THRESHOLD, lead, hang, want_carry, i == 11)
        got, b, carry = d.bursts_slice_device(ptr + 4 * lo if hi > lo else 0, hi - lo, BC.THRESHOLD, lead, hang, carry, i == 11, w.size + 4)
        assert b == w.size
        same(got, w, (i, lead, hang))
        assert carry.tobytes() == want_carry.tobytes(), i


# ------------------------------------------------------------------ 3. cap and carry
@pytest.mark.limit(60)
def test_a_table_shorter_than_b_and_the_repeat(capi, dec_factory, seam):
    """cap below B against poison: nothing at or behind cap, the return value and the carry out are those of a call with room, and the
    same call again with the same carry in gives every record.  in == out."""
    d = dec_factory()
    env, ptr = seam["env"], seam["ptr"]
    R, cut = env.size, capi.burst_tile_runs() + 520                                   # inside the dense stretch: the carry is open
    first, carry_in = LV().bursts_slice(env[:cut], BC.THRESHOLD, LEAD, HANG, LV().burst_carry(), False)
    assert carry_in["open"][0] and first.size > 4
    for lo, hi, cin, final in ((0, cut, LV().burst_carry(), False), (cut, R, carry_in, True), (cut, R, carry_in, False)):
        want, want_carry = LV().bursts_slice(env[lo:hi], BC.THRESHOLD, LEAD, HANG, cin, final)
        B = want.size
        for cap in (0, 1, B // 2, B - 1, B):
            table = np.frombuffer(bytearray([POISON]) * (16 * (B + 4)), dtype=LV().BURST_DTYPE)
            keep = cin.copy()
            got, b, out = d.bursts_slice_device(ptr + 4 * lo, hi - lo, BC.THRESHOLD, LEAD, HANG, cin, final, cap, table=table if cap else None)
            assert b == B and got.size == cap and (cin == keep).all()
            same(got, want[:cap], (lo, cap))
            assert (table[cap:].view(np.uint8) == POISON).all(), (lo, cap)
            assert out.tobytes() == want_carry.tobytes(), (lo, cap)
        # in == out: the carry array is read before it is written
        both = cin.copy()
        got, b, out = d.bursts_slice_device(ptr + 4 * lo, hi - lo, BC.THRESHOLD, LEAD, HANG, both, final, B, out=both)
        assert out is both and both.tobytes() == want_carry.tobytes() and b == B
        same(got, want, "in == out")
    # the host form, its table grown by the second call
    name, aenv, threshold, lead, hang = BC.alternating(capi.burst_tile_runs())
    got, b, out = d.bursts_slice_host(aenv, threshold, lead, hang, LV().burst_carry(), True)
    assert b > 1024
    same(got, LV().bursts(aenv, threshold, lead, hang), name)


# ------------------------------------------------------------------ 4. finals and refusals
@pytest.mark.limit(60)
def test_empty_slices_finals_and_every_refusal(capi, dec_factory, torch_cuda, seam):
    import ctypes as C
    d = dec_factory()
    LVm = LV()
    env, ptr = seam["env"], seam["ptr"]
    zero = LVm.burst_carry()
    # empty slices: without final the carry goes through, with it the carried cluster closes -- nothing is launched (NULL envelope)
    open_carry = LVm.burst_carry()
    open_carry["runs"], open_carry["open"], open_carry["first"], open_carry["last"], open_carry["hot"], open_carry["peak"] = 1000, 1, 990, 997, 5, 321.5
    for cin in (zero, open_carry):
        for final in (False, True):
            want, want_carry = LVm.bursts_slice(np.zeros(0, "<f4"), BC.THRESHOLD, LEAD, HANG, cin, final)
            got, b, out = d.bursts_slice_device(0, 0, BC.THRESHOLD, LEAD, HANG, cin, final, 4)
            assert b == want.size == (1 if final and cin["open"][0] else 0)
            same(got, want, ("empty", final))
            assert out.tobytes() == want_carry.tobytes()
            got, b, out = d.bursts_slice_host(np.zeros(0, "<f4"), BC.THRESHOLD, LEAD, HANG, cin, final, cap=4)
            assert b == want.size and out.tobytes() == want_carry.tobytes()
    # a final call over runs that are not hot closes only the carried cluster, clipped to the stream's end
    quiet = np.zeros(3, "<f4")
    tq, pq = to_dev(torch_cuda, quiet)
    want, want_carry = LVm.bursts_slice(quiet, BC.THRESHOLD, LEAD, HANG, open_carry, True)
    got, b, out = d.bursts_slice_device(pq, 3, BC.THRESHOLD, LEAD, HANG, open_carry, True, 4)
    assert b == 1 and int(want["begin"][0]) == 988 and int(want["end"][0]) == 1002 and int(want["hot"][0]) == 5
    same(got, want, "final closes the carried cluster")
    assert out.tobytes() == want_carry.tobytes()
    # every refusal: -1 with its message, neither the table nor the carry out touched, the handle usable afterwards
    L, h = d._L, d._h
    table = np.full(16 * 8, POISON, np.uint8)
    out = np.full(32, POISON, np.uint8)
    tp, op = table.ctypes.data, out.ctypes.data

    def crafted(**kw):
        c = LVm.burst_carry()
        for k, v in kw.items():
            c[k] = v
        return c
    ok = zero
    long_stream = crafted(runs=(1 << 31) - 5)
    refusals = ((0, 5, BC.THRESHOLD, LEAD, HANG, ok, tp, 8, op, "NULL envelope"),
                (ptr + 2, 5, BC.THRESHOLD, LEAD, HANG, ok, tp, 8, op, "4-byte aligned"),
                (ptr, 1 << 31, BC.THRESHOLD, LEAD, HANG, ok, tp, 8, op, "2^31"),
                (ptr, 64, float("nan"), LEAD, HANG, ok, tp, 8, op, "threshold"),
                (ptr, 64, -0.0, LEAD, HANG, ok, tp, 8, op, "threshold"),
                (ptr, 64, BC.THRESHOLD, (1 << 30) + 1, HANG, ok, tp, 8, op, "2^30"),
                (ptr, 64, BC.THRESHOLD, LEAD, (1 << 30) + 1, ok, tp, 8, op, "2^30"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, ok, 0, 8, op, "NULL table"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, None, tp, 8, op, "NULL carry"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, ok, tp, 8, 0, "NULL carry"),
                (ptr, 5, BC.THRESHOLD, LEAD, HANG, long_stream, tp, 8, op, "2^31 runs"),
                (0, 0, BC.THRESHOLD, LEAD, HANG, crafted(runs=1 << 31), tp, 8, op, "2^31 runs"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, crafted(runs=100, open=1, first=50, last=40, hot=3), tp, 8, op, "open carry"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, crafted(runs=100, open=1, first=50, last=100, hot=3), tp, 8, op, "open carry"),
                (ptr, 64, BC.THRESHOLD, LEAD, HANG, crafted(runs=100, open=1, first=50, last=60, hot=0), tp, 8, op, "open carry"),
                (0, 0, BC.THRESHOLD, LEAD, HANG, crafted(runs=0, open=1, first=0, last=0, hot=1), tp, 8, op, "open carry"))
    for fn in (L.adsb_bursts_slice_device, L.adsb_bursts_slice_host):
        host = fn is L.adsb_bursts_slice_host
        for p, n, th, le, ha, cin, tab, cap, o, word in refusals:
            if host and p:
                p = env.ctypes.data + (p - ptr)
            for final in (0, 1):
                assert fn(h, p or None, n, th, le, ha, cin.ctypes.data if cin is not None else None, final, tab or None, cap, o or None) == -1, (host, word)
                assert word in L.adsb_last_error(h).decode(), (word, L.adsb_last_error(h))
                assert (table == POISON).all() and (out == POISON).all(), word
    assert L.adsb_bursts_slice_device(None, None, 0, 1.0, 0, 0, zero.ctypes.data, 0, None, 0, op) == -1 and (out == POISON).all()
    # the last run the limit leaves: a stream of 2^31 - 1 runs, its last five from this envelope
    five = BC.envelope(5, [1, 4])
    t5, p5 = to_dev(torch_cuda, five)
    cin = crafted(runs=(1 << 31) - 6)
    want, want_carry = LVm.bursts_slice(five, BC.THRESHOLD, LEAD, HANG, cin, True)
    got, b, o = d.bursts_slice_device(p5, 5, BC.THRESHOLD, LEAD, HANG, cin, True, 4)
    assert b == 1 and int(want["begin"][0]) == (1 << 31) - 6 + 1 - LEAD and int(want["end"][0]) == (1 << 31) - 1
    same(got, want, "at the limit")
    assert o.tobytes() == want_carry.tobytes()
    same(stream(d, ptr, env, [0, 77, env.size], BC.THRESHOLD, LEAD, HANG), seam["want"], "after the refusals")


# ------------------------------------------------------------------ 5. between two pushes
@pytest.mark.limit(60)
def test_slice_calls_between_two_pushes(capi, dec_factory, seam):
    from conftest import golden_cases, load_golden
    x, rec = load_golden(golden_cases()[0])
    plain = dec_factory(fresh=True, df18=rec["df18"])
    want_frames = plain.decode(x)
    d = dec_factory(fresh=True, df18=rec["df18"])
    half = x.size // 2 // 8 * 8
    d.push(x[:half])
    same(stream(d, seam["ptr"], seam["env"], [0, 1000, 3000, seam["env"].size], BC.THRESHOLD, LEAD, HANG), seam["want"], "between pushes")
    d.push(x[half:])
    d.finish()
    assert d.drain() == want_frames


# ------------------------------------------------------------------ 6. rebasing the window call
@pytest.mark.limit(60)
def test_level_windows_gives_the_same_at_two_bases(capi, dec_factory, torch_cuda):
    """adsb_level_windows on ONE buffer taken as the stream's samples from base + 40 on, base 0 and 56 k (28 power samples, first_sample
    % 8 kept): the reports and the envelope are equal word for word.  The record mode passes rebased positions on this ground."""
    d = dec_factory()
    rng = np.random.default_rng(24)
    runs = 690
    n = 16 + 56 * runs                                                    # the 16 samples that hold the six older pairs, then whole runs
    x = rng.integers(0, 4096, n, dtype=np.uint16)
    t, ptr = to_dev(torch_cuda, x)
    results = []
    for base in (0, 56 * 3, 56 * 12345, 56 * ((1 << 31) // 56)):
        te, pe = to_dev(torch_cuda, np.full(runs, -1.0, np.float32))
        m_lo = base // 2 + 28                                             # the buffer's sample 16 is the stream's sample base + 56
        edges = [m_lo, m_lo + 28 * 300, m_lo + 28 * runs - 5]
        reps = d.level_windows(ptr, base + 40, n, edges, env_ptr=pe, env_cap=runs)
        results.append((reps, te.cpu().numpy().view(np.uint32).copy()))
    reps0, env0 = results[0]
    assert sum(int(r["samples"]) for r in reps0) == 28 * runs - 5 and (env0 != np.array([-1.0], np.float32).view(np.uint32)[0]).all()
    for reps, env in results[1:]:
        assert np.array_equal(env, env0)
        for r, r0 in zip(reps, reps0):
            assert set(r) == set(r0)
            for key in r0:
                assert np.array_equal(np.asarray(r[key]), np.asarray(r0[key])), key


# ------------------------------------------------------------------ 7. the capture call's tables have not moved
@pytest.mark.limit(60)
def test_the_capture_gate_still_gives_its_tables(capi, dec_factory, seam):
    d = dec_factory()
    got, b = d.bursts_device(seam["ptr"], seam["env"].size, BC.THRESHOLD, LEAD, HANG, seam["want"].size + 8)
    assert b == seam["want"].size
    same(got, seam["want"], "adsb_bursts_device")


# ------------------------------------------------------------------ 8. the host program's record mode
def BA():
    from adsbdec_amd import burst_archive
    return burst_archive


@pytest.mark.limit(120)
def test_host_program_records_a_stream_in_pieces(capi, dec_factory, tmp_path):
    """A uint16 capture of 10 715 runs with a trailing n % 4: -L -U 48,2,4 -K writes the archive of the whole at the threshold T of
    the whole file's median.  -S @T,2,4,piece -O at pieces of 4000, 1000 and 17 runs -- a burst of some 50 runs lies across three
    pieces of 17 -- writes record_statement's bytes, which are that archive's, byte for byte; the stdout lines are the table's; -S
    48,2,4,4000 takes its threshold from the first piece; a FIFO gives what the file gives; -k prints the same packets from both; no
    spool file is left behind."""
    from tools import gen_signal as G
    x, _ = G.sparse_capture(600_002, 12, seed=5)
    a = dec_factory().power(x)
    M = 2 * (x.size // 4)
    (tmp_path / "c.bin").write_bytes(x.tobytes())
    run = lambda *args, **kw: subprocess.run([capi.CLI_PATH, *args], capture_output=True, timeout=100, **kw)
    q = run("-L", "-U", "48,2,4", "-K", str(tmp_path / "k.brs"), "-f", str(tmp_path / "c.bin"))
    assert q.returncode == 0, q.stderr.decode()
    whole = (tmp_path / "k.brs").read_bytes()
    arch = BA().unpack(whole)
    T, table = float(arch["threshold"]), arch["bursts"]
    assert 8 <= table.size <= 40 and (table["end"] - table["begin"]).max() > 2 * 17 + 2
    assert whole == BA().record_statement(x, 4000, T, 2, 4, a=a, absolute=True)
    lines = [f"bursts threshold {T:.9g} lead 2 hang 4"] + [f"{lo} {hi} {int(r['hot'])} {float(r['peak']):.9g}" for r, (lo, hi) in zip(table, LV().burst_samples(table, M))]
    for piece in (4000, 1000, 17):
        out = tmp_path / f"s{piece}.brs"
        q = run("-S", f"@{T:.9g},2,4,{piece}", "-O", str(out), "-f", str(tmp_path / "c.bin"))
        err = q.stderr.decode()
        assert q.returncode == 0, err
        assert out.read_bytes() == whole, piece
        assert q.stdout.decode().splitlines() == lines, piece
        assert f"kept {table.size} bursts, {arch['payload'].size} of {4 * M} bytes" in err and "4 trailing bytes ignored" in err, err
    # the factor form: the first piece's median decides
    q = run("-S", "48,2,4,4000", "-O", str(tmp_path / "f.brs"), "-f", str(tmp_path / "c.bin"))
    assert q.returncode == 0, q.stderr.decode()
    assert (tmp_path / "f.brs").read_bytes() == BA().record_statement(x, 4000, 48.0, 2, 4, a=a)
    # without -O: the lines alone, and no file
    q = run("-S", f"@{T:.9g},2,4,1000", "-f", str(tmp_path / "c.bin"))
    assert q.returncode == 0 and q.stdout.decode().splitlines() == lines and b"kept" not in q.stderr
    # through a FIFO
    fifo = tmp_path / "c.fifo"
    os.mkfifo(fifo)

    def feed():
        with open(fifo, "wb") as f:
            f.write(x.tobytes())
    t = threading.Thread(target=feed)
    t.start()
    q = run("-S", f"@{T:.9g},2,4,1000", "-O", str(tmp_path / "p.brs"), "-f", str(fifo))
    t.join()
    assert q.returncode == 0, q.stderr.decode()
    assert (tmp_path / "p.brs").read_bytes() == whole and q.stdout.decode().splitlines() == lines
    # a threshold every run is above: ONE burst, open from the first piece to the last -- the retained part grows piece by piece
    q = run("-S", "@1e-30,2,4,1000", "-O", str(tmp_path / "all.brs"), "-f", str(tmp_path / "c.bin"))
    assert q.returncode == 0, q.stderr.decode()
    assert q.stdout.decode().splitlines() == [f"bursts threshold {float(np.float32(1e-30)):.9g} lead 2 hang 4", f"0 {M} {-(-M // 28)} {float(LV().level_report(a)['env'].max()):.9g}"]
    assert (tmp_path / "all.brs").read_bytes() == BA().record_statement(x, 1000, 1e-30, 2, 4, a=a, absolute=True)
    os.remove(tmp_path / "all.brs")
    # ... and more retained than the program allows (64 Mi samples; here, for the test, 100 000): the gate never closes
    q = run("-S", "@1e-30,2,4,1000", "-O", str(tmp_path / "all.brs"), "-f", str(tmp_path / "c.bin"), env=dict(os.environ, ADSB_CLI_RECORD_RETAIN="100000"))
    assert q.returncode == 255 and b"raise the factor" in q.stderr and not q.stdout.decode().splitlines()[1:], q.stderr.decode()
    # -k: the packets of the recorded archive are those of -K's
    k1 = run("-k", "-a", "-f", str(tmp_path / "k.brs"))
    k2 = run("-k", "-a", "-f", str(tmp_path / "s17.brs"))
    assert k1.returncode == 0 and k2.returncode == 0 and k1.stdout == k2.stdout and len(k1.stdout) > 0
    assert sorted(os.listdir(tmp_path)) == sorted(["c.bin", "c.fifo", "k.brs", "s4000.brs", "s1000.brs", "s17.brs", "f.brs", "p.brs"])


@pytest.mark.limit(60)
def test_host_program_records_nothing_without_a_threshold(capi, torch_cuda, tmp_path):
    """A first piece without a sign-clear power sample cannot happen with uint16 input, whose power samples are sums of squares; what
    can is a stream without one power sample: status 255, no archive, no spool file.  An empty stream with @threshold: an empty
    archive."""
    (tmp_path / "short.bin").write_bytes(np.zeros(3, np.uint16).tobytes())
    q = subprocess.run([capi.CLI_PATH, "-S", "48,2,4", "-O", str(tmp_path / "out.brs"), "-f", str(tmp_path / "short.bin")], capture_output=True, timeout=50)
    assert q.returncode == 255 and b"no archive is written" in q.stderr, q.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["short.bin"]
    q = subprocess.run([capi.CLI_PATH, "-S", "@5,2,4", "-O", str(tmp_path / "out.brs"), "-f", str(tmp_path / "short.bin")], capture_output=True, timeout=50)
    assert q.returncode == 0, q.stderr.decode()
    assert (tmp_path / "out.brs").read_bytes() == BA().pack(4, 3, 0, 5.0, 2, 4, np.zeros(0, LV().BURST_DTYPE), np.zeros(0, np.uint8))
    assert q.stdout == b"bursts threshold 5 lead 2 hang 4\n" and sorted(os.listdir(tmp_path)) == ["out.brs", "short.bin"]
