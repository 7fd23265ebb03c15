"""Complex int8 (IQ) captures on the MI355X (run with -m gpu): scan_iq8_kernel.hip and every _iq call of the library with fmt 8,
held to the reference's demodulator on the numpy definition of the power samples (sample_formats.iq_power(x, 8) = 256 (I^2 + Q^2),
the widened twin's): the committed fixtures (tests/golden/iq8, minted through oracle/_ref/ref_adsbdec -p), equality with fmt 2 on
the twin, the batch kernels' records offset by offset under tests/front_records_cases.py's table of configurations, the stream
kernels at the stream-only knobs, lengths, alignments, chunks, batches, the refusals and the C host program's -q 8.

Every one of these fails on a library without fmt 8: the _iq calls refuse it there."""
import subprocess

import numpy as np
import pytest

import candidate_model as M
import front_records_cases as F
import iq8_cases as Q
from conftest import golden_records, records
from test_gpu_batch_records import _rebase

pytestmark = [pytest.mark.gpu, pytest.mark.limit(90)]

INT8_IQ, S16_IQ = 8, 2


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


def to_dev(torch, a, lead=0):
    """A numpy array as bytes on the device behind `lead` bytes of loud padding (and 64 behind it): (tensor that keeps the memory
    alive, pointer)."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(lead, 0x7F, np.uint8), b, np.full(64, 0x81, np.uint8)])).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + lead


# ------------------------------------------------------------------ 1. the fixtures through every call
@pytest.mark.parametrize("name", Q.FIXTURES)
def test_fixtures_through_every_call(capi, dec_factory, torch_cuda, name):
    """Frames (g, ts, pw, bytes) and Try/Ok of every fixture through push_iq + finish, push_iq_async in chunks of 30 001 (odd: a
    sample waits for its partner across every push), push_device_iq_final and decode_device_iq; nothing is converted."""
    x, rec = Q.load_iq8(name)
    want, n = golden_records(rec), len(x)
    d = dec_factory(df18=rec["df18"], collect_stats=True)
    t, ptr = to_dev(torch_cuda, x)

    def check(frames, how):
        assert records(frames) == want, (how, len(frames), len(want))
        assert d.stats() == rec["stats"], how
        assert d.format_report() == (0, 0, 0), how

    check(d.decode_iq(INT8_IQ, x), "push_iq + finish")
    check(d.decode_iq(INT8_IQ, x, chunk=30_001, mode="async"), "push_iq_async")
    d.reset()
    d.push_device_iq(INT8_IQ, ptr, n, final=True)
    check(d.drain(), "push_device_iq_final")
    check(d.decode_device_iq(INT8_IQ, ptr, n), "decode_device_iq")


# ------------------------------------------------------------------ 2. equality with fmt 2 on the widened twin
def test_int8_equals_int16_on_the_widened_twin(capi, dec_factory, torch_cuda):
    """The nine kinds quantised with >> 8 and a uniform full-range int8 capture: fmt 8 gives the records and the Try/Ok table
    fmt 2 gives on (I << 8, Q << 8) -- and the oracle's, where it has them."""
    host = Q.cases()
    caps = {name: host[name].x for name in Q.KINDS}
    caps["uniform8"] = np.random.default_rng(8800).integers(-128, 128, size=(Q.N, 2), dtype=np.int8)
    assert int(caps["uniform8"].min()) == -128 and int(caps["uniform8"].max()) == 127
    d8, d16 = dec_factory(df18=True, collect_stats=True), dec_factory(df18=True, collect_stats=True)
    n_frames = 0
    for name, x in caps.items():
        t8, p8 = to_dev(torch_cuda, x)
        t16, p16 = to_dev(torch_cuda, Q.twin(x))
        got = records(d8.decode_device_iq(INT8_IQ, p8, len(x)))
        assert got == records(d16.decode_device_iq(S16_IQ, p16, len(x))), name
        assert d8.stats() == d16.stats(), name
        if name in host:
            wf, ws = host[name].dec[(True, False)]
            assert got == records(wf) and d8.stats() == ws, name
        n_frames += len(got)
    assert n_frames > 300


# ------------------------------------------------------------------ 3. record by record against the oracle
_device = {}


def device(torch):
    """The captures side by side in ONE device buffer: 16-byte aligned starts, loud bytes in every gap and in front of the first
    and behind the last.  -> (the tensor that keeps the memory, {name: pointer})."""
    if not _device:
        host = Q.cases()
        print(f"\n[iq8] the captures, the oracle's lists and decodes of {len(host)} captures took {Q.SECONDS['iq8']:.2f} s")
        rng = np.random.default_rng(5480)
        at, cur = {}, 64
        for name, c in host.items():
            at[name] = cur
            cur = (cur + c.n + 7) // 8 * 8
        buf = rng.integers(-128, 128, size=(cur + 64, 2), dtype=np.int8)
        for name, c in host.items():
            buf[at[name]:at[name] + c.n] = c.x
        t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
        _device["t"] = (t, {name: t.data_ptr() + 2 * a for name, a in at.items()})
        assert all(p % 16 == 0 for p in _device["t"][1].values())
    return _device["t"]


def _key(kw):
    return (kw["df18"], bool(kw.get("fix_1bit")))


def _check_stats(got, want, kw, where):
    assert got["ok"] == want["ok"] and got.get("fixed", 0) == want.get("fixed", 0), where
    if kw["collect_stats"]:
        assert got["try"] == want["try"], where


def _run(capi, torch, cfg_index, cut, all_candidates):
    """One batch call of a cell -> (frames, stats, per-capture candidates, per-capture tries, segments, launches, relaunches)."""
    _, kw, limit = Q.CONFIGS[cfg_index]
    host = Q.cases()
    order, ns, segs_want, launches_want = Q.layout(capi, cfg_index, cut)
    _, ptrs = device(torch)
    d = capi.Decoder(all_candidates=all_candidates, **kw, **(dict(debug_batch_launch_offsets=limit) if cut else {}))
    try:
        before = d.profile()
        frames, stats = d.decode_batch_device_iq(INT8_IQ, [ptrs[name] for name in order], ns, stats=True)
        after = d.profile()
        for j, name in enumerate(order):
            wf, ws = host[name].dec[_key(kw)]
            assert records(frames[j]) == records(wf), name
            _check_stats(stats[j], ws, kw, name)
        assert d.format_report() == (0, 0, 0)
        cands, tries, segs, launches = d.batch_records()
    finally:
        d.close()
    # the layout the call used is adsb_batch_layout_ex's at units(n): the number the widened twin's call is asked at
    assert segs == segs_want and launches == launches_want
    per_c, per_t = _rebase(segs, cands, tries, len(ns))
    return frames, stats, per_c, per_t, segs, launches, after["relaunches"] - before["relaunches"]


@pytest.mark.parametrize("cfg_index", Q.BATCH_CELLS, ids=[Q.IDS[ci] for ci in Q.BATCH_CELLS])
def test_batch_records_equal_the_oracle_offset_by_offset(capi, oracle, torch_cuda, cfg_index):
    """scan_iq8_batch_kernel under the cell's knobs, uncut and cut, all_candidates on and off: the records and try words that
    come back through adsb_batch_records equal oracle.scan_all of iq_power(x, 8) offset by offset, the repaired records exactly
    the set derived from the oracle's try words, the kept records the never-visited filter's model."""
    cid, kw, _ = Q.CONFIGS[cfg_index]
    host = Q.cases()
    k, cap, fix = kw.get("debug_passes", 0), kw.get("debug_clist_cap", M.CLIST_CAP), bool(kw.get("fix_1bit"))
    uncut = None
    for cut in (False, True):
        order = F._order(host, cfg_index)
        frames_a, stats_a, every, tries_a, segs, launches, relaunched_a = _run(capi, torch_cuda, cfg_index, cut, True)
        frames, stats, kept, tries, segs_d, launches_d, relaunched = _run(capi, torch_cuda, cfg_index, cut, False)
        assert segs_d == segs and launches_d == launches and (frames, stats) == (frames_a, stats_a)
        if "debug_cand_cap" in kw:
            assert relaunched_a >= 1 and relaunched >= 1, (cid, cut)
        n_fixed = 0
        for j, name in enumerate(order):
            where = (cid, "cut" if cut else "uncut", name)
            c = host[name]
            want, wtries = c.ev[kw["df18"]]
            end = c.n_off
            if fix:
                assert [r for r in every[j] if r[3] == 0] == want, where
                fixed = [r for r in every[j] if r[3] != 0]
                assert fixed == c.fixed, (where, len(fixed), len(c.fixed), sorted(set(fixed) ^ set(c.fixed))[:4])
                n_fixed += len(fixed)
            else:
                assert every[j] == want, (where, len(every[j]), len(want), sorted(set(every[j]) ^ set(want))[:4])
            for t in (tries_a[j], tries[j]):
                assert np.array_equal(t, wtries) if kw["collect_stats"] else t.size == 0, where
            full = Q.full_list(c, kw)
            assert every[j] == full, where
            assert set(kept[j]) <= set(full) and kept[j] == sorted(kept[j]), where
            parts = F._pieces(segs, j)
            entries = [0] + [e for s in parts[1:] for e in range(s["o_begin"], min(s["o_begin"] + M.ENTRY_REACH, end))]
            assert not M.equivalent_from(full, kept[j], entries, end), where
            if k:
                model = [r for s in parts
                         for r in M.filter_model([r for r in full if s["o_begin"] <= r[0] < s["o_end"]], s["o_begin"], s["o_end"], k, 0, cap)[0]]
                assert kept[j] == model, (where, len(kept[j]), len(model), sorted(set(kept[j]) ^ set(model))[:6])
        if fix:
            assert n_fixed > 20, cid
        if uncut is None:
            uncut = (frames, stats, every, tries)
        else:                                                # the cut run equals the uncut run
            assert (frames, stats) == uncut[:2] and every == uncut[2] and all(np.array_equal(a, b) for a, b in zip(tries, uncut[3]))


@pytest.mark.parametrize("cfg_index", range(len(Q.CONFIGS)), ids=Q.IDS)
def test_stream_kernels_equal_the_oracle_decode(capi, oracle, torch_cuda, cfg_index):
    """scan_iq8_kernel under the cell's knobs -- debug_big_tiles, debug_no_streaming and debug_try_cap among them -- with
    all_candidates on and off: the frames and the Try/Ok table of the gate storm, back-to-back and damaged kinds, decoded in place
    from the buffer of loud gaps, and of one of them pushed from the host in chunks of 30 001 (sync and async), are the oracle's
    greedy decode."""
    cid, kw, _ = Q.CONFIGS[cfg_index]
    host = Q.cases()
    _, ptrs = device(torch_cuda)
    shrunk = "debug_cand_cap" in kw or "debug_try_cap" in kw
    seen = []
    for all_candidates in (True, False):
        d = capi.Decoder(all_candidates=all_candidates, **kw)
        try:
            for name in Q.STREAM_KINDS:
                c = host[name]
                wf, ws = c.dec[_key(kw)]
                where = (cid, all_candidates, name)
                dk = capi.Decoder(all_candidates=all_candidates, **kw) if shrunk else d
                try:
                    assert records(dk.decode_device_iq(INT8_IQ, ptrs[name], c.n)) == records(wf), where
                    _check_stats(dk.stats(), ws, kw, where)
                    seen.append(dk.profile()["relaunches"])
                finally:
                    if dk is not d:
                        dk.close()
                if "debug_try_cap" in kw:
                    assert c.ev[kw["df18"]][1].size > kw["debug_try_cap"] and seen[-1] >= 1, where
            name = Q.STREAM_KINDS[cfg_index % len(Q.STREAM_KINDS)]
            c = host[name]
            wf, ws = c.dec[_key(kw)]
            for mode in ("sync", "async"):
                where = (cid, all_candidates, name, mode)
                assert records(d.decode_iq(INT8_IQ, c.x, chunk=30_001, mode=mode)) == records(wf), where
                _check_stats(d.stats(), ws, kw, where)
        finally:
            d.close()
    if shrunk:
        assert sum(seen) >= 1, cid


# ------------------------------------------------------------------ 4. lengths
def test_every_short_length_and_the_lengths_around_the_horizon(capi, oracle, dec_factory, torch_cuda):
    """Every n in 0 .. 8 and 1 190 .. 1 260 (around the window of one offset), and a few around the first deqframe horizon, as one
    buffer and split in two (an odd first half leaves a sample waiting): the decode of that prefix by oracle.demod_power."""
    from adsbdec_amd.sample_formats import iq_power
    x, rec = Q.load_iq8("ragged")
    t, ptr = to_dev(torch_cuda, x)
    d = dec_factory(df18=True, collect_stats=True)
    lengths = list(range(0, 9)) + list(range(1190, 1261)) + [40_978, 40_979, 40_980, 40_981, 40_982, 40_983, 42_175, 42_176, 42_177, len(x) - 1, len(x)]
    some = 0
    for n in lengths:
        wf, ws = oracle.demod_power(iq_power(x[:n], INT8_IQ), df18=True)
        assert records(d.decode_device_iq(INT8_IQ, ptr if n else 0, n)) == records(wf) and d.stats() == ws, n
        assert records(d.decode_iq(INT8_IQ, x[:n])) == records(wf) and d.stats() == ws, n
        h = n // 2 | 1 if n > 1 else 0                       # an odd first half
        d.reset()
        d.push_iq(INT8_IQ, x[:h])
        d.push_iq(INT8_IQ, x[h:n])
        d.finish()
        assert records(d.drain()) == records(wf) and d.stats() == ws, (n, h)
        d.reset()
        d.push_device_iq(INT8_IQ, ptr, h)
        d.push_device_iq(INT8_IQ, ptr + 2 * h, n - h, final=True)
        assert records(d.drain()) == records(wf) and d.stats() == ws, (n, h)
        some += len(wf)
    assert some > 5


# ------------------------------------------------------------------ 5. alignment and chunking
def test_alignments_chunks_and_the_staged_path_equal_one_aligned_push(capi, dec_factory, torch_cuda):
    """The workload fixture from device pointers at every even byte offset 0 .. 14 mod 16 (offset 0 is scanned in place, the rest
    are staged), in one push and in two; from the host in chunks of 30 001; the odd-length ragged fixture from the host in chunks
    of 1 and of 3 complex samples, and from the device in such pieces: the frames and the Try/Ok table of one aligned push."""
    x, rec = Q.load_iq8("workload_a")
    want, n = golden_records(rec), len(x)
    d = dec_factory(df18=True, collect_stats=True)
    for lead in range(0, 16, 2):
        t, p = to_dev(torch_cuda, x, lead=lead)
        assert p % 16 == lead
        assert records(d.decode_device_iq(INT8_IQ, p, n)) == want and d.stats() == rec["stats"], lead
        d.reset()
        d.push_device_iq(INT8_IQ, p, 50_001)
        d.push_device_iq(INT8_IQ, p + 2 * 50_001, n - 50_001, final=True)
        assert records(d.drain()) == want and d.stats() == rec["stats"], lead
    t, p = to_dev(torch_cuda, x)
    d.reset()                                               # aligned pieces scanned in place, the seam through the staging buffer
    d.push_device_iq(INT8_IQ, p, 40_000)
    d.push_device_iq(INT8_IQ, p + 2 * 40_000, n - 40_000)
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    for mode in ("sync", "async"):
        assert records(d.decode_iq(INT8_IQ, x, chunk=30_001, mode=mode)) == want and d.stats() == rec["stats"], mode
    x, rec = Q.load_iq8("ragged")
    want, n = golden_records(rec), len(x)
    assert n % 2 == 1 and want
    for chunk in (1, 3):
        assert records(d.decode_iq(INT8_IQ, x, chunk=chunk)) == want and d.stats() == rec["stats"], chunk
    t, p = to_dev(torch_cuda, x)
    cuts = np.cumsum([0, 1, 3, 7, 4099, 30_001]).tolist() + [n]
    d.reset()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.push_device_iq(INT8_IQ, p + 2 * lo, hi - lo)
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]


# ------------------------------------------------------------------ 6. batches
def test_batches_equal_the_single_calls(capi, dec_factory, torch_cuda):
    """Seven captures -- 0, 1, 40 979, 40 982 and 40 983 samples and two fixtures -- through the device call and the host call,
    and from device pointers that are only 2-byte aligned: every capture's frames and Try/Ok table are those of its own
    decode_device_iq."""
    work, _ = Q.load_iq8("workload_a")
    full, _ = Q.load_iq8("full_scale")
    ragged, _ = Q.load_iq8("ragged")
    caps = [work[:0], work[:1], ragged[:40_979], ragged[:40_982], ragged[:40_983], work, full]
    d = dec_factory(df18=True, collect_stats=True)
    held = [to_dev(torch_cuda, c) for c in caps]
    single = []
    for c, (_, p) in zip(caps, held):
        single.append((records(d.decode_device_iq(INT8_IQ, p, len(c))), d.stats()))
    assert single[3][0] and single[5][0] and single[6][0] and not single[0][0] and not single[2][0]
    ns = [len(c) for c in caps]
    frames, stats = d.decode_batch_device_iq(INT8_IQ, [p if len(c) else 0 for c, (_, p) in zip(caps, held)], ns, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    assert d.format_report() == (0, 0, 0)
    frames, stats = d.decode_batch_iq(INT8_IQ, caps, stats=True)
    assert [(records(f), s) for f, s in zip(frames, stats)] == single
    for lead in (2, 6, 10):                                  # only 2-byte aligned: through the scratch copy
        held2 = [to_dev(torch_cuda, c, lead=lead) for c in caps]
        assert all(p % 4 == 2 for _, p in held2)
        frames, stats = d.decode_batch_device_iq(INT8_IQ, [p for _, p in held2], ns, stats=True)
        assert [(records(f), s) for f, s in zip(frames, stats)] == single, lead


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_stream_as_it_was(capi, dec_factory, torch_cuda):
    """fmt 8 into a fmt 0 / 2, a real or a power stream and each of them into a fmt 8 stream, NULL, an odd device pointer, 2^31
    samples, a long-stream handle, the power export: -1 with a message that names what it is about, and the stream that was in
    progress still finishes with its fixture's frames."""
    x, rec = Q.load_iq8("workload_a")
    want = golden_records(rec)
    t, ptr = to_dev(torch_cuda, x)
    n, half = len(x), len(x) // 2 + 1
    d = dec_factory(df18=True, collect_stats=True)
    real = np.full(4096, 2048, np.uint16)
    tr, pr = to_dev(torch_cuda, real)
    x16 = Q.twin(x)
    t16, p16 = to_dev(torch_cuda, x16)
    pw = np.zeros(4096, np.float32)

    def refused(call, *words):
        with pytest.raises(capi.AdsbError) as e:
            call()
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    d.reset()
    d.push_iq(INT8_IQ, x[:half])
    refused(lambda: d.push(real), "int8 IQ", "real")                                  # other kinds into an int8 stream: both named
    refused(lambda: d.push_device(pr, real.size), "int8 IQ", "real")
    refused(lambda: d.push_iq(S16_IQ, x16[:8]), "int8 IQ", "fmt 0 / 2")
    refused(lambda: d.push_device_iq(S16_IQ, p16, 8), "int8 IQ", "fmt 0 / 2")
    refused(lambda: d.push_device_iq(0, p16, 8), "int8 IQ", "fmt 0 / 2")
    refused(lambda: d.push_power(pw), "int8 IQ", "power")
    refused(lambda: d.push_device_iq(INT8_IQ, ptr + 1, 8), "2-byte aligned")
    refused(lambda: d.push_iq(INT8_IQ, (None, 8)), "NULL")
    refused(lambda: d.push_device_iq(INT8_IQ, None, 8), "NULL")
    refused(lambda: d.push_iq(INT8_IQ, (x.ctypes.data, 1 << 31)), "2^31")
    refused(lambda: d.push_device_iq(INT8_IQ, ptr, (1 << 31) - half), "2^31")
    d.push_device_iq(INT8_IQ, ptr + 2 * half, n - half)
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    # the whole-capture calls refuse before their reset: the finished stream's statistics are still there
    out = torch_cuda.zeros(4096, dtype=torch_cuda.float32, device="cuda")
    for call, words in ((lambda: d.decode_device_iq(INT8_IQ, ptr + 1, n), ("2-byte aligned",)),
                        (lambda: d.decode_device_iq(INT8_IQ, ptr, 1 << 31), ("2^31",)),
                        (lambda: d.decode_device_iq(INT8_IQ, None, n), ("NULL",)),
                        (lambda: d.decode_batch_device_iq(INT8_IQ, [ptr, ptr + 1], [n, n]), ("capture 1", "2-byte aligned")),
                        (lambda: d.decode_batch_device_iq(INT8_IQ, [ptr, None], [n, n]), ("capture 1", "NULL")),
                        (lambda: d.power_device_iq(INT8_IQ, ptr, 4096, out.data_ptr(), 4096), ("format 8", "not exported"))):
        refused(call, *words)
        assert d.stats() == rec["stats"]
    assert not bool(out.any())
    # fmt 8 into the other kinds of stream
    for first, words in ((lambda: d.push(real), ("real", "int8 IQ")), (lambda: d.push_iq(S16_IQ, x16[:half]), ("fmt 0 / 2", "int8 IQ")),
                         (lambda: d.push_power(pw), ("power", "int8 IQ"))):
        d.reset()
        first()
        refused(lambda: d.push_iq(INT8_IQ, x[:half]), *words)
        refused(lambda: d.push_device_iq(INT8_IQ, ptr, half), *words)
        d.finish()
    d.reset()
    d.push_iq(S16_IQ, x16[:half])                           # ... and the int16 stream goes on to the twin's frames, which are these
    refused(lambda: d.push_iq(INT8_IQ, x[half:]), "fmt 0 / 2", "int8 IQ")
    d.push_iq(S16_IQ, x16[half:])
    d.finish()
    assert records(d.drain()) == want and d.stats() == rec["stats"]
    # a long-stream handle takes no int8 samples, and stays usable for real ones
    dl = dec_factory(df18=True)
    dl.set_long_stream(True)
    refused(lambda: dl.push_iq(INT8_IQ, x[:half]), "long-stream", "int8 IQ")
    refused(lambda: dl.decode_device_iq(INT8_IQ, ptr, n), "long-stream")
    refused(lambda: dl.decode_batch_device_iq(INT8_IQ, [ptr], [n]), "long-stream")
    dl.push(real)
    dl.finish()
    assert dl.drain() == []


# ------------------------------------------------------------------ 8. the C host program
def test_cli_q8(capi, oracle, tmp_path):
    """adsbdec_amd_cli -q 8 -a -m -f prints the fixture's AVR-MLAT bytes and its Try/Ok table -- and, where the compiled reference
    travelled with the tree, the bytes ref_adsbdec -a -p prints for the capture's power file."""
    from adsbdec_amd.sample_formats import iq_power
    x, rec = Q.load_iq8("workload_a")
    path = tmp_path / "workload.cs8"
    x.tofile(path)
    p = subprocess.run([capi.CLI_PATH, "-q", "8", "-a", "-m", "-f", str(path)], capture_output=True, timeout=80)
    assert p.returncode == 0, p.stderr
    assert p.stdout == "".join(f["mlat"] for f in rec["frames"]).encode()
    table = p.stderr.decode().splitlines()
    tr = [ln for ln in table if ln.startswith("Try")][0].split()[2:]
    ok = [ln for ln in table if ln.startswith("Ok")][0].split()[2:]
    assert [int(v) for v in tr] == [rec["stats"]["try"][k] for k in (11, 17, 18)]
    assert [int(v) for v in ok] == [rec["stats"]["ok"][k] for k in (11, 17, 18)]
    pa = subprocess.run([capi.CLI_PATH, "-q", "8", "-a", "-f", str(path)], capture_output=True, timeout=80)
    assert pa.returncode == 0 and pa.stdout == "".join(f["avr"] for f in rec["frames"]).encode()
    if oracle.ref_available():
        # the reference's harness prints a row per frame -- ts, pw, length, then formatpkt's AVR, AVR-MLAT and Beast renderings --
        # and print_stats' table: its AVR and MLAT columns are the bytes the program printed, its table the program's
        pw = tmp_path / "workload.pw"
        iq_power(x, INT8_IQ).tofile(pw)
        r = subprocess.run([oracle.REF_ADSBDEC, "-a", "-p", str(pw)], capture_output=True, timeout=80)
        assert r.returncode == 0
        rows = [ln.split(" ") for ln in r.stdout.decode().splitlines()]
        assert "".join(row[3] + "\n" for row in rows).encode() == pa.stdout and len(rows) == len(rec["frames"])
        assert "".join(row[4] + "\n" for row in rows).encode() == p.stdout
        rerr = r.stderr.decode().splitlines()
        assert [int(v) for v in rerr[1].split(":")[1].split()] == [int(v) for v in tr]
        assert [int(v) for v in rerr[2].split(":")[1].split()] == [int(v) for v in ok]
