"""The IQ and the power scan kernels' own output, record by record, at every knob (run with -m gpu on an MI355X):
scan_iq_kernel.hip and scan_power_kernel.hip are instantiations of their own of the stages the real-sample kernels share
(scan_stages.h), with slow paths of their own for pw (pw_at_iq, pw_at_power).  tests/test_gpu_batch_records.py and
tests/test_gpu_candidates.py hold the real-sample kernels to the oracle offset by offset under forced tile sizes, overflowing
staged lists, survivor queues and record buffers, cut launches and nine kinds of traffic; this module does the same for the two
front ends, with that module's table of configurations and its helpers.

Batch kernels (scan_iq_batch_kernel, scan_power_batch_kernel, with and without statistics): every (front end, configuration)
cell is one adsb_decode_batch_device_iq (int16) / adsb_decode_batch_device_power call over fifteen captures, uncut and cut, with
all_candidates on and off; the records and try words come back through adsb_batch_records and are compared for equality with
oracle.scan_all of the capture's own power array -- sample_formats.iq_power(x), or the array itself -- and the frames with
oracle.demod_power.  With fix_1bit the repaired records are exactly the set derived on the CPU from the oracle's try words and
crc_residual (front_records_cases.repairable): a missed repair fails like a wrong one.  The captures lie side by side in ONE
device buffer with loud samples in every gap.  These kernels have no FIR: an in-range offset reads nothing outside its capture,
so what a segment's clipping at [p_lo, p_hi) can spoil shows at the first and last offsets of the edge captures, which carry
candidates (asserted from the oracle in front_records_cases.cases).

The layout: adsb_batch_layout_ex expresses these kinds -- the batch calls lay out 16-bit units, 4 (n / 2) for n complex or power
samples (front_records_cases.units) -- so the segments and launches a call reports must EQUAL its answer, besides check_layout.

Stream kernels (scan_iq_kernel, scan_power_kernel): there is no record read-out, so every configuration -- the stream-only knobs
debug_big_tiles, debug_no_streaming and debug_try_cap among them -- is held to the oracle's greedy decode on the gate storm,
back-to-back and damaged kinds, from the device buffer and as a chunked host push.

tests/test_front_records_cpu.py asserts without a device that the cells reach what they are for."""
import numpy as np
import pytest

import candidate_model as M
import front_records_cases as F
from conftest import records
from test_gpu_batch_records import _rebase

# measured on an MI355X: see profiles/r16_front_records_tests.txt
pytestmark = [pytest.mark.gpu, pytest.mark.limit(90)]

F32_IQ, S16_IQ = 0, 2
CELLS = [(front, ci) for front in F.FRONTS for ci in range(len(F.CONFIGS))]
CELL_IDS = [f"{front}-{F.IDS[ci]}" for front, ci in CELLS]
BATCH = [(front, ci) for front, ci in CELLS if ci in F.BATCH_CELLS]
BATCH_IDS = [f"{front}-{F.IDS[ci]}" for front, ci in BATCH]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


def _loud(front, n, rng):
    """n loud samples for the guards and gaps: full-range int16 scalars, floats all over the power domain, full-range floats."""
    if front == "iq":
        return rng.integers(-32768, 32768, size=(n, 2), dtype=np.int16)
    if front == "power":
        return rng.uniform(0.0, 2.0 ** 28, n).astype(np.float32)
    return rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)


_device = {}


def device(torch, front):
    """The captures of a front end side by side in one device buffer ("iq_f32": the int16 captures' exact float twins): 16-byte
    aligned starts, the up to three samples between a capture's end and the next start loud like the guards in front of the first
    and behind the last.  -> (the tensor that keeps the memory, {name: pointer})."""
    if front not in _device:
        from adsbdec_amd.sample_formats import power_domain_ok, to_float32_iq
        kind = "power" if front == "power" else "iq"
        host = F.cases(kind)
        print(f"\n[{front}] the captures, the oracle's lists and decodes of {len(host)} captures took {F.SECONDS[kind]:.2f} s")
        rng = np.random.default_rng(5400)
        at, cur = {}, 64
        for name, c in host.items():
            at[name] = cur
            cur = (cur + c.n + 3) // 4 * 4
        buf = _loud(front, cur + 64, rng)
        assert front != "power" or power_domain_ok(buf)
        for name, c in host.items():
            buf[at[name]:at[name] + c.n] = to_float32_iq(c.x) if front == "iq_f32" else c.x
        t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
        step = buf.itemsize * (1 if front == "power" else 2)
        assert t.data_ptr() % 16 == 0 and t.numel() < 64 << 20
        _device[front] = (t, {name: t.data_ptr() + step * a for name, a in at.items()})
        assert all(p % 16 == 0 for p in _device[front][1].values())
    return _device[front]


def _key(kw):
    return (kw["df18"], bool(kw.get("fix_1bit")))


def _check_stats(got, want, kw, where):
    assert got["ok"] == want["ok"] and got.get("fixed", 0) == want.get("fixed", 0), where
    if kw["collect_stats"]:
        assert got["try"] == want["try"], where


def _check_frames(d, order, host, kw, frames, stats):
    total = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for j, name in enumerate(order):
        wf, ws = host[name].dec[_key(kw)]
        assert records(frames[j]) == records(wf), name
        _check_stats(stats[j], ws, kw, name)
        for row in ("try", "ok"):
            for df in (11, 17, 18):
                total[row][df] += stats[j][row][df]
    whole = d.stats()
    assert whole["ok"] == total["ok"] and (not kw["collect_stats"] or whole["try"] == total["try"])


def _run(capi, torch, front, cfg_index, cut, all_candidates, fmt=S16_IQ):
    """One batch call of a cell -> (frames, stats, per-capture candidates, per-capture tries, segments, launches, relaunches)."""
    _, kw, limit = F.CONFIGS[cfg_index]
    host = F.cases(front)
    order, ns, segs_want, launches_want = F.layout(capi, front, cfg_index, cut)
    _, ptrs = device(torch, "iq_f32" if fmt == F32_IQ else front)
    d = capi.Decoder(all_candidates=all_candidates, **kw, **(dict(debug_batch_launch_offsets=limit) if cut else {}))
    try:
        before = d.profile()
        if front == "iq":
            frames, stats = d.decode_batch_device_iq(fmt, [ptrs[name] for name in order], ns, stats=True)
        else:
            frames, stats = d.decode_batch_device_power([ptrs[name] for name in order], ns, stats=True)
        after = d.profile()
        _check_frames(d, order, host, kw, frames, stats)
        if fmt == F32_IQ:                                    # every scalar converted, none off the int16 grid
            assert d.format_report() == (2 * sum(ns), 0, 0)
        cands, tries, segs, launches = d.batch_records()
    finally:
        d.close()
    # the layout the call used is adsb_batch_layout_ex's at units(n), for a device of 256 compute units
    assert segs == segs_want and launches == launches_want
    assert after["launches"] - before["launches"] >= sum(1 for L in launches if L["tiles"])
    per_c, per_t = _rebase(segs, cands, tries, len(ns))
    return frames, stats, per_c, per_t, segs, launches, after["relaunches"] - before["relaunches"]


def _check_cell(capi, oracle, torch, front, cfg_index, cuts=(False, True), fmt=S16_IQ):
    cid, kw, _ = F.CONFIGS[cfg_index]
    host = F.cases(front)
    k, cap, fix = kw.get("debug_passes", 0), kw.get("debug_clist_cap", M.CLIST_CAP), bool(kw.get("fix_1bit"))
    uncut = None
    seen_relaunches = []
    for cut in cuts:
        order = F._order(host, cfg_index)
        frames_a, stats_a, every, tries_a, segs, launches, relaunched_a = _run(capi, torch, front, cfg_index, cut, True, fmt)
        frames, stats, kept, tries, segs_d, launches_d, relaunched = _run(capi, torch, front, cfg_index, cut, False, fmt)
        seen_relaunches.append((relaunched_a, relaunched))
        assert segs_d == segs and launches_d == launches
        assert (frames, stats) == (frames_a, stats_a)
        if "debug_cand_cap" in kw:
            assert relaunched_a >= 1 and relaunched >= 1, (cid, cut)
        n_fixed = 0
        for j, name in enumerate(order):
            where = (front, cid, "cut" if cut else "uncut", name)
            c = host[name]
            want, wtries = c.ev[kw["df18"]]
            end = c.n_off
            # all_candidates = 1: every offset's record, and every try word
            if fix:
                assert [r for r in every[j] if r[3] == 0] == want, where
                wg = {r[0] for r in want}
                fixed = [r for r in every[j] if r[3] != 0]
                for r in fixed:
                    assert r[3] == 1 and len(r[2]) == 14 and oracle.crc_residual(r[2]) == 0 and r[0] not in wg, (where, r)
                # every repairable offset is repaired, to exactly that frame, and nothing else is
                assert fixed == c.fixed, (where, len(fixed), len(c.fixed), sorted(set(fixed) ^ set(c.fixed))[:4])
                n_fixed += len(fixed)
            else:
                assert every[j] == want, (where, len(every[j]), len(want), sorted(set(every[j]) ^ set(want))[:4])
            for t in (tries_a[j], tries[j]):
                assert np.array_equal(t, wtries) if kw["collect_stats"] else t.size == 0, where
            # default: what the never-visited filter leaves
            full = F.full_list(c, kw)
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
            uncut = (frames, stats, every, None, tries)
        else:                                                # the cut run equals the uncut run, byte for byte
            # (the kept lists may differ where a cut moved a tile boundary: each has been held to its own model above)
            assert (frames, stats) == uncut[:2] and every == uncut[2] and all(np.array_equal(a, b) for a, b in zip(tries, uncut[4]))
    print(f"\n[{front}-{cid}] relaunches (all_candidates, default) per run:", seen_relaunches)


@pytest.mark.parametrize("front,cfg_index", BATCH, ids=BATCH_IDS)
def test_batch_records_equal_the_oracle_offset_by_offset(capi, oracle, torch_cuda, front, cfg_index):
    _check_cell(capi, oracle, torch_cuda, front, cfg_index)


def test_float32_iq_feeds_the_same_records(capi, oracle, torch_cuda):
    """k7_clist1, cut, with the captures as float32 IQ (fmt 0, the exact twins x / 32768): the batch conversion launch in front
    of scan_iq_batch_kernel feeds the same records.  (Power samples have one format: no such cell there.)"""
    _check_cell(capi, oracle, torch_cuda, "iq", F.IDS.index("k7_clist1"), cuts=(True,), fmt=F32_IQ)


def _decode_device(d, front, ptr, n):
    return d.decode_device_iq(S16_IQ, ptr, n) if front == "iq" else d.decode_device_power(ptr, n)


def _decode_host(d, front, x, mode):
    return d.decode_iq(S16_IQ, x, chunk=30_001, mode=mode) if front == "iq" else d.decode_power(x, chunk=30_001, mode=mode)


@pytest.mark.parametrize("front,cfg_index", CELLS, ids=CELL_IDS)
def test_stream_kernels_equal_the_oracle_decode(capi, oracle, torch_cuda, front, cfg_index):
    """scan_iq_kernel / scan_power_kernel under the cell's knobs, with all_candidates on and off: the frames and the Try/Ok table
    of the gate storm, back-to-back and damaged kinds, decoded in place from the buffer of loud gaps, and of one of them pushed
    from the host in chunks of 30 001 (sync and async), are the oracle's greedy decode.  A shrunken record or try buffer is
    regrown by a relaunch wherever the oracle counts more than it holds."""
    cid, kw, _ = F.CONFIGS[cfg_index]
    host = F.cases(front)
    _, ptrs = device(torch_cuda, front)
    if kw.get("debug_passes"):
        F.check_stream_reach(front, cfg_index)
    seen = []
    shrunk = "debug_cand_cap" in kw or "debug_try_cap" in kw
    for all_candidates in (True, False):
        d = capi.Decoder(all_candidates=all_candidates, **kw)
        try:
            for name in F.STREAM_KINDS:
                c = host[name]
                wf, ws = c.dec[_key(kw)]
                where = (front, cid, all_candidates, name)
                # (a handle keeps the buffers a relaunch has regrown: shrunken ones are seen by a handle's first decode only)
                dk = capi.Decoder(all_candidates=all_candidates, **kw) if shrunk else d
                try:
                    assert records(_decode_device(dk, front, ptrs[name], c.n)) == records(wf), where
                    _check_stats(dk.stats(), ws, kw, where)
                    relaunched = dk.profile()["relaunches"]
                    if shrunk:                               # ... and the regrown handle gives the same answer again
                        assert records(_decode_device(dk, front, ptrs[name], c.n)) == records(wf), where
                        _check_stats(dk.stats(), ws, kw, where)
                finally:
                    if dk is not d:
                        dk.close()
                seen.append(relaunched)
                # every try goes to the launch-wide list under debug_try_cap; with all_candidates every record to the loose list
                if "debug_try_cap" in kw:
                    assert c.ev[kw["df18"]][1].size > kw["debug_try_cap"] and relaunched >= 1, where
                if "debug_cand_cap" in kw and all_candidates and len(F.full_list(c, kw)) > kw["debug_cand_cap"]:
                    assert relaunched >= 1, where
            name = F.STREAM_KINDS[cfg_index % len(F.STREAM_KINDS)]
            c = host[name]
            wf, ws = c.dec[_key(kw)]
            for mode in ("sync", "async"):
                where = (front, cid, all_candidates, name, mode)
                assert records(_decode_host(d, front, c.x, mode)) == records(wf), where
                _check_stats(d.stats(), ws, kw, where)
        finally:
            d.close()
    print(f"\n[{front}-{cid}] stream relaunches per decode (all_candidates first):", seen)
    if "debug_cand_cap" in kw or "debug_try_cap" in kw:
        assert sum(seen) >= 1, (front, cid)
