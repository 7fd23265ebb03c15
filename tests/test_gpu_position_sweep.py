"""Planted frames swept over EVERY tile-relative offset of a scan tile (run with -m gpu on an MI355X).  The other offset-by-offset
modules (test_gpu_candidates.py, test_gpu_batch_records.py, test_gpu_front_records.py, test_gpu_iq8.py) hold the scan kernels to
the oracle where their captures happen to put a frame; a defect tied to one lane, one residue r = g mod 28, one pass seam or one
chunk boundary passes them unless a frame lands there by luck.  Here the samples stay and the tiles move (the oracle's answer for
an offset does not depend on where a launch's tiles begin), so every record kind is compared at every position of a tile:

* scan_kernel through adsb_scan_shard: [28 j, end) for EVERY j in [0, owned_runs(K)) at K = 2, 3 and 7, with statistics (and at
  K = 2 without: the other Stage B), the buffer start rotated over three values; with all_candidates the candidates and try words
  EQUAL the oracle's slice, with a default handle the list IS candidate_model.filter_model's;
* the end sweep: g_end at every candidate of every planted frame, with the buffer ending exactly with the last owned window and
  with the whole capture behind it; the head sweep: g_begin on the run a frame's candidates start in;
* fix_1bit over the K = 2 shifts of a capture whose long frames are all damaged, every bit 5 .. 111 at every r: the repaired
  records are exactly front_records_cases.repairable's;
* the four batch kernels (real, int16 IQ, int8 IQ, power): one call of 460 captures, capture j the pattern behind 28 j offsets of
  exact quiet -- overlapping views of ONE device buffer -- read back through adsb_batch_records.

No tolerance anywhere.  tests/test_position_sweep_cpu.py asserts without a device that the sweeps reach every position.  Measured
times and counts: profiles/r22_position_sweep_tests.txt."""
import time

import numpy as np
import pytest

import candidate_model as M
import position_sweep_cases as P
from conftest import records
from test_gpu_batch_records import _rebase
from test_gpu_candidates import _scan, _window
from test_gpu_front_records import _check_stats

# measured on an MI355X: every test under 0.7 s, the whole module 5 s behind the session's fixtures (profiles/r22_position_sweep_tests.txt)
pytestmark = [pytest.mark.gpu, pytest.mark.limit(60)]

CAPS = dict(cand_cap=512, try_cap=2048)       # the sweep capture has 262 candidates and 1 176 tries in all


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def swept(oracle, torch_cuda):
    """(capture, on the device, None): what test_gpu_candidates._scan takes; the oracle's lists are position_sweep_cases.sweep()'s."""
    x, _ = P.sweep()
    return x, torch_cuda.from_numpy(x.view(np.int16)).cuda(), None


def _same(k, j, got, want, tries, wtries, stats, what):
    """Equality of a scan's records and try words with the oracle's, the failing position class in the message."""
    assert got == want, (what, len(got), len(want), P.first_difference(k, j, got, want))
    if stats:
        assert np.array_equal(tries, wtries), (what, tries.size, wtries.size, P.first_try_difference(k, j, tries, wtries))
    else:
        assert tries.size == 0, what


# ------------------------------------------------------------------ scan_kernel: the start sweep
@pytest.mark.parametrize("sweep", P.SWEEPS, ids=[s[0] for s in P.SWEEPS])
def test_start_sweep_equals_the_oracle_at_every_shift(capi, swept, sweep):
    """scan_kernel over [28 j, end) for every j in [0, owned_runs(K)): with all_candidates the candidates (g, pw, bytes, reserved)
    and the try words equal the oracle's slice; with a default handle the tries equal it and the list is the filter model's.
    Without statistics (the other Stage B instantiation) the try array is empty."""
    sid, k, df18, stats = sweep
    L = P.sweep()[1]
    kept_want = P.kept_lists(sid)
    kw = dict(df18=df18, collect_stats=stats, debug_passes=k)
    d_all, d = capi.Decoder(all_candidates=True, **kw), capi.Decoder(**kw)
    t0, n_c, n_t = time.perf_counter(), 0, 0
    try:
        for j in P.shifts(k):
            gb, ge, fs = P.RUN * j, L.n_off, P.first_samples(j)
            want, wtries = _window(L.raw[df18], gb, ge)
            got, tries = _scan(capi, d_all, swept, False, fs, P.N_SWEEP - fs, gb, ge, **CAPS)
            _same(k, j, got, want, tries, wtries, stats, (sid, "all_candidates", j, fs))
            kept, tries = _scan(capi, d, swept, False, fs, P.N_SWEEP - fs, gb, ge, **CAPS)
            _same(k, j, kept, kept_want[j], tries, wtries, stats, (sid, "default", j, fs))
            n_c += len(got) + len(kept)
            n_t += 2 * wtries.size * stats
    finally:
        d_all.close()
        d.close()
    print(f"\n[{sid}] {2 * len(P.shifts(k))} scans, {n_c} candidates and {n_t} try words compared in {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ scan_kernel: the end and the head sweep
def test_end_sweep_cuts_every_frame_at_every_candidate(capi, swept):
    """K = 2, g_end = c0 .. cm + 1 of every planted frame (the frame at the capture's end among them): candidates at g_end - 1
    are in, those at g_end are out -- with the buffer ending exactly with the last owned offset's window, so that the last wave
    takes the plain-load road over the frame's own bits, and with the whole capture behind it."""
    L = P.sweep()[1]
    d_all = capi.Decoder(all_candidates=True, df18=True, collect_stats=True, debug_passes=2)
    t0, n_c, n_t, cells = time.perf_counter(), 0, 0, P.end_sweep(L)
    try:
        for gb, ge, fs, n_exact in cells:
            want, wtries = _window(L.raw[True], gb, ge)
            for n in (n_exact, P.N_SWEEP - fs):
                got, tries = _scan(capi, d_all, swept, False, fs, n, gb, ge, **CAPS)
                _same(2, gb // P.RUN, got, want, tries, wtries, True, ("end", gb, ge, fs, n))
                n_c += len(got)
                n_t += wtries.size
    finally:
        d_all.close()
    print(f"\n[end] {2 * len(cells)} scans, {n_c} candidates and {n_t} try words compared in {time.perf_counter() - t0:.2f} s")


def test_head_sweep_starts_a_launch_on_every_frame(capi, swept):
    """K = 2, g_begin on the run a planted frame's candidates start in, the buffer starting six pairs in front of it (the highest
    first_sample the call accepts): the frame's candidates are the first records of tile 0, at every r.  Both handles."""
    L = P.sweep()[1]
    kw = dict(df18=True, collect_stats=True, debug_passes=2)
    d_all, d = capi.Decoder(all_candidates=True, **kw), capi.Decoder(**kw)
    t0, n_c, n_t, cells = time.perf_counter(), 0, 0, P.head_sweep(L)
    try:
        for gb, fs in cells:
            want, wtries = _window(L.raw[True], gb, L.n_off)
            got, tries = _scan(capi, d_all, swept, False, fs, P.N_SWEEP - fs, gb, L.n_off, **CAPS)
            _same(2, gb // P.RUN, got, want, tries, wtries, True, ("head", "all_candidates", gb, fs))
            kept, tries = _scan(capi, d, swept, False, fs, P.N_SWEEP - fs, gb, L.n_off, **CAPS)
            _same(2, gb // P.RUN, kept, M.filter_model(want, gb, L.n_off, 2)[0], tries, wtries, True, ("head", "default", gb, fs))
            n_c += len(got) + len(kept)
            n_t += 2 * wtries.size
    finally:
        d_all.close()
        d.close()
    print(f"\n[head] {2 * len(cells)} scans, {n_c} candidates and {n_t} try words compared in {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ scan_kernel: one-bit repair at every shift
def test_repair_sweep_repairs_exactly_the_repairable(capi, oracle, torch_cuda):
    """fix_1bit and all_candidates over the K = 2 shifts of the damaged capture: the reserved = 1 records are exactly the set
    front_records_cases.repairable derives from the oracle's try words -- a missed repair fails like a wrong one -- and the try
    words are the oracle's."""
    x, L, fixed, every, _ = P.damaged()
    cap = (x, torch_cuda.from_numpy(x.view(np.int16)).cuda(), None)
    caps = dict(cand_cap=2 * len(every), try_cap=2 * L.tg[True].size)
    d_all = capi.Decoder(all_candidates=True, fix_1bit=True, df18=True, collect_stats=True, debug_passes=2)
    t0, n_c, n_t = time.perf_counter(), 0, 0
    g = [r[0] for r in every]
    try:
        for j in P.shifts(2):
            gb, fs = P.RUN * j, P.first_samples(j)
            want = every[int(np.searchsorted(g, gb)):]
            _, wtries = _window(L.raw[True], gb, L.n_off)
            got, tries = _scan(capi, d_all, cap, False, fs, x.size - fs, gb, L.n_off, **caps)
            _same(2, j, got, want, tries, wtries, True, ("repair", j, fs))
            n_c += len(got)
            n_t += wtries.size
    finally:
        d_all.close()
    assert n_c >= len(P.shifts(2)) * len(fixed)
    print(f"\n[repair] {len(P.shifts(2))} scans, {n_c} repaired records and {n_t} try words compared in {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------ the batch kernels
_held = {}


def _device(torch, front):
    """One device buffer per front end: 64 loud samples, 460 * 28 offsets of exact quiet, the pattern, 64 loud samples.  Capture j
    of the batch is the view that starts 28 j offsets in front of the pattern: 112 j bytes for real, int16 IQ and power samples
    (16-byte aligned), 56 j for int8 IQ (16-byte aligned for even j: scanned in place; 8-byte for odd j: through the call's
    scratch copy).  -> (the tensor that keeps the memory, [pointer of capture j], [its sample count])."""
    if front not in _held:
        p = P.pattern(front)
        rng = np.random.default_rng(7100)
        lead = P.BATCH_SHIFTS * P.RUN * p.per
        shape = (64 + lead + p.n + 64,) + p.x.shape[1:]
        if p.x.dtype == np.float32:
            buf = rng.uniform(0.0, 2.0 ** 28, shape).astype(np.float32)
        elif front == "real":
            buf = rng.integers(0, 4096, size=shape, dtype=np.uint16)
        else:
            info = np.iinfo(p.x.dtype)
            buf = rng.integers(info.min, info.max + 1, size=shape, dtype=p.x.dtype)
        buf[64:64 + lead] = p.quiet
        buf[64 + lead:64 + lead + p.n] = p.x
        t = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
        step = buf.itemsize * (buf.shape[1] if buf.ndim == 2 else 1)      # bytes per sample
        base = t.data_ptr() + step * (64 + lead)
        ptrs = [base - step * p.per * P.RUN * j for j in range(P.BATCH_SHIFTS)]
        ns = [p.n + p.per * P.RUN * j for j in range(P.BATCH_SHIFTS)]
        assert t.data_ptr() % 16 == 0 and min(ptrs) >= t.data_ptr() + step * 64
        assert {q % 16 for q in ptrs} == ({0, 8} if front == "iq8" else {0})
        _held[front] = (t, ptrs, ns)
    return _held[front]


def _decode_batch(d, front, ptrs, ns):
    if front == "real":
        return d.decode_batch_device(ptrs, ns, stats=True)
    if front == "power":
        return d.decode_batch_device_power(ptrs, ns, stats=True)
    return d.decode_batch_device_iq(8 if front == "iq8" else 2, ptrs, ns, stats=True)


_expected = {}


def _expect(front):
    if front not in _expected:
        _expected[front] = [P.pattern(front).expected(j) for j in range(P.BATCH_SHIFTS)]
    return _expected[front]


# (handle kind, all_candidates, collect_stats): every capture's records with statistics, what the filter leaves with statistics,
# and every record from the batch kernels' other instantiation, without statistics
KINDS = (("all", True, True), ("default", False, True), ("all_nostats", True, False))


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("front", P.BATCH_FRONTS)
def test_batch_sweep_equals_the_oracle_at_every_shift(capi, oracle, torch_cuda, front, kind):
    """One batch call of 460 captures at K = 2 -- scan_batch_kernel, scan_iq_batch_kernel, scan_iq8_batch_kernel or
    scan_power_batch_kernel: per capture the records, the try words, the frames and the Try/Ok table are those of the unshifted
    pattern moved by 28 j (held to the oracle directly in tests/test_position_sweep_cpu.py), the default handle's list the
    filter model's."""
    name, all_candidates, stats = kind
    p = P.pattern(front)
    want = _expect(front)
    _, ptrs, ns = _device(torch_cuda, front)
    assert ns == [w[0] for w in want]
    units = [n if front == "real" else 4 * (n // 2) for n in ns]
    segs_want, launches_want = capi.batch_layout(units, passes=P.BATCH_K)
    kw = dict(df18=True, collect_stats=stats, debug_passes=P.BATCH_K)
    d = capi.Decoder(all_candidates=all_candidates, **kw)
    t0 = time.perf_counter()
    try:
        frames, st = _decode_batch(d, front, ptrs, ns)
        cands, tries, segs, launches = d.batch_records()
    finally:
        d.close()
    t_call = time.perf_counter() - t0
    assert segs == segs_want and launches == launches_want and len(segs) == len(ns)      # uncut: a segment per capture
    per_c, per_t = _rebase(segs, cands, tries, len(ns))
    n_c = n_t = 0
    for j, (n, wc, wt, wf, ws) in enumerate(want):
        what = (front, name, j)
        if all_candidates:
            full = wc
        else:
            full = M.filter_model(wc, 0, p.offsets(n), P.BATCH_K)[0]
            assert 0 < len(full) < len(wc), what
        assert per_c[j] == full, (what, len(per_c[j]), len(full), P.first_difference(P.BATCH_K, j, per_c[j], full, batch=True))
        if stats:
            assert np.array_equal(per_t[j], wt), (what, per_t[j].size, wt.size, P.first_try_difference(P.BATCH_K, j, per_t[j], wt, batch=True))
        else:
            assert per_t[j].size == 0, what
        assert records(frames[j]) == records(wf), what
        _check_stats(st[j], ws, kw, what)
        n_c += len(full)
        n_t += wt.size * stats
    print(f"\n[{front}-{name}] 1 call of {len(ns)} captures ({t_call:.2f} s), {n_c} candidates and {n_t} try words compared in "
          f"{time.perf_counter() - t0:.2f} s")
