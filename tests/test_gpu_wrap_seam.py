"""The seam kernel's own output (run with -m gpu on an MI355X), sample by sample and offset by offset: the power samples of a
seam launch (adsb_seam_power) against the model of the front end across a counter wrap, bit for bit, and the candidates and try
words of a window across a wrap (adsb_scan_wrap_window: the seam kernel between the two epoch-relative scan launches a stream
makes) against the oracle's exhaustive evaluation of that power.  The cases, and why lists alone could not see a rounding-order
error: tests/wrap_seam_cases.py, tests/test_wrap_seam_cpu.py.  The stream-level view: tests/test_gpu_wrap_stream.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import candidate_model as M
import wrap_model as W
import wrap_seam_cases as S
from conftest import golden_cases, golden_records, load_golden, records

pytestmark = pytest.mark.gpu

LO, HI = S.SEAM_LO, S.SEAM_HI
# Offsets scanned on either side of the seam: more than one K = 2 tile (28 * 460 = 12 880) and a ragged end.  A launch starts at a
# run boundary of ITS epoch and 2^31 mod 28 = 16, so the one in front of the seam has 2^31 - 1196 - A = 0 (mod 28): A = 24 (mod 28);
# its length is then no multiple of 28 either.  The launch behind starts at P + 28; B is ragged by 17.
A = 28 * 470 + 24
B = 28 * 465 + 17
# where a stream's pushes may cut the seam offsets (relative to P): behind the first offset, around P - 1 .. P + 5, before the last.
# A cut c splits into [LO, c) and [c, HI): a cut AT the first offset P - 1196 would leave the first part empty, which a launch
# refuses, so the first cut is one offset behind it; P + 1 and P + 7 stand for the reading "the cut offset ends the first part".
CUTS = (LO + 1, -1, 0, 1, 5, 6, 7, HI - 1)
ALL_PLACEMENTS = (S.ZERO,) + S.PLACEMENTS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


def _dev(torch, y):
    return torch.from_numpy(np.array(y, dtype=np.uint16).view(np.int16)).cuda()      # (a copy: the cases are read-only)


@pytest.fixture(scope="module")
def windows(torch_cuda):
    """{(kind, placement): the window on the device}, and the two windows of extreme codes."""
    out = {(k, p): _dev(torch_cuda, S.window(k, p)) for k in S.KINDS for p in ALL_PLACEMENTS}
    out[("uniform16", None)] = _dev(torch_cuda, S.uniform_window())
    out[("blocks", None)] = _dev(torch_cuda, S.blocks_window())
    return out


@functools.lru_cache(maxsize=None)
def _samples(kind, placement):
    return S.uniform_window() if kind == "uniform16" else S.blocks_window() if kind == "blocks" else S.window(kind, placement)


@functools.lru_cache(maxsize=None)
def _power(kind, placement, w):
    a = S.power(_samples(kind, placement), w)
    a.flags.writeable = False
    return a


@pytest.fixture(scope="module")
def handles(capi):
    """Handles by configuration, made once: get(**keywords); long_stream is on unless it is named."""
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            kw.setdefault("long_stream", True)
            made[key] = capi.Decoder(**kw)
        return made[key]

    yield get
    for d in made.values():
        d.close()


def _tuples(cands, nc):
    return [(int(c.g), int(c.pw), bytes(c.frame[: c.len]), int(c.reserved)) for c in cands[:nc]]


def _scan(d, t, w, gb, ge, fs=None, n=S.N):
    fs = S.first_sample(w) if fs is None else fs
    cands, nc, tries = d.scan_wrap_window(t.data_ptr(), fs, n, gb, ge)
    assert d.wraps() == (0, 0)                                            # no stream state
    return _tuples(cands, nc), tries


def _want(oracle, kind, placement, w, df18, gb, ge):
    cands, tries = S.lists(oracle, _power(kind, placement, w), w, df18, gb, ge)
    return [c + (0,) for c in cands], tries


def _assert_same_power(got, want, first_rel, where):
    """got / want: power samples P + first_rel .. as float32; equal as uint32.  The message names P - 1 .. P + 5."""
    assert got.dtype == np.float32 and got.size == want.size, (where, got.size, want.size)
    g, v = got.view(np.uint32), want.view(np.uint32)
    if np.array_equal(g, v):
        return
    bad = np.nonzero(g != v)[0]
    transient = [(f"P{int(k) + first_rel:+d}", hex(int(g[k])), hex(int(v[k]))) for k in bad if int(k) + first_rel in S.TRANSIENT]
    others = [int(k) + first_rel for k in bad if int(k) + first_rel not in S.TRANSIENT]
    raise AssertionError(f"{where}: {bad.size} of {g.size} power samples differ; of P-1 .. P+5 (got, want): {transient}; "
                         f"others at P+{others[:8]}")


# ------------------------------------------------------------------------------------------------ 1. power, bit for bit
@pytest.mark.limit(5)
@pytest.mark.parametrize("w", S.WRAPS)
@pytest.mark.parametrize("placement", ALL_PLACEMENTS, ids=lambda p: f"at{p}")
def test_seam_power_equals_the_model_bit_for_bit(handles, windows, placement, w):
    d = handles(df18=True)
    _, _, P = S.offsets(w)
    for kind in S.KINDS:
        got = d.seam_power(windows[(kind, placement)].data_ptr(), S.first_sample(w), S.N, P, P + LO, P + HI)
        assert got.size == S.N_POWER == 2419
        _assert_same_power(got, S.seam_power(_power(kind, placement, w), w), LO, (kind, placement, w))


@pytest.mark.limit(5)
@pytest.mark.parametrize("w", S.WRAPS)
@pytest.mark.parametrize("kind", ["uniform16", "blocks"])
def test_seam_power_of_extreme_codes(handles, windows, kind, w):
    """Uniform full-range uint16 codes, and codes 0 / 4095 / 65535 in blocks: the largest products and sums the FIR can meet."""
    d = handles(df18=True)
    _, _, P = S.offsets(w)
    got = d.seam_power(windows[(kind, None)].data_ptr(), S.first_sample(w), S.N, P, P + LO, P + HI)
    _assert_same_power(got, S.seam_power(_power(kind, None, w), w), LO, (kind, w))
    assert np.isfinite(got).all() and got.max() > 1e8


@pytest.mark.limit(5)
@pytest.mark.parametrize("w", S.WRAPS)
def test_seam_power_of_partial_ranges(handles, windows, w):
    """A launch that ends inside the seam offsets and one that starts inside them, at every cut: element i is sample g_begin + i."""
    d = handles(df18=False, collect_stats=True)
    g0, _, P = S.offsets(w)
    for i, cut in enumerate(CUTS):
        kind, placement = S.KINDS[(i + w) % len(S.KINDS)], ALL_PLACEMENTS[i % len(ALL_PLACEMENTS)]
        a, t = _power(kind, placement, w), windows[(kind, placement)]
        for lo, hi in ((LO, cut), (cut, HI)):
            got = d.seam_power(t.data_ptr(), S.first_sample(w), S.N, P, P + lo, P + hi)
            want = a[P + lo - g0: P + hi - 1 + 1196 - g0]
            assert want.size == hi - lo - 1 + 1196
            _assert_same_power(got, want, lo, (kind, placement, w, lo, hi))


# ------------------------------------------------------------------------------------------------ 2. lists, offset by offset
def _cells(index):
    """(kind, placement, w) of one configuration: every kind at every placement, the wraps rotated over them."""
    return [(k, p, S.WRAPS[(i + j + index) % len(S.WRAPS)]) for i, k in enumerate(S.KINDS) for j, p in enumerate(ALL_PLACEMENTS)]


LIST_CONFIGS = [(df18, stats, passes) for passes in (0, 2, 7) for df18 in (True, False) for stats in (True, False)]


@pytest.mark.limit(5)
@pytest.mark.parametrize("index", range(len(LIST_CONFIGS)),
                         ids=[f"df18_{int(a)}-stats_{int(b)}-k{c}" for a, b, c in LIST_CONFIGS])
def test_candidates_and_tries_equal_the_oracle_offset_by_offset(oracle, handles, windows, index):
    df18, stats, passes = LIST_CONFIGS[index]
    kw = dict(df18=df18, collect_stats=stats, **(dict(debug_passes=passes) if passes else {}))
    d_all, d = handles(all_candidates=True, **kw), handles(**kw)
    for kind, placement, w in _cells(index):
        _, _, P = S.offsets(w)
        gb, ge = P + LO - A, P + HI + B
        where = (kind, placement, w)
        want, wtries = _want(oracle, kind, placement, w, df18, gb, ge)
        t = windows[(kind, placement)]
        got, tries = _scan(d_all, t, w, gb, ge)
        assert got == want, (where, sorted(set(got) ^ set(want))[:6])
        assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
        kept, tries = _scan(d, t, w, gb, ge)
        assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
        assert set(kept) <= set(want) and kept == sorted(kept), where
        assert not M.equivalent_from(want, kept, range(gb, gb + M.ENTRY_REACH), ge), where
        # the tile behind the seam: the seam's chain decides where it is entered
        assert not M.equivalent_from(want, kept, range(P + LO, P + HI + M.ENTRY_REACH), ge), where
        in_seam = [c for c in want if P + LO <= c[0] < P + HI]
        assert [c for c in kept if P + LO <= c[0] < P + HI] == in_seam, where    # the seam kernel reports every CRC-valid offset


# ------------------------------------------------------------------------------------------------ 3. two pushes' worth
@pytest.mark.limit(5)
@pytest.mark.parametrize("df18", [True, False])
def test_the_seam_taken_in_two_calls(oracle, handles, windows, df18):
    """A stream's pushes cut the seam offsets anywhere: [g_begin, cut) and [cut, g_end) together are the one call's lists."""
    d = handles(all_candidates=True, df18=df18, collect_stats=True)
    for i, cut in enumerate(CUTS):
        kind, placement, w = S.KINDS[(2 * i + df18) % len(S.KINDS)], S.PLACEMENTS[i % len(S.PLACEMENTS)], S.WRAPS[i % len(S.WRAPS)]
        _, _, P = S.offsets(w)
        gb, ge = P + LO - A, P + HI + B
        t = windows[(kind, placement)]
        whole, wtries = _scan(d, t, w, gb, ge)
        want, wt = _want(oracle, kind, placement, w, df18, gb, ge)
        assert whole == want and np.array_equal(wtries, wt), (kind, placement, w)
        c1, t1 = _scan(d, t, w, gb, P + cut)
        c2, t2 = _scan(d, t, w, P + cut, ge)
        assert c1 + c2 == whole and np.array_equal(np.concatenate([t1, t2]), wtries), (kind, placement, w, cut)
        # ... and the seam offsets alone, in two calls
        s1, u1 = _scan(d, t, w, P + LO, P + cut)
        s2, u2 = _scan(d, t, w, P + cut, P + HI)
        assert s1 + s2 == [c for c in whole if P + LO <= c[0] < P + HI], (kind, placement, w, cut)
        g = wtries >> np.uint64(2)
        assert np.array_equal(np.concatenate([u1, u2]), wtries[(g >= P + LO) & (g < P + HI)]), (kind, placement, w, cut)


# ------------------------------------------------------------------------------------------------ 4. 1-bit repair
@pytest.mark.limit(5)
@pytest.mark.parametrize("placement", S.DAMAGED_PLACEMENTS)
def test_one_bit_repair_in_the_seam_offsets(oracle, handles, torch_cuda, placement):
    """fix_1bit on the `damaged` kind placed so that damaged long frames start in the seam offsets, a different frame with a
    different damaged bit at each placement (tests/test_wrap_seam_cpu.py): the plain records are the oracle's, the repaired ones
    are long, CRC-valid and at offsets the oracle's list does not have -- in the seam, exactly the offsets one flipped bit
    mends, with the mended bytes (S.repairable)."""
    t = _dev(torch_cuda, S.damaged_window(placement))
    for w in S.WRAPS:
        _, _, P = S.offsets(w)
        gb, ge = P + LO - A, P + HI + B
        a = S.power(S.damaged_window(placement), w)
        mend = [m[:3] for m in S.repairable(oracle, a, w)]
        assert len(mend) >= 3
        cands, _ = S.lists(oracle, a, w, True, gb, ge)
        want = [c + (0,) for c in cands]
        for kw in (dict(), dict(debug_passes=2)):
            every, _ = _scan(handles(all_candidates=True, df18=True, fix_1bit=True, **kw), t, w, gb, ge)
            kept, _ = _scan(handles(df18=True, fix_1bit=True, **kw), t, w, gb, ge)
            assert [c for c in every if c[3] == 0] == want, (placement, w, kw)
            fixed = [c for c in every if c[3] == 1]
            wg = {c[0] for c in want}
            for c in fixed:
                assert len(c[2]) == 14 and oracle.crc_residual(c[2]) == 0 and c[0] not in wg, (placement, w, c)
            in_seam = [c for c in fixed if P + LO <= c[0] < P + HI]
            assert len(in_seam) >= 3
            assert [c[:3] for c in in_seam] == mend, (placement, w, kw)
            assert set(kept) <= set(every) and kept == sorted(kept)
            assert not M.equivalent_from(every, kept, range(gb, gb + M.ENTRY_REACH), ge), (placement, w, kw)
            assert not M.equivalent_from(every, kept, range(P + LO, P + HI + M.ENTRY_REACH), ge), (placement, w, kw)


# ------------------------------------------------------------------------------------------------ 5. the real reference
@pytest.fixture(scope="module")
def fixture():
    return W.load()


@pytest.mark.limit(5)
@pytest.mark.parametrize("df18", [False, True])
def test_the_wrap_bursts_of_the_reference(handles, torch_cuda, fixture, df18):
    """Each of the seven bursts the real reference chain decoded across a wrap (tests/golden/wrap_stream/): the window call over
    the burst, then the greedy chain from its first offset, gives that burst's (g, pw, frame) records of the fixture."""
    _, bursts, runs = fixture
    seen = 0
    for name, (s, y, w) in sorted(bursts.items(), key=lambda b: b[1][0]):
        if not w:
            continue
        Pp = (w - 1) * W.E
        gb = Pp + ((s // 2 - Pp) // 28 - 1) * 28                      # a run boundary of the epoch in front of the wrap
        pad = (s - 2 * (gb - 6) + 7) // 8 * 8
        buf = np.concatenate([np.full(pad, W.SILENCE, np.uint16), y, np.full(2400, W.SILENCE, np.uint16)])
        ge = (s + y.size) // 2
        t = _dev(torch_cuda, buf)
        want = [(g, pw, fr) for g, _, pw, fr in W.records(runs[df18], name)]
        assert len(want) > 20 and gb <= want[0][0] and want[-1][0] < ge
        for d in (handles(all_candidates=True, df18=df18), handles(df18=df18, collect_stats=True)):
            cands, _ = _scan(d, t, w, gb, ge, fs=s - pad, n=buf.size)
            assert [c[:3] for c in M.chain(cands, gb, ge)] == want, name
        seen += 1
    assert seen == 7


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.limit(5)
def test_refusals_leave_the_handle_usable(capi, handles, windows):
    L = capi.load()
    name = golden_cases()[0]
    x, rec = load_golden(name)
    d = capi.Decoder(long_stream=True, df18=rec["df18"], collect_stats=True)
    plain = capi.Decoder(df18=rec["df18"], collect_stats=True)
    try:
        w = 2
        _, _, P = S.offsets(w)
        t = windows[("dense", S.PLACEMENTS[0])]
        fs, gb, ge = S.first_sample(w), P + LO - A, P + HI + B
        cands, tries = (capi.Candidate * 4096)(), np.empty(1 << 16, dtype=np.uint64)
        nc, nt = C.c_size_t(0), C.c_size_t(0)
        power = np.empty(4096, dtype=np.float32)

        def scan(h, fs, n, gb, ge):
            return L.adsb_scan_wrap_window(h._h, t.data_ptr(), fs, n, gb, ge, cands, len(cands), C.byref(nc),
                                           tries.ctypes.data_as(C.POINTER(C.c_uint64)), tries.size, C.byref(nt))

        def seam_power(h, gb, ge, cap=power.size):
            return L.adsb_seam_power(h._h, t.data_ptr(), fs, S.N, P, gb, ge, power.ctypes.data_as(C.POINTER(C.c_float)), cap)

        def message(h):
            return (L.adsb_last_error(h._h) or b"").decode()

        assert scan(plain, fs, S.N, gb, ge) == -1 and "adsb_set_long_stream" in message(plain)      # no switch
        assert seam_power(plain, P + LO, P + HI) == -1 and "adsb_set_long_stream" in message(plain)
        for bad in (gb + 1, gb + 16, P + LO - 1, P + HI + 1):                                       # no run boundary, no seam offset
            assert scan(d, fs, S.N, bad, ge) == -1 and "run boundary" in message(d), bad
        assert scan(d, fs, S.N - 8192, gb, ge) == -1 and "does not cover" in message(d)             # the last windows are missing
        assert scan(d, fs + 8192, S.N - 8192, gb, ge) == -1 and "does not cover" in message(d)      # the first samples are
        assert scan(d, fs + 4, S.N - 4, gb, ge) == -1 and "multiple of 8" in message(d)
        for lo, hi in ((P + LO - 1, P + HI), (P + LO, P + HI + 1), (P + 3, P + 3), (P + S.E + LO, P + S.E + HI)):
            assert seam_power(d, lo, hi) == -1 and "seam offsets" in message(d), (lo - P, hi - P)
        assert seam_power(d, P + LO, P + HI, cap=S.N_POWER - 1) == -1 and "2419" in message(d)
        assert scan(d, fs, S.N, gb, ge) == 0 and nc.value > 0                                       # and the good call still works
        for h in (d, plain):
            frames = h.decode(x)
            assert records(frames) == golden_records(rec) and h.stats() == rec["stats"], name
    finally:
        d.close()
        plain.close()
