"""The scan kernel's own output, offset by offset (run with -m gpu on an MI355X): the CRC-valid candidates and DF-gate passes
that adsb_scan_shard hands back, against the oracle's exhaustive evaluation (oracle.scan_all), and the list the device's
never-visited filter leaves, against the host model of that filter (tests/candidate_model.py).  Frame parity tests see only
the chain from offset 0; these see every offset, at every tile geometry and overflow knob, and every entry a shard's
stitcher can re-enter at ([g_begin, g_begin + 1200)).

Per cell (a capture, a window [g_begin, g_end), the buffer's first sample, the handle's knobs):
* all_candidates = 1: the candidates (g, pw, bytes, reserved) and, with collect_stats, the try words equal the oracle's;
* default: the try words equal the oracle's, the list is a subset of the exhaustive one, its greedy chain equals the
  exhaustive one's from every entry of the contract, and -- where K is forced -- it IS the model's kept list."""
import ctypes as C

import numpy as np
import pytest

import candidate_model as M

pytestmark = pytest.mark.gpu

N_SAMPLES = 1 << 20
G_MAX = N_SAMPLES // 2 - 1195                 # offsets [0, G_MAX) of a capture have a whole window of power samples
TILE7 = 28 * M.owned_runs(7)                  # a K = 7 tile
# windows (g_begin, g_end): the whole capture; an odd multiple of 28 mid-capture with a ragged end; a tile boundary +- 28
WINDOWS = ((0, G_MAX), (28 * 4001, G_MAX - 333), (2 * TILE7 + 28, G_MAX - 1), (2 * TILE7 - 28, G_MAX - 28 * 1000 - 5))

# handle configurations: (id, keywords).  debug_passes forces K; every other knob is read at K = 7 unless named.
CONFIGS = [
    ("default", dict(df18=True, collect_stats=True)),
    ("default_df11_17", dict(df18=False, collect_stats=True)),
    ("default_nostats", dict(df18=True, collect_stats=False)),
    ("host_copy", dict(df18=True, collect_stats=True, host=True)),
    ("k2", dict(df18=True, collect_stats=True, debug_passes=2)),
    ("k3_df11_17", dict(df18=False, collect_stats=True, debug_passes=3)),
    ("k4_nostats", dict(df18=True, collect_stats=False, debug_passes=4)),
    ("k7", dict(df18=True, collect_stats=True, debug_passes=7)),
    ("k10", dict(df18=True, collect_stats=True, debug_passes=10)),
    ("k16_nostats", dict(df18=True, collect_stats=False, debug_passes=16)),
    ("k32", dict(df18=True, collect_stats=True, debug_passes=32)),
    ("k7_big1", dict(df18=True, collect_stats=True, debug_passes=7, debug_big_tiles=1)),
    ("k7_big3_host", dict(df18=True, collect_stats=False, debug_passes=7, debug_big_tiles=3, host=True)),
    ("k7_queue256", dict(df18=True, collect_stats=True, debug_passes=7, debug_queue_cap=256)),
    ("k7_clist1", dict(df18=True, collect_stats=True, debug_passes=7, debug_clist_cap=1)),
    ("k2_clist3", dict(df18=True, collect_stats=False, debug_passes=2, debug_clist_cap=3)),
    ("k10_clist64", dict(df18=True, collect_stats=True, debug_passes=10, debug_clist_cap=64)),
    ("k7_candcap", dict(df18=True, collect_stats=True, debug_passes=7, debug_cand_cap=64)),
    ("k7_nostream", dict(df18=False, collect_stats=True, debug_passes=7, debug_no_streaming=1)),
]


def _cells(cfg_index, names):
    """(capture, g_begin, g_end, first_sample, n) of one configuration: every capture, the windows and the two buffer
    starts rotated over them -- the lowest first_sample the call accepts, and one 8 000 samples lower."""
    out = []
    for i, name in enumerate(names):
        gb, ge = WINDOWS[(i + cfg_index) % len(WINDOWS)]
        fs = (2 * (gb - 6)) // 8 * 8 if gb >= 6 else 0
        if (i + cfg_index // 2) % 2:
            fs = max(0, fs - 8000)
        n = 2 * (ge - 1 + 1196) - fs if (i + cfg_index) % 3 else N_SAMPLES - fs
        out.append((name, gb, ge, fs, n))
    return out


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def captures(oracle, torch_cuda):
    """{name: (capture, on the device, {df18: (candidates, tries) of offsets [0, G_MAX)})}: the oracle's exhaustive
    evaluation is per offset, so a window's lists are slices of these."""
    out = {}
    for name, x in M.make_captures(N_SAMPLES).items():
        a = oracle.power(x)
        assert a.size - 1195 == G_MAX
        ev = {df18: oracle.scan_all(a, 0, G_MAX, df18) for df18 in (False, True)}
        out[name] = (x, torch_cuda.from_numpy(x.view(np.int16)).cuda(), ev)
    return out


def _window(ev, gb, ge):
    cands, tries = ev
    g = tries >> np.uint64(2)
    return [c + (0,) for c in cands if gb <= c[0] < ge], tries[(g >= gb) & (g < ge)]


def _scan(capi, dec, cap, host, fs, n, gb, ge, **caps):
    """adsb_scan_shard (or adsb_scan_shard_host from a pageable copy) -> (candidates as tuples, tries).  caps: cand_cap and
    try_cap of Decoder.scan_shard, for callers whose lists are short (its defaults allocate 8 MB a call)."""
    x, t, _ = cap
    if not host:
        cands, nc, tries = dec.scan_shard(t.data_ptr() + 2 * fs, fs, n, gb, ge, **caps)
    else:
        L = capi.load()
        buf = np.ascontiguousarray(x[fs:fs + n])
        cands, tries = (capi.Candidate * (1 << 16))(), np.empty(1 << 20, dtype=np.uint64)
        ncv, ntv = C.c_size_t(0), C.c_size_t(0)
        rc = L.adsb_scan_shard_host(dec._h, buf.ctypes.data, fs, n, gb, ge, cands, len(cands), C.byref(ncv),
                                    tries.ctypes.data_as(C.POINTER(C.c_uint64)), tries.size, C.byref(ntv))
        assert rc == 0, (L.adsb_last_error(dec._h) or b"").decode()
        nc, tries = ncv.value, tries[: ntv.value].copy()
    return _tuples(capi, cands, nc), tries


def _tuples(capi, cands, nc):
    """The first nc records of a capi.Candidate array as (g, pw, bytes, reserved), read through one numpy view of the array."""
    if not nc:
        return []
    size = C.sizeof(capi.Candidate)
    raw = np.frombuffer(cands, dtype=np.uint8, count=nc * size).reshape(nc, size)
    at = {name: getattr(capi.Candidate, name).offset for name in ("g", "pw", "len", "frame", "reserved")}
    g = raw[:, at["g"]:at["g"] + 8].copy().view(np.uint64)[:, 0].tolist()
    pw = raw[:, at["pw"]:at["pw"] + 4].copy().view(np.uint32)[:, 0].tolist()
    ln, res = raw[:, at["len"]].tolist(), raw[:, at["reserved"]].tolist()
    fr = raw[:, at["frame"]:at["frame"] + 14].tobytes()
    return [(g[i], pw[i], fr[14 * i:14 * i + ln[i]], res[i]) for i in range(nc)]


@pytest.mark.limit(120)
@pytest.mark.parametrize("cfg_index", range(len(CONFIGS)), ids=[c[0] for c in CONFIGS])
def test_candidates_and_tries_equal_the_oracle_offset_by_offset(capi, captures, cfg_index):
    _, kw = CONFIGS[cfg_index]
    kw = dict(kw)
    host = kw.pop("host", False)
    k, big = kw.get("debug_passes", 0), kw.get("debug_big_tiles", 0)
    cap = kw.get("debug_clist_cap", M.CLIST_CAP)
    stats, df18 = kw["collect_stats"], kw["df18"]
    d_all = capi.Decoder(all_candidates=True, **kw)
    d = capi.Decoder(**kw)
    try:
        for name, gb, ge, fs, n in _cells(cfg_index, list(captures)):
            where = (name, gb, ge, fs, n)
            want, wtries = _window(captures[name][2][df18], gb, ge)
            got, tries = _scan(capi, d_all, captures[name], host, fs, n, gb, ge)
            assert got == want, where
            assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
            kept, tries = _scan(capi, d, captures[name], host, fs, n, gb, ge)
            assert np.array_equal(tries, wtries) if stats else tries.size == 0, where
            assert set(kept) <= set(want) and kept == sorted(kept), where
            assert not M.equivalent_from(want, kept, range(gb, min(gb + M.ENTRY_REACH, ge)), ge), where
            if k:
                model, _ = M.filter_model(want, gb, ge, k, big, cap)
                assert kept == model, (where, len(kept), len(model), sorted(set(kept) ^ set(model))[:6])
    finally:
        d_all.close()
        d.close()


def test_forced_geometries_reach_every_regime_of_the_filter(captures):
    """The forced-K cells above drive each of the filter's three implementations and the incomplete list: tiles that
    stage <= 64, 65-128 and 129-256 entries, and more than clist_cap (counted by the model on the same cells)."""
    total = np.zeros(4, dtype=np.int64)
    for i, (_, kw) in enumerate(CONFIGS):
        if not kw.get("debug_passes"):
            continue
        cap = kw.get("debug_clist_cap", M.CLIST_CAP)
        for name, gb, ge, _, _ in _cells(i, list(captures)):
            want, _ = _window(captures[name][2][kw["df18"]], gb, ge)
            total += M.regimes(M.filter_model(want, gb, ge, kw["debug_passes"], kw.get("debug_big_tiles", 0), cap)[1], cap)
    print("forced-K tiles per regime (<=64, 65-128, 129-256, incomplete):", total.tolist())
    assert (total > 0).all(), total.tolist()


@pytest.mark.limit(120)
@pytest.mark.parametrize("name", ["damaged", "back_to_back", "noise"])
def test_one_bit_repair_candidates(capi, oracle, captures, name):
    """fix_1bit = 1: the all_candidates list is the oracle's exhaustive list plus repaired long frames (reserved = 1, CRC
    now valid: at offsets absent from the oracle's list); the default list is
    chain-equivalent to it from every entry of the contract, at the default K and at forced ones."""
    x, t, ev = captures[name]
    n_fixed = 0
    for kw, (gb, ge) in ((dict(), WINDOWS[0]), (dict(debug_passes=7), WINDOWS[1]), (dict(debug_passes=2), WINDOWS[2])):
        want, _ = _window(ev[True], gb, ge)
        d_all = capi.Decoder(df18=True, fix_1bit=True, all_candidates=True, **kw)
        d = capi.Decoder(df18=True, fix_1bit=True, **kw)
        try:
            fs = (2 * (gb - 6)) // 8 * 8 if gb >= 6 else 0
            every, _ = _scan(capi, d_all, captures[name], False, fs, N_SAMPLES - fs, gb, ge)
            kept, _ = _scan(capi, d, captures[name], False, fs, N_SAMPLES - fs, gb, ge)
        finally:
            d_all.close()
            d.close()
        assert [c for c in every if c[3] == 0] == want, (name, kw)
        fixed = [c for c in every if c[3] == 1]
        wg = {c[0] for c in want}
        for c in fixed:
            assert len(c[2]) == 14 and oracle.crc_residual(c[2]) == 0 and c[0] not in wg, (name, c)
        n_fixed += len(fixed)
        assert set(kept) <= set(every) and kept == sorted(kept)
        assert not M.equivalent_from(every, kept, range(gb, min(gb + M.ENTRY_REACH, ge)), ge), (name, kw)
    if name == "damaged":
        assert n_fixed > 100
