"""adsb::count_tries_kernel on the MI355X, try by try: every case of tests/try_count_cases.py goes through adsb_count_tries_alone
(one launch by the decoder's own launcher, no handle) and must give the numpy definition's three counts, its carry-out as a
multiset, the true number of appended entries, the overflow flag, a zeroed n_carry_next -- and leave every input array and the 64
sentinel words behind every array as they were.  tests/test_try_count_cpu.py shows that each case reaches the branch it is for."""
import collections

import numpy as np
import pytest

import try_count_cases as T

pytestmark = pytest.mark.gpu

SENT = 0xA5                                   # every sentinel byte
FILL = 0x0BADC0DE0BADC0DE                     # carry_out before the launch
ACC0 = (5, (1 << 33) + 7, 11, 0)              # the counters before the launch: the kernel adds to them
NEXT0 = 0x12345                               # n_carry_next before the launch: the kernel zeroes it


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


class Dev:
    """A host array on the device with 64 sentinel elements behind it."""

    def __init__(self, torch, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        pad = np.full(64 * a.dtype.itemsize, SENT, np.uint8)
        self.host = np.concatenate([a.view(np.uint8).ravel(), pad])
        self.n, self.dtype = a.size, a.dtype
        self.t = torch.from_numpy(self.host.copy()).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr()

    def back(self):
        return self.t.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.back(), self.host)

    def values(self):
        got = self.back()
        body = self.n * self.dtype.itemsize
        assert (got[body:] == SENT).all(), "sentinel behind an output array"
        return got[:body].view(self.dtype)


def run(capi, torch, p, acc0=ACC0):
    """One launch over the pass p -> a Result-like object: acc (what the launch added), carried (the stored entries, as they lie),
    n_carry_out, overflow.  Asserts the sentinels, the inputs, n_carry_next and the untouched tail of carry_out."""
    L = capi.load()
    T.check_contract(p)
    regions = p.regions is not None
    inputs = dict(tries=Dev(torch, p.tries, np.uint32), frames=Dev(torch, p.frames, T.FRAME), carry_in=Dev(torch, p.carry_in, np.uint64),
                  n_carry=Dev(torch, [p.n_carry], np.uint32))
    if regions:
        inputs["regions"] = Dev(torch, p.regions, np.uint32)
        inputs["region_counts"] = Dev(torch, p.region_counts, np.uint32)
    carry_out = Dev(torch, np.full(p.carry_cap, FILL, np.uint64), np.uint64)
    n_out, n_next, acc = Dev(torch, [0], np.uint32), Dev(torch, [NEXT0], np.uint32), Dev(torch, acc0, np.uint64)
    rc = L.adsb_count_tries_alone(inputs["tries"].ptr, p.tries.size, inputs["regions"].ptr if regions else None,
                                  inputs["region_counts"].ptr if regions else None, p.n_tiles, p.passes, p.big_tiles, p.g_base,
                                  inputs["carry_in"].ptr, inputs["n_carry"].ptr, inputs["frames"].ptr, len(p.frames), p.hi, p.final,
                                  carry_out.ptr, p.carry_cap, n_out.ptr, n_next.ptr, acc.ptr, None)
    assert rc == 0, L.adsb_last_error(None)
    torch.cuda.synchronize()
    for name, d in inputs.items():
        assert d.unchanged(), f"the kernel wrote to {name} or behind it"
    r = T.Result()
    a = acc.values()
    r.acc = [int(a[k]) - acc0[k] for k in range(3)]
    r.overflow = int(a[3]) != 0
    r.n_carry_out = int(n_out.values()[0])
    assert int(n_next.values()[0]) == 0, "n_carry_next is not zeroed"
    out = carry_out.values()
    stored = min(r.n_carry_out, p.carry_cap)
    assert (out[stored:] == FILL).all(), "carry_out is written beyond the entries counted"
    r.carried = out[:stored].copy()
    assert not (r.carried == FILL).any()
    return r


def check(capi, torch, p, what=""):
    """Run p and hold the result to the model."""
    want = T.model(p)
    got = run(capi, torch, p)
    assert got.acc == want.acc, (what, got.acc, want.acc)
    assert got.n_carry_out == want.n_carry_out and got.overflow == want.overflow, (what, got.n_carry_out, want.n_carry_out, got.overflow)
    if want.overflow:
        assert got.carried.size == p.carry_cap
        left = collections.Counter(want.carried.tolist())
        left.subtract(collections.Counter(got.carried.tolist()))
        assert min(left.values()) >= 0, (what, "a stored entry is not one of the undecided tries")
    else:
        assert np.array_equal(np.sort(got.carried), want.carried), what
    return got, want


# ------------------------------------------------------------------ 1. window edges
@pytest.mark.limit(60)
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_window_edges(capi, torch_cuda, d):
    """Windows of 0, 1, 63, 64, 65 and 64 frames, the 65th frame behind the window of 64 at t1 + d; regions of 1, 127, 128, 129,
    4095 and 4096 words; the same tries through the regions, through the list and through the carry."""
    for route in T.ROUTES:
        p, _ = T.window_edges(d, route)
        check(capi, torch_cuda, p, (d, route))


# ------------------------------------------------------------------ 2. a frame in front of the tile and of the launch
@pytest.mark.limit(60)
@pytest.mark.parametrize("g_base", T.FRONT_BASES)
def test_frame_in_front_of_the_tile(capi, torch_cuda, g_base):
    """A frame that reaches t0 from 1199 offsets in front, one that ends at t0, one at t0 - 1: tile 0 and an inner tile, bases
    from 0 (key clamps to 0) over a launch that crosses 2^32 to 2^35; once with hi more than 2^32 beyond the base."""
    for kind in T.FRONT_KINDS:
        for route in T.ROUTES:
            p, _ = T.front_frames(g_base, kind, route)
            check(capi, torch_cuda, p, (g_base, kind, route))
    p, _ = T.front_frames(g_base, "reaches_t0", "regions", hi=g_base + (1 << 32) + 12345)
    got, _ = check(capi, torch_cuda, p, (g_base, "hi_rel clamp"))
    assert got.n_carry_out == 0


# ------------------------------------------------------------------ 3. hi
@pytest.mark.limit(60)
@pytest.mark.parametrize("final", [0, 1])
@pytest.mark.parametrize("kind", T.HI_KINDS)
def test_hi(capi, torch_cuda, kind, final):
    for route in T.ROUTES + ("mixed",):
        p, _ = T.hi_case(kind, final, route)
        check(capi, torch_cuda, p, (kind, final, route))


@pytest.mark.limit(60)
@pytest.mark.parametrize("n_late", [101, 5000])
def test_carry_overflow(capi, torch_cuda, n_late):
    """carry_cap = 100 with 101 and with 5 000 undecided tries: the flag, the true count, exactly 100 stored entries out of the
    model's multiset, nothing behind them, and the model's three counters."""
    p, _ = T.carry_overflow(n_late)
    got, want = check(capi, torch_cuda, p, n_late)
    assert got.overflow and got.n_carry_out == n_late and got.carried.size == 100 and len(set(got.carried.tolist())) == 100


@pytest.mark.limit(60)
def test_carry_count_above_cap(capi, torch_cuda):
    p, _ = T.carry_count_above_cap()
    check(capi, torch_cuda, p)


# ------------------------------------------------------------------ 4. geometry
@pytest.mark.limit(60)
@pytest.mark.parametrize("k,big,n_tiles", T.GEOMETRIES)
def test_geometry(capi, torch_cuda, k, big, n_tiles):
    p, _ = T.geometry_case(k, big, n_tiles)
    check(capi, torch_cuda, p, (k, big, n_tiles))


@pytest.mark.limit(60)
def test_region_count_above_cap(capi, torch_cuda):
    p, _ = T.region_count_above_cap()
    check(capi, torch_cuda, p)


# ------------------------------------------------------------------ 5. the list and carry trips, the frame array's size
@pytest.mark.limit(60)
def test_list_and_carry_trips(capi, torch_cuda):
    for make in (T.list_trips, T.carry_trips):
        p, _ = make()
        check(capi, torch_cuda, p, make.__name__)


@pytest.mark.limit(60)
@pytest.mark.parametrize("n_frames", T.FRAME_COUNTS)
def test_frame_array_sizes(capi, torch_cuda, n_frames):
    p, _ = T.frame_counts(n_frames)
    check(capi, torch_cuda, p, n_frames)


# ------------------------------------------------------------------ 6. real traffic
@pytest.mark.limit(120)
@pytest.mark.parametrize("k", [2, 7])
@pytest.mark.parametrize("kind", T.REPLAY_KINDS)
def test_replay_of_real_traffic(capi, torch_cuda, kind, k):
    """The oracle's try words of a capture, dealt into tile regions, against the frames the oracle decodes: one final pass, and three
    passes chained through the carry on the device -> stats["try"] of oracle.demod_power, and every pass the model's."""
    import front_records_cases as F
    c = F.cases("power")[kind]
    for df18 in (False, True):
        want = c.dec[(df18, False)][1]["try"]
        want = [want[11], want[17], want[18]]
        for passes in (T.replay_single(c, df18, k), T.replay_three(c, df18, k)):
            total, got = T.chain(passes, lambda p: run(capi, torch_cuda, p))
            assert total == want, (kind, k, df18, len(passes), total, want)
            for p, r in zip(passes, got):                      # (chain() left every pass with the carry-in it ran with)
                m = T.model(p)
                assert r.acc == m.acc and np.array_equal(np.sort(r.carried), m.carried) and not r.overflow, (kind, k, df18)


# ------------------------------------------------------------------ the refusals
@pytest.mark.limit(60)
def test_refusals_launch_nothing(capi, torch_cuda):
    torch = torch_cuda
    L = capi.load()
    p, _ = T.hi_case("in_span", 0, "mixed")
    d = dict(tries=Dev(torch, p.tries, np.uint32), regions=Dev(torch, p.regions, np.uint32), counts=Dev(torch, p.region_counts, np.uint32),
             carry_in=Dev(torch, p.carry_in, np.uint64), n_carry=Dev(torch, [p.n_carry], np.uint32), frames=Dev(torch, p.frames, T.FRAME),
             carry_out=Dev(torch, np.full(p.carry_cap, FILL, np.uint64), np.uint64), n_out=Dev(torch, [0], np.uint32),
             n_next=Dev(torch, [NEXT0], np.uint32), acc=Dev(torch, ACC0, np.uint64))

    def call(**kw):
        a = dict(tries=d["tries"].ptr, n_tries=p.tries.size, regions=d["regions"].ptr, counts=d["counts"].ptr, n_tiles=p.n_tiles,
                 passes=p.passes, big_tiles=0, g_base=p.g_base, carry_in=d["carry_in"].ptr, n_carry=d["n_carry"].ptr, frames=d["frames"].ptr,
                 n_frames=len(p.frames), hi=p.hi, final=0, carry_out=d["carry_out"].ptr, carry_cap=p.carry_cap, n_out=d["n_out"].ptr,
                 n_next=d["n_next"].ptr, acc=d["acc"].ptr)
        a.update(kw)
        return L.adsb_count_tries_alone(*a.values(), None)

    refused = [(dict(tries=None), b"NULL"), (dict(regions=None), b"NULL"), (dict(counts=None), b"NULL"), (dict(frames=None), b"NULL"),
               (dict(carry_in=None), b"NULL"), (dict(carry_out=None), b"NULL"), (dict(n_carry=None), b"NULL"), (dict(n_out=None), b"NULL"),
               (dict(n_next=None), b"NULL"), (dict(acc=None), b"NULL"), (dict(regions=None, counts=None), b"NULL"),
               (dict(tries=d["tries"].ptr + 2), b"aligned"), (dict(regions=d["regions"].ptr + 1), b"aligned"),
               (dict(frames=d["frames"].ptr + 4), b"aligned"), (dict(carry_in=d["carry_in"].ptr + 4), b"aligned"),
               (dict(carry_out=d["carry_out"].ptr + 4), b"aligned"), (dict(acc=d["acc"].ptr + 4), b"aligned"),
               (dict(n_out=d["n_out"].ptr + 2), b"aligned"), (dict(passes=1), b"passes"), (dict(passes=33), b"passes"),
               (dict(passes=0), b"passes"), (dict(carry_cap=0), b"carry_cap")]
    for kw, word in refused:
        assert call(**kw) == -1, kw
        msg = L.adsb_last_error(None)
        assert b"adsb_count_tries_alone" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all(x.unchanged() for x in d.values())
    # what it accepts: NULL where the count is zero (and carry_cap == 0 with final: nothing is carried in or out)
    assert call(tries=None, n_tries=0, regions=None, counts=None, n_tiles=0, frames=None, n_frames=0, carry_in=None, carry_out=None,
                carry_cap=0, final=1) == 0, L.adsb_last_error(None)
    torch.cuda.synchronize()
    assert d["acc"].unchanged() and int(d["n_next"].values()[0]) == 0
