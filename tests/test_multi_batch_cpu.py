"""adsb_multi_batch_plan, the pure host function behind adsb_multi_decode_batch_*: contiguous ranges of captures per worker,
balanced by the offsets the reference scans in each capture, every range cut into sub-batches of bounded size."""
import numpy as np
import pytest


def offsets(n):
    """What batch.hpp's batch_offsets says, restated from air.c:59-99: the offsets of a file of n samples the reference scans."""
    power, m = 2 * ((n + 3) // 4), 2 * (n // 4)
    return m - 1196 + 1 if power >= 40980 and m >= 1196 else 0


def nbytes(n, packed):
    return n // 8 * 12 if packed else 2 * n


def check_plan(capi, ns, workers, batch_bytes, packed=False):
    rng, subs = capi.multi_batch_plan(ns, workers, batch_bytes, packed)
    k = len(ns)
    # ranges: contiguous, in order, every capture once
    assert len(rng) == workers + 1 and rng[0] == 0 and rng[-1] == k
    assert all(a <= b for a, b in zip(rng, rng[1:]))
    # sub-batches: in order, non-empty, every capture once, none across two ranges
    assert subs[-1] == k and (subs[0] == 0 if k else subs == [0])
    assert all(a < b for a, b in zip(subs, subs[1:]))
    limit = batch_bytes if batch_bytes else 256 << 20
    for a, b in zip(subs, subs[1:]):
        assert any(rng[w] <= a and b <= rng[w + 1] for w in range(workers)), (a, b, rng)
        assert b - a == 1 or sum(nbytes(n, packed) for n in ns[a:b]) <= limit, (a, b)
    # balance: the largest worker's offsets <= the mean + the largest single capture's
    off = [offsets(n) for n in ns]
    loads = [sum(off[rng[w]:rng[w + 1]]) for w in range(workers)]
    assert sum(loads) == sum(off)
    if k:
        assert max(loads) <= sum(off) / workers + max(off), (loads, max(off))
    return rng, subs, loads


def test_offsets_restatement_matches_the_layout(capi):
    for n in (0, 8, 2392, 81952, 81956, 81957, 81960, 81961, 1 << 20, (1 << 20) + 3):
        segs, _ = capi.batch_layout([n])
        assert sum(s["o_end"] - s["o_begin"] for s in segs) == offsets(n), n


@pytest.mark.parametrize("workers", [1, 2, 3, 8, 64])
def test_plan_of_mixed_lengths(capi, workers):
    r = np.random.default_rng(workers)
    ns = [int(v) for v in r.integers(0, 1 << 21, 500)] + [0, 8, 2392, 81952, 81960, 0, 0]
    r.shuffle(ns)
    for batch_bytes in (0, 1 << 20, 3 << 20, 64 << 20):
        for packed in (False, True):
            use = [n // 8 * 8 for n in ns] if packed else ns
            check_plan(capi, use, workers, batch_bytes, packed)


def test_equal_captures_split_evenly(capi):
    rng, subs, loads = check_plan(capi, [1 << 20] * 2048, 8, 0)
    assert [b - a for a, b in zip(rng, rng[1:])] == [256] * 8
    assert len(subs) - 1 == 8 * 2                                        # 256 x 2 MiB = 512 MiB per worker: two sub-batches of 256 MiB
    assert max(loads) == min(loads)


def test_one_capture_larger_than_batch_bytes_is_a_sub_batch_of_its_own(capi):
    ns = [1 << 16, 1 << 16, 1 << 22, 1 << 16, 1 << 16]
    rng, subs, _ = check_plan(capi, ns, 1, 1 << 20)
    assert subs == [0, 2, 3, 5]
    rng, subs, _ = check_plan(capi, ns, 1, 1 << 17)                      # ... and exactly at the bound: one capture each
    assert subs == [0, 1, 2, 3, 4, 5]


def test_more_workers_than_captures_and_no_capture(capi):
    rng, subs, loads = check_plan(capi, [1 << 20, 1 << 19, 1 << 20], 8, 0)
    assert sum(1 for a, b in zip(rng, rng[1:]) if b > a) == 3 and len(subs) == 4
    assert check_plan(capi, [], 4, 0)[:2] == ([0] * 5, [0])


def test_captures_without_offsets(capi):
    """Zero-length captures and captures below the reference's first deqframe call have no offsets: they are dealt out evenly
    when nothing else is there, and ride along otherwise."""
    rng, subs, loads = check_plan(capi, [0, 8, 2392, 81952] * 25, 4, 0)
    assert loads == [0] * 4 and [b - a for a, b in zip(rng, rng[1:])] == [25] * 4
    check_plan(capi, [0] * 10 + [1 << 20] + [0] * 10 + [1 << 20] + [0] * 10, 2, 0)
    check_plan(capi, [0] * 10, 3, 1)


def test_one_dominant_capture(capi):
    ns = [1 << 16] * 100 + [1 << 28] + [1 << 16] * 100
    rng, subs, loads = check_plan(capi, ns, 4, 0)
    assert max(loads) >= offsets(1 << 28)


def test_bad_arguments(capi):
    L = capi.load()
    import ctypes as C
    r = (C.c_size_t * 2)()
    assert L.adsb_multi_batch_plan(1, None, 1, 0, 0, r, None, 0) == -1
    n = (C.c_size_t * 1)(8)
    assert L.adsb_multi_batch_plan(1, n, 0, 0, 0, r, None, 0) == -1
    assert L.adsb_multi_batch_plan(1, n, 1, 0, 0, None, None, 0) == -1
    assert L.adsb_multi_batch_plan(1, n, 1, 0, 0, r, None, 0) == 1 and list(r) == [0, 1]   # sub_cap 0: the count alone
    assert L.adsb_multi_set_batch_bytes(None, 0) == -1
