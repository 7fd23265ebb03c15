"""What keeps the cells of tests/test_gpu_front_records.py from passing vacuously, for the IQ and the power front end, from the
oracle's lists and the batch layout alone (nothing here reads a device): the captures carry candidates and tries, the cut runs
cut, roll over and mix captures in a launch, back-to-back traffic has candidates close to both sides of every cut, the forced-K
cells reach every regime of the never-visited filter and overflow the shrunken staged list and survivor queue, and the 1-bit
repair has records to add.  The pattern of test_gpu_batch_records.py::test_cut_layouts_reach_what_they_are_for."""
import numpy as np
import pytest

import candidate_model as M
import front_records_cases as F
from test_batch_cpu import launch_limit


@pytest.mark.parametrize("front", F.FRONTS)
def test_cells_reach_what_they_are_for(capi, front):
    host = F.cases(front)
    # every kind but `uniform` has CRC-valid candidates and tries to compare
    for name in F.KINDS:
        cands, tries = host[name].ev[True]
        assert name == "uniform" or (len(cands) >= 50 and tries.size >= 500), (front, name, len(cands), tries.size)
    total = np.zeros(4, dtype=np.int64)
    for ci in F.BATCH_CELLS:
        cid, kw, limit = F.CONFIGS[ci]
        k = kw.get("debug_passes", 0)
        cap = kw.get("debug_clist_cap", M.CLIST_CAP)
        for cut in (False, True):
            order, ns, segs, launches = F.layout(capi, front, ci, cut)
            if k:
                for j, name in enumerate(order):
                    want = F.full_list(host[name], kw)
                    for s in F._pieces(segs, j):
                        counts = M.filter_model([c for c in want if s["o_begin"] <= c[0] < s["o_end"]], s["o_begin"], s["o_end"], k, 0, cap)[1]
                        total += M.regimes(counts, cap)
            if not cut:
                assert len(launches) == 1 and len(segs) == len(ns), cid
                continue
            n_segs = [len(F._pieces(segs, j)) for j in range(len(ns))]
            # (a K = 32 tile is longer than any capture here: that cell rolls over, it cannot cut)
            assert launch_limit(limit, k) == limit and len(launches) >= 4 and (k == 32 or sum(v >= 2 for v in n_segs) >= 6), (cid, n_segs)
            b2b = order.index("back_to_back")
            gs = np.array([c[0] for c in host["back_to_back"].ev[kw["df18"]][0]])
            cuts = [s["o_begin"] for s in F._pieces(segs, b2b)][1:]
            assert cuts or k == 32, cid
            # a candidate within 1 200 offsets (a frame every 1 200) on both sides of every cut; with DF18 off every third frame
            # is no candidate: within 2 400
            reach = 1200 if kw["df18"] else 2400
            for c in cuts:
                assert ((gs >= c - reach) & (gs < c)).any() and ((gs >= c) & (gs < c + reach)).any(), (cid, c)
            if F.NAMED_CUTS.get(cid) == 2:                   # four pieces a capture: at least six captures in three segments or more
                assert sum(v >= 3 for v in n_segs) >= 6, (cid, n_segs)
            elif F.NAMED_CUTS.get(cid) == 7 or (k == 7 and limit == F.BATCH_CONFIGS[0][2]):
                # a launch that holds segments of two captures or more behind a launch that ended on a roll-over (its last segment
                # ends a capture, the next capture did not fit what was left)
                mixed = [li for li in range(1, len(launches))
                         if len({s["capture"] for s in segs[launches[li]["seg_first"]:launches[li]["seg_end"]] if s["o_end"] > s["o_begin"]}) >= 2
                         and segs[launches[li]["seg_first"]]["o_begin"] == 0
                         and segs[launches[li]["seg_first"] - 1]["capture"] != segs[launches[li]["seg_first"]]["capture"]]
                assert mixed, (cid, [(L["seg_first"], L["seg_end"]) for L in launches])
    print(front, "forced-K batch tiles per regime (<=64, 65-128, 129-256, incomplete):", total.tolist())
    assert (total > 0).all(), (front, total.tolist())
    # the gate storm overflows a survivor queue of 256 in a K = 7 tile
    tg = (host["gate_storm"].ev[True][1] >> np.uint64(2)).astype(np.int64)
    storm = max(int(np.searchsorted(tg, t1) - np.searchsorted(tg, t0)) for t0, t1 in M.tile_bounds(0, host["gate_storm"].n_off, 7))
    print(front, "most tries of the gate storm in one K = 7 tile:", storm)
    assert storm > 256, (front, storm)
    # the stream kernels' forced-K cells, on the kinds they decode
    for ci, (cid, kw, _) in enumerate(F.CONFIGS):
        if kw.get("debug_passes"):
            print(front, cid, "stream kinds: most staged entries / tries in one tile:", F.check_stream_reach(front, ci))
    # what fix_1bit has to add
    n_fixed = sum(len(c.fixed) for c in host.values())
    print(front, "records the 1-bit repair adds:", n_fixed, "of them in `damaged`:", len(host["damaged"].fixed))
    assert n_fixed > 20, (front, n_fixed)
