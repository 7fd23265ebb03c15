"""What the int8 IQ tests share (fmt 8 of the _iq calls): the committed fixtures of tests/golden/iq8, and the captures, the
oracle's lists and the greedy decodes that hold scan_iq8_kernel.hip to the oracle record by record.  tests/test_iq8_cpu.py
asserts, from the oracle and the layout alone, what the captures are for; tests/test_gpu_iq8.py runs them on the device.

The captures are those of tests/front_records_cases.py for the int16 IQ front end -- the nine kinds, the five edge captures, the
capture without offsets, in that order -- quantised with an arithmetic shift by 8 (sample_formats.to_int8_iq).  The reference
is the oracle on sample_formats.iq_power(x, 8) = 256 (I^2 + Q^2): the power samples of the widened twin (I << 8, Q << 8).  The
table of configurations, the greedy model, the repair list and the capture order are front_records_cases', imported."""
import functools
import json
import os
import time

import numpy as np

import front_records_cases as F
from conftest import GOLDEN
from front_records_cases import CONFIGS, IDS, BATCH_CELLS, KINDS, STREAM_KINDS, N, N_EDGE, units, n_offsets  # noqa: F401
from test_gpu_batch_records import EDGES
from test_batch_cpu import check_layout, launch_limit

IQ8_DIR = os.path.join(GOLDEN, "iq8")
INT8_IQ, S16_IQ = 8, 2
FIXTURES = ["full_scale", "noise", "ragged", "too_short", "workload_a", "workload_noa"]
SECONDS = {}


def iq8_fixtures():
    return sorted(f[:-5] for f in os.listdir(IQ8_DIR) if f.endswith(".json") and f != "generator_digests.json")


def load_iq8(name):
    with open(os.path.join(IQ8_DIR, name + ".json")) as f:
        rec = json.load(f)
    x = np.load(os.path.join(IQ8_DIR, rec["input"]))["x"]
    assert x.dtype == np.int8 and x.shape == (rec["n_samples"], 2)
    rec["stats"] = {k: {int(d): v for d, v in rec["stats"][k].items()} for k in rec["stats"]}
    return x, rec


def twin(x8):
    """The int16 capture (I << 8, Q << 8) an int8 capture is decoded as."""
    from adsbdec_amd.sample_formats import widen_int8_iq
    return widen_int8_iq(x8)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: front_records_cases.Case} in the order of the device buffer; evaluated once per process.  x is int8 of shape (n, 2)."""
    from adsbdec_amd.sample_formats import iq_power, power_domain_ok, to_int8_iq
    from oracle import oracle as O
    O.build()
    t0 = time.perf_counter()
    out = {}
    for name, x16 in F._captures(O, "iq").items():
        c = F.Case()
        c.x = np.ascontiguousarray(to_int8_iq(x16)[0])
        c.a = iq_power(c.x, INT8_IQ)
        c.n = int(len(c.x))
        c.n_off = n_offsets(c.n)
        assert c.a.dtype == np.float32 and c.a.size == c.n and power_domain_ok(c.a), name
        assert np.array_equal(c.a, iq_power(twin(c.x), S16_IQ)), name
        c.ev, c.dec = {}, {}
        m = c.n - (c.n & 1)
        for df18 in (False, True):
            cands, tries = O.scan_all(c.a, 0, c.n_off, df18)
            c.ev[df18] = ([r + (0,) for r in cands], tries)
            frames, stats = O.demod_power(c.a, df18=df18)
            c.dec[(df18, False)] = (frames, stats)
            mf, ms, _ = F.greedy(c.ev[df18][0], tries, m)
            assert F._records(mf) == F._records(frames) and (ms["try"], ms["ok"], ms["fixed"]) == (stats["try"], stats["ok"], 0), (name, df18)
        c.fixed = F.repairable(O, c.a, *c.ev[True]) if c.n_off else []
        c.dec[(True, True)] = F.greedy(sorted(c.ev[True][0] + c.fixed), c.ev[True][1], m)[:2]
        out[name] = c
    assert out["short"].n_off == 0 and [n for n in out if n not in EDGES and n != "short"] == list(KINDS)
    SECONDS["iq8"] = time.perf_counter() - t0
    return out


def full_list(c, kw):
    return F.full_list(c, kw)


def layout(capi, cfg_index, cut):
    """(capture order, sample counts, segments, launches) of a batch cell: adsb_batch_layout_ex asked at units(n), the number the
    widened twin's call is asked at."""
    _, kw, limit = CONFIGS[cfg_index]
    host = cases()
    order = F._order(host, cfg_index)
    ns = [host[name].n for name in order]
    k = kw.get("debug_passes", 0)
    lo = limit if cut else 0
    segs, launches = capi.batch_layout([units(n) for n in ns], passes=k, launch_offsets=lo)
    check_layout([units(n) for n in ns], segs, launches, launch_limit(lo, k))
    return order, ns, segs, launches
