"""The level report of an array of power samples: the numpy statement that the adsb_level_* calls (include/adsbdec_amd.h,
csrc/level_kernel.hip) are held to, bit for bit.

`a` is a float32 array of M power samples and b = a.view('<u4') their bit patterns:

    samples    M
    negative   samples with the sign bit set (-0.0 counts)
    hist[k]    k in 0 .. 2047, uint64: sign-clear samples with b >> 20 == k -- the exponent and the top three mantissa bits, 8 bins
               per octave (about 0.75 dB each).  1.0 is bin 1016, 2^29 is bin 1248, Inf and NaN are bins 2040 and up.
               hist.sum() + negative == M.
    env[r]     r in 0 .. ceil(M / 28) - 1, float32: the float whose bit pattern is the unsigned maximum over samples
               [28 r, min(28 r + 28, M)) of (b if the sign is clear, else 0).  For data in the _power calls' domain that is the
               float maximum of the run; on any data it does not depend on order and is safe with NaN.

Every quantity is an integer or a maximum: any order of reduction gives the same bits.

sample_formats.power_domain_ok(a)  <=>  negative == 0 and hist[1248:].sum() == 0  (domain_ok below; tests/test_level_cpu.py).

The rail counters of a report (rail_lo, rail_hi, over) are counted on the INPUT codes, not on power samples: rails() below.
"""
from __future__ import annotations

import numpy as np

BINS = 2048
RUN = 28                      # power samples per envelope float: a lane's run in the kernels
BIN_ONE = 1016                # 1.0
BIN_DOMAIN_END = 1248         # 2^29: the first bin outside the _power calls' domain
BIN_NONFINITE = 2040          # Inf, and every NaN above it


def level_report(a) -> dict:
    a = np.ascontiguousarray(a)
    if a.dtype != np.dtype("<f4"):
        raise ValueError(f"power samples are float32, not {a.dtype}")
    b = a.reshape(-1).view("<u4")
    m = b.size
    minus = (b >> 31).astype(bool)
    hist = np.bincount((b[~minus] >> 20).astype(np.int64), minlength=BINS).astype(np.uint64)
    clear = np.where(minus, np.uint32(0), b)
    runs = -(-m // RUN)
    padded = np.zeros(runs * RUN, dtype=np.uint32)
    padded[:m] = clear
    env = padded.reshape(runs, RUN).max(axis=1).astype("<u4").view("<f4") if runs else np.zeros(0, dtype=np.float32)
    return dict(samples=m, negative=int(minus.sum()), rail_lo=0, rail_hi=0, over=0, hist=hist, env=env)


def bin_lower_edge(k: int) -> float:
    """The smallest float of bin k (k < 2040: finite)."""
    return float(np.array([int(k) << 20], dtype="<u4").view("<f4")[0])


def percentile(hist, q: float) -> float:
    """The lower edge of the bin that holds the q-quantile (0 <= q <= 1) of the sign-clear samples: the first bin at which the
    running count reaches q of the total, and at least one sample."""
    hist = np.asarray(hist, dtype=np.uint64)
    if hist.shape != (BINS,):
        raise ValueError("a histogram has 2048 bins")
    if not 0.0 <= q <= 1.0:
        raise ValueError("q lies in [0, 1]")
    total = int(hist.sum())
    if total == 0:
        raise ValueError("an empty histogram has no percentile")
    need = max(1, int(np.ceil(q * total)))
    return bin_lower_edge(int(np.searchsorted(np.cumsum(hist), need, side="left")))


def domain_ok(report: dict) -> bool:
    """The verdict sample_formats.power_domain_ok gives on the array, from its report."""
    return report["negative"] == 0 and int(np.asarray(report["hist"])[BIN_DOMAIN_END:].sum()) == 0


def rails(x, kind: str) -> tuple:
    """(rail_lo, rail_hi, over) of a capture's input codes.  kind "real": x uint16 codes, == 0, == 4095, > 4095, counted over EVERY
    sample of a capture that has power samples -- the trailing n % 4 codes make no power sample (the reference reads four at a
    time) but they are samples of the capture all the same; a capture below four samples has no power sample and an all-zero
    report.  "iq16" / "iq8": x int16 / int8 scalars of complex samples: == the format's minimum, == its maximum; over 0."""
    x = np.asarray(x).reshape(-1)
    if kind == "real":
        if x.size < 4:
            return 0, 0, 0
        return int((x == 0).sum()), int((x == 4095).sum()), int((x > 4095).sum())
    lo, hi = {"iq16": (-32768, 32767), "iq8": (-128, 127)}[kind]
    return int((x == lo).sum()), int((x == hi).sum()), 0


def with_rails(report: dict, x, kind: str) -> dict:
    """level_report's dict with the input's rail counters filled in: what the call of that flavour reports."""
    r = dict(report)
    r["rail_lo"], r["rail_hi"], r["over"] = rails(x, kind)
    return r


ZERO = dict(samples=0, negative=0, rail_lo=0, rail_hi=0, over=0)


def zero_report() -> dict:
    """The report of no samples: the identity of add()."""
    return dict(ZERO, hist=np.zeros(BINS, dtype=np.uint64))


def add(r: dict, s: dict) -> dict:
    """The sum of two reports, field by field (adsb_level_add): every field is a count, so the reports of the windows of a stream
    add up to the report of their union.  An envelope is not a report's to add: the sum has none."""
    out = {k: int(r[k]) + int(s[k]) for k in ZERO}
    out["hist"] = np.asarray(r["hist"], dtype=np.uint64) + np.asarray(s["hist"], dtype=np.uint64)
    return out


def check_edges(edges) -> list:
    """The edges of K consecutive windows, e[0] <= e[1] <= ... <= e[K]: every edge but the last is a multiple of 28, so a run of 28
    never spans two windows."""
    e = [int(v) for v in edges]
    if not e:
        raise ValueError("K windows have K + 1 edges")
    if any(b < a for a, b in zip(e, e[1:])):
        raise ValueError("the edges must ascend")
    if any(v % RUN for v in e[:-1]):
        raise ValueError("every edge but the last is a multiple of 28")
    return e


def level_windows(a, x, edges) -> tuple:
    """The statement of adsb_level_windows.  `a`: the power samples of a stream of uint16 real samples `x`, indexed from the
    stream's start (the reference's ampbuff, what adsb_power_window writes; for a buffer that starts at first_sample: the power
    samples of the stream with x[:first_sample] replaced by 2048).  Window i is power samples [e[i], e[i + 1]).

    -> (reports, env).  reports[i] = level_report(a[e[i]:e[i + 1]]) without its envelope, the rail counters counted on the codes the
    window owns, x[2 e[i] : 2 e[i + 1]] (== 0, == 4095, > 4095) -- a stream's trailing n % 4 codes belong to no window; an empty
    window has a zeroed report.  env: ONE envelope for all windows, env[r] over power samples
    [e[0] + 28 r, min(e[0] + 28 r + 28, e[K])), defined as in level_report -- that of a[e[0]:e[K]]."""
    e = check_edges(edges)
    a = np.ascontiguousarray(a).reshape(-1)
    x = np.asarray(x).reshape(-1)
    if e[-1] > a.size or 2 * e[-1] > x.size:
        raise ValueError("the last edge lies beyond the stream")
    reports = []
    for lo, hi in zip(e, e[1:]):
        r = level_report(a[lo:hi])
        del r["env"]
        own = x[2 * lo:2 * hi]
        r["rail_lo"], r["rail_hi"], r["over"] = int((own == 0).sum()), int((own == 4095).sum()), int((own > 4095).sum())
        reports.append(r)
    return reports, level_report(a[e[0]:e[-1]])["env"]


# ---- the gate behind the envelope: an envelope's bursts (adsb_bursts_device, csrc/burst_kernel.hip) ----
BURST_DTYPE = np.dtype([("begin", "<u4"), ("end", "<u4"), ("hot", "<u4"), ("peak", "<f4")])   # adsb_burst; [begin, end) in runs of 28
BURST_RUN_LIMIT = 1 << 30     # the most lead or hang may be


def _burst_args(env, threshold, lead, hang):
    env = np.ascontiguousarray(env)
    if env.dtype != np.dtype("<f4"):
        raise ValueError(f"an envelope is float32, not {env.dtype}")
    t = np.array([threshold], dtype="<f4")
    tb = int(t.view("<u4")[0])
    if np.isnan(t[0]) or tb >> 31:
        raise ValueError("the threshold is a float with the sign bit clear, and no NaN")
    lead, hang = int(lead), int(hang)
    if not (0 <= lead <= BURST_RUN_LIMIT and 0 <= hang <= BURST_RUN_LIMIT):
        raise ValueError("lead and hang lie in [0, 2^30]")
    b = env.reshape(-1).view("<u4")
    return np.where(b >> 31, np.uint32(0), b).astype(np.uint32), tb, lead, hang


def bursts(env, threshold, lead, hang) -> np.ndarray:
    """The bursts of an envelope of R floats: the statement adsb_bursts_device is held to, record for record.

    u[r] = the bit pattern of env[r] if its sign bit is clear, else 0 (the envelope's own rule, level_report); run r is HOT iff
    u[r] >= bits(threshold), compared as unsigned 32-bit integers -- NaN and Inf are hot at any finite threshold, +0.0 makes every
    run hot, no float is compared.  join = lead + hang + 1: the hot runs in ascending order, cut wherever two neighbours differ by
    more than join; a piece with first hot run s and last hot run e is one burst
        begin = max(0, s - lead)    end = min(R, e + hang + 1), exclusive    hot = the hot runs in [s, e]
        peak  = the float whose bits are the maximum of u over them
    -> a structured array (BURST_DTYPE), ascending; two neighbours always have a run between them."""
    u, tb, lead, hang = _burst_args(env, threshold, lead, hang)
    r = u.size
    h = np.flatnonzero(u >= np.uint32(tb)).astype(np.int64)
    out = np.zeros(0, dtype=BURST_DTYPE)
    if h.size == 0:
        return out
    cut = np.flatnonzero(np.diff(h) > lead + hang + 1) + 1
    first = np.concatenate(([0], cut))
    last = np.concatenate((cut, [h.size])) - 1
    out = np.zeros(first.size, dtype=BURST_DTYPE)
    out["begin"] = np.maximum(0, h[first] - lead)
    out["end"] = np.minimum(r, h[last] + hang + 1)
    out["hot"] = last - first + 1
    out["peak"] = np.maximum.reduceat(u[h], first).astype("<u4").view("<f4")
    return out


# ---- the gate of a slice of a stream (adsb_bursts_slice_*, csrc/burst_slice_kernel.hip) ----
# adsb_burst_carry: what the slices so far leave to the next one.  runs: the runs they covered; open: a cluster is open, and then
# its first and last hot run (stream runs), its hot count and its peak.  Zeroed: the start of a stream.
BURST_CARRY_DTYPE = np.dtype([("runs", "<u8"), ("open", "<u4"), ("first", "<u4"), ("last", "<u4"), ("hot", "<u4"), ("peak", "<f4"), ("reserved", "<u4")])
BURST_STREAM_RUNS = 1 << 31   # a stream's runs stay below this


def burst_carry() -> np.ndarray:
    """A zeroed carry, the start of a stream: one record of BURST_CARRY_DTYPE."""
    return np.zeros(1, dtype=BURST_CARRY_DTYPE)


def bursts_slice(env, threshold, lead, hang, carry, final):
    """The bursts that the next slice of a stream closes: the statement adsb_bursts_slice_device is held to -> (table, carry_out).

    The stream's runs count from 0 and `carry` says what the slices before left: run r of env is stream run carry.runs + r, hot by
    bursts()'s rule.  The carried cluster's hot runs (first .. last; only the two ends matter) followed by the slice's, as stream
    runs, are cut into clusters wherever two neighbours differ by more than join = lead + hang + 1 -- so the carried cluster and the
    slice's first hot run h0 are one cluster iff h0 - last <= join: the counts add, peak is the float of the larger bits.  A cluster
    with first hot run s and last hot run e is CLOSED iff final or e + join < carry.runs + R (every run that could still join it has
    been seen and was not hot), and is then the record
        begin = max(0, s - lead)    end = min(carry.runs + R, e + hang + 1)    hot    peak        in STREAM runs, ascending
    (the minimum binds under final only).  At most one cluster, the last, stays open: it is carry_out, carry_out.runs = carry.runs + R.
    A pure function: carry is not changed.  For one threshold, lead and hang the tables of consecutive calls, the last one final,
    concatenated, are bursts() of the concatenated envelope, however it is cut; threshold, lead and hang may also differ from
    call to call, and closing and merging then go by the current call's join."""
    u, tb, lead, hang = _burst_args(env, threshold, lead, hang)
    c = np.asarray(carry, dtype=BURST_CARRY_DTYPE).reshape(-1)
    if c.size != 1:
        raise ValueError("a carry is one record of BURST_CARRY_DTYPE")
    c = c[0]
    runs, join = int(c["runs"]), lead + hang + 1
    seen = runs + u.size
    if seen >= BURST_STREAM_RUNS:
        raise ValueError("a stream's runs stay below 2^31")
    h = runs + np.flatnonzero(u >= np.uint32(tb)).astype(np.int64)
    cut = np.flatnonzero(np.diff(h) > join) + 1
    lo = np.concatenate(([0], cut)) if h.size else np.zeros(0, dtype=np.int64)
    hi = (np.concatenate((cut, [h.size])) - 1) if h.size else np.zeros(0, dtype=np.int64)
    s, e, hot = h[lo], h[hi], hi - lo + 1
    peak = np.maximum.reduceat(u[h - runs], lo).astype(np.uint32) if h.size else np.zeros(0, dtype=np.uint32)
    if c["open"]:
        first, last, chot, cpeak = int(c["first"]), int(c["last"]), int(c["hot"]), np.uint32(np.array([c["peak"]], dtype="<f4").view("<u4")[0])
        if not (first <= last < runs and chot >= 1):
            raise ValueError("an open carry has first <= last < runs and hot >= 1")
        if h.size and h[0] - last <= join:
            s, hot, peak = s.copy(), hot.copy(), peak.copy()
            s[0], hot[0], peak[0] = first, hot[0] + chot, max(peak[0], cpeak)
        else:
            s, e, hot = np.concatenate(([first], s)), np.concatenate(([last], e)), np.concatenate(([chot], hot))
            peak = np.concatenate((np.array([cpeak], dtype=np.uint32), peak))
    out = burst_carry()
    out["runs"] = seen
    n = s.size
    if n and not final and e[-1] + join >= seen:
        n -= 1
        out["open"], out["first"], out["last"], out["hot"] = 1, s[n], e[n], hot[n]
        out["peak"] = peak[n:n + 1].view("<f4")[0]
    table = np.zeros(n, dtype=BURST_DTYPE)
    table["begin"] = np.maximum(0, s[:n] - lead)
    table["end"] = np.minimum(seen, e[:n] + hang + 1)
    table["hot"] = hot[:n]
    table["peak"] = peak[:n].view("<f4")
    return table, out


def burst_samples(bursts, M: int) -> np.ndarray:
    """The bursts of an envelope of M power samples, in power samples: an (B, 2) int64 array of [28 begin, min(28 end, M))."""
    b = np.asarray(bursts)
    out = np.empty((b.size, 2), dtype=np.int64)
    out[:, 0] = RUN * b["begin"].astype(np.int64)
    out[:, 1] = np.minimum(RUN * b["end"].astype(np.int64), int(M))
    return out
