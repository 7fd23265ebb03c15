"""The cases of the gate behind the envelope (adsb_bursts_*; adsbdec_amd/levels.py bursts is the statement), shared by
tests/test_bursts_cpu.py and tests/test_gpu_bursts.py.  No GPU and no reference here: envelopes with hot runs where a tile's seam is
(T = adsb_burst_tile_runs() is handed in), the slow paint-and-merge wording of the definition, and the one fixture the defaults
of lead and hang rest on.

A case is (name, env, threshold, lead, hang): env a float32 array, everything else what levels.bursts takes."""
import functools

import numpy as np

THRESHOLD = 100.0


def envelope(R, hot, seed=0):
    """R floats: the runs of `hot` at or above THRESHOLD (the first of them exactly on it), the others below; all different enough
    that a wrong peak shows."""
    rng = np.random.default_rng([seed, R])
    env = rng.uniform(0.0, 99.0, R).astype("<f4")
    hot = np.asarray(hot, dtype=np.int64)
    env[hot] = rng.uniform(100.0, 1.0e6, hot.size).astype("<f4")
    if hot.size:
        env[hot[0]] = np.float32(THRESHOLD)
    return env


def paint_and_merge(env, threshold, lead, hang):
    """The other wording, slowly: paint [h - lead, h + hang] for every hot run h, take the maximal painted intervals (intervals that
    touch merge), and count the hot runs and their largest u inside each.  -> a list of (begin, end, hot, peak bits)."""
    b = np.ascontiguousarray(env, dtype="<f4").view("<u4")
    u = [0 if int(v) >> 31 else int(v) for v in b]
    tb = int(np.array([threshold], dtype="<f4").view("<u4")[0])
    R = len(u)
    painted = [False] * R
    for h in range(R):
        if u[h] >= tb:
            for r in range(max(0, h - lead), min(R, h + hang + 1)):
                painted[r] = True
    out, r = [], 0
    while r < R:
        if not painted[r]:
            r += 1
            continue
        e = r
        while e < R and painted[e]:
            e += 1
        hot = [u[k] for k in range(r, e) if u[k] >= tb]
        out.append((r, e, len(hot), max(hot)))
        r = e
    return out


def as_tuples(recs):
    """A structured array of bursts as paint_and_merge's list."""
    return [(int(b["begin"]), int(b["end"]), int(b["hot"]), int(np.array([b["peak"]], dtype="<f4").view("<u4")[0])) for b in recs]


LENGTHS = lambda T: (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 5, 40 * T + 3)


def length_cases(T):
    """Every length of the list: a tenth of the runs hot; the first and the last run hot; nothing hot."""
    out = []
    for R in LENGTHS(T):
        rng = np.random.default_rng([11, R])
        out.append((f"R={R} a tenth hot", envelope(R, np.flatnonzero(rng.random(R) < 0.1), 1), THRESHOLD, 1, 2))
        out.append((f"R={R} both ends hot", envelope(R, sorted({0, R - 1}), 2), THRESHOLD, 2, 3))
        out.append((f"R={R} nothing hot", envelope(R, [], 3), THRESHOLD, 2, 3))
    return out


def named_cases(T):
    R = 6 * T + 3
    lead, hang = 2, 3
    join = lead + hang + 1
    out = [("no hot run", envelope(R, []), THRESHOLD, lead, hang),
           ("every run hot", envelope(R, np.arange(R)), THRESHOLD, 1, 1),
           ("every run hot, nothing kept around", envelope(R, np.arange(R)), THRESHOLD, 0, 0)]
    for at, name in ((0, "0"), (R - 1, "R - 1"), (T - 1, "T - 1"), (T, "T")):
        out.append((f"a single hot run at {name}", envelope(R, [at]), THRESHOLD, lead, hang))
    out.append(("hot at T - 1 and T: one burst across the seam", envelope(R, [T - 1, T]), THRESHOLD, lead, hang))
    out.append(("hot at T - 1 and T - 1 + join: joined", envelope(R, [T - 1, T - 1 + join]), THRESHOLD, lead, hang))
    out.append(("hot at T - 1 and T + join: split", envelope(R, [T - 1, T + join]), THRESHOLD, lead, hang))
    # two hot tiles, three empty ones between them: the last hot run of tile 0 and the first of tile 4 are `apart` apart
    a, b = T - 5, 4 * T + 7
    apart = b - a
    hot = [3, 40, a, b, b + 1, 5 * T - 1]
    for j, what in ((apart, "join spans the three empty tiles: joined"), (apart - 1, "join one smaller: split")):
        out.append((f"two hot tiles, three empty between, {what}", envelope(R, hot), THRESHOLD, j // 2, j - 1 - j // 2))
    out.append(("lead and hang larger than R", envelope(100, [7, 60]), THRESHOLD, 1000, 5000))
    out.append(("lead and hang larger than R, several tiles", envelope(2 * T + 3, [5, T + 9, 2 * T]), THRESHOLD, 3 * T, 3 * T))
    out.append(("lead and hang at their limit", envelope(2 * T + 3, [5, T + 9, 2 * T]), THRESHOLD, 1 << 30, 1 << 30))
    rng = np.random.default_rng(12)
    some = np.flatnonzero(rng.random(R) < 0.02)
    out.append(("lead 0, hang 5", envelope(R, some), THRESHOLD, 0, 5))
    out.append(("lead 5, hang 0", envelope(R, some), THRESHOLD, 5, 0))
    return out


def alternating(T):
    """Every second run hot with lead = hang = 0: every hot run a burst of its own, the most bursts an envelope can have."""
    R = 5 * T + 1
    return ("every second run hot", envelope(R, np.arange(0, R, 2)), THRESHOLD, 0, 0)


VALUE_THRESHOLDS = (0.0, 1.0e-40, 1.0, float("inf"), 3.4028234663852886e38)


def value_env():
    """An array of the caller's own: NaN of both signs, Inf of both signs, -0.0, negative floats, subnormals, the largest finite
    float, among ordinary ones."""
    rng = np.random.default_rng(13)
    R = 5000
    env = rng.uniform(0.0, 4.0, R).astype("<f4")
    special = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x007FFFFF, 0x80000001,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001, 0x3F800000, 0xBF800000, 0x00011C71], dtype="<u4").view("<f4")
    where = rng.choice(R, size=40 * special.size, replace=False)
    env[where] = np.tile(special, 40)
    env.view("<u4")[rng.choice(R, size=300, replace=False)] ^= np.uint32(0x80000000)      # (the sign bit, whatever the float)
    return env


def random_cases(T, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        R = int(rng.integers(1, 40 * T + 1)) if i % 4 else int(rng.integers(1, 3 * T))
        density = float(rng.choice([0.0003, 0.003, 0.03, 0.3, 0.9]))
        lead, hang = (int(rng.choice([0, 1, 2, 5, 40, 3000])) for _ in range(2))
        out.append((f"random {i}: R={R} density={density} lead={lead} hang={hang}",
                    envelope(R, np.flatnonzero(rng.random(R) < density), i), THRESHOLD, lead, hang))
    return out


# ------------------------------------------------------------------ the pipeline fixture
# 36 frames -- short and long, amplitudes 40 .. 1500 against noise of sigma 1 -- planted in 6 000 000 complex int16 samples (0.6 s).
# The gate's threshold is FACTOR times the median power sample; LEAD and HANG are the host program's defaults.  HANG is 1468 and not
# the 4 first meant: a decode call keeps the reference's end-of-file horizon (deqframe runs only once 40 980 power samples are in),
# so a piece shorter than that decodes nothing -- with hang 4 every one of the 36 frames is lost.
# COVER: a burst around one frame is at most 2 + 43 + 1468 + 1 runs = 42 392 power samples, 36 of them 25.4 % of the capture when none
# overlap; the slices must stay below 40 %, which "one burst over everything" (100 %) cannot.
PIPE_N, PIPE_SEED, PIPE_FRAMES = 6_000_000, 7, 36
FACTOR, LEAD, HANG = 48.0, 2, 1468
COVER = 0.40


@functools.lru_cache(maxsize=None)
def pipeline():
    """-> dict: x (int16, (n, 2)), truth [(start, frame bytes)], a (the float32 power samples, sample_formats.iq_power), env, threshold,
    bursts (levels.bursts) and slices (levels.burst_samples)."""
    from tools import gen_signal
    from adsbdec_amd import levels, sample_formats
    x, truth = gen_signal.make_iq_workload(PIPE_N, seed=PIPE_SEED, n_frames=PIPE_FRAMES, sigma=1.0, amp=(40.0, 1500.0),
                                           dfs=(17, 17, 11, 11, 18, 17))
    a = np.ascontiguousarray(sample_formats.iq_power(x, 2))
    rep = levels.level_report(a)
    threshold = float(np.float32(FACTOR * levels.percentile(rep["hist"], 0.5)))
    b = levels.bursts(rep["env"], threshold, LEAD, HANG)
    for arr in (x, a, rep["env"], b):
        arr.setflags(write=False)
    return dict(x=x, truth=[(int(s), bytes(f)) for s, f in truth], a=a, report=rep, env=rep["env"], threshold=threshold, bursts=b,
                slices=levels.burst_samples(b, a.size))


_record = {}


def frames_per_burst(oracle):
    """The record: the oracle's decode (df18 on) of every slice, a list of (g, ts, pw, frame) per burst; computed once."""
    if "frames" not in _record:
        p = pipeline()
        _record["frames"] = [[(f["g"], f["ts"], f["pw"], f["frame"]) for f in oracle.demod_power(np.ascontiguousarray(p["a"][lo:hi]), df18=True)[0]]
                             for lo, hi in p["slices"]]
    return _record["frames"]
