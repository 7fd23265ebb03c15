"""The front end (air.c:54-92) across the wrap of its 32-bit sample counter, restated in numpy float32 with a 64-bit
sample number -- and the wrap_stream fixture (tests/golden/wrap_stream/, minted by tools/mint_wrap_stream.py through the
real reference chain): a stream of 7 * 2^32 + 2^21 samples that is silence (code 2048) but for nine committed bursts.

Power index g = w * 2^31 + r, r < 2^31: w is the epoch, P = w * 2^31 its first power sample.  The reference's `fidx` counts
input samples modulo 2^32, i.e. pairs modulo 2^31.  Pair q is written to ring slot pair slot(q) = (q mod 2^31) mod 7; the
output behind pair m uses tap offset c(m) = ((m + 1) mod 2^31) mod 7 (`o = 14 - fidx % 14` read AFTER the two increments):
slot pair i meets taps T[(2 i - 2 c) mod 14] and the next one, and the seven products are added in slot order i = 0 .. 6.
Inside an epoch that is the fresh-stream rule in r (order p, p-1, .., 0, 6, .., p+1 with p = r mod 7).  At a wrap the ring
is not cleared: slot pair i holds the LATEST pair q <= m with slot(q) = i, whichever epoch wrote it, so the outputs
P - 1 .. P + 5 (c wraps one output early; slots above r still hold the old epoch's pairs, in the old epoch's places) follow
neither epoch's formula.

Three modes:
  true          the rule above;
  stale_phase   epoch w computed with epoch w - 1's order: slot and c from q - (w - 1) 2^31 without a wrap (what a counter
                wider than 32 bits does);
  no_transient  each epoch by its own formula; P - 1 .. P + 5 by the NEW epoch's formula over a zeroed history (P - 1: no
                pair of the new epoch exists yet, zero power).
Power from the model goes through oracle.demod_power (demod.c / valid.c restated and pinned)."""
import json
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "wrap_stream")
E = 1 << 31                        # power samples (pairs) per epoch
N = 7 * (1 << 32) + (1 << 21)      # samples of the fixture's stream
SILENCE = 2048
TAIL = 42181                       # ADSB_TAIL_OFFSETS
SILENCE_AFTER = 2 * TAIL + 4096
SPAN = {7: 80 + 80 * 7, 14: 80 + 80 * 14}
MODES = ("true", "stale_phase", "no_transient")

_LIT = (0.012627, 0.025254, 0.037881, 0.050508, 0.063135, 0.075761, 0.088388,
        0.088388, 0.075761, 0.063135, 0.050508, 0.037881, 0.025254, 0.012627)   # air.c:36-45
TAPS = np.array(_LIT, dtype=np.float64).astype(np.float32)


def power(y, first_sample, mode="true", wrap=None):
    """Power samples of burst y (uint16, first_sample % 4 == 0, y.size % 4 == 0) behind silence: a[k] is power sample
    first_sample / 2 + k.  `wrap`: the epoch w whose start the modes stale_phase / no_transient get wrong (default: the
    epoch of the burst's last sample)."""
    y = np.asarray(y, dtype=np.uint16)
    assert first_sample % 4 == 0 and y.size % 4 == 0 and mode in MODES
    q0 = first_sample // 2
    n = y.size // 2
    w = (q0 + n - 1) // E if wrap is None else wrap
    B = w * E
    hist = 16
    q = np.arange(q0 - hist, q0 + n, dtype=np.int64)              # pairs, with silent history
    v = np.zeros((q.size, 2), np.float32)
    v[hist:] = y.astype(np.float32).reshape(-1, 2) - np.float32(2048.0)   # air.c:64,66
    v[q % 2 == 1] *= np.float32(-1.0)                              # air.c:79-82: every other pair negated
    if mode == "true":
        slot = (q % E) % 7
        seen = np.ones(q.size, bool)
        c_of = lambda m: ((m + 1) % E) % 7
    elif mode == "stale_phase":
        base = B - E if w >= 1 else 0
        slot = (q - base) % 7
        seen = np.ones(q.size, bool)
        c_of = lambda m: (m - base + 1) % 7
    else:
        slot = (q % E) % 7
        seen = np.ones(q.size, bool)
        c_of = lambda m: ((m + 1) % E) % 7
    m = q[hist:]
    idx = np.arange(hist, q.size)
    c = c_of(m)
    s = np.zeros((m.size, 2), np.float32)
    for i in range(7):
        src = np.full(m.size, -1, np.int64)
        for d in range(14):                                        # the latest pair <= m in slot pair i
            k = idx - d
            hit = (src < 0) & (slot[k] == i) & seen[k]
            if mode == "no_transient" and w >= 1:
                hit &= ~((m >= B) & (q[k] < B))                    # the new epoch starts over a zeroed ring
            src[hit] = k[hit]
        t = (2 * i - 2 * c) % 14
        val = np.where((src >= 0)[:, None], v[np.maximum(src, 0)], np.float32(0.0)).astype(np.float32)
        prod = np.stack([TAPS[t] * val[:, 0], TAPS[t + 1] * val[:, 1]], axis=1).astype(np.float32)   # air.c:72-73
        s = prod if i == 0 else (s + prod).astype(np.float32)
    a = (s[:, 0] * s[:, 0]).astype(np.float32) + (s[:, 1] * s[:, 1]).astype(np.float32)            # air.c:76,91
    a = a.astype(np.float32)
    if mode == "no_transient" and w >= 1:
        a[m == B - 1] = np.float32(0.0)
    return a


LEAD = 2048   # zero power samples in front of a burst's power (a multiple of 2)


def demod(a, first_sample, df18, after=SILENCE_AFTER // 2):
    """oracle.demod_power of zeros(LEAD) ++ a ++ zeros(after): (records [(g, ts - g, pw, frame)], stats) with g moved to the
    stream; ts is reported as ts - g (its shift against the stream is a constant per burst: the offsets jumped before)."""
    from oracle import oracle as O
    full = np.concatenate([np.zeros(LEAD, np.float32), a, np.zeros(after, np.float32)])
    frames, stats = O.demod_power(full, df18=df18, cap=1 << 16)
    shift = first_sample // 2 - LEAD
    return [(f["g"] + shift, f["ts"] - f["g"], f["pw"], bytes(f["frame"])) for f in frames], stats


def pack(rec):
    """The fixture's two files from the mint script's record: expected.json keeps what a reader wants to see (bursts, Try/Ok
    tables, provenance); the frames -- g, ts, pw, bytes, the reference's AVR-MLAT line -- go to records.npz as arrays, one
    set per run (a0: without -a, a1: with -a), and so does the prefix run's AVR-MLAT output."""
    names = [b["name"] for b in rec["bursts"]]
    arrays = {"prefix_mlat": np.frombuffer(rec["prefix"]["mlat"].encode(), np.uint8)}
    for run in rec["runs"]:
        k, fs = f"a{int(run['df18'])}_", run["frames"]
        fr = np.zeros((len(fs), 14), np.uint8)
        for i, f in enumerate(fs):
            b = bytes.fromhex(f["frame"])
            fr[i, : len(b)] = np.frombuffer(b, np.uint8)
        arrays.update({k + "g": np.array([f["g"] for f in fs], np.uint64), k + "ts": np.array([f["ts"] for f in fs], np.uint64),
                       k + "pw": np.array([f["pw"] for f in fs], np.uint32), k + "frame": fr,
                       k + "len": np.array([len(f["frame"]) // 2 for f in fs], np.uint8),
                       k + "burst": np.array([names.index(f["burst"]) for f in fs], np.uint8),
                       k + "mlat": np.frombuffer("".join(f["mlat"] for f in fs).encode(), np.uint8)})
    small = dict(rec, records="records.npz", runs=[dict(df18=r["df18"], stats=r["stats"], n_frames=len(r["frames"])) for r in rec["runs"]],
                 prefix={k: v for k, v in rec["prefix"].items() if k != "mlat"})
    return small, arrays


def unpack(small, z):
    """The inverse of pack(): the mint script's record."""
    names = [b["name"] for b in small["bursts"]]
    rec = dict(small, prefix=dict(small["prefix"], mlat=bytes(z["prefix_mlat"]).decode()), runs=[])
    for r in small["runs"]:
        k = f"a{int(r['df18'])}_"
        mlat = bytes(z[k + "mlat"]).decode().splitlines(keepends=True)
        assert len(mlat) == r["n_frames"] == z[k + "g"].size
        frames = [dict(burst=names[int(z[k + "burst"][i])], g=int(z[k + "g"][i]), ts=int(z[k + "ts"][i]), pw=int(z[k + "pw"][i]),
                       frame=bytes(z[k + "frame"][i, : int(z[k + "len"][i])]).hex().upper(), mlat=mlat[i]) for i in range(r["n_frames"])]
        rec["runs"].append(dict(df18=r["df18"], stats=r["stats"], frames=frames))
    return rec


def load():
    """(expected record, {burst name: (first_sample, uint16 samples, wrap or None)}, {df18: run})."""
    with open(os.path.join(DIR, "expected.json")) as f:
        small = json.load(f)
    rec = unpack(small, np.load(os.path.join(DIR, small["records"])))
    bursts = {}
    for b in rec["bursts"]:
        y = np.load(os.path.join(DIR, b["file"]))["y"]
        assert y.size == b["n_samples"]
        bursts[b["name"]] = (b["first_sample"], y, b["wrap"])
    runs = {}
    for run in rec["runs"]:
        run["stats"] = {k: {int(d): v for d, v in run["stats"][k].items()} for k in run["stats"]}
        runs[run["df18"]] = run
    return rec, bursts, runs


def records(run, burst=None):
    return [(f["g"], f["ts"], f["pw"], bytes.fromhex(f["frame"])) for f in run["frames"] if burst in (None, f["burst"])]


def pieces(bursts, silence, total=N):
    """(first_sample, array) of the stream's first `total` samples in order: every burst, `silence` repeated between."""
    at = 0
    for s, y, _ in sorted(bursts.values(), key=lambda b: b[0]) + [(total, None, None)]:
        if s >= total:
            s, y = total, None
        while at < s:
            k = min(silence.size, s - at)
            yield at, silence[:k]
            at += k
        if y is not None:
            assert at + y.size <= total
            yield at, y
            at += y.size
        if at >= total:
            break
    assert at == total


# ---- the restatement (oracle/adsb_oracle.c) started just below a wrap: orc_state_t is a public struct ----------------------
def _state_type():
    import ctypes as C
    from oracle import oracle as O

    class OrcState(C.Structure):   # oracle/adsb_oracle.h orc_state_t
        _fields_ = [("ring", C.c_float * 14), ("fidx", C.c_uint32), ("ampbuff", C.c_float * (40980 + 4)), ("aidx", C.c_uint32),
                    ("df", C.c_int), ("fix1", C.c_int), ("stat_fixed", C.c_uint32), ("ts", C.c_uint64),
                    ("stat_try", C.c_uint32 * 32), ("stat_ok", C.c_uint32 * 32), ("gbase", C.c_uint64),
                    ("n_deq_calls", C.c_uint64), ("sink", C.c_void_p), ("sink_user", C.c_void_p)]
    return OrcState, C.CFUNCTYPE(None, C.c_void_p, C.POINTER(O.OrcFrame))


STANDIN_LEAD = 4096   # samples of silence in front of the burst (a multiple of 4)


def standin(y, first_sample, df18, fix1=False, after=SILENCE_AFTER):
    """silence(STANDIN_LEAD) ++ y ++ silence(after) through orc_decode_buffer from a state whose fidx, gbase and ts are those
    of a stream that was silence up to sample first_sample - STANDIN_LEAD: (records [(g, ts, pw, frame)], stats).  The ring
    and ampbuff of such a stream hold zeros, as orc_init leaves them; ts - g is what a stream with no earlier frame has."""
    import ctypes as C
    from oracle import oracle as O
    L = O.lib()
    State, Sink = _state_type()
    start = first_sample - STANDIN_LEAD
    assert start % 4 == 0 and start >= 0
    got = []
    sink = Sink(lambda user, f: got.append((int(f[0].g), int(f[0].ts), int(f[0].pw), bytes(f[0].frame[: f[0].len]))))
    st = State()
    L.orc_init.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.orc_init.restype = None
    L.orc_decode_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.orc_decode_buffer.restype = None
    L.orc_init(C.byref(st), int(df18), C.cast(sink, C.c_void_p), None)
    st.fix1 = 1 if fix1 else 0
    st.fidx = start % (1 << 32)
    st.gbase = start // 2
    st.ts = start // 2
    x = np.concatenate([np.full(STANDIN_LEAD, SILENCE, np.uint16), np.asarray(y, np.uint16), np.full(after, SILENCE, np.uint16)])
    L.orc_decode_buffer(C.byref(st), x.ctypes.data, x.size)
    stats = {"try": {11: st.stat_try[11], 17: st.stat_try[17], 18: st.stat_try[18]},
             "ok": {11: st.stat_ok[11], 17: st.stat_ok[17], 18: st.stat_ok[18]}}
    if fix1:
        stats["fixed"] = int(st.stat_fixed)
    return got, stats
