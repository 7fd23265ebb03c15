"""The long_stream fixture (tests/golden/long_stream/, minted by oracle/make_golden.py through the real reference chain): a
stream of 2^32 - 4 samples that is silence -- code 2048, a zero FIR input, so zero power, no preamble pass, no Try -- but for
three bursts of signal whose samples are committed.  b1 straddles sample 2^31, b2 lies at 3 * 2^30, b3 ends at the stream's
last sample, across the end-of-file horizon.

The shift rule ties a burst to a short stand-in: decode(silence(F) ++ y ++ silence(S)) equals decode(silence(F mod 28) ++ y
++ silence(S)) with g and ts moved by (F - F mod 28) / 2 and the same Try/Ok table, as long as S keeps the end-of-file
horizon in silence (28 samples: the FIR ring's 14 phases times the sign flip of every other pair, air.c:59-92)."""
import json
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "long_stream")
N = (1 << 32) - 4
SILENCE = 2048
TAIL = 42181                      # ADSB_TAIL_OFFSETS
SILENCE_AFTER = 2 * TAIL + 4096   # samples of silence behind a burst that keep the horizon out of its reach
SPAN = {7: 80 + 80 * 7, 14: 80 + 80 * 14}   # power samples a frame of 7 / 14 bytes jumps over (demod.c:128-134)


def load():
    """(expected json, {burst name: (first_sample, uint16 samples)}, {df18: run})."""
    with open(os.path.join(DIR, "expected.json")) as f:
        rec = json.load(f)
    z = np.load(os.path.join(DIR, rec["input"]))
    bursts = {b["name"]: (b["first_sample"], z[b["name"]]) for b in rec["bursts"]}
    for b in rec["bursts"]:
        assert bursts[b["name"]][1].size == b["n_samples"]
    runs = {}
    for run in rec["runs"]:
        run["stats"] = {k: {int(d): v for d, v in run["stats"][k].items()} for k in run["stats"]}
        runs[run["df18"]] = run
    return rec, bursts, runs


def records(run, burst=None):
    return [(f["g"], f["ts"], f["pw"], bytes.fromhex(f["frame"])) for f in run["frames"] if burst in (None, f["burst"])]


def padded(first_sample, y, after=SILENCE_AFTER, lead=None):
    """silence(lead, default first_sample mod 28) ++ y ++ silence(after), and the shift (first_sample - lead) / 2 that
    takes its offsets to the stream's."""
    r = first_sample % 28 if lead is None else lead
    assert (first_sample - r) % 28 == 0
    x = np.concatenate([np.full(r, SILENCE, np.uint16), y, np.full(after, SILENCE, np.uint16)])
    return x, (first_sample - r) // 2


def shifted(frames, shift, ts_shift=None):
    """Records of restatement frames moved to the stream: g by `shift`, ts by `ts_shift` (default: the same)."""
    ts_shift = shift if ts_shift is None else ts_shift
    return [(f["g"] + shift, f["ts"] + ts_shift, f["pw"], bytes(f["frame"])) for f in frames]


def add_stats(a, b):
    return {k: {d: a[k][d] + b[k][d] for d in a[k]} for k in a}


def pieces(bursts, silence):
    """(first_sample, array) of the whole stream in order: every burst, `silence` (all 2048) repeated between them."""
    at = 0
    for s, y in sorted(bursts.values(), key=lambda b: b[0]) + [(N, None)]:
        while at < s:
            k = min(silence.size, s - at)
            yield at, silence[:k]
            at += k
        if y is not None:
            yield at, y
            at += y.size
    assert at == N
