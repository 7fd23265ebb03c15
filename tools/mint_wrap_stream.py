"""Mints tests/golden/wrap_stream/: a stream of 7 * 2^32 + 2^21 samples, silence (code 2048) but for nine bursts, piped whole
into the REAL reference chain (oracle/_ref/ref_adsbdec through oracle.ref_decode_pieces), with and without -a; and the
stream's first 2^32 + 2^21 samples once more with -a, for the C host program's test (its end-of-file horizon is its own).

    python tools/mint_wrap_stream.py            # needs oracle/_ref (oracle/Makefile ref)

Time on the machine that minted the committed files: 289 s, of which 247 s for the three reference runs side by side (each
of the two long ones reads 3.0e10 samples through a pipe: 35 s per epoch) behind the seed search; expected.json keeps the figures of the last minting.

Bursts (every start a multiple of 8; tests/wrap_model.py explains the epochs):
  w1 .. w7  across the wrap into epoch w = 1 .. 7 (all seven ring phases; epoch 7 has epoch 0's again).  Frames back to back,
            short and long, of varied amplitude, from the burst's start to its end; the greedy chain runs across P = w 2^31:
              Y  an intact short frame decoded at P - 635 (P - 636 where the chain arrives an offset early): its bit 55
                 compares a[P - 5] with a[P] (a[P - 6] with a[P - 1]): data bits on the transient samples P - 1 .. P + 5;
              D  a DF17 with ONE bit flipped decoded at P + 5, back to back behind Y: its preamble test reads a[P + 5] (a
                 Try, no Ok for the reference; with the 1-bit repair a frame whose pw reads the transient); g = P + 5 is the
                 last of the seam offsets [P - 1196, P + 5];
              the chain goes on at P + 1204 or P + 1205.
            (An accepted frame with its preamble on the transient AND another with data bits there cannot both be visited:
            they overlap.  D is the visited preamble, Y the accepted data bits.)
  mid       in the interior of epoch 4, 2^20 samples and more from any wrap.
  end       ends at the stream's last sample, across the end-of-file horizon (epoch 7).

Sensitivity is a condition of the fixture (tests/wrap_model.py, modes stale_phase and no_transient): for every wrap burst,
with and without -a, each wrong model must differ from the true one in a frame field or a Try count.  The seed of a burst
is searched until that holds; after the reference has run, the true model and the restatement's stand-in must both
reproduce the reference's records of every burst exactly, or nothing is written."""
from __future__ import annotations

import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import gen_signal as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
import wrap_model as W  # noqa: E402

SIGMA = 3.0
PREFIX = (1 << 32) + (1 << 21)


def _frame(rng, df, damaged=False):
    fr = bytearray(G.make_frame(df, rng))
    if damaged:
        k = int(rng.integers(5, 112))
        fr[k >> 3] ^= 0x80 >> (k & 7)
    return bytes(fr), float(rng.uniform(150.0, 1850.0)), float(rng.uniform(0, 2 * np.pi))


def _chain(rng, n):
    """n frames for a back-to-back run: (df, samples taken)."""
    out = []
    for _ in range(n):
        df = (11, 11, 11, 11, 17, 18)[int(rng.integers(0, 6))]
        out.append((df, 1280 if df == 11 else 2400))
    return out


def wrap_burst(w, seed, n_before=60, n_after=170):
    rng = np.random.default_rng(1000 * w + seed)
    before, after = _chain(rng, n_before), _chain(rng, n_after)
    y_at, d_at = 2 - 1280, 2                      # relative to the wrap sample: decoded 4 power samples later
    lead = sum(n for _, n in before) - y_at + 400
    lead += (-lead) % 8 + 8 * w                   # the start a multiple of 8, another residue mod 28 per wrap
    frames = []
    at = lead + y_at
    for df, n in reversed(before):
        at -= n
        frames.append((at, *_frame(rng, df)))
    frames.append((lead + y_at, *_frame(rng, 11)))
    frames.append((lead + d_at, *_frame(rng, 17, damaged=True)))
    at = lead + d_at + 2400
    for df, n in after:
        frames.append((at, *_frame(rng, df)))
        at += n
    n_samples = at + 400
    n_samples += (-n_samples) % 8
    y = G.synth(n_samples, frames, SIGMA, 1000 * w + seed)
    return w * (1 << 32) - lead, y


def plain_burst(seed, n_frames, first_sample=None, end=None):
    rng = np.random.default_rng(seed)
    frames, at = [], 600
    for df, n in _chain(rng, n_frames):
        frames.append((at, *_frame(rng, df, damaged=int(rng.integers(0, 8)) == 0 and df == 17)))
        at += n + int(rng.integers(0, 3)) * 700
    n_samples = at + 8 - at % 8
    if end is not None:     # ends at `end`: the last frames lie across the end-of-file horizon, the very last one is cut off
        first_sample = end - n_samples
    return first_sample, G.synth(n_samples, frames, SIGMA, seed)


def sensitive(w, first_sample, y):
    for df18 in (False, True):
        true = W.demod(W.power(y, first_sample, "true"), first_sample, df18)
        for mode in W.MODES[1:]:
            if W.demod(W.power(y, first_sample, mode, wrap=w), first_sample, df18) == true:
                return False
    return True


def bursts():
    out = []
    for w in range(1, 8):
        for seed in range(64):
            s, y = wrap_burst(w, seed)
            if sensitive(w, s, y):
                break
        else:
            raise SystemExit(f"no seed makes burst w{w} sensitive to both wrong models")
        print(f"w{w}: seed {seed}, {y.size} samples at {s} (mod 28: {s % 28})", flush=True)
        out.append((f"w{w}", s, y, w))
    s, y = plain_burst(77, 120, first_sample=4 * (1 << 32) + (1 << 31) + 8 * 12345)
    out.append(("mid", s, y, None))
    s, y = plain_burst(78, 150, end=W.N)
    out.append(("end", s, y, None))
    out.sort(key=lambda b: b[1])
    for name, s, y, _ in out:
        assert s % 8 == 0 and y.size % 8 == 0 and y.dtype == np.uint16 and y.max() <= 4095, name
    return out


def main():
    if not O.build_ref():
        raise SystemExit("oracle/_ref is not available")
    t0 = time.time()
    bs = bursts()
    by_name = {name: (s, y, w) for name, s, y, w in bs}
    silence = np.full(1 << 26, W.SILENCE, np.uint16)
    runs = {}

    def run(key, df18, total):
        runs[key] = O.ref_decode_pieces((x for _, x in W.pieces(by_name, silence, total)), df18=df18)

    th = [threading.Thread(target=run, args=a) for a in ((False, False, W.N), (True, True, W.N), ("prefix", True, PREFIX))]
    t1 = time.time()
    for t in th:
        t.start()
    for t in th:
        t.join()
    ref_s = time.time() - t1
    out = []
    for df18 in (False, True):
        rf, rstats = runs[df18]
        skipped, gs = 0, []
        for r in rf:                     # g from the reference's own ts (demod.c:86,99,128,134)
            gs.append(r["ts"] - 1 + skipped)
            skipped += (80 + 80 * len(r["frame"])) - 1
        where = []
        for g in gs:
            hit = [name for name, s, y, _ in bs if s // 2 <= g < (s + y.size) // 2]
            assert len(hit) == 1, g
            where.append(hit[0])
        total = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
        jumped = 0
        for name, s, y, w in bs:
            mine = [(g, r["ts"], r["pw"], r["frame"]) for g, r, wh in zip(gs, rf, where) if wh == name]
            assert len(mine) > 20, (name, len(mine))
            if name != "end":            # (the last burst lies across the end-of-file horizon: the whole-stream run alone says)
                mf, mstats = W.demod(W.power(y, s, "true"), s, df18)
                assert [(g, d + g - jumped, pw, fr) for g, d, pw, fr in mf] == mine, f"{name}: the true model differs from the reference"
                sf, sstats = W.standin(y, s, df18)
                assert [(g, ts - jumped, pw, fr) for g, ts, pw, fr in sf] == mine, f"{name}: the stand-in differs from the reference"
                assert sstats == mstats
                for k in total:
                    for d in total[k]:
                        total[k][d] += mstats[k][d]
            jumped += sum(W.SPAN[len(fr)] - 1 for _, _, _, fr in mine)
        for d in (11, 17, 18):           # what is left of the table is the last burst's
            assert 0 <= rstats["try"][d] - total["try"][d] and 0 < rstats["ok"][11] - total["ok"][11]
        out.append(dict(
            df18=df18, stats={k: {str(d): int(v) for d, v in rstats[k].items()} for k in rstats},
            frames=[dict(burst=wh, g=g, ts=r["ts"], pw=r["pw"], frame=r["frame"].hex().upper(), mlat=r["mlat"].decode())
                    for g, r, wh in zip(gs, rf, where)]))
        print(f"wrap_stream df18={df18}: {len(rf)} frames, stats {rstats}", flush=True)
    pf, pstats = runs["prefix"]
    rec = dict(
        name="wrap_stream", n_samples=W.N, silence=W.SILENCE, minted_in_s=round(time.time() - t0), reference_runs_s=round(ref_s),
        bursts=[dict(name=name, first_sample=s, n_samples=int(y.size), wrap=w, file=name + ".npz") for name, s, y, w in bs],
        provenance="every record from the REAL reference chain (oracle/_ref/ref_adsbdec) run over the whole stream, fed through a "
                   "pipe; g from the reference's ts; every burst but the last also equal to tests/wrap_model.py's true model and "
                   "to the restatement started just below the wrap",
        runs=out,
        prefix=dict(n_samples=PREFIX, df18=True, stats={k: {str(d): int(v) for d, v in pstats[k].items()} for k in pstats},
                    mlat="".join(r["mlat"].decode() for r in pf)))
    os.makedirs(W.DIR, exist_ok=True)
    for name, s, y, _ in bs:
        np.savez_compressed(os.path.join(W.DIR, name + ".npz"), y=y)
    small, arrays = W.pack(rec)          # (the frames as arrays in records.npz: 3 400 records are no reading matter)
    assert W.unpack(small, arrays) == dict(rec, records="records.npz")
    np.savez_compressed(os.path.join(W.DIR, "records.npz"), **arrays)
    with open(os.path.join(W.DIR, "expected.json"), "w") as f:
        json.dump(small, f, indent=1)
    print(f"minted in {time.time() - t0:.0f} s (reference runs: {ref_s:.0f} s)")


if __name__ == "__main__":
    main()
