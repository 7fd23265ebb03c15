"""make_golden_iq.py -- TEST INFRASTRUCTURE ONLY: mints tests/golden/iq/* (complex captures; the _iq calls of the library).

    python tools/make_golden_iq.py          # needs oracle/_ref (oracle.build_ref()), as oracle/make_golden.py does

For every case it writes <input>.npz (x: int16 of shape (n, 2) = I, Q) and <name>.json (expected records, keys as in
tests/golden/*.json; n_samples counts complex samples).  How the expectation is produced:

  x --> a = adsbdec_amd.sample_formats.iq_power(x): the library's definition of the power samples, in numpy
    --> oracle/_ref/ref_adsbdec [-a] -p a.f32 = the REAL deqframe / getdf / getabyte (demod.c), validShort / validLong (valid.c,
        crc.h), formatpkt (output.c) and print_stats, fed power samples two at a time through the harness's carry loop
    --> frames, ts, pw, AVR / AVR-MLAT / Beast bytes, Try/Ok table.

Nothing is written unless the restatement (oracle.demod_power) gives the same records one by one; g is the restatement's and is
checked against the reference's ts.  The fixtures live in the subdirectory: the top level of tests/golden is listed as uint16
cases.  The generator's digests go to tests/golden/iq/generator_digests.json.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd.sample_formats import iq_power  # noqa: E402
from tools import gen_signal as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "iq")
HORIZON = 40980   # ADSB_APBUFFSZ: deqframe runs once this many power samples are in


def _planted(rng, starts, dfs, amp):
    return [(int(s), G.make_frame(dfs[i % len(dfs)], rng), float(rng.uniform(*amp)), float(rng.uniform(0, 2 * np.pi)))
            for i, s in enumerate(starts)]


def cases():
    """(name, input name, x, df18)"""
    # ~30 DF11/17/18 frames, amplitude 100-1500 ADC units, sigma = 4
    rng = np.random.default_rng(101)
    n = 1 << 17
    starts = np.cumsum(rng.integers(1300, 7000, size=31))
    x = G.iq_synth(n, _planted(rng, starts[starts < n - 1300], (17, 11, 18), (100.0, 1500.0)), 4.0, 101)
    yield "mixed_df_a", "mixed_df", x, True
    yield "mixed_df_noa", "mixed_df", x, False
    # sigma = 1 ADC LSB on the ADC's own grid (multiples of 16), noise only: a handful of power values, so a quarter of the
    # a[m] > a[m+5] comparisons are exact ties and the preamble's c > 2 c' tests meet equal sums -- the strict inequalities
    x = (16 * np.rint(np.random.default_rng(102).normal(0.0, 1.0, size=(1 << 17, 2)))).astype(np.int16)
    a = iq_power(x)
    assert 0.15 < float(np.mean(a[:-5] == a[5:])) < 0.35
    yield "ties_noise", "ties_noise", x, True
    # wide-band noise, sigma = 300 ADC units
    x = G.iq_synth(100_000, [], 300.0, 103)
    yield "wide_noise", "wide_noise", x, True
    # full scale: frames at amplitude 2047 ADC units on either axis and both, and the value -32768 (pw up to ~4.2 M)
    rng = np.random.default_rng(104)
    fr = [(3000 + 2600 * k, G.make_frame((17, 11, 18)[k % 3], rng), 2047.0, phi)
          for k, phi in enumerate((0.0, np.pi / 2, np.pi, -np.pi / 2, 0.0, np.pi, np.pi / 2, np.pi))]
    x = G.iq_synth(48_000, fr, 2.0, 104)
    for k, both in ((5, False), (7, True)):   # frame 5 (phase pi): I pinned to the most negative int16; frame 7: I and Q both
        env = G.iq_frame_envelope(fr[k][1])
        seg = x[fr[k][0]: fr[k][0] + env.size]
        seg[env > 0, 0] = -32768
        if both:
            seg[env > 0, 1] = -32768
    yield "full_scale", "full_scale", x, True
    # too short for deqframe ever to fire: 40 978 samples, nothing decoded
    rng = np.random.default_rng(105)
    x = G.iq_synth(40_978, _planted(rng, (2000, 9000, 20000), (17, 11, 17), (500.0, 900.0)), 4.0, 105)
    yield "too_short", "too_short", x, True
    # ragged: an odd number of samples just above one deqframe call, frames before, across and behind its horizon
    rng = np.random.default_rng(106)
    n = HORIZON + 2601
    x = G.iq_synth(n, _planted(rng, (1500, HORIZON - 1200 - 2300, HORIZON - 1200 - 600, HORIZON - 1200 + 50, HORIZON + 900, n - 700),
                               (17, 11, 18, 17, 11, 17), (400.0, 1200.0)), 4.0, 106)
    yield "ragged", "ragged", x, True


def generator_digests():
    """sha256 of what the IQ generator gives for fixed arguments (tests/test_iq_cpu.py recomputes them)."""
    x, truth = G.make_iq_workload(200_000, seed=5)
    h = hashlib.sha256(np.ascontiguousarray(x).tobytes())
    for s, fr in truth:
        h.update(f"{s}:{fr.hex()}".encode())
    return {"make_iq_workload(200000, seed=5)": h.hexdigest(),
            "iq_synth(4096, [], 300.0, 9)": hashlib.sha256(G.iq_synth(4096, [], 300.0, 9).tobytes()).hexdigest()}


def main():
    from oracle import oracle as O
    O.build()
    if not O.build_ref():
        raise SystemExit("oracle/_ref is not available: nothing written")
    os.makedirs(OUT, exist_ok=True)
    for name, input_name, x, df18 in cases():
        assert x.dtype == np.int16 and x.ndim == 2 and x.shape[1] == 2 and len(x) <= (1 << 17), name
        a = iq_power(x)
        rf, rstats = O.ref_demod(a, df18=df18)
        of, ostats = O.demod_power(a, df18=df18)
        if ostats != rstats or [(f["ts"], f["pw"], f["frame"]) for f in of] != [(f["ts"], f["pw"], f["frame"]) for f in rf]:
            raise SystemExit(f"{name}: the restatement and the reference disagree: nothing written")
        skipped = 0
        for r, o in zip(rf, of):   # g is the restatement's; tie it to the reference's ts
            assert r["ts"] == o["g"] + 1 - skipped, name
            skipped += (80 + 80 * len(r["frame"])) - 1
        rec = dict(
            name=name, input=input_name + ".npz", df18=df18, n_samples=int(len(x)),
            provenance="x: int16 (I, Q); a = iq_power(x) (adsbdec_amd/sample_formats.py); every record from the REAL reference "
                       "demodulator on a (oracle/_ref/ref_adsbdec -p: demod.c, valid.c, output.c formatpkt); g from the "
                       "restatement (oracle.demod_power), which agrees record for record, checked against the reference's ts",
            stats={k: {str(d): int(v) for d, v in rstats[k].items()} for k in rstats},
            frames=[dict(g=o["g"], ts=r["ts"], pw=r["pw"], frame=r["frame"].hex().upper(),
                         avr=r["avr"].decode(), mlat=r["mlat"].decode(), beast=r["beast"].hex().upper())
                    for r, o in zip(rf, of)],
        )
        np.savez_compressed(os.path.join(OUT, input_name + ".npz"), x=x)
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(rec, f, indent=0)
        print(f"{name}: {len(x)} samples, {len(rf)} frames, max pw {max([r['pw'] for r in rf], default=0)}, stats {rstats}")
    with open(os.path.join(OUT, "generator_digests.json"), "w") as f:
        json.dump(generator_digests(), f, indent=1)


if __name__ == "__main__":
    main()
