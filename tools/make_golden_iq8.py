"""make_golden_iq8.py -- TEST INFRASTRUCTURE ONLY: mints tests/golden/iq8/* (complex int8 captures; the _iq calls with fmt 8).

    python tools/make_golden_iq8.py         # needs oracle/_ref (oracle.build_ref()), as tools/make_golden_iq.py does

For every case it writes <input>.npz (x: int8 of shape (n, 2) = I, Q) and <name>.json (expected records, keys as in
tests/golden/iq/*.json; n_samples counts complex samples).  How the expectation is produced:

  x --> a = adsbdec_amd.sample_formats.iq_power(x, 8) = 256 (I^2 + Q^2): the power samples of the widened twin (I << 8, Q << 8)
    --> oracle/_ref/ref_adsbdec [-a] -p a.f32 = the REAL deqframe / getdf / getabyte (demod.c), validShort / validLong (valid.c,
        crc.h), formatpkt (output.c) and print_stats, fed power samples two at a time through the harness's carry loop
    --> frames, ts, pw, AVR / AVR-MLAT / Beast bytes, Try/Ok table.

Nothing is written unless the restatement (oracle.demod_power) gives the same records one by one; g is the restatement's and is
checked against the reference's ts.  Every capture is an int16 one of tools/gen_signal shifted right by 8 (an arithmetic shift:
sample_formats.to_int8_iq).  The generator's digests go to tests/golden/iq8/generator_digests.json.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd.sample_formats import INT8_IQ, iq_power, to_int8_iq  # noqa: E402
from tools import gen_signal as G  # noqa: E402
from tools.make_golden_iq import HORIZON, _planted  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "iq8")


def cases():
    """(name, input name, x, df18)"""
    # the quantised workload: ten frames in noise that falls below one int8 step, so a third of the a[m] > a[m+5] comparisons are ties
    x = to_int8_iq(G.make_iq_workload(100_000, seed=2)[0])[0]
    yield "workload_a", "workload", x, True
    yield "workload_noa", "workload", x, False
    # full scale: frames at amplitude 2047 ADC units on either axis and both, and the value -128 (a[m] up to 2^23)
    rng = np.random.default_rng(204)
    fr = [(3000 + 2600 * k, G.make_frame((17, 11, 18)[k % 3], rng), 2047.0, phi)
          for k, phi in enumerate((0.0, np.pi / 2, np.pi, -np.pi / 2, 0.0, np.pi, np.pi / 2, np.pi))]
    x = to_int8_iq(G.iq_synth(48_000, fr, 40.0, 204))[0]
    for k, both in ((5, False), (7, True)):   # frame 5 (phase pi): I pinned to the most negative int8; frame 7: I and Q both
        env = G.iq_frame_envelope(fr[k][1])
        seg = x[fr[k][0]: fr[k][0] + env.size]
        seg[env > 0, 0] = -128
        if both:
            seg[env > 0, 1] = -128
    yield "full_scale", "full_scale", x, True
    # ragged: an odd number of samples just above one deqframe call, frames before, across and behind its horizon
    rng = np.random.default_rng(206)
    n = HORIZON + 2601
    x = to_int8_iq(G.iq_synth(n, _planted(rng, (1500, HORIZON - 1200 - 2300, HORIZON - 1200 - 600, HORIZON - 1200 + 50, HORIZON + 900, n - 700),
                                         (17, 11, 18, 17, 11, 17), (400.0, 1200.0)), 20.0, 206))[0]
    yield "ragged", "ragged", x, True
    # too short for deqframe ever to fire: 40 978 samples, nothing decoded
    rng = np.random.default_rng(205)
    x = to_int8_iq(G.iq_synth(40_978, _planted(rng, (2000, 9000, 20000), (17, 11, 17), (500.0, 900.0)), 20.0, 205))[0]
    yield "too_short", "too_short", x, True
    # wide-band noise alone, sigma = 300 ADC units = 19 int8 steps
    x = to_int8_iq(G.iq_synth(100_000, [], 300.0, 203))[0]
    yield "noise", "noise", x, True


def generator_digests():
    """sha256 of what the generator gives for fixed arguments, quantised (tests/test_iq8_cpu.py recomputes them)."""
    x8, lost = to_int8_iq(G.make_iq_workload(100_000, seed=2)[0])
    return {"to_int8_iq(make_iq_workload(100000, seed=2))": hashlib.sha256(np.ascontiguousarray(x8).tobytes()).hexdigest(),
            "to_int8_iq(make_iq_workload(100000, seed=2)): inexact": int(lost),
            "to_int8_iq(iq_synth(4096, [], 300.0, 9))": hashlib.sha256(to_int8_iq(G.iq_synth(4096, [], 300.0, 9))[0].tobytes()).hexdigest()}


def main():
    from oracle import oracle as O
    O.build()
    if not O.build_ref():
        raise SystemExit("oracle/_ref is not available: nothing written")
    os.makedirs(OUT, exist_ok=True)
    for name, input_name, x, df18 in cases():
        assert x.dtype == np.int8 and x.ndim == 2 and x.shape[1] == 2 and len(x) <= 120_000, name
        a = iq_power(x, INT8_IQ)
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
            provenance="x: int8 (I, Q); a = iq_power(x, 8) = 256 (I^2 + Q^2) (adsbdec_amd/sample_formats.py); every record from the REAL "
                       "reference demodulator on a (oracle/_ref/ref_adsbdec -p: demod.c, valid.c, output.c formatpkt); g from the "
                       "restatement (oracle.demod_power), which agrees record for record, checked against the reference's ts",
            stats={k: {str(d): int(v) for d, v in rstats[k].items()} for k in rstats},
            frames=[dict(g=o["g"], ts=r["ts"], pw=r["pw"], frame=r["frame"].hex().upper(),
                         avr=r["avr"].decode(), mlat=r["mlat"].decode(), beast=r["beast"].hex().upper())
                    for r, o in zip(rf, of)],
        )
        np.savez_compressed(os.path.join(OUT, input_name + ".npz"), x=x)
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(rec, f, indent=0)
        ties = float(np.mean(a[:-5] == a[5:])) if len(a) > 5 else 0.0
        print(f"{name}: {len(x)} samples, {len(rf)} frames, max pw {max([r['pw'] for r in rf], default=0)}, ties {ties:.3f}, stats {rstats}")
    with open(os.path.join(OUT, "generator_digests.json"), "w") as f:
        json.dump(generator_digests(), f, indent=1)


if __name__ == "__main__":
    main()
