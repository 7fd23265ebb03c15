"""make_golden.py -- TEST INFRASTRUCTURE ONLY: mints tests/golden/*.

Run in the build container (needs /root/reference for oracle/_ref):

    python oracle/make_golden.py

For every case it writes <name>.npz (the uint16 input) and <name>.json (expected
records).  How the expectation is produced, precisely:

  input x (uint16 file) --> oracle/_ref/ref_adsbdec = the REAL reference code,
      compiled from /root/reference by oracle/Makefile and executed here:
      decodeiq + ampbuff carry (air.c:29-101) -> deqframe/getdf/getabyte (demod.c)
      -> validShort/validLong/CrcStep/CrcEnd/print_stats (valid.c, crc.h)
      -> formatpkt (output.c), behind a fileInput-shaped read loop (air.c:217-246)
  --> frames, ts, pw, AVR / AVR-MLAT / Beast bytes, Try/Ok table.

Nothing in a fixture comes from the restatement except `g` (the preamble's power-
sample index, which the reference never materialises): the script asserts that the
restatement's records equal the reference's and that g is consistent with the
reference's ts through ts = g + 1 - sum(span - 1) (demod.c:86,99,128,134).
The reference's own tests hold no vectors for this path; the
public CRC known answers it cites are in crc_kat.json.

long_stream/ (`python oracle/make_golden.py long_stream` mints it alone, in about a
minute): a stream of 2^32 - 4 samples, silence but for three bursts whose samples are
committed (bursts.npz); the reference reads the whole stream through a pipe, and its
records and Try/Ok table, with and without -a, are in expected.json.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_signal as G  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def cases():
    # BASELINE.json configs[0]: 1 Mi samples, ~100 DF17, the reference's own CPU case
    x, _ = G.sparse_capture(1 << 20, 100, seed=1)
    yield "config1_1Mi_100xDF17", "config1_1Mi_100xDF17", x, False
    # mixed DF11/17/18 with -a, frames back to back and overlapping, moderate noise
    x, _ = G.dense_capture(3 * (1 << 17), seed=7, sigma=40.0, n_frames=120, amp=(300, 1800))
    yield "mixed_df_a_384Ki", "mixed_df_384Ki", x, True
    # same input without -a: DF18 must vanish from Try and Ok
    yield "mixed_df_noa_384Ki", "mixed_df_384Ki", x, False
    # config-3 flavour: wide-band noise, ~7 % of offsets pass the preamble test
    x, _ = G.dense_capture(1 << 18, seed=11, sigma=300.0, n_frames=30)
    yield "dense_noise_256Ki", "dense_noise_256Ki", x, True
    # ragged length (not a multiple of 4) just above the first deqframe call
    x, _ = G.sparse_capture(4 * 40980 // 2 + 4 * 1300 + 3, 6, seed=13, dfs=(17, 11))
    yield "ragged_tail", "ragged_tail", x, True
    # too short for deqframe ever to fire: no output at all
    x, _ = G.sparse_capture(81000, 5, seed=17)
    yield "too_short", "too_short", x, False
    # frames across the first calls' T-1200 horizons: deqframe returns mid-buffer after a
    # jump, so the carry base turns odd (air.c:94-99); length % 4 == 1
    rng = np.random.default_rng(23)
    frames = [(2 * (40980 * c - 1200) + d, G.make_frame(df, rng), 900.0, 0.3 * c)
              for c, d, df in ((1, -2300, 17), (1, 2601, 11), (2, -1101, 18), (2, 1501, 17), (3, -2399, 11),
                               (3, 201, 17), (4, -301, 18))]
    x = G.synth(5 * 81960 + 4 * 300 + 1, frames, 6.0, 23)
    yield "odd_carry_base_a", "odd_carry_base", x, True
    # codes beyond 12 bits (still inside the domain where the reference's float->int is defined)
    x = np.random.default_rng(29).integers(0, 30000, 3 * 81960 + 2, dtype=np.uint16)
    yield "wide_codes_noise", "wide_codes_noise", x, True


# ---- long_stream: 2^32 - 4 samples, silence (code 2048: zero FIR input, zero power) but for three bursts of signal ----------
LONG_N = (1 << 32) - 4
LONG_DIR = os.path.join(OUT, "long_stream")
SILENCE = 2048
TAIL = 42181                  # offsets at the end of a stream that the last deqframe call may leave unread (ADSB_TAIL_OFFSETS)
SILENCE_AFTER = 2 * TAIL + 4096   # samples of silence behind a burst that keep the end-of-file horizon out of its reach


def _planted(starts, dfs, rng, damage=False):
    out = []
    for i, st in enumerate(starts):
        fr = bytearray(G.make_frame(dfs[i % len(dfs)], rng))
        if damage and len(fr) == 14 and i % 2 == 0:       # one bit of a long frame flipped: a Try, no Ok (1-bit repair: fixed)
            k = int(rng.integers(5, 112))
            fr[k >> 3] ^= 0x80 >> (k & 7)
        out.append((int(st), bytes(fr), float(rng.uniform(500.0, 1500.0)), float(rng.uniform(0, 2 * np.pi))))
    return out


def long_stream_bursts():
    """[(name, first_sample, uint16 samples)] of the long_stream case.  Every start is a multiple of 8 (packed input);
    b1 and b2 start at different non-zero residues mod 28 (the FIR phase), b3 ends at the stream's last sample."""
    half = 1 << 17
    # b1: 256 Ki samples centred on sample 2^31 (power sample 2^30), frames on both sides and across it
    s1 = (1 << 31) - half
    rng = np.random.default_rng(41)
    fr = _planted(range(1500, half - 2900, 2900), (17, 11, 18), rng) + \
        _planted([half - 1100, half + 1400, half + 3800, half + 6200], (17, 11, 18, 17), rng) + \
        _planted(range(half + 9000, 2 * half - 3000, 3100), (17, 11, 18), rng)
    b1 = G.synth(2 * half, fr, 8.0, 41)
    # b2: 128 Ki samples at 3 * 2^30, frames back to back, then one-bit-damaged long frames
    s2 = 3 * (1 << 30) - (1 << 16) + 8
    rng = np.random.default_rng(42)
    fr = _planted(range(2000, 60000, 2400), (17, 18, 11), rng) + \
        _planted(range(62000, half - 3000, 2700), (17, 18), rng, damage=True)
    b2 = G.synth(half, fr, 8.0, 42)
    # b3: up to the last sample, frames before, across and after the end-of-file horizon, the last one cut off by the end
    n3 = 196612
    s3 = LONG_N - n3
    rng = np.random.default_rng(43)
    b3 = G.synth(n3, _planted(list(range(1800, n3 - 2400, 2600)) + [n3 - 1000], (17, 11, 18), rng), 8.0, 43)
    return [("b1", s1, b1), ("b2", s2, b2), ("b3", s3, b3)]


def long_stream_pieces(bursts, silence):
    """The stream in order: the bursts, and `silence` (an all-2048 array) repeated in between."""
    at = 0
    for _, s, b in bursts + [("end", LONG_N, np.zeros(0, np.uint16))]:
        while at < s:
            k = min(silence.size, s - at)
            yield silence[:k]
            at += k
        yield b
        at += b.size
    assert at == LONG_N


def padded(first_sample, b, after=SILENCE_AFTER):
    """The shift rule's short stand-in for a burst at `first_sample` behind silence: first_sample mod 28 samples of
    silence, the burst, silence after.  Its offsets are the stream's minus (first_sample - first_sample mod 28) / 2."""
    r = first_sample % 28
    return np.concatenate([np.full(r, SILENCE, np.uint16), b, np.full(after, SILENCE, np.uint16)]), (first_sample - r) // 2


def mint_long_stream():
    import threading
    bursts = long_stream_bursts()
    for name, s, b in bursts:
        assert s % 8 == 0 and b.max() <= 4095 and b.dtype == np.uint16, name
    assert bursts[0][1] % 28 != bursts[1][1] % 28 and bursts[0][1] % 28 and bursts[1][1] % 28
    assert bursts[-1][1] + bursts[-1][2].size == LONG_N
    silence = np.full(1 << 26, SILENCE, np.uint16)
    runs = {}

    def run(df18):
        runs[df18] = O.ref_decode_pieces(long_stream_pieces(bursts, silence), df18=df18)

    th = [threading.Thread(target=run, args=(df18,)) for df18 in (False, True)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    out = []
    for df18 in (False, True):
        rf, rstats = runs[df18]
        skipped, gs = 0, []
        for r in rf:                     # g from the reference's own ts (demod.c:86,99,128,134)
            gs.append(r["ts"] - 1 + skipped)
            skipped += (80 + 80 * len(r["frame"])) - 1
        where = []
        for g in gs:
            w = [name for name, s, b in bursts if s // 2 <= g < (s + b.size) // 2]
            assert len(w) == 1, g
            where.append(w[0])
        # b1 and b2 under the shift rule, through the restatement and the real chain on short stand-ins: the same records
        for name, s, b in bursts[:2]:
            x, shift = padded(s, b)
            of, ostats = O.decode(x, df18=df18)
            lf, lstats = O.ref_decode(x, df18=df18)
            assert ostats == lstats, name
            assert [(f["ts"], f["pw"], f["frame"]) for f in of] == [(f["ts"], f["pw"], f["frame"]) for f in lf], name
            mine = [(g, r["pw"], r["frame"], r["avr"]) for g, r, w in zip(gs, rf, where) if w == name]
            assert mine == [(o["g"] + shift, o["pw"], o["frame"], lr["avr"]) for o, lr in zip(of, lf)], name
            assert len(mine) > 10, name
        assert sum(w == "b3" for w in where) > 10
        out.append(dict(
            df18=df18,
            stats={k: {str(d): int(v) for d, v in rstats[k].items()} for k in rstats},
            frames=[dict(burst=w, g=g, ts=r["ts"], pw=r["pw"], frame=r["frame"].hex().upper(), avr=r["avr"].decode(),
                         mlat=r["mlat"].decode(), beast=r["beast"].hex().upper()) for g, r, w in zip(gs, rf, where)]))
        print(f"long_stream df18={df18}: {len(rf)} frames, stats {rstats}")
    rec = dict(
        name="long_stream", n_samples=LONG_N, silence=SILENCE, input="bursts.npz",
        bursts=[dict(name=name, first_sample=s, n_samples=int(b.size)) for name, s, b in bursts],
        provenance="every record from the REAL reference chain (oracle/_ref/ref_adsbdec) run once over the whole stream of "
                   "2^32 - 4 samples, fed through a pipe; g from the reference's ts, and for b1 and b2 equal to the shift rule's "
                   "g through the restatement and through the real chain on short stand-ins",
        runs=out)
    os.makedirs(LONG_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(LONG_DIR, "bursts.npz"), **{name: b for name, _, b in bursts})
    with open(os.path.join(LONG_DIR, "expected.json"), "w") as f:
        json.dump(rec, f, indent=0)


def main():
    if not O.build_ref():
        raise SystemExit("oracle/_ref is not available (needs /root/reference)")
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["long_stream"]:
        mint_long_stream()
        return
    for name, input_name, x, df18 in cases():
        rf, rstats = O.ref_decode(x, df18=df18)
        of, ostats = O.decode(x, df18=df18)
        assert ostats == rstats, (name, ostats, rstats)
        assert [(f["ts"], f["pw"], f["frame"]) for f in of] == [(f["ts"], f["pw"], f["frame"]) for f in rf], name
        skipped = 0
        for r, o in zip(rf, of):   # g is the restatement's; tie it to the reference's ts
            assert r["ts"] == o["g"] + 1 - skipped, name
            skipped += (80 + 80 * len(r["frame"])) - 1
        rec = dict(
            name=name, input=input_name + ".npz", df18=df18, n_samples=int(x.size),
            provenance="every record from the REAL reference chain executed on the uint16 input "
                       "(oracle/_ref/ref_adsbdec: air.c:29-101 decodeiq, demod.c, valid.c, output.c "
                       "formatpkt, compiled from /root/reference); g from the restatement, checked "
                       "against the reference's ts",
            stats={k: {str(d): int(v) for d, v in rstats[k].items()} for k in rstats},
            frames=[dict(g=o["g"], ts=r["ts"], pw=r["pw"], frame=r["frame"].hex().upper(),
                         avr=r["avr"].decode(), mlat=r["mlat"].decode(), beast=r["beast"].hex().upper())
                    for r, o in zip(rf, of)],
        )
        np.savez_compressed(os.path.join(OUT, input_name + ".npz"), x=x)
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(rec, f, indent=0)
        print(f"{name}: {x.size} samples, {len(rf)} frames, stats {rstats}")

    # CRC known answers the survey verified through the reference's crc.h
    kat = dict(
        source="public DF17 frames with residual 0 and a DF11 with residual F8740F (SURVEY.md section 4)",
        vectors=[
            dict(frame="8D4840D6202CC371C32CE0576098", residual="000000"),
            dict(frame="8D40621D58C382D690C8AC2863A7", residual="000000"),
            dict(frame="5D4840D6000000", residual="F8740F"),
        ],
        table_first8=["000000", "FFF409", "001C1B", "FFE812", "003836", "FFCC3F", "00242D", "FFD024"],
        table_last=["FA0480"],
    )
    with open(os.path.join(OUT, "crc_kat.json"), "w") as f:
        json.dump(kat, f, indent=1)
    mint_long_stream()


if __name__ == "__main__":
    main()
