"""Pins the oracle's restatement against the REAL reference chain, executed.

oracle/_ref/ref_adsbdec is the reference's own code -- air.c:29-101 (fbuff/fidx,
dsfilter, ampbuff/aidx, decodeiq), demod.c, valid.c (+ crc.h) and output.c's
formatpkt -- compiled from /root/reference by oracle/Makefile, fed by a read loop
shaped like fileInput (air.c:217-246).  oracle/_ref/ref_power is the same decodeiq
with a recording deqframe behind it.  These tests run both on uint16 captures and
require the restatement (oracle/adsb_oracle.c) to agree bit for bit on

  * every power sample                                   (air.c:54-92),
  * every accepted frame's bytes, ts and pw              (demod.c:84-143, valid.c),
  * the Try/Ok table                                     (valid.c:84-100),
  * the AVR / AVR-MLAT / Beast renderings                (output.c:204-262),

over > 2000 seeded captures: all seven FIR phases, full-range noise, codes beyond
12 bits, lengths around the first deqframe call (81 960 samples) and the EOF horizon
(SURVEY Q10), ragged tails (len % 4 != 0), frames planted across the
call horizons so that the carry base turns odd, with and without -a.

Where oracle/_ref is absent (it is built only where the reference sources are at hand),
the chain's answers on these very captures come from tests/golden/ref_recordings.json.gz,
recorded through it by oracle/make_ref_recordings.py; power samples are compared by
sha256 of their bits.
"""
import numpy as np
import pytest

from tools import gen_signal as G
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not O.ref_answers_available(), reason="neither oracle/_ref nor its recorded answers are here")

FIRST_CALL = 2 * 40980          # input samples at which aidx first reaches APBUFFSZ (air.c:94)
N_GROUPS, PER_GROUP = 16, 130   # 2080 captures


def key(fs):
    return [(f["ts"], f["pw"], f["frame"]) for f in fs]


def fuzz_capture(seed):
    """-> (x uint16, df18).  Small captures (1-4 deqframe calls) so thousands run in a minute."""
    rng = np.random.default_rng(seed)
    kind = int(rng.integers(0, 8))
    base = int(rng.choice([FIRST_CALL, 2 * FIRST_CALL, 3 * FIRST_CALL, int(rng.integers(60_000, 330_000))]))
    n = max(28, base + int(rng.choice([-8, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 8, 2400, 2404, 4000])))
    df18 = bool(rng.integers(0, 2))
    if kind == 0:                       # silence / constant code
        return np.full(n, int(rng.integers(0, 4096)), np.uint16), df18
    if kind == 1:                       # full-range uniform noise: ~7 % of offsets pass the preamble test
        return rng.integers(0, int(rng.choice([4096, 12000, 30000])), n, dtype=np.uint16), df18
    sigma = float(rng.choice([0.0, 3.0, 8.0, 30.0, 120.0, 300.0, 900.0]))
    frames = []
    nf = int(rng.integers(1, max(2, n // 3000)))
    for _ in range(nf):
        f = bytearray(G.make_frame(int(rng.choice([11, 17, 18])), rng))
        if rng.random() < 0.25:         # damaged: CRC rejects, Try without Ok
            k = int(rng.integers(0, 8 * len(f)))
            f[k >> 3] ^= 0x80 >> (k & 7)
        frames.append([int(rng.integers(0, max(1, n - 2400))), bytes(f),
                       float(rng.uniform(40, 2000)), float(rng.uniform(0, 6.28))])
    if kind == 2:                       # packed back to back: greedy skip lands exactly on the next preamble
        for i, fr in enumerate(frames):
            fr[0] = 5_000 + (2_400 if len(fr[1]) == 14 else 1_280) * i
    if kind in (3, 4):                  # frames around the T-1200 horizons of the first calls: the scan
        for i, fr in enumerate(frames):  # returns mid-frame or past it, and the carry base turns odd
            call = 1 + i % 3
            fr[0] = 2 * (40980 * call - 1200) + int(rng.integers(-2500, 200))
    if kind == 5:                       # near the end of the capture (the EOF horizon)
        for fr in frames:
            fr[0] = max(0, n - int(rng.integers(2400, 90_000)))
    frames = [tuple(fr) for fr in frames if 0 <= fr[0] < n - 200]
    return G.synth(n, frames, sigma, int(rng.integers(0, 1 << 30))), df18


@pytest.mark.parametrize("group", range(N_GROUPS))
def test_restatement_equals_real_chain_fuzz(oracle, group):
    seen_frames = 0
    for seed in range(group * PER_GROUP, (group + 1) * PER_GROUP):
        x, df18 = fuzz_capture(seed)
        rf, rstats = oracle.ref_decode(x, df18)
        of, ostats = oracle.decode(x, df18)
        assert key(of) == key(rf), f"seed {seed}: frames differ ({len(of)} vs {len(rf)})"
        assert ostats == rstats, f"seed {seed}: Try/Ok differ"
        if seed % 4 == 0:
            a = oracle.power(x)
            m = x.size // 4 * 2     # a ragged tail's last pair is stale-buffer arithmetic in the reference
            assert oracle.ref_power_digest(x, m=m) == (a.size, oracle.power_digest(a, m)), f"seed {seed}: power samples differ"
        for f, r in zip(of[:8], rf[:8]):
            assert oracle.formatpkt(f["frame"], f["ts"], f["pw"], 0) == r["avr"]
            assert oracle.formatpkt(f["frame"], f["ts"], f["pw"], 1) == r["mlat"]
            assert oracle.formatpkt(f["frame"], f["ts"], f["pw"], 2) == r["beast"]
        seen_frames += len(rf)
    assert seen_frames > 100       # the group did decode things


def test_power_bit_exact_all_phases_and_full_range(oracle):
    """air.c:54-92 alone: every uint16 code, every one of the 7 ring phases, chunked
    reads of several sizes (state carried in the reference's statics across calls)."""
    rng = np.random.default_rng(77)
    for hi, n in ((4096, 28 * 3000), (65536, 28 * 3000 + 4), (4096, 4 * 40980 + 12)):
        x = rng.integers(0, hi, n, dtype=np.uint16)
        want = oracle.power(x)
        for chunk in (None, 4, 28, 4096, 65536 + 4):
            assert oracle.ref_power_digest(x, chunk) == (want.size, oracle.power_digest(want)), (hi, n, chunk)
    # the 7 summation orders really differ (otherwise the test above proves less than it says)
    x = rng.integers(0, 4096, 28 * 50, dtype=np.uint16)
    a = oracle.power(x)
    shifted = oracle.power(np.concatenate([np.full(4, 2048, np.uint16), x]))[2:]
    assert not np.array_equal(a[7:], shifted[7:a.size])


@pytest.mark.parametrize("df18", [False, True])
def test_chunked_reads_do_not_change_the_real_chain(oracle, df18):
    """The reference's statics make decodeiq a stream: 1 Mi-sample reads (fileInput)
    and tiny reads give the same frames.  This is what adsb_push has to reproduce."""
    x, _ = G.dense_capture(3 << 17, seed=21, sigma=50.0, n_frames=150)
    want = oracle.ref_decode(x, df18)
    for chunk in (4, 4096, 40980 * 2 - 4, 1 << 17):
        assert oracle.ref_decode(x, df18, chunk=chunk) == want
    assert (key(want[0]), want[1]) == (key(oracle.decode(x, df18)[0]), oracle.decode(x, df18)[1])


def test_first_call_boundary_lengths(oracle):
    """A frame well inside the first 39 780 offsets decodes iff the capture reaches
    81 960 samples (aidx >= APBUFFSZ fires, air.c:94); one sample pair less and the
    reference prints nothing."""
    rng = np.random.default_rng(5)
    fr = G.make_frame(17, rng)
    for n in range(FIRST_CALL - 8, FIRST_CALL + 9):
        x = G.synth(n, [(20_000, fr, 900.0, 0.4)], 5.0, 3)
        rf, rstats = oracle.ref_decode(x, False)
        of, ostats = oracle.decode(x, False)
        assert key(of) == key(rf) and ostats == rstats, n
        # n = 81957..81959: the reference's loop runs one more pass on the ragged quad
        assert (len(rf) == 1) == (n > FIRST_CALL - 4), n


def test_native_flags_vs_strict(oracle):
    """SURVEY Q3, measured on the REAL slice: the reference's own flags (-O3
    -march=native, contraction allowed) against the strict build every parity claim
    here is made for.  Frames and Try/Ok must agree on this capture; pw may differ by
    one unit on a few frames when the host fuses."""
    import os
    if O.ref_available() and not os.path.exists(O.REF_ADSBDEC_NATIVE):
        pytest.skip("native build absent")
    x, _ = G.dense_capture(1 << 21, seed=31, sigma=60.0, n_frames=800, amp=(100, 1800))
    try:
        nf, nstats = oracle.ref_decode(x, True, native=True)
    except Exception as e:  # -march=native objects built on another host
        pytest.skip(f"native build does not run here: {e}")
    sf, sstats = oracle.ref_decode(x, True)
    assert [(f["ts"], f["frame"]) for f in nf] == [(f["ts"], f["frame"]) for f in sf]
    assert nstats == sstats
    assert all(abs(a["pw"] - b["pw"]) <= 1 for a, b in zip(nf, sf))
