"""The batch conversion's cases without a GPU (tests/batch_convert_cases.py): what tests/test_gpu_batch_convert.py rests on is
asserted here from the lengths and the numpy definition alone, so that no case of the GPU test is a vacuous one -- the second
grid trip, a chunk of 256 rows, every tail length, every element-aligned source residue, pads over another call's samples, the
two counter batches' counts -- and the kernel's row look-up (csrc/sample_format.h convert_row) compiled for the host."""
import os
import subprocess

import numpy as np
import pytest

import batch_convert_cases as B
from conftest import ROOT
from test_batch_cpu import offsets_of

IDS = [B.NAMES[c] for c in B.CONVS]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cases_afterwards():
    yield
    B.call.cache_clear()                                     # (two calls' sources and expectations: ~100 MiB)


@pytest.mark.parametrize("conv", B.CONVS, ids=IDS)
def test_the_patterns_reach_what_they_are_for(conv):
    per = B.PER[conv]
    scratch = None
    for k in range(len(B.CALLS)):
        b = B.call(conv, k)
        geo = B.geometry(b.scalars)
        what = (B.NAMES[conv], k, {key: v for key, v in geo.items() if key != "tails"})
        # the grid-stride loop's second trip: more chunks than blocks, and a second-trip chunk that starts in one capture and ends
        # in another
        assert geo["chunks"] > B.GRID and geo["groups"] > B.GRID * B.CHUNK, what
        assert geo["second_trip_straddles"], what
        # a chunk of 256 short groups of 256 different captures (r1 - r0 = 255: a lane searches among all of them)
        assert geo["rows_max"] == B.CHUNK and geo["short_chunks"] >= 1, what
        # every tail length behind whole groups, and alone
        assert geo["tails"] >= set(B.tails(conv)) and {n for n in b.scalars if n < 8} >= set(B.tails(conv)) | {0}, what
        # 255 / 256 / 257 groups, exact and ragged
        counts = [(n + 7) // 8 for n in b.scalars]
        for g in (255, 256, 257):
            assert any(c == g and n % 8 == 0 for c, n in zip(counts, b.scalars)) and any(c == g and n % 8 for c, n in zip(counts, b.scalars)), (what, g)
        assert b.n.count(0) >= 20 and len(b.n) >= 900, what
        # the captures that bring the groups up have no offset to scan; the decodable ones have
        units = [4 * (n // 2) if conv == B.F32_IQ else n for n in b.n]        # (what the batch scan counts for an IQ capture)
        assert sorted(i for i, u in enumerate(units) if offsets_of(u)) == sorted(b.frames) and len(b.frames) == 3, what
        assert max(n for i, n in enumerate(b.n) if i not in b.frames) == B.NO_OFFSETS // per, what
        # the sources: every multiple of the element size mod 16, element-only alignment included
        _, at = b.device_image()
        assert {a % 16 for a, n in zip(at, b.scalars) if n} == set(range(0, 16, B.ELEM[conv])), what
        assert all(a % B.ELEM[conv] == 0 for a in at)
        # the contents: off-grid and on-grid scalars in short groups and in whole ones; both counts (only floats clamp)
        assert b.n_off_grid(True) > 300 and b.n_off_grid(False) > 100_000, what
        assert b.n_off_grid(True) + b.n_off_grid(False) == b.inexact + b.clamped
        assert b.inexact > 100_000 and ((b.clamped > 100_000) if conv != B.S16 else b.clamped == 0), what
        short_on = sum(int((~o[s // 8 * 8:]).sum()) for s, o in zip(b.scalars, b.off_grid))
        assert short_on > 100, what
        for i in b.frames:                                   # the decodable captures stay on their grid
            assert not b.off_grid[i].any()
        assert b.report() == (sum(b.scalars), b.inexact, b.clamped)
        assert b.host_bytes() + b.device_image()[0].nbytes < 64 << 20, what
        # the scratch across the calls: the second fits the first one's, and its pads lie on the first one's non-zero samples
        if scratch is None:
            scratch = B.Scratch(b.total)
        else:
            assert b.total <= scratch.model.size
            n_pad = 0
            for i in range(len(b.n)):
                _, known, model = scratch.pad(b, i)
                n_pad += int(np.count_nonzero(known & (model != 0)))
            assert n_pad > 2000, (what, n_pad)
        scratch.write(b)
    assert B.call(conv, 0).scalars != B.call(conv, 1).scalars


@pytest.mark.parametrize("conv", B.CONVS, ids=IDS)
def test_the_counter_batches_have_the_counts_claimed(conv):
    """One batch has its off-grid scalars in short last groups only, the other in whole groups only; both count."""
    short, whole = B.counter_batch(conv, True), B.counter_batch(conv, False)
    for b, on_short in ((short, True), (whole, False)):
        assert b.n_off_grid(not on_short) == 0 and b.n_off_grid(on_short) == b.inexact + b.clamped, (B.NAMES[conv], on_short)
        assert b.inexact > 50 and ((b.clamped > 50) if conv != B.S16 else b.clamped == 0), (B.NAMES[conv], on_short, b.report())
        assert sum(1 for n in b.scalars if n % 8) > 100 and sum(1 for n in b.scalars if n >= 8) > 100
    assert short.report() != whole.report()


def test_expected_codes_are_the_definitions():
    """expected() is the three numpy definitions, the IQ scalars viewed as uint16, on a vector with every special value."""
    from adsbdec_amd import sample_formats as S
    rng = np.random.default_rng(1)
    for conv in B.CONVS:
        x = B.random_source(conv, 20_000, rng)
        codes, inexact, clamped = B.expected(conv, x)
        assert codes.dtype == np.uint16 and inexact.any() and (~inexact & ~clamped).any() and clamped.any() == (conv != B.S16)
        if conv == B.S16:
            assert np.array_equal(codes, S.from_int16_real(x)[0])
        elif conv == B.F32:
            assert np.array_equal(codes, S.from_float32_real(x)[0]) and np.isnan(x).any() and np.isinf(x).any()
        else:
            assert np.array_equal(codes.view(np.int16), S.to_int16_iq(x)[0]) and np.isnan(x).any() and np.isinf(x).any()
            fin = x[np.isfinite(x)].astype(np.float64) * 32768
            ties = np.abs(fin - np.floor(fin) - 0.5) == 0
            assert ties.sum() > 20                              # exact ties of the IQ grid (the edge vector)
        assert np.array_equal(B.expected(conv, B.on_grid(conv, rng, 4096))[1:], (np.zeros(4096, bool),) * 2)
    assert B.slots([0, 1, 64, 65, 0, 3]) == ([0, 0, 64, 128, 256, 256], 320)


def test_row_lookup_on_the_host(tmp_path):
    """csrc/sample_format.h convert_row and ConvertSeg -- what the kernel finds a group's capture with -- compiled for the host:
    captures of 1 .. 7 samples and of 2^29 groups side by side, every group around every capture boundary and random ones, looked
    up chunk-wise as the kernel does; 8 k < n always, and a short group only at a capture's end."""
    exe = tmp_path / "convert_rows"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "convert_rows.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 200 tables"), p.stdout + p.stderr
