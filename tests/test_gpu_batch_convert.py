"""The batch conversion kernel held to its definition word for word (run with -m gpu on an MI355X): what convert_batch_kernel
(csrc/convert_samples.hip) leaves in the handle's scratch for EVERY capture of an adsb_decode_batch_*_as call and of an
adsb_decode_batch_*_iq call with fmt 0, read back through adsb_batch_unpacked_copy, against the numpy definition
(adsbdec_amd/sample_formats.py); the pads behind the captures, which no kernel writes; the two counters, exactly; and the frames
of the few captures that have any.  The cases are tests/batch_convert_cases.py's; tests/test_batch_convert_cpu.py asserts that
they reach the second grid trip, a chunk of 256 rows, every tail length and every element-aligned source address.  Every
comparison is exact.

The other tests of a converted batch (test_gpu_sample_formats.py, test_gpu_iq.py) see its frames and the sum of its counters."""
import numpy as np
import pytest

import batch_convert_cases as B
from conftest import records

# measured on an MI355X (profiles/r18_batch_convert_tests.txt): 0.33 - 0.45 s for a word-for-word test (the cases made, two
# uploads, ~3 500 copies of a slot back), 0.04 s for the counter batches, 2.1 s of pytest for the file
pytestmark = [pytest.mark.gpu, pytest.mark.limit(120)]

IDS = [B.NAMES[c] for c in B.CONVS]
ZERO = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cases_afterwards():
    yield
    B.call.cache_clear()                                     # (two calls' sources and expectations: ~100 MiB)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture()
def decoders(capi, torch_cuda):
    made = []

    def make(**kw):
        d = capi.Decoder(**kw)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


def upload(torch, batch):
    """The captures of a batch side by side in ONE device buffer, every capture at an address aligned to its element and skewed
    off the 16-byte boundaries in turn (batch_convert_cases.device_offsets).  -> (the tensor that keeps it, pointers)."""
    host, at = batch.device_image()
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, [t.data_ptr() + a if n else 0 for a, n in zip(at, batch.scalars)]


def decode_device(d, batch, ptrs):
    if batch.conv == B.F32_IQ:
        return d.decode_batch_device_iq(0, ptrs, batch.n, stats=True)
    return d.decode_batch_device_as(batch.conv, ptrs, batch.n, stats=True)


def decode_host(d, batch):
    if batch.conv == B.F32_IQ:
        return d.decode_batch_iq(0, batch.src, stats=True)
    return d.decode_batch_as(batch.conv, batch.src, stats=True)


def reference_frames(ref, batch):
    """{capture index: (records, Try/Ok table)} of the decodable captures: the uint16 (IQ: int16) batch call on the numpy codes."""
    idx = sorted(batch.frames)
    for i in idx:                                            # the raw twin IS the numpy codes of the capture: it lies on its grid
        assert np.array_equal(batch.frames[i].reshape(-1).view(np.uint16), batch.codes[i]), i
    raw = [batch.frames[i] for i in idx]
    frames, stats = ref.decode_batch_iq(2, raw, stats=True) if batch.conv == B.F32_IQ else ref.decode_batch(raw, stats=True)
    assert sum(len(f) for f in frames) > 20 and all(len(f) > 0 for f in frames)
    return {i: (records(f), s) for i, f, s in zip(idx, frames, stats)}


def check_scratch(d, batch, scratch, what):
    """Every capture's samples are the numpy codes; every pad sample the model knows is the model's.  -> known non-zero pad samples."""
    n_pad = 0
    for i, (n, codes) in enumerate(zip(batch.scalars, batch.codes)):
        slot, known, model = scratch.pad(batch, i)
        got = d.batch_unpacked(i, slot)
        if not np.array_equal(got[:n], codes):
            bad = np.nonzero(got[:n] != codes)[0]
            raise AssertionError((what, "capture", i, "of", n, "scalars: first wrong sample", int(bad[0]), "of", bad.size,
                                  "got", int(got[bad[0]]), "want", int(codes[bad[0]])))
        assert np.array_equal(got[n:][known], model[known]), (what, "pad of capture", i, n)
        n_pad += int(np.count_nonzero(known & (model != 0)))
    return n_pad


def check_frames(batch, want, frames, stats, what):
    assert len(frames) == len(stats) == len(batch.n)
    for i in range(len(batch.n)):
        if i in want:
            assert (records(frames[i]), stats[i]) == want[i], (what, i)
        else:                                                # no offset to scan (air.c:94)
            assert frames[i] == [] and stats[i] == ZERO, (what, i, batch.n[i])


@pytest.mark.parametrize("conv", B.CONVS, ids=IDS)
def test_batch_conversion_word_for_word(capi, torch_cuda, decoders, conv):
    """Two calls with different capture patterns on ONE handle (~1 100 captures each: runs of captures of one short group, captures of
    1 .. 40 scalars, 255 / 256 / 257 groups, every tail length, 52 captures of 81 952 scalars that take the grid through a second
    trip, three decodable captures), from one device buffer with sources aligned to their element only, and the first call's
    captures again from host memory.  After each: every sample of every capture, every known pad sample (the second call's pads
    lie on samples the first call wrote), the format report, and the frames and Try/Ok tables."""
    d, ref = decoders(df18=True, collect_stats=True), decoders(df18=True, collect_stats=True)
    scratch = None
    for k in range(len(B.CALLS)):
        batch = B.call(conv, k)
        what = (B.NAMES[conv], "call", k)
        want = reference_frames(ref, batch)
        held, ptrs = upload(torch_cuda, batch)
        if scratch is None:
            scratch = B.Scratch(batch.total)
        scratch.write(batch)
        d.reset()
        frames, stats = decode_device(d, batch, ptrs)
        assert d.format_report() == batch.report(), (what, d.format_report(), batch.report())
        n_pad = check_scratch(d, batch, scratch, what)
        assert k == 0 or n_pad > 2000, (what, n_pad)         # an "untouched" that can be seen
        check_frames(batch, want, frames, stats, what)
        slot_0 = scratch.pad(batch, 0)[0]
        for bad_i, bad_n in ((len(batch.n), 0), (0, slot_0 + 1)):
            with pytest.raises(capi.AdsbError, match="adsb_batch_unpacked_copy"):
                d.batch_unpacked(bad_i, bad_n)
        del held
        if k == 0:                                           # the host flavour: the same captures, landed by copies first
            d.reset()
            frames, stats = decode_host(d, batch)
            assert d.format_report() == batch.report(), (what, "host", d.format_report(), batch.report())
            check_scratch(d, batch, scratch, what + ("host",))
            check_frames(batch, want, frames, stats, what + ("host",))


@pytest.mark.parametrize("conv", B.CONVS, ids=IDS)
def test_counts_of_the_short_road_and_of_whole_groups(capi, torch_cuda, decoders, conv):
    """Two batches: in one every off-grid scalar lies in a short last group (the sample-by-sample road), in the other none does.
    Each gives its own exact report, from device and from host memory: a count lost on either road cannot hide in the other."""
    d = decoders(df18=True, collect_stats=True)
    for short_road in (True, False):
        batch = B.counter_batch(conv, short_road)
        what = (B.NAMES[conv], "short road" if short_road else "whole groups")
        assert batch.n_off_grid(not short_road) == 0 and batch.inexact > 0 and (conv == B.S16 or batch.clamped > 0)
        held, ptrs = upload(torch_cuda, batch)
        scratch = B.Scratch(batch.total)
        scratch.write(batch)
        d.reset()
        frames, stats = decode_device(d, batch, ptrs)
        assert d.format_report() == batch.report(), (what, d.format_report(), batch.report())
        check_scratch(d, batch, scratch, what)
        check_frames(batch, {}, frames, stats, what)
        d.reset()
        decode_host(d, batch)
        assert d.format_report() == batch.report(), (what, "host", d.format_report(), batch.report())
        check_scratch(d, batch, scratch, what + ("host",))
        del held


def test_unpacked_copy_refuses_after_a_batch_that_fills_no_scratch(capi, torch_cuda, decoders):
    """adsb_batch_unpacked_copy answers for the last packed or converted batch call only: after an IQ fmt-2 batch whose captures
    are 4-byte aligned (copied into the same scratch), a power batch and a uint16 batch -- from device and from host memory --
    it refuses, where it used to answer with the layout of an earlier call; a converted call before and after them still works."""
    torch = torch_cuda
    d = decoders(df18=True, collect_stats=True)
    rng = np.random.default_rng(4900)
    batch = B.counter_batch(B.S16, True)
    held, ptrs = upload(torch, batch)
    scratch = B.Scratch(batch.total)
    scratch.write(batch)

    def converted():
        decode_device(d, batch, ptrs)
        for i in (0, 1, len(batch.n) - 1):
            n = batch.scalars[i]
            assert np.array_equal(d.batch_unpacked(i, n), batch.codes[i]), i

    n_iq = [1000, 0, 333]
    iq = torch.from_numpy(rng.integers(-2048, 2048, 4 + 2 * 1024 * len(n_iq), dtype=np.int16)).cuda()
    p_iq = [iq.data_ptr() + 4 + 4096 * i if n else 0 for i, n in enumerate(n_iq)]
    assert iq.data_ptr() % 16 == 0 and all(p % 16 == 4 for p in p_iq if p)
    n_pw = [1000, 7, 0]
    pw = torch.from_numpy(rng.uniform(0, 4e6, 1024 * len(n_pw)).astype("<f4")).cuda()
    p_pw = [pw.data_ptr() + 4096 * i if n else 0 for i, n in enumerate(n_pw)]
    n_u16 = [2000, 0, 64]
    u16 = torch.from_numpy(rng.integers(0, 4096, 2048 * len(n_u16), dtype=np.uint16).view(np.int16)).cuda()
    p_u16 = [u16.data_ptr() + 4096 * i if n else 0 for i, n in enumerate(n_u16)]
    host_u16 = [rng.integers(0, 4096, n, dtype=np.uint16) for n in n_u16]
    host_iq = [rng.integers(-2048, 2048, 2 * n).astype("<i2") for n in n_iq]
    host_pw = [rng.uniform(0, 4e6, n).astype("<f4") for n in n_pw]
    converted()
    for name, other in (("iq fmt 2, device", lambda: d.decode_batch_device_iq(2, p_iq, n_iq)),
                        ("power, device", lambda: d.decode_batch_device_power(p_pw, n_pw)),
                        ("uint16, device", lambda: d.decode_batch_device(p_u16, n_u16)),
                        ("uint16 through _as, device", lambda: d.decode_batch_device_as(4, p_u16, n_u16)),
                        ("iq fmt 2, host", lambda: d.decode_batch_iq(2, host_iq)),
                        ("power, host", lambda: d.decode_batch_power(host_pw)),
                        ("uint16, host", lambda: d.decode_batch(host_u16))):
        assert other() == [[], [], []], name
        for i, n in ((0, 1), (0, 0), (2, 1)):
            with pytest.raises(capi.AdsbError, match="adsb_batch_unpacked_copy"):
                d.batch_unpacked(i, n)
        converted()
    del held
