"""adsb_multi_decode_batch_host / _files and the C host program's -B: a batch of independent captures over the workers of
adsb_multi.  The workers here all sit on device 0 (an ordinal may repeat: plumbing on a one-GPU box, as tests/test_gpu_multi.py
does) -- what is checked is that every capture comes back exactly as the single-handle batch call decodes it, whatever the
number of workers, the sub-batch size, and whether the captures are arrays, files, uint16 or packed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import golden_cases, load_golden, records
from test_batch_cpu import seeded_capture
from test_gpu_batch_packed import build_mixed, packable

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(capi, tmp_path_factory):
    """The mixed batch of tests/test_gpu_batch_packed.py (40 captures, every one whole 8-sample groups of 12-bit codes) as
    uint16 arrays, packed bytes, files of both kinds, and what ONE handle's batch call gives for it: the reference here."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from adsbdec_amd.packed12 import pack12
    caps = build_mixed()
    packed = [pack12(x) for x in caps]
    where = tmp_path_factory.mktemp("multi_batch")
    u16, p12 = [], []
    for i, (x, b) in enumerate(zip(caps, packed)):
        u16.append(str(where / f"cap{i:03d}.u16"))
        p12.append(str(where / f"cap{i:03d}.p12"))
        x.tofile(u16[-1])
        b.tofile(p12[-1])
    want = {}
    for stats in (False, True):
        d = capi.Decoder(df18=True, collect_stats=stats)
        try:
            want[stats] = d.decode_batch(caps, stats=True)
            assert d.decode_batch_packed(packed, stats=True)[1] == want[stats][1]
        finally:
            d.close()
    assert sum(bool(f) for f in want[True][0]) >= 25
    return caps, packed, u16, p12, want


def _same(got, want, what):
    frames, stats = got
    assert len(frames) == len(want[0]) and len(stats) == len(want[1]), what
    for i in range(len(frames)):
        assert records(frames[i]) == records(want[0][i]), (what, i)
        assert stats[i] == want[1][i], (what, i)


def _sum(stats):
    tot = {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    for s in stats:
        for row in tot:
            for df in tot[row]:
                tot[row][df] += s[row][df]
    return tot


@pytest.mark.limit(600)
@pytest.mark.parametrize("workers", [1, 2, 3])
def test_every_ingress_equals_the_single_handle_batch(capi, batch, workers):
    from adsbdec_amd import sharding
    caps, packed, u16, p12, want = batch
    sizes = [x.size for x in caps]
    for stats in (True, False):
        md = sharding.MultiDecoder(workers, [0] * workers, df18=True, collect_stats=stats)
        try:
            for what, call in (("host uint16", lambda: md.decode_batch_host(caps, stats=True)),
                               ("host packed", lambda: md.decode_batch_host(packed, packed=True, stats=True)),
                               ("files uint16", lambda: md.decode_batch_files(u16, stats=True)),
                               ("files packed", lambda: md.decode_batch_files(p12, packed=True, stats=True))):
                got = call()
                _same(got, want[stats], (what, workers, stats))
                tot = _sum(got[1])
                whole = md.stats()                                                    # adsb_multi_get_stats: the sum
                assert {k: whole[k] for k in ("try", "ok")} == tot, what
                rng, _ = capi.multi_batch_plan(sizes, workers, 0, "packed" in what)
                assert md.info()["shards"] == sum(1 for a, b in zip(rng, rng[1:]) if b > a) >= min(workers, 2), what
            assert md.decode_batch_host([]) == [] and md.decode_batch_files([], packed=True) == []
            assert md.info()["shards"] == 0
        finally:
            md.close()


@pytest.mark.limit(600)
@pytest.mark.parametrize("workers", [1, 3])
def test_several_sub_batches_per_worker_and_a_capture_larger_than_one(capi, batch, workers):
    """batch_bytes = 1 MiB: the 9 Mi-sample capture (18 MiB) is a sub-batch of its own, the 1 Mi ones fill one each, the short
    ones share; the result does not change."""
    from adsbdec_amd import sharding
    caps, packed, u16, p12, want = batch
    sizes = [x.size for x in caps]
    rng, subs = capi.multi_batch_plan(sizes, workers, 1 << 20)
    per_worker = [sum(1 for s in subs[:-1] if rng[w] <= s < rng[w + 1]) for w in range(workers)]
    assert max(per_worker) >= 3 and max(2 * n for n in sizes) > 1 << 20
    md = sharding.MultiDecoder(workers, [0] * workers, df18=True, collect_stats=True)
    try:
        md.set_batch_bytes(1 << 20)
        _same(md.decode_batch_host(caps, stats=True), want[True], "host uint16")
        _same(md.decode_batch_host(packed, packed=True, stats=True), want[True], "host packed")
        _same(md.decode_batch_files(u16, stats=True), want[True], "files uint16")
        _same(md.decode_batch_files(p12, packed=True, stats=True), want[True], "files packed")
        assert {k: md.stats()[k] for k in ("try", "ok")} == _sum(want[True][1])
        md.set_batch_bytes(0)                                                         # the default again
        _same(md.decode_batch_files(p12, packed=True, stats=True), want[True], "files packed, default")
    finally:
        md.close()


@pytest.mark.limit(300)
def test_an_unreadable_path_fails_the_call_and_leaves_the_driver_usable(capi, batch, tmp_path):
    from adsbdec_amd import sharding
    caps, packed, u16, p12, want = batch
    md = sharding.MultiDecoder(2, [0, 0], df18=True, collect_stats=True)
    try:
        missing = str(tmp_path / "not_there.u16")
        with pytest.raises(sharding.ShardError, match="capture 5.*not_there.u16"):
            md.decode_batch_files(u16[:5] + [missing] + u16[5:])
        with pytest.raises(sharding.ShardError, match="capture 0.*" + os.path.basename(str(tmp_path))):
            md.decode_batch_files([str(tmp_path)], packed=True)                       # a directory
        with pytest.raises(sharding.ShardError):
            md.stats()                                                                # no partial result
        _same(md.decode_batch_files(u16, stats=True), want[True], "after the failures")
        L = capi.load()
        import ctypes as C
        bad = (C.c_void_p * 2)(caps[0].ctypes.data, None)
        first = (C.c_uint64 * 3)()
        out = C.POINTER(capi.Frame)()
        assert L.adsb_multi_decode_batch_host(md._h, 2, bad, (C.c_size_t * 2)(caps[0].size, 8), 0, C.byref(out), first, None) == -1
        assert b"capture 1" in L.adsb_multi_last_error(md._h)
        assert L.adsb_multi_decode_batch_host(md._h, 2, bad, (C.c_size_t * 2)(12, 0), 1, C.byref(out), first, None) == -1
        assert b"capture 0" in L.adsb_multi_last_error(md._h) and b"multiple of 8" in L.adsb_multi_last_error(md._h)
        _same(md.decode_batch_host(packed, packed=True, stats=True), want[True], "after the refusals")
    finally:
        md.close()


def _table_rows(lines, at):
    return ([int(v) for v in lines[at + 2].split(":")[1].split()], [int(v) for v in lines[at + 3].split(":")[1].split()])


@pytest.mark.limit(900)
def test_cli_batch_list(capi, tmp_path):
    """adsbdec_amd_cli -a -B list over 100 capture files and more, and -p -B over their packed twins, on one device and with
    -G 0,0: every <capture>.avr equals, byte for byte, what adsbdec_amd_cli -a -f capture writes to stdout, and for the files
    made of golden fixtures the committed expected bytes."""
    from adsbdec_amd.packed12 import pack12
    golden = {}
    caps = []
    for name in golden_cases():
        x, rec = load_golden(name)
        if rec["df18"] and x.size % 8 == 0 and int(x.max()) <= 4095:
            golden[len(caps)] = "".join(f["avr"] for f in rec["frames"]).encode()
            caps.append(x)
    assert len(golden) >= 2
    caps += [packable(seeded_capture(i)) for i in range(100)]
    assert len(caps) >= 100 and any(x.size == 0 for x in caps)
    u16, p12 = [], []
    for i, x in enumerate(caps):
        u16.append(str(tmp_path / f"c{i:03d}.u16"))
        p12.append(str(tmp_path / f"c{i:03d}.p12"))
        x.tofile(u16[-1])
        pack12(x).tofile(p12[-1])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:     # (a process per capture is what the list spares: eight side by side keep the test short)
        runs = list(pool.map(lambda path: subprocess.run([capi.CLI_PATH, "-a", "-f", path], capture_output=True, timeout=300), u16))
    single = []
    for p in runs:
        assert p.returncode == 0, p.stderr
        err = p.stderr.decode().splitlines()
        at = next(k for k, line in enumerate(err) if line.startswith("Try :")) - 1
        single.append((p.stdout, _table_rows(err, at - 1)))
    for i, want in golden.items():
        assert single[i][0] == want and want
    assert sum(1 for out, _ in single if out) >= 90
    (tmp_path / "u16.list").write_text("\n".join(u16[:50]) + "\n\n\n" + "\n".join(u16[50:]))      # empty lines; no newline at the end
    (tmp_path / "p12.list").write_text("\n".join(p12) + "\n")
    for opts in ([], ["-G", "0,0"], ["-d", "0"]):
        for paths, listfile, flags in ((u16, "u16.list", []), (p12, "p12.list", ["-p"])):
            for path in paths:
                if os.path.exists(path + ".avr"):
                    os.remove(path + ".avr")
            p = subprocess.run([capi.CLI_PATH, "-a"] + flags + opts + ["-B", str(tmp_path / listfile)], capture_output=True, timeout=600)
            assert p.returncode == 0 and p.stdout == b"", p.stderr
            err = p.stderr.decode().splitlines()
            heads = [k for k, line in enumerate(err) if line.startswith("== ")]
            assert len(heads) == len(paths)
            for i, path in enumerate(paths):
                got = open(path + ".avr", "rb").read()
                assert got == single[i][0], (opts, path)
                if i in golden:
                    assert got == golden[i], (opts, path)
                assert err[heads[i]] == f"== {path}: {got.count(b';')} frames -> {path}.avr", err[heads[i]]
                assert _table_rows(err, heads[i]) == single[i][1], (opts, path)
    p = subprocess.run([capi.CLI_PATH, "-a", "-B", str(tmp_path / "u16.list")], capture_output=True, timeout=600, cwd=str(tmp_path),
                       env=dict(os.environ, ADSB_CLI_TIMING="1"))
    assert p.returncode == 0 and b"timing: runtime init" in p.stderr
    (tmp_path / "bad.list").write_text(u16[0] + "\n" + str(tmp_path / "gone.u16") + "\n")
    p = subprocess.run([capi.CLI_PATH, "-a", "-B", str(tmp_path / "bad.list")], capture_output=True, timeout=600)
    assert p.returncode == 255 and b"capture 1" in p.stderr and b"gone.u16" in p.stderr
