#!/usr/bin/env python3
"""The conversion of signed 16-bit real and float32 real input (adsb_*_as) on one GPU, ONE process, the sides of every
comparison interleaved.

    python tools/format_probe.py [--reps 20] [--out profiles/r11_formats.txt]
    python tools/format_probe.py --iq [--reps 20] [--out profiles/r14_iq.txt]      # complex captures: see iq_probe()
    python tools/format_probe.py --power [--reps 20] [--out profiles/r15_power.txt] [--ab parent=path/to/libadsbdec_amd.so]   # power_probe()
    python tools/format_probe.py --export [--reps 20] [--out profiles/r17_power_export.txt] [--layout name=path/to/libadsbdec_amd.so ...]   # export_probe()
    python tools/format_probe.py --export-batch [--reps 20] [--out profiles/r20_export_batch.txt] [--ab path/to/parent/libadsbdec_amd.so]   # export_batch_probe()
    python tools/format_probe.py --level [--reps 20] [--out profiles/r23_level.txt] [--variant name=path/to/libadsbdec_amd.so ...]   # level_probe()
    python tools/format_probe.py --level-windows [--reps 20] [--ab parent/libadsbdec_amd.so] [--out profiles/r27_level_windows.txt]   # level_windows_probe()
    python tools/format_probe.py --burst-stream [--reps 20] [--ab parent/libadsbdec_amd.so] [--out profiles/rNN_burst_stream.txt]   # burst_stream_probe()
    python tools/format_probe.py --bursts [--reps 20] [--ab parent/libadsbdec_amd.so] [--out profiles/rNN_bursts.txt]   # bursts_probe(): NN is the next free round
    python tools/format_probe.py --flush [--reps 10] [--ab parent/libadsbdec_amd.so] [--out profiles/r30_flush.txt]   # flush_probe()
    python tools/format_probe.py --gather [--reps 10] [--ab parent/libadsbdec_amd.so] [--variant name=path/to/libadsbdec_amd.so ...] [--out profiles/r32_gather.txt]   # gather_probe()
    python tools/format_probe.py --gather-pack12 [--reps 10] [--ab parent/libadsbdec_amd.so] [--variant name=path/to/libadsbdec_amd.so ...] [--out profiles/r33_pack12.txt]   # gather_pack12_probe()
    python tools/format_probe.py --level-batch [--reps 20] [--out profiles/r26_level_batch.txt] [--variant name=path/to/libadsbdec_amd.so ...]   # level_batch_probe()

(a) The kernels alone at 256 Mi samples, timed with device events around each launch: adsb_convert_samples for both formats
    (with counters, and without: a kernel that does not classify its samples at all) and adsb_unpack_packed12 at the same n
    as the yardstick -- all three are streaming passes.  Bytes moved:
    (element size + 2) x n for a conversion, 3.5 x n for the unpack; the share of the 8 TB/s HBM peak beside it.
(b) Whole calls, wall time: adsb_decode_device_as against adsb_decode_device on the raw twin at 256 Mi samples (sparse
    traffic: BASELINE configs[1]'s generator), and one adsb_decode_batch_device_as of 256 captures of 1 Mi samples against the
    loop of 256 adsb_decode_device_as calls.
Medians over --reps repetitions after a warm-up of each side; frames equal on all sides, or the probe stops.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: one HIP runtime)

from adsbdec_amd import capi  # noqa: E402
from tools.gen_signal import make_workload  # noqa: E402

N = 1 << 28
PEAK = 8e12          # bytes/s of HBM3E (MI355X)
F32, S16 = capi.FMT_FLOAT32_REAL, capi.FMT_INT16_REAL
NAMES = {F32: "FLOAT32_REAL", S16: "INT16_REAL"}


def med(v):
    return statistics.median(v)


def kernels(L, t, conv, reps, lines):
    from adsbdec_amd.packed12 import pack12
    import numpy as np
    x = t.cpu().numpy().view(np.uint16)
    step = 1 << 24
    pk = torch.cat([torch.from_numpy(pack12(x[i:i + step])).cuda() for i in range(0, x.size, step)])
    del x
    dst = torch.empty(N, dtype=torch.int16, device="cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    sides = {
        "convert INT16_REAL": (lambda: L.adsb_convert_samples(dst.data_ptr(), conv[S16].data_ptr(), S16, N, counters.data_ptr(), None), 4.0),
        "convert FLOAT32_REAL": (lambda: L.adsb_convert_samples(dst.data_ptr(), conv[F32].data_ptr(), F32, N, counters.data_ptr(), None), 6.0),
        "INT16_REAL, no count": (lambda: L.adsb_convert_samples(dst.data_ptr(), conv[S16].data_ptr(), S16, N, None, None), 4.0),
        "FLOAT32_REAL, no count": (lambda: L.adsb_convert_samples(dst.data_ptr(), conv[F32].data_ptr(), F32, N, None, None), 6.0),
        "unpack packed 12-bit": (lambda: L.adsb_unpack_packed12(dst.data_ptr(), pk.data_ptr(), N, None), 3.5),
    }
    ms = {k: [] for k in sides}
    for rep in range(-3, reps):                             # three warm-up rounds
        for name, (fn, _) in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0, L.adsb_last_error(None)
            e1.record()
            e1.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
            if rep == -3:
                assert torch.equal(dst, t), f"{name} does not give the capture back"
                dst.zero_()
    assert counters.cpu().tolist() == [0, 0]
    lines += ["# (a) the kernels alone, 256 Mi samples, device events around one launch on the null stream (launch included); median, min, max",
              "#   kernel                 bytes/sample   median ms   min ms   max ms   TB/s (median)   share of 8 TB/s   vs unpack (bytes/s)"]
    base = 3.5 * N / (med(ms["unpack packed 12-bit"]) * 1e-3)
    for name, (_, per) in sides.items():
        m = med(ms[name])
        rate = per * N / (m * 1e-3)
        lines.append(f"    {name:22s} {per:12.1f}  {m:10.4f}  {min(ms[name]):7.4f}  {max(ms[name]):7.4f}  {rate * 1e-12:14.3f}  {rate / PEAK:16.3f}  {rate / base:12.3f}")
        print(lines[-1], flush=True)
    del pk, dst


def whole_calls(L, t, conv, reps, lines):
    d_raw, d_as, d_batch, d_loop = (capi.Decoder(df18=False) for _ in range(4))
    out = C.POINTER(capi.Frame)()

    def raw():
        t0 = time.perf_counter()
        k = L.adsb_decode_device(d_raw._h, t.data_ptr(), N, C.byref(out))
        return time.perf_counter() - t0, k

    def as_(fmt):
        t0 = time.perf_counter()
        k = L.adsb_decode_device_as(d_as._h, fmt, conv[fmt].data_ptr(), N, C.byref(out))
        return time.perf_counter() - t0, k

    k0 = raw()[1]
    assert k0 > 0 and all(as_(f)[1] == k0 for f in (S16, F32)), "frames differ from the raw twin"
    tr, ta = [], {S16: [], F32: []}
    for _ in range(reps):
        tr.append(raw()[0])
        for f in (S16, F32):
            ta[f].append(as_(f)[0])
    lines += ["#", f"# (b) whole calls, wall time in ms, medians; one capture of 256 Mi samples, {k0} frames on every side",
              f"    adsb_decode_device (raw twin)          {med(tr) * 1e3:9.3f}"]
    for f in (S16, F32):
        lines.append(f"    adsb_decode_device_as {NAMES[f]:13s}    {med(ta[f]) * 1e3:9.3f}   (+{(med(ta[f]) - med(tr)) * 1e3:.3f} ms over the raw twin)")
    for ln in lines[-3:]:
        print(ln, flush=True)

    B, n = 256, 1 << 20
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    lines += ["#", "# one adsb_decode_batch_device_as of 256 captures of 1 Mi samples (slices of the same buffer) against the loop of 256",
              "# adsb_decode_device_as calls; frames per capture equal",
              "#   format          batch ms    loop ms   loop/batch   frames"]
    for f in (S16, F32):
        el = 2 if f == S16 else 4
        ptrs = [conv[f].data_ptr() + el * n * i for i in range(B)]
        p = (C.c_void_p * B)(*ptrs)

        def batch():
            t0 = time.perf_counter()
            k = L.adsb_decode_batch_device_as(d_batch._h, f, B, p, nn, C.byref(out), first, None)
            dt = time.perf_counter() - t0
            assert k >= 0, L.adsb_last_error(d_batch._h)
            return dt, [int(first[i + 1] - first[i]) for i in range(B)]

        def loop():
            per = []
            t0 = time.perf_counter()
            for i in range(B):
                per.append(L.adsb_decode_device_as(d_loop._h, f, ptrs[i], n, d_loop._out_ref))
            return time.perf_counter() - t0, per

        (_, fb), (_, fl) = batch(), loop()
        assert fb == fl, f"{NAMES[f]}: frames per capture differ"
        tb, tl = [], []
        for _ in range(reps):
            tb.append(batch()[0])
            tl.append(loop()[0])
        lines.append(f"    {NAMES[f]:13s}  {med(tb) * 1e3:9.3f}  {med(tl) * 1e3:9.3f}  {med(tl) / med(tb):10.2f}  {sum(fb):7d}")
        print(lines[-1], flush=True)
    for d in (d_raw, d_as, d_batch, d_loop):
        assert d.format_report()[1:] == (0, 0)
        d.close()


def iq_probe(L, reps, lines):
    """Complex captures (the _iq calls), every comparison interleaved in this one process:
    (a) the scan kernel's own time (cfg.profile: adsb_profile.big_ms / big_launches) and the call's wall time of
        adsb_decode_device_iq on 128 Mi complex int16 samples against adsb_decode_device on the 256 Mi-sample real workload --
        512 MiB each, one frame per millisecond of signal on both sides;
    (b) the float32 conversion: adsb_convert_iq_float32 alone (device events), and the fmt-0 call against the fmt-2 call;
    (c) one adsb_decode_batch_device_iq of 256 captures of 512 Ki complex samples against the loop of 256 single calls."""
    import numpy as np
    from tools.gen_signal import make_iq_workload
    NC = 1 << 27
    real, _ = make_workload(torch, N, seed=1)
    # the generator is numpy's: one block of 4 Mi complex samples (419 frames, a millisecond slot each), repeated 32 times
    block, truth = make_iq_workload(1 << 22, seed=1)
    iq = torch.from_numpy(block.reshape(-1)).cuda().repeat(NC >> 22)
    iqf = iq.to(torch.float32) / 32768.0
    torch.cuda.synchronize()
    d_real, d_iq, d_f = (capi.Decoder(df18=False, profile=True) for _ in range(3))
    out = C.POINTER(capi.Frame)()

    def kernel_ms(d):
        p = d.profile()
        return p["big_ms"], p["big_launches"]

    sides = {
        "real   adsb_decode_device       256 Mi real samples": (d_real, lambda: L.adsb_decode_device(d_real._h, real.data_ptr(), N, C.byref(out))),
        "IQ     adsb_decode_device_iq 2  128 Mi complex int16": (d_iq, lambda: L.adsb_decode_device_iq(d_iq._h, 2, iq.data_ptr(), NC, C.byref(out))),
        "IQ     adsb_decode_device_iq 0  128 Mi complex float": (d_f, lambda: L.adsb_decode_device_iq(d_f._h, 0, iqf.data_ptr(), NC, C.byref(out))),
    }
    frames = {}
    for name, (d, fn) in sides.items():
        for _ in range(3):
            frames[name] = fn()
        assert frames[name] > 0, (name, L.adsb_last_error(d._h))
    names = list(sides)
    assert frames[names[1]] == frames[names[2]], frames
    assert d_f.format_report() == (2 * NC, 0, 0)
    kms, wall = {k: [] for k in sides}, {k: [] for k in sides}
    steps = 5
    for r in range(reps):
        order = names[r % 3:] + names[:r % 3]
        for name in order:
            d, fn = sides[name]
            m0, l0 = kernel_ms(d)
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            m1, l1 = kernel_ms(d)
            kms[name].append((m1 - m0) / max(1, l1 - l0))
    lines += ["# (a) scan kernel on its own clock (cfg.profile, ms per launch) and the call's wall time; 512 MiB of int16 on both sides,",
              f"#     one frame per ms of signal; {reps} rounds x {steps} calls per side, the sides in rotation; medians (quartiles)",
              "#   side                                                   frames   kernel ms (q1 .. q3)            call ms   kernel / real (median of rounds)"]
    base = kms[names[0]]
    for name in names:
        q = statistics.quantiles(kms[name], n=4)
        ratio = med([a / b for a, b in zip(kms[name], base)])
        lines.append(f"    {name:54s} {frames[name]:7d}   {med(kms[name]):.5f} ({q[0]:.5f} .. {q[2]:.5f})   {med(wall[name]):8.4f}   {ratio:.4f}")
        print(lines[-1], flush=True)

    # (b) the conversion alone
    dst = torch.empty(2 * NC, dtype=torch.int16, device="cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    conv = {"convert FLOAT32_IQ": lambda: L.adsb_convert_iq_float32(dst.data_ptr(), iqf.data_ptr(), 2 * NC, counters.data_ptr(), None),
            "FLOAT32_IQ, no count": lambda: L.adsb_convert_iq_float32(dst.data_ptr(), iqf.data_ptr(), 2 * NC, None, None)}
    ms = {k: [] for k in conv}
    for rep in range(-3, reps):
        for name, fn in conv.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0, L.adsb_last_error(None)
            e1.record()
            e1.synchronize()
            if rep >= 0:
                ms[name].append(e0.elapsed_time(e1))
            if rep == -3:
                assert torch.equal(dst, iq), f"{name} does not give the int16 capture back"
    assert counters.cpu().tolist() == [0, 0]
    lines += ["#", "# (b) the float32 conversion alone: 256 Mi scalars (6 bytes moved per scalar), device events around one launch; median, min, max",
              "#   kernel                  median ms   min ms   max ms   TB/s (median)   share of 8 TB/s"]
    for name in conv:
        m = med(ms[name])
        rate = 6.0 * 2 * NC / (m * 1e-3)
        lines.append(f"    {name:22s} {m:10.4f}  {min(ms[name]):7.4f}  {max(ms[name]):7.4f}  {rate * 1e-12:14.3f}  {rate / PEAK:16.3f}")
        print(lines[-1], flush=True)
    del dst

    # (c) a batch against the loop of single calls
    B, n = 256, 1 << 19
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    d_batch, d_loop = capi.Decoder(df18=False), capi.Decoder(df18=False)
    lines += ["#", "# (c) one adsb_decode_batch_device_iq of 256 captures of 512 Ki complex samples (slices of the same buffer) against the loop of",
              "#     256 adsb_decode_device_iq calls; frames per capture equal; wall time, medians",
              "#   format        batch ms    loop ms   loop/batch   frames"]
    for f, buf, el in ((2, iq, 4), (0, iqf, 8)):
        ptrs = [buf.data_ptr() + el * n * i for i in range(B)]
        p = (C.c_void_p * B)(*ptrs)

        def batch():
            t0 = time.perf_counter()
            k = L.adsb_decode_batch_device_iq(d_batch._h, f, B, p, nn, C.byref(out), first, None)
            dt = time.perf_counter() - t0
            assert k >= 0, L.adsb_last_error(d_batch._h)
            return dt, [int(first[i + 1] - first[i]) for i in range(B)]

        def loop():
            per = []
            t0 = time.perf_counter()
            for i in range(B):
                per.append(L.adsb_decode_device_iq(d_loop._h, f, ptrs[i], n, d_loop._out_ref))
            return time.perf_counter() - t0, per

        (_, fb), (_, fl) = batch(), loop()
        assert fb == fl, f"fmt {f}: frames per capture differ"
        tb, tl = [], []
        for _ in range(reps):
            tb.append(batch()[0])
            tl.append(loop()[0])
        lines.append(f"    {'INT16_IQ' if f == 2 else 'FLOAT32_IQ':11s}  {med(tb) * 1e3:9.3f}  {med(tl) * 1e3:9.3f}  {med(tl) / med(tb):10.2f}  {sum(fb):7d}")
        print(lines[-1], flush=True)
    for d in (d_real, d_iq, d_f, d_batch, d_loop):
        d.close()


def power_probe(L, reps, lines):
    """float32 power samples (the _power calls), every comparison interleaved in this one process:
    (a) the scan kernel's own time (cfg.profile: adsb_profile.big_ms / big_launches) and the call's wall time of
        adsb_decode_device_power on 128 Mi power samples against adsb_decode_device_iq (fmt 2) on the int16 capture those samples
        are iq_power of -- 512 MiB each, the same frames;
    (b) one adsb_decode_batch_device_power of 256 captures of 512 Ki power samples against the loop of 256 single calls."""
    from tools.gen_signal import make_iq_workload
    NC = 1 << 27
    block, truth = make_iq_workload(1 << 22, seed=1)
    iq = torch.from_numpy(block.reshape(-1)).cuda().repeat(NC >> 22)
    s = iq.view(-1, 2).to(torch.float32) * 0.0625
    ii, qq = s[:, 0] * s[:, 0], s[:, 1] * s[:, 1]          # (one rounded operation per line: sample_formats.iq_power)
    pw = (ii + qq).contiguous()
    del s, ii, qq
    torch.cuda.synchronize()
    from adsbdec_amd.sample_formats import iq_power
    assert torch.equal(pw[: 1 << 22].cpu(), torch.from_numpy(iq_power(block))), "torch's power samples are not iq_power's"
    d_iq, d_pw = (capi.Decoder(df18=False, profile=True) for _ in range(2))
    out = C.POINTER(capi.Frame)()

    def kernel_ms(d):
        p = d.profile()
        return p["big_ms"], p["big_launches"]

    sides = {
        "IQ     adsb_decode_device_iq 2   128 Mi complex int16": (d_iq, lambda: L.adsb_decode_device_iq(d_iq._h, 2, iq.data_ptr(), NC, C.byref(out))),
        "power  adsb_decode_device_power  128 Mi float32 power": (d_pw, lambda: L.adsb_decode_device_power(d_pw._h, pw.data_ptr(), NC, C.byref(out))),
    }
    frames = {}
    for name, (d, fn) in sides.items():
        for _ in range(3):
            frames[name] = fn()
        assert frames[name] > 0, (name, L.adsb_last_error(d._h))
    names = list(sides)
    assert frames[names[0]] == frames[names[1]], frames
    kms, wall = {k: [] for k in sides}, {k: [] for k in sides}
    steps = 5
    for r in range(reps):
        order = names[r % 2:] + names[:r % 2]
        for name in order:
            d, fn = sides[name]
            m0, l0 = kernel_ms(d)
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            m1, l1 = kernel_ms(d)
            kms[name].append((m1 - m0) / max(1, l1 - l0))
    lines += ["# (a) scan kernel on its own clock (cfg.profile, ms per launch) and the call's wall time; 512 MiB on both sides, the power samples",
              f"#     iq_power of the int16 capture; {reps} rounds x {steps} calls per side, the sides in rotation; medians (quartiles)",
              "#   side                                                    frames   kernel ms (q1 .. q3)            call ms   kernel / IQ (median of rounds)   call / IQ"]
    base, wbase = kms[names[0]], wall[names[0]]
    for name in names:
        q = statistics.quantiles(kms[name], n=4)
        ratio = med([a / b for a, b in zip(kms[name], base)])
        wratio = med([a / b for a, b in zip(wall[name], wbase)])
        lines.append(f"    {name:55s} {frames[name]:7d}   {med(kms[name]):.5f} ({q[0]:.5f} .. {q[2]:.5f})   {med(wall[name]):8.4f}   {ratio:.4f}   {wratio:.4f}")
        print(lines[-1], flush=True)

    B, n = 256, 1 << 19
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    d_batch, d_loop = capi.Decoder(df18=False), capi.Decoder(df18=False)
    ptrs = [pw.data_ptr() + 4 * n * i for i in range(B)]
    p = (C.c_void_p * B)(*ptrs)

    def batch():
        t0 = time.perf_counter()
        k = L.adsb_decode_batch_device_power(d_batch._h, B, p, nn, C.byref(out), first, None)
        dt = time.perf_counter() - t0
        assert k >= 0, L.adsb_last_error(d_batch._h)
        return dt, [int(first[i + 1] - first[i]) for i in range(B)]

    def loop():
        per = []
        t0 = time.perf_counter()
        for i in range(B):
            per.append(L.adsb_decode_device_power(d_loop._h, ptrs[i], n, d_loop._out_ref))
        return time.perf_counter() - t0, per

    (_, fb), (_, fl) = batch(), loop()
    assert fb == fl, "frames per capture differ"
    tb, tl = [], []
    for _ in range(reps):
        tb.append(batch()[0])
        tl.append(loop()[0])
    lines += ["#", "# (b) one adsb_decode_batch_device_power of 256 captures of 512 Ki power samples (slices of the same buffer) against the loop of",
              "#     256 adsb_decode_device_power calls; frames per capture equal; wall time, medians",
              "#   batch ms    loop ms   loop/batch   frames",
              f"    {med(tb) * 1e3:9.3f}  {med(tl) * 1e3:9.3f}  {med(tl) / med(tb):10.2f}  {sum(fb):7d}"]
    print(lines[-1], flush=True)
    for d in (d_iq, d_pw, d_batch, d_loop):
        d.close()
    del iq, pw
    torch.cuda.empty_cache()


def iq8_probe(L, reps, lines):
    """Complex int8 captures (fmt 8 of the _iq calls, scan_iq8_kernel.hip), every comparison interleaved in this one process and the
    A/A spread of the same run -- the same side measured twice, in rotation with the others -- beside every ratio:
    (a) the scan kernel's own time (cfg.profile) and the call's wall time of adsb_decode_device_iq fmt 8 on 128 Mi complex int8
        samples (256 MiB) against fmt 2 on the widened twin (512 MiB; scan_iq_kernel.hip, unchanged), the same frames;
    (b) the fmt 8 call against what a user could do before: widen on the device with torch (x.to(int16) << 8, then a device
        synchronisation: the library's stream is its own) and adsb_decode_device_iq fmt 2.  GATED: the old route moves five times
        the bytes, so it has to be slower by more than the A/A spread;
    (c) one adsb_decode_batch_device_iq fmt 8 of 256 captures of 512 Ki samples against the loop of 256 single calls."""
    from tools.gen_signal import make_iq_workload
    from adsbdec_amd.sample_formats import to_int8_iq
    NC = 1 << 27
    block16, truth = make_iq_workload(1 << 22, seed=1)
    block = to_int8_iq(block16)[0]
    x8 = torch.from_numpy(block.reshape(-1)).cuda().repeat(NC >> 22)
    widen = lambda: x8.to(torch.int16) << 8
    tw = widen().contiguous()
    torch.cuda.synchronize()
    assert torch.equal(tw[: 1 << 12].cpu(), torch.from_numpy(block.reshape(-1)[: 1 << 12].astype("int16") * 256))
    decs = {k: capi.Decoder(df18=False, profile=True) for k in ("i16", "i16'", "i8", "i8'", "old")}
    out = C.POINTER(capi.Frame)()

    def old_route():
        w = widen()
        torch.cuda.synchronize()
        return L.adsb_decode_device_iq(decs["old"]._h, 2, w.data_ptr(), NC, C.byref(out))

    sides = {
        "int16  adsb_decode_device_iq 2 on the widened twin    ": ("i16", lambda: L.adsb_decode_device_iq(decs["i16"]._h, 2, tw.data_ptr(), NC, C.byref(out))),
        "int16' the same side again (A/A)                      ": ("i16'", lambda: L.adsb_decode_device_iq(decs["i16'"]._h, 2, tw.data_ptr(), NC, C.byref(out))),
        "int8   adsb_decode_device_iq 8, 128 Mi complex int8   ": ("i8", lambda: L.adsb_decode_device_iq(decs["i8"]._h, 8, x8.data_ptr(), NC, C.byref(out))),
        "int8'  the same side again (A/A)                      ": ("i8'", lambda: L.adsb_decode_device_iq(decs["i8'"]._h, 8, x8.data_ptr(), NC, C.byref(out))),
        "old    torch widening + synchronize + fmt 2           ": ("old", old_route),
    }
    frames = {}
    for name, (k, fn) in sides.items():
        for _ in range(3):
            frames[name] = fn()
        assert frames[name] > 0, (name, L.adsb_last_error(decs[k]._h))
    names = list(sides)
    assert len(set(frames.values())) == 1, frames
    kms, wall = {k: [] for k in sides}, {k: [] for k in sides}
    steps = 5
    for r in range(reps):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            k, fn = sides[name]
            p0 = decs[k].profile()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            p1 = decs[k].profile()
            kms[name].append((p1["big_ms"] - p0["big_ms"]) / max(1, p1["big_launches"] - p0["big_launches"]))
    n16, n16b, n8, n8b, nold = names
    ratio = lambda v, a, b: med([x / y for x, y in zip(v[a], v[b])])
    lines += ["# (a), (b): scan kernel on its own clock (cfg.profile, ms per launch) and the call's wall time; 128 Mi complex samples on every side,",
              f"#     the same frames; {reps} rounds x {steps} calls per side, the sides in rotation; medians (quartiles of the kernel time)",
              "#   side                                                    frames   kernel ms (q1 .. q3)            call ms"]
    for name in names:
        q = statistics.quantiles(kms[name], n=4)
        lines.append(f"    {name:55s} {frames[name]:7d}   {med(kms[name]):.5f} ({q[0]:.5f} .. {q[2]:.5f})   {med(wall[name]):8.4f}")
        print(lines[-1], flush=True)
    aa_k = max(abs(ratio(kms, n16b, n16) - 1), abs(ratio(kms, n8b, n8) - 1))
    aa_w = max(abs(ratio(wall, n16b, n16) - 1), abs(ratio(wall, n8b, n8) - 1))
    lines += ["#   ratios (median over the rounds of the per-round ratio); A/A = the larger |ratio - 1| of the two sides measured twice",
              f"    (a) int8 / int16   kernel {ratio(kms, n8, n16):.4f} (A/A {aa_k:.4f})   call {ratio(wall, n8, n16):.4f} (A/A {aa_w:.4f})",
              f"    (b) old / int8     call {ratio(wall, nold, n8):.4f} (A/A {aa_w:.4f})   [the old route's scan kernel / int8's: {ratio(kms, nold, n8):.4f}]"]
    print("\n".join(lines[-2:]), flush=True)
    gate_ok = ratio(wall, nold, n8) > 1 + aa_w
    lines.append(f"    (b) gate: the old route is slower than the fmt 8 call by more than the A/A spread: {'PASS' if gate_ok else 'FAIL'}")

    B, n = 256, 1 << 19
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    d_batch, d_loop = capi.Decoder(df18=False), capi.Decoder(df18=False)
    ptrs = [x8.data_ptr() + 2 * n * i for i in range(B)]
    p = (C.c_void_p * B)(*ptrs)

    def batch():
        t0 = time.perf_counter()
        k = L.adsb_decode_batch_device_iq(d_batch._h, 8, B, p, nn, C.byref(out), first, None)
        dt = time.perf_counter() - t0
        assert k >= 0, L.adsb_last_error(d_batch._h)
        return dt, [int(first[i + 1] - first[i]) for i in range(B)]

    def loop():
        per = []
        t0 = time.perf_counter()
        for i in range(B):
            per.append(L.adsb_decode_device_iq(d_loop._h, 8, ptrs[i], n, d_loop._out_ref))
        return time.perf_counter() - t0, per

    (_, fb), (_, fl) = batch(), loop()
    assert fb == fl, "frames per capture differ"
    tb, tl = [], []
    for _ in range(reps):
        tb.append(batch()[0])
        tl.append(loop()[0])
    lines += ["#", "# (c) one adsb_decode_batch_device_iq fmt 8 of 256 captures of 512 Ki complex samples (slices of the same buffer) against the loop",
              "#     of 256 adsb_decode_device_iq fmt 8 calls; frames per capture equal; wall time, medians (reported, not gated)",
              "#   batch ms    loop ms   loop/batch   frames",
              f"    {med(tb) * 1e3:9.3f}  {med(tl) * 1e3:9.3f}  {med(tl) / med(tb):10.2f}  {sum(fb):7d}"]
    print(lines[-1], flush=True)
    for d in list(decs.values()) + [d_batch, d_loop]:
        d.close()
    del x8, tw
    torch.cuda.empty_cache()
    return gate_ok


def export_probe(L, reps, lines, layouts):
    """The power export (power_export_kernel.hip, the adsb_power_* calls), every comparison interleaved in this one process:
    (a) adsb_power_device on the 256 Mi-sample benchmark workload (512 MiB in, 512 MiB out; the call waits for its kernel, so its wall
        time is launch + kernel + wait) twice over -- the A/A -- beside adsb_decode_device on the same capture (wall, and the scan
        kernel on its own clock), and beside every other build given with --layout name=path: measurement builds of the library
        whose power_export_kernel.hip was compiled with another store layout (-DADSB_EXPORT_STORE=0: seven plain 16-byte stores
        per lane; =1: the same, non-temporal; =3: the tree's transposition through LDS with non-temporal stores);
    (b) adsb_power_device_iq (fmt 2) on 128 Mi complex samples; (c) adsb_power_window_host on 16 Mi samples, host memory both ways."""
    import numpy as np
    t, _ = make_workload(torch, N, seed=1)
    M = N // 2
    out = torch.empty(M, dtype=torch.float32, device="cuda")
    d_dec = capi.Decoder(df18=False, profile=True)
    fr = C.POINTER(capi.Frame)()

    def bind(path):
        B = C.CDLL(path)
        B.adsb_create.restype = C.c_void_p
        B.adsb_create.argtypes = [C.c_void_p]
        B.adsb_power_device.restype = C.c_long
        B.adsb_power_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        cfg = capi.make_config()
        h = B.adsb_create(C.byref(cfg))
        assert h, path
        return B, h

    d_tree = capi.Decoder()
    tree = (L, d_tree._h)
    builds = {"tree (transposed through LDS)": tree, "tree again (the A/A)": tree}
    for spec in layouts:
        name, _, path = spec.partition("=")
        builds[name] = bind(path)
    ref = None
    for name, (B, h) in builds.items():                    # warm-up, and every layout writes the same floats
        for _ in range(3):
            assert B.adsb_power_device(h, t.data_ptr(), N, out.data_ptr(), M) == M, name
        if ref is None:
            ref = out.clone()
            from oracle import oracle as O
            O.build()
            # the oracle's power samples: the head, and a slice from each later trip of the grid (the phase of a stream has a period
            # of 28 samples: oracle.power(x[f:])[6:] == oracle.power(x)[f // 2 + 6:] for f a multiple of 28)
            for f in [0] + [28 * (j * (N >> 3) // 28) for j in range(1, 8)] + [28 * ((N - (1 << 20)) // 28)]:
                piece = t[f: f + (1 << 20)].cpu().numpy().view(np.uint16)
                want = O.power(piece)[: 2 * (piece.size // 4)].view(np.uint32)
                got = out[f // 2: f // 2 + want.size].cpu().numpy().view(np.uint32)
                lead = 6 if f else 0
                assert np.array_equal(got[lead:], want[lead:]), f"not the oracle's power samples at sample {f}"
        else:
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"{name}: other floats"
        out.zero_()
    del ref
    for _ in range(3):
        frames = L.adsb_decode_device(d_dec._h, t.data_ptr(), N, C.byref(fr))
    assert frames > 0

    def kernel_ms():
        p = d_dec.profile()
        return p["big_ms"], p["big_launches"]

    steps = 5
    wall = {k: [] for k in builds}
    dec_wall, dec_k = [], []
    names = list(builds)
    for r in range(reps):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            B, h = builds[name]
            t0 = time.perf_counter()
            for _ in range(steps):
                B.adsb_power_device(h, t.data_ptr(), N, out.data_ptr(), M)
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        m0, l0 = kernel_ms()
        t0 = time.perf_counter()
        for _ in range(steps):
            L.adsb_decode_device(d_dec._h, t.data_ptr(), N, C.byref(fr))
        dec_wall.append((time.perf_counter() - t0) * 1e3 / steps)
        m1, l1 = kernel_ms()
        dec_k.append((m1 - m0) / max(1, l1 - l0))
    lines += [f"# (a) adsb_power_device, 256 Mi uint16 samples -> 128 Mi float32 power samples (512 MiB in, 512 MiB out); {reps} rounds x {steps} calls per side,",
              "#     the sides in rotation; wall time of the call (launch + kernel + the wait for it), medians (quartiles); traffic = 1 GiB / median",
              "#   side                                        call ms (q1 .. q3)              TB/s    / tree (median of rounds)"]
    base = wall[names[0]]
    for name in names:
        q = statistics.quantiles(wall[name], n=4)
        ratio = med([a / b for a, b in zip(wall[name], base)])
        lines.append(f"    {name:42s} {med(wall[name]):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {2 * 2 * N / (med(wall[name]) * 1e-3) * 1e-12:6.3f}   {ratio:.4f}")
        print(lines[-1], flush=True)
    q = statistics.quantiles(dec_k, n=4)
    lines += [f"    adsb_decode_device on the same capture: call {med(dec_wall):.4f} ms, its scan kernel {med(dec_k):.5f} ms per launch ({q[0]:.5f} .. {q[2]:.5f}), {frames} frames",
              "#   (the scan kernel has the same loads and FIR, everything else of the decoder, and no stores; DESIGN.md section 7's Stage A floors:",
              "#    0.098 ms loads, 0.098 ms arithmetic, 0.118 ms both)"]
    print(lines[-2], flush=True)
    del out

    NC = 1 << 27
    iq = t.view(torch.int16)[: 2 * NC]                      # (any int16 pairs: the kernel's time does not depend on the values)
    out = torch.empty(NC, dtype=torch.float32, device="cuda")
    d = capi.Decoder()
    ms = []
    for r in range(-3, reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            assert L.adsb_power_device_iq(d._h, 2, iq.data_ptr(), NC, out.data_ptr(), NC) == NC
        if r >= 0:
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
    from adsbdec_amd.sample_formats import iq_power
    for f in (0, NC // 2 + 4, NC - (1 << 20)):                # the head and two later trips of the grid
        assert np.array_equal(out[f: f + (1 << 20)].cpu().numpy().view(np.uint32),
                              iq_power(iq[2 * f: 2 * f + (1 << 21)].cpu().numpy().reshape(-1, 2)).view(np.uint32)), f
    q = statistics.quantiles(ms, n=4)
    lines += ["#", "# (b) adsb_power_device_iq (fmt 2), 128 Mi complex int16 samples -> 128 Mi power samples (512 MiB in, 512 MiB out); wall time of the call",
              f"    call {med(ms):.4f} ms ({q[0]:.4f} .. {q[2]:.4f})   {2 * 4 * NC / (med(ms) * 1e-3) * 1e-12:.3f} TB/s"]
    print(lines[-1], flush=True)
    del out, iq

    NH = 1 << 24
    x = t[:NH].cpu().numpy().view(np.uint16)
    ms = []
    for r in range(-2, max(5, reps // 2)):
        t0 = time.perf_counter()
        a = d.power_window_host(x, 0, 0, NH // 2)
        if r >= 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert len(a) == NH // 2
    lines += ["#", "# (c) adsb_power_window_host, 16 Mi samples (32 MiB in from pageable host memory, 32 MiB out to it); wall time of the call",
              f"    call {med(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})   {NH / (med(ms) * 1e-3) * 1e-9:.2f} GS/s"]
    print(lines[-1], flush=True)


def level_probe(L, reps, lines, variants):
    """The level report (level_kernel.hip, the adsb_level_* calls), every comparison interleaved in this one process, wall time of the
    calls (each waits for its kernels):
    (a) adsb_level_device with an envelope on 256 Mi samples of three contents -- the benchmark workload, clipped Gaussian noise, silence
        -- twice over (the A/A), beside adsb_power_device and adsb_decode_device on the same capture, and beside every build given with
        --variant name=path: measurement builds whose level_kernel.hip was compiled with another accumulation (-DADSB_LEVEL_HIST=k),
        flush (-DADSB_LEVEL_FLUSH=1) or grid cap (-DADSB_LEVEL_BLOCKS=n).  Every build gives the tree's report and envelope;
    (b) the element-wise flavours on 128 Mi units (fmt 2, fmt 8, power input) beside adsb_power_device_iq (fmt 2)."""
    import numpy as np
    from adsbdec_amd import levels
    M = N // 2
    work, _ = make_workload(torch, N, seed=1)
    g = torch.Generator(device="cuda").manual_seed(23)
    noise = (torch.randn(N, device="cuda", generator=g) * 600.0 + 2048.0).round_().clamp_(0, 4095).to(torch.int16)
    silence = torch.full((N,), 0x800, dtype=torch.int16, device="cuda")
    contents = {"workload": work, "noise": noise, "silence": silence}
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    out = torch.empty(M, dtype=torch.float32, device="cuda")
    KE = -(-M // 28)
    env = torch.empty(KE, dtype=torch.float32, device="cuda")
    d_dec = capi.Decoder(df18=False)
    fr = C.POINTER(capi.Frame)()

    def bind(path):
        B = C.CDLL(path)
        B.adsb_create.restype = C.c_void_p
        B.adsb_create.argtypes = [C.c_void_p]
        B.adsb_level_device.restype = C.c_long
        B.adsb_level_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
        cfg = capi.make_config()
        h = B.adsb_create(C.byref(cfg))
        assert h, path
        return B, h

    d_tree = capi.Decoder()
    tree = (L, d_tree._h)
    builds = {"tree": tree, "tree again (the A/A)": tree}
    for spec in variants:
        name, _, path = spec.partition("=")
        builds[name] = bind(path)
    rep = capi.LevelReport()
    steps = 5
    lines += [f"# (a) adsb_level_device with an envelope, 256 Mi uint16 samples -> the report of 128 Mi power samples (512 MiB in, {KE * 4 / 2 ** 20:.1f} MiB out);",
              f"#     {reps} rounds x {steps} calls per side, the sides in rotation; wall time of the call (memset + kernel + copy of the totals + the wait), medians (quartiles)"]
    summary = {}
    for cname, t in contents.items():
        ref = None
        for name, (B, h) in builds.items():                # warm-up, and every build gives the same report and envelope
            for _ in range(3):
                env.zero_()
                assert B.adsb_level_device(h, t.data_ptr(), N, C.byref(rep), env.data_ptr(), KE) == M, (name, cname)
            got = (capi.Decoder.level_dict(rep), env.clone())
            assert int(got[0]["hist"].sum()) + got[0]["negative"] == M == got[0]["samples"]
            if ref is None:
                ref = got
                piece = t[: 1 << 22].cpu().numpy().view(np.uint16)  # the head against the definition
                from oracle import oracle as O
                O.build()
                want = levels.level_report(O.power(piece)[: 1 << 21])
                kf = (1 << 21) // 28                        # (the head's whole runs: its last one is cut short in `want`)
                assert np.array_equal(ref[1][:kf].cpu().numpy().view(np.uint32), want["env"][:kf].view(np.uint32)), cname
            else:
                assert all(got[0][k] == ref[0][k] for k in ("negative", "rail_lo", "rail_hi", "over")) and np.array_equal(got[0]["hist"], ref[0]["hist"]), (name, cname)
                assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), (name, cname)
        h0 = ref[0]["hist"]
        for _ in range(3):
            assert L.adsb_power_device(d_tree._h, t.data_ptr(), N, out.data_ptr(), M) == M
            frames = L.adsb_decode_device(d_dec._h, t.data_ptr(), N, C.byref(fr))
        names = list(builds)
        wall = {k: [] for k in names}
        exp, dec = [], []
        for r in range(reps):
            order = names[r % len(names):] + names[:r % len(names)]
            for name in order:
                B, h = builds[name]
                t0 = time.perf_counter()
                for _ in range(steps):
                    B.adsb_level_device(h, t.data_ptr(), N, C.byref(rep), env.data_ptr(), KE)
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
            t0 = time.perf_counter()
            for _ in range(steps):
                L.adsb_power_device(d_tree._h, t.data_ptr(), N, out.data_ptr(), M)
            exp.append((time.perf_counter() - t0) * 1e3 / steps)
            t0 = time.perf_counter()
            for _ in range(steps):
                L.adsb_decode_device(d_dec._h, t.data_ptr(), N, C.byref(fr))
            dec.append((time.perf_counter() - t0) * 1e3 / steps)
        lines += ["#", f"#   content: {cname} -- {np.count_nonzero(h0)} bins, the fullest holds {100.0 * int(h0.max()) / M:.1f} % of the samples; rail_lo {ref[0]['rail_lo']}, rail_hi {ref[0]['rail_hi']}; {frames} frames",
                  "#   side                                        call ms (q1 .. q3)          / tree   / adsb_power_device (medians of rounds)"]
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            lines.append(f"    {name:42s} {med(wall[name]):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med([a / b for a, b in zip(wall[name], wall['tree'])]):.4f}   {med([a / b for a, b in zip(wall[name], exp)]):.4f}")
            print(lines[-1], flush=True)
        for name, v in (("adsb_power_device (512 MiB out)", exp), ("adsb_decode_device", dec)):
            q = statistics.quantiles(v, n=4)
            lines.append(f"    {name:42s} {med(v):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med([a / b for a, b in zip(v, wall['tree'])]):.4f}   {med([a / b for a, b in zip(v, exp)]):.4f}")
            print(lines[-1], flush=True)
        summary[cname] = med(wall["tree"])
    lines += ["#", "#   the tree's call by content: " + ", ".join(f"{k} {v:.4f} ms ({v / summary['workload']:.3f} x the workload's)" for k, v in summary.items())]
    print(lines[-1], flush=True)
    del out, noise, silence

    from tools.gen_signal import make_iq_workload
    from adsbdec_amd.sample_formats import to_int8_iq
    NC = 1 << 27
    # the generator is numpy's: one block of 4 Mi complex samples, repeated 32 times (as tools/format_probe.py --iq); its int8 twin
    # (>> 8); its power samples, one rounded operation per line as sample_formats.iq_power
    block, _ = make_iq_workload(1 << 22, seed=1)
    iq = torch.from_numpy(block.reshape(-1)).cuda().repeat(NC >> 22)
    iq8 = torch.from_numpy(to_int8_iq(block)[0].reshape(-1)).cuda().repeat(NC >> 22)
    sc = iq.view(-1, 2).to(torch.float32) * 0.0625
    ii, qq = sc[:, 0] * sc[:, 0], sc[:, 1] * sc[:, 1]
    pw = (ii + qq).contiguous()
    del sc, ii, qq
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    # the worst content found: the real workload's codes read as (I, Q) -- a constant offset of 2048 on both, so every power sample
    # lies in one of TWO neighbouring bins and hardly a run of 28 agrees: all 64 lanes of every increment on two LDS words
    two = work.view(torch.int16)[: 2 * NC]
    out = torch.empty(NC, dtype=torch.float32, device="cuda")
    KC = -(-NC // 28)
    d = d_tree
    assert L.adsb_level_device_iq(d._h, 2, two.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC) == NC
    two_bins = int(np.count_nonzero(np.ctypeslib.as_array(rep.hist)))
    assert L.adsb_level_device_iq(d._h, 2, iq.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC) == NC
    h2 = np.ctypeslib.as_array(rep.hist).copy()
    assert L.adsb_level_device_power(d._h, pw.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC) == NC
    assert np.array_equal(h2, np.ctypeslib.as_array(rep.hist)), "fmt 2 and its own power samples give different bins"
    sides = {
        "adsb_level_device_iq fmt 2 (512 MiB in)": lambda: L.adsb_level_device_iq(d._h, 2, iq.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC),
        "adsb_level_device_iq fmt 2 again (the A/A)": lambda: L.adsb_level_device_iq(d._h, 2, iq.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC),
        "adsb_level_device_iq fmt 8 (256 MiB in)": lambda: L.adsb_level_device_iq(d._h, 8, iq8.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC),
        "adsb_level_device_power (512 MiB in)": lambda: L.adsb_level_device_power(d._h, pw.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC),
        f"fmt 2, power samples in {two_bins} bins only": lambda: L.adsb_level_device_iq(d._h, 2, two.data_ptr(), NC, C.byref(rep), env.data_ptr(), KC),
        "adsb_power_device_iq fmt 2 (512 MiB out)": lambda: L.adsb_power_device_iq(d._h, 2, iq.data_ptr(), NC, out.data_ptr(), NC),
    }
    ms = {k: [] for k in sides}
    names = list(sides)
    for r in range(-2, reps):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            t0 = time.perf_counter()
            for _ in range(steps):
                assert sides[name]() == NC, name
            if r >= 0:
                ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    lines += ["#", f"# (b) the element-wise flavours, 128 Mi units, with an envelope; wall time of the call, medians (quartiles).  The capture: a 4 Mi-sample block of",
              f"#     tools/gen_signal.py make_iq_workload (seed 1) repeated 32 times ({np.count_nonzero(h2)} bins, the fullest {100.0 * int(h2.max()) / NC:.1f} % of the samples), its int8 twin, its power samples",
              "#   side                                        call ms (q1 .. q3)          / adsb_power_device_iq (median of rounds)"]
    base = ms[names[-1]]
    for name in names:
        q = statistics.quantiles(ms[name], n=4)
        lines.append(f"    {name:42s} {med(ms[name]):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med([a / b for a, b in zip(ms[name], base)]):.4f}")
        print(lines[-1], flush=True)


def export_batch_probe(L, reps, lines, parent):
    """The batch power export (power_export_batch_kernel.hip, the adsb_power_batch_* calls) against the loop of single calls, every
    comparison interleaved in this one process, wall time of the calls (each waits for its kernels; the ctypes arrays are built once):
    (a) 256 captures of 1 Mi uint16 samples; (b) the same for _packed, _as fmt 3 and fmt 1, _iq fmt 2 and fmt 0 (512 Ki complex samples
    each); (c) ONE capture of 256 Mi samples as a batch of one beside adsb_power_device -- the tree's, the tree's again (the A/A) and
    the parent commit's (--ab), loaded into this process; (d) 4096 captures of 2048 samples, every pass a plain-load pass."""
    import numpy as np
    from adsbdec_amd.packed12 import pack12
    t, _ = make_workload(torch, N, seed=1)
    d = capi.Decoder()
    h = d._h
    out = torch.empty(N // 2, dtype=torch.float32, device="cuda")
    out2 = torch.empty(N // 2, dtype=torch.float32, device="cuda")

    def arrays(base, stride_bytes, ns, obase, counts):
        k = len(ns)
        oat = np.concatenate([[0], np.cumsum(counts)[:-1]]) * 4
        return (k, (C.c_void_p * k)(*[base + i * stride_bytes for i in range(k)]), (C.c_size_t * k)(*ns),
                (C.c_void_p * k)(*[obase + int(o) for o in oat]), (C.c_size_t * k)(*counts))

    def leg(title, batch_fn, single_fn, src, elem_bytes, k, n, count, steps):
        """k captures of n units (elem_bytes each) from src, count floats each: batch, batch again, loop -- in rotation."""
        A = arrays(src.data_ptr(), int(n * elem_bytes), [n] * k, out.data_ptr(), [count] * k)
        A2 = arrays(src.data_ptr(), int(n * elem_bytes), [n] * k, out2.data_ptr(), [count] * k)

        def batch():
            assert batch_fn(*A) == k * count

        def loop(B=A2):
            for i in range(k):
                single_fn(B[1][i], n, B[3][i], count)
        for _ in range(2):
            batch()
            loop()
        torch.cuda.synchronize()
        assert torch.equal(out[: k * count].view(torch.int32), out2[: k * count].view(torch.int32)), title + ": the batch and the loop write other floats"
        sides = {"batch": batch, "batch again (the A/A)": batch, "loop of single calls": loop}
        wall = {s_: [] for s_ in sides}
        names = list(sides)
        for r in range(reps):
            for name in names[r % 3:] + names[:r % 3]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        aa = [b / a_ for a_, b in zip(wall[names[0]], wall[names[1]])]
        ratio = [b / a_ for a_, b in zip(wall[names[0]], wall[names[2]])]
        qa, qr = statistics.quantiles(aa, n=4), statistics.quantiles(ratio, n=4)
        lines.append(f"    {title:34s} batch {med(wall[names[0]]):9.4f} ms   loop {med(wall[names[2]]):9.4f} ms   loop / batch {med(ratio):7.3f} ({qr[0]:.3f} .. {qr[2]:.3f})"
                     f"   A/A {med(aa):.4f} ({qa[0]:.4f} .. {qa[2]:.4f})")
        print(lines[-1], flush=True)
        return med(ratio), med(aa)

    K, N1 = 256, 1 << 20
    lines += [f"# (a), (b) {K} captures side by side in one allocation; {reps} rounds x 3 calls per side, the sides in rotation; medians of the rounds (quartiles);",
              "#     every leg: the batch and the loop write the same floats (compared on the device) before anything is timed",
              "#   leg                                  one batch call        256 single calls     ratio of the rounds                    batch / batch"]
    S1 = lambda name: (lambda p, n, o, c: getattr(L, name)(h, p, n, o, c))
    S2 = lambda name, fmt: (lambda p, n, o, c: getattr(L, name)(h, fmt, p, n, o, c))
    B1 = lambda name: (lambda k, p, n, o, c: getattr(L, name)(h, k, p, n, o, c))
    B2 = lambda name, fmt: (lambda k, p, n, o, c: getattr(L, name)(h, fmt, k, p, n, o, c))
    leg("(a) uint16, 1 Mi samples each", B1("adsb_power_batch_device"), S1("adsb_power_device"), t, 2, K, N1, N1 // 2, 3)
    packed = torch.from_numpy(pack12(t[:N1].cpu().numpy().view(np.uint16))).cuda().repeat(K)
    leg("(b) _packed", B1("adsb_power_batch_device_packed"), S1("adsb_power_device_packed"), packed, 1.5, K, N1, N1 // 2, 3)
    del packed
    s16 = ((t.to(torch.int32) - 2048) * 16).to(torch.int16)
    leg("(b) _as fmt 3 INT16_REAL", B2("adsb_power_batch_device_as", S16), S2("adsb_power_device_as", S16), s16, 2, K, N1, N1 // 2, 3)
    del s16
    f32 = (t.to(torch.float32) - 2048.0) / 2048.0
    leg("(b) _as fmt 1 FLOAT32_REAL", B2("adsb_power_batch_device_as", F32), S2("adsb_power_device_as", F32), f32, 4, K, N1, N1 // 2, 3)
    del f32
    iq = t.view(torch.int16)
    leg("(b) _iq fmt 2, 512 Ki complex each", B2("adsb_power_batch_device_iq", 2), S2("adsb_power_device_iq", 2), iq, 4, K, N1 // 2, N1 // 2, 3)
    fiq = iq.to(torch.float32) / 32768.0
    leg("(b) _iq fmt 0, 512 Ki complex each", B2("adsb_power_batch_device_iq", 0), S2("adsb_power_device_iq", 0), fiq, 8, K, N1 // 2, N1 // 2, 3)
    del fiq, iq
    lines += ["#", "# (d) 4096 captures of 2048 samples: every pass takes the plain-load road (a capture's first pass always does)"]
    leg("(d) uint16, 2048 samples each", B1("adsb_power_batch_device"), S1("adsb_power_device"), t, 2, 4096, 2048, 1024, 1)

    # (c) one large capture: the batch of one beside the single call, the tree's and the parent's
    M = N // 2
    one = arrays(t.data_ptr(), 0, [N], out.data_ptr(), [M])
    sides = {"adsb_power_device (tree)": lambda: L.adsb_power_device(h, t.data_ptr(), N, out.data_ptr(), M),
             "adsb_power_device (tree again: the A/A)": lambda: L.adsb_power_device(h, t.data_ptr(), N, out.data_ptr(), M)}
    if parent:
        P = C.CDLL(parent)
        P.adsb_create.restype = C.c_void_p
        P.adsb_create.argtypes = [C.c_void_p]
        P.adsb_power_device.restype = C.c_long
        P.adsb_power_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        cfg = capi.make_config()
        ph = P.adsb_create(C.byref(cfg))
        assert ph, parent
        sides["adsb_power_device (parent commit)"] = lambda: P.adsb_power_device(ph, t.data_ptr(), N, out.data_ptr(), M)
    sides["adsb_power_batch_device, n_captures = 1"] = lambda: L.adsb_power_batch_device(h, *one)
    ref = None
    for name, fn in sides.items():
        for _ in range(3):
            assert fn() == M, name
        if ref is None:
            ref = out.clone()
        else:
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), name + ": other floats"
        out.zero_()
    del ref
    names, steps = list(sides), 5
    wall = {k_: [] for k_ in names}
    for r in range(reps):
        for name in names[r % len(names):] + names[:r % len(names)]:
            t0 = time.perf_counter()
            for _ in range(steps):
                sides[name]()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
    lines += ["#", f"# (c) ONE capture of 256 Mi samples (512 MiB in, 512 MiB out); {reps} rounds x {steps} calls per side, the sides in rotation; wall time of the call;",
              "#     every side writes the same floats",
              "#   side                                        call ms (q1 .. q3)              TB/s    / tree (median of rounds, q1 .. q3)"]
    base = wall[names[0]]
    for name in names:
        q = statistics.quantiles(wall[name], n=4)
        rr = [a_ / b for a_, b in zip(wall[name], base)]
        qr = statistics.quantiles(rr, n=4)
        lines.append(f"    {name:42s} {med(wall[name]):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {2 * 2 * N / (med(wall[name]) * 1e-3) * 1e-12:6.3f}   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
        print(lines[-1], flush=True)
    if not parent:
        lines += ["#   (the parent commit's library was not given with --ab: its side was not measured in this run)"]


def level_batch_probe(L, reps, lines, variants):
    """The batch level report (level_batch_kernel.hip, the adsb_level_batch_* calls) against the loop of single calls, every comparison
    interleaved in this one process, wall time of the calls (each waits for its kernels; the ctypes arrays are built once):
    (a) 256 captures of 1 Mi samples, every flavour; (b) 4096 captures of 2048 samples, with and without envelopes; (c) ONE capture of
    256 Mi samples as a batch of one beside adsb_level_device; (d) leg (a) on noise and on silence; (e) on (a), (b) and (c) every build
    given with --variant name=path beside the tree's: measurement builds whose level_batch_kernel.hip was compiled with another walk
    (-DADSB_LEVEL_BATCH_WALK=1) or end (-DADSB_LEVEL_BATCH_MERGE=0).  Every leg: the batch, the loop and every variant give the same reports and envelopes before anything
    is timed.  Returns whether on (a) and (b) the batch beats the loop by more than the A/A spread."""
    import numpy as np
    from adsbdec_amd.packed12 import pack12
    work, _ = make_workload(torch, N, seed=1)
    g = torch.Generator(device="cuda").manual_seed(23)
    noise = (torch.randn(N, device="cuda", generator=g) * 600.0 + 2048.0).round_().clamp_(0, 4095).to(torch.int16)
    silence = torch.full((N,), 0x800, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    KE = -(-(N // 2) // 28) + 4096
    env, env2 = torch.zeros(KE, dtype=torch.float32, device="cuda"), torch.zeros(KE, dtype=torch.float32, device="cuda")
    d = capi.Decoder()
    h = d._h
    SZ = C.sizeof(capi.LevelReport)

    def bind(path):
        B = C.CDLL(path)
        for name in ("adsb_create", "adsb_level_batch_device"):
            fn = getattr(B, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        cfg = capi.make_config()
        hh = B.adsb_create(C.byref(cfg))
        assert hh, path
        return B, hh

    others = {}
    for spec in variants:
        name, _, path = spec.partition("=")
        others[name] = bind(path)
    gates = []

    def leg(title, bname, sname, fmt, src, elem_bytes, k, n, m, steps, with_env=True, with_variants=False, gated=True):
        """k captures of n units (elem_bytes each) from src, m power samples each: batch, batch again, loop, variants -- in rotation."""
        ke = -(-m // 28)
        pl = [src.data_ptr() + int(i * n * elem_bytes) for i in range(k)]
        ptrs, ns = (C.c_void_p * k)(*pl), (C.c_size_t * k)(*([n] * k))
        el = [env2.data_ptr() + 4 * i * ke if with_env else None for i in range(k)]
        eb = ((C.c_void_p * k)(*[env.data_ptr() + 4 * i * ke for i in range(k)]), (C.c_size_t * k)(*([ke] * k))) if with_env else (None, None)
        cap = ke if with_env else 0
        rb, rl = (capi.LevelReport * k)(), (capi.LevelReport * k)()
        refs = [C.byref(rl, i * SZ) for i in range(k)]
        head = () if fmt is None else (fmt,)
        sfn = getattr(L, sname)

        def batch(B=L, hh=h):
            assert getattr(B, bname)(hh, *head, k, ptrs, ns, rb, *eb) == k * m

        def loop():
            for i in range(k):
                sfn(h, *head, pl[i], n, refs[i], el[i], cap)
        sides = {"batch": batch, "batch again (the A/A)": batch, "loop of single calls": loop}
        for _ in range(2):
            loop()
            batch()
        torch.cuda.synchronize()
        assert bytes(rb) == bytes(rl), title + ": the batch and the loop give other reports"
        assert torch.equal(env[: k * ke].view(torch.int32), env2[: k * ke].view(torch.int32)) or not with_env, title + ": other envelopes"
        if with_variants:
            for name, (B, hh) in others.items():
                C.memset(C.addressof(rb), 0, C.sizeof(rb))
                env.zero_()
                torch.cuda.synchronize()
                for _ in range(2):
                    batch(B, hh)
                assert bytes(rb) == bytes(rl), f"{title}: {name} gives other reports"
                assert torch.equal(env[: k * ke].view(torch.int32), env2[: k * ke].view(torch.int32)) or not with_env, f"{title}: {name}: other envelopes"
                sides[name] = (lambda B=B, hh=hh: batch(B, hh))
        wall = {s_: [] for s_ in sides}
        names = list(sides)
        for r in range(reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        aa = [b / a_ for a_, b in zip(wall[names[0]], wall[names[1]])]
        ratio = [b / a_ for a_, b in zip(wall[names[0]], wall[names[2]])]
        qa, qr = statistics.quantiles(aa, n=4), statistics.quantiles(ratio, n=4)
        lines.append(f"    {title:40s} batch {med(wall[names[0]]):9.4f} ms   loop {med(wall[names[2]]):9.4f} ms   loop / batch {med(ratio):7.3f} ({qr[0]:.3f} .. {qr[2]:.3f})"
                     f"   A/A {med(aa):.4f} ({qa[0]:.4f} .. {qa[2]:.4f})")
        print(lines[-1], flush=True)
        for name in names[3:]:
            rr = [b / a_ for a_, b in zip(wall[names[0]], wall[name])]
            q = statistics.quantiles(rr, n=4)
            lines.append(f"        (e) {name:32s} batch {med(wall[name]):9.4f} ms   / the tree's batch {med(rr):.4f} ({q[0]:.4f} .. {q[2]:.4f})")
            print(lines[-1], flush=True)
        if gated:
            gates.append((title, med(ratio) > 1.0 + max(abs(qa[0] - 1.0), abs(qa[2] - 1.0), abs(med(aa) - 1.0))))

    K, N1 = 256, 1 << 20
    steps = 5
    lines += [f"# (a) {K} captures of 1 Mi samples side by side in one allocation, an envelope each; {reps} rounds x {steps} calls per side, the sides in rotation;",
              "#     medians of the rounds (quartiles); every leg: the batch and the loop give the same reports and envelopes before anything is timed",
              "#   leg                                        one batch call        256 single calls     ratio of the rounds                    batch / batch"]
    t = work
    leg("(a) uint16", "adsb_level_batch_device", "adsb_level_device", None, t, 2, K, N1, N1 // 2, steps, with_variants=True)
    packed = torch.from_numpy(pack12(t[:N1].cpu().numpy().view(np.uint16))).cuda().repeat(K)
    leg("(a) _packed", "adsb_level_batch_device_packed", "adsb_level_device_packed", None, packed, 1.5, K, N1, N1 // 2, steps)
    del packed
    s16 = ((t.to(torch.int32) - 2048) * 16).to(torch.int16)
    leg("(a) _as fmt 3 INT16_REAL", "adsb_level_batch_device_as", "adsb_level_device_as", S16, s16, 2, K, N1, N1 // 2, steps)
    del s16
    f32 = (t.to(torch.float32) - 2048.0) / 2048.0
    leg("(a) _as fmt 1 FLOAT32_REAL", "adsb_level_batch_device_as", "adsb_level_device_as", F32, f32, 4, K, N1, N1 // 2, steps)
    del f32
    iq = t.view(torch.int16)
    leg("(a) _iq fmt 2, 512 Ki complex each", "adsb_level_batch_device_iq", "adsb_level_device_iq", 2, iq, 4, K, N1 // 2, N1 // 2, steps)
    fiq = iq.to(torch.float32) / 32768.0
    leg("(a) _iq fmt 0, 512 Ki complex each", "adsb_level_batch_device_iq", "adsb_level_device_iq", 0, fiq, 8, K, N1 // 2, N1 // 2, steps)
    del fiq
    iq8 = (iq >> 4).to(torch.int8)
    leg("(a) _iq fmt 8, 512 Ki complex each", "adsb_level_batch_device_iq", "adsb_level_device_iq", 8, iq8, 2, K, N1 // 2, N1 // 2, steps)
    del iq8
    pw = iq[: N // 2].to(torch.float32)
    pw = pw * pw
    leg("(a) _power, 512 Ki floats each", "adsb_level_batch_device_power", "adsb_level_device_power", None, pw, 4, K, N1 // 2, N1 // 2, steps)
    del pw, iq
    lines += ["#", "# (b) 4096 captures of 2048 samples (1024 power samples: one pass each, four sub-batches of 1024 captures)"]
    leg("(b) uint16, with envelopes", "adsb_level_batch_device", "adsb_level_device", None, t, 2, 4096, 2048, 1024, steps, with_variants=True)
    leg("(b) uint16, no envelope", "adsb_level_batch_device", "adsb_level_device", None, t, 2, 4096, 2048, 1024, steps, with_env=False, with_variants=True)
    lines += ["#", "# (d) leg (a), uint16, on other contents: Gaussian noise of sigma 600 codes round 2048, clipped to 0 .. 4095; silence (every code 0x800)"]
    leg("(d) uint16, noise", "adsb_level_batch_device", "adsb_level_device", None, noise, 2, K, N1, N1 // 2, steps, with_variants=True, gated=False)
    leg("(d) uint16, silence", "adsb_level_batch_device", "adsb_level_device", None, silence, 2, K, N1, N1 // 2, steps, with_variants=True, gated=False)

    # (c) one large capture: the batch of one beside the single call
    M = N // 2
    ke = -(-M // 28)
    one = (1, (C.c_void_p * 1)(t.data_ptr()), (C.c_size_t * 1)(N), None, (C.c_void_p * 1)(env.data_ptr()), (C.c_size_t * 1)(ke))
    rep1, repb = capi.LevelReport(), (capi.LevelReport * 1)()
    sides = {"adsb_level_device (tree)": lambda: L.adsb_level_device(h, t.data_ptr(), N, C.byref(rep1), env2.data_ptr(), ke),
             "adsb_level_device (tree again: the A/A)": lambda: L.adsb_level_device(h, t.data_ptr(), N, C.byref(rep1), env2.data_ptr(), ke),
             "adsb_level_batch_device, n_captures = 1": lambda: L.adsb_level_batch_device(h, 1, one[1], one[2], repb, one[4], one[5])}
    for name, (B, hh) in others.items():
        sides[f"... n_captures = 1, {name}"] = (lambda B=B, hh=hh: B.adsb_level_batch_device(hh, 1, one[1], one[2], repb, one[4], one[5]))
    for name, fn in sides.items():
        C.memset(C.addressof(repb), 0, SZ)
        for _ in range(3):
            assert fn() == M, name
        assert "adsb_level_device" in name or (bytes(repb) == bytes(rep1) and torch.equal(env[:ke].view(torch.int32), env2[:ke].view(torch.int32))), name
    names = list(sides)
    wall = {k_: [] for k_ in names}
    for r in range(reps):
        for name in names[r % len(names):] + names[:r % len(names)]:
            t0 = time.perf_counter()
            for _ in range(steps):
                sides[name]()
            wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
    lines += ["#", f"# (c) ONE capture of 256 Mi samples (512 MiB in), with its envelope; {reps} rounds x {steps} calls per side, the sides in rotation; wall time of the call;",
              "#     every side gives the same report and envelope; recorded, not gated",
              "#   side                                        call ms (q1 .. q3)          / tree (median of rounds, q1 .. q3)"]
    base = wall[names[0]]
    for name in names:
        q = statistics.quantiles(wall[name], n=4)
        rr = [a_ / b for a_, b in zip(wall[name], base)]
        qr = statistics.quantiles(rr, n=4)
        lines.append(f"    {name:42s} {med(wall[name]):.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
        print(lines[-1], flush=True)
    lines += ["#", "# gate: on (a) and (b) the batch call beats the loop of single calls by more than the A/A spread of the same leg"]
    for title, ok in gates:
        lines.append(f"    {title:40s} {'PASS' if ok else 'FAIL'}")
    print("\n".join(lines[-len(gates):]), flush=True)
    return all(ok for _, ok in gates)


def level_windows_probe(L, reps, lines, parent):
    """The window form of the level report (level_windows_kernel.hip, adsb_level_windows) on the benchmark's 256 Mi samples, every
    comparison interleaved in this one process, wall time of the calls (each waits for its kernel and its copy of the totals):
    (a) ONE window over the whole buffer beside adsb_level_device on the same buffer; (b) 1024 and 13 000 windows over the same buffer
    beside the loop of adsb_level_device on the slices -- the route without a window call, inexact at every slice's first six pairs;
    (c) adsb_level_device of this tree beside the library built from the parent commit (--ab).  Before anything is timed: the window
    reports add up (adsb_level_add) to adsb_level_device's report, word for word, and the envelopes are equal."""
    t, _ = make_workload(torch, N, seed=1)
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    M = N // 2
    ke = -(-M // 28)
    env, env2 = torch.zeros(ke, dtype=torch.float32, device="cuda"), torch.zeros(ke, dtype=torch.float32, device="cuda")
    d = capi.Decoder()
    h = d._h
    SZ = C.sizeof(capi.LevelReport)
    rep1 = capi.LevelReport()
    steps = 5

    def single(B=L, hh=h):
        assert B.adsb_level_device(hh, t.data_ptr(), N, C.byref(rep1), env2.data_ptr(), ke) == M

    def rotate(sides):
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table(names, wall, base):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:46s} {med(wall[name]):9.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
            print(lines[-1], flush=True)

    def windows(k):
        """k windows over [0, M): M / k rounded down to a multiple of 28 each, the last one takes the rest"""
        win = M // k // 28 * 28
        e = [i * win for i in range(k)] + [M]
        return (C.c_uint64 * (k + 1))(*e), e, (capi.LevelReport * k)()

    def check(k, edges, reps_k):
        for _ in range(2):
            single()
        env.zero_()
        torch.cuda.synchronize()
        assert L.adsb_level_windows(h, t.data_ptr(), 0, N, k, edges, reps_k, env.data_ptr(), ke) == M
        total = capi.LevelReport()
        for i in range(k):
            L.adsb_level_add(C.byref(total), C.byref(reps_k, i * SZ))
        assert bytes(total) == bytes(rep1), f"{k} windows do not add up to adsb_level_device's report"
        assert torch.equal(env.view(torch.int32), env2.view(torch.int32)), f"{k} windows: another envelope"

    # (a)
    e1, _, r1 = windows(1)
    check(1, e1, r1)
    sides = {"adsb_level_device": single, "adsb_level_device again (the A/A)": single,
             "adsb_level_windows, n_windows = 1": lambda: L.adsb_level_windows(h, t.data_ptr(), 0, N, 1, e1, r1, env.data_ptr(), ke)}
    names, wall = rotate(sides)
    lines += [f"# (a) ONE window over 256 Mi samples (512 MiB in) beside adsb_level_device on the same buffer, both with the envelope; {reps} rounds x {steps}",
              "#     calls per side, the sides in rotation; the same report and envelope from both before anything is timed",
              "#   side                                              call ms (q1 .. q3)             / adsb_level_device (median of rounds, q1 .. q3)"]
    table(names, wall, names[0])
    # (b)
    lines += ["#", "# (b) K windows over the same buffer in ONE adsb_level_windows call beside K adsb_level_device calls on the slices (each a fresh stream:",
              "#     its first six pairs see silence, so those reports do not add up to the capture's); no envelope on either side; the window reports",
              "#     add up to adsb_level_device's report of the whole buffer, word for word",
              "#   K       window (power samples)   adsb_level_windows ms   again / first (the A/A)      loop of single calls ms   loop / windows (q1 .. q3)"]
    for k in (1024, 13000):
        ek, el, rk = windows(k)
        check(k, ek, rk)
        ptrs = [t.data_ptr() + 4 * el[i] for i in range(k)]
        ns = [2 * (el[i + 1] - el[i]) for i in range(k)]
        one = capi.LevelReport()

        def call(k=k, ek=ek, rk=rk):
            assert L.adsb_level_windows(h, t.data_ptr(), 0, N, k, ek, rk, None, 0) == M

        def loop(k=k, ptrs=ptrs, ns=ns):
            for i in range(k):
                L.adsb_level_device(h, ptrs[i], ns[i], C.byref(one), None, 0)
        loop()
        names, wall = rotate({"windows": call, "again": call, "loop": loop})
        aa = [b / a_ for a_, b in zip(wall["windows"], wall["again"])]
        rr = [b / a_ for a_, b in zip(wall["windows"], wall["loop"])]
        qa, qr = statistics.quantiles(aa, n=4), statistics.quantiles(rr, n=4)
        lines.append(f"    {k:<7d} {el[1]:<24d} {med(wall['windows']):9.4f}               {med(aa):.4f} ({qa[0]:.4f} .. {qa[2]:.4f})     {med(wall['loop']):10.4f}"
                     f"                {med(rr):8.3f} ({qr[0]:.3f} .. {qr[2]:.3f})")
        print(lines[-1], flush=True)
    # (c)
    lines += ["#", "# (c) adsb_level_device of this tree beside the library built from the parent commit, loaded into this process: the existing call did not move"]
    if parent:
        B = C.CDLL(parent)
        for name in ("adsb_create", "adsb_level_device"):
            fn = getattr(B, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        assert not hasattr(B, "adsb_level_windows"), "the --ab library is not the parent's: it has the window call"
        cfg = capi.make_config()
        hh = B.adsb_create(C.byref(cfg))
        assert hh, parent
        single()
        want = bytes(rep1)
        single(B, hh)
        assert bytes(rep1) == want, "the parent's library reports other levels"
        names, wall = rotate({"adsb_level_device (tree)": single, "adsb_level_device (tree again: the A/A)": single,
                              "adsb_level_device (parent commit)": lambda: single(B, hh)})
        lines.append("#   side                                              call ms (q1 .. q3)             / tree (median of rounds, q1 .. q3)")
        table(names, wall, names[0])
    else:
        lines.append("#     not measured in this run: no --ab parent library given")


def bursts_probe(L, reps, lines, parent):
    """The gate behind the envelope (burst_kernel.hip, adsb_bursts_device) on the envelope of the benchmark's 256 Mi samples (about 4.8 M
    runs), every comparison interleaved in this one process, wall time of the calls (each ends with the table in HOST memory):
    (a) at three densities of hot runs, beside the same gate written in torch on the device and beside a copy of the envelope to the
    host and levels.bursts; (b) adsb_level_device with the envelope, alone and followed by the gate; (c) adsb_level_device of this tree
    beside the library built from the parent commit (--ab).  Before anything is timed every side's table is levels.bursts's."""
    import numpy as np
    from adsbdec_amd import levels
    t, _ = make_workload(torch, N, seed=1)
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    M = N // 2
    ke = -(-M // 28)
    env = torch.zeros(ke, dtype=torch.float32, device="cuda")
    d = capi.Decoder()
    h = d._h
    rep1 = capi.LevelReport()
    steps = 3

    def level(B=L, hh=h):
        assert B.adsb_level_device(hh, t.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M
    level()
    median = L.adsb_level_percentile(C.byref(rep1), 0.5)
    threshold = float(np.float32(capi.Decoder.BURST_FACTOR * median))
    tb = int(np.array([threshold], dtype="<f4").view("<u4")[0])
    big = float(np.float32(1.0e6 * max(median, 1.0)))
    g = torch.Generator(device="cuda").manual_seed(1)
    dense = env.clone()                                    # 10 % of the runs hot, in stretches of 43 runs (a long frame is 1200 power samples)
    starts = torch.randint(0, ke - 43, (ke // 430,), generator=g, device="cuda")
    dense[(starts[:, None] + torch.arange(43, device="cuda")[None, :]).flatten()] = big
    second = env.clone().clamp_(max=threshold / 2)         # every second run hot, the others below the threshold
    second[::2] = big
    table = np.zeros(ke // 2 + 8, dtype=levels.BURST_DTYPE)

    def lib(e, lead, hang):
        b = L.adsb_bursts_device(h, e.data_ptr(), ke, threshold, lead, hang, table.ctypes.data, table.size)
        assert 0 <= b <= table.size
        return table[:b]

    def torch_gate(e, lead, hang):
        """What a caller has today: elementwise kernels, two nonzero() (each waits for the device), a segmented maximum, five copies."""
        u = e.view(torch.int32).clamp(min=0)               # (sign set -> 0; sign-clear patterns compare as signed integers do)
        hot = torch.nonzero(u >= tb).flatten()
        if hot.numel() == 0:
            return np.zeros(0, dtype=levels.BURST_DTYPE)
        cut = torch.nonzero(hot[1:] - hot[:-1] > lead + hang + 1).flatten() + 1
        zero, n = torch.zeros(1, dtype=cut.dtype, device="cuda"), torch.full((1,), hot.numel(), dtype=cut.dtype, device="cuda")
        first, last = torch.cat([zero, cut]), torch.cat([cut, n]) - 1
        out = np.zeros(first.numel(), dtype=levels.BURST_DTYPE)
        out["begin"] = (hot[first] - lead).clamp(min=0).cpu().numpy()
        out["end"] = (hot[last] + hang + 1).clamp(max=ke).cpu().numpy()
        out["hot"] = (last - first + 1).cpu().numpy()
        out["peak"] = torch.segment_reduce(e[hot], "max", lengths=last - first + 1).cpu().numpy()    # (no NaN in these envelopes)
        return out

    def host(e, lead, hang):
        return levels.bursts(e.cpu().numpy(), threshold, lead, hang)

    def rotate(sides):
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table_of(names, wall, base):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:46s} {med(wall[name]):9.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
            print(lines[-1], flush=True)

    # (a)
    lines += [f"# (a) adsb_bursts_device on an envelope of {ke} runs, threshold {threshold:.9g} ({capi.Decoder.BURST_FACTOR:g} x the median {median:.9g}); {reps} rounds x {steps} calls",
              "#     per side, the sides in rotation; every side ends with its table in host memory, and all three gave levels.bursts's table before",
              "#     anything was timed.  sparse: the benchmark workload's own envelope; dense: 10 % of its runs made hot in stretches of 43; second:",
              "#     every second run hot with lead = hang = 0, the most bursts there can be.",
              "#   side                                              call ms (q1 .. q3)             / adsb_bursts_device (median of rounds, q1 .. q3)"]
    for what, e, lead, hang in (("sparse, lead 2 hang 4", env, 2, 4), ("sparse, lead 2 hang 1468 (the defaults)", env, 2, capi.Decoder.BURST_HANG),
                                ("dense 10 %, lead 2 hang 4", dense, 2, 4), ("every second run hot, lead 0 hang 0", second, 0, 0)):
        want = host(e, lead, hang)
        for side in (lib, torch_gate):
            got = side(e, lead, hang)
            assert got.size == want.size and all(np.array_equal(got[k_], want[k_]) for k_ in ("begin", "end", "hot")), (what, side.__name__)
            assert np.array_equal(got["peak"].view(np.uint32), want["peak"].view(np.uint32)), (what, side.__name__, "peak")
        lines.append(f"#   {what}: B = {want.size}, hot runs = {int(want['hot'].sum())}")
        names, wall = rotate({"adsb_bursts_device": lambda: lib(e, lead, hang), "adsb_bursts_device again (the A/A)": lambda: lib(e, lead, hang),
                              "the gate in torch on the device": lambda: torch_gate(e, lead, hang),
                              "envelope to the host, levels.bursts": lambda: host(e, lead, hang)})
        table_of(names, wall, names[0])
        table.view(np.uint8)[:] = 0xA5                     # ... and behind the timed calls, into a poisoned table: still that table
        got = lib(e, lead, hang)
        assert got.tobytes() == want.tobytes() and (table[want.size:].view(np.uint8) == 0xA5).all(), what
    # (b)
    lines += ["#", "# (b) adsb_level_device with the envelope on the 256 Mi samples, alone and followed by the gate (the defaults) on what it wrote"]

    def both():
        level()
        lib(env, capi.Decoder.BURST_LEAD, capi.Decoder.BURST_HANG)
    names, wall = rotate({"adsb_level_device": level, "adsb_level_device again (the A/A)": level, "adsb_level_device + adsb_bursts_device": both})
    lines.append("#   side                                              call ms (q1 .. q3)             / adsb_level_device (median of rounds, q1 .. q3)")
    table_of(names, wall, names[0])
    # (c)
    lines += ["#", "# (c) adsb_level_device of this tree beside the library built from the parent commit, loaded into this process: the existing call did not move"]
    if parent:
        B = C.CDLL(parent)
        for name in ("adsb_create", "adsb_level_device"):
            fn = getattr(B, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        assert not hasattr(B, "adsb_bursts_device"), "the --ab library is not the parent's: it has the gate"
        cfg = capi.make_config()
        hh = B.adsb_create(C.byref(cfg))
        assert hh, parent
        level()
        want = bytes(rep1)
        level(B, hh)
        assert bytes(rep1) == want, "the parent's library reports other levels"
        names, wall = rotate({"adsb_level_device (tree)": level, "adsb_level_device (tree again: the A/A)": level,
                              "adsb_level_device (parent commit)": lambda: level(B, hh)})
        lines.append("#   side                                              call ms (q1 .. q3)             / tree (median of rounds, q1 .. q3)")
        table_of(names, wall, names[0])
    else:
        lines.append("#     not measured in this run: no --ab parent library given")


def burst_stream_probe(L, reps, lines, parent):
    """The gate of a slice of a stream (burst_slice_kernel.hip, adsb_bursts_slice_device) and the host program's record mode (-S -O), wall
    time, the sides of a leg interleaved in this one process, the A/A beside every ratio: (a) the envelope of the benchmark's 256 Mi
    samples as ONE slice beside adsb_bursts_device on it -- the price of the carry; (b) the same envelope in 16 slices beside the one
    call; (c) adsb_bursts_device beside the library built from the parent commit (--ab); (d) the host program: -S 48,2,4 -O on the
    256 Mi-sample file beside -L -U 48,2,4 -K on it, each a process of its own, with where the record mode's time went.  Before anything
    is timed every side's table is levels.bursts's, and the two archives are equal byte for byte."""
    import subprocess
    import tempfile
    import numpy as np
    from adsbdec_amd import levels
    t, _ = make_workload(torch, N, seed=1)
    torch.cuda.synchronize()
    M = N // 2
    ke = -(-M // 28)
    env = torch.zeros(ke, dtype=torch.float32, device="cuda")
    d = capi.Decoder()
    h = d._h
    rep1 = capi.LevelReport()
    steps = 3
    assert L.adsb_level_device(h, t.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M
    median = L.adsb_level_percentile(C.byref(rep1), 0.5)
    threshold = float(np.float32(capi.Decoder.BURST_FACTOR * median))
    lead, hang = 2, 4
    want = levels.bursts(env.cpu().numpy(), threshold, lead, hang)
    table = np.zeros(want.size + 8, dtype=levels.BURST_DTYPE)
    carry, zero = levels.burst_carry(), levels.burst_carry()

    def one(B=L, hh=h):
        b = B.adsb_bursts_device(hh, env.data_ptr(), ke, threshold, lead, hang, table.ctypes.data, table.size)
        assert b == want.size
        return table[:b]

    def sliced(k):
        """k slices of equal length (the last takes the rest), the records one behind the other in the table"""
        edges = [ke * i // k for i in range(k)] + [ke]
        carry[:] = zero
        at = 0
        for i in range(k):
            b = L.adsb_bursts_slice_device(h, env.data_ptr() + 4 * edges[i], edges[i + 1] - edges[i], threshold, lead, hang, carry.ctypes.data,
                                           int(i == k - 1), table.ctypes.data + 16 * at, table.size - at, carry.ctypes.data)
            assert b >= 0
            at += b
        assert at == want.size
        return table[:at]

    def rotate(sides):
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table_of(names, wall, base):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:52s} {med(wall[name]):9.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
            print(lines[-1], flush=True)

    for side in (one, lambda: sliced(1), lambda: sliced(16)):
        assert side().tobytes() == want.tobytes()
    lines += [f"# (a), (b) an envelope of {ke} runs, threshold {threshold:.9g}, lead {lead} hang {hang}: B = {want.size}; {reps} rounds x {steps} calls per side, the",
              "#     sides in rotation; every side ends with its table in host memory and gave levels.bursts's table before anything was timed",
              "#   side                                                    call ms (q1 .. q3)             / adsb_bursts_device (median of rounds, q1 .. q3)"]
    names, wall = rotate({"adsb_bursts_device": one, "adsb_bursts_device again (the A/A)": one,
                          "adsb_bursts_slice_device, ONE slice": lambda: sliced(1), "adsb_bursts_slice_device, 16 slices": lambda: sliced(16)})
    table_of(names, wall, names[0])
    lines += ["#", "# (c) adsb_bursts_device of this tree beside the library built from the parent commit, loaded into this process"]
    if parent:
        B = C.CDLL(parent)
        for name in ("adsb_create", "adsb_bursts_device"):
            fn = getattr(B, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        assert not hasattr(B, "adsb_bursts_slice_device"), "the --ab library is not the parent's: it has the slice call"
        cfg = capi.make_config()
        hh = B.adsb_create(C.byref(cfg))
        assert hh, parent
        assert one(B, hh).tobytes() == want.tobytes(), "the parent's library gives another table"
        names, wall = rotate({"adsb_bursts_device (tree)": one, "adsb_bursts_device (tree again: the A/A)": one,
                              "adsb_bursts_device (parent commit)": lambda: one(B, hh)})
        lines.append("#   side                                                    call ms (q1 .. q3)             / tree (median of rounds, q1 .. q3)")
        table_of(names, wall, names[0])
    else:
        lines.append("#     not measured in this run: no --ab parent library given")
    # (d) the host program, a process per run
    lines += ["#", f"# (d) the host program on a file of the {N} samples ({2 * N >> 20} MiB, in the page cache): wall time of the whole process, the two runs in turn;",
              "#     [record]: the record mode's own account (ADSB_CLI_TIMING=1) of its last run"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "capture.bin")
        t.cpu().numpy().tofile(path)
        cmds = {"-L -U 48,2,4 -K": [capi.CLI_PATH, "-L", "-U", "48,2,4", "-K", os.path.join(tmp, "k.brs"), "-f", path],
                "-S 48,2,4 -O (pieces of 299593 runs)": [capi.CLI_PATH, "-S", "48,2,4", "-O", os.path.join(tmp, "s.brs"), "-f", path]}
        wall = {k_: [] for k_ in cmds}
        account = ""
        for r in range(max(3, reps // 4)):
            for name in list(cmds)[r % 2:] + list(cmds)[:r % 2]:
                t0 = time.perf_counter()
                q = subprocess.run(cmds[name], capture_output=True, env=dict(os.environ, ADSB_CLI_TIMING="1"))
                wall[name].append((time.perf_counter() - t0) * 1e3)
                assert q.returncode == 0, q.stderr.decode()[-2000:]
                account = next((ln for ln in q.stderr.decode().splitlines() if ln.startswith("[record]")), account)
        k_arch, s_arch = (open(os.path.join(tmp, f), "rb").read() for f in ("k.brs", "s.brs"))
        same = k_arch == s_arch     # (the first piece's median bin is the whole file's on this workload, or the thresholds differ)
        lines.append(f"#     the two archives: {len(k_arch)} and {len(s_arch)} bytes of {2 * N}, {'equal byte for byte' if same else 'thresholds differ: ' + str(k_arch[36:40] != s_arch[36:40])}")
        lines.append("#   run                                                     process ms (q1 .. q3)          / -L -U -K")
        for name in cmds:
            q = statistics.quantiles(wall[name], n=4)
            lines.append(f"    {name:52s} {med(wall[name]):9.1f} ({q[0]:.1f} .. {q[2]:.1f})   {med(wall[name]) / med(wall['-L -U 48,2,4 -K']):.3f}")
            print(lines[-1], flush=True)
        lines.append("#     " + account)
        rate = 2.0 * N / (med(wall["-S 48,2,4 -O (pieces of 299593 runs)"]) * 1e-3) / 1e6
        lines.append(f"#     the record mode takes the file at {rate:.0f} MB/s, the process's start included: {rate / 40.0:.1f} x a live stream's 40 MB/s")


def flush_probe(L, reps, lines, parent):
    """Flush (adsb_set_flush), every comparison interleaved in this one process, wall time of the calls, the run's A/A beside every ratio:
    (1) adsb_decode_device on the benchmark capture: the tree without flush beside itself (the A/A), beside the library built from the
    parent commit (--ab) and beside a flush handle; (2) 4 096 captures of 2 048 samples through adsb_decode_batch_device on a flush
    handle, beside the loop of single flush calls and beside adsb_power_batch_device on the same batch; (3) the gated pipeline --
    adsb_level_device with the envelope, adsb_bursts_device at lead 2 hang 4, ONE adsb_decode_batch_device of the pieces on a flush handle
    -- beside the whole decode, on a sparse capture (the pipeline fixture's density: 6 frames per million power samples) and on the
    benchmark workload (a frame per millisecond)."""
    import numpy as np
    from adsbdec_amd import levels
    out = C.POINTER(capi.Frame)()
    steps = 3

    def rotate(sides, steps=steps):
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(-1, reps):                            # (round -1: the warm-up)
            for name in names[r % len(names):] + names[:r % len(names)]:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                if r >= 0:
                    wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table_of(names, wall, base):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:58s} {med(wall[name]):10.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
            print(lines[-1], flush=True)

    head = "#   side                                                          call ms (q1 .. q3)               / the first side (median of rounds, q1 .. q3)"
    t, _ = make_workload(torch, N, seed=1)
    torch.cuda.synchronize()                               # (the library's streams do not wait for torch's)
    plain, flush = capi.Decoder(), capi.Decoder(flush=True)

    def dec(B, hh):
        k = B.adsb_decode_device(hh, t.data_ptr(), N, C.byref(out))
        assert k >= 0
        return k
    k_plain, k_flush = dec(L, plain._h), dec(L, flush._h)
    lines += [f"# (1) adsb_decode_device on the benchmark capture (make_workload, 256 Mi samples, seed 1): {k_plain} frames without flush, {k_flush} with it;",
              f"#     {reps} rounds x {steps} calls per side, the sides in rotation", head]
    sides = {"tree, flush off": lambda: dec(L, plain._h), "tree, flush off again (the A/A)": lambda: dec(L, plain._h)}
    if parent:
        B = C.CDLL(parent)
        for name in ("adsb_create", "adsb_decode_device"):
            fn = getattr(B, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        assert not hasattr(B, "adsb_set_flush"), "the --ab library is not the parent's: it has the flush"
        cfg = capi.make_config()
        hh = B.adsb_create(C.byref(cfg))
        assert hh, parent
        assert dec(B, hh) == k_plain
        sides["parent commit"] = lambda: dec(B, hh)
    else:
        lines.append("#     (no --ab parent library given: the parent's side is missing)")
    sides["tree, flush on"] = lambda: dec(L, flush._h)
    names, wall = rotate(sides)
    table_of(names, wall, names[0])

    # (2)
    K, NS = 4096, 2048
    rng = np.random.default_rng(30)
    from tools import gen_signal as G
    host = np.empty((K, NS), np.uint16)
    for i in range(K):
        frames = [(int(rng.integers(0, NS - 1300)), G.make_frame(11, rng), float(rng.uniform(300, 1500)), 0.3)] if i % 16 == 7 else []
        host[i] = G.synth(NS, frames, 8.0, 4000 + i)
    batch = torch.from_numpy(host.view(np.int16)).cuda()
    ptrs = (C.c_void_p * K)(*[batch.data_ptr() + 2 * NS * i for i in range(K)])
    ns = (C.c_size_t * K)(*[NS] * K)
    first = (C.c_uint64 * (K + 1))()
    pw = torch.empty(K * NS // 2, dtype=torch.float32, device="cuda")
    pptrs = (C.c_void_p * K)(*[pw.data_ptr() + 4 * (NS // 2) * i for i in range(K)])
    caps = (C.c_size_t * K)(*[NS // 2] * K)

    def batch_flush():
        k = L.adsb_decode_batch_device(flush._h, K, ptrs, ns, C.byref(out), first, None)
        assert k >= 0
        return k

    def loop_flush():
        tot = 0
        for i in range(K):
            tot += L.adsb_decode_device(flush._h, ptrs[i], NS, C.byref(out))
        return tot

    def export():
        assert L.adsb_power_batch_device(plain._h, K, ptrs, ns, pptrs, caps) >= 0
    kb = batch_flush()
    assert kb == loop_flush() and kb >= K // 32, kb
    assert L.adsb_decode_batch_device(plain._h, K, ptrs, ns, C.byref(out), first, None) == 0
    lines += ["#", f"# (2) {K} captures of {NS} samples, a short frame in every 16th: adsb_decode_batch_device on a flush handle ({kb} frames; without flush: 0,",
              "#     by construction), the loop of single flush calls, and adsb_power_batch_device on the same batch; one call per side and round", head]
    names, wall = rotate({"adsb_decode_batch_device, flush": batch_flush, "adsb_decode_batch_device, flush again (the A/A)": batch_flush,
                          "loop of 4 096 adsb_decode_device, flush": loop_flush, "adsb_power_batch_device": export}, steps=1)
    table_of(names, wall, names[0])
    del batch, pw

    # (3)
    M = N // 2
    ke = -(-M // 28)
    env = torch.zeros(ke, dtype=torch.float32, device="cuda")
    rep1 = capi.LevelReport()
    for what, cap_t in (("sparse: 805 frames in 256 Mi samples (the pipeline fixture's 6 per million power samples)", make_workload(torch, N, n_frames=805, seed=2)[0]),
                        ("the benchmark workload: a frame per millisecond", t)):
        torch.cuda.synchronize()
        table = np.zeros(1 << 15, dtype=levels.BURST_DTYPE)
        state = {}

        def whole():
            k = L.adsb_decode_device(plain._h, cap_t.data_ptr(), N, C.byref(out))
            assert k >= 0
            return k

        def gated():
            assert L.adsb_level_device(plain._h, cap_t.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M
            thr = float(np.float32(capi.Decoder.BURST_FACTOR * L.adsb_level_percentile(C.byref(rep1), 0.5)))
            b = L.adsb_bursts_device(plain._h, env.data_ptr(), ke, thr, 2, 4, table.ctypes.data, table.size)
            assert 0 <= b <= table.size, b
            begin, end = table["begin"][:b].astype(np.int64), np.minimum(table["end"][:b].astype(np.int64) * 28, M)
            pp = (C.c_void_p * max(1, b))(*[cap_t.data_ptr() + 112 * int(v) for v in begin])          # (56 samples a run: 112 bytes, 16-byte aligned)
            nn = (C.c_size_t * max(1, b))(*[int(2 * (e - 28 * s)) for s, e in zip(begin, end)])
            ff = (C.c_uint64 * (b + 1))()
            k = L.adsb_decode_batch_device(flush._h, b, pp, nn, C.byref(out), ff, None)
            assert k >= 0
            state.update(b=b, k=k, cover=float(sum(nn)) / N)
            return k
        kw, kg = whole(), gated()
        lines += ["#", f"# (3) {what}: the whole decode finds {kw} frames; the gate gives {state['b']} pieces that cover {100 * state['cover']:.2f} % of the capture",
                  f"#     and hold {kg} frames (a piece is decoded as a capture of its own: a frame the gate cuts, or one behind the whole decode's horizon, differs)", head]
        names, wall = rotate({"adsb_decode_device (the whole capture)": whole, "adsb_decode_device again (the A/A)": whole,
                              "level + gate (lead 2, hang 4) + batch flush decode": gated}, steps=1)
        table_of(names, wall, names[0])
    lines += ["#", "# The pipeline's cost on the benchmark workload is tile count: every piece takes a tile of two passes (12 880 offsets) of its own whatever its",
              "# length, beside the gate's round trips.  Pieces that share a tile are the follow-up; not built here."]


def gather_probe(L, reps, lines, parent, variants=()):
    """The burst gather (adsb_gather_device, gather_kernel.hip) and the burst archive, every comparison interleaved in this one process,
    wall time of the calls, the run's A/A beside every ratio:
    (a) the gather of the bursts the gate finds at lead 2, hang 4 on the benchmark workload and on the sparse capture, beside itself (the
        A/A), beside a loop of one device-to-device copy per piece, a loop of one device-to-host copy per
        piece, and the same gather written in torch on the device;
    (b) its effective bytes per second beside adsb_power_device's, the nearest all-load-all-store kernel, with one burst that is the
        whole capture and with the benchmark's bursts;
    (c) archive bytes over capture bytes for both captures;
    (d) end to end from page-locked host memory: the archive's pieces through ONE adsb_decode_batch_host on a flush handle beside the
        host-fed decode of the whole capture (adsb_push);
    (e) s = 2 with every begin odd beside every begin even, and the same two tables through every --variant name=path: a measurement
        build of the library whose gather_kernel.hip loads a full word another way (-DADSB_GATHER_LOAD=0);
    (f) adsb_level_device and adsb_decode_device beside the parent commit's library (--ab)."""
    import numpy as np
    from adsbdec_amd import burst_archive as BA, levels
    out = C.POINTER(capi.Frame)()

    order_rng = __import__("random").Random(32)

    def rotate(sides, steps=1):
        """Every round runs the sides in a NEW random order (seeded), so no side always runs behind the same neighbour."""
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(-1, reps):                            # (round -1: the warm-up)
            order = names[:]
            order_rng.shuffle(order)
            for name in order:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                if r >= 0:
                    wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table_of(names, wall, base, note=None):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:62s} {med(wall[name]):10.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})"
                         + (note(name, med(wall[name])) if note else ""))
            print(lines[-1], flush=True)

    head = "#   side                                                              call ms (q1 .. q3)               / the first side (median of rounds, q1 .. q3)"
    M = N // 2
    ke = -(-M // 28)
    d = capi.Decoder()
    flush = capi.Decoder(flush=True)
    env = torch.zeros(ke, dtype=torch.float32, device="cuda")
    rep1 = capi.LevelReport()
    dst = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    pinned = torch.empty(2 * N, dtype=torch.uint8).pin_memory()
    t_bench = make_workload(torch, N, seed=1)[0]
    captures = (("the benchmark workload: a frame per millisecond", t_bench),
                ("sparse: 805 frames in 256 Mi samples", make_workload(torch, N, n_frames=805, seed=2)[0]))
    torch.cuda.synchronize()
    kept = {}
    for what, cap_t in captures:
        assert L.adsb_level_device(d._h, cap_t.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M
        thr = float(np.float32(capi.Decoder.BURST_FACTOR * L.adsb_level_percentile(C.byref(rep1), 0.5)))
        tab, b = d.bursts_device(env.data_ptr(), ke, thr, 2, 4, 1 << 16)
        assert 0 < b <= 1 << 16
        tab = np.ascontiguousarray(tab)
        off = BA.layout(tab, M, 4)
        total = int(off[-1])
        sl = levels.burst_samples(tab, M)
        cap_b = cap_t.view(torch.uint8)
        src_lo, nbytes = [4 * int(lo) for lo, _ in sl], [4 * int(hi - lo) for lo, hi in sl]
        offs = [int(o) for o in off[:-1]]
        offp = np.zeros(b + 1, np.uint64)

        def call():
            got = L.adsb_gather_device(d._h, cap_t.data_ptr(), 2 * N, 4, M, tab.ctypes.data, b, dst.data_ptr(), 2 * N, offp.ctypes.data)
            assert got == total, (got, capi.load().adsb_last_error(d._h))

        def call_and_copy():
            call()
            pinned[:total].copy_(dst[:total], non_blocking=True)
            torch.cuda.synchronize()

        def loop_d2d():
            for a_, n_, o_ in zip(src_lo, nbytes, offs):
                dst[o_:o_ + n_].copy_(cap_b[a_:a_ + n_], non_blocking=True)
            torch.cuda.synchronize()

        def loop_d2h():
            for a_, n_, o_ in zip(src_lo, nbytes, offs):
                pinned[o_:o_ + n_].copy_(cap_b[a_:a_ + n_], non_blocking=True)
            torch.cuda.synchronize()

        cap_w, dst_w = cap_t.view(torch.int32), dst.view(torch.int32)     # (a piece of a real capture is whole 4-byte words)
        lo_h = torch.tensor([v // 4 for v in src_lo], dtype=torch.int64).pin_memory()
        n_h = torch.tensor([v // 4 for v in nbytes], dtype=torch.int64).pin_memory()
        o_h = torch.tensor([v // 4 for v in offs], dtype=torch.int64).pin_memory()

        def torch_gather():
            lo_d, n_d, o_d = (v.cuda(non_blocking=True) for v in (lo_h, n_h, o_h))
            first = torch.cumsum(n_d, 0) - n_d
            k = torch.arange(int(n_h.sum()), device="cuda") - torch.repeat_interleave(first, n_d)
            dst_w[:total // 4].zero_()
            dst_w[torch.repeat_interleave(o_d, n_d) + k] = cap_w[torch.repeat_interleave(lo_d, n_d) + k]
            torch.cuda.synchronize()

        want, _ = BA.gather(cap_t.cpu().numpy(), tab, M, 4)
        for side in (call, loop_d2d, torch_gather):
            dst[:total].fill_(0xA5)
            side()
            assert np.array_equal(dst[:total].cpu().numpy(), want), side
        pinned[:total].fill_(0)
        loop_d2h()
        assert np.array_equal(pinned[:total].numpy(), want)        # (where the pad is zero already)
        lines += [f"# (a) {what}: {b} bursts at factor 48, lead 2, hang 4; {total} bytes of {2 * N} ({100.0 * total / (2 * N):.3f} %); every side checked",
                  f"#     against burst_archive.gather first; {reps} rounds, the sides in a new random order every round, one call per side and round", head]
        names, wall = rotate({"adsb_gather_device": call, "adsb_gather_device again (the A/A)": call,
                              "adsb_gather_device + ONE device-to-host copy": call_and_copy,
                              "loop: one device-to-device copy per piece": loop_d2d, "loop: one device-to-host copy per piece": loop_d2h,
                              "the same gather in torch on the device": torch_gather})
        table_of(names, wall, names[0])
        arch = 64 + 16 * b + total
        lines += [f"# (c) the archive: {arch} bytes (64 + 16 x {b} + {total}) over the capture's {2 * N}: {100.0 * arch / (2 * N):.3f} %", "#"]
        kept[what] = (tab, b, total, thr)

    # (b)
    pw = torch.empty(M, dtype=torch.float32, device="cuda")
    whole = np.zeros(1, dtype=levels.BURST_DTYPE)
    whole[0] = (0, ke, 1, 1.0)
    tab, b, total, _ = kept[captures[0][0]]

    def export():
        assert L.adsb_power_device(d._h, t_bench.data_ptr(), N, pw.data_ptr(), M) == M

    def gather_whole():
        assert L.adsb_gather_device(d._h, t_bench.data_ptr(), 2 * N, 4, M, whole.ctypes.data, 1, dst.data_ptr(), 2 * N, None) == 4 * M

    def gather_bench():
        assert L.adsb_gather_device(d._h, t_bench.data_ptr(), 2 * N, 4, M, tab.ctypes.data, b, dst.data_ptr(), 2 * N, None) == total
    moved = {"adsb_power_device (2 N bytes in, 2 N out)": 4 * N, "adsb_power_device again (the A/A)": 4 * N,
             "adsb_gather_device, one burst = the whole capture": 4 * N, "adsb_gather_device, the benchmark's bursts": 2 * total}
    lines += ["# (b) effective bytes per second (bytes loaded + bytes stored over the call's wall time) beside adsb_power_device on the same capture", head]
    names, wall = rotate(dict(zip(moved, (export, export, gather_whole, gather_bench))))
    table_of(names, wall, names[0], note=lambda name, ms: f"   {moved[name] / ms / 1e9:8.3f} TB/s")
    lines.append("#")
    del pw

    # (d)
    host_cap = torch.empty(N, dtype=torch.int16).pin_memory()
    host_cap.copy_(t_bench.view(torch.int16))
    lines += ["# (d) end to end from page-locked host memory, frames in host memory at the end: ONE adsb_decode_batch_host of the archive's pieces on a",
              "#     flush handle beside the host-fed decode of the whole capture (adsb_reset, adsb_push, adsb_finish)", head]
    for what, cap_t in captures:
        tab, b, total, _ = kept[what]
        assert L.adsb_gather_device(d._h, cap_t.data_ptr(), 2 * N, 4, M, tab.ctypes.data, b, dst.data_ptr(), 2 * N, None) == total
        pinned[:total].copy_(dst[:total])
        host_cap.copy_(cap_t.view(torch.int16))
        torch.cuda.synchronize()
        off = BA.layout(tab, M, 4)
        sl = levels.burst_samples(tab, M)
        pp = (C.c_void_p * b)(*[pinned.data_ptr() + int(o) for o in off[:-1]])
        nn = (C.c_size_t * b)(*[2 * int(hi - lo) for lo, hi in sl])
        ff = (C.c_uint64 * (b + 1))()
        state = {}

        def archive_route():
            k = L.adsb_decode_batch_host(flush._h, b, pp, nn, C.byref(out), ff, None)
            assert k >= 0
            state["k"] = k

        def whole_route():
            assert L.adsb_reset(d._h) == 0 and L.adsb_push(d._h, host_cap.data_ptr(), N) == 0 and L.adsb_finish(d._h) == 0
            state["w"] = L.adsb_pending(d._h)
            L.adsb_take(d._h, C.byref(out))
        archive_route(), whole_route()
        lines.append(f"#   {what}: {state['w']} frames from the whole capture, {state['k']} from the archive's {b} pieces ({total} bytes)")
        names, wall = rotate({"adsb_push of the whole capture + adsb_finish": whole_route, "the same again (the A/A)": whole_route,
                              "adsb_decode_batch_host of the archive's pieces, flush": archive_route})
        table_of(names, wall, names[0])
    lines.append("#")
    del host_cap

    # (e)
    M8 = N                                                   # 256 Mi power samples of int8 IQ: 512 MiB, as the real capture
    cap8 = captures[0][1].view(torch.uint8)
    R8 = M8 // 28
    even = np.zeros(R8 // 128, dtype=levels.BURST_DTYPE)
    even["begin"] = 128 * np.arange(even.size)
    even["end"] = even["begin"] + 64
    odd = even.copy()
    odd["begin"] += 1
    odd["end"] += 1
    tot8 = int(BA.layout(even, M8, 2)[-1])
    assert tot8 == int(BA.layout(odd, M8, 2)[-1])

    builds = [("tree (one 16-byte load at 8-byte alignment)", L, d._h)]
    for spec in variants:
        vname, _, vpath = spec.partition("=")
        V = C.CDLL(vpath)
        for fname in ("adsb_create", "adsb_gather_device"):
            fn = getattr(V, fname)
            fn.restype, fn.argtypes = capi.SYMBOLS[fname]
        vcfg = capi.make_config()
        vh = V.adsb_create(C.byref(vcfg))
        assert vh, vpath
        builds.append((vname, V, vh))

    def g8(tab8, lib, h):
        assert lib.adsb_gather_device(h, cap8.data_ptr(), 2 * N, 2, M8, tab8.ctypes.data, tab8.size, dst.data_ptr(), 2 * N, None) == tot8
    for tab8 in (even, odd):
        for _, lib, h in builds:
            g8(tab8, lib, h)
            head8 = BA.gather(cap8[:1 << 22].cpu().numpy(), tab8[:100], 1 << 21, 2)[0]           # (the first hundred pieces, checked)
            assert np.array_equal(dst[:head8.size].cpu().numpy(), head8)
    lines += [f"# (e) s = 2 (int8 IQ, {M8} power samples): {even.size} pieces of 64 runs, one in every 128 runs, {tot8} bytes; every begin even (each source",
              "#     16-byte aligned) beside every begin odd (each source 8 bytes behind a 16-byte boundary); builds named with --variant differ in",
              "#     gather_kernel.hip alone (-DADSB_GATHER_LOAD=0: an aligned source by one 16-byte load, a source 8 behind by two 8-byte loads)", head]
    sides8 = {"begin even, tree": lambda: g8(even, L, d._h), "begin even, tree again (the A/A)": lambda: g8(even, L, d._h),
              "begin odd, tree": lambda: g8(odd, L, d._h)}
    for vname, lib, h in builds[1:]:
        sides8[f"begin even, {vname}"] = lambda lib=lib, h=h: g8(even, lib, h)
        sides8[f"begin odd, {vname}"] = lambda lib=lib, h=h: g8(odd, lib, h)
    names, wall = rotate(sides8)
    table_of(names, wall, names[0], note=lambda name, ms: f"   {2 * tot8 / ms / 1e9:8.3f} TB/s")
    lines.append("#")

    # (f)
    lines += ["# (f) the untouched paths beside the parent commit's library (--ab), adsb_level_device and adsb_decode_device on the benchmark capture", head]
    if not parent:
        lines.append("#     (no --ab parent library given: not measured in this run)")
        return
    B = C.CDLL(parent)
    for name in ("adsb_create", "adsb_decode_device", "adsb_level_device"):
        fn = getattr(B, name)
        fn.restype, fn.argtypes = capi.SYMBOLS[name]
    assert not hasattr(B, "adsb_gather_device"), "the --ab library is not the parent's: it has the gather"
    cfg = capi.make_config()
    hh = B.adsb_create(C.byref(cfg))
    assert hh, parent

    def level(lib, h):
        assert lib.adsb_level_device(h, t_bench.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M

    def decode(lib, h):
        assert lib.adsb_decode_device(h, t_bench.data_ptr(), N, C.byref(out)) >= 0
    for what, fn, steps in (("adsb_level_device", level, 1), ("adsb_decode_device", decode, 3)):
        names, wall = rotate({f"{what}, tree": lambda: fn(L, d._h), f"{what}, tree again (the A/A)": lambda: fn(L, d._h),
                              f"{what}, parent commit": lambda: fn(B, hh)}, steps=steps)
        table_of(names, wall, names[0])


def gather_pack12_probe(L, reps, lines, parent, variants=()):
    """The 12-bit burst gather (adsb_gather_pack12_*, gather_pack12_kernel.hip), every comparison interleaved in this one process, wall
    time of the calls, the run's A/A beside every ratio.  On the benchmark workload's table and on the sparse capture's (factor 48,
    lead 2, hang 4):
    (a) adsb_gather_pack12_device beside itself (the A/A), beside adsb_gather_device on the same table, beside that gather followed by
        a separate pack in torch, beside _packed and _as (fmt 3) with their unpack / conversion launch, and through every --variant
        name=path: a measurement build of the library whose gather_pack12_kernel.hip differs;
    (b) archive bytes of kind 12 over kind 4's and over the capture's;
    (c) adsb_level_device and adsb_decode_device beside the parent commit's library (--ab)."""
    import numpy as np
    from adsbdec_amd import burst_archive as BA, levels, packed12, sample_formats
    out = C.POINTER(capi.Frame)()
    order_rng = __import__("random").Random(33)

    def rotate(sides, steps=1):
        names = list(sides)
        wall = {k_: [] for k_ in names}
        for r in range(-1, reps):                            # (round -1: the warm-up)
            order = names[:]
            order_rng.shuffle(order)
            for name in order:
                t0 = time.perf_counter()
                for _ in range(steps):
                    sides[name]()
                if r >= 0:
                    wall[name].append((time.perf_counter() - t0) * 1e3 / steps)
        return names, wall

    def table_of(names, wall, base):
        for name in names:
            q = statistics.quantiles(wall[name], n=4)
            rr = [a_ / b for a_, b in zip(wall[name], wall[base])]
            qr = statistics.quantiles(rr, n=4)
            lines.append(f"    {name:62s} {med(wall[name]):10.4f} ({q[0]:.4f} .. {q[2]:.4f})   {med(rr):.4f} ({qr[0]:.4f} .. {qr[2]:.4f})")
            print(lines[-1], flush=True)

    head = "#   side                                                              call ms (q1 .. q3)               / the first side (median of rounds, q1 .. q3)"
    M = N // 2
    ke = -(-M // 28)
    d = capi.Decoder()
    env = torch.zeros(ke, dtype=torch.float32, device="cuda")
    rep1 = capi.LevelReport()
    dst = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    dst16 = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    t_bench = make_workload(torch, N, seed=1)[0]
    captures = (("the benchmark workload: a frame per millisecond", t_bench),
                ("sparse: 805 frames in 256 Mi samples", make_workload(torch, N, n_frames=805, seed=2)[0]))
    builds = []
    for spec in variants:
        vname, _, vpath = spec.partition("=")
        V = C.CDLL(vpath)
        for fname in ("adsb_create", "adsb_gather_pack12_device"):
            fn = getattr(V, fname)
            fn.restype, fn.argtypes = capi.SYMBOLS[fname]
        vcfg = capi.make_config()
        vh = V.adsb_create(C.byref(vcfg))
        assert vh, vpath
        builds.append((vname, V, vh))
    torch.cuda.synchronize()
    for what, cap_t in captures:
        assert L.adsb_level_device(d._h, cap_t.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M
        thr = float(np.float32(capi.Decoder.BURST_FACTOR * L.adsb_level_percentile(C.byref(rep1), 0.5)))
        tab, b = d.bursts_device(env.data_ptr(), ke, thr, 2, 4, 1 << 16)
        assert 0 < b <= 1 << 16
        tab = np.ascontiguousarray(tab)
        host = cap_t.cpu().numpy().view(np.uint16)
        want12, off12, over = BA.gather12(host, tab, M)
        total12, total16 = int(off12[-1]), int(BA.layout(tab, M, 4)[-1])
        assert over == 0
        sl = levels.burst_samples(tab, M)
        # the twins of the capture for _packed and _as: the same codes, so the same table and the same bytes
        t_p12 = torch.from_numpy(packed12.pack12(host)).cuda()
        t_i16 = torch.from_numpy(sample_formats.to_format(3, host)).cuda()
        over_c = C.c_uint64(0)

        def g12(lib=L, h=d._h):
            assert lib.adsb_gather_pack12_device(h, cap_t.data_ptr(), N, tab.ctypes.data, b, dst.data_ptr(), 2 * N, None, C.byref(over_c)) == total12

        def g12_packed():
            assert L.adsb_gather_pack12_device_packed(d._h, t_p12.data_ptr(), N, tab.ctypes.data, b, dst.data_ptr(), 2 * N, None, C.byref(over_c)) == total12

        def g12_as():
            assert L.adsb_gather_pack12_device_as(d._h, 3, t_i16.data_ptr(), N, tab.ctypes.data, b, dst.data_ptr(), 2 * N, None, C.byref(over_c)) == total12

        def g16():
            assert L.adsb_gather_device(d._h, cap_t.data_ptr(), 2 * N, 4, M, tab.ctypes.data, b, dst16.data_ptr(), 2 * N, None) == total16

        # the separate pack in torch: adsb_gather_device's pieces (whole groups here: M % 4 == 0) -> the 12-bit layout, on the device
        assert M % 4 == 0
        groups = [int(hi - lo) // 4 for lo, hi in sl]
        g_h = torch.tensor(groups, dtype=torch.int64).pin_memory()
        s_h = torch.tensor([int(o) // 16 for o in BA.layout(tab, M, 4)[:-1]], dtype=torch.int64).pin_memory()   # a group is 16 bytes there
        o_h = torch.tensor([int(o) // 4 for o in off12[:-1]], dtype=torch.int64).pin_memory()                   # ... and 3 dwords here
        dst_w = dst.view(torch.int32)

        def g16_then_torch_pack():
            g16()
            g_d, s_d, o_d = (v.cuda(non_blocking=True) for v in (g_h, s_h, o_h))
            first = torch.cumsum(g_d, 0) - g_d
            k = torch.arange(int(g_h.sum()), device="cuda") - torch.repeat_interleave(first, g_d)
            c = dst16.view(torch.int16).view(-1, 8)[torch.repeat_interleave(s_d, g_d) + k].to(torch.int64) & 0xFFF
            w0 = (c[:, 0] << 20) | (c[:, 1] << 8) | (c[:, 2] >> 4)
            w1 = ((c[:, 2] & 0xF) << 28) | (c[:, 3] << 16) | (c[:, 4] << 4) | (c[:, 5] >> 8)
            w2 = ((c[:, 5] & 0xFF) << 24) | (c[:, 6] << 12) | c[:, 7]
            at = torch.repeat_interleave(o_d, g_d) + 3 * k
            dst_w[:total12 // 4].zero_()
            for j, w in enumerate((w0, w1, w2)):
                dst_w[at + j] = ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)                 # (the dword's bits as a signed int32)
            torch.cuda.synchronize()

        sides = {"adsb_gather_pack12_device": g12, "adsb_gather_pack12_device again (the A/A)": g12, "adsb_gather_device, the same table": g16,
                 "adsb_gather_device, then a pack in torch": g16_then_torch_pack, "adsb_gather_pack12_device_packed (unpack + gather)": g12_packed,
                 "adsb_gather_pack12_device_as fmt 3 (convert + gather)": g12_as}
        for vname, lib, h in builds:
            sides[f"adsb_gather_pack12_device, {vname}"] = lambda lib=lib, h=h: g12(lib, h)
        for name, side in sides.items():
            if side is g16:
                continue
            dst[:total12].fill_(0xA5)
            side()
            assert np.array_equal(dst[:total12].cpu().numpy(), want12), name
        lines += [f"# (a) {what}: {b} bursts at factor 48, lead 2, hang 4; {total12} bytes at 12 bits, {total16} as uint16, of {2 * N}; every side checked",
                  f"#     against burst_archive.gather12 first; {reps} rounds, the sides in a new random order every round, one call per side and round", head]
        names, wall = rotate(sides)
        table_of(names, wall, names[0])
        a12, a16 = 64 + 16 * b + total12, 64 + 16 * b + total16
        lines += [f"# (b) the archive: kind 12 {a12} bytes (64 + 16 x {b} + {total12}), kind 4 {a16}: {100.0 * a12 / a16:.2f} % of it; over the capture's "
                  f"{2 * N}: {100.0 * a12 / (2 * N):.3f} % against {100.0 * a16 / (2 * N):.3f} %", "#"]
        del t_p12, t_i16

    lines += ["# (c) the untouched paths beside the parent commit's library (--ab), adsb_level_device and adsb_decode_device on the benchmark capture", head]
    if not parent:
        lines.append("#     (no --ab parent library given: not measured in this run)")
        return
    B = C.CDLL(parent)
    for name in ("adsb_create", "adsb_decode_device", "adsb_level_device"):
        fn = getattr(B, name)
        fn.restype, fn.argtypes = capi.SYMBOLS[name]
    assert not hasattr(B, "adsb_gather_pack12_device"), "the --ab library is not the parent's: it has the 12-bit gather"
    cfg = capi.make_config()
    hh = B.adsb_create(C.byref(cfg))
    assert hh, parent

    def level(lib, h):
        assert lib.adsb_level_device(h, t_bench.data_ptr(), N, C.byref(rep1), env.data_ptr(), ke) == M

    def decode(lib, h):
        assert lib.adsb_decode_device(h, t_bench.data_ptr(), N, C.byref(out)) >= 0
    for what, fn, steps in (("adsb_level_device", level, 1), ("adsb_decode_device", decode, 3)):
        names, wall = rotate({f"{what}, tree": lambda: fn(L, d._h), f"{what}, tree again (the A/A)": lambda: fn(L, d._h),
                              f"{what}, parent commit": lambda: fn(B, hh)}, steps=steps)
        table_of(names, wall, names[0])


def next_round(stem):
    """profiles/rNN_<stem>.txt with the next free round number."""
    import re
    seen = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(seen, default=0) + 1}_{stem}.txt")


def real_kernel_ab(builds, rounds, lines):
    """(c) the existing real-sample kernel across the change: tools/ab_interleaved.py in a process of its own (it dlopens every build
    side by side), the first build listed twice for the A/A."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ab_interleaved.py"), "--rounds", str(rounds), "--steps", "10"] + builds
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"ab_interleaved.py failed:\n{r.stdout}\n{r.stderr}")
    lines += ["#", "# (c) the existing real-sample kernel (scan_kernel.hip, adsb_decode_device on the sparse 256 Mi-sample workload) across the change:",
              "#     tools/ab_interleaved.py " + " ".join(cmd[2:6]) + " parent=<--ab> parent2=<--ab> tree=<this tree's library>", "#     parent = the library of the parent commit, parent2 = the same file again (the A/A), tree = this tree"]
    lines += ["    " + ln for ln in r.stdout.splitlines()]
    print(r.stdout, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iq", action="store_true", help="complex captures (the _iq calls) instead: profiles/r14_iq.txt")
    ap.add_argument("--power", action="store_true", help="float32 power samples (the _power calls) instead: profiles/r15_power.txt")
    ap.add_argument("--iq8", action="store_true", help="complex int8 captures (fmt 8 of the _iq calls) instead: profiles/r19_iq8.txt")
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB", help="with --power or --iq8: the parent commit's libadsbdec_amd.so, for the A/B of the real kernel")
    ap.add_argument("--export", action="store_true", help="the power export (the adsb_power_* calls) instead: profiles/r17_power_export.txt")
    ap.add_argument("--layout", action="append", default=[], metavar="NAME=LIB", help="with --export: a build of the library with another store layout, measured beside the tree's")
    ap.add_argument("--export-batch", action="store_true", help="the batch power export (the adsb_power_batch_* calls) against the loop of single calls instead: profiles/r20_export_batch.txt; --ab: the parent commit's library, for (c)")
    ap.add_argument("--level", action="store_true", help="the level report (the adsb_level_* calls) instead: profiles/r23_level.txt")
    ap.add_argument("--level-batch", action="store_true", help="the batch level report (the adsb_level_batch_* calls) against the loop of single calls instead: profiles/r26_level_batch.txt")
    ap.add_argument("--level-windows", action="store_true", help="the window form of the level report (adsb_level_windows) beside adsb_level_device instead: profiles/r27_level_windows.txt; --ab: the parent commit's library, for (c)")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB", help="with --level, --level-batch or --gather: a build of the library with another accumulation, flush, grid or load width, measured beside the tree's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bursts", action="store_true", help="the gate behind the envelope (adsb_bursts_device) beside a torch gate and a host gate instead: profiles/rNN_bursts.txt with the next free NN; --ab: the parent commit's library, for (c)")
    ap.add_argument("--flush", action="store_true", help="flush (adsb_set_flush): the decode call across the change, the batch of short captures, the gated pipeline: profiles/r30_flush.txt; --ab: the parent commit's library")
    ap.add_argument("--burst-stream", action="store_true", help="the gate of a slice of a stream (adsb_bursts_slice_device) as one slice and as 16 beside adsb_bursts_device, and the host program's -S -O beside -L -U -K on a 256 Mi-sample file: profiles/rNN_burst_stream.txt with the next free NN; --ab: the parent commit's library, for (c)")
    ap.add_argument("--gather", action="store_true", help="the burst gather (adsb_gather_device) beside copy loops and a torch gather, its bytes per second, the archive's size, the archive route end to end, odd against even begins (and --variant builds with another load): profiles/r32_gather.txt; --ab: the parent commit's library")
    ap.add_argument("--gather-pack12", action="store_true", help="the 12-bit burst gather (adsb_gather_pack12_*) beside adsb_gather_device, a separate pack in torch, the _packed and _as flavours (and --variant builds with another kernel), the archive's size: profiles/r33_pack12.txt; --ab: the parent commit's library")
    a = ap.parse_args()
    if a.gather_pack12:
        a.out = a.out or os.path.join(ROOT, "profiles", "r33_pack12.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --gather-pack12: a real capture's bursts kept at 12 bits (gather_pack12_kernel.hip, adsb_gather_pack12_*), one",
                 f"# process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved in a new random order every round, a warm-up round first.",
                 "# The captures are tools/gen_signal.py make_workload, 256 Mi samples (512 MiB): seed 1 (the benchmark's) and 805 frames, seed 2 (sparse).",
                 "# Wall time of the calls through ctypes / torch; every side waits for its kernels and copies.", "#"]
        gather_pack12_probe(capi.load(), a.reps, lines, a.ab, a.variant)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.gather:
        a.out = a.out or os.path.join(ROOT, "profiles", "r32_gather.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --gather: a capture cut down to its bursts (gather_kernel.hip, adsb_gather_device) and the burst archive, one",
                 f"# process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved in a new random order every round, a warm-up round first.",
                 "# The captures are tools/gen_signal.py make_workload, 256 Mi samples (512 MiB): seed 1 (the benchmark's) and 805 frames, seed 2 (sparse).",
                 "# Wall time of the calls through ctypes / torch; every side waits for its kernels and copies.", "#"]
        gather_probe(capi.load(), a.reps, lines, a.ab, a.variant)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.flush:
        a.out = a.out or os.path.join(ROOT, "profiles", "r30_flush.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --flush: decoding past the end-of-file horizon (adsb_set_flush), one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved, a warm-up round first.",
                 "# Wall time of the C calls through ctypes; every call ends with its frames in host memory.", "#"]
        flush_probe(capi.load(), a.reps, lines, a.ab)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.burst_stream:
        a.out = a.out or next_round("burst_stream")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --burst-stream: the gate of a slice of a stream (burst_slice_kernel.hip, adsb_bursts_slice_device) and the host",
                 f"# program's record mode, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; every side runs once, checked, before",
                 "# its rounds.  The samples are the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1; the envelope is adsb_level_device's.",
                 "# Wall time of the calls through ctypes; every call waits for its kernels and leaves its table in host memory.", "#"]
        burst_stream_probe(capi.load(), a.reps, lines, a.ab)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.bursts:
        a.out = a.out or next_round("bursts")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --bursts: the gate behind the envelope (burst_kernel.hip, adsb_bursts_device), one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first (every side runs once, checked, before its rounds).",
                 "# The samples are the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1; the envelope is adsb_level_device's.",
                 "# Wall time of the calls through ctypes / torch; every side waits for its kernels and leaves its table in host memory.", "#"]
        bursts_probe(capi.load(), a.reps, lines, a.ab)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.level_windows:
        a.out = a.out or os.path.join(ROOT, "profiles", "r27_level_windows.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --level-windows: the window form of the level report (level_windows_kernel.hip, adsb_level_windows) beside",
                 f"# adsb_level_device, one process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The samples are the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1.  Wall time of the C calls through ctypes; every",
                 "# call waits for its kernel and its copy of the totals (16 KiB a window).", "#"]
        level_windows_probe(capi.load(), a.reps, lines, a.ab)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.level_batch:
        a.out = a.out or os.path.join(ROOT, "profiles", "r26_level_batch.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --level-batch: the batch level report (level_batch_kernel.hip, the adsb_level_batch_* calls) beside the loop of",
                 f"# single calls, one process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The samples are the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1, cut into captures (and converted on the device",
                 "# into each format; the packed leg repeats the first capture's packed bytes).  Wall time of the C calls through ctypes; every call waits for",
                 "# its kernels and its copy of the totals, so a loop pays a memset, a launch, a 16 KiB copy and a wait per capture (two launches for the",
                 "# flavours that unpack or convert).  Sides named with --variant are builds of the library that differ in level_batch_kernel.hip alone, loaded",
                 "# beside the tree's in this process:",
                 "#   -DADSB_LEVEL_BATCH_WALK=1   the passes go to the waves grid-stride, as the single kernel walks, and a wave flushes at every change of",
                 "#                               capture; the tree (WALK=0) gives every wave a contiguous range of passes",
                 "#   -DADSB_LEVEL_BATCH_MERGE=0  every wave flushes alone at its end; the tree (MERGE=1) sums the four histograms of a workgroup whose waves",
                 "#                               end in the same capture and flushes once", "#"]
        ok = level_batch_probe(capi.load(), a.reps, lines, a.variant)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if not ok:
            raise SystemExit("on (a) or (b) the batch call does not beat the loop of single calls by more than the A/A spread")
        return
    if a.level:
        a.out = a.out or os.path.join(ROOT, "profiles", "r23_level.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --level: the level report (level_kernel.hip, the adsb_level_* calls), one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# Contents, 256 Mi samples each: the benchmark's workload (tools/gen_signal.py make_workload, seed 1); Gaussian noise of sigma 600 codes",
                 "# round 2048, clipped to 0 .. 4095; silence (every code 0x800).",
                 "# Sides named with --variant are builds of the library that differ in level_kernel.hip alone, loaded beside the tree's in this process:",
                 "#   -DADSB_LEVEL_HIST=k   bit 0: a histogram per workgroup (0) or per wave (1) in LDS; bit 1: the wave-uniform shortcut (one add when a wave agrees on an increment)",
                 "#                         bit 2: the run-uniform shortcut instead (one add when a lane's 28 samples agree)",
                 "#   -DADSB_LEVEL_FLUSH=1  a row of 32-bit counts per workgroup and a second small kernel that sums the rows, instead of 64-bit atomics on the totals",
                 "#   -DADSB_LEVEL_BLOCKS=n the grid's cap (workgroups of 4 waves)",
                 "#   the tree is HIST=5 (per wave, run-uniform shortcut), FLUSH=0, BLOCKS=2048; a variant changes the one thing its name says",
                 "#   (names as built for this record: hK = -DADSB_LEVEL_HIST=K, rows = -DADSB_LEVEL_FLUSH=1, bN = -DADSB_LEVEL_BLOCKS=N)", "#"]
        level_probe(capi.load(), a.reps, lines, a.variant)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.export_batch:
        a.out = a.out or os.path.join(ROOT, "profiles", "r20_export_batch.txt")
        torch.cuda.set_device(0)
        lines = ["# tools/format_probe.py --export-batch: the batch power export (power_export_batch_kernel.hip, the adsb_power_batch_* calls) beside",
                 f"# the loop of single calls, one process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The samples are the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1, cut into captures (and converted on the device",
                 "# into each format; the packed leg repeats the first capture's packed bytes).  Wall time of the C calls through ctypes; every call waits for",
                 "# its kernels, so a loop pays one launch-and-wait round trip per capture (two launches for the flavours that unpack or convert).", "#"]
        export_batch_probe(capi.load(), a.reps, lines, a.ab)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "r17_power_export.txt" if a.export else "r19_iq8.txt" if a.iq8 else "r15_power.txt" if a.power else "r14_iq.txt" if a.iq else "r11_formats.txt")
    torch.cuda.set_device(0)
    L = capi.load()
    if a.export:
        lines = ["# tools/format_probe.py --export: the power export (power_export_kernel.hip, the adsb_power_* calls), one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The capture is the benchmark's: tools/gen_signal.py make_workload, 256 Mi samples, seed 1.",
                 "# Sides named with --layout are builds of the library that differ in power_export_kernel.hip alone (-DADSB_EXPORT_STORE=k; a lane's",
                 "# 28 floats are 112 contiguous bytes of the output), loaded beside the tree's in this process; every build writes the same floats:",
                 "#   tree     k = 2: a wave's 1792 samples turned through 7 KiB of LDS of its own; each of seven stores writes 1 KiB of contiguous lines",
                 "#   plain    k = 0: seven 16-byte stores per lane, 112 bytes apart by lane, as Stage A's loads are",
                 "#   nt       k = 1: plain's stores, non-temporal",
                 "#   lds-nt   k = 3: the tree's stores, non-temporal", "#"]
        export_probe(L, a.reps, lines, a.layout)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.iq8:
        lines = ["# tools/format_probe.py --iq8: complex int8 captures (scan_iq8_kernel.hip, fmt 8 of the _iq calls) beside the int16 IQ kernel, one",
                 f"# process, {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The capture is one 4 Mi-sample block of tools/gen_signal.py make_iq_workload (seed 1) quantised with >> 8 and repeated 32 times.", "#"]
        gate_ok = iq8_probe(L, a.reps, lines)
        if a.ab:
            real_kernel_ab([f"parent={a.ab}", f"parent2={a.ab}", f"tree={capi.LIB_PATH}"], 2 * a.reps, lines)
            lines[lines.index("# (c) the existing real-sample kernel (scan_kernel.hip, adsb_decode_device on the sparse 256 Mi-sample workload) across the change:")] = \
                "# (d) the existing real-sample kernel (scan_kernel.hip, adsb_decode_device on the sparse 256 Mi-sample workload) across the change:"
        else:
            lines += ["#", "# (d) not measured in this run: no --ab parent library given"]
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        if not gate_ok:
            raise SystemExit("(b): the fmt 8 call is not faster than torch widening + fmt 2 by more than the A/A spread")
        return
    if a.power:
        lines = ["# tools/format_probe.py --power: float32 power samples (scan_power_kernel.hip, the _power calls) beside the IQ kernel, one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The IQ capture is one 4 Mi-sample block of tools/gen_signal.py make_iq_workload (seed 1) repeated 32 times.", "#"]
        power_probe(L, a.reps, lines)
        if a.ab:
            real_kernel_ab([f"parent={a.ab}", f"parent2={a.ab}", f"tree={capi.LIB_PATH}"], 2 * a.reps, lines)
        else:
            lines += ["#", "# (c) not measured in this run: no --ab parent library given"]
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.iq:
        lines = ["# tools/format_probe.py --iq: complex captures (scan_iq_kernel.hip, the _iq calls) beside the real-sample kernel, one process,",
                 f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; warm-up first.",
                 "# The IQ capture is one 4 Mi-sample block of tools/gen_signal.py make_iq_workload (seed 1) repeated 32 times.", "#"]
        iq_probe(L, a.reps, lines)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    t, _ = make_workload(torch, N, seed=1)
    assert int(t.max()) <= 4095 and int(t.min()) >= 0
    conv = {S16: ((t.to(torch.int32) - 2048) * 16).to(torch.int16), F32: (t.to(torch.float32) - 2048.0) / 2048.0}
    torch.cuda.synchronize()
    lines = ["# tools/format_probe.py: signed 16-bit real and float32 real input converted on the GPU (csrc/convert_samples.hip), one process,",
             f"# {torch.cuda.get_device_name(0)}; the sides of every comparison interleaved; {a.reps} repetitions after warm-up.", "#"]
    kernels(L, t, conv, a.reps, lines)
    whole_calls(L, t, conv, a.reps, lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
