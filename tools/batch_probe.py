#!/usr/bin/env python3
"""One adsb_decode_batch_device call against a loop of adsb_decode_device over the same captures, ONE process.

    python tools/batch_probe.py [--reps 7] [--out profiles/r9_batch.txt]
    python tools/batch_probe.py --packed [--reps 7] [--out profiles/r10_batch_packed.txt]

For B in {1, 16, 256, 2048} captures of n in {64 Ki, 1 Mi, 16 Mi} samples each (sparse traffic, ~1 k frames/s: BASELINE
configs[1]'s generator), and for one capture of 256 Mi samples: the wall time of the batch call, of the loop (B calls), their
ratio, the launches the batch took and the frames (equal on both sides in every cell, or the probe stops).  The captures are
B slices of one buffer of at most 1 Gi samples; beyond that the slices repeat (the same pointers again).  Medians over --reps
repetitions, batch and loop alternating, after a warm-up of each.  The same handle configuration on both sides
(df18 off, no statistics); a handle per side.

--packed: the same captures as Airspy packed 12-bit bytes.  One adsb_decode_batch_device_packed call against the loop of
adsb_decode_device_packed (what a packed archive had before: an unpack launch, a scan launch and a host round trip per capture)
and against adsb_decode_batch_device on the unpacked twins (the price of the extra pass: 1.5 B read + 2 B written per sample).
Cells whose unpacked scratch (2 B x B x n) would pass 8 GiB are left out.
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

CAP = 1 << 30


def cell(L, d_batch, d_loop, t, B, n, reps):
    slices = max(1, min(B, t.numel() // n))
    ptrs = [t.data_ptr() + 2 * n * (i % slices) for i in range(B)]
    p = (C.c_void_p * B)(*ptrs)
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    out = C.POINTER(capi.Frame)()

    def batch():
        t0 = time.perf_counter()
        k = L.adsb_decode_batch_device(d_batch._h, B, p, nn, C.byref(out), first, None)
        dt = time.perf_counter() - t0
        assert k >= 0, L.adsb_last_error(d_batch._h)
        return dt, [int(first[i + 1] - first[i]) for i in range(B)]

    def loop():
        per = []
        t0 = time.perf_counter()
        for i in range(B):
            per.append(d_loop._decode_device(d_loop._h, ptrs[i], n, d_loop._out_ref))
        return time.perf_counter() - t0, per

    l0 = d_batch.profile()["launches"]
    (_, fb), (_, fl) = batch(), loop()
    launches = d_batch.profile()["launches"] - l0
    assert fb == fl, f"B = {B}, n = {n}: frames per capture differ"
    tb, tl = [], []
    for _ in range(reps):
        tb.append(batch()[0])
        tl.append(loop()[0])
    return statistics.median(tb), statistics.median(tl), launches, sum(fb)


PACKED_CAP = 1 << 28


def packed_cell(L, d_batch, d_loop, d_twin, pk, t, B, n, reps):
    per = n // 8 * 12
    slices = max(1, min(B, t.numel() // n))
    ptrs = [pk.data_ptr() + per * (i % slices) for i in range(B)]
    uptrs = [t.data_ptr() + 2 * n * (i % slices) for i in range(B)]
    p, up = (C.c_void_p * B)(*ptrs), (C.c_void_p * B)(*uptrs)
    nn = (C.c_size_t * B)(*([n] * B))
    first = (C.c_uint64 * (B + 1))()
    out = C.POINTER(capi.Frame)()

    def batch(fn, d, pp):
        t0 = time.perf_counter()
        k = fn(d._h, B, pp, nn, C.byref(out), first, None)
        dt = time.perf_counter() - t0
        assert k >= 0, L.adsb_last_error(d._h)
        return dt, [int(first[i + 1] - first[i]) for i in range(B)]

    def loop():
        per_capture = []
        t0 = time.perf_counter()
        for i in range(B):
            per_capture.append(L.adsb_decode_device_packed(d_loop._h, ptrs[i], n, d_loop._out_ref))
        return time.perf_counter() - t0, per_capture

    sides = ((L.adsb_decode_batch_device_packed, d_batch, p), (L.adsb_decode_batch_device, d_twin, up))
    (_, fb), (_, fu), (_, fl) = batch(*sides[0]), batch(*sides[1]), loop()
    assert fb == fl == fu, f"B = {B}, n = {n}: frames per capture differ"
    tb, tl, tu = [], [], []
    for _ in range(reps):
        tb.append(batch(*sides[0])[0])
        tl.append(loop()[0])
        tu.append(batch(*sides[1])[0])
    return statistics.median(tb), statistics.median(tl), statistics.median(tu), sum(fb)


def main_packed(a):
    import numpy as np
    from adsbdec_amd.packed12 import pack12
    torch.cuda.set_device(0)
    L = capi.load()
    d_batch, d_loop, d_twin = capi.Decoder(df18=False), capi.Decoder(df18=False), capi.Decoder(df18=False)
    t, _ = make_workload(torch, PACKED_CAP, seed=1)
    x = t.cpu().numpy().view(np.uint16)
    assert int(x.max()) <= 4095
    step = 1 << 24
    pk = torch.cat([torch.from_numpy(pack12(x[i:i + step])).cuda() for i in range(0, x.size, step)])
    lines = ["# tools/batch_probe.py --packed: adsb_decode_batch_device_packed (one call) against a loop of adsb_decode_device_packed (B calls)",
             "# and against adsb_decode_batch_device on the unpacked twins (one call), one process,",
             f"# {torch.cuda.get_device_name(0)}; sparse traffic; medians of {a.reps} repetitions, wall time of the calls in ms.",
             "# Slices of one 256 Mi-sample buffer (B x n beyond that: the same pointers again; the scratch is 2 B x B x n all the same).",
             "# Frames per capture equal on all three sides in every cell.  64 Ki samples are below the reference's first deqframe call",
             "# (81 960 samples, air.c:94): no frames and no scan launch -- that row is the unpack and the calls alone.",
             "#",
             "#     B   n (samples)   packed batch ms   packed loop ms   loop/batch   unpacked batch ms   packed/unpacked   frames"]
    for n in (1 << 16, 1 << 20, 1 << 24):
        for B in (1, 16, 256, 2048):
            if 2 * B * n > 8 << 30:
                continue
            tb, tl, tu, frames = packed_cell(L, d_batch, d_loop, d_twin, pk, t, B, n, a.reps)
            lines.append(f"  {B:5d}  {n:11d}  {tb * 1e3:16.3f}  {tl * 1e3:15.3f}  {tl / tb:11.2f}  {tu * 1e3:18.3f}  {tb / tu:16.2f}  {frames:7d}")
            print(lines[-1], flush=True)
    for d in (d_batch, d_loop, d_twin):
        d.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--packed", action="store_true", help="packed 12-bit captures: the batch call against the loop of packed single calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r10_batch_packed.txt" if a.packed else "r9_batch.txt")
    if a.packed:
        return main_packed(a)
    torch.cuda.set_device(0)
    L = capi.load()
    d_batch, d_loop = capi.Decoder(df18=False), capi.Decoder(df18=False)
    t, _ = make_workload(torch, CAP, seed=1)
    lines = ["# tools/batch_probe.py: adsb_decode_batch_device (one call) against a loop of adsb_decode_device (B calls), one process,",
             f"# {torch.cuda.get_device_name(0)}; sparse traffic; medians of {a.reps} repetitions, wall time of the calls in ms.",
             "# Slices of one 1 Gi-sample buffer (B x n beyond that: the same pointers again).  Frames per capture equal in every cell.",
             "# 64 Ki samples are below the reference's first deqframe call (81 960 samples, air.c:94): no frames, and no launch on",
             "# either side -- that row is the cost of the calls alone.",
             "#",
             "#     B   n (samples)   batch ms    loop ms   loop/batch   launches   frames   batch Gsamples/s"]
    for n in (1 << 16, 1 << 20, 1 << 24):
        for B in (1, 16, 256, 2048):
            tb, tl, launches, frames = cell(L, d_batch, d_loop, t, B, n, a.reps)
            lines.append(f"  {B:5d}  {n:11d}  {tb * 1e3:9.3f}  {tl * 1e3:9.3f}  {tl / tb:10.2f}  {launches:9d}  {frames:7d}  {B * n / tb * 1e-9:10.1f}")
            print(lines[-1], flush=True)
    tb, tl, launches, frames = cell(L, d_batch, d_loop, t, 1, 1 << 28, a.reps)
    lines += ["#", "# One large capture (no gate: the batch path collects AFTER its kernel, the single call while it runs --",
              "# for one large capture adsb_decode_device stays the call to use):",
              f"  {1:5d}  {1 << 28:11d}  {tb * 1e3:9.3f}  {tl * 1e3:9.3f}  {tl / tb:10.2f}  {launches:9d}  {frames:7d}  {(1 << 28) / tb * 1e-9:10.1f}"]
    print(lines[-1], flush=True)
    d_batch.close()
    d_loop.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
