#!/usr/bin/env python3
"""The conversion of signed 16-bit real and float32 real input (adsb_*_as) on one GPU, ONE process, the sides of every
comparison interleaved.

    python tools/format_probe.py [--reps 20] [--out profiles/r11_formats.txt]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_formats.txt"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = capi.load()
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
