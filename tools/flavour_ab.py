#!/usr/bin/env python3
"""Host time of four capture calls over several builds of the library IN ONE PROCESS, calls interleaved (the scheme of
tools/ab_interleaved.py): at 1024 captures of 4096 samples the batch calls are bound by what the host does per capture.

    python tools/flavour_ab.py [--rounds 60] [--reps 5] parent=PATH parent2=COPY_OF_PATH tree=PATH

The first build is the base; a second copy of it under another file name is the run's own A/A.  Per call and build: the median of
the per-round wall time of one call (the call returns when its answer is there), the per-round ratio to the base with its quartiles
and range.  A build lies inside the A/A spread where the median of its ratios lies between the 5th and the 95th percentile of the
A/A ratios."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from adsbdec_amd import capi  # noqa: E402
from adsbdec_amd.packed12 import pack12  # noqa: E402

K, N = 1024, 4096
CALLS = ["adsb_level_batch_device", "adsb_power_batch_device_as", "adsb_decode_batch_device_packed", "adsb_power_device_as"]


def bind(path):
    L = C.CDLL(path)
    for name in CALLS + ["adsb_config_init", "adsb_create", "adsb_destroy", "adsb_last_error"]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = capi.SYMBOLS[name]
    return L


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 60
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    builds = [a.split("=", 1) for a in args if "=" in a and not a.startswith("--")]
    torch.cuda.set_device(0)
    x = np.clip(np.random.RandomState(35).normal(2048, 40, K * N), 0, 4095).astype("<u2")
    dev = {"u16": torch.from_numpy(x.view(np.int16)).cuda(), "i16": torch.from_numpy(((x.astype(np.int32) - 2048) << 4).astype("<i2")).cuda(),
           "packed": torch.from_numpy(pack12(x)).cuda()}
    power = torch.empty(K * N // 2, dtype=torch.float32, device="cuda")
    reports = (capi.LevelReport * K)()
    ns = (C.c_size_t * K)(*[N] * K)
    caps = (C.c_size_t * K)(*[N // 2] * K)
    stride = {"u16": 2 * N, "i16": 2 * N, "packed": 3 * N // 2}   # bytes of a capture
    ptrs = {k: (C.c_void_p * K)(*[t.data_ptr() + i * stride[k] for i in range(K)]) for k, t in dev.items()}
    outs = (C.c_void_p * K)(*[power.data_ptr() + 2 * N * i for i in range(K)])
    frames, first, stats = C.POINTER(capi.Frame)(), (C.c_uint64 * (K + 1))(), (capi.Stats * K)()
    void = lambda a: C.cast(a, C.c_void_p)
    libs, handles = {}, {}
    for name, path in builds:
        libs[name] = bind(path)
        cfg = capi.Config()
        libs[name].adsb_config_init(C.byref(cfg), C.sizeof(cfg))
        cfg.device = 0
        handles[name] = libs[name].adsb_create(C.byref(cfg))
        assert handles[name], name

    def call(name, which):
        L, h = libs[name], handles[name]
        if which == CALLS[0]:
            r = L.adsb_level_batch_device(h, K, void(ptrs["u16"]), void(ns), void(reports), None, None)
        elif which == CALLS[1]:
            r = L.adsb_power_batch_device_as(h, 3, K, void(ptrs["i16"]), void(ns), void(outs), void(caps))
        elif which == CALLS[2]:
            r = L.adsb_decode_batch_device_packed(h, K, ptrs["packed"], ns, C.byref(frames), first, stats)
        else:
            r = L.adsb_power_device_as(h, 3, dev["i16"].data_ptr(), N, power.data_ptr(), N // 2)
        assert r >= 0, (name, which, L.adsb_last_error(h))

    print(f"# {K} captures of {N} samples; {rounds} rounds of {reps} calls per build, interleaved; builds: {', '.join(n for n, _ in builds)}")
    for which in CALLS:
        per = {name: [] for name, _ in builds}
        for name, _ in builds:   # warm: scratch, tables, the first launch of every kernel
            call(name, which), call(name, which)
        for _ in range(rounds):
            for name, _ in builds:
                t0 = time.perf_counter()
                for _ in range(reps):
                    call(name, which)
                per[name].append((time.perf_counter() - t0) / reps * 1e3)
        base = builds[0][0]
        print(f"{which}")
        spread = None
        for name, _ in builds:
            ratios = sorted(a / b for a, b in zip(per[name], per[base]))
            q = statistics.quantiles(ratios, n=20)
            line = f"  {name:8s} median {statistics.median(per[name]):8.4f} ms   ratio to {base}: median {statistics.median(ratios):.4f}  " \
                   f"quartiles {q[4]:.4f} .. {q[14]:.4f}  5 % .. 95 % {q[0]:.4f} .. {q[18]:.4f}  range {ratios[0]:.4f} .. {ratios[-1]:.4f}"
            if name != base and spread is None:
                spread = (q[0], q[18])   # the A/A build comes second
                line += "   <- the A/A spread"
            elif name != base:
                line += "   inside the A/A spread" if spread[0] <= statistics.median(ratios) <= spread[1] else "   OUTSIDE the A/A spread"
            print(line)
    for name, _ in builds:
        libs[name].adsb_destroy(handles[name])


if __name__ == "__main__":
    main()
