#!/usr/bin/env python3
"""Airspy packed 12-bit input against uint16 input, ONE process, the two formats alternating on the same capture.

    python tools/packed_ingest.py [--rounds 5] [--out FILE] [--skip-cli] [--kernels-only]

  host    host-fed Gsamples/s from page-locked memory (adsb_push_async / adsb_push_packed_async in 32 Mi-sample pieces, then
          adsb_finish), 1 handle and 2 handles fed side by side from two threads;
  cli     the C host program's decode phase (ADSB_CLI_TIMING) on a 510 MiB uint16 file and its 383 MiB packed twin;
  device  adsb_decode_device against adsb_decode_device_packed per 256 Mi-sample capture (BASELINE configs[1]): wall time of
          the call, and the unpack's share;
  unpack  adsb_unpack_packed12 alone over 256 Mi samples: bytes moved (1.5 B read + 2 B written per sample) over the time.
--kernels-only: only a few device decodes and unpacks (the workload of a `rocprofv3 --kernel-trace --stats` run).
Every line says what was measured; medians over the rounds.
"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

from adsbdec_amd import capi  # noqa: E402
from tools.gen_signal import make_workload  # noqa: E402

PIECE = 32 << 20
N = 256 << 20


def pack_on_device(t):
    s = t.view(-1, 8).to(torch.int64) & 0xFFF
    w = [(s[:, 0] << 20) | (s[:, 1] << 8) | (s[:, 2] >> 4),
         ((s[:, 2] & 0xF) << 28) | (s[:, 3] << 16) | (s[:, 4] << 4) | (s[:, 5] >> 8),
         ((s[:, 5] & 0xFF) << 24) | (s[:, 6] << 12) | s[:, 7]]
    del s
    out = torch.empty((t.numel() // 8, 12), dtype=torch.uint8, device=t.device)
    for q in range(3):
        for j in range(4):
            out[:, 4 * q + j] = ((w[q] >> (8 * j)) & 0xFF).to(torch.uint8)
    return out.view(-1)


def pinned_copy(L, t):
    nbytes = t.numel() * t.element_size()
    p = L.adsb_host_alloc(nbytes)
    assert p, "adsb_host_alloc failed"
    host = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p))
    host[:] = t.view(torch.uint8).cpu().numpy()
    return p, host


def host_decode(d, ptr, n, packed):
    """One whole-capture decode fed from page-locked memory in PIECE-sample pieces -> (seconds, frames)."""
    L = d._L
    d.reset()
    t0 = time.perf_counter()
    for a in range(0, n, PIECE):
        k = min(PIECE, n - a)
        if packed:
            rc = L.adsb_push_packed_async(d._h, ptr + a // 8 * 12, k)
        else:
            rc = L.adsb_push_async(d._h, ptr + 2 * a, k)
        d._check(rc, "push")
    d._check(L.adsb_finish(d._h), "adsb_finish")
    dt = time.perf_counter() - t0
    _, nf = d.take_raw()
    return dt, nf


def run_host(L, out, rounds, u16_ptr, p12_ptr):
    for handles in (1, 2):
        decs = [capi.Decoder(device=0) for _ in range(handles)]
        res = {False: [], True: []}
        frames = {}
        for r in range(rounds + 1):
            for packed in (False, True):
                ts = [None] * handles

                def work(i):
                    ts[i] = host_decode(decs[i], p12_ptr if packed else u16_ptr, N, packed)
                th = [threading.Thread(target=work, args=(i,)) for i in range(handles)]
                t0 = time.perf_counter()
                for x in th:
                    x.start()
                for x in th:
                    x.join()
                wall = time.perf_counter() - t0
                frames.setdefault(packed, set()).update(t[1] for t in ts)
                if r:   # round 0 warms up (first-use costs of the landing buffers, page-locked mappings)
                    res[packed].append(handles * N / wall / 1e9)
        for d in decs:
            d.close()
        a, b = statistics.median(res[False]), statistics.median(res[True])
        out(f"host  {handles} handle(s), pinned memory, {PIECE >> 20} Mi-sample pieces: uint16 {a:.2f} Gsamples/s "
            f"(min {min(res[False]):.2f}, max {max(res[False]):.2f}); packed {b:.2f} Gsamples/s (min {min(res[True]):.2f}, "
            f"max {max(res[True]):.2f}); packed / uint16 = {b / a:.3f}; frames per decode {sorted(frames[False])} / {sorted(frames[True])}")


def run_cli(out, rounds, u16_host, p12_host):
    tmpdir = "/dev/shm" if os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    n = 255 << 20                       # 510 MiB as uint16
    with tempfile.TemporaryDirectory(dir=tmpdir) as td:
        fu, fp = os.path.join(td, "c.u16"), os.path.join(td, "c.p12")
        u16_host[: 2 * n].tofile(fu)
        p12_host[: n // 8 * 12].tofile(fp)
        res = {False: [], True: []}
        outs = {}
        lines = {False: [], True: []}
        for r in range(rounds + 1):
            for packed in (False, True):
                cmd = [capi.CLI_PATH] + (["-p"] if packed else []) + ["-f", fp if packed else fu]
                p = subprocess.run(cmd, capture_output=True, timeout=300, env={**os.environ, "ADSB_CLI_TIMING": "1"})
                if p.returncode != 0:
                    raise RuntimeError(p.stderr.decode()[-2000:])
                line = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("timing:")][0]
                dec_ms = float(line.split("decode ")[1].split(" ms")[0])
                outs.setdefault(packed, set()).add(hash(p.stdout))
                if r:
                    res[packed].append(dec_ms)
                    lines[packed].append((dec_ms, line))
        a, b = statistics.median(res[False]), statistics.median(res[True])
        for packed in (False, True):   # where the time of the median run went (the program's own ADSB_CLI_TIMING line)
            line = sorted(lines[packed])[len(lines[packed]) // 2][1]
            out(f"cli   {'packed' if packed else 'uint16'} median run: {line}")
        out(f"cli   decode phase, {n >> 20} Mi samples from /dev/shm: uint16 (510 MiB) {a:.1f} ms = {n / a / 1e6:.2f} Gsamples/s; "
            f"packed (383 MiB) {b:.1f} ms = {n / b / 1e6:.2f} Gsamples/s; uint16 / packed time = {a / b:.3f}; "
            f"stdout identical: {outs[False] == outs[True] and len(outs[False]) == 1}")


def run_device(out, rounds, t, p, kernels_only=False):
    d = capi.Decoder(device=0)
    res = {False: [], True: []}
    counts = {}
    for r in range(rounds + 1):
        for packed in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, k = d.decode_device_packed_raw(p.data_ptr(), N) if packed else d.decode_device_raw(t.data_ptr(), N)
            dt = time.perf_counter() - t0
            counts.setdefault(packed, set()).add(k)
            if r:
                res[packed].append(dt * 1e3)
    d.close()
    if kernels_only:
        return
    a, b = statistics.median(res[False]), statistics.median(res[True])
    out(f"device  {N >> 20} Mi samples resident in HBM, wall time of one call: decode_device {a:.3f} ms, decode_device_packed "
        f"{b:.3f} ms (+{b - a:.3f} ms, x{b / a:.3f}); frames {sorted(counts[False])} / {sorted(counts[True])}")


def run_unpack(L, out, rounds, p):
    dst = torch.empty(N, dtype=torch.int16, device="cuda")
    ms = []
    for r in range(rounds + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        assert L.adsb_unpack_packed12(dst.data_ptr(), p.data_ptr(), N, None) == 0
        e.record()
        torch.cuda.synchronize()
        if r:
            ms.append(s.elapsed_time(e))
    m = statistics.median(ms)
    out(f"unpack  adsb_unpack_packed12 over {N >> 20} Mi samples (events around the launch): {m:.3f} ms, "
        f"{3.5 * N / m / 1e9:.2f} TB/s of 1.5 B read + 2 B written per sample = {3.5 * N / m / 1e9 / 6.3:.2f} of 6.3 TB/s")
    return dst


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    path = args[args.index("--out") + 1] if "--out" in args else None
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    L = capi.load()
    t, _ = make_workload(torch, N, seed=1)
    p = pack_on_device(t)
    torch.cuda.synchronize()
    if "--kernels-only" in args:
        run_device(out, 2, t, p, kernels_only=True)
        run_unpack(L, out, 2, p)
        return
    out(f"# tools/packed_ingest.py on {torch.cuda.get_device_name(0)}: BASELINE configs[1] capture (make_workload seed 1), "
        f"{rounds} rounds after one warm-up, uint16 and packed alternating")
    dst = run_unpack(L, out, rounds, p)
    assert torch.equal(dst, t), "unpacked capture differs from the uint16 one"
    del dst
    run_device(out, rounds, t, p)
    u16_ptr, u16_host = pinned_copy(L, t)
    p12_ptr, p12_host = pinned_copy(L, p)
    run_host(L, out, rounds, u16_ptr, p12_ptr)
    if "--skip-cli" not in args:
        run_cli(out, rounds, u16_host, p12_host)
    L.adsb_host_free(u16_ptr)
    L.adsb_host_free(p12_ptr)
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
