#!/usr/bin/env python3
"""A/B of the staging steps (csrc/decoder_stage.hip, push_copy) over several builds of the library IN ONE PROCESS, calls interleaved.

    python tools/stage_probe.py [--rounds 15] [--out FILE] parent=path/to/libadsbdec_amd.so parent_again=copy/of/it.so tree=adsbdec_amd/lib/libadsbdec_amd.so

tools/ab_interleaved.py times adsb_decode_device, which stages nothing.  Here every build gets a handle of its own and the rounds go
A B C A B C .. over one call per staging step and buffer policy, on the same inputs: wall time of the call through adsbdec_amd.capi
(the Python around it is the same for every build), the median per build and the per-round ratio to the FIRST build (median and
quartiles).  Name the same library twice (a copy of the file: dlopen gives one handle per path) for the A/A spread of the run.
  to_scratch        power_device_packed, level_device_as fmt 3, decode_device_packed, decode_device_as fmt 1 (the device pushes)
  land_captures     decode_batch, decode_batch_packed, decode_batch_as fmt 3 (copy streams in turn, waited for);
                    power_batch, level_batch (one copy stream, floats back from pow_buf)
  batch_to_scratch  decode_batch_device_packed, power_batch_device_as fmt 3, level_batch_device_packed
  window_in / floats_out   power_window_host, level (adsb_level_host)
  push_copy         the host-fed stream in 1 Mi pieces: decode (uint16, synchronous and asynchronous), decode_packed, decode_as fmt 3
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from adsbdec_amd import capi, sample_formats as S  # noqa: E402
from adsbdec_amd.packed12 import pack12  # noqa: E402
from tools import gen_signal as G  # noqa: E402


def decoder_of(path, **kw):
    """A capi.Decoder whose calls go to the library at `path`."""
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in capi.SYMBOLS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    tree = capi.load()
    capi._lib = L
    try:
        return capi.Decoder(**kw)
    finally:
        capi._lib = tree


def legs(n_one, n_cap, k_caps, n_push):
    """-> [(name, f(decoder))]: the inputs are made once and shared by every build."""
    x, _ = G.dense_capture(n_one, seed=2810, sigma=40.0, n_frames=n_one // 8192, amp=(200, 1800))
    x = np.minimum(x, 4095).astype(np.uint16)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    t_p, t_s, t_f = dev(pack12(x)), dev(S.to_int16_real(x)), dev(S.to_float32_real(x))
    out = torch.empty(n_one // 2, dtype=torch.float32, device="cuda")
    caps = [np.ascontiguousarray(x[i * 4096:i * 4096 + n_cap - 8 * (i % 5)]) for i in range(k_caps)]
    caps_p, caps_s = [pack12(c) for c in caps], [S.to_int16_real(c) for c in caps]
    ns = [c.size for c in caps]
    tb_p, tb_s = [dev(c) for c in caps_p], [dev(c) for c in caps_s]
    outs = [torch.empty(2 * (n // 4), dtype=torch.float32, device="cuda") for n in ns]
    po, pc = [o.data_ptr() for o in outs], [o.numel() for o in outs]
    big = np.ascontiguousarray(np.tile(x, -(-n_push // n_one))[:n_push])
    big_p, big_s = pack12(big), S.to_int16_real(big)
    piece = 1 << 20
    torch.cuda.synchronize()
    return [
        ("to_scratch        power_device_packed", lambda d: d.power_device_packed(t_p.data_ptr(), n_one, out.data_ptr(), out.numel())),
        ("to_scratch        level_device_as 3", lambda d: d.level_device_as(3, t_s.data_ptr(), n_one)),
        ("to_scratch        decode_device_packed", lambda d: d.decode_device_packed_raw(t_p.data_ptr(), n_one)),
        ("to_scratch        decode_device_as 1", lambda d: d.decode_device_as_raw(1, t_f.data_ptr(), n_one)),
        ("land_captures     decode_batch", lambda d: d.decode_batch(caps)),
        ("land_captures     decode_batch_packed", lambda d: d.decode_batch_packed(caps_p)),
        ("land_captures     decode_batch_as 3", lambda d: d.decode_batch_as(3, caps_s)),
        ("land_captures     power_batch", lambda d: d.power_batch(caps)),
        ("land_captures     level_batch", lambda d: d.level_batch(caps)),
        ("batch_to_scratch  decode_batch_device_packed", lambda d: d.decode_batch_device_packed_raw([t.data_ptr() for t in tb_p], ns)),
        ("batch_to_scratch  power_batch_device_as 3", lambda d: d.power_batch_device_as(3, [t.data_ptr() for t in tb_s], ns, po, pc)),
        ("batch_to_scratch  level_batch_device_packed", lambda d: d.level_batch_device_packed([t.data_ptr() for t in tb_p], ns)),
        ("window_in / out   power_window_host", lambda d: d.power_window_host(x, 0, 0, 2 * (n_one // 4))),
        ("window_in / out   level (host)", lambda d: d.level(x)),
        ("push_copy         decode sync", lambda d: d.decode(big, chunk=piece, mode="sync")),
        ("push_copy         decode async", lambda d: d.decode(big, chunk=piece, mode="async")),
        ("push_copy         decode_packed sync", lambda d: d.decode_packed(big_p, chunk=piece, mode="sync")),
        ("push_copy         decode_as 3 sync", lambda d: d.decode_as(3, big_s, chunk=piece, mode="sync")),
    ]


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 15
    out = args[args.index("--out") + 1] if "--out" in args else None
    builds = [a.split("=", 1) for a in args if "=" in a and not a.startswith("--")]
    assert len(builds) >= 2, __doc__
    torch.cuda.set_device(0)
    decs = [(name, decoder_of(path, df18=True)) for name, path in builds]
    lines = [f"# tools/stage_probe.py: {rounds} rounds, builds interleaved in one process; wall ms per call, median; ratio to `{builds[0][0]}`: median of the",
             "# per-round ratios (quartiles).  8 Mi samples per single call, 32 captures of about 256 Ki per batch, 16 Mi samples per host-fed stream."]
    for name, f in legs(8 << 20, 1 << 18, 32, 16 << 20):
        for _, d in decs:                                    # warm-up: buffers grown, code paged in
            f(d)
        ms = {b: [] for b, _ in decs}
        for _ in range(rounds):
            for b, d in decs:
                t0 = time.perf_counter()
                f(d)
                ms[b].append(1e3 * (time.perf_counter() - t0))
        row = f"{name:<46}"
        for b, _ in decs:
            r = sorted(v / w for v, w in zip(ms[b], ms[builds[0][0]]))
            q = statistics.quantiles(r, n=4)
            row += f"  {b} {statistics.median(ms[b]):9.4f} ms  {statistics.median(r):.4f} ({q[0]:.4f} .. {q[2]:.4f})"
        lines.append(row)
        print(row, flush=True)
    for _, d in decs:
        d.close()
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
