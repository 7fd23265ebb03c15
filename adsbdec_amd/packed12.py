"""Airspy packed 12-bit samples (include/adsbdec_amd.h: the format) in plain numpy: the test-side definition, independent of
the library's unpack kernel, and a converter for capture files.

A group is 8 samples s0..s7 (12-bit codes) in three little-endian 32-bit words w0, w1, w2; read as one 96-bit big-endian
number w0:w1:w2 the group is s0 s1 ... s7, 12 bits each, most significant first.

    python -m adsbdec_amd.packed12 in.u16 out.p12            # uint16 capture -> packed
    python -m adsbdec_amd.packed12 --unpack in.p12 out.u16   # packed -> uint16 (a trailing partial group is dropped)
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

GROUP_SAMPLES = 8
GROUP_BYTES = 12


def packed_bytes(n_samples: int) -> int:
    """ADSB_PACKED12_BYTES(n): bytes that n samples (a multiple of 8) take packed."""
    return n_samples // GROUP_SAMPLES * GROUP_BYTES


def pack12(x) -> np.ndarray:
    """uint16 samples (codes 0..4095, a multiple of 8 of them) -> packed bytes (uint8, 12 per 8 samples)."""
    x = np.asarray(x)
    if x.ndim != 1 or x.size % GROUP_SAMPLES:
        raise ValueError(f"pack12: {x.size} samples is not a whole number of 8-sample groups")
    if x.size and int(x.max()) > 0xFFF:
        raise ValueError("pack12: codes above 4095 do not fit 12 bits")
    s = x.astype(np.uint32).reshape(-1, GROUP_SAMPLES)
    w = np.empty((s.shape[0], 3), dtype="<u4")
    w[:, 0] = (s[:, 0] << 20) | (s[:, 1] << 8) | (s[:, 2] >> 4)
    w[:, 1] = ((s[:, 2] & 0xF) << 28) | (s[:, 3] << 16) | (s[:, 4] << 4) | (s[:, 5] >> 8)
    w[:, 2] = ((s[:, 5] & 0xFF) << 24) | (s[:, 6] << 12) | s[:, 7]
    return w.reshape(-1).view(np.uint8)


def unpack12(buf) -> np.ndarray:
    """Packed bytes (a multiple of 12) -> uint16 samples."""
    b = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    if b.size % GROUP_BYTES:
        raise ValueError(f"unpack12: {b.size} bytes is not a whole number of 12-byte groups")
    w = np.ascontiguousarray(b).view("<u4").astype(np.uint32).reshape(-1, 3)
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    s = np.empty((w.shape[0], GROUP_SAMPLES), dtype=np.uint16)
    s[:, 0] = w0 >> 20
    s[:, 1] = (w0 >> 8) & 0xFFF
    s[:, 2] = ((w0 & 0xFF) << 4) | (w1 >> 28)
    s[:, 3] = (w1 >> 16) & 0xFFF
    s[:, 4] = (w1 >> 4) & 0xFFF
    s[:, 5] = ((w1 & 0xF) << 8) | (w2 >> 24)
    s[:, 6] = (w2 >> 12) & 0xFFF
    s[:, 7] = w2 & 0xFFF
    return s.reshape(-1)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m adsbdec_amd.packed12", description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--unpack", action="store_true", help="packed -> uint16 instead of uint16 -> packed")
    a = ap.parse_args(argv)
    if a.unpack:
        b = np.fromfile(a.src, dtype=np.uint8)
        cut = b.size % GROUP_BYTES
        if cut:
            sys.stderr.write(f"{a.src}: {cut} trailing bytes (a partial group) ignored\n")
        unpack12(b[: b.size - cut]).tofile(a.dst)
    else:
        x = np.fromfile(a.src, dtype=np.uint16)
        cut = x.size % GROUP_SAMPLES
        if cut:
            sys.stderr.write(f"{a.src}: {cut} trailing samples (a partial group) ignored\n")
        pack12(x[: x.size - cut]).tofile(a.dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
