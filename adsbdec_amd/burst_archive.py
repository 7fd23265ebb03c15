"""A capture cut down to its bursts: the numpy statement that adsb_gather_layout and adsb_gather_device (include/adsbdec_amd.h,
csrc/gather.h, csrc/gather_kernel.hip) are held to, byte for byte, and the burst archive (.brs) that holds the result.

The layout.  A capture has M power samples at s bytes each (SAMPLE_BYTES: 2 for int8 IQ; 4 for uint16 real, int16 IQ and float32
power; 8 for float32 IQ) and an ordered burst table of B records (levels.bursts).  Piece i is the power samples
[lo_i, hi_i) = [28 begin_i, min(28 end_i, M)) (levels.burst_samples); its bytes are capture[s lo_i : s hi_i].  The pieces lie in the
output in table order, each from a multiple of 16 bytes on:

    off_0 = 0        off_{i+1} = round_up(off_i + s (hi_i - lo_i), 16)        total = off_B        pad bytes are zero

A piece's start is then a legal adsb_decode_batch_device* pointer: 16-byte aligned, at a multiple of 4 samples.  What follows from
28 being 4 x 7: for s = 4 and 8 every source offset s lo_i is a multiple of 16; for s = 2 it is 56 begin_i, which is 0 (begin
even) or 8 (begin odd) mod 16.  A piece's length is a multiple of 16 except in two cases: the table's last piece where M clips it,
and s = 2 with an odd number of runs (56 x odd is 8 mod 16).

The archive, little-endian.  A header of 64 bytes:

    0 magic "ADSBBRS1" | 8 u32 version 1 | 12 u32 kind | 16 u32 sample_bytes | 20 u64 n_units | 28 u64 M | 36 f32 threshold
    | 40 u32 lead | 44 u32 hang | 48 u64 n_bursts | 56 u64 payload_bytes

(no reserved words: the eleven fields are 64 bytes as they stand, so the 64-bit fields lie at multiples of 4, not of 8, and a reader
takes them byte by byte.)  kind is the call's format number (KINDS: 4 uint16 real, 2 int16 IQ, 0 float32 IQ, 8 int8 IQ, 16 float32 power), n_units the capture's
length in its own samples.  Behind the header the table, n_bursts records of 16 bytes (levels.BURST_DTYPE, adsb_burst), and behind
it the payload: the layout's output, which starts at a multiple of 16 because 64 + 16 B is one.  A reader refuses a file it does not
understand: another magic or version, a kind and sample_bytes that do not go together, a table the layout refuses, a payload of
another size than the layout's total.

Decoding an archive (decode): the pieces go through ONE adsb_decode_batch_host* call of the archive's kind on a FLUSH handle (a
piece is far below the end-of-file horizon), pointers payload + off_i.  Piece i's records are those of its silent twin; they are
reported with g + 28 begin_i, which is exact, and ts + 28 begin_i -- in the original stream ts lags g by what accepted frames jumped
(demod.c:99,128,134), so this is the original's ts only up to those jumps.  The Try/Ok table is the sum of the pieces' tables.

The 12-bit layout (kind 12, BRS_KIND_PACKED12_REAL; layout12, gather12; adsb_gather_pack12_*, csrc/gather_pack12.h).  A real capture
is n uint16 samples x carrying 12-bit codes, M = 2 (n // 4); piece i is the samples x[2 lo_i : 2 hi_i].  2 lo_i is a multiple of 8;
2 hi_i is one too, or -- where M clips the last piece and M % 4 == 2 -- 4 behind one.  The piece is completed to whole groups of 8
with code 2048 (the silence the decoders read outside a buffer: at most four codes, on that clipped last piece only), masked with
0x0FFF and packed as Airspy packed 12-bit samples (packed12.pack12): 12 ceil((hi_i - lo_i) / 4) bytes, 84 per run, 3 bytes per power
sample where kind 4 takes 4.

    off_0 = 0        off_{i+1} = round_up(off_i + 12 ceil((hi_i - lo_i) / 4), 16)        total = off_B        pad bytes are zero

A piece's start is a legal adsb_decode_batch_device_packed pointer (4-byte aligned, a multiple of 8 samples).  `over` counts the
pieces' OWN samples above 4095 -- never the fill, never a sample outside the pieces; their low 12 bits are what is stored.  Every
real flavour has a uint16 twin to gather from: a uint16 capture itself, the unpacked or converted scratch of a packed or _as one.
In the archive kind 12 goes with sample_bytes 3, n_units counts the capture's samples, and the payload is checked against layout12.

A stream of any length (record_statement; the host program's -S -O).  The archive of a uint16 stream that is read in pieces of
`piece` runs is the archive of the whole: levels.bursts of the whole envelope at ONE threshold, fixed by the first piece (a factor
times the median of its power samples, or a float given outright), and the gather of that table.  The host program gets there
piece by piece -- adsb_bursts_slice_device joins the bursts across the pieces, and a piece's gathered bytes, a multiple of 16, are
appended to those before -- and the result does not depend on the piece.

Out of scope: gathering straight from a packed source without the unpack, 12-bit forms of the IQ and power kinds, a batch form,
the multi-GPU driver; in the record mode: other input than uint16, kind 12, run numbers beyond 32 bits.

    python -m adsbdec_amd.burst_archive info file.brs      the header and the kept share
"""
from __future__ import annotations

import struct
import sys

import numpy as np

from . import levels
from .levels import BURST_DTYPE, RUN, burst_samples
from .packed12 import pack12

MAGIC = b"ADSBBRS1"
VERSION = 1
HEADER = struct.Struct("<8sIIIQQfIIQQ")
assert HEADER.size == 64
BRS_KIND_PACKED12_REAL = 12                                   # a real capture's pieces as Airspy packed 12-bit samples (layout12)
KINDS = {4: "uint16 real", 2: "int16 IQ", 0: "float32 IQ", 8: "int8 IQ", 16: "float32 power", BRS_KIND_PACKED12_REAL: "packed 12-bit real"}
SAMPLE_BYTES = {4: 4, 2: 4, 0: 8, 8: 2, 16: 4, BRS_KIND_PACKED12_REAL: 3}             # bytes per POWER sample
UNITS_PER_POWER_SAMPLE = {4: 2, 2: 1, 0: 1, 8: 1, 16: 1, BRS_KIND_PACKED12_REAL: 2}   # the capture's own samples per power sample
UNIT_DTYPES = {4: "<u2", 2: "<i2", 0: "<f4", 8: "i1", 16: "<f4", BRS_KIND_PACKED12_REAL: "u1"}  # (kind 12: a piece is bytes, 12 per 8 samples)
FILL12 = 2048                                                 # the code that completes a clipped last piece to a whole group


class ArchiveError(ValueError):
    """A burst table the layout refuses, or a file that is no burst archive of this version."""


def power_samples(kind: int, n_units: int) -> int:
    """The most power samples a capture of n_units of its own samples has: 2 floor(n / 4) for real samples (the reference reads four
    at a time), n for complex and power samples (what the export and level calls of the kind count)."""
    return 2 * (n_units // 4) if kind in (4, BRS_KIND_PACKED12_REAL) else n_units


def _table(bursts) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(bursts, dtype=BURST_DTYPE).reshape(-1))


def check(bursts, M: int, s: int) -> np.ndarray:
    """The table as a contiguous array, or ArchiveError naming the record: what adsb_gather_layout refuses."""
    if s not in (2, 4, 8):
        raise ArchiveError(f"sample_bytes = {s} is none of 2, 4, 8")
    b = _table(bursts)
    begin, end = b["begin"].astype(np.int64), b["end"].astype(np.int64)
    for i in range(b.size):
        if end[i] <= begin[i]:
            raise ArchiveError(f"burst {i}: end = {end[i]} is not above begin = {begin[i]}")
        if RUN * begin[i] >= M:
            raise ArchiveError(f"burst {i}: begin = {begin[i]} lies outside the capture's m = {M}")
        if i and begin[i] <= end[i - 1]:
            raise ArchiveError(f"burst {i}: begin = {begin[i]} does not leave a run behind burst {i - 1}'s end = {end[i - 1]}")
    return b


def layout(bursts, M: int, s: int) -> np.ndarray:
    """offsets[B + 1], uint64: where piece i starts in the output, and the total."""
    b = check(bursts, M, s)
    sl = burst_samples(b, M)
    size = (s * (sl[:, 1] - sl[:, 0]) + 15) // 16 * 16
    off = np.zeros(b.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(size)
    return off


def gather(capture_bytes, bursts, M: int, s: int):
    """-> (out, offsets): the uint8 array the layout describes, of the capture's bytes (any array; its bytes are taken as they lie)."""
    cap = np.ascontiguousarray(capture_bytes).reshape(-1).view(np.uint8)
    if cap.size < s * M:
        raise ArchiveError(f"the capture's {cap.size} bytes hold fewer than m = {M} power samples of {s} bytes")
    off = layout(bursts, M, s)
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    for (lo, hi), at in zip(burst_samples(_table(bursts), M), off[:-1]):
        out[int(at):int(at) + s * int(hi - lo)] = cap[s * int(lo):s * int(hi)]
    return out, off


# ------------------------------------------------------------------ the 12-bit layout
def piece_bytes12(lo: int, hi: int) -> int:
    """Bytes of the packed piece of power samples [lo, hi): whole groups of 8 samples, 12 bytes each."""
    return 12 * -(-(hi - lo) // 4)


def layout12(bursts, M: int) -> np.ndarray:
    """offsets[B + 1], uint64: where packed piece i starts in the output of gather12 / adsb_gather_pack12_*, and the total."""
    b = check(bursts, M, 4)
    off = np.zeros(b.size + 1, dtype=np.uint64)
    at = 0
    for i, (lo, hi) in enumerate(burst_samples(b, M)):
        at = (at + piece_bytes12(int(lo), int(hi)) + 15) // 16 * 16
        off[i + 1] = at
    return off


def gather12(x, bursts, M: int):
    """-> (payload, offsets, over): the pieces of the uint16 capture x, each completed to whole groups with code 2048, masked to 12
    bits and packed; over = the pieces' own samples above 4095."""
    x = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1)
    if x.size < 2 * M:
        raise ArchiveError(f"the capture's {x.size} samples hold fewer than m = {M} power samples")
    off = layout12(bursts, M)
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    over = 0
    for (lo, hi), at in zip(burst_samples(_table(bursts), M), off[:-1]):
        own = x[2 * int(lo):2 * int(hi)]
        over += int(np.count_nonzero(own > 0x0FFF))
        whole = np.full(-(-own.size // 8) * 8, FILL12, dtype=np.uint16)
        whole[:own.size] = own
        p = pack12(whole & 0x0FFF)
        out[int(at):int(at) + p.size] = p
    return out, off, over


def _layout_of(kind: int, bursts, M: int) -> np.ndarray:
    return layout12(bursts, M) if kind == BRS_KIND_PACKED12_REAL else layout(bursts, M, SAMPLE_BYTES[kind])


# ------------------------------------------------------------------ the archive
def pack(kind: int, n_units: int, M: int, threshold: float, lead: int, hang: int, bursts, payload) -> bytes:
    """The archive's bytes.  The payload is what gather returns for the table (its size is checked, its bytes are not)."""
    if kind not in KINDS:
        raise ArchiveError(f"kind = {kind} is none of {sorted(KINDS)}")
    s = SAMPLE_BYTES[kind]
    b = _table(bursts)
    payload = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    total = int(_layout_of(kind, b, M)[-1])
    if payload.size != total:
        raise ArchiveError(f"the payload has {payload.size} bytes, the table's layout {total}")
    head = HEADER.pack(MAGIC, VERSION, kind, s, n_units, M, threshold, lead, hang, b.size, total)
    return head + b.tobytes() + payload.tobytes()


def write(path, kind: int, n_units: int, M: int, threshold: float, lead: int, hang: int, bursts, payload) -> int:
    """Write the archive to `path`; returns its size in bytes."""
    data = pack(kind, n_units, M, threshold, lead, hang, bursts, payload)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def record_statement(x, piece: int, factor_or_threshold: float, lead: int, hang: int, *, a, absolute: bool = False) -> bytes:
    """The archive the host program's -S factor,lead,hang,piece -O must write for the uint16 stream x, numpy only.  a: the 2 (n // 4)
    power samples of x (the reference's ampbuff: adsb_power_device, or the oracle).  The threshold is float32(factor x the median of
    the first piece's power samples, a[:28 piece]) -- levels.percentile of their report at 0.5 -- or, with absolute, the float given;
    the table is levels.bursts of the WHOLE envelope, the payload gather's, the bytes pack's: version 1, kind 4.  ArchiveError where
    the first piece has no sign-clear sample to take a median of."""
    x = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1)
    a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
    M = 2 * (x.size // 4)
    if a.size != M or int(piece) < 1:
        raise ArchiveError(f"{a.size} power samples for a stream of {x.size} samples (M = {M}), in pieces of {piece} runs")
    if absolute:
        threshold = float(np.float32(factor_or_threshold))
    else:
        first = levels.level_report(a[:RUN * int(piece)])
        if int(np.asarray(first["hist"]).sum()) == 0:
            raise ArchiveError("the first piece has no sign-clear power sample: the gate has no threshold")
        threshold = float(np.float32(factor_or_threshold * levels.percentile(first["hist"], 0.5)))
    table = levels.bursts(levels.level_report(a)["env"], threshold, lead, hang)
    payload, _ = gather(x, table, M, 4)
    return pack(4, x.size, M, threshold, lead, hang, table, payload)


def unpack(data: bytes) -> dict:
    """The archive in `data` -> dict(kind, sample_bytes, n_units, M, threshold, lead, hang, bursts, offsets, payload), or ArchiveError."""
    if len(data) < HEADER.size:
        raise ArchiveError(f"{len(data)} bytes are no burst archive: the header alone has {HEADER.size}")
    magic, version, kind, s, n_units, M, threshold, lead, hang, n_bursts, payload_bytes = HEADER.unpack_from(data)
    if magic != MAGIC:
        raise ArchiveError(f"bad magic {magic!r}: no burst archive")
    if version != VERSION:
        raise ArchiveError(f"version {version}: this reader knows version {VERSION}")
    if kind not in KINDS or SAMPLE_BYTES[kind] != s:
        raise ArchiveError(f"kind {kind} with sample_bytes {s}: no format this reader knows")
    if M > power_samples(kind, n_units):
        raise ArchiveError(f"M = {M} power samples are more than the {n_units} units of a {KINDS[kind]} capture make")
    if n_bursts > (len(data) - HEADER.size) // BURST_DTYPE.itemsize:
        raise ArchiveError(f"the file is too short for its table of {n_bursts} bursts")
    b = np.frombuffer(data, dtype=BURST_DTYPE, count=n_bursts, offset=HEADER.size)
    off = _layout_of(kind, b, M)
    at = HEADER.size + BURST_DTYPE.itemsize * n_bursts
    if payload_bytes != int(off[-1]) or len(data) - at != payload_bytes:
        raise ArchiveError(f"the payload has {len(data) - at} bytes, the header says {payload_bytes}, the table's layout {int(off[-1])}")
    return dict(kind=kind, sample_bytes=s, n_units=n_units, M=M, threshold=threshold, lead=lead, hang=hang, bursts=b, offsets=off,
                payload=np.frombuffer(data, dtype=np.uint8, count=payload_bytes, offset=at))


def read(path) -> dict:
    with open(path, "rb") as f:
        return unpack(f.read())


def piece_units(archive: dict) -> list:
    """The length of every piece in the capture's own samples: what the batch call of the archive's kind counts."""
    per = UNITS_PER_POWER_SAMPLE[archive["kind"]]
    if archive["kind"] == BRS_KIND_PACKED12_REAL:  # whole groups of 8 samples: a clipped last piece counts its fill
        return [8 * -(-int(hi - lo) // 4) for lo, hi in burst_samples(archive["bursts"], archive["M"])]
    return [per * int(hi - lo) for lo, hi in burst_samples(archive["bursts"], archive["M"])]


def decode(decoder, archive: dict):
    """The archive's frames through ONE adsb_decode_batch_host* call on `decoder`, a capi.Decoder with flush=True -> (frames, stats):
    the frames of all pieces in order, g and ts shifted by 28 begin_i; stats the sum of the pieces' Try/Ok tables."""
    if not decoder.flush:
        raise ArchiveError("an archive decodes on a flush handle (Decoder(flush=True)): a piece is far below the end-of-file horizon")
    kind, off = archive["kind"], archive["offsets"]
    # (the payload's own memory need not be 16-byte aligned, and a piece's view of it is at the alignment of its dtype: host calls ask no more)
    payload = np.ascontiguousarray(archive["payload"])
    units = piece_units(archive)
    item = np.dtype(UNIT_DTYPES[kind]).itemsize
    if kind == BRS_KIND_PACKED12_REAL:
        pieces = [payload[int(o):int(o) + n // 8 * 12] for o, n in zip(off[:-1], units)]
    else:
        per_unit = archive["sample_bytes"] // UNITS_PER_POWER_SAMPLE[kind]
        pieces = [payload[int(o):int(o) + per_unit * n].view(UNIT_DTYPES[kind]) for o, n in zip(off[:-1], units)]
        assert all(p.size * item == per_unit * n for p, n in zip(pieces, units))
    if not pieces:
        return [], {"try": {11: 0, 17: 0, 18: 0}, "ok": {11: 0, 17: 0, 18: 0}}
    if kind == BRS_KIND_PACKED12_REAL:
        frames, stats = decoder.decode_batch_packed(pieces, stats=True)
    elif kind == 4:
        frames, stats = decoder.decode_batch(pieces, stats=True)
    elif kind == 16:
        frames, stats = decoder.decode_batch_power(pieces, stats=True)
    else:
        frames, stats = decoder.decode_batch_iq(kind, pieces, stats=True)
    out = []
    for rec, mine in zip(archive["bursts"], frames):
        shift = RUN * int(rec["begin"])
        out += [dict(f, g=f["g"] + shift, ts=f["ts"] + shift) for f in mine]
    total = {k: {df: sum(st[k][df] for st in stats) for df in (11, 17, 18)} for k in ("try", "ok")}
    if any("fixed" in st for st in stats):
        total["fixed"] = sum(st.get("fixed", 0) for st in stats)
    return out, total


def info(archive: dict) -> str:
    kept, whole = int(archive["offsets"][-1]), archive["sample_bytes"] * archive["M"]
    share = f"{100.0 * kept / whole:.3f} %" if whole else "-"
    return (f"burst archive version {VERSION}: {KINDS[archive['kind']]} (kind {archive['kind']}), {archive['sample_bytes']} bytes per power sample\n"
            f"capture: {archive['n_units']} samples, {archive['M']} power samples\n"
            f"gate: threshold {archive['threshold']:.9g}, lead {archive['lead']}, hang {archive['hang']}\n"
            f"kept {archive['bursts'].size} bursts, {kept} of {whole} bytes ({share})\n")


def main(argv) -> int:
    if len(argv) != 3 or argv[1] != "info":
        sys.stderr.write("usage: python -m adsbdec_amd.burst_archive info file.brs\n")
        return 2
    try:
        sys.stdout.write(info(read(argv[2])))
    except (ArchiveError, OSError) as e:
        sys.stderr.write(f"{argv[2]}: {e}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
