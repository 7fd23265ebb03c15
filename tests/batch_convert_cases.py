"""The cases and the expectation that hold the batch conversion kernel (csrc/convert_samples.hip convert_batch_kernel) word for
word: tests/test_batch_convert_cpu.py pins them on the CPU, tests/test_gpu_batch_convert.py holds the kernel to them.

A conversion is S16 (int16 real), F32 (float32 real) or F32_IQ (the float32 scalars of a complex capture).  Per conversion there
are two calls with different capture patterns (CALLS), built by call(conv, k), and two small batches for the counters alone
(counter_batch).  Lengths are in samples for the real formats and in COMPLEX samples for IQ; the kernel sees the scalars, two per
complex sample, and `scalars` is what every layout below counts.  A capture of s scalars is ceil(s / 8) groups of 8, the last one
possibly short (the sample-by-sample road); a block takes chunks of CHUNK consecutive groups of the whole batch, GRID blocks at
most, so chunk c >= GRID is a block's second trip.

Expected codes and flags: adsbdec_amd.sample_formats.flags_int16_real / flags_float32_real / flags_float32_iq.  Expected scratch:
capture i from slots(scalars)[0][i] on (128-byte rounded, in uint16 samples), nothing else written -- Scratch keeps what two
calls in a row leave, with a mask of what is known."""
import functools

import numpy as np

from conftest import load_golden
from test_iq_cpu import edge_bits, load_iq

S16, F32, F32_IQ = 3, 1, 8                       # the _as numbers of the real formats; the library's number for the IQ scalars
CONVS = (S16, F32, F32_IQ)
NAMES = {S16: "s16", F32: "f32", F32_IQ: "f32_iq"}
ELEM = {S16: 2, F32: 4, F32_IQ: 4}               # bytes per scalar
PER = {S16: 1, F32: 1, F32_IQ: 2}                # scalars per sample of the call's n[]
DTYPE = {S16: np.dtype("<i2"), F32: np.dtype("<f4"), F32_IQ: np.dtype("<f4")}
CHUNK, GRID = 256, 2048                          # sample_format.h kConvertChunk; launch_convert_batch's block limit
NO_OFFSETS = 81_952                              # the longest real capture without an offset to scan (air.c:94); IQ: half of it
CALLS = ((4600, True), (4601, False))            # (seed, big captures first)
N_EDGE_IQ = 12 + 17 + 4096 + 4096                # edge_bits() without its random tail


def _flags(conv, x):
    from adsbdec_amd import sample_formats as S
    if conv == S16:
        codes, inexact = S.flags_int16_real(x)
        return codes, inexact, np.zeros(inexact.shape, bool)
    if conv == F32:
        return S.flags_float32_real(x)
    codes, inexact, clamped = S.flags_float32_iq(x)
    return codes.view(np.uint16), inexact, clamped


def expected(conv, x):
    """Scalars of one capture -> (uint16 codes -- the int16 scalars of IQ viewed as uint16 --, inexact mask, clamped mask)."""
    return _flags(conv, np.ascontiguousarray(x, dtype=DTYPE[conv]).reshape(-1))


def on_grid(conv, rng, n):
    """n random scalars that lie on the conversion's grid."""
    from adsbdec_amd import sample_formats as S
    if conv == F32_IQ:
        return S.to_float32_iq(rng.integers(-32768, 32768, n).astype(np.int16))
    return S.to_format(conv, rng.integers(0, 4096, n, dtype=np.uint16))


def random_source(conv, n, rng):
    """n scalars of random bits, as tests/test_gpu_sample_formats.py _random_source plants them: int16 any 16 bits; float a
    quarter in range and off the grid, a quarter on it, the rest any bits, and every 48th scalar one of the special values
    (+-Inf, NaN, denormals, -0.0, +-1.0, a grid point, a tie; IQ: the edge vector of tests/test_iq_cpu.py)."""
    if conv == S16:
        return rng.integers(0, 1 << 16, n, dtype=np.uint32).astype("<u2").view("<i2")
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    k = n // 4
    bits[:k] = (bits[:k] & 0x80FFFFFF) | 0x3F000000            # |x| in [0.5, 1): inside the range, off either grid
    bits[k:2 * k] = on_grid(conv, rng, k).view("<u4")
    if conv == F32:
        special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x807FFFFF, 0x80000000, 0x3F800000, 0xBF800000,
                            0x3A000000, 0x39800000], dtype="<u4")
    else:
        special = _edge_iq()
    rng.shuffle(bits)
    if n:
        at = rng.integers(0, n, (n + 47) // 48)
        bits[at] = special[rng.integers(0, special.size, at.size)]
    return bits.view("<f4")


@functools.lru_cache(maxsize=None)
def _edge_iq():
    e = edge_bits()[:N_EDGE_IQ]
    # the specials and the values next to a tie or a clamp as often as the thousands of grid points and exact ties behind them
    return np.concatenate([np.tile(e[:29], 280), e])


# ---------------------------------------------------------------- the capture patterns
def tails(conv):
    """The lengths of a short last group, in scalars."""
    return (2, 4, 6) if conv == F32_IQ else (1, 2, 3, 4, 5, 6, 7)


def decodable(conv):
    """A few captures with frames, on their grid: [(name, scalars in the conversion's format, raw twin)] -- the raw twin is what
    decode_batch (real: uint16 codes) or decode_batch_iq with fmt 2 (IQ: int16 pairs) takes."""
    from adsbdec_amd import sample_formats as S
    if conv == F32_IQ:
        out = []
        for name, cut in (("mixed_df_a", None), ("ragged", None), ("full_scale", 47_999)):
            x = np.ascontiguousarray(load_iq(name)[0][:cut])
            out.append((name, S.to_float32_iq(x).reshape(-1), x))
        return out
    mixed, ragged = load_golden("mixed_df_a_384Ki")[0], load_golden("ragged_tail")[0]
    caps = (("ragged_tail", ragged), ("mixed_df_a[:131075]", mixed[:131_075]), ("mixed_df_a[150000:250001]", mixed[150_000:250_001]))
    return [(name, S.to_format(conv, x), np.ascontiguousarray(x)) for name, x in caps]


def lengths(conv, k):
    """The capture lengths of call k, in samples of the call's n[] (IQ: complex samples); a str names a decodable capture."""
    seed, big_first = CALLS[k]
    rng = np.random.default_rng(seed)
    per = PER[conv]
    top = 8 // per                                           # samples of a whole group
    # captures of one short group each, side by side: 520 of them hold a whole chunk (256 groups from a multiple of 256 on)
    # wherever they start -- a chunk of 256 rows and nothing but the short road
    short = [int(v) for v in rng.integers(1, top, size=520)]
    # ~500 captures of 1 .. 40 scalars, a capture without samples every 23
    small = [int(v) for v in rng.integers(1, 40 // per + 1, size=500)]
    for at in range(7, 500, 23):
        small.insert(at, 0)
    # 255 / 256 / 257 groups: once exact, once with the last group short
    edge = []
    for j, g in enumerate((255, 256, 257)):
        edge += [g * top, (g - 1) * top + tails(conv)[(j + k) % len(tails(conv))] // per]
    # every tail length behind many whole groups
    tail = [int(rng.integers(300, 900)) * top + t // per for t in tails(conv)]
    # captures without an offset to scan, up to the longest such: they bring the batch's groups above GRID * CHUNK
    longest = NO_OFFSETS // per
    big = [longest - int(v) for v in rng.integers(0, 64, size=52)]
    big[0] = big[-1] = longest
    names = [name for name, _, _ in decodable(conv)]
    if big_first:   # (the larger pattern: the second call fits the scratch this one leaves)
        return big[:30] + names[:2] + edge + big[30:] + names[2:] + tail + small + [40 // per] * 60 + short
    return small[:300] + edge + short + small[300:] + tail + big[:20] + names + big[20:] + [3, 0, 1] * 10


def slots(scalars):
    """-> (every capture's first sample in the scratch, the scratch's size), in uint16 samples: 128-byte rounded slots."""
    at, cur = [], 0
    for n in scalars:
        at.append(cur)
        cur += (2 * n + 127) // 128 * 64
    return at, cur


def device_offsets(scalars, elem):
    """Byte offsets of the captures side by side in one device buffer (16-byte aligned itself): every capture starts
    elem, 2 elem, ... bytes past a 16-byte boundary in turn, and at one now and then.  -> (offsets, bytes of the buffer)."""
    skew = [elem * j for j in range(1, 16 // elem)] + [0]
    at, cur = [], 0
    for i, n in enumerate(scalars):
        cur = (cur + 15) // 16 * 16 + skew[i % len(skew)]
        at.append(cur)
        cur += n * elem
    return at, cur + 16


class Batch:
    """One call's captures: n (what the call takes), scalars, src (arrays of the conversion's dtype), codes (uint16), the two
    counts, and frames = {capture index: raw twin} of the decodable captures."""

    def __init__(self, conv, n, src, frames=None):
        self.conv, self.n, self.src, self.frames = conv, [int(v) for v in n], src, frames or {}
        self.scalars = [int(s.size) for s in src]
        assert self.scalars == [PER[conv] * v for v in self.n] and all(s.dtype == DTYPE[conv] for s in src)
        whole = np.concatenate(src) if src else np.empty(0, DTYPE[conv])
        codes, inexact, clamped = expected(conv, whole)
        self.inexact, self.clamped = int(inexact.sum()), int(clamped.sum())
        ends = np.cumsum(self.scalars)
        self.codes = [codes[e - s:e] for s, e in zip(self.scalars, ends)]
        off = inexact | clamped
        self.off_grid = [off[e - s:e] for s, e in zip(self.scalars, ends)]
        self.at, self.total = slots(self.scalars)

    def report(self):
        return (sum(self.scalars), self.inexact, self.clamped)

    def host_bytes(self):
        return sum(s.nbytes for s in self.src) + sum(c.nbytes for c in self.codes) + sum(o.nbytes for o in self.off_grid)

    def device_image(self):
        """-> (the bytes of the device buffer, every capture's byte offset in it)."""
        at, total = device_offsets(self.scalars, ELEM[self.conv])
        rng = np.random.default_rng(4700)
        host = rng.integers(0, 256, total, dtype=np.uint8)   # the gaps: a neighbour's samples are never silence
        for a, s in zip(at, self.src):
            host[a:a + s.nbytes] = s.view(np.uint8)
        return host, at

    def n_off_grid(self, short_road):
        """The off-grid scalars that lie in a short last group (short_road) or in a whole group (not)."""
        total = 0
        for s, o in zip(self.scalars, self.off_grid):
            cut = s // 8 * 8
            total += int(o[cut:].sum()) if short_road else int(o[:cut].sum())
        return total


@functools.lru_cache(maxsize=2)
def call(conv, k):
    rng = np.random.default_rng(CALLS[k][0] + 10 * conv)
    dec = {name: (src, raw) for name, src, raw in decodable(conv)}
    ns, src, frames = [], [], {}
    for i, n in enumerate(lengths(conv, k)):
        if isinstance(n, str):
            frames[i] = dec[n][1]
            src.append(dec[n][0])
            ns.append(dec[n][0].size // PER[conv])
        else:
            src.append(random_source(conv, PER[conv] * n, rng))
            ns.append(n)
    return Batch(conv, ns, src, frames)


@functools.lru_cache(maxsize=None)
def counter_batch(conv, short_road):
    """~260 captures for the two counters alone.  short_road: every off-grid scalar lies in a short last group, everything in a
    whole group is on the grid; not short_road: the other way round.  A count lost on one road cannot hide in the other."""
    rng = np.random.default_rng(4800 + conv + (100 if short_road else 0))
    per = PER[conv]
    top = 8 // per
    ns = [int(v) for v in rng.integers(1, top, size=100)] + [int(v) for v in rng.integers(1, 40 * top, size=150)] + [3 * top, 0, top] * 4
    src = []
    for n in ns:
        s = per * n
        cut = s // 8 * 8
        wild, tame = random_source(conv, s, rng), on_grid(conv, rng, s)
        src.append(np.concatenate([tame[:cut], wild[cut:]] if short_road else [wild[:cut], tame[cut:]]).astype(DTYPE[conv]))
    return Batch(conv, ns, src)


class Scratch:
    """What the handle's scratch holds across calls: `model` where `known`.  A call writes its captures' codes at their slots and
    nothing else, so a pad keeps what an earlier call put there."""

    def __init__(self, total):
        self.model, self.known = np.zeros(total, np.uint16), np.zeros(total, bool)

    def write(self, batch):
        assert batch.total <= self.model.size                # (the scratch is not reallocated)
        for a, c in zip(batch.at, batch.codes):
            self.model[a:a + c.size] = c
            self.known[a:a + c.size] = True

    def pad(self, batch, i):
        """-> (slot length, the known mask of capture i's pad, the model's samples there)."""
        a, n = batch.at[i], batch.scalars[i]
        end = batch.at[i + 1] if i + 1 < len(batch.at) else batch.total
        return end - a, self.known[a + n:end], self.model[a + n:end]


# ---------------------------------------------------------------- what the kernel's geometry makes of a pattern
def geometry(scalars):
    """The facts the GPU test rests on, from the lengths alone: chunks; the most rows a chunk holds and the most a chunk of the
    second trip holds; whether a second-trip chunk starts in one capture and ends in another; the tail lengths that occur; and
    whether some chunk consists of CHUNK short groups of CHUNK different captures."""
    rows = [n for n in scalars if n]
    g_first = np.concatenate([[0], np.cumsum([(n + 7) // 8 for n in rows])])
    groups = int(g_first[-1])
    chunks = (groups + CHUNK - 1) // CHUNK
    g0 = np.arange(chunks, dtype=np.int64) * CHUNK
    g1 = np.minimum(g0 + CHUNK - 1, groups - 1)
    r0 = np.searchsorted(g_first, g0, side="right") - 1
    r1 = np.searchsorted(g_first, g1, side="right") - 1
    per_chunk = r1 - r0 + 1
    short_row = np.array([n < 8 for n in rows])
    all_short = [bool(per_chunk[c] == CHUNK and short_row[r0[c]:r1[c] + 1].all()) for c in range(chunks)]
    return dict(groups=groups, chunks=chunks, rows_max=int(per_chunk.max()), rows_max_second_trip=int(per_chunk[GRID:].max()) if chunks > GRID else 0,
                second_trip_straddles=bool((per_chunk[GRID:] >= 2).any()), tails={n % 8 for n in rows if n >= 8},
                short_chunks=int(np.sum(all_short)), short_chunks_second_trip=int(np.sum(all_short[GRID:])))
