"""The burst gather and the burst archive without a GPU: the numpy statement (adsbdec_amd/burst_archive.py layout, gather) against
a literal loop over pieces and bytes on every named case and on random small tables, for s in {2, 4, 8}; adsb_gather_layout against
the statement, and each of its refusals naming the record; the properties the layout promises (source and length alignment); the
archive written and read back, in Python, through the C reader and writer built into a stand-alone program under AddressSanitizer
and UBSan, and through the host program's -k; every malformed file refused by all three; -K's and -k's refusals, before any GPU call;
the declarations, exports and bindings; and the pipeline fixture's condition at lead 2, hang 4 -- the payload is 4 x sum(hi - lo)
bytes plus padding, and under 1 % of the capture."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import burst_cases as BC
import gather_cases as GC
from conftest import ROOT

C_FOR_CPU = 4      # (the statement knows no chunk: any C gives valid cases; a small one keeps the byte loops short)


def BA():
    from adsbdec_amd import burst_archive
    return burst_archive


def LV():
    from adsbdec_amd import levels
    return levels


# ------------------------------------------------------------------ the statement
def test_statement_against_the_literal_loop_on_the_named_cases():
    for s in GC.S_ALL:
        for C_ in (C_FOR_CPU, 7):
            for name, M, tab in GC.named_cases(C_, s):
                cap = GC.capture_bytes(M, s, 41, extra=6)
                out, off = BA().gather(cap, tab, M, s)
                want, woff = GC.slow_gather(cap, tab, M, s)
                assert off.dtype == np.uint64 and off.tolist() == woff, (s, name)
                assert BA().layout(tab, M, s).tolist() == woff, (s, name)
                assert out.dtype == np.uint8 and out.tolist() == want, (s, name)


def test_statement_against_the_literal_loop_on_random_small_tables():
    for i, (M, tab) in enumerate(GC.random_tables(120, 4101, runs=210)):
        s = GC.S_ALL[i % 3]
        cap = GC.capture_bytes(M, s, i)
        out, off = BA().gather(cap, tab, M, s)
        want, woff = GC.slow_gather(cap, tab, M, s)
        assert off.tolist() == woff and out.tolist() == want, (i, s, M)


def test_layout_properties():
    """s = 4, 8: every source offset is a multiple of 16; s = 2: 0 or 8 mod 16, by begin's parity.  A piece's length is a multiple of
    16 but for the table's last piece where M clips it, and s = 2 with an odd number of runs.  Every piece starts at a multiple of 16
    and of 4 samples; pad bytes are zero; the pieces do not overlap."""
    cases = [(M, tab) for _, M, tab in GC.named_cases(256, 2)] + GC.random_tables(60, 4102)
    for s in GC.S_ALL:
        for M, tab in cases:
            off = BA().layout(tab, M, s)
            sl = LV().burst_samples(tab, M)
            assert off[0] == 0 and (off % 16 == 0).all() and (np.diff(off.astype(np.int64)) > 0).all()
            src = s * sl[:, 0]
            if s == 2:
                assert ((src % 16) == 8 * (tab["begin"].astype(np.int64) % 2)).all()
            else:
                assert (src % 16 == 0).all()
            length = s * (sl[:, 1] - sl[:, 0])
            runs = tab["end"].astype(np.int64) - tab["begin"].astype(np.int64)
            clipped = 28 * tab["end"].astype(np.int64) > M
            assert not clipped[:-1].any()
            ragged = length % 16 != 0
            assert (ragged <= (clipped | ((s == 2) & (runs % 2 == 1)))).all()
            assert (off[1:].astype(np.int64) == off[:-1].astype(np.int64) + (length + 15) // 16 * 16).all()
            cap = GC.capture_bytes(M, s, 7)
            out, _ = BA().gather(cap, tab, M, s)
            keep = np.zeros(out.size, bool)
            for (lo, hi), at in zip(sl, off[:-1]):
                keep[int(at):int(at) + s * int(hi - lo)] = True
            assert (out[keep] != 0).all() and (out[~keep] == 0).all()


# ------------------------------------------------------------------ adsb_gather_layout
def test_c_layout_is_the_statements(capi):
    cases = [(M, tab) for C_ in (4, 256) for _, M, tab in GC.named_cases(C_, 2)] + GC.random_tables(100, 4103)
    for s in GC.S_ALL:
        for M, tab in cases:
            want = BA().layout(tab, M, s)
            got = capi.gather_layout(tab, M, s)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (s, M, tab.size)
    # offsets and total are optional, each on its own
    L = capi.load()
    M, tab = cases[5]
    total = C.c_uint64(0)
    assert L.adsb_gather_layout(M, 4, tab.ctypes.data, tab.size, None, C.byref(total)) == 0 and total.value == int(BA().layout(tab, M, 4)[-1])
    off = np.zeros(tab.size + 1, np.uint64)
    assert L.adsb_gather_layout(M, 4, tab.ctypes.data, tab.size, off.ctypes.data, None) == 0 and np.array_equal(off, BA().layout(tab, M, 4))
    assert L.adsb_gather_layout(0, 4, None, 0, off.ctypes.data, C.byref(total)) == 0 and total.value == 0 and off[0] == 0
    # no 32-bit product anywhere: a piece beyond 2^32 bytes
    big = GC.table([(0, 1), ((1 << 31) - 40, (1 << 31) - 1)])
    assert np.array_equal(capi.gather_layout(big, 28 << 31, 8), BA().layout(big, 28 << 31, 8))
    assert int(BA().layout(big, 28 << 31, 8)[-1]) == 224 + 8 * 28 * 39


def test_refusals_name_the_record(capi):
    L = capi.load()
    for name, M, s, tab, word in GC.refusals():
        with pytest.raises(BA().ArchiveError) as e:
            BA().layout(tab, M, s)
        assert word in str(e.value), (name, str(e.value))
        off = np.full(tab.size + 1, 0x5A5A5A5A, np.uint64)
        total = C.c_uint64(77)
        assert L.adsb_gather_layout(M, s, tab.ctypes.data, tab.size, off.ctypes.data, C.byref(total)) == -1, name
        msg = L.adsb_last_error(None).decode()
        assert msg.startswith("adsb_gather_layout: ") and word in msg, (name, msg)
        assert (off == 0x5A5A5A5A).all() and total.value == 77, name                  # a refusal writes nothing
        with pytest.raises(capi.AdsbError) as e:
            capi.gather_layout(tab, M, s)
        assert word in str(e.value)
    assert L.adsb_gather_layout(100, 4, None, 3, None, None) == -1 and "NULL table" in L.adsb_last_error(None).decode()
    with pytest.raises(BA().ArchiveError):
        BA().gather(np.zeros(10, np.uint8), GC.table([(0, 1)]), 28, 4)                   # a capture shorter than s M


# ------------------------------------------------------------------ interface and build
def test_entry_points_are_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    text = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    main = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adsbdec_amd_diag.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name, n_args in (("adsb_gather_layout", 6), ("adsb_gather_device", 10)):
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == n_args and capi.SYMBOLS[name][0] is C.c_long, name
    assert re.search(r"\buint32_t\s+adsb_gather_chunk_words\s*\(\s*void\s*\)", diag) and "adsb_gather_chunk_words" in exported
    assert callable(capi.Decoder.gather_device) and callable(capi.gather_layout)
    assert capi.gather_chunk_words() == 256
    assert "gather_kernel.hip" in _build.HIP_SOURCES and "decoder_gather.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "gather_kernel.hip.o" in mk and "decoder_gather.hip.o" in mk and "burst_archive.c" in mk
    assert L.adsb_abi_version() == 5 and "#define ADSB_ABI_VERSION 5" in main               # only symbols were added
    assert len(text.splitlines()) <= 250
    # NULL handle: -1, nothing touched
    off = np.full(4, 0x5A, np.uint64)
    assert L.adsb_gather_device(None, None, 0, 4, 0, None, 0, None, 0, off.ctypes.data) == -1 and (off == 0x5A).all()
    for name in ("layout", "gather", "write", "read", "decode", "info"):
        assert callable(getattr(BA(), name)), name


def test_the_gather_is_one_kernel_without_scratch():
    """The unit's code object, by its directives alone: gfx950 only, ONE kernel, no scratch and no LDS."""
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "gather_kernel.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True,
                         check=True).stdout
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and all("gather_kernel" in k and int(v) == 0 for k, v in sizes.items()), sizes
    assert set(re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", isa)) == {"0"}


# ------------------------------------------------------------------ the archive
def _archive_case(s_kind):
    kind, s = s_kind
    M = 28 * 37 + 14
    tab = GC.table([(1, 2), (4, 9), (11, 12), (30, 38)])
    per = BA().UNITS_PER_POWER_SAMPLE[kind]
    n_units = per * M + (3 if kind == 4 else 0)
    cap = GC.capture_bytes(M, s, 50 + kind, extra=6 if kind == 4 else 0)
    payload, off = BA().gather(cap, tab, M, s)
    return dict(kind=kind, n_units=n_units, M=M, threshold=123.456, lead=2, hang=4, bursts=tab, payload=payload), off


KIND_S = [(4, 4), (2, 4), (0, 8), (8, 2), (16, 4)]


@pytest.mark.parametrize("s_kind", KIND_S)
def test_archive_write_read_is_the_identity(tmp_path, s_kind):
    a, off = _archive_case(s_kind)
    path = tmp_path / "a.brs"
    size = BA().write(path, **a)
    assert size == os.path.getsize(path) == 64 + 16 * a["bursts"].size + a["payload"].size
    data = path.read_bytes()
    assert data[:8] == b"ADSBBRS1" and struct.unpack_from("<III", data, 8) == (1, s_kind[0], s_kind[1])
    assert struct.unpack_from("<QQ", data, 48) == (a["bursts"].size, a["payload"].size)
    assert (64 + 16 * a["bursts"].size) % 16 == 0                                        # the payload starts at a multiple of 16
    r = BA().read(path)
    assert (r["kind"], r["sample_bytes"], r["n_units"], r["M"], r["lead"], r["hang"]) == (s_kind[0], s_kind[1], a["n_units"], a["M"], 2, 4)
    assert np.float32(r["threshold"]) == np.float32(123.456)
    assert np.array_equal(r["bursts"], a["bursts"]) and r["bursts"].dtype == LV().BURST_DTYPE
    assert np.array_equal(r["payload"], a["payload"]) and np.array_equal(r["offsets"], off)
    assert BA().pack(**{k: r[k] for k in a}) == data
    # an archive of no burst at all
    BA().write(tmp_path / "e.brs", s_kind[0], 100, 40, 1.0, 2, 4, GC.table([]), np.zeros(0, np.uint8))
    e = BA().read(tmp_path / "e.brs")
    assert e["bursts"].size == 0 and e["payload"].size == 0 and os.path.getsize(tmp_path / "e.brs") == 64


def malformed(good: bytes):
    """[(name, bytes, a word of the reason)]: every way of section 4's list, from a good archive of three or more bursts."""
    n_b = struct.unpack_from("<Q", good, 48)[0]
    out = [("bad magic", b"ADSBBRS2" + good[8:], "magic"),
           ("version 2", good[:8] + struct.pack("<I", 2) + good[12:], "version"),
           ("an unknown kind", good[:12] + struct.pack("<I", 5) + good[16:], "kind"),
           ("sample_bytes that do not go with the kind", good[:16] + struct.pack("<I", 2 if good[16] != 2 else 4) + good[20:], "sample_bytes"),
           ("shorter than a header", good[:40], "header"),
           ("a payload one byte short", good[:-1], "payload"),
           ("a payload sixteen bytes long", good + bytes(16), "payload"),
           ("payload_bytes that is not the layout's", good[:56] + struct.pack("<Q", struct.unpack_from("<Q", good, 56)[0] + 16) + good[64:] + bytes(16), "payload"),
           ("more bursts than the file holds", good[:48] + struct.pack("<Q", 1 << 40) + good[56:], "table")]
    # a table the layout refuses: the second record's end below its begin; two records swapped; a record outside M
    rec = lambda i: 64 + 16 * i
    t = bytearray(good)
    t[rec(1) + 4:rec(1) + 8] = struct.pack("<I", 0)
    out.append(("a record with end <= begin", bytes(t), "burst 1"))
    t = bytearray(good)
    t[rec(0):rec(1)], t[rec(1):rec(2)] = good[rec(1):rec(2)], good[rec(0):rec(1)]
    out.append(("records that descend", bytes(t), "burst 1"))
    t = bytearray(good)
    t[28:36] = struct.pack("<Q", 28 * 20)
    out.append(("a record outside M", bytes(t), f"burst {n_b - 1}"))
    t = bytearray(good)
    t[20:28] = struct.pack("<Q", 10)
    out.append(("M beyond what n_units make", bytes(t), "M = "))
    return out


def test_python_reader_refuses_malformed_files(tmp_path):
    a, _ = _archive_case((2, 4))
    good = BA().pack(**a)
    assert BA().unpack(good)["M"] == a["M"]
    for name, data, word in malformed(good):
        with pytest.raises(BA().ArchiveError) as e:
            BA().unpack(data)
        assert word in str(e.value), (name, str(e.value))
    with pytest.raises(BA().ArchiveError):
        BA().pack(**dict(a, payload=a["payload"][:-16]))
    with pytest.raises(BA().ArchiveError):
        BA().pack(**dict(a, kind=5))


@pytest.fixture(scope="module")
def brs_tool(tmp_path_factory):
    """csrc/cli/burst_archive.c in a stand-alone program (tests/cpp/brs_tool.cpp) under AddressSanitizer and UBSan."""
    d = tmp_path_factory.mktemp("brs_tool")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    inc = ["-I", os.path.join(ROOT, "include")]
    obj, exe = str(d / "burst_archive.o"), str(d / "brs_tool")
    for cmd in (["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "adsbdec_amd", "csrc", "cli", "burst_archive.c"), "-o", obj],
                ["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "brs_tool.cpp"), obj, "-o", exe]):
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=env)
        assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        return p
    return run


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for v in bytes(b):
        h = ((h ^ v) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("s_kind", KIND_S)
def test_python_writes_c_reads_and_back(tmp_path, brs_tool, s_kind):
    a, off = _archive_case(s_kind)
    src, dst = tmp_path / "py.brs", tmp_path / "c.brs"
    BA().write(src, **a)
    p = brs_tool("info", str(src))
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    tb = int(np.array([a["threshold"]], "<f4").view("<u4")[0])
    assert lines[0] == (f"kind {s_kind[0]} sample_bytes {s_kind[1]} n_units {a['n_units']} m {a['M']} threshold_bits 0x{tb:08x} lead 2 hang 4 "
                        f"n_bursts {a['bursts'].size} payload_bytes {a['payload'].size}")
    for i, (r, line) in enumerate(zip(a["bursts"], lines[1:])):
        pb = int(np.array([r["peak"]], "<f4").view("<u4")[0])
        assert line == f"burst {i} begin {r['begin']} end {r['end']} hot {r['hot']} peak_bits 0x{pb:08x} offset {int(off[i])}"
    assert lines[-1] == f"total {int(off[-1])} payload_fnv1a 0x{_fnv1a(a['payload']):016x} payload_aligned 1"
    # C reads and C writes: the same bytes; Python reads what C wrote
    p = brs_tool("copy", str(src), str(dst))
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == src.read_bytes()
    r = BA().read(dst)
    assert np.array_equal(r["payload"], a["payload"]) and np.array_equal(r["bursts"], a["bursts"])


def test_c_reader_refuses_malformed_files(capi, tmp_path, brs_tool):
    """The stand-alone program and the host program's -k, on every malformed file: a reason that names what is wrong, before any GPU
    call (-k: exit 255 and not a word about a device)."""
    a, _ = _archive_case((2, 4))
    good = BA().pack(**a)
    for i, (name, data, word) in enumerate(malformed(good)):
        path = tmp_path / f"bad{i}.brs"
        path.write_bytes(data)
        p = brs_tool("info", str(path))
        assert p.returncode == 1 and word in p.stderr and not p.stdout, (name, p.stderr)
        q = subprocess.run([capi.CLI_PATH, "-k", "-f", str(path)], capture_output=True, text=True, timeout=60)
        assert q.returncode == 255 and word in q.stderr and "adsb_create" not in q.stderr and not q.stdout, (name, q.stderr)
    p = brs_tool("info", str(tmp_path / "nothing.brs"))
    assert p.returncode == 1 and "cannot open" in p.stderr


def test_info_prints_the_header_and_the_kept_share(tmp_path):
    a, off = _archive_case((8, 2))
    BA().write(tmp_path / "a.brs", **a)
    p = subprocess.run([sys.executable, "-m", "adsbdec_amd.burst_archive", "info", str(tmp_path / "a.brs")], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    assert "int8 IQ (kind 8), 2 bytes per power sample" in p.stdout and f"{a['M']} power samples" in p.stdout
    assert "lead 2, hang 4" in p.stdout
    share = 100.0 * int(off[-1]) / (2 * a["M"])
    assert f"kept 4 bursts, {int(off[-1])} of {2 * a['M']} bytes ({share:.3f} %)" in p.stdout
    (tmp_path / "bad.brs").write_bytes(b"ADSBBRS9" + bytes(100))
    p = subprocess.run([sys.executable, "-m", "adsbdec_amd.burst_archive", "info", str(tmp_path / "bad.brs")], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 1 and "magic" in p.stderr and not p.stdout


def test_decode_wants_a_flush_handle():
    class Plain:
        flush = False
    a, _ = _archive_case((4, 4))
    with pytest.raises(BA().ArchiveError) as e:
        BA().decode(Plain(), BA().unpack(BA().pack(**a)))
    assert "flush" in str(e.value)


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_keep_and_archive_refusals_and_usage(capi, tmp_path):
    """-K without -L -U, or with -t, -p, -I, -G, -B or -W; -k with -t, -p, -q, -w, -E, -G, -B, -L, -W or -K: exit 1 with a message that
    names the letter, before any GPU call (the files do not even exist, and nothing is created)."""
    capi.load()
    for args in (["-K", "o.brs"], ["-L", "-K", "o.brs"], ["-U", "8", "-K", "o.brs"]):
        p = _cli(capi, tmp_path, *args, "-f", "nothing.bin")
        assert p.returncode == 1 and "-K is not supported without -L -U" in p.stderr and not p.stdout, (args, p.stderr)
    for extra, word in ((["-t", "3"], "-t"), (["-p"], "-p"), (["-I", "5"], "-I"), (["-G", "2"], "-G"), (["-B", "list.txt"], "-B"), (["-W", "o.pw"], "-W")):
        p = _cli(capi, tmp_path, "-L", "-U", "48,2,4", "-K", "o.brs", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-K is not supported with {word}: " in p.stderr and not p.stdout, (extra, p.stderr)
    for extra, word in ((["-t", "3"], "-t"), (["-p"], "-p"), (["-q", "2"], "-q"), (["-w"], "-w"), (["-E"], "-E"), (["-G", "2"], "-G"),
                        (["-B", "list.txt"], "-B"), (["-L"], "-L"), (["-W", "o.pw"], "-W"), (["-K", "o.brs"], "-K")):
        p = _cli(capi, tmp_path, "-k", *extra, "-f", "nothing.brs")
        assert p.returncode == 1 and f"-k is not supported with {word}: " in p.stderr and not p.stdout, (extra, p.stderr)
    assert not os.listdir(tmp_path)
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "-L -U factor[,lead[,hang]] -K out.brs -f filename" in u.stdout and "\t-K out.brs :" in u.stdout
    assert "-k -f in.brs" in u.stdout and "\t-k :" in u.stdout
    assert "-L -U factor[,lead[,hang]] -f filename" in u.stdout and "\t-U factor[,lead[,hang]] :" in u.stdout   # (what the burst tests pin stays)
    # well-formed lines get as far as the file
    p = _cli(capi, tmp_path, "-L", "-U", "48,2,4", "-K", "o.brs", "-q", "8", "-f", "nothing.bin")
    assert p.returncode == 255 and "nothing.bin" in p.stderr
    p = _cli(capi, tmp_path, "-k", "-a", "-m", "-x", "-f", "nothing.brs")
    assert p.returncode == 255 and "nothing.brs" in p.stderr and "cannot open" in p.stderr
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------ the pipeline fixture's condition
def test_pipeline_fixture_payload_is_under_one_percent():
    p = BC.pipeline()
    M = p["a"].size
    b = LV().bursts(p["env"], p["threshold"], 2, 4)
    assert b.size == BC.PIPE_FRAMES
    sl = LV().burst_samples(b, M)
    off = BA().layout(b, M, 4)
    kept = int((sl[:, 1] - sl[:, 0]).sum())
    assert kept < 0.01 * M, kept / M
    assert int(off[-1]) == int(((4 * (sl[:, 1] - sl[:, 0]) + 15) // 16 * 16).sum())
    assert 4 * kept <= int(off[-1]) < 4 * kept + 16 * b.size
    assert int(off[-1]) < 0.01 * p["x"].nbytes, int(off[-1]) / p["x"].nbytes
    out, _ = BA().gather(p["x"], b, M, 4)
    for (lo, hi), at in zip(sl, off[:-1]):
        assert np.array_equal(out[int(at):int(at) + 4 * int(hi - lo)].view("<i2").reshape(-1, 2), p["x"][lo:hi])
