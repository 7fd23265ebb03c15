"""The 12-bit burst gather and the kind-12 burst archive without a GPU: the numpy statement (adsbdec_amd/burst_archive.py layout12,
gather12) against a literal loop over pieces, groups and bits; pack12_group (csrc/packed12.h) against unpack12_group, the definition
and the known answers, in a stand-alone program under AddressSanitizer and UBSan; adsb_gather_pack12_layout against the statement,
and each of its refusals naming the record; the claim the fill rests on -- a capture with n % 8 == 4 decodes, on the oracle, as the
same capture with four codes 2048 appended; the archive written and read back, in Python and through the C reader and writer in the
existing stand-alone program under the sanitizers; every malformed kind-12 file refused by both readers; -P's refusals and usage,
before any GPU call; the declarations, exports and bindings; the kernel unit's code object by its directives."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import flush_cases as FC
import gather_cases as GC
import gather_pack12_cases as PC
from conftest import ROOT
from test_gather_cpu import brs_tool, malformed, _fnv1a  # noqa: F401  (the existing stand-alone program, its build and its cases)

KIND = 12


def BA():
    from adsbdec_amd import burst_archive
    return burst_archive


def LV():
    from adsbdec_amd import levels
    return levels


# ------------------------------------------------------------------ the statement
def test_statement_against_the_literal_loop():
    """Every named shape at every M of the grid, captures with trailing samples and with codes above 4095 inside and outside."""
    for C_ in (4, 7):
        for M in PC.m_values(runs=60):
            for name, M_, tab in PC.named_cases(C_, M):
                x = PC.codes(PC.n_for(M, tail=M % 3), 41 + C_, top=4200)
                out, off, over = BA().gather12(x, tab, M)
                want, woff, wover = PC.slow_gather12(x, tab, M)
                assert off.dtype == np.uint64 and off.tolist() == woff, (M, name)
                assert BA().layout12(tab, M).tolist() == woff, (M, name)
                assert out.dtype == np.uint8 and out.tolist() == want and over == wover, (M, name)
    for i, (M, tab) in enumerate(PC.random_tables(60, 4201)):
        x = PC.codes(PC.n_for(M, tail=i % 4), i)
        out, off, over = BA().gather12(x, tab, M)
        want, woff, wover = PC.slow_gather12(x, tab, M)
        assert off.tolist() == woff and out.tolist() == want and over == wover == 0, (i, M)


def test_layout12_properties_and_over():
    """A piece starts at a multiple of 16, is 12 bytes per group of 8 samples -- 84 per run --, its samples start at a multiple of 8;
    only a last piece that M clips at M % 4 == 2 has a fill, of exactly four codes 2048; the pad is zero; the packed pieces unpack to
    the capture's samples & 0x0fff; over counts the pieces' own samples above 4095 and nothing else."""
    from adsbdec_amd import packed12
    for M in PC.m_values():
        for name, M_, tab in PC.named_cases(256, M):
            x = PC.codes(PC.n_for(M, tail=3), 43, top=4096)
            loud = x.copy()
            loud[::37] |= 0x1000                                # above 4095, inside and outside the pieces, the trailing samples too
            out, off, over = BA().gather12(loud, tab, M)
            clean, off2, over0 = BA().gather12(x, tab, M)
            assert np.array_equal(off, off2) and over0 == 0 and np.array_equal(out, clean), (M, name)   # the low 12 bits are what is stored
            sl = LV().burst_samples(tab, M)
            assert over == sum(int(np.count_nonzero(loud[2 * lo:2 * hi] > 4095)) for lo, hi in sl), (M, name)
            assert off[0] == 0 and (off % 16 == 0).all()
            keep = np.zeros(out.size, bool)
            for i, ((lo, hi), at) in enumerate(zip(sl, off[:-1])):
                lo, hi, at = int(lo), int(hi), int(at)
                assert (2 * lo) % 8 == 0
                groups = -(-(hi - lo) // 4)
                assert (hi - lo) % 28 or 12 * groups == 84 * ((hi - lo) // 28)
                fill = 8 * groups - 2 * (hi - lo)
                assert fill in (0, 4) and (fill == 0 or (i == tab.size - 1 and hi == M and M % 4 == 2)), (M, name, i)
                got = packed12.unpack12(out[at:at + 12 * groups])
                assert np.array_equal(got[:2 * (hi - lo)], x[2 * lo:2 * hi] & 0x0FFF) and (got[2 * (hi - lo):] == 2048).all()
                assert int(off[i + 1]) == (at + 12 * groups + 15) // 16 * 16
                keep[at:at + 12 * groups] = True
            assert (out[~keep] == 0).all()
    with pytest.raises(BA().ArchiveError):
        BA().gather12(np.zeros(10, np.uint16), GC.table([(0, 1)]), 28)          # a capture shorter than 2 M samples


# ------------------------------------------------------------------ pack12_group
def test_pack12_group_is_the_inverse_of_unpack12_group(tmp_path):
    exe = tmp_path / "pack12_group"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "pack12_group.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "3 known answers, 32768 groups, 200000 random words" in p.stdout and "runtime error" not in p.stderr


# ------------------------------------------------------------------ adsb_gather_pack12_layout
def test_c_layout_is_the_statements(capi):
    cases = [(M_, tab) for C_ in (4, 256) for M in PC.m_values() for _, M_, tab in PC.named_cases(C_, M)] + PC.random_tables(100, 4203)
    cases += GC.random_tables(40, 4204)                          # odd M too: the layout takes any m
    for M, tab in cases:
        want = BA().layout12(tab, M)
        got = capi.gather_pack12_layout(tab, M)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (M, tab.size)
    L = capi.load()
    M, tab = cases[5]
    total = C.c_uint64(0)
    assert L.adsb_gather_pack12_layout(M, tab.ctypes.data, tab.size, None, C.byref(total)) == 0 and total.value == int(BA().layout12(tab, M)[-1])
    off = np.zeros(tab.size + 1, np.uint64)
    assert L.adsb_gather_pack12_layout(M, tab.ctypes.data, tab.size, off.ctypes.data, None) == 0 and np.array_equal(off, BA().layout12(tab, M))
    assert L.adsb_gather_pack12_layout(0, None, 0, off.ctypes.data, C.byref(total)) == 0 and total.value == 0 and off[0] == 0
    # three quarters of the uint16 layout where every piece is whole runs
    tab = GC.table([(0, 4), (8, 12), (16, 32)])
    assert int(capi.gather_pack12_layout(tab, 28 * 40)[-1]) * 4 == int(capi.gather_layout(tab, 28 * 40, 4)[-1]) * 3
    # no 32-bit product anywhere: a piece beyond 2^32 bytes
    big = GC.table([(0, 1), ((1 << 31) - 40, (1 << 31) - 1)])
    assert np.array_equal(capi.gather_pack12_layout(big, 28 << 31), BA().layout12(big, 28 << 31))
    assert int(BA().layout12(big, 28 << 31)[-1]) == 96 + 84 * 39 + 4


def test_layout_refusals_name_the_record(capi):
    L = capi.load()
    for name, M, tab, word in PC.refusals():
        with pytest.raises(BA().ArchiveError) as e:
            BA().layout12(tab, M)
        assert word in str(e.value), (name, str(e.value))
        off = np.full(tab.size + 1, 0x5A5A5A5A, np.uint64)
        total = C.c_uint64(77)
        assert L.adsb_gather_pack12_layout(M, tab.ctypes.data, tab.size, off.ctypes.data, C.byref(total)) == -1, name
        msg = L.adsb_last_error(None).decode()
        assert msg.startswith("adsb_gather_pack12_layout: ") and word in msg, (name, msg)
        assert (off == 0x5A5A5A5A).all() and total.value == 77, name                  # a refusal writes nothing
        with pytest.raises(capi.AdsbError) as e:
            capi.gather_pack12_layout(tab, M)
        assert word in str(e.value)
    assert len(PC.refusals()) == 8
    assert L.adsb_gather_pack12_layout(100, None, 3, None, None) == -1 and "NULL table" in L.adsb_last_error(None).decode()


# ------------------------------------------------------------------ why four codes of fill change nothing
def test_four_codes_of_silence_change_nothing_on_the_oracle(oracle):
    """A capture of n samples, n % 8 == 4, on a flush handle decodes as its silent twin; so does the capture with four codes 2048
    appended, whose twin is the first one's with two more power samples of silence.  Equal records, equal Try/Ok tables."""
    seen = 0
    rng = np.random.default_rng(1204)
    for i in range(24):
        n = int(rng.integers(1_300, 6_000)) // 8 * 8 + 4
        x = FC.real_capture(n, 3000 + i, FC.ENDS[i % len(FC.ENDS)], (17, 11, 18)[i % 3])
        assert x.size % 8 == 4
        a, sa = FC.want_real(oracle, x)
        b, sb = FC.want_real(oracle, np.concatenate([x, np.full(4, 2048, np.uint16)]))
        assert a == b and sa == sb, (i, n)
        seen += len(a)
    for i, n in enumerate((90_004, 101_236)):                     # long ones, with frames in front of the end too
        M = 2 * (n // 4)
        x = FC.real_capture(n, 3100 + i, FC.ENDS[i], 17, extra=[(int(s), (17, 11)[k % 2]) for k, s in enumerate(range(500, M - 3000, 9_000))])
        a, sa = FC.want_real(oracle, x)
        b, sb = FC.want_real(oracle, np.concatenate([x, np.full(4, 2048, np.uint16)]))
        assert a == b and sa == sb and len(a) >= 5, (i, n)
        seen += len(a)
    assert seen >= 20                                            # (the claim is about captures that decode something)


# ------------------------------------------------------------------ the archive
def _archive_case(M=28 * 37 + 14, tail=3):
    tab = GC.table([(1, 2), (4, 9), (11, 12), (30, 38)])
    x = PC.codes(PC.n_for(M, tail), 62)
    payload, off, over = BA().gather12(x, tab, M)
    assert over == 0
    return dict(kind=KIND, n_units=x.size, M=M, threshold=123.456, lead=2, hang=4, bursts=tab, payload=payload), off, x


@pytest.mark.parametrize("M", (28 * 37 + 14, 28 * 37 + 16, 28 * 38))
def test_archive_write_read_is_the_identity(tmp_path, M):
    a, off, x = _archive_case(M)
    assert BA().BRS_KIND_PACKED12_REAL == KIND and BA().SAMPLE_BYTES[KIND] == 3 and BA().UNITS_PER_POWER_SAMPLE[KIND] == 2
    path = tmp_path / "a.brs"
    size = BA().write(path, **a)
    assert size == os.path.getsize(path) == 64 + 16 * a["bursts"].size + a["payload"].size
    data = path.read_bytes()
    assert data[:8] == b"ADSBBRS1" and struct.unpack_from("<III", data, 8) == (1, KIND, 3)          # version 1 stays
    assert struct.unpack_from("<QQ", data, 20) == (x.size, M)
    r = BA().read(path)
    assert (r["kind"], r["sample_bytes"], r["n_units"], r["M"], r["lead"], r["hang"]) == (KIND, 3, x.size, M, 2, 4)
    assert np.array_equal(r["bursts"], a["bursts"]) and np.array_equal(r["payload"], a["payload"]) and np.array_equal(r["offsets"], off)
    assert BA().pack(**{k: r[k] for k in a}) == data
    sl = LV().burst_samples(a["bursts"], M)
    assert BA().piece_units(r) == [8 * -(-int(hi - lo) // 4) for lo, hi in sl]
    assert "packed 12-bit real (kind 12), 3 bytes per power sample" in BA().info(r)
    # 3 bytes per power sample where the uint16 archive has 4 (before each piece is padded to a multiple of 16)
    assert sum(n // 8 * 12 for n in BA().piece_units(r)) * 4 == sum(4 * -(-int(hi - lo) // 4) * 4 for lo, hi in sl) * 3
    assert a["payload"].size < int(BA().layout(a["bursts"], M, 4)[-1])
    BA().write(tmp_path / "e.brs", KIND, 100, 40, 1.0, 2, 4, GC.table([]), np.zeros(0, np.uint8))
    e = BA().read(tmp_path / "e.brs")
    assert e["bursts"].size == 0 and e["payload"].size == 0 and os.path.getsize(tmp_path / "e.brs") == 64


def malformed12(good: bytes):
    """test_gather_cpu's list on a kind-12 file, and the pairs that only kind 12 can get wrong."""
    out = [m for m in malformed(good) if m[0] != "sample_bytes that do not go with the kind"]
    out.append(("kind 12 with sample_bytes 4", good[:16] + struct.pack("<I", 4) + good[20:], "sample_bytes"))
    out.append(("kind 12 with sample_bytes 2", good[:16] + struct.pack("<I", 2) + good[20:], "sample_bytes"))
    out.append(("kind 4 with sample_bytes 3", good[:12] + struct.pack("<I", 4) + good[16:], "sample_bytes"))
    out.append(("kind 4 with the 12-bit payload", good[:12] + struct.pack("<II", 4, 4) + good[20:], "payload"))
    return out


def test_python_reader_refuses_malformed_files():
    a, _, _ = _archive_case()
    good = BA().pack(**a)
    assert BA().unpack(good)["M"] == a["M"]
    cases = malformed12(good)
    assert len(cases) == 16
    for name, data, word in cases:
        with pytest.raises(BA().ArchiveError) as e:
            BA().unpack(data)
        assert word in str(e.value), (name, str(e.value))
    with pytest.raises(BA().ArchiveError):
        BA().pack(**dict(a, payload=a["payload"][:-16]))
    b, _, _ = _archive_case()
    with pytest.raises(BA().ArchiveError):                       # the uint16 payload of the table is not the 12-bit one
        BA().pack(**dict(b, payload=np.zeros(int(BA().layout(b["bursts"], b["M"], 4)[-1]), np.uint8)))


@pytest.mark.parametrize("M", (28 * 37 + 14, 28 * 37 + 16))
def test_python_writes_c_reads_and_back(tmp_path, brs_tool, M):  # noqa: F811
    a, off, _ = _archive_case(M)
    src, dst = tmp_path / "py.brs", tmp_path / "c.brs"
    BA().write(src, **a)
    p = brs_tool("info", str(src))
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert lines[0].startswith(f"kind 12 sample_bytes 3 n_units {a['n_units']} m {M} ") and lines[0].endswith(
        f"lead 2 hang 4 n_bursts {a['bursts'].size} payload_bytes {a['payload'].size}")
    for i, (r, line) in enumerate(zip(a["bursts"], lines[1:])):
        assert line.startswith(f"burst {i} begin {r['begin']} end {r['end']} ") and line.endswith(f" offset {int(off[i])}")
    assert lines[-1] == f"total {int(off[-1])} payload_fnv1a 0x{_fnv1a(a['payload']):016x} payload_aligned 1"
    p = brs_tool("copy", str(src), str(dst))
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == src.read_bytes()
    r = BA().read(dst)
    assert r["kind"] == KIND and np.array_equal(r["payload"], a["payload"]) and np.array_equal(r["bursts"], a["bursts"])


def test_c_reader_refuses_malformed_files(capi, tmp_path, brs_tool):  # noqa: F811
    """The stand-alone program and the host program's -k, on every malformed kind-12 file: a reason that names what is wrong, before
    any GPU call (-k: exit 255 and not a word about a device)."""
    a, _, _ = _archive_case()
    good = BA().pack(**a)
    for i, (name, data, word) in enumerate(malformed12(good)):
        path = tmp_path / f"bad{i}.brs"
        path.write_bytes(data)
        p = brs_tool("info", str(path))
        assert p.returncode == 1 and word in p.stderr and not p.stdout, (name, p.stderr)
        q = subprocess.run([capi.CLI_PATH, "-k", "-f", str(path)], capture_output=True, text=True, timeout=60)
        assert q.returncode == 255 and word in q.stderr and "adsb_create" not in q.stderr and not q.stdout, (name, q.stderr)


def test_decode_sends_kind_12_through_one_packed_batch_call():
    """burst_archive.decode on a kind-12 archive: ONE decode_batch_packed call, the pieces as bytes of whole groups where they lie in
    the payload, g and ts rebased by 28 begin."""
    a, off, _ = _archive_case()
    arch = BA().unpack(BA().pack(**a))

    class Fake:
        flush = True
        calls = []

        def decode_batch_packed(self, bufs, stats=False):
            self.calls.append([np.array(b) for b in bufs])
            st = {"try": {11: 1, 17: 2, 18: 0}, "ok": {11: 0, 17: 1, 18: 0}}
            return [[dict(g=5 + i, ts=7 + i, pw=1, frame=b"x")] for i in range(len(bufs))], [st] * len(bufs)

    fake = Fake()
    frames, stats = BA().decode(fake, arch)
    assert len(fake.calls) == 1 and len(fake.calls[0]) == 4
    units = BA().piece_units(arch)
    for buf, o, n in zip(fake.calls[0], off[:-1], units):
        assert buf.dtype == np.uint8 and buf.size == n // 8 * 12 and np.array_equal(buf, a["payload"][int(o):int(o) + buf.size])
    assert [(f["g"], f["ts"]) for f in frames] == [(5 + i + 28 * int(r["begin"]), 7 + i + 28 * int(r["begin"])) for i, r in enumerate(a["bursts"])]
    assert stats["try"] == {11: 4, 17: 8, 18: 0} and stats["ok"] == {11: 0, 17: 4, 18: 0}


# ------------------------------------------------------------------ the C host program
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_pack_refusals_and_usage(capi, tmp_path):
    """-P without -L -U, or with -q, -w, -K, -I, -G, -B, -W or -k: exit 1 with a message that names the letter, before any GPU call
    (the files do not even exist, and nothing is created).  -p and -t are taken."""
    capi.load()
    for args in (["-P", "o.brs"], ["-L", "-P", "o.brs"], ["-U", "8", "-P", "o.brs"]):
        p = _cli(capi, tmp_path, *args, "-f", "nothing.bin")
        assert p.returncode == 1 and "-P is not supported without -L -U" in p.stderr and not p.stdout, (args, p.stderr)
    for extra, word in ((["-q", "2"], "-q"), (["-w"], "-w"), (["-K", "k.brs"], "-K"), (["-I", "5"], "-I"), (["-G", "2"], "-G"),
                        (["-B", "list.txt"], "-B"), (["-W", "o.pw"], "-W"), (["-k"], "-k")):
        p = _cli(capi, tmp_path, "-L", "-U", "48,2,4", "-P", "o.brs", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-P is not supported with {word}: " in p.stderr and not p.stdout, (extra, p.stderr)
    assert not os.listdir(tmp_path)
    u = _cli(capi, tmp_path, "-e")
    assert u.returncode == 1 and "[-p | -t type] [-d gpu] -L -U factor[,lead[,hang]] -P out.brs -f filename" in u.stdout
    assert "\t-P out.brs :" in u.stdout and "\t-K out.brs :" in u.stdout and "\t-k :" in u.stdout
    # well-formed lines get as far as the file: a uint16 file, -p, -t 3 and -t 1
    for extra in ([], ["-p"], ["-t", "3"], ["-t", "1"]):
        p = _cli(capi, tmp_path, "-L", "-U", "48,2,4", "-P", "o.brs", *extra, "-f", "nothing.bin")
        assert p.returncode == 255 and "nothing.bin" in p.stderr, (extra, p.stderr)
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------ interface and build
def test_entry_points_are_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    text = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    main = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name, n_args in (("adsb_gather_pack12_layout", 5), ("adsb_gather_pack12_device", 9), ("adsb_gather_pack12_device_as", 10),
                         ("adsb_gather_pack12_device_packed", 9)):
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == n_args and capi.SYMBOLS[name][0] is C.c_long, name
    for name in ("gather_pack12_device", "gather_pack12_device_as", "gather_pack12_device_packed"):
        assert callable(getattr(capi.Decoder, name)), name
    assert callable(capi.gather_pack12_layout)
    assert "gather_pack12_kernel.hip" in _build.HIP_SOURCES and "decoder_gather_pack12.hip" in _build.HIP_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "gather_pack12_kernel.hip.o" in mk and "decoder_gather_pack12.hip.o" in mk
    assert L.adsb_abi_version() == 5                                                        # only symbols were added
    # NULL handle: -1, nothing touched
    off = np.full(4, 0x5A, np.uint64)
    over = C.c_uint64(0x5A)
    assert L.adsb_gather_pack12_device(None, None, 0, None, 0, None, 0, off.ctypes.data, C.byref(over)) == -1
    assert L.adsb_gather_pack12_device_as(None, 3, None, 0, None, 0, None, 0, off.ctypes.data, C.byref(over)) == -1
    assert L.adsb_gather_pack12_device_packed(None, None, 0, None, 0, None, 0, off.ctypes.data, C.byref(over)) == -1
    assert (off == 0x5A).all() and over.value == 0x5A
    for name in ("layout12", "gather12"):
        assert callable(getattr(BA(), name)), name
    hdr = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "cli", "burst_archive.h")).read()
    assert re.search(r"BRS_KIND_PACKED12_REAL\s*=\s*12\b", hdr)


def test_the_pack12_gather_is_one_kernel_without_scratch_or_lds():
    """The unit's code object, by its directives alone: gfx950 only, ONE kernel, no scratch and no LDS."""
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "gather_pack12_kernel.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True,
                         check=True).stdout
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 1 and all("gather_pack12_kernel" in k and int(v) == 0 for k, v in sizes.items()), sizes
    assert set(re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", isa)) == {"0"}
