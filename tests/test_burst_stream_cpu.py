"""The gate of a slice of a stream, and the record mode, without a GPU: the numpy statement (adsbdec_amd/levels.py bursts_slice) held to
levels.bursts -- the records of consecutive calls, concatenated, are the bursts of the concatenated envelope, however it is cut -- and,
where lead and hang change from call to call, to a slow paint-and-merge on the hot mask; the archive's statement
(burst_archive.record_statement) against the archive built in one piece; the declarations, the exports and the bindings; the host
program's -S / -O refusals, before any GPU call, and the -U / -K ones it had; and the C writer that takes the payload from a spool
file, in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import burst_cases as BC
from conftest import ROOT


def LV():
    from adsbdec_amd import levels
    return levels


def BA():
    from adsbdec_amd import burst_archive
    return burst_archive


THRESHOLDS = (0.0, 1.0e-40, 1.0, 2.5, float("inf"), 3.4028234663852886e38)       # as tests/test_bursts_cpu.py's
SPECIALS = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x80000000, 0, 1, 0x7F7FFFFF], dtype="<u4").view("<f4")


def random_envelope(rng, most=400):
    R = int(rng.integers(0, most + 1))
    env = rng.uniform(0.0, 4.0, R).astype("<f4")
    if R and rng.random() < 0.5:
        env[rng.random(R) < rng.choice([0.5, 0.9, 0.99])] = np.float32(0.5)       # sparse: clusters with room between them
    if R and rng.random() < 0.3:
        at = rng.integers(0, R, size=min(R, 6))
        env[at] = SPECIALS[rng.integers(0, SPECIALS.size, at.size)]
    return env


def through_slices(env, edges, threshold, lead, hang):
    """-> the concatenated records; the input carry of every call is left as it was."""
    carry, recs = LV().burst_carry(), []
    for i in range(len(edges) - 1):
        before = carry.copy()
        table, out = LV().bursts_slice(env[edges[i]:edges[i + 1]], threshold, lead, hang, carry, i == len(edges) - 2)
        assert carry.tobytes() == before.tobytes() and out is not carry                 # purity
        assert table.dtype == LV().BURST_DTYPE and out.dtype == LV().BURST_CARRY_DTYPE and out["runs"][0] == edges[i + 1]
        recs.append(table)
        carry = out
    assert not carry["open"][0]
    return np.concatenate(recs)


# ------------------------------------------------------------------ the statement
def test_slices_give_the_bursts_of_the_whole_on_random_cuts():
    rng = np.random.default_rng(3601)
    for i in range(3000):
        env = random_envelope(rng)
        R = env.size
        lead, hang = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        threshold = float(rng.choice(THRESHOLDS))
        k = int(rng.integers(1, 7))
        edges = [0, *sorted(int(v) for v in rng.integers(0, R + 1, k - 1)), R]           # (equal edges: empty slices)
        want = LV().bursts(env, threshold, lead, hang)
        got = through_slices(env, edges, threshold, lead, hang)
        assert got.tobytes() == want.tobytes(), (i, R, lead, hang, threshold, edges)


def test_every_two_slice_cut_of_fifty_envelopes():
    rng = np.random.default_rng(3602)
    for i in range(50):
        env = random_envelope(rng, most=160)
        lead, hang = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        threshold = float(rng.choice(THRESHOLDS[:4]))
        want = LV().bursts(env, threshold, lead, hang).tobytes()
        for cut in range(env.size + 1):
            assert through_slices(env, [0, cut, env.size], threshold, lead, hang).tobytes() == want, (i, cut, lead, hang)


def test_a_carry_is_32_bytes_and_bad_ones_are_refused():
    c = LV().burst_carry()
    assert c.shape == (1,) and c.dtype.itemsize == 32 and not c.tobytes().strip(b"\0")
    assert [c.dtype.fields[k][1] for k in ("runs", "open", "first", "last", "hot", "peak", "reserved")] == [0, 8, 12, 16, 20, 24, 28]
    env = np.zeros(4, "<f4")
    for bad in (dict(runs=10, open=1, first=5, last=4, hot=1), dict(runs=10, open=1, first=5, last=10, hot=1), dict(runs=10, open=1, first=5, last=6, hot=0)):
        for k, v in bad.items():
            c[k] = v
        with pytest.raises(ValueError):
            LV().bursts_slice(env, 1.0, 2, 4, c, False)
    c = LV().burst_carry()
    c["runs"] = (1 << 31) - 4
    with pytest.raises(ValueError):
        LV().bursts_slice(env, 1.0, 2, 4, c, False)
    table, out = LV().bursts_slice(env[:3], 0.0, 2, 4, c, True)                          # the last runs a stream may have
    assert out["runs"][0] == (1 << 31) - 1 and BC.as_tuples(table) == [((1 << 31) - 6, (1 << 31) - 1, 3, 0)]


def slow_changing(env, edges, threshold, leads, hangs):
    """lead and hang that change from call to call, slowly and in other words: walk the hot mask run by run; a cluster is the hot runs
    since the last cut, and it is cut -- at a hot run, or at the end of a call -- by the join of the call that is running then."""
    b = np.ascontiguousarray(env, dtype="<f4").view("<u4")
    u = [0 if int(v) >> 31 else int(v) for v in b]
    tb = int(np.array([threshold], dtype="<f4").view("<u4")[0])
    per_call, cluster = [], None                                                        # cluster: [first, last, hot, peak]
    for i in range(len(edges) - 1):
        lead, hang, final = leads[i], hangs[i], i == len(edges) - 2
        join, out = lead + hang + 1, []

        def close(c):
            out.append((max(0, c[0] - lead), min(edges[i + 1], c[1] + hang + 1), c[2], c[3]))
        for r in range(edges[i], edges[i + 1]):
            if u[r] < tb:
                continue
            if cluster and r - cluster[1] > join:
                close(cluster)
                cluster = None
            cluster = [r, r, 1, u[r]] if cluster is None else [cluster[0], r, cluster[2] + 1, max(cluster[3], u[r])]
        if cluster and (final or cluster[1] + join < edges[i + 1]):
            close(cluster)
            cluster = None
        per_call.append(out)
    return per_call


def test_lead_and_hang_that_change_between_calls():
    rng = np.random.default_rng(3603)
    for i in range(400):
        env = random_envelope(rng, most=200)
        R = env.size
        k = int(rng.integers(1, 7))
        edges = [0, *sorted(int(v) for v in rng.integers(0, R + 1, k - 1)), R]
        leads, hangs = [int(v) for v in rng.integers(0, 7, k)], [int(v) for v in rng.integers(0, 7, k)]
        threshold = float(rng.choice(THRESHOLDS[:4]))
        want = slow_changing(env, edges, threshold, leads, hangs)
        carry = LV().burst_carry()
        for j in range(k):
            table, carry = LV().bursts_slice(env[edges[j]:edges[j + 1]], threshold, leads[j], hangs[j], carry, j == k - 1)
            assert BC.as_tuples(table) == want[j], (i, j, edges, leads, hangs)


# ------------------------------------------------------------------ the archive's statement
def test_record_statement_is_the_archive_built_in_one_piece():
    rng = np.random.default_rng(3604)
    n = 56 * 500 + 3                                                                    # a trailing n % 4, and M = 28 R exactly
    x = rng.integers(0, 4096, n, dtype=np.uint16)
    M = 2 * (n // 4)
    R = -(-M // 28)
    a = rng.uniform(0.5, 2.0, M).astype("<f4")
    loud = np.flatnonzero(rng.random(R) < 0.03)
    a[28 * loud + rng.integers(0, 28, loud.size)] = np.float32(1000.0)
    a[:28] = np.float32(4.0)                                                            # the first run alone has another median
    for piece in (1, 7, 64, R):
        median = LV().percentile(LV().level_report(a[:28 * piece])["hist"], 0.5)
        threshold = float(np.float32(48.0 * median))
        table = LV().bursts(LV().level_report(a)["env"], threshold, 2, 4)
        payload, _ = BA().gather(x, table, M, 4)
        want = BA().pack(4, n, M, threshold, 2, 4, table, payload)
        got = BA().record_statement(x, piece, 48.0, 2, 4, a=a)
        assert got == want and BA().unpack(got)["bursts"].size == table.size, piece
        assert BA().record_statement(x, piece, threshold, 2, 4, a=a, absolute=True) == want, piece
    assert BA().unpack(BA().record_statement(x, 1, 48.0, 2, 4, a=a))["threshold"] == np.float32(48.0 * 4.0)
    assert 3 < BA().unpack(BA().record_statement(x, R, 48.0, 2, 4, a=a))["bursts"].size < R
    with pytest.raises(BA().ArchiveError):                                              # no sign-clear sample in the first piece
        BA().record_statement(x, 2, 48.0, 2, 4, a=np.concatenate([np.full(56, -1.0, "<f4"), a[56:]]))
    with pytest.raises(BA().ArchiveError):
        BA().record_statement(x, 2, 48.0, 2, 4, a=a[:-2])


# ------------------------------------------------------------------ interfaces
def test_slice_calls_are_declared_exported_and_bound(capi):
    from adsbdec_amd import _build
    text = open(os.path.join(ROOT, "include", "adsbdec_amd.h")).read()
    main = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (adsb_[a-z0-9_]+)", out))
    L = capi.load()
    for name in ("adsb_bursts_slice_device", "adsb_bursts_slice_host"):
        assert re.search(rf"\blong\s+{name}\s*\(", main), name
        assert name in exported and name in capi.SYMBOLS and hasattr(L, name), name
        assert len(capi.SYMBOLS[name][1]) == 11 and capi.SYMBOLS[name][0] is C.c_long, name
    assert ("typedef struct adsb_burst_carry { uint64_t runs; uint32_t open, first, last, hot; float peak; uint32_t reserved; } "
            "adsb_burst_carry;") in main
    assert "the caller joins" not in text
    for m in ("bursts_slice_device", "bursts_slice_host"):
        assert callable(getattr(capi.Decoder, m)), m
    c = capi.burst_carry()
    assert c.dtype == LV().BURST_CARRY_DTYPE and c.shape == (1,) and not c.tobytes().strip(b"\0")
    assert "burst_slice_kernel.hip" in _build.HIP_SOURCES and "record.c" in _build.CLI_SOURCES
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "burst_slice_kernel.hip.o" in mk and "record.c" in mk
    assert L.adsb_abi_version() == 5 and len(text.splitlines()) <= 250
    # NULL handle: -1, nothing touched
    tab, out = np.full(64, 0x5A, np.uint8), np.full(32, 0x5A, np.uint8)
    for fn in (L.adsb_bursts_slice_device, L.adsb_bursts_slice_host):
        assert fn(None, None, 0, 1.0, 0, 0, c.ctypes.data, 1, tab.ctypes.data, 4, out.ctypes.data) == -1
    assert (tab == 0x5A).all() and (out == 0x5A).all()


def test_the_slice_unit_has_three_kernels_without_scratch():
    """burst_slice_kernel.hip for gfx950: the capture unit's three kernels in their slice form, none with scratch."""
    from adsbdec_amd import _build
    src = os.path.join(ROOT, "adsbdec_amd", "csrc", "burst_slice_kernel.hip")
    isa = subprocess.run([_build.HIPCC] + _build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True,
                         check=True).stdout
    assert ".amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"" in isa
    sizes = dict(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", isa, flags=re.M))
    assert len(sizes) == 3 and all(int(v) == 0 for v in sizes.values()), sizes
    for k in ("burst_slice_summary_kernel", "burst_slice_combine_kernel", "burst_slice_emit_kernel"):
        assert any(k in name for name in sizes), (k, sorted(sizes))


# ------------------------------------------------------------------ the host program's refusals
def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_record_refusals_and_usage(capi, tmp_path):
    """-S with an option it cannot be meant with, -O without -S, a factor that is no finite number above 0 or a piece of 0: exit 1 with
    the option's name in the message, before any GPU call (the file does not even exist, and nothing is created)."""
    capi.load()
    clashes = (["-L"], ["-L", "-I", "1"], ["-L", "-U", "8"], ["-L", "-U", "8", "-K", "o.brs"], ["-L", "-U", "8", "-P", "o.brs"], ["-k"], ["-t", "3"], ["-p"],
               ["-q", "2"], ["-w"], ["-W", "o.pw"], ["-G", "2"], ["-B", "list.txt"], ["-E"], ["-x"], ["-m"], ["-b"])
    named = ("-L", "-L", "-L", "-L", "-L", "-k", "-t", "-p", "-q", "-w", "-W", "-G", "-B", "-E", "-x", "-m", "-b")
    for extra, word in zip(clashes, named):
        p = _cli(capi, tmp_path, "-S", "48,2,4", "-O", "out.brs", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-S is not supported with {word}: " in p.stderr and not p.stdout, (extra, p.stderr)
    for extra, word in ((["-I", "1"], "-I"), (["-U", "8"], "-U"), (["-K", "o.brs"], "-K"), (["-P", "o.brs"], "-P")):    # each alone, too
        p = _cli(capi, tmp_path, "-S", "48", *extra, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-S is not supported with {word}: " in p.stderr and not p.stdout, (extra, p.stderr)
    p = _cli(capi, tmp_path, "-O", "out.brs", "-f", "nothing.bin")
    assert p.returncode == 1 and "-O is not supported without -S" in p.stderr and not p.stdout, p.stderr
    p = _cli(capi, tmp_path, "-L", "-O", "out.brs", "-f", "nothing.bin")
    assert p.returncode == 1 and "-O is not supported without -S" in p.stderr and not p.stdout, p.stderr
    for bad in ("0", "-1", "abc", "nan", "inf", "1e999", "", "8,", "8,x", "8,-1", "8,1.5", "8,1,2,", "8,1,2,0", "8,1,2,3,4", "8,1073741825", "8,1,1073741825",
                "8,1,2,16777217", "@", "@0", "@-1", "@inf", "@nan", "@1e39"):
        p = _cli(capi, tmp_path, "-S", bad, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-S {bad}: " in p.stderr and "a finite factor above 0" in p.stderr and not p.stdout, (bad, p.stderr)
    assert not os.listdir(tmp_path)
    manual = open(os.path.join(ROOT, "adsbdec_amd", "csrc", "cli", "adsbdec_amd_cli.c")).read()
    assert " *     -S factor[,lead[,hang[,piece]]]  EXTENSION" in manual and " *     -O out.brs    EXTENSION, with -S" in manual
    # well-formed ones get as far as the file
    for good in ("48", "48,2,4", "48,0,1073741824,16777216", "@123.5,2,4,7"):
        p = _cli(capi, tmp_path, "-S", good, "-O", "out.brs", "-f", "nothing.bin")
        assert p.returncode == 255 and "nothing.bin" in p.stderr, (good, p.stderr)
    assert not os.listdir(tmp_path)
    # what -U and -K refused, they refuse
    p = _cli(capi, tmp_path, "-U", "8", "-f", "nothing.bin")
    assert p.returncode == 1 and "-U is not supported without -L" in p.stderr
    p = _cli(capi, tmp_path, "-L", "-I", "1", "-U", "8", "-f", "nothing.bin")
    assert p.returncode == 1 and "-U is not supported with -I: " in p.stderr
    p = _cli(capi, tmp_path, "-L", "-I", "1", "-U", "8", "-K", "o.brs", "-f", "nothing.bin")
    assert p.returncode == 1 and "-K is not supported with -I: " in p.stderr
    p = _cli(capi, tmp_path, "-K", "o.brs", "-f", "nothing.bin")
    assert p.returncode == 1 and "-K is not supported without -L -U" in p.stderr


# ------------------------------------------------------------------ the recorder's archive writer
def test_c_writer_takes_the_payload_from_a_spool_file(tmp_path):
    """csrc/cli/burst_archive.c brs_write_spooled in a stand-alone program (tests/cpp/brs_spool_tool.cpp) under AddressSanitizer and
    UBSan: header, table and a payload appended to a spool file in pieces are burst_archive.py's bytes; no spool file is left."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    inc = ["-I", os.path.join(ROOT, "include")]
    obj, exe = str(tmp_path / "burst_archive.o"), str(tmp_path / "brs_spool_tool")
    for cmd in (["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "adsbdec_amd", "csrc", "cli", "burst_archive.c"), "-o", obj],
                ["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "cpp", "brs_spool_tool.cpp"), obj, "-o", exe]):
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
    rng = np.random.default_rng(3605)
    n = 56 * 3000 + 2
    x = rng.integers(0, 4096, n, dtype=np.uint16)
    M = 2 * (n // 4)
    a = rng.uniform(0.5, 2.0, M).astype("<f4")
    a[28 * np.flatnonzero(rng.random(-(-M // 28)) < 0.02)] = np.float32(1000.0)
    a[-1] = np.float32(1000.0)                                                          # the last burst is clipped by M
    cases = {"bursts": BA().record_statement(x, 64, 48.0, 2, 4, a=a), "none": BA().record_statement(x, 64, 1.0e9, 2, 4, a=a, absolute=True)}
    assert BA().unpack(cases["bursts"])["bursts"].size > 10 and BA().unpack(cases["none"])["bursts"].size == 0
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for name, data in cases.items():
        for chunk in (16, 4096, 1 << 20):
            src, dst = tmp_path / f"{name}.py.brs", tmp_path / f"{name}.{chunk}.brs"
            src.write_bytes(data)
            p = subprocess.run([exe, str(src), str(dst), str(chunk)], capture_output=True, text=True, timeout=60, env=env)
            assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
            assert p.returncode == 0, p.stderr
            assert dst.read_bytes() == data, (name, chunk)
            assert not os.path.exists(str(dst) + ".spool") and not os.path.exists(str(dst) + ".tmp")
