"""Flush (adsb_set_flush; DESIGN.md "Flush") without a GPU: the definition's three claims on the oracle, the resolver's end-of-stream
rule and the batch layout of a flush handle through the host-only entry points, declarations and bindings, and the C host program's
-E refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import flush_cases as FC
from conftest import ROOT

RUN, GAP = 28, FC.WINDOW + FC.DECOFFSET


# ------------------------------------------------------------------ the definition, on the oracle
@pytest.mark.parametrize("kind", ["real", "iq"])
def test_definition_claims_on_the_oracle(oracle, kind):
    """200 seeded captures per kind: (1) silence of 43 400, 81 960 and 120 000 power samples gives ONE answer, records and Try/Ok;
    (2) no frame starts at or behind M - 32; (3) the non-flush frames stand unchanged at the front of the flush answer."""
    some_plain = some_cut = 0
    for x in FC.seeded_cached(kind):
        if kind == "real":
            M = 2 * (x.size // 4)
            answers = [FC.want_real(oracle, x, P=P) for P in FC.P_ALL]
            plain = FC.recs(oracle.decode(x, df18=True)[0])
        else:
            a = FC.iq_power(x)
            M = 2 * (a.size // 2)
            answers = [FC.want_power(oracle, a, P=P) for P in FC.P_ALL]
            plain = FC.recs(oracle.demod_power(a, df18=True)[0])
        assert answers[0] == answers[1] == answers[2], (kind, x.shape)
        got = answers[1][0]
        assert all(g < M - 32 for g, _, _, _ in got), (kind, M, got[-1:])
        assert got[:len(plain)] == plain, (kind, x.shape)
        some_plain += len(plain)
        some_cut += sum(g + (640 if len(fr) == 7 else 1200) > M for g, _, _, fr in got)
    assert some_plain > 20 and some_cut > 20      # (the long captures decode without flush too; frames do reach past M)
    if oracle.ref_available():                    # ... and where the reference's own code is built, it says the same of the twin
        x = FC.seeded_cached(kind)[19]
        if kind == "real":
            (fr, st), want = oracle.ref_decode(FC.twin_real(x), df18=True), FC.want_real(oracle, x)
        else:
            (fr, st), want = oracle.ref_demod(FC.twin_power(FC.iq_power(x)), df18=True), FC.want_power(oracle, FC.iq_power(x))
        assert [(f["ts"], f["pw"], f["frame"]) for f in fr] == [r[1:] for r in want[0]] and st == want[1]


# ------------------------------------------------------------------ the resolver's rule
def _resolve_flush(capi, oracle, a, df18=True):
    """oracle.scan_all's records of the offsets below M, fed to a resolver that ends the stream as a flush handle does."""
    M = 2 * (a.size // 2)
    tw = FC.twin_power(a)
    cands, tries = oracle.scan_all(tw, 0, M, df18)
    r = capi.Resolver()
    r.feed(cands, tries)
    r.finish_flush(M)
    got = FC.recs(r.drain()), r.stats()
    r.close()
    return got


@pytest.mark.parametrize("n", [2_048, 4_096, 40_978, 40_980, 40_982, 42_181, 81_960, 100_001])
@pytest.mark.parametrize("end", [-1, 0, 1, 5, 20])
def test_resolver_flush_rule(capi, oracle, n, end):
    """M below, at and just above the reference's buffer (40 980), and well above; a frame that ends `end` power samples behind M: with
    end 1 .. 5 it is accepted (its last bit is 1) and its jump carries the scan past M."""
    extra = [(s, 17) for s in range(300, n - 3000, 7_000)]
    x = FC.iq_capture(n, 50 + n % 97 + end, end=end, df=(17, 11)[end % 2], extra=extra)
    a = FC.iq_power(x)
    want = FC.want_power(oracle, a)
    assert _resolve_flush(capi, oracle, a) == want
    M = 2 * (n // 2)
    if end in (0, 1, 5):
        assert want[0] and want[0][-1][0] + (640 if len(want[0][-1][3]) == 7 else 1200) >= M, want[0][-1:]


def test_resolver_flush_rule_in_pieces(capi, oracle):
    """The same answer when the records arrive launch by launch with the reference's own calls in between (a stream's pushes)."""
    x = FC.iq_capture(120_000, 9, end=3, extra=[(s, (17, 11)[k % 2]) for k, s in enumerate(range(100, 117_000, 5_000))])
    a = FC.iq_power(x)
    M = a.size
    tw = FC.twin_power(a)
    r = capi.Resolver()
    cuts = [0, 28 * 700, 28 * 1500, 28 * 3000, M - FC.WINDOW + 1 - (M - FC.WINDOW + 1) % 28, M]
    for lo, hi in zip(cuts, cuts[1:]):
        c, t = oracle.scan_all(tw, lo, hi, True)
        r.feed(c, t)
        if hi != M:
            r.advance(hi + FC.WINDOW - 1 - (hi + FC.WINDOW - 1) % 2, hi)      # what a stream has produced once it has scanned to hi
    r.finish_flush(M)
    assert (FC.recs(r.drain()), r.stats()) == FC.want_power(oracle, a)


# ------------------------------------------------------------------ the batch layout
def _check_flush_layout(ns, segs, launches):
    by = {}
    for s in segs:
        by.setdefault(s["capture"], []).append(s)
    assert sorted(by) == list(range(len(ns)))
    prev_reach = None
    for i, n in enumerate(ns):
        M = 2 * (n // 4)
        parts = by[i]
        assert parts[0]["o_begin"] == 0 and parts[-1]["o_end"] == M, (i, n, parts)        # the segments cover [0, M)
        for a, b in zip(parts, parts[1:]):
            assert a["o_end"] == b["o_begin"] > a["o_begin"]
        for s in parts:
            assert s["base"] % RUN == 0
            if prev_reach is not None:
                assert s["base"] >= prev_reach + GAP, (i, s, prev_reach)                   # free offsets behind the neighbour's REACH
            span = s["o_end"] - s["o_begin"]
            prev_reach = s["base"] + span + (FC.WINDOW - 1 if span else 0)
            L = launches[s["launch"]]
            assert L["g_begin"] <= s["base"] and s["base"] + span <= max(L["g_end"], s["base"])
            assert s["tiles"] == -(-span // (RUN * (252 * L["passes"] - 44)))


@pytest.mark.parametrize("k", [1, 2, 300])
def test_batch_layout_with_flush(capi, k):
    rng = np.random.default_rng(k)
    ns = [int(v) for v in rng.integers(0, 30_001, size=k)]
    ns[0] = (0, 30_000, 3)[k % 3]
    for passes, limit in ((0, 0), (2, 0), (0, 28 * 1720), (2, 28 * 460)):
        segs, launches = capi.batch_layout(ns, passes=passes, launch_offsets=limit, flush=True)
        _check_flush_layout(ns, segs, launches)
        # without flush the layout is the parent's, byte for byte: the _ex entry point and the flush twin with flush = 0 agree, and
        # captures this short have no offsets at all there
        plain = capi.batch_layout(ns, passes=passes, launch_offsets=limit, flush=False)
        assert plain == _layout_ex(capi, ns, passes, limit)
        assert all(s["o_end"] == 0 for s in plain[0])


def _layout_ex(capi, ns, passes, limit):
    import ctypes as C
    L = capi.load()
    k = len(ns)
    n = (C.c_size_t * max(1, k))(*ns)
    nl = C.c_size_t(0)
    cnt = L.adsb_batch_layout_ex(k, n, 0, passes, limit, None, 0, None, 0, C.byref(nl))
    segs, launches = (capi.BatchSegment * max(1, cnt))(), (capi.BatchLaunch * max(1, nl.value))()
    assert L.adsb_batch_layout_ex(k, n, 0, passes, limit, segs, cnt, launches, nl.value, C.byref(nl)) == cnt
    return [capi._struct_dict(segs[i]) for i in range(cnt)], [capi._struct_dict(launches[i]) for i in range(nl.value)]


def test_parent_layout_unchanged_for_long_captures(capi):
    """Captures the reference does scan: the non-flush layout is what batch.hpp's rules give (m - 1195 offsets each), and the flush
    one differs only by the offsets up to M."""
    ns = [81_960, 200_001, 81_959, 123_456]
    plain, _ = capi.batch_layout(ns)
    assert [s["o_end"] for s in plain] == [2 * (n // 4) - 1195 if 2 * ((n + 3) // 4) >= 40_980 else 0 for n in ns]
    flush, launches = capi.batch_layout(ns, flush=True)
    _check_flush_layout(ns, flush, launches)


def test_batch_resolve_with_flush(capi, oracle):
    """adsb_batch_resolve_flush: records in the virtual offsets of the flush layout -> every capture's twin answer; the same
    records through the non-flush entry point are refused (they lie in no segment of that layout)."""
    caps = [FC.iq_capture(n, 70 + i, end=(0, 3, -1, 20, 1)[i % 5], df=(17, 11)[i % 2]) for i, n in enumerate((1500, 0, 2999, 700, 5000, 2048))]
    pw = [FC.iq_power(x) if len(x) else np.zeros(0, np.float32) for x in caps]
    ns = [4 * (a.size // 2) for a in pw]                       # the units the batch machinery counts for a power capture
    segs, _ = capi.batch_layout(ns, flush=True)
    cands, tries = [], []
    for s in segs:
        a = pw[s["capture"]]
        if s["o_end"] > s["o_begin"]:
            c, t = oracle.scan_all(FC.twin_power(a), s["o_begin"], s["o_end"], True)
            off = s["base"] - s["o_begin"]
            cands += [(g + off, p, fr) for g, p, fr in c]
            tries += [int(((int(w) >> 2) + off) << 2 | (int(w) & 3)) for w in t]
    frames, stats = capi.batch_resolve(ns, cands, np.array(tries, dtype=np.uint64), flush=True)
    for i, a in enumerate(pw):
        want = FC.want_power(oracle, a)
        assert (FC.recs(frames[i]), stats[i]) == want, i
    assert sum(len(f) for f in frames) >= 3
    with pytest.raises(capi.AdsbError):
        capi.batch_resolve(ns, cands, np.array(tries, dtype=np.uint64), flush=False)


# ------------------------------------------------------------------ declarations, bindings, refusals without a device
def test_entry_points_are_declared_exported_and_bound(capi):
    inc = os.path.join(ROOT, "include")
    strip = lambda h: re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
    main, diag = strip("adsbdec_amd.h"), strip("adsbdec_amd_diag.h")
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = capi.load()
    for name, header in (("adsb_set_flush", main), ("adsb_get_flush", main), ("adsb_resolver_finish_flush", diag),
                         ("adsb_batch_layout_flush", diag), ("adsb_batch_resolve_flush", diag)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\b%s\b" % name, exported) and name in capi.SYMBOLS and hasattr(L, name), name
    assert "adsb_multi_set_flush" not in main + diag                     # no multi-GPU setter: that driver keeps the horizon
    assert L.adsb_abi_version() == 5                                     # symbols were added, no struct changed
    assert L.adsb_set_flush(None, 1) == -1 and L.adsb_get_flush(None) == -1 and L.adsb_resolver_finish_flush(None, 0) == -1
    import inspect
    assert "flush" in inspect.signature(capi.Decoder.__init__).parameters
    assert hasattr(capi.Decoder, "set_flush") and isinstance(capi.Decoder.flush, property)
    assert "hang 4" in capi.Decoder.bursts.__doc__ and inspect.signature(capi.Decoder.bursts).parameters["hang"].default == 1468


def _cli(capi, tmp_path, *args):
    return subprocess.run([capi.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)


def test_cli_flush_refusals_and_usage(capi, tmp_path):
    """-E with -G, -L or -W: exit 1 with a message before any GPU call (the file does not exist, nothing is created); the usage text
    names -E and says that hang 4 is enough for pieces decoded with it; -e still only prints the usage text."""
    capi.load()
    for other, word in ((("-G", "2"), "-G"), (("-L",), "-L"), (("-W", "out.pw"), "-W"), (("-L", "-U", "8"), "-L")):
        p = _cli(capi, tmp_path, "-E", *other, "-f", "nothing.bin")
        assert p.returncode == 1 and f"-E is not supported with {word}: " in p.stderr and not p.stdout, (other, p.stderr)
    p = _cli(capi, tmp_path, "-E", "-G", "2", "-B", "nothing.txt")
    assert p.returncode == 1 and "-E is not supported with -G: " in p.stderr
    assert not os.listdir(tmp_path)
    p = _cli(capi, tmp_path, "-e")
    assert p.returncode == 1 and "\t-E : (extension) decode to the file's last sample" in p.stdout and "hang 4 is enough" in p.stdout
