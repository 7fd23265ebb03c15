"""Did a change move what the capture calls answer?  The library of a git revision and the working tree's, each loaded (ADSB_LIB_PATH) in
a fresh process of its own, one after the other, run the same deterministic list of calls over every capture call that takes a sample
flavour -- the single and batch exports, level calls and decodes, the 12-bit gather -- and record after every call: the return value,
adsb_last_error (every printed pointer as its value modulo 256), a digest of every output array (device and host, filled with a
sentinel before the call), adsb_get_format_report; and after the last call on a handle the frames of one small plain decode.

    python tools/abi_identity.py [revision]                  # on a GPU: both records, compared; exit status 1 on any difference
    python tools/abi_identity.py [revision] --build-only     # the revision's library into adsbdec_amd/lib_ab/parent/ (git-ignored)
    python tools/abi_identity.py [revision] --write-golden   # ... and tests/golden/flavour/flavour_answers.json from the REVISION's record alone
    python tools/abi_identity.py --list                      # the rows, no GPU needed
    python tools/abi_identity.py ... --summary=FILE          # the summary to FILE as well

The default revision is the parent commit -- HEAD while the tree has uncommitted changes, else HEAD~1 -- checked out into a
temporary git worktree and built there, unless adsbdec_amd/lib_ab/parent/ holds a library whose REVISION stamp names that revision (a
machine without the history runs what another one has built and stamped; a library without a stamp is refused).  Each process runs under `timeout`; the second is not started where the first does not
exit with status 0.  tests/test_gpu_flavour_answers.py replays rows() against the recording.

The rows.  Refusals: every refusal of a call alone, every two that stand next to each other in the call's order together (the first of
the two is the one reported), for batch calls with the offending capture first and last of three, and the earlier check on the last
capture against the later one on the first -- for the _host entry points too, where no alignment is asked and captures at odd
addresses are answered.  Format numbers: every fmt of -1 .. 9 through every _as and _iq call.  Answers: real
captures of 0, 3, 4, 8, 30 and 64 samples, IQ and power captures of 0, 1, 28 and 29, alone and as one batch, with a rail code, a code
above 4095, inexact and clamped samples planted; one capture of the IQ and power batch decodes 4- but not 16-byte aligned; a level batch
of kLevelBatchCaptures + 1 captures; a batch decode of a capture with frames.  Every pointer a row passes lies inside a live
allocation that holds what the call would read or write if no refusal fired.  So NOT in the grid, and listed as such by the summary:
  - a NULL device pointer where samples are due ("NULL buffer", "NULL samples", "NULL capture / output with n bursts"),
  - 2^31 / 2^32 samples or more in one capture, 2^32 - 1 bursts, more than 2^32 captures,
  - a failed allocation, and the `internal:` refusals, which no argument reaches."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_DIR = os.path.join(ROOT, "adsbdec_amd", "lib_ab", "parent")
PARENT_LIB = os.path.join(PARENT_DIR, "libadsbdec_amd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "flavour", "flavour_answers.json")   # (a directory of its own: every *.json directly under golden/ is a decode fixture)
LIMIT_S = 300
SENT = 0xA5
UNITS = ["decoder_export.hip", "decoder_export_batch.hip", "decoder_level.hip", "decoder_level_batch.hip", "decoder_gather_pack12.hip",
         "decoder_batch.hip", "decoder_stage.hip", "decoder_flavour.hip", "decoder.hip"]
# refusals of the units above that no row reaches: (a piece of the sentence, why)
NOT_IN_THE_GRID = [
    ("NULL buffer", "a NULL device pointer"), ("NULL samples", "a NULL device pointer"), ("NULL capture with", "a NULL device pointer"),
    ("NULL output with", "a NULL device pointer"), ("2^32 or more", "2^32 samples"), ("2^31 or more", "2^31 samples"),
    ("reaches 2^32", "2^32 samples / bursts"), ("would reach 2^31", "2^31 samples"), ("indexes its rows in 32 bits", "2^32 captures"),
    ("cannot allocate", "a failed allocation"), ("out of host memory", "a failed allocation"), ("internal: ", "no argument reaches it")]
# ... and the sentences of calls that take no flavour (the stream pushes, the window exports, the diagnostics beside the batch calls)
OUT_OF_SCOPE = ["buffer must start at a multiple of 8", "m_begin must be", "lies below m_begin", "does not hold the own pair", "the window has",
                "adsb_batch_unpacked_copy", "adsb_debug_set_level_batch_blocks"]

REAL_N, TWOS_N = (0, 3, 4, 8, 30, 64), (0, 1, 28, 29)
REGION = {"u16": 0, "as1": 1024, "as3": 2048, "packed": 3072, "iq2": 4096, "iq0": 5120, "iq8": 6144, "power": 7168}
ELEM = {"u16": 2, "as1": 4, "as3": 2, "packed": 1.5, "iq2": 4, "iq0": 8, "iq8": 2, "power": 4}
BIG_AT, BIG_N = {"u16": 16384, "as3": 16384 + 32768, "packed": 16384 + 65536}, 1 << 14
IN_BYTES, OUT_BYTES, ENV_AT, STRIDE = 128 << 10, 64 << 10, 32 << 10, 64
FAMILY = {"u16": "", "as1": "_as", "as3": "_as", "packed": "_packed", "iq0": "_iq", "iq2": "_iq", "iq8": "_iq", "power": "_power"}
FMT = {"as1": 1, "as3": 3, "iq0": 0, "iq2": 2, "iq8": 8}
ALIGN = {"u16": 16, "as1": 4, "as3": 2, "packed": 4, "iq0": 4, "iq2": 4, "iq8": 2, "power": 4}


def is_real(fl):
    return fl in ("u16", "as1", "as3", "packed")


def count(fl, n):
    return 2 * (n // 4) if is_real(fl) else n


def sizes(fl):
    return tuple(n for n in REAL_N if fl != "packed" or n % 8 == 0) if is_real(fl) else TWOS_N


def input_bytes():
    """The one input arena: a region per flavour, a capture with frames behind them as uint16, int16 and packed."""
    import numpy as np

    from adsbdec_amd.packed12 import pack12
    from tools import gen_signal as G
    rs = np.random.RandomState(35)
    a = rs.randint(0, 256, IN_BYTES).astype(np.uint8)

    def put(at, x):
        b = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        a[at:at + b.size] = b
    u16 = rs.randint(0, 4096, 512).astype("<u2")
    u16[[5, 29, 61]], u16[[6, 30]], u16[[7, 31]] = 4095, 0, 5000   # rail codes and codes above 4095, among the trailing n % 4 too
    put(REGION["u16"], u16)
    f = ((rs.randint(0, 4096, 256) - 2048) / 2048.0).astype("<f4")
    f[3], f[9], f[40] = 5.0, 0.3, float("nan")
    put(REGION["as1"], f)
    i16 = ((rs.randint(0, 4096, 512) - 2048) << 4).astype("<i2")
    i16[[2, 33]] += 3
    put(REGION["as3"], i16)
    put(REGION["iq2"], rs.randint(-2000, 2000, 512).astype("<i2"))
    q = (rs.randint(-2000, 2000, 256) / 32768.0).astype("<f4")
    q[4], q[11] = 3.0, 1e-7
    put(REGION["iq0"], q)
    put(REGION["power"], (rs.rand(256) * 1000).astype("<f4"))
    rng = np.random.default_rng(35)   # five frames, quiet noise: what a flush handle decodes of so short a capture
    planted = [(s, G.make_frame(df, rng), 600.0 + 100 * i, 0.5 * i) for i, (s, df) in enumerate([(1000, 17), (4000, 17), (7000, 18), (10000, 11), (12500, 17)])]
    big = G.synth(BIG_N, planted, 4.0, 35).astype("<u2")
    put(BIG_AT["u16"], big)
    put(BIG_AT["as3"], ((big.astype(np.int32) - 2048) << 4).astype("<i2"))
    put(BIG_AT["packed"], pack12(big))
    return a


# ---- the rows: (label, handle, operation, flavour, arguments) -- plain data, built without a GPU ----
# arguments: fmt (overrides the flavour's), n | ns, mis / out_mis / env_mis (bytes added to a pointer), cap / env_cap (overrides),
# env (an envelope is asked for), null (names of host arrays passed as NULL), at (the capture a per-capture defect sits on),
# odd (n is not whole groups), table (a bad burst table), host (the _host entry point), big (the capture with frames)

DEFECTS = {
    "fmt_bad": dict(fmt=7), "fmt8": dict(fmt=8), "n_odd": dict(odd=True), "src_mis": dict(mis=True), "out_mis": dict(out_mis=4),
    "cap_small": dict(cap_less=1), "rep_null": dict(null=("rep",)), "arrays_null": dict(null=("srcs",)), "env_xor": dict(null=("env_caps",)),
    "env_null_cap": dict(env_null_cap=True), "env_mis": dict(env_mis=2), "env_small": dict(env_cap_less=1), "table_bad": dict(table=True),
    "frames_null": dict(null=("frames",)), "long": dict(long=True)}
PER_CAPTURE = ("n_odd", "src_mis", "out_mis", "cap_small", "env_null_cap", "env_mis", "env_small")


def order(op, fl, host=False):
    """The refusals a row can reach, in the call's order today.  Host memory is asked no alignment: src_mis and out_mis are no
    refusals there (rows() has such captures answered)."""
    first = ["fmt_bad"] if FAMILY[fl] in ("_as", "_iq") else []
    odd = ["n_odd"] if fl == "packed" else []
    env = ["env_null_cap", "env_mis", "env_small"]
    mis = [] if host else ["src_mis"]
    if op == "power":
        if fl == "u16":
            return ["src_mis", "out_mis", "cap_small"]
        if FAMILY[fl] == "_iq":
            return ["fmt8", "fmt_bad", "src_mis", "out_mis", "cap_small"]
        return first + odd + ["src_mis", "cap_small", "out_mis"]
    if op == "level":
        return first + odd + mis + ["rep_null"] + env
    if op == "gather":
        return first + odd + ["table_bad", "src_mis", "out_mis", "cap_small"]
    if op == "power_batch":
        return (["fmt8"] if FAMILY[fl] == "_iq" else []) + first + ["arrays_null"] + odd + mis + ([] if host else ["out_mis"]) + ["cap_small"]
    if op == "level_batch":
        return first + ["rep_null", "arrays_null", "env_xor"] + odd + mis + env
    if op == "decode_batch":
        if is_real(fl):
            return ["frames_null"] + first + ["arrays_null"] + odd + mis
        return ["frames_null", "arrays_null"] + first + ["long"] + mis
    raise KeyError(op)


def merged(*muts):
    out = {}
    for m in muts:
        for k, v in m.items():
            if k in out and k != "null":
                return None   # (two defects of one argument: no such call)
            out[k] = out.get(k, ()) + v if k == "null" else v
    if out.get("env_null_cap") and ("env_mis" in out or "env_cap_less" in out):
        return None
    return out


def flavours_of(op):
    if op in ("power", "power_batch"):
        return ["u16", "as1", "as3", "packed", "iq0", "iq2"]
    if op == "gather":
        return ["u16", "as1", "as3", "packed"]
    return ["u16", "as1", "as3", "packed", "iq0", "iq2", "iq8", "power"]


OPS = ["power", "level", "gather", "power_batch", "level_batch", "decode_batch"]


def has_host(op, fl):
    """The entry points that take host memory."""
    return (op == "decode_batch") or (fl == "u16" and op in ("level", "level_batch", "power_batch"))


def rows():
    out = []

    def add(label, op, fl, host, **a):
        out.append((f"{op} {fl} {label}" + (", host" if host else ""), op, op, fl, dict(a, host=True) if host else a))
    for op in OPS:
        batch = op.endswith("_batch")
        for fl, host in [(fl, host) for fl in flavours_of(op) for host in (False, True) if not host or has_host(op, fl)]:
            base = dict(ns=[8, 64, 8] if is_real(fl) else [28, 29, 28], env=op.startswith("level")) if batch else \
                dict(n=64 if is_real(fl) else 28, env=op == "level")
            seq = order(op, fl, host)
            # refusals: alone; the two next to each other; per capture first and last
            for i, name in enumerate(seq):
                spots = (0, 2) if batch and name in PER_CAPTURE else (0,)
                for at in spots:
                    add(f"refusal {name}@{at}", op, fl, host, **base, at=at, **DEFECTS[name])
                if i + 1 < len(seq):
                    both = merged(DEFECTS[name], DEFECTS[seq[i + 1]])
                    if both is not None:
                        add(f"refusal {name}+{seq[i + 1]}", op, fl, host, **base, at=0, **both)
                        if batch and name in PER_CAPTURE and seq[i + 1] in PER_CAPTURE:
                            add(f"refusal {name}@2 {seq[i + 1]}@0", op, fl, host, **base, at=2, **DEFECTS[name], second=(0, DEFECTS[seq[i + 1]]))
            # format numbers
            if fl in ("as3", "iq2"):
                for fmt in range(-1, 10):
                    add(f"fmt {fmt}", op, fl, host, **base, fmt=fmt)
            # answers
            if host:   # no alignment is asked of host memory: captures (and float arrays) at odd addresses are answered
                for at in ((0, 2) if batch else (0,)):
                    add(f"answers, the capture at an odd address @{at}", op, fl, host, **base, at=at, odd_addr=True)
                if op == "power_batch":
                    add("answers, a power array at an address that is no multiple of 16", op, fl, host, **base, at=0, out_mis=4)
            if batch:
                add("answers", op, fl, host, ns=list(sizes(fl)), env=op == "level_batch")
                if op == "level_batch":
                    add("answers, no envelope", op, fl, host, ns=list(sizes(fl)), env=False)
                    add("answers, envelopes for some", op, fl, host, ns=list(sizes(fl)), env=True, env_some=True)
                if op == "decode_batch" and not is_real(fl) and not host:
                    add("answers, one capture 4- not 16-byte aligned", op, fl, host, ns=list(sizes(fl)), off16=1)
                if op == "decode_batch" and fl in BIG_AT:
                    add("answers, a capture with frames", op, fl, host, ns=[8, BIG_N, 64], big=1)
            else:
                for n in sizes(fl):
                    if op == "gather":
                        add(f"answers n={n}", op, fl, host, n=n, bursts=1 if count(fl, n) else 0)
                        continue
                    add(f"answers n={n}", op, fl, host, n=n, env=op == "level")
                    if op == "level":
                        add(f"answers n={n}, no envelope", op, fl, host, n=n, env=False)
        if op == "level_batch":
            for fl in ("u16", "as3", "iq0"):
                add("answers, kLevelBatchCaptures + 1 captures", op, fl, False, ns=[8] * 1025, env=False, same=True)
    return out


# ---- running them ----
class Env:
    def __init__(self):
        import numpy as np
        import torch
        from adsbdec_amd import capi
        self.np, self.torch, self.capi = np, torch, capi
        self.L = capi.load()
        torch.cuda.set_device(0)
        self.inp = self.aligned(IN_BYTES)
        self.inp[:] = input_bytes()
        self.IN = torch.from_numpy(self.inp.copy()).cuda()
        self.OUT = torch.empty(OUT_BYTES, dtype=torch.uint8, device="cuda")
        self.out_host = self.aligned(OUT_BYTES)
        self.handles = {}
        self.texts, self.records = [], []

    def aligned(self, nbytes):
        raw = self.np.zeros(nbytes + 256, self.np.uint8)
        at = (-raw.ctypes.data) % 256
        return raw[at:at + nbytes]

    def handle(self, name):
        if name not in self.handles:
            self.handles[name] = self.capi.Decoder(device=0, df18=True, collect_stats=True, long_stream=name.endswith("long"), flush=name.endswith("flush"))
        return self.handles[name]._h

    def text(self, h):
        t = (self.L.adsb_last_error(h) or b"").decode("utf-8", "replace")
        t = re.sub(r"0x[0-9a-fA-F]+", lambda m: "P%d" % (int(m.group(), 16) % 256), t)
        if t not in self.texts:
            self.texts.append(t)
        return self.texts.index(t)

    def run(self, row):
        from adsbdec_amd.levels import BURST_DTYPE
        label, hname, op, fl, a = row
        np, L = self.np, self.L
        h = self.handle(hname + (" long" if a.get("long") else " flush" if a.get("big") else ""))
        host = bool(a.get("host"))
        fam = FAMILY[fl]
        fmt = a.get("fmt", FMT.get(fl))
        head = [fmt] if fam in ("_as", "_iq") else []
        in_base = self.inp.ctypes.data if host else self.IN.data_ptr()
        out_base = self.out_host.ctypes.data if host else self.OUT.data_ptr()
        self.OUT.fill_(SENT)
        self.out_host[:] = SENT
        null = a.get("null", ())
        keep = []   # host arrays whose bytes are part of the record

        def sentinel(nbytes):
            x = self.aligned(max(nbytes, 8))
            x[:] = SENT
            keep.append(x)
            return x

        def src_of(i, n, single=False):
            if a.get("big") and i == 1:
                return in_base + BIG_AT[fl]
            p = in_base + REGION[fl] + (0 if a.get("same") or single else STRIDE * i)
            if a.get("off16") and i == 1:
                p += 4 if fl != "iq8" else 2
            return p

        def defects(i):
            d = dict(a) if a.get("at", 0) == i else {}
            if "second" in a and a["second"][0] == i:
                d = dict(a["second"][1])
            return d

        def capture(i, n, single=False):
            """(pointer, n, out pointer, cap, env pointer, env cap) of capture i with its defects"""
            d = defects(i)
            if d.get("odd"):
                n -= 4
            m = count(fl, n)
            p = src_of(i, n, single) + (ALIGN[fl] // 2 if d.get("mis") else 1 if d.get("odd_addr") else 0)
            o = out_base + 1024 * i + d.get("out_mis", 0)
            cap = max(0, m - d.get("cap_less", 0))
            ef = (m + 27) // 28
            want_env = a.get("env") and not (a.get("env_some") and i % 2)
            e = out_base + ENV_AT + 256 * i + d.get("env_mis", 0) if want_env else 0
            ecap = max(0, ef - d.get("env_cap_less", 0)) if want_env else 0
            if d.get("env_null_cap"):
                e, ecap = 0, 3
            return p, n, o, cap, e, ecap

        if not op.endswith("_batch"):
            p, n, o, cap, e, ecap = capture(0, a["n"], single=True)
            if op == "power":
                args = [h] + head + [p, n, o, cap]
            elif op == "level":
                rep = sentinel(C.sizeof(self.capi.LevelReport))
                args = [h] + head + [p, n, None if "rep" in null else rep.ctypes.data, e or None, ecap]
            else:
                nb = a.get("bursts", 1)
                tab = np.zeros(max(nb, 1), BURST_DTYPE)
                if nb:
                    tab[0] = (1, 1, 0, 0.0) if a.get("table") else (0, 1, 0, 0.0)
                off, over = sentinel(8 * (nb + 1)), sentinel(8)
                groups = (min(28, count(fl, n)) + 3) // 4 if nb else 0
                total = (12 * groups + 15) // 16 * 16
                args = [h] + head + [p, n, tab.ctypes.data if nb else None, nb, o, max(0, total - 16 * a.get("cap_less", 0)), off.ctypes.data,
                                     C.cast(over.ctypes.data, C.POINTER(C.c_uint64))]
            name = {"power": "adsb_power_device", "level": "adsb_level_host" if host else "adsb_level_device", "gather": "adsb_gather_pack12_device"}[op]
            name += "" if host else fam
        else:
            ns = a["ns"]
            k = len(ns)
            caps6 = [capture(i, ns[i]) for i in range(k)]
            srcs = (C.c_void_p * k)(*[c[0] for c in caps6])
            nn = (C.c_size_t * k)(*[c[1] for c in caps6])
            asrc = None if "srcs" in null else C.cast(srcs, C.c_void_p)
            ann = C.cast(nn, C.c_void_p)
            if op == "power_batch":
                outs = (C.c_void_p * k)(*[c[2] for c in caps6])
                caps = (C.c_size_t * k)(*[c[3] for c in caps6])
                args = [h] + head + [k, asrc, ann, C.cast(outs, C.c_void_p), C.cast(caps, C.c_void_p)]
                name = "adsb_power_batch_host" if host else "adsb_power_batch_device" + fam
            elif op == "level_batch":
                rep = sentinel(k * C.sizeof(self.capi.LevelReport))
                envs = (C.c_void_p * k)(*[c[4] or None for c in caps6])
                ecaps = (C.c_size_t * k)(*[c[5] for c in caps6])
                with_env = bool(a.get("env"))
                args = [h] + head + [k, asrc, ann, None if "rep" in null else rep.ctypes.data, C.cast(envs, C.c_void_p) if with_env else None,
                                     C.cast(ecaps, C.c_void_p) if with_env and "env_caps" not in null else None]
                name = "adsb_level_batch_host" if host else "adsb_level_batch_device" + fam
            else:
                frames = C.POINTER(self.capi.Frame)()
                first = (C.c_uint64 * (k + 1))(*([0xA5A5] * (k + 1)))
                st = (self.capi.Stats * k)()
                args = [h] + head + [k, None if "srcs" in null else srcs, nn, None if "frames" in null else C.byref(frames), first, st]
                name = "adsb_decode_batch_" + ("host" if host else "device") + fam
        ret = getattr(L, name)(*args)
        digest = hashlib.sha1()
        digest.update(self.OUT.cpu().numpy().tobytes())
        digest.update(self.out_host.tobytes())
        for x in keep:
            digest.update(x.tobytes())
        if op == "decode_batch":
            digest.update(bytes(first))
            digest.update(bytes(st))
            if ret > 0:
                digest.update(C.string_at(frames, ret * C.sizeof(self.capi.Frame)))
        fr = self.capi.FormatReport()
        rc = L.adsb_get_format_report(h, C.byref(fr))
        self.records.append([label, name, int(ret), self.text(h), digest.hexdigest()[:16], [rc, fr.converted, fr.inexact, fr.clamped]])

    def states(self):
        """Behind the last call on every handle: the frames of one small plain decode to its last sample (a reset, flush on -- a
        long-stream handle refuses that and decodes to the horizon), and its Try/Ok table."""
        out = {}
        for name, d in sorted(self.handles.items()):
            frames = C.POINTER(self.capi.Frame)()
            self.L.adsb_reset(d._h)
            self.L.adsb_set_flush(d._h, 1)
            k = self.L.adsb_decode_device(d._h, self.IN.data_ptr() + BIG_AT["u16"], BIG_N, C.byref(frames))
            st = self.capi.Stats()
            self.L.adsb_get_stats(d._h, C.byref(st))
            body = C.string_at(frames, k * C.sizeof(self.capi.Frame)) if k > 0 else b""
            out[name] = [int(k), self.text(d._h), hashlib.sha1(body + bytes(st)).hexdigest()[:16]]
        return out


def record(env=None):
    """The record of every row with the library ADSB_LIB_PATH names (or the tree's)."""
    env = env or Env()
    for r in rows():
        env.run(r)
    states = env.states()
    for d in env.handles.values():
        d.close()
    return {"texts": env.texts, "rows": env.records, "states": states}


def pack(rec, sha):
    """The recording as the fixture holds it: no labels (rows() has them; their digest is kept), a text as (entry point, sentence)."""
    heads, bodies, pairs = [], [], []
    for t in rec["texts"]:
        h, sep, b = t.partition(": ")
        h, b = (h, b) if sep else ("", t)
        for x, xs in ((h, heads), (b, bodies)):
            if x not in xs:
                xs.append(x)
        pairs.append([heads.index(h), bodies.index(b)])
    return {"revision": sha, "labels": hashlib.sha1("\n".join(r[0] for r in rec["rows"]).encode()).hexdigest(), "heads": heads, "bodies": bodies,
            "texts": pairs, "rows": [r[2:4] + [r[4][:12]] + [r[5]] for r in rec["rows"]], "states": rec["states"]}


def unpack(gold, labels_and_names):
    """... back into a record's form, with the labels and entry points of `labels_and_names` (rows of a record made here)."""
    assert gold["labels"] == hashlib.sha1("\n".join(r[0] for r in labels_and_names).encode()).hexdigest(), "rows() is not what was recorded"
    texts = [(gold["heads"][h] + ": " if gold["heads"][h] else "") + gold["bodies"][b] for h, b in gold["texts"]]
    return {"texts": texts, "rows": [list(ln[:2]) + g[:2] + [g[2]] + [g[3]] for ln, g in zip(labels_and_names, gold["rows"])], "states": gold["states"]}


def run_child(lib, path):
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", path]
    p = subprocess.run(cmd, env=dict(os.environ, ADSB_LIB_PATH=lib), cwd=ROOT)
    if p.returncode != 0:
        sys.exit(f"the process that loaded {lib} ended with status {p.returncode}: stopping here")
    with open(path) as f:
        return json.load(f)


def parent_library(rev):
    """The revision's library in PARENT_DIR -> the revision's name.  Built in a temporary worktree, unless one lies there whose REVISION
    stamp names the revision asked for; where the history is not at hand, a stamped library is taken for what its stamp says.  A
    library without a stamp is nobody's: refused."""
    stamp = os.path.join(PARENT_DIR, "REVISION")
    have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(PARENT_LIB) else None
    if os.path.exists(PARENT_LIB) and have is None:
        sys.exit(f"{PARENT_LIB} has no REVISION stamp beside it: remove it, or say which revision it was built from")
    history = subprocess.run(["git", "-C", ROOT, "rev-parse", "--git-dir"], capture_output=True).returncode == 0
    if not history:
        if have is None:
            sys.exit(f"no history and no library in {PARENT_DIR}: build it where the history is (--build-only)")
        return have
    if rev is None:
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], check=True, capture_output=True).stdout
        rev = "HEAD" if dirty else "HEAD~1"
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], check=True, capture_output=True, text=True).stdout.strip()
    if have == sha:
        return sha
    os.makedirs(PARENT_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", old, rev], check=True, capture_output=True)
        try:
            subprocess.run([sys.executable, "-m", "adsbdec_amd._build"], cwd=old, check=True, capture_output=True)
            subprocess.run(["cp", os.path.join(old, "adsbdec_amd", "lib", "libadsbdec_amd.so"), PARENT_LIB], check=True)
        finally:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", old], check=True, capture_output=True)
    with open(stamp, "w") as f:
        f.write(sha + "\n")
    return sha


def fail_sites():
    """(unit, line number, the longest fixed piece of the sentence, the line) of every d->fail of the units the rows reach."""
    from adsbdec_amd import _build as B
    out = []
    for unit in UNITS:
        path = os.path.join(B.CSRC, unit)
        if not os.path.exists(path):
            continue
        for no, line in enumerate(open(path), 1):
            m = re.search(r'd->fail\("((?:[^"\\]|\\.)*)"', line)
            if m:
                pieces = re.split(r"%[-0-9.]*(?:zu|llu|lu|u|d|s|p|zd)", m.group(1).replace("%s: ", "", 1))
                out.append((unit, no, max(pieces, key=len).strip(), line))
    return out


def summary(sha, old, new):
    lines, ok = [], True
    said = "\n".join(old["texts"])
    lines.append(f"# the library of {sha} against the working tree's: {len(old['rows'])} rows, each run by both, one process after the other")
    differing = [(o, n) for o, n in zip(old["rows"], new["rows"]) if o != n]
    ok = ok and not differing and len(old["rows"]) == len(new["rows"]) and old["states"] == new["states"]
    lines.append(f"{len(differing):7d}  differing rows")
    for o, n in differing[:40]:
        lines.append(f"DIFFERS {o[0]} [{o[1]}]\n  returns {o[2]} -> {n[2]}\n  says {old['texts'][o[3]]!r}\n    -> {new['texts'][n[3]]!r}\n"
                     f"  outputs {o[4]} -> {n[4]}   format report {o[5]} -> {n[5]}")
    lines.append(f"{sum(1 for r in old['rows'] if r[2] < 0):7d}  refused rows, {sum(1 for r in old['rows'] if r[2] >= 0)} answered, "
                 f"{sum(1 for r in old['rows'] if any(r[5][1:]))} with a format report that is not zero")
    lines.append(f"# the handles' state behind their last call (frames of a plain decode, text, digest): {'same' if old['states'] == new['states'] else 'DIFFERS'}")
    for name in sorted(old["states"]):
        lines.append(f"  {name:20s} {old['states'][name]}" + ("" if old["states"][name] == new["states"].get(name) else f"  -> {new['states'].get(name)}"))
    unreached = []
    for unit, no, piece, line in fail_sites():
        if not piece or piece in said:   # (no fixed piece: the sentence is another function's reason, handed through)
            continue
        why = next((w for p, w in NOT_IN_THE_GRID if p in line), None)
        if unit == "decoder.hip" or any(p in line for p in OUT_OF_SCOPE):
            continue
        unreached.append((unit, no, piece, why))
    lines.append(f"# d->fail sites of {', '.join(UNITS[:-1])} that no row reached: {len(unreached)}, "
                 f"{sum(1 for u in unreached if u[3] is None)} of them unexplained")
    for unit, no, piece, why in unreached:
        lines.append(f"  {unit}:{no}  {piece[:70]!r}  -- {'not in the grid: ' + why if why else 'UNEXPLAINED'}")
    ok = ok and all(u[3] for u in unreached)
    lines.append(f"# the {len(old['texts'])} distinct texts seen")
    lines += [f"  {t!r}" for t in sorted(old["texts"])]
    return ok, "\n".join(lines) + "\n"


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    revs = [a for a in argv if not a.startswith("--")]
    if "--child" in flags:
        with open(revs[0], "w") as f:
            json.dump(record(), f)
        return 0
    if "--list" in flags:
        rs = rows()
        for r in rs:
            print(r[0], r[4])
        print(f"{len(rs)} rows")
        return 0
    sha = parent_library(revs[0] if revs else None)
    if "--build-only" in flags:
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        old = run_child(PARENT_LIB, os.path.join(tmp, "old.json"))
        if "--write-golden" in flags:
            with open(GOLDEN, "w") as f:
                json.dump(pack(old, sha), f, separators=(",", ":"))
                f.write("\n")
            print(f"{GOLDEN}: {len(old['rows'])} rows of {sha}, {len(old['texts'])} distinct texts")
        from adsbdec_amd import _build as B
        new = run_child(B.LIB, os.path.join(tmp, "new.json"))
    ok, text = summary(sha, old, new)
    sys.stdout.write(text)
    for f in flags:
        if f.startswith("--summary="):
            with open(f.split("=", 1)[1], "w") as fh:
                fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
