"""Did a change move the host program?  The files of csrc/cli/ of a git revision and of the working tree, each compiled with the
build's own gcc line against the working tree's library (the library's ABI must be the same), run over the same command lines:
exit status, stdout bytes and stderr bytes compared.

    python tools/cli_identity.py [revision]                 # the option grid: no GPU needed, nothing it compares reaches the runtime
    python tools/cli_identity.py [revision] --write-golden  # tests/golden/cli_options.grid from the REVISION's program
    python tools/cli_identity.py [revision] --runs          # real runs on a GPU, one process at a time; files written compared too
    python tools/cli_identity.py [revision] --programs=DIR  # keep the two programs in DIR, or take the pair that lies there

The default revision is the parent commit -- HEAD while the tree has uncommitted changes, else HEAD~1 -- checked out into a
temporary git worktree, removed afterwards.  Both programs are started under the same argv[0] (getopt's own messages print it),
every command in an empty directory of its own and under a time limit of its own.  A grid case whose revision run says
`adsb_create() failed` or `adsb_multi_create() failed`, or runs into its time limit, has reached the GPU runtime: counted by
class and not compared, the text behind it belongs to the machine.  No compared grid case may leave a file behind.  The summary
(case counts per class, the distinct texts seen, the coverage of the refusals) goes to stdout; exit status 1 on any difference."""
import glob
import itertools
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd import _build as B  # noqa: E402

CLI_REL = os.path.relpath(os.path.join(B.CSRC, "cli"), ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_options.grid")
ARGV0 = "adsbdec_amd_cli"
LIMIT_S = 20

TOKENS = [["-a"], ["-m"], ["-b"], ["-x"], ["-p"], ["-w"], ["-E"], ["-L"], ["-k"],
          ["-t", "3"], ["-t", "1"], ["-t", "0"], ["-t", "2"], ["-t", "9"], ["-t", "x"],
          ["-q", "2"], ["-q", "0"], ["-q", "8"], ["-q", "5"], ["-q", "x"],
          ["-d", "0"], ["-d", "x"], ["-G", "2"], ["-G", "0,0"], ["-G", "x"],
          ["-B", "list.txt"], ["-W", "o.pw"], ["-K", "o.brs"], ["-P", "o.brs"],
          ["-I", "5"], ["-I", "0"], ["-I", "x"], ["-I", "0.001"],
          ["-U", "8"], ["-U", "48,2,4"], ["-U", "0"], ["-U", "8,x"], ["-e"]]
PEER_TOKENS = [["-s", "127.0.0.1:1"], ["-l", "127.0.0.1:1"]]   # loopback only; crossed with the prefixes that refuse them
PEER_PREFIXES = (["-L"], ["-W", "o.pw"], ["-B", "list.txt"])
PREFIXES = [[], ["-L"], ["-L", "-U", "8"], ["-L", "-U", "8", "-K", "o.brs"], ["-L", "-U", "8", "-P", "o.brs"], ["-L", "-I", "5"],
            ["-k"], ["-W", "o.pw"], ["-B", "list.txt"], ["-G", "2"], ["-E"], ["-q", "8"]]
TAILS = [[], ["-f", "nothing.bin"], ["-f", "nothing.bin", "-f", "nothing2.bin"]]

# What the revision's program must have said at least once among the compared cases: (name, a piece of its stderr or stdout)
WITH = {"-P": "-q -w -K -I -G -B -W -k", "-k": "-t -p -q -w -E -G -B -L -W -K several_-f", "-K": "-t -p -I -G -B -W", "-E": "-G -L -W",
        "-L": "-G -B -W -s -l several_-f", "-I": "-t -p -q -w", "-U": "-I", "-q 8": "-t -p -G -B -w -W", "-W": "-w -t -p -G -B -s -l several_-f",
        "-t 3": "-p -G -B", "-t 1": "-p -G -B", "-q 2": "-t -p -G -B", "-w": "-t -q -p -G -B", "-p (packed 12-bit input)": "-G"}
COVERAGE = [(f"{s} with {w}", f"{s} is not supported with {w.replace('_', ' ')}: ") for s, ws in WITH.items() for w in ws.split()] + [
    ("-P without -L -U", "-P is not supported without -L -U"), ("-K without -L -U", "-K is not supported without -L -U"),
    ("-I without -L", "-I is not supported without -L"), ("-I bad value", "-I x: the windows' length"), ("-I below 28 samples", "a window holds at least 28"),
    ("-U without -L", "the level report's call writes\n"), ("-U without -L (-G)", "(and not with -G)"), ("-U without -L (-B)", "(and not with -B)"),
    ("-U without -L (-W)", "(and not with -W)"), ("-U bad value", "-U 8,x: factor[,lead[,hang]]"),
    ("-t 0", "-t 0 (FLOAT32_IQ) is not a real sample type"), ("-t 2", "-t 2 (INT16_IQ) is not a real sample type"), ("-t unknown", "-t 9: unknown sample type"),
    ("-q unknown", "-q 5: not an IQ sample type"),
    ("-L, missing file", "nothing.bin: cannot read as a regular file"), ("-W | -L -I, missing file", "nothing.bin: cannot read: "),
    ("-k, missing file", "nothing.bin: cannot open"), ("-k, no archive", "bad magic: no burst archive"), ("unusable address", "Invalid IPV6 address"), ("-B, missing list", "list.txt: cannot read the list of captures")]
USAGE_CASES = [("no -f", ["-a"]), ("several -f without -G", ["-f", "nothing.bin", "-f", "nothing2.bin"]), ("-d with -G", ["-G", "2", "-d", "0", "-f", "nothing.bin"]),
               ("-B with -f", ["-B", "list.txt", "-f", "nothing.bin"]), ("-B with -s", ["-B", "list.txt", "-s", "127.0.0.1:1"]),
               ("-B with -l", ["-B", "list.txt", "-l", "127.0.0.1:1"]), ("bad -d", ["-d", "x", "-f", "nothing.bin"]), ("bad -G", ["-G", "x", "-f", "nothing.bin"]),
               ("the 65th -f", ["-f", "nothing.bin"] * 65), ("-e", ["-e", "-f", "nothing.bin"])]


def grid():
    """Every prefix x (every token, every ordered pair of tokens) x every tail, the 65 -f, each once."""
    cases = []
    for prefix in PREFIXES:
        tokens = TOKENS + (PEER_TOKENS if prefix in PEER_PREFIXES else [])
        middles = [a for a in tokens] + [a + b for a, b in itertools.permutations(tokens, 2)]
        cases += [prefix + m + tail for m in middles for tail in TAILS]
    cases += [args for _, args in USAGE_CASES]
    return sorted(set(map(tuple, cases)))


def golden_subset():
    """Every prefix x every token with one -f, and every ordered pair of tokens without a prefix (one -f)."""
    one_f = TAILS[1]
    cases = [p + t + one_f for p in PREFIXES for t in TOKENS + (PEER_TOKENS if p in PEER_PREFIXES else [])]
    cases += [a + b + one_f for a, b in itertools.permutations(TOKENS, 2)]
    return sorted(set(map(tuple, cases)))


def compile_cli(tree, out):
    srcs = sorted(glob.glob(os.path.join(tree, CLI_REL, "*.c")))
    p = subprocess.run(B.cli_command(out, srcs), capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{tree}: the host program does not compile\n{p.stderr}")
    return out


def run(exe, args, env=None, limit=LIMIT_S, base=None):
    """(status, stdout, stderr, files left) of one run in an empty directory (under `base`); status None: the time limit."""
    env = dict(env or os.environ)
    env["LD_LIBRARY_PATH"] = B.LIBDIR + os.pathsep + env.get("LD_LIBRARY_PATH", "")   # (the programs do not lie beside the library)
    with tempfile.TemporaryDirectory(dir=base) as cwd:
        try:
            p = subprocess.run([ARGV0] + list(args), executable=exe, cwd=cwd, capture_output=True, timeout=limit, stdin=subprocess.DEVNULL, env=env)
            status, out, err = p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            status, out, err = None, e.stdout or b"", e.stderr or b""
        left = {}
        for f in sorted(os.listdir(cwd)):
            with open(os.path.join(cwd, f), "rb") as fh:
                left[f] = fh.read()
        return status, out, err, left


def reaches_runtime(status, err):
    return "time limit" if status is None else "adsb_create() failed" if b"adsb_create() failed" in err else \
        "adsb_multi_create() failed" if b"adsb_multi_create() failed" in err else None


# Endings before the runtime that need a file that EXISTS: the reader thread is at work on it while the program leaves
WITH_A_FILE = [["-s", "[::1", "-f", "../capture.u16"], ["-l", "[::1", "-f", "../capture.u16"], ["-a", "-s", "[::1", "-f", "../capture.u16"],
               ["-k", "-f", "../capture.u16"], ["-k", "-s", "[::1", "-f", "../capture.u16"]]


def run_grid(old, new):
    cases = grid() + [tuple(c) for c in WITH_A_FILE for _ in range(8)]
    with tempfile.TemporaryDirectory() as base, ThreadPoolExecutor(16) as pool:
        with open(os.path.join(base, "capture.u16"), "wb") as f:
            f.truncate(512 << 20)   # (sparse: zeros, long enough to keep the reader busy; every run's directory lies beside it)
        olds = list(pool.map(lambda a: run(old, a, base=base), cases))
        news = list(pool.map(lambda a: run(new, a, base=base), cases))
    classes, texts, differing, left_behind = {}, {}, [], []
    for args, o, n in zip(cases, olds, news):
        cls = reaches_runtime(o[0], o[2]) or "ends before the runtime"
        classes[cls] = classes.get(cls, 0) + 1
        if cls != "ends before the runtime":
            continue
        texts.setdefault((o[0], o[2], len(o[1])), []).append(args)
        if n is not None and n[:3] != o[:3]:
            differing.append((args, o, n))
        if o[3] or (n is not None and n[3]):
            left_behind.append(args)
    return cases, olds, classes, texts, differing, left_behind


def report_grid(sha, cases, olds, classes, texts, differing, left_behind):
    ok = True
    print(f"# the host program of {sha} against the working tree's, option grid: {len(cases)} command lines, each run by both")
    for cls, k in sorted(classes.items()):
        print(f"{k:7d}  {cls}" + ("" if cls == "ends before the runtime" else "  (not compared)"))
    print(f"{len(differing):7d}  differing among the compared")
    print(f"{len(left_behind):7d}  compared cases that left a file behind")
    for args, o, n in differing[:40]:
        print(f"DIFFERS {' '.join(args)}\n  status {o[0]} -> {n[0]}\n  stderr {o[2]!r}\n      -> {n[2]!r}" + ("" if o[1] == n[1] else "\n  stdout differs"))
    for args in left_behind[:40]:
        print(f"LEFT A FILE {' '.join(args)}")
    ok = ok and not differing and not left_behind
    compared = [o for a, o in zip(cases, olds) if not reaches_runtime(o[0], o[2])]
    said = b"\n".join(o[1][:200] + o[2] for o in compared).decode("utf-8", "replace") + "\n"
    missing = [name for name, piece in COVERAGE if piece not in said]
    by_args = dict(zip(cases, olds))
    missing += [f"usage text: {name}" for name, args in USAGE_CASES if not (by_args[tuple(args)][0] == 1 and by_args[tuple(args)][1].startswith(b"adsbdec_amd : "))]
    print(f"# coverage: {len(COVERAGE) + len(USAGE_CASES)} messages asked for, {len(missing)} never seen" + "".join(f"\nNEVER SEEN {m}" for m in missing))
    ok = ok and not missing
    print(f"# the {len(texts)} distinct (status, stderr, bytes of stdout) among the compared, with the number of cases and one of them")
    for (status, err, n_out), which in sorted(texts.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print(f"{len(which):6d}  status {status} stdout {n_out:5d}  {err.decode('utf-8', 'replace').strip()!r}  [{' '.join(which[0])}]")
    return ok


def write_golden(old):
    cases = golden_subset()
    with ThreadPoolExecutor(16) as pool:
        got = list(pool.map(lambda a: run(old, a), cases))
    texts, rows = [], []
    for args, (status, out, err, left) in zip(cases, got):
        if reaches_runtime(status, err):
            continue
        assert not left, args
        idx = []
        for t in (out.decode(), err.decode()):
            if t not in texts:
                texts.append(t)
            idx.append(texts.index(t))
        rows.append([list(args), status] + idx)
    with open(FIXTURE, "w") as f:
        json.dump({"argv0": ARGV0, "texts": texts, "cases": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{FIXTURE}: {len(rows)} cases of {len(cases)} ({len(cases) - len(rows)} reach the runtime), {len(texts)} distinct texts")


def real_runs(old, new):
    """On a GPU: the committed golden capture as every kind of input (the same bytes reinterpreted: good enough for a comparison
    of two programs), each command once per program, one process at a time; stops at the first abnormal exit."""
    import numpy as np
    x = np.load(os.path.join(ROOT, "tests", "golden", "config1_1Mi_100xDF17.npz"))["x"].astype("<u2")
    y = np.load(os.path.join(ROOT, "tests", "golden", "ragged_tail.npz"))["x"].astype("<u2")
    with tempfile.TemporaryDirectory() as data:
        cap, cap2, lst = (os.path.join(data, f) for f in ("a.bin", "b.bin", "list.txt"))
        x.tofile(cap), y.tofile(cap2)
        with open(lst, "w") as f:
            f.write(cap + "\n\n" + cap2 + "\n")
        f1 = ["-f", cap]
        commands = [([], f1), ([], ["-m"] + f1), ([], ["-b"] + f1), ([], ["-a", "-x"] + f1), ([], ["-p"] + f1), ([], ["-t", "3"] + f1),
                    ([], ["-q", "2"] + f1), ([], ["-q", "8"] + f1), ([], ["-w"] + f1), ([], ["-E"] + f1), ([], ["-W", "o.pw"] + f1), ([], ["-L"] + f1),
                    (["ADSB_CLI_LEVEL_PIECE=2"], ["-L", "-I", "1"] + f1), ([], ["-L", "-U", "8"] + f1),
                    ([], ["-L", "-U", "48,2,4", "-K", os.path.join(data, "{}_k.brs")] + f1), ([], ["-k", "-f", os.path.join(data, "{}_k.brs")]),
                    ([], ["-L", "-U", "48,2,4", "-P", os.path.join(data, "{}_p.brs")] + f1), ([], ["-k", "-f", os.path.join(data, "{}_p.brs")]),
                    ([], ["-B", lst]), ([], ["-G", "0,0"] + f1), ([], ["-G", "0,0"] + f1 + ["-f", cap2])]
        outputs = [cap + e for e in (".avr", ".mlat", ".beast")] + [cap2 + e for e in (".avr", ".mlat", ".beast")]
        differing = 0
        print(f"# real runs, one process at a time: {len(commands)} commands, each by both programs; timing: lines left out")
        for env_add, args in commands:
            got = []
            for tag, exe in (("old", old), ("new", new)):
                env = dict(os.environ, ADSB_CLI_TIMING="1", **dict(e.split("=") for e in env_add))
                mine = [a.format(tag) for a in args]
                status, out, err, left = run(exe, mine, env=env, limit=120)
                for path in outputs + [a for a in mine if a.endswith(".brs") and "-k" not in mine]:
                    if os.path.exists(path):
                        with open(path, "rb") as fh:
                            left[os.path.basename(path).replace(tag + "_", "")] = fh.read()
                        if not path.endswith(".brs"):
                            os.remove(path)
                if status is None or status < 0 or status in (124, 134, 137, 139):
                    print(f"ABNORMAL EXIT {status} of the {tag} program: {' '.join(mine)}\n{err.decode('utf-8', 'replace')}\nstopping here")
                    return False
                err = b"".join(line for line in err.splitlines(True) if not line.startswith(b"timing:")).replace(tag.encode() + b"_", b"")
                got.append((status, out, err, left))
            same = got[0] == got[1]
            differing += not same
            o = got[0]
            print(f"{'same   ' if same else 'DIFFERS'} status {o[0]} stdout {len(o[1])} stderr {len(o[2])} files {sorted((k, len(v)) for k, v in o[3].items())}  "
                  f"{' '.join(env_add + [a.replace(data + os.sep, '') for a in args])}")
            if not same:
                print(f"  old: {got[0][0]} {got[0][2][-600:]!r}\n  new: {got[1][0]} {got[1][2][-600:]!r}")
        print(f"{differing:7d}  differing of {len(commands)}")
        return differing == 0


def programs(rev, where):
    """The revision's program and the tree's, compiled into `where`; a pair that lies there already is taken as it is (a machine
    without the history runs what another one has compiled)."""
    old, new = (os.path.join(os.path.abspath(where), name) for name in ("cli_old", "cli_new"))
    if os.path.exists(old) and os.path.exists(new):
        return old, new, rev or "the revision"
    if rev is None:
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], check=True, capture_output=True).stdout
        rev = "HEAD" if dirty else "HEAD~1"
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", old_tree, rev], check=True, capture_output=True)
        try:
            compile_cli(old_tree, old)
        finally:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", old_tree], check=True, capture_output=True)
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], check=True, capture_output=True, text=True).stdout.strip()
    return old, compile_cli(ROOT, new), sha


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    revs = [a for a in argv if not a.startswith("--")]
    rev = revs[0] if revs else None
    kept = [f.split("=", 1)[1] for f in flags if f.startswith("--programs=")]
    with tempfile.TemporaryDirectory() as tmp:
        if kept:
            os.makedirs(kept[0], exist_ok=True)
        old, new, sha = programs(rev, kept[0] if kept else tmp)
        if "--build-only" in flags:
            return 0
        if "--write-golden" in flags:
            write_golden(old)
            return 0
        if "--runs" in flags:
            return 0 if real_runs(old, new) else 1
        return 0 if report_grid(sha, *run_grid(old, new)) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
