"""Did a change move the device code?  The gfx950 assembly of every HIP unit of the library (_build.HIP_SOURCES), compiled
from a git revision's tree and from the working tree with the build's flags, compared line by line.  CPU only: nothing runs.

    python tools/isa_identity.py [revision]        # default: the parent commit -- HEAD while the tree has uncommitted changes, else HEAD~1
    python tools/isa_identity.py HEAD~1 > profiles/<tag>_isa_identity.txt

The revision is checked out into a temporary git worktree, removed afterwards.  Per unit: "identical (N lines)" or the number of
differing lines, and behind the list a unified diff of every unit that has any.  The per-unit hash symbol (__hip_cuid_*, a hash
of the unit's path) is left out: it differs between any two trees.  A unit that one of the trees lacks is said so.  Two texts
are compared; no instruction is looked for."""
import difflib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adsbdec_amd import _build as B  # noqa: E402

CSRC_REL = os.path.relpath(B.CSRC, ROOT)


def device_asm(tree, unit, out):
    """Lines of `unit`'s device assembly in `tree` (None: the tree has no such unit).  Compiled from inside csrc/ under the
    unit's bare name, so that no line of the text depends on where the tree lies."""
    csrc = os.path.join(tree, CSRC_REL)
    if not os.path.exists(os.path.join(csrc, unit)):
        return None
    p = subprocess.run([B.HIPCC] + B.HIP_FLAGS + ["--cuda-device-only", "-S", unit, "-o", out], cwd=csrc, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"{csrc}: {unit} does not compile\n{p.stderr}")
    with open(out) as f:
        return [line for line in f if "__hip_cuid_" not in line]


def main(rev):
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", old_tree, rev], check=True, capture_output=True)
        try:
            units = sorted(B.HIP_SOURCES)
            jobs = [(tree, u, os.path.join(tmp, f"{tag}_{u}.s")) for u in units for tag, tree in (("old", old_tree), ("new", ROOT))]
            with ThreadPoolExecutor(16) as pool:
                texts = list(pool.map(lambda j: device_asm(*j), jobs))
        finally:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", old_tree], check=True, capture_output=True)
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], check=True, capture_output=True, text=True).stdout.strip()
    print(f"# gfx950 device code per unit, {sha} against the working tree: {' '.join(B.HIP_FLAGS)} --cuda-device-only -S;")
    print("# __hip_cuid_* lines left out")
    hunks = []
    for i, unit in enumerate(units):
        old, new = texts[2 * i], texts[2 * i + 1]
        if old is None:
            print(f"{unit}.s new ({len(new)} lines)")
            continue
        diff = list(difflib.unified_diff(old, new, f"{sha}/{unit}.s", f"tree/{unit}.s", n=2))
        n = sum(1 for d in diff if d[0] in "+-" and not d.startswith(("+++", "---")))
        print(f"{unit}.s identical ({len(new)} lines)" if n == 0 else f"{unit}.s {n} differing lines ({len(old)} -> {len(new)} lines)")
        hunks += diff
    sys.stdout.writelines(hunks)
    return 0


if __name__ == "__main__":
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], check=True, capture_output=True).stdout
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "HEAD" if dirty else "HEAD~1"))
