"""make_ref_recordings.py -- TEST INFRASTRUCTURE ONLY: mints tests/golden/ref_recordings.json.gz.

Run where oracle/_ref can be built (it needs the reference sources, oracle/Makefile):

    python oracle/make_ref_recordings.py

Runs the CPU tests that pin the restatement against the REAL reference chain
(tests/test_oracle_vs_ref.py, the ref tests of tests/test_oracle.py) with every call of
oracle.ref_decode / ref_demod / ref_power_digest recorded: key = sha256 of the call's
options and input bytes, value = the chain's frames, renderings and Try/Ok table (power
samples: their count and the sha256 of their bits).  Where oracle/_ref is absent the same
tests replay these answers, so they need nothing outside the repository.
"""
from __future__ import annotations

import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

TESTS = ["tests/test_oracle_vs_ref.py", "tests/test_oracle.py"]


def main() -> None:
    if not O.build_ref():
        raise SystemExit("oracle/_ref cannot be built here: the recordings need the real chain")
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "calls.jsonl")
        open(log, "w").close()
        env = dict(os.environ, ORACLE_REF_RECORD=log)
        subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
        rec = {}
        with open(log) as f:
            for line in f:
                key, value = json.loads(line)
                assert rec.setdefault(key, value) == value, f"the reference answered {key[:16]} twice, differently"
    with open(O.REF_RECORDINGS, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode())
    print(f"{O.REF_RECORDINGS}: {len(rec)} calls, {os.path.getsize(O.REF_RECORDINGS)} bytes")


if __name__ == "__main__":
    main()
