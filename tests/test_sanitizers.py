"""The library's threaded host code under ThreadSanitizer and AddressSanitizer / UBSan, without a GPU.

Two harnesses (tests/cpp/), each built twice with g++:
  handoff_tsan.cpp  the reading side of the device -> host hand-off (handoff.hpp: HandCursor, StreamReader, the two
                    consumer loops and the finish after completion) + the resolver behind it, with a thread that plays the device: random completion
                    order, torn and stale writes, overflow, a tile twice, a tile never;
  multi_tsan.cpp    the multi-GPU driver (multi.cpp: workers, job hand-over, stitch, gather, fallback, error paths) against
                    a fake device backend whose scan is a table look-up; everything behind the scan is the product's code.
What the reference has in these places is one mutex + condition variable (output.c:159-202); this replaces it with
lock-free polling and a pool of workers, so it gets a race detector behind it."""
import os
import platform
import shutil
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
# ThreadSanitizer wants a PIE program where the kernel's default randomisation puts it; a host with wider mmap randomisation
# maps it elsewhere and TSan stops at start-up ("unexpected memory mapping"): the sanitized programs run with it off (setarch -R,
# a personality flag of that one child)
NO_ASLR = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []
SAN = {"tsan": ["-fsanitize=thread"], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _build(tmp_path, src, san):
    exe = tmp_path / (os.path.splitext(src)[0] + "_" + san)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wno-subobject-linkage"] + SAN[san] + [os.path.join(CPP, src), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def _run(exe, rounds, timeout=600):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run(NO_ASLR + [exe, str(rounds)], capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith("ok:"), (p.stdout[-500:], p.stderr[-4000:])
    assert "ThreadSanitizer" not in p.stderr and "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return p.stdout


@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_handoff_reader_under_sanitizers(tmp_path, san):
    out = _run(_build(tmp_path, "handoff_tsan.cpp", san), 32)
    # every way a collect can end was exercised, by one thread and by two
    assert "16 complete, 8 finish-after-completion, 4 tile-twice, 4 never-published" in out, out
    # ... and each of the eight launches that asked for it was finished after completion: the sorted union of stream and loose list
    assert int(out.split(" records finished after completion")[0].split()[-1]) > 1000, out


@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_multi_gpu_driver_under_sanitizers(tmp_path, san):
    out = _run(_build(tmp_path, "multi_tsan.cpp", san), 8)
    assert "24 sharded decodes" in out and "streams and error paths" in out, out
    # adsb_multi_host_alloc + adsb_multi_worker_placement against a made-up two-node map (numa.cpp): where the kernel answers
    # the placement query at all, every slice was asked about and the answers were what a one-node machine must give
    assert "slices asked where they live" in out
    # round 6: every fourth round gives the workers' handles a gang of frame-writing threads (cfg.host_threads = 5): shards in
    # chain mode over tiles with the frames written by the gang, independent streams decided ahead by it -- several handles'
    # gangs at work at once inside one driver
    import re
    m = re.search(r"(\d+) shards and (\d+) streams through a handle's gang", out)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, out
