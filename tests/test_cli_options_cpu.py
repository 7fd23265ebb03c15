"""The host program's command line, held to a recording: tests/golden/cli_options.grid is what the program printed BEFORE its
source was split by mode (tools/cli_identity.py --write-golden records it from a revision's program, never from the tree's) for
every prefix x every option with one -f and every ordered pair of options -- exit status, stdout and stderr of about 1400
command lines, none of which reaches the GPU runtime, so the result is the same with and without a GPU.  An option added later
cannot move an old message unnoticed."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from conftest import GOLDEN


def test_cli_options_print_what_the_recording_holds(capi, tmp_path):
    with open(os.path.join(GOLDEN, "cli_options.grid")) as f:
        rec = json.load(f)
    texts = rec["texts"]
    assert len(rec["cases"]) >= 1400

    def run(case):
        args, status, out, err = case
        p = subprocess.run([rec["argv0"]] + args, executable=capi.CLI_PATH, cwd=tmp_path, capture_output=True, stdin=subprocess.DEVNULL, timeout=60)
        return None if (p.returncode, p.stdout.decode(), p.stderr.decode()) == (status, texts[out], texts[err]) else \
            (args, status, texts[err], p.returncode, p.stderr.decode(), p.stdout.decode() == texts[out])

    with ThreadPoolExecutor(16) as pool:
        wrong = [w for w in pool.map(run, rec["cases"]) if w]
    assert not wrong, (len(wrong), wrong[:5])
    assert os.listdir(tmp_path) == []   # (a command line that is turned away writes nothing)


def test_cli_leaves_in_order_while_its_reader_thread_is_at_work(capi, tmp_path):
    """A run that fails after the reader thread has started -- an unusable peer address here, before any GPU call -- returns
    through main and a normal exit while that thread is still filling the ring: the ring has to outlive the function that
    started it.  Status 255 and the one message, every time; the file is sparse and long enough to keep the reader busy."""
    big = tmp_path / "zeros.u16"
    with open(big, "wb") as f:
        f.truncate(512 << 20)
    for flag in ["-s", "-l"] * 8:
        p = subprocess.run([capi.CLI_PATH, flag, "[::1", "-f", str(big)], capture_output=True, timeout=60)
        assert (p.returncode, p.stdout, p.stderr) == (255, b"", b"Invalid IPV6 address\n"), flag
