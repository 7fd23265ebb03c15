"""The capture calls over every sample flavour against what the library answered BEFORE the flavours had one definition
(csrc/flavour.hpp): tools/abi_identity.py's rows -- every refusal alone and next to its neighbour, every format number through every
_as and _iq call, captures of 0 .. 64 samples alone and in batches -- replayed against tests/golden/flavour/flavour_answers.json, which that
tool recorded from the parent revision's library (--write-golden), never from the tree under test.  Per row (the device and the host entry points): the return value, the
text of adsb_last_error, a digest of every output array and the format report; per handle, the frames of a plain decode behind its
last call."""
import json

import pytest

from test_gpu_power import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_every_row_answers_as_the_parent_did(capi, torch_cuda):
    from tools import abi_identity as A
    with open(A.GOLDEN) as f:
        gold = json.load(f)
    got = A.record()
    want = A.unpack(gold, got["rows"])   # (asserts that rows() names the rows that were recorded)
    differing = []
    for g, w in zip(got["rows"], want["rows"]):
        g_text, w_text = got["texts"][g[3]], want["texts"][w[3]]
        if (g[2], g_text, g[4][:12], g[5]) != (w[2], w_text, w[4], w[5]):
            differing.append((g[0], g[1], (w[2], w_text, w[4:]), (g[2], g_text, g[4:])))
    assert len(got["rows"]) == len(want["rows"]) and not differing, (len(differing), differing[:5])
    state = lambda rec: {k: (v[0], rec["texts"][v[1]], v[2]) for k, v in rec["states"].items()}
    assert state(got) == state(want)
    # the recording is not an empty one: refusals, answers, conversions that were counted, host entry points
    rows = want["rows"]
    assert len(rows) > 850 and sum(1 for w in rows if w[2] < 0) > 300 and sum(1 for w in rows if w[2] > 0) > 100
    assert sum(1 for w in rows if any(w[5][1:])) > 50 and sum(1 for w in rows if "_host" in w[1]) > 100
