"""GPU: every refusal of the K-population entry points (pgt_{dxy,fst,pi}_pops_reduce_dev, pgt_{dxy,fst,pi}_pops_reduce and the
Python device wrappers) — return code and FULL message, byte for byte, against tests/golden/pops_messages.json, which was
recorded on the commit before the three statistics came to share one checker.  The statistics' own refusal tests look for the
argument's name in the message; this one notices a reworded message or two checks changing places."""
import json
import os

import pytest

import pops_message_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pops_messages.json")


def test_refusals_keep_code_and_words(pgt, ctx):
    import torch
    with open(GOLDEN) as f:
        want = json.load(f)["gpu"]
    todo, keep = cases.gpu_cases(pgt, ctx)
    got = cases.run(todo)
    torch.cuda.synchronize()
    del keep
    assert sorted(got) == sorted(want)
    accepted = [key for key in got if got[key][0] == 0]
    assert accepted == ["pgt_dxy_pops_reduce: minind=0"]  # the one call of the list that the C ABI takes (PGT_OK)
    for key in want:
        assert got[key] == want[key], key
    for key, (code, msg) in want.items():  # the fixture itself: a message that names an entry point names the one that was called
        stat = key.split("_pops_reduce")[0].split(".")[-1].replace("pgt_", "")
        assert "_pops_reduce" not in msg or f"{stat}_pops_reduce" in msg, (key, msg)
