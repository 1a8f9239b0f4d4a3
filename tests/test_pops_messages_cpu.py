"""CPU: the refusals of dxy_window, dxy_window_pops, fst_window_pops and pi_window_pops that come before a context is opened —
return code and FULL message against tests/golden/pops_messages.json (recorded on the commit before the three functions came to
share one body: a substring check would not notice a reworded message or two checks changing places)."""
import json
import os

import pops_message_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pops_messages.json")


def test_refusals_before_the_device_keep_code_and_words():
    with open(GOLDEN) as f:
        want = json.load(f)["cpu"]
    got = cases.run(cases.cpu_cases())
    assert sorted(got) == sorted(want)
    assert len(got) == 4 + 3 * 7
    for key in want:
        assert got[key] == want[key], key
        assert got[key][0] != 0, key  # every one of these is a refusal
