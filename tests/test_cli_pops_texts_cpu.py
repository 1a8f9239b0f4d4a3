"""CPU: what the five K-population tools (dxy / fst / pi / dstat / f3 WindowPops) say before they open a file or touch the device
— the help texts, the refusals of the shared and of each tool's own options, and the order in which they come — exit code,
stdout and stderr byte for byte against tests/golden/pops_cli_texts.json (recorded on the commit before the five `main`s came to
share one driver: a substring check would not notice a reworded text or two refusals changing places)."""
import json
import os

import pytest

import pops_cli_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pops_cli_texts.json")


@pytest.fixture(scope="module")
def bin_dir():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(ROOT, "popgenomicstools_amd", "bin")


def test_texts_before_any_file_is_opened(bin_dir):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = cases.run(bin_dir, cases.cases())
    assert sorted(got) == sorted(want)
    assert len(got) == 5 * 14 + (2 * 7 + 3) + (2 + 4) + (2 + 4)  # shared, -jackknife, -fd, -estimator
    for key in want:
        assert got[key] == want[key], key
        if key.endswith(": no arguments"):  # the whole help text on stdout
            assert got[key][0] == 0 and got[key][2] == "" and got[key][1].count("\n") > 30, key
        else:  # a refusal: one line on stderr, nothing on stdout
            assert got[key][0] == 255 and got[key][1] == "" and got[key][2].count("\n") == 1, key
