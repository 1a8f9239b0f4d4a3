"""Writes tests/golden/pbs_jack_ref.json: the 60-digit block jackknife of PBS and PBSn1 (tests/pbs_jack_model.py: jack_ref) of the
65 537-block table of that module (synth_rows(65537, 2): two trios, six items each), floats as hex strings.  About ten seconds of
`decimal` arithmetic per trio, which is why it is recorded; everything smaller is evaluated in the tests.

    python tests/golden/make_pbs_jack_ref.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pbs_jack_model as model  # noqa: E402


def main():
    n_win, n_trios = model.GOLDEN_N_WIN, model.GOLDEN_TRIOS
    rows = model.synth_rows(n_win, n_trios)
    items = []
    for t in range(n_trios):
        items.append([{k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in r.items()} for r in model.jack_rows(rows[t], model.jack_ref)])
    with open(model.GOLDEN, "w") as f:
        json.dump({"n_win": n_win, "n_trios": n_trios, "digits": model.DIGITS, "items": items}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
