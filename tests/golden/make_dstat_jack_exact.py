"""Writes tests/golden/dstat_jack_exact.json: the exact-rational block jackknife (tests/dstat_jack_model.py: jack_exact) of the
4 096-block table of tests/dstat_jack_shapes.py (synth_rows(4096): 20 trios, three topologies each), floats as hex strings.
About a minute of integer arithmetic, which is why it is recorded; tests/test_dstat_jack_cpu.py re-evaluates one item of it.

    python tests/golden/make_dstat_jack_exact.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dstat_jack_model  # noqa: E402
import dstat_jack_shapes  # noqa: E402


def main():
    n_win = dstat_jack_shapes.GOLDEN_N_WIN
    rows = dstat_jack_shapes.synth_rows(n_win)
    items = []
    for t in range(dstat_jack_shapes.MAX_TRIOS):
        trio = []
        for r in dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_exact):
            trio.append({k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in r.items() if k != "var"})
        items.append(trio)
    with open(os.path.join(HERE, "dstat_jack_exact.json"), "w") as f:
        json.dump({"n_win": n_win, "n_trios": dstat_jack_shapes.MAX_TRIOS, "seed": 0, "items": items}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
