"""Writes tests/golden/dstat_jack_u32_exact.json: the exact-rational block jackknife (tests/dstat_jack_model.py: jack_exact) of
the 4 097-block table of tests/special_inputs.py (jack_u32_rows: 4 trios, every used block weighted 0xFFFFFFFF), floats as hex
strings.  Ten seconds of integer arithmetic, recorded so that the GPU test need not repeat them;
tests/test_special_values_pops_cpu.py re-evaluates one trio of it.

    python tests/golden/make_dstat_jack_u32_exact.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dstat_jack_model  # noqa: E402
import special_inputs  # noqa: E402


def main():
    n_win = special_inputs.JACK_U32_GOLDEN_N_WIN
    rows = special_inputs.jack_u32_rows(n_win)
    items = []
    for t in range(special_inputs.JACK_U32_TRIOS):
        trio = []
        for r in dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_exact):
            trio.append({k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in r.items() if k != "var"})
        items.append(trio)
    with open(os.path.join(HERE, "dstat_jack_u32_exact.json"), "w") as f:
        json.dump({"n_win": n_win, "n_trios": special_inputs.JACK_U32_TRIOS, "seed": 1, "items": items}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
