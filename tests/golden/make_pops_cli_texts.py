"""Record tests/golden/pops_cli_texts.json: exit code, stdout and stderr of every command line of tests/pops_cli_cases.py.

    python tests/golden/make_pops_cli_texts.py [--bin DIR] [--out PATH]

Run it with the tools (popgenomicstools_amd/bin, or --bin DIR) built from the commit whose texts are to be pinned (the fixture in
the tree was recorded on the parent of the commit that gave the five K-population tools one driver), never from the code a test
is about to judge with it.  No case opens a file or the device: no GPU is needed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import pops_cli_cases as cases  # noqa: E402


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(HERE, "pops_cli_texts.json")
    bin_dir = argv[argv.index("--bin") + 1] if "--bin" in argv else os.path.join(ROOT, "popgenomicstools_amd", "bin")
    doc = cases.run(bin_dir, cases.cases())
    for key, (code, _, err) in doc.items():
        assert code == (0 if key.endswith(": no arguments") else 255) and "Unable to open" not in err, (key, code, err)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc)} cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1:])
