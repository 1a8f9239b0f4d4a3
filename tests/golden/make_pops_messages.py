"""Record tests/golden/pops_messages.json: (return code, full message) of every refused call of tests/pops_message_cases.py.

    python tests/golden/make_pops_messages.py [--out PATH]

Run it on the commit whose wording is to be pinned (the fixture in the tree was recorded on the parent of the commit that
merged the three K-population entry points' checkers), never on the code a test is about to judge with it.  The "cpu" section
needs no GPU; the "gpu" section is recorded where a device is present and otherwise carried over from the existing file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pops_message_cases as cases  # noqa: E402


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(HERE, "pops_messages.json")
    doc = {"cpu": cases.run(cases.cpu_cases())}
    import torch
    if torch.cuda.is_available():
        import popgenomicstools_amd as pgt
        with pgt.Context() as ctx:
            gpu, keep = cases.gpu_cases(pgt, ctx)
            doc["gpu"] = cases.run(gpu)
            torch.cuda.synchronize()
            del keep
    else:
        existing = os.path.join(HERE, "pops_messages.json")
        doc["gpu"] = json.load(open(existing))["gpu"] if os.path.exists(existing) else {}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cpu'])} cpu and {len(doc['gpu'])} gpu cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1:])
