"""The inputs of the two randomised reference checks, and the SHA-256 of what the unmodified reference tools print for each:
tests/test_oracle_golden.py::test_live_reference_fuzz (oracle port vs reference) and
tests/test_cli.py::test_cli_live_against_the_reference_binaries (retained hosts vs reference).

    make -C oracle ref && python tests/golden/make_ref_sha256.py      (writes tests/golden/ref_sha256.json)

The inputs are generated from fixed seeds (make_golden's generators), so only their hashes and the reference's are stored.
Where oracle/_ref is absent the checks still hold: the oracle port's output for every case must hash to the reference's
stored SHA-256 (so it IS the reference's output, byte for byte), and the hosts are compared with that output.  Where the
compiled reference is present it is run as well and must print the stored bytes.
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

FIXTURE = os.path.join(HERE, "ref_sha256.json")


def _case(key, tool, files, args):
    return {"key": key, "tool": tool, "files": files, "args": args}


def oracle_fuzz_cases():
    """test_live_reference_fuzz: 80 small fstWindow / hetWindow runs."""
    rng = random.Random(99)
    for i in range(80):
        tool = rng.choice(["fstWindow", "hetWindow"])
        text, W, S = mg.random_case(rng, tool)
        yield _case(f"fuzz{i}", tool, {"in.txt": text}, ["@in.txt", str(W), str(S)])


# S << W with windows of two and more level-2 tiles: the group query (steps 1 .. 1024), the sliding query (short windows,
# steps up to 32) and one wave per window, each against the reference's own re-summation (fstWindow.cpp:80-83,95-99)
LARGE = ((60_000, 3, 20_000, 1), (90_000, 2, 16_384, 7), (150_000, 4, 50_000, 100), (150_000, 1, 24_577, 64),
         (200_000, 5, 30_000, 1000), (30_000, 2, 3_000, 5), (200_000, 3, 50_000, 2500), (400_000, 2, 140_000, 300))


def cli_cases():
    """test_cli_live_against_the_reference_binaries: small fstWindow / hetWindow runs, ihsWindow / xpehhWindow runs, and
    larger fstWindow + hetWindow tables with S << W (kind "large")."""
    import synth
    rng = random.Random(20261004)
    k = 0
    for tool in ("fstWindow", "hetWindow"):
        for _ in range(15):
            text, W, S = mg.random_case(rng, tool, max_chr=6, max_sites=60, max_w=25)
            yield dict(_case(f"cli{k}", tool, {"in.txt": text}, ["@in.txt", str(W), str(S)]), kind="small")
            k += 1
    for tool in ("ihsWindow", "xpehhWindow"):
        for _ in range(12):
            files, args = mg.extreme_case(rng, tool, max_chr=5, max_sites=60)
            yield dict(_case(f"cli{k}", tool, files, args), kind="extreme")
            k += 1
    nrng = np.random.default_rng(20261004)
    for n, n_chr, W, S in LARGE:
        chr_ids, pos = synth.chromosomes(nrng, n, n_chr, equal=False)
        a_, b_ = synth.fst_columns(nrng, n)
        g_ = synth.het_column(nrng, n)
        fst = "".join(f"chr{c}\t{p}\t{x:.6f}\t{y:.6f}\n" for c, p, x, y in zip(chr_ids, pos, a_, b_))
        het = "".join(f"chr{c}\t{p}\t{v}\n" for c, p, v in zip(chr_ids, pos, g_))
        yield dict(_case(f"cli{k}", "fstWindow", {"big.txt": fst}, ["@big.txt", str(W), str(S)]), kind="large")
        yield dict(_case(f"cli{k + 1}", "hetWindow", {"big.het.txt": het}, ["@big.het.txt", str(W), str(S)]), kind="large")
        k += 2


def input_sha256(case):
    h = hashlib.sha256()
    for name in sorted(case["files"]):
        h.update(name.encode() + b"\0" + case["files"][name].encode() + b"\0")
    h.update("\0".join(case["args"]).encode())
    return h.hexdigest()


def materialise(case, d):
    """Write the case's files into directory d -> argv after the tool name."""
    for name, text in case["files"].items():
        with open(os.path.join(str(d), name), "w") as fh:
            fh.write(text)
    return [os.path.join(str(d), a[1:]) if a.startswith("@") else a for a in case["args"]]


def oracle_stdout(oracle, case, d):
    """(rc, stdout) of the oracle port (oracle/liboracle.so) for the case, its files written into directory d."""
    argv = materialise(case, d)
    out = os.path.join(str(d), "oracle.out")
    tool = case["tool"]
    if tool in ("fstWindow", "hetWindow"):
        rc = (oracle.fst_text if tool == "fstWindow" else oracle.het_text)(argv[0], int(argv[1]), int(argv[2]), out)
    else:
        a = case["args"]
        W = int(a[a.index("-winsize") + 1])
        chrlen = argv[a.index("-chrlen") + 1] if "-chrlen" in a else None
        if tool == "ihsWindow":
            rc = oracle.ihs_text(argv[0], W, float(a[a.index("-cutoff") + 1]), chrlen, out)
        else:
            rc = oracle.xpehh_text(argv[0], float(a[1]), W, chrlen, out)
    with open(out) as fh:
        text = fh.read()
    os.unlink(out)
    return rc, text


def sha256(text):
    return hashlib.sha256(text.encode() if isinstance(text, str) else text).hexdigest()


def load():
    with open(FIXTURE) as fh:
        return json.load(fh)["cases"]


def main():
    ref_dir = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref")
    cases = {}
    for case in list(oracle_fuzz_cases()) + list(cli_cases()):
        exe = os.path.join(ref_dir, case["tool"])
        if not os.path.exists(exe):
            sys.exit(f"{exe} is missing: run `make -C oracle ref` where the reference sources are")
        d = tempfile.mkdtemp()
        try:
            r = subprocess.run([exe] + materialise(case, d), capture_output=True, timeout=300)
        finally:
            for name in os.listdir(d):
                os.unlink(os.path.join(d, name))
            os.rmdir(d)
        cases[case["key"]] = {"tool": case["tool"], "input_sha256": input_sha256(case), "rc": r.returncode,
                              "stdout_sha256": sha256(r.stdout), "stdout_lines": r.stdout.count(b"\n")}
    with open(FIXTURE, "w") as fh:
        json.dump({"generator": "tests/golden/make_ref_sha256.py (reference binaries built by oracle/Makefile)", "cases": cases},
                  fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"wrote {FIXTURE}: {len(cases)} cases")


if __name__ == "__main__":
    main()
