#!/usr/bin/env python3
"""Regenerate tests/golden/special_tokens.json: tiny inputs whose value columns carry the tokens `nan`, `-nan`, `inf`, `-inf`.

The contract of the shipped hosts: such a token is the IEEE value, and the rows are what the reference's
arithmetic gives on that value — the oracle's text front end (`expected`).  The compiled, unmodified reference cannot read
these tokens (`ss >> double` fails: the field reads as 0 and the fields behind it keep stale values); what it prints is
recorded beside it (`reference`) for the record, as H4 / H6 are in dxy_hand_walked.json: it differs from `expected` only in
windows that hold such a token (tests/test_oracle_golden.py).  Runs only where oracle/_ref exists (`make -C oracle ref`).
Only data is committed.

    python tests/golden/make_special_tokens.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
import oracle_bind  # noqa: E402

XP_HEADER = "id\tpos\tgpos\tp1\tihh1\tp2\tihh2\txpehh\tnormxpehh\tcrit\n"


def ihs_text(sites):
    """sites: [(chromosome, position, score token)]"""
    return "".join(f"{c}_{p}\t{p}\t0.3\t1.1\t2.2\t0.5\t{s}\t0\n" for c, p, s in sites)


def xp_text(sites):
    return XP_HEADER + "".join(f"{c}_{p}\t{p}\t0.01\t0.3\t1.1\t0.2\t2.2\t0.5\t{s}\t0\n" for c, p, s in sites)


def fst_text(sites):
    """sites: [(chromosome, position, a token, b token)]"""
    return "".join(f"{c}\t{p}\t{a}\t{b}\n" for c, p, a, b in sites)


def sites_of(chrom, positions, tokens):
    return [(chrom, p, t) for p, t in zip(positions, tokens.split())]


PROBE_POS = [1, 2, 3, 11, 12, 13, 21, 22]
PROBE = sites_of("c1", PROBE_POS, "nan 1.5 -3 1 -nan inf nan nan")
LATER = sites_of("c1", PROBE_POS, "1.5 nan -3 -inf inf inf 2.5 -nan")
TWO = sites_of("c1", [2, 4, 6, 12], "-nan nan nan 0.5") + sites_of("c2", [1, 5, 11, 15, 25], "-inf -inf inf inf 1.25")

CASES = [
    ("ihsWindow", {"in.norm": ihs_text(PROBE)}, ["@in.norm", "-winsize", "10", "-cutoff", "2"], "the probe: first key NaN, NaN later, all NaN"),
    ("ihsWindow", {"in.norm": ihs_text(LATER), "len.txt": "c1\t45\n"}, ["@in.norm", "-winsize", "10", "-cutoff", "2", "-chrlen", "@len.txt"],
     "NaN only later, |-inf| = |inf| tie (first occurrence), trailing empty windows"),
    ("ihsWindow", {"in.norm": ihs_text(TWO)}, ["@in.norm", "-winsize", "10", "-cutoff", "0.5"], "two chromosomes; an all-NaN window"),
    ("xpehhWindow", {"in.norm": xp_text(PROBE)}, ["@in.norm", "2", "-winsize", "10"], "the probe, maximum"),
    ("xpehhWindow", {"in.norm": xp_text(PROBE)}, ["@in.norm", "-2", "-winsize", "10"], "the probe, minimum"),
    ("xpehhWindow", {"in.norm": xp_text(TWO)}, ["@in.norm", "2", "-winsize", "10"], "an all -inf window under the maximum"),
    ("xpehhWindow", {"in.norm": xp_text(TWO)}, ["@in.norm", "-2", "-winsize", "10"], "an all +inf window under the minimum"),
    ("xpehhWindow", {"in.norm": xp_text(LATER), "len.txt": "c1\t30\n"}, ["@in.norm", "-1.5", "-winsize", "10", "-chrlen", "@len.txt"],
     "minimum: -inf first, NaN later"),
    ("fstWindow", {"in.txt": fst_text([("c1", 1, "0.25", "0.5"), ("c1", 2, "nan", "0.5"), ("c1", 3, "0.125", "0.25"), ("c1", 4, "0.5", "1"),
                                       ("c1", 5, "0.25", "-nan"), ("c1", 6, "0.75", "1"), ("c1", 7, "0.25", "0.5"), ("c1", 8, "0.5", "0.5")])},
     ["@in.txt", "2", "1"], "NaN in a and in b"),
    ("fstWindow", {"in.txt": fst_text([("c1", 1, "inf", "0.5"), ("c1", 2, "0.5", "0.5"), ("c1", 3, "0.25", "inf"), ("c1", 4, "0.5", "1"),
                                       ("c1", 5, "-inf", "inf"), ("c1", 6, "0.75", "1"), ("c1", 7, "0.25", "-inf"), ("c1", 8, "0.5", "0.5"),
                                       ("c2", 1, "inf", "0"), ("c2", 2, "-inf", "0"), ("c2", 3, "0.5", "0.25"), ("c2", 4, "0.25", "0.25")])},
     ["@in.txt", "2", "2"], "infinities: x / inf, inf / inf, inf - inf, a zero denominator under an infinite numerator"),
    ("fstWindow", {"in.txt": fst_text([("c1", p, a, b) for p, (a, b) in enumerate(
        [("0.5", "1"), ("0.25", "1"), ("-nan", "1"), ("0.5", "1"), ("0.25", "1"), ("0.5", "1"), ("0.25", "inf"), ("0.5", "1"), ("0.25", "1"), ("0.5", "1")], 1)])},
     ["@in.txt", "3", "1"], "windows before, across and behind a token"),
]


def oracle_tsv(oracle, tool, files, args):
    d = tempfile.mkdtemp()
    try:
        paths = {}
        for k, v in files.items():
            paths[k] = os.path.join(d, k)
            open(paths[k], "w").write(v)
        out = os.path.join(d, "out.tsv")
        chrlen = paths[args[args.index("-chrlen") + 1][1:]] if "-chrlen" in args else None
        if tool == "fstWindow":
            rc = oracle.fst_text(paths["in.txt"], int(args[1]), int(args[2]), out)
        elif tool == "ihsWindow":
            rc = oracle.ihs_text(paths["in.norm"], int(args[args.index("-winsize") + 1]), float(args[args.index("-cutoff") + 1]), chrlen, out)
        else:
            rc = oracle.xpehh_text(paths["in.norm"], float(args[1]), int(args[args.index("-winsize") + 1]), chrlen, out)
        assert rc == 0, (tool, args, rc)
        return open(out).read()
    finally:
        for f in os.listdir(d):
            os.unlink(os.path.join(d, f))
        os.rmdir(d)


def main():
    for tool in ("fstWindow", "ihsWindow", "xpehhWindow"):
        if not os.path.exists(os.path.join(make_golden.REF, tool)):
            sys.exit("oracle/_ref is missing: run `make -C oracle ref` where the reference sources exist")
    oracle = oracle_bind.load()
    out = []
    for tool, files, args, note in CASES:
        stdout, rc = make_golden.run_ref_args(tool, files, args)
        again, _ = make_golden.run_ref_args(tool, files, args)
        assert stdout == again, (tool, note, "the reference's own output is not reproducible")
        out.append({"tool": tool, "note": note, "files": files, "args": args, "expected": oracle_tsv(oracle, tool, files, args),
                    "reference": {"stdout": stdout, "rc": rc}})
    json.dump({"source": "expected = the oracle's text front ends (oracle/window_oracle.c) on inputs with nan / -nan / inf / -inf tokens: the "
                         "hosts' contract.  reference = what the unmodified reference binaries (oracle/_ref) print for the same input, "
                         "for the record: they cannot read these tokens (the field reads as 0).",
               "cases": out}, open(os.path.join(HERE, "special_tokens.json"), "w"), indent=1)
    print(f"wrote special_tokens.json ({len(out)} cases)")


if __name__ == "__main__":
    main()
