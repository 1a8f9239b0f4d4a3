"""Exact-rational evaluation of Hudson's FST as a ratio of averages with PER-SITE sample sizes and the -minind predicate: the
definition of pgt_fst_hudson_pops_reduce_dev (include/pgtwin.h), written out in `fractions` (no rounding anywhere; the inputs
are the float64 values the kernels read).  Writes tests/golden/hudson_exact.json:

    python tests/golden/make_hudson_exact.py

3 populations x 200 sites (6-decimal frequencies, nInd uniform in 0 .. 20, so 0 and 1 occur; population 2 is population 0
shifted by about 1e-3, so that the numerator of pair (0, 2) is negative throughout), explicit windows (the whole range, every
site alone, ragged ones), minind 1 and 5.  Every sum is stored as the float64 nearest to the exact rational."""
import json
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES, N_POPS = 200, 3
PAIRS = [(i, j) for i in range(N_POPS) for j in range(i + 1, N_POPS)]


def hudson_site(p1, p2, n1, n2):
    """Fractions in, (num, den) out: num = (p1-p2)^2 - h1 - h2 with h = p(1-p)/(2n-1); den = p1(1-p2) + p2(1-p1)"""
    h1 = p1 * (1 - p1) / (2 * n1 - 1)
    h2 = p2 * (1 - p2) / (2 * n2 - 1)
    return (p1 - p2) ** 2 - h1 - h2, p1 * (1 - p2) + p2 * (1 - p1)


def exact_sites(freqs, ninds, i, j, minind):
    """per site: None where the pair does not count the site, else the exact (num, den)"""
    out = []
    for s in range(len(freqs[i])):
        n1, n2 = int(ninds[i][s]), int(ninds[j][s])
        if n1 >= minind and n2 >= minind:
            out.append(hudson_site(Fraction(float(freqs[i][s])), Fraction(float(freqs[j][s])), Fraction(n1), Fraction(n2)))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (asum, bsum, n) of the sites [lo, hi): exact rationals and the count"""
    took = [x for x in sites[lo:hi] if x is not None]
    return sum((x[0] for x in took), Fraction(0)), sum((x[1] for x in took), Fraction(0)), len(took)


def inputs():
    rng = np.random.default_rng(20261019)
    f0 = np.round(rng.uniform(0.05, 0.95, N_SITES), 6)
    f1 = np.round(rng.uniform(0, 1, N_SITES), 6)
    f2 = np.round(f0 + rng.uniform(0.0008, 0.0012, N_SITES), 6)
    ninds = [rng.integers(0, 21, N_SITES).astype(np.int32) for _ in range(N_POPS)]
    pos = np.cumsum(rng.integers(1, 50, N_SITES)).astype(np.uint32)
    return pos, [f0, f1, f2], ninds


def windows():
    w = [(s, s + 1) for s in range(N_SITES)]                              # every site alone
    w += [(lo, min(lo + 7, N_SITES)) for lo in range(0, N_SITES - 3, 3)]   # 7 sites, step 3
    w += [(0, N_SITES), (0, 128), (64, 192), (13, 13), (199, 200), (37, 150)]
    return w


def main():
    pos, freqs, ninds = inputs()
    win = windows()
    cases = []
    for minind in (1, 5):
        pairs = []
        for i, j in PAIRS:
            sites = exact_sites(freqs, ninds, i, j, minind)
            rows = [exact_window(sites, lo, hi) for lo, hi in win]
            pairs.append({"pair": [i, j], "asum": [float(r[0]) for r in rows], "bsum": [float(r[1]) for r in rows], "n": [r[2] for r in rows]})
        cases.append({"minind": minind, "pairs": pairs})
    doc = {"source": "tests/golden/make_hudson_exact.py", "pos": pos.tolist(), "freq": [f.tolist() for f in freqs],
           "nind": [c.tolist() for c in ninds], "windows": win, "cases": cases}
    with open(os.path.join(HERE, "hudson_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
