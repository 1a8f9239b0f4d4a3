"""Exact-rational evaluation of WCFst() (betaAFOutlier.R:405-417) with PER-SITE sample sizes and the -minind predicate of
dxyWindow.cpp:381: the spec of pgt_fst_pops_reduce_dev, written out line by line in `fractions` (no rounding anywhere; the
inputs are the float64 values the kernels read).  Writes tests/golden/wcfst_nind_exact.json:

    python tests/golden/make_wcfst_nind_exact.py

3 populations x 200 sites (6-decimal frequencies, nInd uniform in 0 .. 20; population 2 is population 0 shifted by about 1e-3,
so that a of pair (0, 2) is negative throughout), explicit windows, minind 1 and 5.  Every sum is stored as the float64
nearest to the exact rational."""
import json
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES, N_POPS = 200, 3
PAIRS = [(i, j) for i in range(N_POPS) for j in range(i + 1, N_POPS)]


def reynolds_var(f1, f2, n1, n2):
    """betaAFOutlier.R:406-412, literally; Fractions in, (a, b) out"""
    npool = n1 + n2
    fpool = n1 / npool * f1 + n2 / npool * f2
    alpha1 = 2 * f1 * (1 - f1)
    alpha2 = 2 * f2 * (1 - f2)
    b = (n1 * alpha1 + n2 * alpha2) / (npool - 1)
    a = (4 * n1 * (f1 - fpool) ** 2 + 4 * n2 * (f2 - fpool) ** 2 - b) / (4 * n1 * n2 / npool)
    return a, b


def exact_sites(freqs, ninds, i, j, minind):
    """per site: None where the pair does not count the site, else the exact (a, a + b) — the two columns WCFst returns"""
    out = []
    for s in range(len(freqs[i])):
        n1, n2 = int(ninds[i][s]), int(ninds[j][s])
        if n1 >= minind and n2 >= minind:
            a, b = reynolds_var(Fraction(float(freqs[i][s])), Fraction(float(freqs[j][s])), Fraction(n1), Fraction(n2))
            out.append((a, a + b))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (asum, bsum, n) of the sites [lo, hi): exact rationals and the count"""
    took = [x for x in sites[lo:hi] if x is not None]
    return sum((x[0] for x in took), Fraction(0)), sum((x[1] for x in took), Fraction(0)), len(took)


def inputs():
    rng = np.random.default_rng(20240905)
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
    doc = {"source": "tests/golden/make_wcfst_nind_exact.py", "pos": pos.tolist(), "freq": [f.tolist() for f in freqs],
           "nind": [c.tolist() for c in ninds], "windows": win, "cases": cases}
    with open(os.path.join(HERE, "wcfst_nind_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
