"""Exact-rational evaluation of the per-site nucleotide diversity pgt_pi_pops_reduce_dev defines (include/pgtwin.h):
    counted = nind >= minind;   pi = 2 p (1 - p) * 2 nind / (2 nind - 1)
written out in `fractions` (no rounding anywhere; the inputs are the float64 values the kernels read).  Writes
tests/golden/pi_exact.json:

    python tests/golden/make_pi_exact.py

3 populations x 200 sites (6-decimal frequencies, nInd uniform in 0 .. 20; population 2 has small counts, 0 .. 3, where the
finite-sample factor is largest), explicit windows, minind 1 and 5.  Every sum is stored as the float64 nearest to the
exact rational."""
import json
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES, N_POPS = 200, 3


def exact_sites(freq, nind, minind):
    """per site: None where the population does not count the site, else the exact pi"""
    out = []
    for p, n in zip(freq, nind):
        n = int(n)
        if n >= minind:
            p = Fraction(float(p))
            out.append(2 * p * (1 - p) * Fraction(2 * n, 2 * n - 1))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (sum, neff) of the sites [lo, hi): the exact rational and the count"""
    took = [x for x in sites[lo:hi] if x is not None]
    return sum(took, Fraction(0)), len(took)


def inputs():
    rng = np.random.default_rng(20241018)
    freqs = [np.round(rng.uniform(0, 1, N_SITES), 6) for _ in range(N_POPS)]
    freqs[1][:4] = [0.0, 1.0, 0.5, 0.000001]
    ninds = [rng.integers(0, 21, N_SITES).astype(np.int32) for _ in range(N_POPS - 1)] + [rng.integers(0, 4, N_SITES).astype(np.int32)]
    pos = np.cumsum(rng.integers(1, 50, N_SITES)).astype(np.uint32)
    return pos, freqs, ninds


def windows():
    w = [(s, s + 1) for s in range(0, N_SITES, 9)]                           # single sites
    w += [(lo, min(lo + 7, N_SITES)) for lo in range(0, N_SITES - 3, 31)]     # 7 sites
    w += [(0, N_SITES), (0, 128), (64, 192), (13, 13), (199, 200), (37, 150)]
    return w


def main():
    pos, freqs, ninds = inputs()
    win = windows()
    cases = []
    for minind in (1, 5):
        pops = []
        for k in range(N_POPS):
            sites = exact_sites(freqs[k], ninds[k], minind)
            rows = [exact_window(sites, lo, hi) for lo, hi in win]
            pops.append({"pop": k, "sum": [float(r[0]) for r in rows], "neff": [r[1] for r in rows]})
        cases.append({"minind": minind, "pops": pops})
    doc = {"source": "tests/golden/make_pi_exact.py", "pos": pos.tolist(), "freq": [f.tolist() for f in freqs],
           "nind": [c.tolist() for c in ninds], "windows": win, "cases": cases}
    with open(os.path.join(HERE, "pi_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
