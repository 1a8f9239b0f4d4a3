"""Exact-rational evaluation of the ABBA-BABA site patterns of every ingroup trio against an outgroup, with the -minind
predicate over the four populations: the definition of pgt_dstat_pops_reduce_dev (include/pgtwin.h), written out in
`fractions` (no rounding anywhere; the inputs are the float64 values the kernels read).  Writes tests/golden/dstat_exact.json:

    python tests/golden/make_dstat_exact.py

5 populations (4 ingroup, the last the outgroup: 4 trios) x 200 sites (6-decimal frequencies, nInd uniform in 0 .. 20, so 0
and 1 occur; the outgroup is population 0 shifted by about 1e-3, so that ABBA and BABA of the trios with population 0 nearly
cancel), explicit windows (the whole range, every site alone, ragged ones), minind 1 and 5.  Every sum is stored as the
float64 nearest to the exact rational."""
import json
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES, N_POPS = 200, 5
OUT = N_POPS - 1
TRIOS = [(i, j, k) for i in range(OUT) for j in range(i + 1, OUT) for k in range(j + 1, OUT)]


def dstat_site(pi, pj, pk, po):
    """Fractions in, (bbaa, abba, baba) out: each pattern plus the pattern with the two alleles' roles swapped"""
    qi, qj, qk, qo = 1 - pi, 1 - pj, 1 - pk, 1 - po
    return (pi * pj * qk * qo + qi * qj * pk * po,
            qi * pj * pk * qo + pi * qj * qk * po,
            pi * qj * pk * qo + qi * pj * qk * po)


def exact_sites(freqs, ninds, i, j, k, minind):
    """per site: None where the trio does not count the site, else the exact (bbaa, abba, baba)"""
    o = len(freqs) - 1
    out = []
    for s in range(len(freqs[i])):
        if all(int(ninds[x][s]) >= minind for x in (i, j, k, o)):
            out.append(dstat_site(*[Fraction(float(freqs[x][s])) for x in (i, j, k, o)]))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (bbaa, abba, baba, n) of the sites [lo, hi): exact rationals and the count"""
    took = [x for x in sites[lo:hi] if x is not None]
    return tuple(sum((x[c] for x in took), Fraction(0)) for c in range(3)) + (len(took),)


def inputs():
    rng = np.random.default_rng(20261020)
    f = [np.round(rng.uniform(0.05, 0.95, N_SITES), 6)]
    f += [np.round(rng.uniform(0, 1, N_SITES), 6) for _ in range(N_POPS - 2)]
    f.append(np.round(f[0] + rng.uniform(0.0008, 0.0012, N_SITES), 6))
    ninds = [rng.integers(0, 21, N_SITES).astype(np.int32) for _ in range(N_POPS)]
    pos = np.cumsum(rng.integers(1, 50, N_SITES)).astype(np.uint32)
    return pos, f, ninds


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
        trios = []
        for i, j, k in TRIOS:
            sites = exact_sites(freqs, ninds, i, j, k, minind)
            rows = [exact_window(sites, lo, hi) for lo, hi in win]
            trios.append({"trio": [i, j, k], "bbaa": [float(r[0]) for r in rows], "abba": [float(r[1]) for r in rows],
                          "baba": [float(r[2]) for r in rows], "n": [r[3] for r in rows]})
        cases.append({"minind": minind, "trios": trios})
    doc = {"source": "tests/golden/make_dstat_exact.py", "pos": pos.tolist(), "freq": [f.tolist() for f in freqs],
           "nind": [c.tolist() for c in ninds], "windows": win, "cases": cases}
    with open(os.path.join(HERE, "dstat_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
