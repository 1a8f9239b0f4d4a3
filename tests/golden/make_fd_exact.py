"""Exact-rational evaluation of f_d's and f_dM's three per-site terms (num, fd_den, fdm_den) of every ingroup trio
((P1 = i, P2 = j), P3 = k) against an outgroup, with the -minind predicate over the four populations: the definition of
pgt_fd_pops_reduce_dev (include/pgtwin.h), written out in `fractions` (no rounding anywhere; the inputs are the float64 values
the kernels read).  Writes tests/golden/fd_exact.json:

    python tests/golden/make_fd_exact.py

5 populations (4 ingroup, the last the outgroup: 4 trios) x 200 sites, 6-decimal frequencies uniform in [0, 1] with about one
site in eight set to exactly 0 or 1 in every population, the outgroup fixed (0 or 1) at half of its sites and polymorphic at the
rest; runs of sites where two ingroup populations carry the SAME frequency (every pair: each trio meets p_i == p_j, p_j == p_k
and p_i == p_k); nInd uniform in 0 .. 20.  Explicit windows (the whole range, every site alone, ragged ones), minind 1 and 5.
Every sum is stored as the float64 nearest to the exact rational."""
import json
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES, N_POPS = 200, 5
OUT = N_POPS - 1
TRIOS = [(i, j, k) for i in range(OUT) for j in range(i + 1, OUT) for k in range(j + 1, OUT)]
PAIRS = [(a, b) for a in range(OUT) for b in range(a + 1, OUT)]
TIE_RUN = 6  # sites per tied pair: sites 20 + 6 m .. 20 + 6 m + 5 carry f[b] = f[a] for PAIRS[m]


def fd_site(pi, pj, pk, po):
    """Fractions in, (num, fd_den, fdm_den) out, line by line as the definition has them"""
    qi, qj, qk, qo = 1 - pi, 1 - pj, 1 - pk, 1 - po
    abba = qi * pj * pk * qo + pi * qj * qk * po
    baba = pi * qj * pk * qo + qi * pj * qk * po
    pH, qH = (pj, qj) if pj >= pk else (pk, qk)
    pL, qL = (pj, qj) if pj <= pk else (pk, qk)
    pG, qG = (pi, qi) if pi >= pk else (pk, qk)
    pS, qS = (pi, qi) if pi <= pk else (pk, qk)
    B1 = (qi * pH) * (pH * qo) - (pi * qH) * (pH * qo)
    A1 = (pi * qL) * (qL * po) - (qi * pL) * (qL * po)
    B2 = (pG * qj) * (pG * qo) - (qG * pj) * (pG * qo)
    A2 = (qS * pj) * (qS * po) - (pS * qj) * (qS * po)
    return abba - baba, B1 + A1, (B1 if pj >= pi else B2) + (A1 if pj <= pi else A2)


def exact_sites(freqs, ninds, i, j, k, minind):
    """per site: None where the trio does not count the site, else the exact (num, fd_den, fdm_den)"""
    o = len(freqs) - 1
    out = []
    for s in range(len(freqs[i])):
        if all(int(ninds[x][s]) >= minind for x in (i, j, k, o)):
            out.append(fd_site(*[Fraction(float(freqs[x][s])) for x in (i, j, k, o)]))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (num, fd_den, fdm_den, n) of the sites [lo, hi): exact rationals and the count"""
    took = [x for x in sites[lo:hi] if x is not None]
    return tuple(sum((x[c] for x in took), Fraction(0)) for c in range(3)) + (len(took),)


def inputs():
    rng = np.random.default_rng(20261021)
    f = [np.round(rng.uniform(0, 1, N_SITES), 6) for _ in range(N_POPS)]
    for x in f:  # exact 0 and 1 in every population
        u = rng.uniform(0, 1, N_SITES)
        x[u < 1 / 16] = 0.0
        x[u > 15 / 16] = 1.0
    u = rng.uniform(0, 1, N_SITES)  # the outgroup: fixed ancestral, fixed derived, or polymorphic
    f[OUT][u < 0.35] = 0.0
    f[OUT][u > 0.85] = 1.0
    for m, (a, b) in enumerate(PAIRS):  # ties between every two ingroup populations
        s = slice(20 + TIE_RUN * m, 20 + TIE_RUN * (m + 1))
        f[b][s] = f[a][s]
    ninds = [rng.integers(0, 21, N_SITES).astype(np.int32) for _ in range(N_POPS)]
    for c in ninds:  # most tie sites are counted under both minind
        c[20:20 + TIE_RUN * len(PAIRS):2] = 20
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
            trios.append({"trio": [i, j, k], "num": [float(r[0]) for r in rows], "fd_den": [float(r[1]) for r in rows],
                          "fdm_den": [float(r[2]) for r in rows], "n": [r[3] for r in rows]})
        cases.append({"minind": minind, "trios": trios})
    doc = {"source": "tests/golden/make_fd_exact.py", "pos": pos.tolist(), "freq": [f.tolist() for f in freqs],
           "nind": [c.tolist() for c in ninds], "windows": win, "cases": cases}
    with open(os.path.join(HERE, "fd_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
