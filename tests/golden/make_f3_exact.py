"""Exact-rational evaluation of f3's three per-site terms of every trio i < j < k of ALL populations, each population of the trio
as the target, with the -minind predicate over the trio's three populations: the definition of pgt_f3_pops_reduce_dev
(include/pgtwin.h), written out in `fractions` (no rounding anywhere; the inputs are the float64 values the kernels read).
Writes tests/golden/f3_exact.json:

    python tests/golden/make_f3_exact.py

Two input sets, K = 3 (1 trio) and K = 4 (4 trios), 96 sites each: 6-decimal frequencies uniform in [0, 1] with about one site
in eight set to exactly 0 or 1, a run of sites where two populations carry the SAME frequency (every pair), nInd uniform in
0 .. 20.  Explicit windows (the whole range, every site alone, ragged ones), minind 1 and 5.  Every sum is stored as the
float64 nearest to the exact rational (Python's int / int is correctly rounded)."""
import json
import os
import random
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES = 96
TIE_RUN = 4  # sites per tied pair: sites 10 + 4 m .. 10 + 4 m + 3 carry f[b] = f[a] for pair m


def trios_of(n_pops):
    return [(i, j, k) for i in range(n_pops) for j in range(i + 1, n_pops) for k in range(j + 1, n_pops)]


def f3_site(p, n):
    """p, n: the trio's three frequencies (Fractions) and counts (ints) -> (f3(i; j,k), f3(j; i,k), f3(k; i,j))"""
    h = [x * (1 - x) / (2 * c - 1) for x, c in zip(p, n)]
    (pi, pj, pk) = p
    return ((pi - pj) * (pi - pk) - h[0], (pj - pi) * (pj - pk) - h[1], (pk - pi) * (pk - pj) - h[2])


def exact_sites(freqs, ninds, trio, minind):
    """per site: None where the trio does not count the site, else the three exact terms"""
    out = []
    for s in range(N_SITES):
        if all(ninds[x][s] >= minind for x in trio):
            out.append(f3_site([Fraction(freqs[x][s]) for x in trio], [ninds[x][s] for x in trio]))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    took = [x for x in sites[lo:hi] if x is not None]
    return tuple(sum((x[c] for x in took), Fraction(0)) for c in range(3)) + (len(took),)


def nearest(q):
    return q.numerator / q.denominator


def inputs(n_pops, seed):
    rng = random.Random(seed)
    f = [[round(rng.uniform(0, 1), 6) for _ in range(N_SITES)] for _ in range(n_pops)]
    for x in f:
        for s in range(N_SITES):
            u = rng.random()
            if u < 1 / 16:
                x[s] = 0.0
            elif u > 15 / 16:
                x[s] = 1.0
    pairs = [(a, b) for a in range(n_pops) for b in range(a + 1, n_pops)]
    for m, (a, b) in enumerate(pairs):
        for s in range(10 + TIE_RUN * m, 10 + TIE_RUN * (m + 1)):
            f[b][s] = f[a][s]
    ninds = [[rng.randint(0, 20) for _ in range(N_SITES)] for _ in range(n_pops)]
    pos, at = [], 0
    for _ in range(N_SITES):
        at += rng.randint(1, 49)
        pos.append(at)
    return pos, f, ninds


def windows():
    w = [[s, s + 1] for s in range(N_SITES)]                                # every site alone
    w += [[lo, min(lo + 7, N_SITES)] for lo in range(0, N_SITES - 3, 3)]     # 7 sites, step 3
    w += [[0, N_SITES], [0, 64], [32, 96], [13, 13], [95, 96], [37, 80]]
    return w


def main():
    win = windows()
    sets = []
    for n_pops, seed in ((3, 20261020), (4, 20261021)):
        pos, freqs, ninds = inputs(n_pops, seed)
        cases = []
        for minind in (1, 5):
            trios = []
            for trio in trios_of(n_pops):
                sites = exact_sites(freqs, ninds, trio, minind)
                rows = [exact_window(sites, lo, hi) for lo, hi in win]
                trios.append({"trio": list(trio), "f3_i": [nearest(r[0]) for r in rows], "f3_j": [nearest(r[1]) for r in rows],
                              "f3_k": [nearest(r[2]) for r in rows], "n": [r[3] for r in rows]})
            cases.append({"minind": minind, "trios": trios})
        sets.append({"n_pops": n_pops, "pos": pos, "freq": freqs, "nind": ninds, "cases": cases})
    doc = {"source": "tests/golden/make_f3_exact.py", "windows": win, "sets": sets}
    with open(os.path.join(HERE, "f3_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
