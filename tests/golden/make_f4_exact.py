"""Exact-rational evaluation of f4's three per-site terms of every quartet i < j < k < l of ALL populations, each quartet in its
three pairings (ij;kl), (ik;jl), (il;jk), with the -minind predicate over the quartet's four populations: the definition of
pgt_f4_pops_reduce_dev (include/pgtwin.h), written out in `fractions` (no rounding anywhere; the inputs are the float64 values
the kernels read).  Writes tests/golden/f4_exact.json:

    python tests/golden/make_f4_exact.py

Two input sets, K = 4 (1 quartet) and K = 5 (5 quartets), 64 sites each: 6-decimal frequencies uniform in [0, 1] with about one
site in eight set to exactly 0 or 1, a run of sites where two populations carry the SAME frequency (every pair), nInd uniform
in 0 .. 20 (so sites below either minind occur), raised to 5 where a tie, a 0 or a 1 is planted so that every quartet counts
one.  Explicit windows (the whole range, every site alone, ragged ones), minind 1 and 5.  Every sum is stored as the float64
nearest to the exact rational (Python's int / int is correctly rounded)."""
import json
import os
import random
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES = 64
TIE_RUN = 4  # sites per tied pair: sites 10 + 4 m .. 10 + 4 m + 3 carry f[b] = f[a] for pair m
SETS = ((4, 20261022), (5, 20261023))  # (n_pops, seed)


def quartets_of(n_pops):
    return [(i, j, k, l) for i in range(n_pops) for j in range(i + 1, n_pops) for k in range(j + 1, n_pops) for l in range(k + 1, n_pops)]


def f4_site(p):
    """p: the quartet's four frequencies (Fractions) -> (f4(i,j; k,l), f4(i,k; j,l), f4(i,l; j,k))"""
    (pi, pj, pk, pl) = p
    return ((pi - pj) * (pk - pl), (pi - pk) * (pj - pl), (pi - pl) * (pj - pk))


def exact_sites(freqs, ninds, quartet, minind):
    """per site: None where the quartet does not count the site, else the three exact terms"""
    out = []
    for s in range(N_SITES):
        if all(ninds[x][s] >= minind for x in quartet):
            out.append(f4_site([Fraction(freqs[x][s]) for x in quartet]))
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
    assert 10 + TIE_RUN * len(pairs) <= N_SITES
    for m, (a, b) in enumerate(pairs):
        for s in range(10 + TIE_RUN * m, 10 + TIE_RUN * (m + 1)):
            f[b][s] = f[a][s]
    for x in range(n_pops):  # site 2 + x: population x at exactly 0 (x even) or 1 (x odd)
        f[x][2 + x] = float(x % 2)
    ninds = [[rng.randint(0, 20) for _ in range(N_SITES)] for _ in range(n_pops)]
    # those sites and the first site of every tied run are counted by every quartet under either minind
    for s in [2 + x for x in range(n_pops)] + [10 + TIE_RUN * m for m in range(len(pairs))]:
        for x in ninds:
            x[s] = max(x[s], 5)
    pos, at = [], 0
    for _ in range(N_SITES):
        at += rng.randint(1, 49)
        pos.append(at)
    return pos, f, ninds


def windows():
    w = [[s, s + 1] for s in range(N_SITES)]                                # every site alone
    w += [[lo, min(lo + 7, N_SITES)] for lo in range(0, N_SITES - 3, 3)]     # 7 sites, step 3
    w += [[0, N_SITES], [0, 40], [24, 64], [13, 13], [63, 64], [17, 50]]
    return w


def main():
    win = windows()
    sets = []
    for n_pops, seed in SETS:
        pos, freqs, ninds = inputs(n_pops, seed)
        cases = []
        for minind in (1, 5):
            quartets = []
            for quartet in quartets_of(n_pops):
                sites = exact_sites(freqs, ninds, quartet, minind)
                rows = [exact_window(sites, lo, hi) for lo, hi in win]
                quartets.append({"quartet": list(quartet), "f4_ij_kl": [nearest(r[0]) for r in rows], "f4_ik_jl": [nearest(r[1]) for r in rows],
                                 "f4_il_jk": [nearest(r[2]) for r in rows], "n": [r[3] for r in rows]})
            cases.append({"minind": minind, "quartets": quartets})
        sets.append({"n_pops": n_pops, "pos": pos, "freq": freqs, "nind": ninds, "cases": cases})
    doc = {"source": "tests/golden/make_f4_exact.py", "windows": win, "sets": sets}
    with open(os.path.join(HERE, "f4_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
