"""Exact-rational evaluation of the six sums pgt_pbs_pops_reduce_dev keeps per trio i < j < k of ALL populations — the FST
numerator and denominator of the trio's pairs (i,j), (i,k), (j,k) over the sites where all THREE populations have minind
individuals — for both estimators (include/pgtwin.h), written out in `fractions` (no rounding anywhere; the inputs are the
float64 values the kernels read).  Writes tests/golden/pbs_exact.json:

    python tests/golden/make_pbs_exact.py

Two input sets, K = 3 (1 trio) and K = 4 (4 trios), 96 sites each: 6-decimal frequencies uniform in [0, 1] with about one site
in eight set to exactly 0 or 1, a run of sites where two populations carry the SAME frequency (every pair), nInd uniform in
0 .. 20 (so that every trio has sites one of its pairs counts and the trio does not).  Explicit windows (the whole range,
every eighth site alone, ragged ones), minind 1 and 5.  Every sum is stored as the float64 nearest to the exact rational (Python's
int / int is correctly rounded).  The branch statistics are not stored: they hold a logarithm."""
import json
import os
import random
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES = 96
TIE_RUN = 4  # sites per tied pair: sites 10 + 4 m .. 10 + 4 m + 3 carry f[b] = f[a] for pair m
SEEDS = ((3, 20261023), (4, 20261033))  # the first seeds whose inputs have every property tests/test_pbs_pops_cpu.py asserts
ESTIMATORS = ("wc", "hudson")
FIELDS = ("num_ij", "num_ik", "num_jk", "den_ij", "den_ik", "den_jk")


def trios_of(n_pops):
    return [(i, j, k) for i in range(n_pops) for j in range(i + 1, n_pops) for k in range(j + 1, n_pops)]


def wc_site(f1, f2, n1, n2):
    """the lines of WCFst() (betaAFOutlier.R:405-417) with the site's sample sizes -> (a, a + b)"""
    npool = n1 + n2
    fpool = Fraction(n1, npool) * f1 + Fraction(n2, npool) * f2
    alpha1, alpha2 = 2 * f1 * (1 - f1), 2 * f2 * (1 - f2)
    b = (n1 * alpha1 + n2 * alpha2) / (npool - 1)
    a = (4 * n1 * (f1 - fpool) ** 2 + 4 * n2 * (f2 - fpool) ** 2 - b) / Fraction(4 * n1 * n2, npool)
    return a, a + b


def hudson_site(f1, f2, n1, n2):
    """Hudson's ratio of averages -> (num, den)"""
    h1, h2 = f1 * (1 - f1) / (2 * n1 - 1), f2 * (1 - f2) / (2 * n2 - 1)
    return (f1 - f2) ** 2 - h1 - h2, f1 * (1 - f2) + f2 * (1 - f1)


SITE = {"wc": wc_site, "hudson": hudson_site}


def exact_sites(freqs, ninds, trio, minind, estimator):
    """per site: None where the trio does not count the site, else the six exact values in the order of FIELDS"""
    i, j, k = trio
    out = []
    for s in range(N_SITES):
        if all(ninds[x][s] >= minind for x in trio):
            v = [SITE[estimator](Fraction(freqs[a][s]), Fraction(freqs[b][s]), ninds[a][s], ninds[b][s]) for a, b in ((i, j), (i, k), (j, k))]
            out.append(tuple(x[0] for x in v) + tuple(x[1] for x in v))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    took = [x for x in sites[lo:hi] if x is not None]
    return tuple(sum((x[c] for x in took), Fraction(0)) for c in range(6)) + (len(took),)


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
    w = [[s, s + 1] for s in range(2, N_SITES, 8)]                          # every eighth site alone: the first of every other tie run
    w += [[lo, min(lo + 7, N_SITES)] for lo in range(0, N_SITES - 3, 18)]    # 7 sites, step 18
    w += [[0, N_SITES], [0, 64], [32, 96], [13, 13], [95, 96], [37, 80]]
    return w


def main():
    win = windows()
    sets = []
    for n_pops, seed in SEEDS:
        pos, freqs, ninds = inputs(n_pops, seed)
        cases = []
        for estimator in ESTIMATORS:
            for minind in (1, 5):
                trios = []
                for trio in trios_of(n_pops):
                    sites = exact_sites(freqs, ninds, trio, minind, estimator)
                    rows = [exact_window(sites, lo, hi) for lo, hi in win]
                    entry = {"trio": list(trio), "n": [r[6] for r in rows]}
                    for c, fld in enumerate(FIELDS):
                        entry[fld] = [nearest(r[c]) for r in rows]
                    trios.append(entry)
                cases.append({"estimator": estimator, "minind": minind, "trios": trios})
        sets.append({"n_pops": n_pops, "pos": pos, "freq": freqs, "nind": ninds, "cases": cases})
    doc = {"source": "tests/golden/make_pbs_exact.py", "windows": win, "sets": sets}
    with open(os.path.join(HERE, "pbs_exact.json"), "w") as fh:
        json.dump(doc, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
