"""Exact-rational evaluation of the f4-ratio's three per-site terms e d_ij, e d_ik, e d_jk (e = p_A - p_O, A the first and O the
last population) of every triple i < j < k of the middle populations, with the -minind predicate over FIVE populations, and of
the six admixture proportions a window's three sums give: the definition of pgt_f4ratio_pops_reduce_dev (include/pgtwin.h),
written out in `fractions` (no rounding anywhere; the inputs are the float64 values the kernels read).  Writes
tests/golden/f4ratio_exact.json:

    python tests/golden/make_f4ratio_exact.py

One input set, K = 6 (4 triples, every middle pair in two of them), 320 sites.  Frequencies are multiples of 2^-10 drawn from an
admixture tree, so that no denominator is near zero: ancestral a ~ U(.1, .9); O = a + N(.10); root = a + N(.05);
c = root + N(.05); ab = root + N(.15); A = ab + N(.05); b = ab + N(.05); middle k = alpha_k b + (1 - alpha_k) c + N(.03) with
alpha_k = linspace(.9, .1, m); all clipped to [0, 1] and rounded to the grid.  nInd uniform in 2 .. 20 (so sites below minind 5
occur).  Explicit windows (the whole range, two overlapping two-thirds, a ragged long one, single sites, short ragged ones, an
empty one), minind 1 and 5.  Ratios are recorded for the windows of 256 sites or more; the generator ASSERTS that each of their three sums — every
one is the denominator of two ratios — has kappa = Σ|term| / |Σ term| <= 8.  Floats are stored as hex strings (trailing zeros dropped); every sum and
ratio is the float64 nearest to the exact rational (Python's int / int is correctly rounded)."""
import json
import os
import random
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
N_SITES = 320
GRID = 1024
KAPPA_CAP = 8
RATIO_MIN_SITES = 256
SETS = ((6, 20261102),)  # (n_pops, seed)
# (numerator, denominator) of item c as (sign, index of the sum): c = 0 .. 5 is (B, X, C) = (i,j,k), (j,i,k), (i,k,j), (k,i,j), (j,k,i), (k,j,i)
RATIOS = (((+1, 2), (+1, 1)), ((+1, 1), (+1, 2)), ((-1, 2), (+1, 0)), ((+1, 0), (-1, 2)), ((+1, 1), (+1, 0)), ((+1, 0), (+1, 1)))


def triples_of(n_pops):
    g = n_pops - 1
    return [(i, j, k) for i in range(1, g) for j in range(i + 1, g) for k in range(j + 1, g)]


def site_terms(pa, po, pi, pj, pk):
    """exact: (f4(A,O; i,j), f4(A,O; i,k), f4(A,O; j,k)) of one site"""
    e = pa - po
    return (e * (pi - pj), e * (pi - pk), e * (pj - pk))


def exact_sites(freqs, ninds, triple, minind):
    """per site: None where the triple does not count the site (A, O or one of its three below minind), else the exact terms"""
    five = (0, len(freqs) - 1) + tuple(triple)
    out = []
    for s in range(N_SITES):
        if all(ninds[x][s] >= minind for x in five):
            out.append(site_terms(*[Fraction(freqs[x][s]) for x in five]))
        else:
            out.append(None)
    return out


def exact_window(sites, lo, hi):
    """-> (S0, S1, S2, n, A0, A1, A2): the sums, the counted sites, the sums of |term|"""
    took = [x for x in sites[lo:hi] if x is not None]
    sums = tuple(sum((x[c] for x in took), Fraction(0)) for c in range(3))
    mags = tuple(sum((abs(x[c]) for x in took), Fraction(0)) for c in range(3))
    return sums + (len(took),) + mags


def exact_ratios(sums):
    """the six q(N_c, D_c), q(a, b) = b != 0 ? a / b : 0"""
    out = []
    for (sn, n), (sd, d) in RATIOS:
        num, den = sn * sums[n], sd * sums[d]
        out.append(num / den if den != 0 else Fraction(0))
    return out


def nearest(x):
    return x.numerator / x.denominator


def inputs(n_pops, seed):
    rng = random.Random(seed)
    m = n_pops - 2
    alpha = [0.9 - 0.8 * t / (m - 1) for t in range(m)]
    cols = [[] for _ in range(n_pops)]
    for _ in range(N_SITES):
        a = rng.uniform(0.1, 0.9)
        O = a + rng.gauss(0, 0.10)
        root = a + rng.gauss(0, 0.05)
        c = root + rng.gauss(0, 0.05)
        ab = root + rng.gauss(0, 0.15)
        A = ab + rng.gauss(0, 0.05)
        b = ab + rng.gauss(0, 0.05)
        mid = [al * b + (1 - al) * c + rng.gauss(0, 0.03) for al in alpha]
        for x, v in zip(cols, [A] + mid + [O]):
            x.append(round(min(max(v, 0.0), 1.0) * GRID) / GRID)
    ninds = [[rng.randint(2, 20) for _ in range(N_SITES)] for _ in range(n_pops)]
    pos, at = [], 0
    for _ in range(N_SITES):
        at += rng.randint(1, 49)
        pos.append(at)
    return pos, cols, ninds


def windows():
    w = [[s, s + 1] for s in range(24)]                          # single sites
    w += [[lo, lo + 7] for lo in range(0, 30, 3)]                 # 7 sites, step 3
    w += [[0, N_SITES], [0, 256], [64, 320], [32, 300], [100, 300], [13, 13], [319, 320]]
    return w


def ratio_windows():
    return [n for n, (lo, hi) in enumerate(windows()) if hi - lo >= RATIO_MIN_SITES]


def hexes(xs):
    """float.hex() without the trailing zeros of the mantissa (float.fromhex reads either form)"""
    out = []
    for x in xs:
        m, _, e = float(x).hex().partition("p")
        out.append((m.rstrip("0").rstrip(".") + "p" + e) if e else m)
    return out


def main():
    win = windows()
    rw = ratio_windows()
    sets = []
    for n_pops, seed in SETS:
        pos, freqs, ninds = inputs(n_pops, seed)
        cases = []
        for minind in (1, 5):
            triples = []
            for triple in triples_of(n_pops):
                sites = exact_sites(freqs, ninds, triple, minind)
                rows = [exact_window(sites, lo, hi) for lo, hi in win]
                for n in rw:  # the condition cap of every denominator a test compares
                    for c in range(3):
                        assert rows[n][c] != 0 and rows[n][4 + c] <= KAPPA_CAP * abs(rows[n][c]), (n_pops, minind, triple, win[n], c)
                triples.append({"triple": list(triple), "g_ij": hexes(nearest(r[0]) for r in rows), "g_ik": hexes(nearest(r[1]) for r in rows),
                                "g_jk": hexes(nearest(r[2]) for r in rows), "n": [r[3] for r in rows],
                                "alpha": [hexes(nearest(x) for x in exact_ratios(rows[n][:3])) for n in rw]})
            cases.append({"minind": minind, "triples": triples})
        sets.append({"n_pops": n_pops, "pos": pos, "freq": [hexes(x) for x in freqs], "nind": ninds, "cases": cases})
    doc = {"source": "tests/golden/make_f4ratio_exact.py", "windows": win, "ratio_windows": rw, "sets": sets}
    with open(os.path.join(HERE, "f4ratio_exact.json"), "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
