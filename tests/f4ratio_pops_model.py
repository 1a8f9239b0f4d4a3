"""A float64 NumPy model of pgt_f4ratio_pops_reduce_dev's definition (include/pgtwin.h): the three sums of (p_A - p_O)(p_x - p_y)
of every triple i < j < k of the MIDDLE populations 1 .. K-2, population 0 being A and population K-1 the outgroup O, with the
-minind predicate over FIVE populations (A, O and the triple's three), and the six admixture proportions a row's sums give —
the reference the GPU and command-line tests of f4ratioWindowPops compare against.  Per-site terms are float64 in the literal
grouping of the definition (elementwise NumPy rounds every operation on its own: no contraction); window sums are differences
of x87 extended-precision prefix sums (their error, 1e-19 of the prefix of |term|, is far below the tests' bound).  Beside each
sum the model returns A, the window's Σ|product| of the same sum: the site terms have both signs, so a bound on a sum's error
is relative to A, not to the sum, and kappa = A / |sum| is the condition of a ratio that has the sum as its denominator."""
import numpy as np

from f4_pops_model import coordinates  # start / end / mid of a window: the K-population rows fill them alike
from popgenomicstools_amd._lib import F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE

SUMS = ("g_ij", "g_ik", "g_jk")
GRID = 1024.0   # frequencies that are multiples of 2^-10: differences, products and short sums of them are exact in float64
KAPPA_CAP = 8.0  # the tests compare a ratio only where its denominator has kappa <= 8
# (numerator, denominator) of item c as (sign, index into SUMS): alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C)
RATIOS = (((+1, 2), (+1, 1)), ((+1, 1), (+1, 2)), ((-1, 2), (+1, 0)), ((+1, 0), (-1, 2)), ((+1, 1), (+1, 0)), ((+1, 0), (+1, 1)))


def middle_triple_order(n_pops):
    """the model's own triple order (the package's middle_triple_order is held to it by tests/test_f4ratio_pops_cpu.py)"""
    g = n_pops - 1
    return [(i, j, k) for i in range(1, g) for j in range(i + 1, g) for k in range(j + 1, g)]


def ratio_order(i, j, k):
    """(B, X, C) of item c = 0 .. 5"""
    return [(i, j, k), (j, i, k), (i, k, j), (k, i, j), (j, k, i), (k, j, i)]


def site_terms(p_a, p_o, p_i, p_j, p_k, shared=None):
    """-> ((s0, s1, s2), (a0, a1, a2)) per site, float64, in the definition's grouping; a_c = |product| of term c.
    shared: None, or (e, d_ij, d_ik, d_jk) already evaluated by these same lines"""
    p_a, p_o, p_i, p_j, p_k = (np.asarray(x, dtype=np.float64) for x in (p_a, p_o, p_i, p_j, p_k))
    with np.errstate(all="ignore"):
        e, d_ij, d_ik, d_jk = (p_a - p_o, p_i - p_j, p_i - p_k, p_j - p_k) if shared is None else shared
        s = (e * d_ij, e * d_ik, e * d_jk)
        a = tuple(np.abs(x) for x in s)
    return s, a


def counted(ninds, i, j, k, minind):
    """all FIVE populations: A (the first), O (the last) and the triple's"""
    return (ninds[0] >= minind) & (ninds[-1] >= minind) & (ninds[i] >= minind) & (ninds[j] >= minind) & (ninds[k] >= minind)


def q(num, den):
    """den != 0 ? num / den : 0, one division"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)


def alphas(s0, s1, s2):
    """the six admixture proportions of a row (or a total) from its three sums -> float64 [..., 6]"""
    s = (np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64))
    return np.stack([q(sn * s[n], sd * s[d]) for (sn, n), (sd, d) in RATIOS], axis=-1)


def alphas_of(rows):
    return alphas(rows[SUMS[0]], rows[SUMS[1]], rows[SUMS[2]])


def kappa(total, A):
    """Σ|term| / |Σ term| of a sum (inf where the sum is 0 and the terms are not; 1 for an empty sum)"""
    total, A = np.asarray(total, dtype=np.float64), np.asarray(A, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(A == 0, 1.0, A / np.abs(total))


def admixture_inputs(rng, n, n_pops, lo_count=0):
    """Grid frequencies drawn from an admixture tree, so that no f4(A,O; x,y) of two middle populations is near zero:
    ancestral a ~ U(.1, .9); O = a + N(.10); root = a + N(.05); c = root + N(.05); ab = root + N(.15); A = ab + N(.05);
    b = ab + N(.05); middle k = alpha_k b + (1 - alpha_k) c + N(.03) with alpha_k = linspace(.9, .1, m); all clipped to [0, 1]
    and rounded to multiples of 2^-10.  -> (freqs [A, M1 .. Mm, O], ninds uniform in lo_count .. 20)"""
    m = n_pops - 2

    def N(sd):
        return rng.normal(0.0, sd, n)
    a = rng.uniform(0.1, 0.9, n)
    O = a + N(0.10)
    root = a + N(0.05)
    c = root + N(0.05)
    ab = root + N(0.15)
    A = ab + N(0.05)
    b = ab + N(0.05)
    mid = [al * b + (1.0 - al) * c + N(0.03) for al in np.linspace(0.9, 0.1, m)]
    f = [np.round(np.clip(x, 0.0, 1.0) * GRID) / GRID for x in [A] + mid + [O]]
    return f, [rng.integers(lo_count, 21, n, dtype=np.int32) for _ in range(n_pops)]


def model(pos, freqs, ninds, minind, win, ranges_only=False):
    """-> (rows[n_triples, n_win] of F4RATIO_ROW_DTYPE, totals[n_triples] of F4RATIO_TOTAL_DTYPE, A, A_tot): A[s][n_triples,
    n_win] and A_tot[s][n_triples] are Σ|product| of sum s over the window's (all) counted sites.  A one-site window is that
    site's term itself (a prefix difference would round it again).  ranges_only: for a table of a few windows over a long
    column — every window summed on its own slice by NumPy's pairwise float64 sum (error below log2(n) 2^-53 A), no
    extended-precision prefix sums over the column."""
    assert np.finfo(np.longdouble).eps < 2e-19, "the model's sums want the 80-bit long double"
    n = int(pos.size)
    K = len(freqs)
    triples = middle_triple_order(K)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    rows = np.zeros((len(triples), win.size), dtype=F4RATIO_ROW_DTYPE)
    tot = np.zeros(len(triples), dtype=F4RATIO_TOTAL_DTYPE)
    A = {s: np.zeros((len(triples), win.size)) for s in SUMS}
    A_tot = {s: np.zeros(len(triples)) for s in SUMS}
    start, end, mid = coordinates(pos, win)
    one = hi - lo == 1

    def window_sums(x):
        if ranges_only:
            whole = x.sum()
            return np.array([whole if (a, b) == (0, n) else x[a:b].sum() for a, b in zip(lo, hi)]), float(whole)
        px = np.concatenate(([0], np.cumsum(x.astype(np.longdouble))))
        return (px[hi] - px[lo]).astype(np.float64), float(px[-1])

    with np.errstate(all="ignore"):
        e = np.asarray(freqs[0], dtype=np.float64) - np.asarray(freqs[K - 1], dtype=np.float64)
        d = {(a, b): np.asarray(freqs[a], dtype=np.float64) - np.asarray(freqs[b], dtype=np.float64)
             for a in range(1, K - 1) for b in range(a + 1, K - 1)}
    for t, (i, j, k) in enumerate(triples):
        ok = counted(ninds, i, j, k, minind)
        terms, mags = site_terms(freqs[0], freqs[K - 1], freqs[i], freqs[j], freqs[k], shared=(e, d[i, j], d[i, k], d[j, k]))
        if ranges_only:
            n_ok = int(np.count_nonzero(ok))
            r_n = [n_ok if (a, b) == (0, n) else int(np.count_nonzero(ok[a:b])) for a, b in zip(lo, hi)]
        else:
            pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
            n_ok, r_n = int(pn[-1]), pn[hi] - pn[lo]
        r = rows[t]
        r["start"], r["end"], r["mid"] = start, end, mid
        r["n"] = r_n
        for fld, x, a in zip(SUMS, terms, mags):
            x = np.where(ok, x, 0.0) + 0.0  # selected, never multiplied; -0.0 -> +0.0 as the row epilogue
            a = np.where(ok, a, 0.0)
            r[fld], tot[fld][t] = window_sums(x)
            r[fld][one] = x[lo[one]]
            A[fld][t], A_tot[fld][t] = window_sums(a)
        tot["neff"][t] = n_ok
        tot["nskip"][t] = n - n_ok
    return rows, tot, A, A_tot
