"""Two restatements of the block jackknife of include/pgtwin.h (pgt_dstat_jackknife_dev), for ONE item: the blocks' x_j, y_j
and weights m_j (a block with m_j == 0 is not used).  Not a test.

    ratio(a, b) = (a + b) != 0 ? (a - b) / (a + b) : 0
    theta = ratio(X, Y)        theta_-j = ratio(X - x_j, Y - y_j)        h_j = n / m_j
    theta_J = g theta - sum_j (1 - m_j / n) theta_-j
    tau_j   = theta + (h_j - 1) (theta - theta_-j)
    sigma^2 = (1 / g) sum_j (tau_j - theta_J)^2 / (h_j - 1)

jack_float: numpy float64, the formulas as written.  jack_exact: fractions.Fraction on the exact values of the given floats, the
square root taken at the end from the exact variance.  Both return a dict with d, d_jack, se, z, n_sites, n_blocks (jack_exact
also var, the exact variance as an unreduced (numerator, denominator), or None)."""
import math
from fractions import Fraction

import numpy as np

NAN = float("nan")

# (x, y) of topology c = 0, 1, 2 among a row's sums: ((i,j),k), ((i,k),j), ((j,k),i)
TOPOLOGY_FIELDS = (("abba", "baba"), ("bbaa", "baba"), ("bbaa", "abba"))


def _ratio(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = a + b
    with np.errstate(all="ignore"):
        return np.where(den != 0, (a - b) / np.where(den != 0, den, 1.0), 0.0)


def jack_float(x, y, m):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = np.asarray(m, dtype=np.uint64)
    used = m > 0
    xu, yu, mu = x[used], y[used], m[used].astype(np.float64)
    g, n = int(used.sum()), int(m[used].sum())
    with np.errstate(all="ignore"):
        X, Y = float(np.sum(xu)), float(np.sum(yu))
        theta = float(_ratio(X, Y))
        if g < 2:
            return {"d": theta, "d_jack": theta, "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g}
        th = _ratio(X - xu, Y - yu)
        theta_j = g * theta - float(np.sum((1.0 - mu / n) * th))
        h1 = n / mu - 1.0
        tau = theta + h1 * (theta - th)
        var = float(np.sum((tau - theta_j) ** 2 / h1)) / g
        se = math.sqrt(var) if var >= 0 else NAN
        z = theta_j / se if se > 0 else NAN
    return {"d": theta, "d_jack": theta_j, "se": se, "z": z, "n_sites": n, "n_blocks": g}


def _tree_sum(pairs):
    """The exact sum of the rationals (numerator, denominator), combined pairwise as integers and never reduced: a running
    Fraction sum would take the gcd of numbers of several hundred thousand bits at every one of its additions."""
    pairs = list(pairs)
    while len(pairs) > 1:
        nxt = [(a * d + c * b, b * d) for (a, b), (c, d) in zip(pairs[0::2], pairs[1::2])]
        if len(pairs) % 2:
            nxt.append(pairs[-1])
        pairs = nxt
    return pairs[0] if pairs else (0, 1)


def _ratio_exact(a, b):
    return (a - b) / (a + b) if a + b != 0 else Fraction(0)


def jack_exact(x, y, m):
    """Finite inputs only.  Per block everything is a Fraction; the sums over the blocks, theta_J and the variance are kept
    as unreduced integer pairs (num, den) and rounded once, by Python's correctly rounded int / int.  The variance sum is
    evaluated as sum w tau^2 - 2 theta_J sum w tau + theta_J^2 sum w with w = 1 / (h - 1): in exact arithmetic the same
    number as the definition's sum, without squaring the several hundred thousand bits of theta_J once per block."""
    used = [j for j in range(len(m)) if int(m[j]) > 0]
    xs, ys, ms = [Fraction(float(x[j])) for j in used], [Fraction(float(y[j])) for j in used], [int(m[j]) for j in used]
    g, n = len(used), sum(ms)
    X, Y = sum(xs, Fraction(0)), sum(ys, Fraction(0))
    theta = _ratio_exact(X, Y)
    if g < 2:
        return {"d": float(theta), "d_jack": float(theta), "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g, "var": None}
    th = [_ratio_exact(X - a, Y - b) for a, b in zip(xs, ys)]
    p, q = _tree_sum(((n - mj) * t.numerator, n * t.denominator) for mj, t in zip(ms, th))
    ja, jb = g * theta.numerator * q - p * theta.denominator, theta.denominator * q          # theta_J = ja / jb
    w = [Fraction(mj, n - mj) for mj in ms]                                                   # 1 / (h_j - 1)
    tau = [theta + (theta - t) / wj for t, wj in zip(th, w)]                                  # theta + (h_j - 1) (theta - theta_-j)
    a2, b2 = _tree_sum(((wj * t * t).numerator, (wj * t * t).denominator) for wj, t in zip(w, tau))
    a1, b1 = _tree_sum(((wj * t).numerator, (wj * t).denominator) for wj, t in zip(w, tau))
    sw = sum(w, Fraction(0))
    a0, b0 = sw.numerator, sw.denominator
    # g var = a2/b2 - 2 (ja/jb) (a1/b1) + (ja/jb)^2 (a0/b0), over the common denominator b2 b1 b0 jb^2
    num = a2 * b1 * b0 * jb * jb - 2 * ja * jb * a1 * b2 * b0 + ja * ja * a0 * b2 * b1
    den = b2 * b1 * b0 * jb * jb * g
    if den < 0:
        num, den = -num, -den
    assert num >= 0
    se = math.sqrt(num / den)  # int / int is correctly rounded, the root then within an ulp
    d_jack = ja / jb
    z = d_jack / se if se > 0 else NAN
    return {"d": float(theta), "d_jack": d_jack, "se": se, "z": z, "n_sites": n, "n_blocks": g, "var": (num, den)}


def jack_rows(rows, fn=jack_float):
    """fn applied to the three topologies of one trio's rows (DSTAT_ROW_DTYPE, one per block) -> [3 dicts]"""
    return [fn(rows[fx], rows[fy], rows["n"]) for fx, fy in TOPOLOGY_FIELDS]
