"""Two restatements of the block jackknife of a SIGNED RATIO OF TWO BLOCK SUMS of include/pgtwin.h (pgt_f4ratio_jackknife_dev),
for ONE item: the blocks' numerators n_j, denominators d_j and weights m_j (a block with m_j == 0 is not used).  Not a test.

    q(a, b) = b != 0 ? a / b : 0
    theta = q(N, D)           theta_-j = q(N - n_j, D - d_j)           h_j = n / m_j          (N, D, n: sums over the used blocks)
    theta_J = g theta - sum_j (1 - m_j / n) theta_-j
    tau_j   = theta + (h_j - 1) (theta - theta_-j)
    sigma^2 = (1 / g) sum_j (tau_j - theta_J)^2 / (h_j - 1)

jack_float: numpy float64, the formulas as written.  jack_exact: fractions.Fraction on the exact values of the given floats, the
square root taken at the end from the exact variance; its long sums are added pairwise and the variance as
(sum tau^2 / (h - 1) - 2 theta_J sum tau / (h - 1) + theta_J^2 sum 1 / (h - 1)) / g — the same rational, with short operands.
Both return a dict with alpha, alpha_jack, se, z, n_sites, n_blocks.  The six items of a row of three sums S0, S1, S2
(F4RATIO_ROW_DTYPE: g_ij, g_ik, g_jk) take (numerator, denominator) = (S2, S1), (S1, S2), (-S2, S0), (S0, -S2), (S1, S0),
(S0, S1).  The synthetic tables are those of tests/dstat_jack_shapes.py viewed as F4RATIO_ROW_DTYPE (the estimators share the
plan and the row layout): their sums are positive, so no denominator, whole or with a block left out, is near zero."""
import functools
import math
from fractions import Fraction

import numpy as np

import dstat_jack_shapes as shapes
from popgenomicstools_amd._lib import F4RATIO_ROW_DTYPE

NAN = float("nan")
FIELDS = ("g_ij", "g_ik", "g_jk")
ITEMS = 6
MAX_TRIPLES = 10
# (numerator, denominator) of item c as (sign, index into FIELDS)
RATIOS = (((+1, 2), (+1, 1)), ((+1, 1), (+1, 2)), ((-1, 2), (+1, 0)), ((+1, 0), (-1, 2)), ((+1, 1), (+1, 0)), ((+1, 0), (+1, 1)))
WORDS_PER_PARTIAL = 5 + 6 + 6  # kJackTotalWords + 2 * kJackRatioItems, 8 bytes each


def work_bytes(n_triples, n_win):
    """jack_work(n_triples, n_win, kJackRatioItems).bytes of csrc/pgt_internal.h, restated: 0 outside 1 ... 10 triples"""
    if not 1 <= n_triples <= MAX_TRIPLES:
        return 0
    cap = min(shapes.plan(n_win)[0], shapes.MAX_PARTIALS)
    return max(256, -(-(n_triples * cap * 8 * WORDS_PER_PARTIAL) // 256) * 256)


def _q(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def jack_float(num, den, m):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    m = np.asarray(m, dtype=np.uint64)
    used = m > 0
    nu, du, mu = num[used], den[used], m[used].astype(np.float64)
    g, n = int(used.sum()), int(m[used].sum())
    with np.errstate(all="ignore"):
        N, D = float(np.sum(nu)), float(np.sum(du))
        theta = float(_q(N, D))
        if g < 2:
            return {"alpha": theta, "alpha_jack": theta, "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g}
        th = _q(N - nu, D - du)
        theta_j = g * theta - float(np.sum((1.0 - mu / n) * th))
        h1 = n / mu - 1.0
        tau = theta + h1 * (theta - th)
        var = float(np.sum((tau - theta_j) ** 2 / h1)) / g
        se = math.sqrt(var) if var >= 0 else NAN
        z = theta_j / se if se > 0 else NAN
    return {"alpha": theta, "alpha_jack": theta_j, "se": se, "z": z, "n_sites": n, "n_blocks": g}


def fsum(xs):
    """the exact sum of Fractions, added pairwise (the operands of a long sum stay short)"""
    xs = list(xs)
    if not xs:
        return Fraction(0)
    while len(xs) > 1:
        xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
    return xs[0]


def jack_exact(num, den, m):
    """Finite inputs only (it never looks at an unused block).  Everything is a Fraction; the results are rounded once, by
    Python's correctly rounded int / int, the root then within an ulp."""
    used = [j for j in range(len(m)) if int(m[j]) > 0]
    ns, ds, ms = [Fraction(float(num[j])) for j in used], [Fraction(float(den[j])) for j in used], [int(m[j]) for j in used]
    g, n = len(used), sum(ms)
    N, D = fsum(ns), fsum(ds)
    theta = N / D if D != 0 else Fraction(0)
    as_float = lambda x: x.numerator / x.denominator
    if g < 2:
        return {"alpha": as_float(theta), "alpha_jack": as_float(theta), "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g}
    th = [(N - a) / (D - b) if D - b != 0 else Fraction(0) for a, b in zip(ns, ds)]
    theta_j = g * theta - fsum(Fraction(n - mj, n) * t for mj, t in zip(ms, th))
    h1 = [Fraction(n - mj, mj) for mj in ms]  # g >= 2 and every m_j > 0: n - m_j > 0
    tau = [theta + h * (theta - t) for h, t in zip(h1, th)]
    var = (fsum(a * a / h for a, h in zip(tau, h1)) - 2 * theta_j * fsum(a / h for a, h in zip(tau, h1)) + theta_j * theta_j * fsum(1 / h for h in h1)) / g
    assert var >= 0
    se = math.sqrt(as_float(var))
    alpha_jack = as_float(theta_j)
    return {"alpha": as_float(theta), "alpha_jack": alpha_jack, "se": se, "z": alpha_jack / se if se > 0 else NAN, "n_sites": n, "n_blocks": g}


def jack_rows(rows, fn=jack_float):
    """fn applied to the six items of one triple's rows (F4RATIO_ROW_DTYPE, one per block) -> [6 dicts]"""
    s = [np.asarray(rows[f], dtype=np.float64) for f in FIELDS]
    return [fn(sn * s[a], sd * s[b], rows["n"]) for (sn, a), (sd, b) in RATIOS]


def synth_rows(n_win, n_triples=MAX_TRIPLES):
    """tests/dstat_jack_shapes.py's table (positive sums in (0, 50) on the 2^-10 grid, n in 1 ... 512, about one block in seven
    unused with NaN sums) as [n_triples, n_win] F4RATIO_ROW_DTYPE.  Read-only."""
    return np.ascontiguousarray(shapes.synth_rows(n_win, n_triples)).view(F4RATIO_ROW_DTYPE).reshape(n_triples, n_win)


@functools.lru_cache(maxsize=None)
def exact_reference(n_win, n_triples=MAX_TRIPLES):
    rows = synth_rows(n_win, n_triples)
    return [jack_rows(rows[t], jack_exact) for t in range(n_triples)]


@functools.lru_cache(maxsize=None)
def float_reference(n_win, n_triples=MAX_TRIPLES):
    rows = synth_rows(n_win, n_triples)
    return [jack_rows(rows[t], jack_float) for t in range(n_triples)]


# Hand-checkable tables of one item: blocks (num, den, m) and what the definition gives, every value exact in f64 but the last
# case's z, which is the f64 quotient of its alpha_jack and se (the CPU test holds both models to them, the GPU test the kernels,
# bit for bit).
HAND_CASES = [
    # theta = 4 / 4; theta_-j = 3 / 2, 1 / 2; theta_J = 2 - (3 / 2 + 1 / 2) / 2 = 1; tau = 1 / 2, 3 / 2; sigma^2 = (1 / 4 + 1 / 4) / 2
    ("two blocks", [(1, 2, 1), (3, 2, 1)], dict(alpha=1.0, alpha_jack=1.0, se=0.5, z=2.0, n_blocks=2, n_sites=2)),
    # theta = 192 / 256 = theta_-j = 189 / 252; theta_J = 48 - 64 * (63 / 64) * 0.75
    ("64 identical blocks", [(3, 4, 8)] * 64, dict(alpha=0.75, alpha_jack=0.75, se=0.0, z=NAN, n_blocks=64, n_sites=512)),
    ("one block", [(3, 4, 5)], dict(alpha=0.75, alpha_jack=0.75, se=NAN, z=NAN, n_blocks=1, n_sites=5)),
    ("an unused block between two used ones", [(1, 2, 1), (NAN, NAN, 0), (3, 2, 1)],
     dict(alpha=1.0, alpha_jack=1.0, se=0.5, z=2.0, n_blocks=2, n_sites=2)),
    # leaving the second block out leaves a denominator of 0: theta_-2 = 0 by the convention; theta = 4 / 2, theta_-1 = 3 / 2;
    # theta_J = 4 - (3 / 2 + 0) / 2 = 3.25; tau = 2.5, 4; sigma^2 = (0.5625 + 0.5625) / 2 = 0.75^2
    ("a deletion that leaves a zero denominator", [(1, 0, 1), (3, 2, 1)],
     dict(alpha=2.0, alpha_jack=3.25, se=0.75, z=3.25 / 0.75, n_blocks=2, n_sites=2)),
    ("no block", [], dict(alpha=0.0, alpha_jack=0.0, se=NAN, z=NAN, n_blocks=0, n_sites=0)),
]


def hand_rows(blocks):
    """one triple whose items 5 = q(S0, S1) and 3 = q(S0, -S2) both read (num, den) of the case: S0 = num, S1 = den, S2 = -den"""
    rows = np.zeros((1, len(blocks)), dtype=F4RATIO_ROW_DTYPE)
    for j, (a, b, m) in enumerate(blocks):
        rows[0, j] = (100 * j + 1, 100 * j + 100, 100 * j + 50, m, 0.0, a, b, -b)
    return rows


def same_item(got, want):
    """equal value for value (NaN equals NaN, -0.0 equals 0.0); got / want: mappings with the six result fields"""
    for k in ("alpha", "alpha_jack", "se", "z"):
        a, b = float(got[k]), float(want[k])
        if not (a == b or (a != a and b != b)):
            return False
    return int(got["n_blocks"]) == int(want["n_blocks"]) and int(got["n_sites"]) == int(want["n_sites"])
