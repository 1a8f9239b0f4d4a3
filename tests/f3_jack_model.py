"""Two restatements of the block jackknife of a MEAN of include/pgtwin.h (pgt_f3_jackknife_dev), for ONE item: the blocks' sums
x_j and weights m_j (a block with m_j == 0 is not used).  Not a test.

    mean(a, b) = b != 0 ? a / b : 0
    theta = mean(X, n)        theta_-j = mean(X - x_j, n - m_j)        h_j = n / m_j
    theta_J = g theta - sum_j (1 - m_j / n) theta_-j
    tau_j   = theta + (h_j - 1) (theta - theta_-j)
    sigma^2 = (1 / g) sum_j (tau_j - theta_J)^2 / (h_j - 1)

jack_float: numpy float64, the formulas as written.  jack_exact: fractions.Fraction on the exact values of the given floats, the
square root taken at the end from the exact variance.  Both return a dict with f3, f3_jack, se, z, n_sites, n_blocks.  The
synthetic tables, the hand cases and the shared references of the f3 jackknife tests are here too (the launch arithmetic and
the table sizes are those of tests/dstat_jack_shapes.py: the two estimators share the plan)."""
import functools
import math
from fractions import Fraction

import numpy as np

from popgenomicstools_amd._lib import F3_ROW_DTYPE

NAN = float("nan")
FIELDS = ("f3_i", "f3_j", "f3_k")  # x of item c = 0, 1, 2 among a row's sums: the target i, j, k
MAX_TRIOS = 20


def _mean(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def jack_float(x, m):
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(m, dtype=np.uint64)
    used = m > 0
    xu, mu = x[used], m[used].astype(np.float64)
    g, n = int(used.sum()), int(m[used].sum())
    with np.errstate(all="ignore"):
        X = float(np.sum(xu))
        theta = float(_mean(X, float(n)))
        if g < 2:
            return {"f3": theta, "f3_jack": theta, "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g}
        th = _mean(X - xu, float(n) - mu)
        theta_j = g * theta - float(np.sum((1.0 - mu / n) * th))
        h1 = n / mu - 1.0
        tau = theta + h1 * (theta - th)
        var = float(np.sum((tau - theta_j) ** 2 / h1)) / g
        se = math.sqrt(var) if var >= 0 else NAN
        z = theta_j / se if se > 0 else NAN
    return {"f3": theta, "f3_jack": theta_j, "se": se, "z": z, "n_sites": n, "n_blocks": g}


def jack_exact(x, m):
    """Finite inputs only (it never looks at an unused block).  Everything is a Fraction; the results are rounded once, by
    Python's correctly rounded int / int, the root then within an ulp."""
    used = [j for j in range(len(m)) if int(m[j]) > 0]
    xs, ms = [Fraction(float(x[j])) for j in used], [int(m[j]) for j in used]
    g, n = len(used), sum(ms)
    X = sum(xs, Fraction(0))
    theta = X / n if n else Fraction(0)
    as_float = lambda q: q.numerator / q.denominator
    if g < 2:
        return {"f3": as_float(theta), "f3_jack": as_float(theta), "se": NAN, "z": NAN, "n_sites": n, "n_blocks": g}
    th = [(X - a) / (n - mj) for a, mj in zip(xs, ms)]  # g >= 2 and every m_j > 0: n - m_j > 0
    theta_j = g * theta - sum((Fraction(n - mj, n) * t for mj, t in zip(ms, th)), Fraction(0))
    h1 = [Fraction(n - mj, mj) for mj in ms]
    var = sum(((theta + h * (theta - t) - theta_j) ** 2 / h for h, t in zip(h1, th)), Fraction(0)) / g
    assert var >= 0
    se = math.sqrt(as_float(var))
    f3_jack = as_float(theta_j)
    return {"f3": as_float(theta), "f3_jack": f3_jack, "se": se, "z": f3_jack / se if se > 0 else NAN, "n_sites": n, "n_blocks": g}


def jack_rows(rows, fn=jack_float):
    """fn applied to the three targets of one trio's rows (F3_ROW_DTYPE, one per block) -> [3 dicts]"""
    return [fn(rows[f], rows["n"]) for f in FIELDS]


@functools.lru_cache(maxsize=None)
def synth_rows(n_win, n_trios=MAX_TRIOS, seed=0):
    """[n_trios, n_win] F3_ROW_DTYPE: per trio and target independent SIGNED block sums — n times a per-site mean drawn around
    -0.004 with standard deviation 0.02, rounded to a multiple of 2^-20 — and n in 1 ... 512; one block in seven has n = 0 and
    NaN sums (a block that is not used must never reach a sum).  The coordinates are filled but mean nothing to the
    jackknife.  A table of fewer trios of the same n_win and seed is a prefix of this one.  Read-only."""
    rows = np.zeros((n_trios, n_win), dtype=F3_ROW_DTYPE)
    for t in range(n_trios):
        rng = np.random.default_rng([seed, n_win, t, 3])
        rows["n"][t] = rng.integers(1, 513, n_win)
        for f in FIELDS:
            rows[f][t] = np.round(rng.normal(-0.004, 0.02, n_win) * rows["n"][t] * 2.0 ** 20) / 2.0 ** 20
        empty = np.arange(n_win) % 7 == (3 + t) % 7
        rows["n"][t][empty] = 0
        for f in FIELDS:
            rows[f][t][empty] = np.nan
        rows["start"][t] = np.arange(n_win) * 100 + 1
        rows["end"][t] = rows["start"][t] + 99
        rows["mid"][t] = rows["start"][t] + 49
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def exact_reference(n_win, n_trios=MAX_TRIOS):
    rows = synth_rows(n_win, n_trios)
    return [jack_rows(rows[t], jack_exact) for t in range(n_trios)]


@functools.lru_cache(maxsize=None)
def float_reference(n_win, n_trios=MAX_TRIOS):
    rows = synth_rows(n_win, n_trios)
    return [jack_rows(rows[t], jack_float) for t in range(n_trios)]


# Hand-checkable tables of one item: blocks (x, m) and what the definition gives, every value exact in f64 (the CPU test holds
# both models to them, the GPU test the kernels, bit for bit).
HAND_CASES = [
    # theta = 4 / 2; theta_-j = 1, 3; theta_J = 2 * 2 - (1 + 3) / 2 = 2; tau = 3, 1; sigma^2 = (1 + 1) / 2
    ("two blocks", [(3, 1), (1, 1)], dict(f3=2.0, f3_jack=2.0, se=1.0, z=2.0, n_blocks=2, n_sites=2)),
    # theta = 192 / 512 = theta_-j = 189 / 504; theta_J = 24 - 64 * (63 / 64) * 0.375
    ("64 identical blocks", [(3, 8)] * 64, dict(f3=0.375, f3_jack=0.375, se=0.0, z=NAN, n_blocks=64, n_sites=512)),
    ("one block", [(3, 4)], dict(f3=0.75, f3_jack=0.75, se=NAN, z=NAN, n_blocks=1, n_sites=4)),
    ("an unused block between two used ones", [(3, 1), (NAN, 0), (1, 1)], dict(f3=2.0, f3_jack=2.0, se=1.0, z=2.0, n_blocks=2, n_sites=2)),
    ("no block", [], dict(f3=0.0, f3_jack=0.0, se=NAN, z=NAN, n_blocks=0, n_sites=0)),
]


def same_item(got, want):
    """equal value for value (NaN equals NaN, -0.0 equals 0.0); got / want: mappings with the six result fields"""
    for k in ("f3", "f3_jack", "se", "z"):
        a, b = float(got[k]), float(want[k])
        if not (a == b or (a != a and b != b)):
            return False
    return int(got["n_blocks"]) == int(want["n_blocks"]) and int(got["n_sites"]) == int(want["n_sites"])
