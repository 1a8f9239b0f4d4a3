"""A float64 NumPy model of pgt_fst_hudson_pops_reduce_dev's definition (include/pgtwin.h): Hudson's FST as a ratio of
averages (Hudson, Slatkin & Maddison 1992; Bhatia et al. 2013, eq. 10) with per-site sample sizes and the -minind predicate —
the reference the GPU and command-line tests of the estimator compare against.  Per-site lines are literally those of the
definition, every operation a float64 operation of its own (one-site windows bit for bit); window sums are differences of x87
extended-precision prefix sums (their error, 1e-19 of the prefix, is far below the tests' bound)."""
import numpy as np

from popgenomicstools_amd._lib import FST_ROW_DTYPE, FST_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import pair_order


def site_components(f1, f2, n1, n2):
    """-> (num, den) per site, float64, in the literal order of the definition; whatever they are where the site is not
    counted (nind <= 0 gives a negative divisor, never 0: 2 nind - 1 is odd)"""
    p1, p2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    with np.errstate(all="ignore"):
        m1 = 2.0 * np.asarray(n1).astype(np.float64) - 1.0
        m2 = 2.0 * np.asarray(n2).astype(np.float64) - 1.0
        h1 = (p1 * (1.0 - p1)) / m1
        h2 = (p2 * (1.0 - p2)) / m2
        d = p1 - p2
        num = (d * d - h1) - h2
        den = p1 * (1.0 - p2) + p2 * (1.0 - p1)
    return num, den


def model(pos, freqs, ninds, minind, win):
    """-> (rows[n_pairs, n_win] of FST_ROW_DTYPE, totals[n_pairs] of FST_TOTAL_DTYPE)"""
    assert np.finfo(np.longdouble).eps < 2e-19, "the model's prefix sums want the 80-bit long double"
    n = int(pos.size)
    pairs = pair_order(len(freqs))
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    rows = np.zeros((len(pairs), win.size), dtype=FST_ROW_DTYPE)
    tot = np.zeros(len(pairs), dtype=FST_TOTAL_DTYPE)
    coords = (win["flags"] & 1) != 0
    some = hi > lo
    start = np.where(coords, win["start"], np.where(some, pos[np.minimum(lo, max(n - 1, 0))] if n else 0, 0)).astype(np.uint32)
    end = np.where(coords, win["end"], np.where(some, pos[np.maximum(hi, 1) - 1] if n else 0, 0)).astype(np.uint32)
    one = hi - lo == 1  # a one-site window is that site's values themselves (a prefix difference would round them again)
    for p, (i, j) in enumerate(pairs):
        ok = (np.asarray(ninds[i]).astype(np.int64) >= int(minind)) & (np.asarray(ninds[j]).astype(np.int64) >= int(minind))
        num, den = site_components(freqs[i], freqs[j], ninds[i], ninds[j])
        num, den = np.where(ok, num, 0.0) + 0.0, np.where(ok, den, 0.0) + 0.0  # selected, never multiplied; -0.0 -> +0.0 as the row epilogue
        pa = np.concatenate(([0], np.cumsum(num.astype(np.longdouble))))
        pb = np.concatenate(([0], np.cumsum(den.astype(np.longdouble))))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        r = rows[p]
        r["start"], r["end"] = start, end
        r["mid"] = ((start.astype(np.uint64) + end.astype(np.uint64)) & 0xFFFFFFFF) // 2  # u32 arithmetic, as the WC rows
        r["n"] = pn[hi] - pn[lo]
        r["asum"] = (pa[hi] - pa[lo]).astype(np.float64)
        r["bsum"] = (pb[hi] - pb[lo]).astype(np.float64)
        r["asum"][one] = num[lo[one]]
        r["bsum"][one] = den[lo[one]]
        with np.errstate(all="ignore"):
            r["fst"] = np.where(r["bsum"] != 0, r["asum"] / r["bsum"], 0.0)
        tot[p] = (float(pa[-1]), float(pb[-1]), int(pn[-1]), n - int(pn[-1]))
    return rows, tot


def fst_of(asum, bsum):
    return asum / bsum if bsum != 0 else 0.0
