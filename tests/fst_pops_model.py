"""A float64 NumPy model of pgt_fst_pops_reduce_dev's spec (the lines of WCFst(), betaAFOutlier.R:405-417, with per-site
sample sizes and the -minind predicate of dxyWindow.cpp:381) — the reference the GPU and command-line tests of the all-pairs
FST front end compare against.  Per-site components are float64 in the literal form of the R lines; window sums are
differences of x87 extended-precision prefix sums (their error, 1e-19 of the prefix, is far below the tests' bound)."""
import numpy as np

from popgenomicstools_amd._lib import FST_ROW_DTYPE, FST_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import pair_order


def site_components(f1, f2, n1, n2):
    """-> (a, a + b) per site, float64; NaN / inf where n1 n2 == 0 (such a site is never counted: minind >= 1)"""
    n1, n2 = n1.astype(np.float64), n2.astype(np.float64)
    with np.errstate(all="ignore"):
        npool = n1 + n2
        fpool = n1 / npool * f1 + n2 / npool * f2
        alpha1 = 2 * f1 * (1 - f1)
        alpha2 = 2 * f2 * (1 - f2)
        b = (n1 * alpha1 + n2 * alpha2) / (npool - 1)
        a = (4 * n1 * (f1 - fpool) ** 2 + 4 * n2 * (f2 - fpool) ** 2 - b) / (4 * n1 * n2 / npool)
        ab = a + b
    return a, ab


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
    for p, (i, j) in enumerate(pairs):
        ok = (ninds[i] >= minind) & (ninds[j] >= minind)
        a, ab = site_components(freqs[i], freqs[j], ninds[i], ninds[j])
        pa = np.concatenate(([0], np.cumsum(np.where(ok, a, 0.0).astype(np.longdouble))))
        pb = np.concatenate(([0], np.cumsum(np.where(ok, ab, 0.0).astype(np.longdouble))))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        r = rows[p]
        r["start"], r["end"] = start, end
        r["mid"] = ((start.astype(np.uint64) + end.astype(np.uint64)) & 0xFFFFFFFF) // 2  # u32 arithmetic, fstWindow.cpp:73
        r["n"] = pn[hi] - pn[lo]
        r["asum"] = (pa[hi] - pa[lo]).astype(np.float64)
        r["bsum"] = (pb[hi] - pb[lo]).astype(np.float64)
        with np.errstate(all="ignore"):
            r["fst"] = np.where(r["bsum"] != 0, r["asum"] / r["bsum"], 0.0)
        tot[p] = (float(pa[-1]), float(pb[-1]), int(pn[-1]), n - int(pn[-1]))
    return rows, tot


def fst_of(asum, bsum):
    return asum / bsum if bsum != 0 else 0.0
