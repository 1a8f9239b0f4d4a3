"""A float64 NumPy model of pgt_pi_pops_reduce_dev's spec (include/pgtwin.h): per population and site, counted where
nind >= minind,
    dn = float64(nind);  c = (2.0*dn) / (2.0*dn - 1.0);  h = (2.0*p) * (1.0 - p);  pi = h * c
every operation a float64 operation of its own, in this order — the reference the GPU and command-line tests of the pi front
end compare against (one-site windows bit for bit).  Window sums are differences of x87 extended-precision prefix sums
(their error, 1e-19 of the prefix, is far below the tests' bound)."""
import numpy as np

from popgenomicstools_amd._lib import DXY_ROW_DTYPE, DXY_TOTAL_DTYPE


def site_pi(p, nind):
    """-> pi per site, float64, in the literal order of the spec; whatever it is where the site is not counted"""
    dn = np.asarray(nind).astype(np.float64)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        two_n = 2.0 * dn
        c = two_n / (two_n - 1.0)
        h = (2.0 * p) * (1.0 - p)
        return h * c


def model(pos, freqs, ninds, minind, win):
    """-> (rows[n_pops, n_win] of DXY_ROW_DTYPE, totals[n_pops] of DXY_TOTAL_DTYPE)"""
    assert np.finfo(np.longdouble).eps < 2e-19, "the model's prefix sums want the 80-bit long double"
    n = int(pos.size)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    rows = np.zeros((len(freqs), win.size), dtype=DXY_ROW_DTYPE)
    tot = np.zeros(len(freqs), dtype=DXY_TOTAL_DTYPE)
    coords = (win["flags"] & 1) != 0
    some = hi > lo
    start = np.where(coords, win["start"], np.where(some, pos[np.minimum(lo, max(n - 1, 0))] if n else 0, 0)).astype(np.uint32)
    end = np.where(coords, win["end"], np.where(some, pos[np.maximum(hi, 1) - 1] if n else 0, 0)).astype(np.uint32)
    for k in range(len(freqs)):
        ok = np.asarray(ninds[k]).astype(np.int64) >= int(minind)
        v = np.where(ok, site_pi(freqs[k], ninds[k]), 0.0)  # selected, never multiplied
        ps = np.concatenate(([0], np.cumsum(v.astype(np.longdouble))))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        r = rows[k]
        r["start"], r["end"] = start, end
        r["neff"] = pn[hi] - pn[lo]
        r["nskip"] = (hi - lo) - (pn[hi] - pn[lo])
        r["sum"] = (ps[hi] - ps[lo]).astype(np.float64)
        one = hi - lo == 1  # a one-site window is that site's value itself (a prefix difference would round it again)
        r["sum"][one] = v[lo[one]]
        tot[k] = (float(ps[-1]), int(pn[-1]), n - int(pn[-1]))
    return rows, tot
