"""A float64 NumPy model of pgt_fd_pops_reduce_dev's definition (include/pgtwin.h): f_d (Martin et al. 2015) and f_dM (Malinsky
et al. 2015) of every ingroup trio ((P1 = i, P2 = j), P3 = k) against the last population, with the -minind predicate over the
four populations — the reference the GPU and command-line tests of `dstatWindowPops -fd 1` compare against.  Per-site terms
are float64 in the literal grouping of the definition (elementwise NumPy rounds every operation on its own: no contraction;
the selects pick OPERANDS by comparing the input frequencies, as the definition is written); window sums are differences of
x87 extended-precision prefix sums (their error, 1e-19 of the prefix of |term|, is far below the tests' bound).  Beside each
sum the model returns A, the window's Σ|site term|: the site terms have both signs, so a bound on a sum's error is relative to
A, not to the sum."""
import numpy as np

from popgenomicstools_amd._lib import FD_ROW_DTYPE, FD_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import trio_order

SUMS = ("num", "fd_den", "fdm_den")


def site_terms(p_i, p_j, p_k, p_o, choose=None):
    """-> (num, fd_den, fdm_den) per site, float64, in the definition's grouping.  choose: None, or a dict of boolean arrays
    that replace the definition's comparisons 'H_is_j', 'L_is_j', 'G_is_i', 'S_is_i' (the tests of tie indifference pass the
    other choice at ties)."""
    p_i, p_j, p_k, p_o = (np.asarray(x, dtype=np.float64) for x in (p_i, p_j, p_k, p_o))
    choose = choose or {}
    with np.errstate(all="ignore"):
        q_i, q_j, q_k, q_o = 1.0 - p_i, 1.0 - p_j, 1.0 - p_k, 1.0 - p_o
        abba = (q_i * p_j) * (p_k * q_o) + (p_i * q_j) * (q_k * p_o)
        baba = (p_i * q_j) * (p_k * q_o) + (q_i * p_j) * (q_k * p_o)
        num = abba - baba
        h = choose.get("H_is_j", p_j >= p_k)
        l = choose.get("L_is_j", p_j <= p_k)
        g = choose.get("G_is_i", p_i >= p_k)
        s = choose.get("S_is_i", p_i <= p_k)
        p_H, q_H = np.where(h, p_j, p_k), np.where(h, q_j, q_k)
        p_L, q_L = np.where(l, p_j, p_k), np.where(l, q_j, q_k)
        p_G, q_G = np.where(g, p_i, p_k), np.where(g, q_i, q_k)
        p_S, q_S = np.where(s, p_i, p_k), np.where(s, q_i, q_k)
        B1 = (q_i * p_H) * (p_H * q_o) - (p_i * q_H) * (p_H * q_o)
        A1 = (p_i * q_L) * (q_L * p_o) - (q_i * p_L) * (q_L * p_o)
        B2 = (p_G * q_j) * (p_G * q_o) - (q_G * p_j) * (p_G * q_o)
        A2 = (q_S * p_j) * (q_S * p_o) - (p_S * q_j) * (q_S * p_o)
        fd_den = B1 + A1
        fdm_den = np.where(p_j >= p_i, B1, B2) + np.where(p_j <= p_i, A1, A2)
    return num, fd_den, fdm_den


def ratio(num, den):
    """a row's fd / fdm from its own sums: den != 0 ? num / den : 0, one division rounded once"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)


def counted(ninds, i, j, k, minind):
    o = len(ninds) - 1
    return (ninds[i] >= minind) & (ninds[j] >= minind) & (ninds[k] >= minind) & (ninds[o] >= minind)


def coordinates(pos, win):
    """-> (start, end, mid) of every window, as pgt_dstat_row's are filled"""
    n = int(pos.size)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    coords = (win["flags"] & 1) != 0
    some = hi > lo
    start = np.where(coords, win["start"], np.where(some, pos[np.minimum(lo, max(n - 1, 0))] if n else 0, 0)).astype(np.uint32)
    end = np.where(coords, win["end"], np.where(some, pos[np.maximum(hi, 1) - 1] if n else 0, 0)).astype(np.uint32)
    mid = (((start.astype(np.uint64) + end.astype(np.uint64)) & 0xFFFFFFFF) // 2).astype(np.uint32)  # u32 arithmetic, as the FST rows
    return start, end, mid


def model(pos, freqs, ninds, minind, win):
    """-> (rows[n_trios, n_win] of FD_ROW_DTYPE, totals[n_trios] of FD_TOTAL_DTYPE, A, A_tot): A[s][n_trios, n_win] and
    A_tot[s][n_trios] are Σ|site term| of sum s over the window's (all) counted sites."""
    assert np.finfo(np.longdouble).eps < 2e-19, "the model's prefix sums want the 80-bit long double"
    n = int(pos.size)
    trios = trio_order(len(freqs))
    o = len(freqs) - 1
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    rows = np.zeros((len(trios), win.size), dtype=FD_ROW_DTYPE)
    tot = np.zeros(len(trios), dtype=FD_TOTAL_DTYPE)
    A = {s: np.zeros((len(trios), win.size)) for s in SUMS}
    A_tot = {s: np.zeros(len(trios)) for s in SUMS}
    start, end, mid = coordinates(pos, win)
    for t, (i, j, k) in enumerate(trios):
        ok = counted(ninds, i, j, k, minind)
        terms = site_terms(freqs[i], freqs[j], freqs[k], freqs[o])
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        r = rows[t]
        r["start"], r["end"], r["mid"] = start, end, mid
        r["n"] = pn[hi] - pn[lo]
        for fld, x in zip(SUMS, terms):
            x = np.where(ok, x, 0.0).astype(np.longdouble)
            px = np.concatenate(([0], np.cumsum(x)))
            pa = np.concatenate(([0], np.cumsum(np.abs(x))))
            r[fld] = (px[hi] - px[lo]).astype(np.float64)
            A[fld][t] = (pa[hi] - pa[lo]).astype(np.float64)
            tot[fld][t] = float(px[-1])
            A_tot[fld][t] = float(pa[-1])
        r["fd"] = ratio(r["num"], r["fd_den"])
        r["fdm"] = ratio(r["num"], r["fdm_den"])
        tot["neff"][t] = int(pn[-1])
        tot["nskip"][t] = n - int(pn[-1])
    return rows, tot, A, A_tot
