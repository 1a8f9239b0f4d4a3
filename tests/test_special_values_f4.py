"""GPU: pgt_f4_pops_reduce_dev on NaN, infinite, denormal and edge-of-range frequencies and on counts over the whole int32 range
(include/pgtwin.h, "Values the columns admit").

One NaN, one +inf, one -inf and one denormal frequency are planted in ONE population, each at one COUNTED site: through the
build's reduce-scatter, the query's whole-quad loads, the level-2 nodes and the build waves' partials, only the rows of the
quartets that hold that population, and of them only the windows that hold such a site, change — to the sums the per-site
definition gives on the IEEE operands (special_inputs.window_sums, which carries NaN and infinities; assert_sums: the NaN mask
and the infinities exact, a finite sum within 1e-9 A + 1e-12, one-site windows bit for bit) — and every other row is, bit for
bit, the row of the clean run.  The same values planted at UNcounted sites change nothing at all.  Frequencies at the edge of
[0, 1] (-0.0, denormals, 1 - 2^-53, 0, 1) are ordinary values.  Counts of INT32_MIN, -1, 0, minind - 1, minind and INT32_MAX
under minind 1, 20 and INT32_MAX decide the predicate as a signed compare and nothing else.

Sizes: 8192 + 513 sites (leaf 512, level-2 tile 8192, a ragged last tile, n mod 4 = 1); K = 4 and 6 (both occupancies)."""
import numpy as np
import pytest

import f4_pops_model
import special_inputs as si
from f4_pops_model import SUMS, all_quartet_order
from helpers import rows_equal
from popgenomicstools_amd._lib import F4_ROW_DTYPE, F4_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, windows_to_device

pytestmark = pytest.mark.gpu

WHO = 1  # the population the values are planted in
PLANTED = {511: si.NAN, 4001: si.INF, 8192: -si.INF, si.POPS_N - 1: np.float64(5e-324)}  # a leaf's last site, inside a quad, a tile's first, the last


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(_dev())


def call(ctx, tp, f, c, minind, win):
    import torch
    out, tot, _ = ctx.f4_pops_reduce_dev(tp, [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    Q = len(all_quartet_order(len(f)))
    return rows_from_device(out, F4_ROW_DTYPE)[: Q * win.size].reshape(Q, win.size).copy(), rows_from_device(tot, F4_TOTAL_DTYPE)[:Q].copy()


def assert_against_the_definition(got, tot, f, c, minind, win, what):
    """every quartet's rows and genome-wide line against the model's per-site terms on the IEEE operands"""
    n = f[0].size
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    one = hi - lo == 1
    for t, (i, j, kk, l) in enumerate(all_quartet_order(len(f))):
        ok = si.pops_counted((i, j, kk, l), c, minind)
        assert np.array_equal(ok, f4_pops_model.counted(c, i, j, kk, l, np.int32(minind)))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        assert np.array_equal(got[t]["n"], (pn[hi] - pn[lo]).astype(np.uint32)), (what, t, "n")
        assert (int(tot[t]["neff"]), int(tot[t]["nskip"])) == (int(ok.sum()), n - int(ok.sum())), (what, t)
        assert not got[t]["reserved_"].view(np.uint64).any(), (what, t, "reserved_")
        terms, _ = f4_pops_model.site_terms(f[i], f[j], f[kk], f[l])
        for fld, x in zip(SUMS, terms):
            x = np.where(ok, x, 0.0)
            want, A, _ = si.window_sums(x, lo, hi)
            si.assert_sums(got[t][fld], want, A, f"{what} quartet {(i, j, kk, l)} {fld}")
            if one.any():
                si.assert_float_column(got[t][fld][one], want[one], f"{what} quartet {(i, j, kk, l)} {fld}, one-site windows")
            whole, A_all, _ = si.window_sums(x, [0], [n])
            si.assert_sums([tot[t][fld]], whole, A_all, f"{what} quartet {(i, j, kk, l)} genome-wide {fld}")


@pytest.mark.parametrize("k", [4, 6])
def test_special_frequencies_at_counted_sites_reach_exactly_their_quartets_and_windows(ctx, k):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c = si.pops_clean_columns(n, k, 6100 + k, planted=sites)  # the planted sites are counted for every population
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[WHO][s] = v
    quartets = all_quartet_order(k)
    for name, win in si.pops_tables(n, planted=sites):
        what = f"f4 K={k} table {name}"
        crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        unhit = si.windows_without(lo, hi, np.array(sites))
        assert unhit.any() or name == "(0,n)"
        assert (~unhit).any()
        for t, q in enumerate(quartets):
            if WHO not in q:
                rows_equal(got[t], crow[t], f"{what} quartet {q}, which does not hold population {WHO}")
                assert tot[t].tobytes() == ctot[t].tobytes(), (what, q, "genome-wide line")
                continue
            rows_equal(got[t][unhit], crow[t][unhit], f"{what} quartet {q}: windows without a planted site")
            assert got[t][~unhit].tobytes() != crow[t][~unhit].tobytes(), (what, q, "the planted values must show")
            for fld in ("start", "end", "mid", "n"):  # the values decide no count
                assert np.array_equal(got[t][fld], crow[t][fld]), (what, q, fld)
            for fld in SUMS:
                assert np.isnan(tot[t][fld])  # the NaN site is in every genome-wide line of the population's quartets
        assert_against_the_definition(got, tot, f, c, si.POPS_MININD, win, what)
        assert k == 4 or any(WHO not in q for q in quartets)


def test_special_frequencies_at_uncounted_sites_change_nothing(ctx):
    k, n = 5, si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c0 = si.pops_clean_columns(n, k, 6200, planted=sites)
    c = [x.copy() for x in c0]
    c[WHO][list(sites)] = si.POPS_MININD - 1  # population WHO is not counted there: no quartet that holds it counts the site
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[WHO][s] = v
    for name, win in si.pops_tables(n, planted=sites):
        crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        assert got.tobytes() == crow.tobytes() and tot.tobytes() == ctot.tobytes(), name
        assert all(np.all(np.isfinite(got[fld])) for fld in SUMS), name


@pytest.mark.parametrize("k", [4, 6])
def test_frequencies_at_the_edge_of_the_range_are_ordinary_values(ctx, k):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f0, c = si.pops_clean_columns(n, k, 6300 + k)
    m = len(si.POPS_PLANTED)
    edge = np.array(si.POPS_EDGE_VALUES)
    f = si.pops_plant(f0, {0: edge[np.arange(m) % edge.size], 1: edge[(np.arange(m) + 3) % edge.size], k - 1: edge[(np.arange(m) + 1) % edge.size]})
    for name, win in si.pops_tables(n):
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        assert all(np.all(np.isfinite(got[fld])) for fld in SUMS), name
        assert_against_the_definition(got, tot, f, c, si.POPS_MININD, win, f"f4 K={k} edge values, table {name}")


@pytest.mark.parametrize("minind", si.POPS_MININDS)
def test_counts_over_the_whole_int32_range_decide_the_predicate_only(ctx, minind):
    """nInd of INT32_MIN, -1, 0, minind - 1, minind and INT32_MAX: a signed compare, and no count enters a value — the rows are
    those of the same columns with every counted site's count replaced by minind and every other by 0."""
    k, n = 5, si.POPS_N
    assert si.POPS_MININDS == (1, 20, si.I32_MAX)
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns("f4", k, minind)
    present = set(np.concatenate(c).tolist())
    assert {si.I32_MIN, -1, 0, si.I32_MAX} <= present and minind in present
    flat = [np.where(x >= np.int32(minind), np.int32(minind), np.int32(0)).astype(np.int32) for x in c]
    for name, win in si.pops_tables(n):
        got, tot = call(ctx, tp, f, c, minind, win)
        assert_against_the_definition(got, tot, f, c, minind, win, f"f4 minind={minind} table {name}")
        same, same_t = call(ctx, tp, f, flat, minind, win)
        assert got.tobytes() == same.tobytes() and tot.tobytes() == same_t.tobytes(), (minind, name)
        assert np.all(tot["neff"] > 0) and np.all(tot["nskip"] > 0)  # both kinds of site, for every quartet
