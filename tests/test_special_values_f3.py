"""GPU: pgt_f3_pops_reduce_dev on NaN, infinite and denormal frequencies (include/pgtwin.h, "Values the columns admit").

One NaN, one +inf, one -inf and one denormal frequency are planted in ONE population, each at one COUNTED site: through the
build's reduce-scatter, the query's whole-quad loads, the level-2 nodes and the build waves' partials, only the rows of the
trios that hold that population, and of them only the windows that hold such a site, change — to the sums the per-site
definition gives on the IEEE operands (special_inputs.window_sums, which carries NaN and infinities; assert_sums: the NaN mask
and the infinities exact, a finite sum within 1e-9 A + 1e-12, one-site windows bit for bit) — and every other row is, bit for
bit, the row of the clean run.  The same values planted at UNcounted sites change nothing at all.

Sizes: 8192 + 513 sites (leaf 512, level-2 tile 8192, a ragged last tile, n mod 4 = 1); K = 4 and 6 (both occupancies)."""
import numpy as np
import pytest

import f3_pops_model
import special_inputs as si
from f3_pops_model import SUMS, all_trio_order
from helpers import rows_equal
from popgenomicstools_amd._lib import F3_ROW_DTYPE, F3_TOTAL_DTYPE
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
    out, tot, _ = ctx.f3_pops_reduce_dev(tp, [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    T = len(all_trio_order(len(f)))
    return rows_from_device(out, F3_ROW_DTYPE)[: T * win.size].reshape(T, win.size).copy(), rows_from_device(tot, F3_TOTAL_DTYPE)[:T].copy()


@pytest.mark.parametrize("k", [4, 6])
def test_special_frequencies_at_counted_sites_reach_exactly_their_trios_and_windows(ctx, k):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c = si.pops_clean_columns(n, k, 5100 + k, planted=sites)  # the planted sites are counted for every population
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[WHO][s] = v
    trios = all_trio_order(k)
    for name, win in si.pops_tables(n, planted=sites):
        what = f"f3 K={k} table {name}"
        crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        unhit = si.windows_without(lo, hi, np.array(sites))
        assert unhit.any() or name == "(0,n)"
        assert (~unhit).any()
        one = hi - lo == 1
        for t, ijk in enumerate(trios):
            if WHO not in ijk:
                rows_equal(got[t], crow[t], f"{what} trio {ijk}, which does not hold population {WHO}")
                assert tot[t].tobytes() == ctot[t].tobytes(), (what, ijk, "genome-wide line")
                continue
            rows_equal(got[t][unhit], crow[t][unhit], f"{what} trio {ijk}: windows without a planted site")
            assert got[t][~unhit].tobytes() != crow[t][~unhit].tobytes(), (what, ijk, "the planted values must show")
            for fld in ("start", "end", "mid", "n"):  # the values decide no count
                assert np.array_equal(got[t][fld], crow[t][fld]), (what, ijk, fld)
            assert (int(tot[t]["neff"]), int(tot[t]["nskip"])) == (int(ctot[t]["neff"]), int(ctot[t]["nskip"]))
            assert not got[t]["reserved_"].view(np.uint64).any(), (what, ijk, "reserved_")
            i, j, kk = ijk
            ok = f3_pops_model.counted(c, i, j, kk, si.POPS_MININD)
            terms, _ = f3_pops_model.site_terms(f[i], f[j], f[kk], c[i], c[j], c[kk])
            for fld, x in zip(SUMS, terms):
                x = np.where(ok, x, 0.0)
                want, A, _ = si.window_sums(x, lo, hi)
                si.assert_sums(got[t][fld], want, A, f"{what} trio {ijk} {fld}")
                if one.any():
                    si.assert_float_column(got[t][fld][one], want[one], f"{what} trio {ijk} {fld}, one-site windows")
                whole, A_all, _ = si.window_sums(x, [0], [n])
                si.assert_sums([tot[t][fld]], whole, A_all, f"{what} trio {ijk} genome-wide {fld}")
                assert np.isnan(tot[t][fld])  # the NaN site is in every genome-wide line of the population's trios


def test_special_frequencies_at_uncounted_sites_change_nothing(ctx):
    k, n = 4, si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c0 = si.pops_clean_columns(n, k, 5200, planted=sites)
    c = [x.copy() for x in c0]
    c[WHO][list(sites)] = si.POPS_MININD - 1  # population WHO is not counted there: no trio that holds it counts the site
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[WHO][s] = v
    for name, win in si.pops_tables(n, planted=sites):
        crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        assert got.tobytes() == crow.tobytes() and tot.tobytes() == ctot.tobytes(), name
        assert all(np.all(np.isfinite(got[fld])) for fld in SUMS), name
