"""GPU: pgt_f4ratio_pops_reduce_dev on NaN, infinite, denormal and edge-of-range frequencies and on counts over the whole int32
range (include/pgtwin.h, "Values the columns admit"), with the patterns of tests/test_special_values_f4.py.

One NaN, one +inf, one -inf and one denormal frequency are planted in ONE population, each at one COUNTED site: through the
build's reduce-scatter, the query's whole-quad loads, the level-2 nodes and the build waves' partials, only the rows of the
triples that hold that population (every triple, when it is A), and of them only the windows that hold such a site, change — to
the sums the per-site definition gives on the IEEE operands (special_inputs.window_sums, which carries NaN and infinities;
assert_sums: the NaN mask and the infinities exact, a finite sum within 1e-9 A + 1e-12, one-site windows bit for bit) — and
every other row is, bit for bit, the row of the clean run; within a triple that holds a middle population, the sum of the pair
WITHOUT it keeps its bits too.  The same values planted at UNcounted sites change nothing at all.  Frequencies at the edge of
[0, 1] (-0.0, denormals, 1 - 2^-53, 0, 1) are ordinary values.  Counts of INT32_MIN, -1, 0, minind - 1, minind and INT32_MAX
under minind 1, 20 and INT32_MAX decide the predicate as a signed compare and nothing else.

Sizes: 8192 + 513 sites (leaf 512, level-2 tile 8192, a ragged last tile, n mod 4 = 1); K = 5 and 7 (both build occupancies,
both query launch bounds)."""
import numpy as np
import pytest

import f4ratio_pops_model as model
import special_inputs as si
from f4ratio_pops_model import SUMS, middle_triple_order
from helpers import rows_equal
from popgenomicstools_amd._lib import F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, windows_to_device
from test_special_values_f4 import PLANTED, _dev, _t  # NaN, +inf, -inf, a denormal: a leaf's last site, inside a quad, a tile's first, the last

pytestmark = pytest.mark.gpu


def call(ctx, tp, f, c, minind, win):
    import torch
    out, tot, _ = ctx.f4ratio_pops_reduce_dev(tp, [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    T = len(middle_triple_order(len(f)))
    return rows_from_device(out, F4RATIO_ROW_DTYPE)[: T * win.size].reshape(T, win.size).copy(), rows_from_device(tot, F4RATIO_TOTAL_DTYPE)[:T].copy()


def sums_that_read(who, triple, k):
    """the sums of a triple's row whose per-site product reads population `who`: all three for A and O (through e), else the two
    of the pairs that hold it"""
    i, j, kk = triple
    if who in (0, k - 1):
        return list(SUMS)
    return [s for s, pair in zip(SUMS, ((i, j), (i, kk), (j, kk))) if who in pair]


def assert_against_the_definition(got, tot, f, c, minind, win, what):
    """every triple's rows and genome-wide line against the model's per-site terms on the IEEE operands"""
    n, k = f[0].size, len(f)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    one = hi - lo == 1
    for t, (i, j, kk) in enumerate(middle_triple_order(k)):
        ok = si.pops_counted((0, k - 1, i, j, kk), c, minind)
        assert np.array_equal(ok, model.counted(c, i, j, kk, np.int32(minind)))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        assert np.array_equal(got[t]["n"], (pn[hi] - pn[lo]).astype(np.uint32)), (what, t, "n")
        assert (int(tot[t]["neff"]), int(tot[t]["nskip"])) == (int(ok.sum()), n - int(ok.sum())), (what, t)
        assert not got[t]["reserved_"].view(np.uint64).any(), (what, t, "reserved_")
        terms, _ = model.site_terms(f[0], f[k - 1], f[i], f[j], f[kk])
        for fld, x in zip(SUMS, terms):
            x = np.where(ok, x, 0.0)
            want, A, _ = si.window_sums(x, lo, hi)
            si.assert_sums(got[t][fld], want, A, f"{what} triple {(i, j, kk)} {fld}")
            if one.any():
                si.assert_float_column(got[t][fld][one], want[one], f"{what} triple {(i, j, kk)} {fld}, one-site windows")
            whole, A_all, _ = si.window_sums(x, [0], [n])
            si.assert_sums([tot[t][fld]], whole, A_all, f"{what} triple {(i, j, kk)} genome-wide {fld}")


@pytest.mark.parametrize("k,who", [(5, 2), (7, 2), (6, 0), (6, 5)], ids=["K5-middle", "K7-middle", "K6-A", "K6-O"])
def test_special_frequencies_at_counted_sites_reach_exactly_their_triples_and_windows(ctx, k, who):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c = si.pops_clean_columns(n, k, 9100 + 10 * k + who, planted=sites)  # the planted sites are counted for every population
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[who][s] = v
    triples = middle_triple_order(k)
    for name, win in si.pops_tables(n, planted=sites):
        what = f"f4ratio K={k} population {who} table {name}"
        crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        unhit = si.windows_without(lo, hi, np.array(sites))
        assert unhit.any() or name == "(0,n)"
        assert (~unhit).any()
        for t, q in enumerate(triples):
            hit = sums_that_read(who, q, k)
            if not hit:
                rows_equal(got[t], crow[t], f"{what} triple {q}, which does not hold population {who}")
                assert tot[t].tobytes() == ctot[t].tobytes(), (what, q, "genome-wide line")
                continue
            rows_equal(got[t][unhit], crow[t][unhit], f"{what} triple {q}: windows without a planted site")
            assert got[t][~unhit].tobytes() != crow[t][~unhit].tobytes(), (what, q, "the planted values must show")
            for fld in ("start", "end", "mid", "n"):  # the values decide no count
                assert np.array_equal(got[t][fld], crow[t][fld]), (what, q, fld)
            for fld in SUMS:
                if fld in hit:
                    assert np.isnan(tot[t][fld])  # the NaN site is in every genome-wide line that reads the population
                else:  # the pair without the population: its sum never saw the values
                    assert got[t][fld].tobytes() == crow[t][fld].tobytes() and tot[t][fld].tobytes() == ctot[t][fld].tobytes(), (what, q, fld)
        assert_against_the_definition(got, tot, f, c, si.POPS_MININD, win, what)
    if (k, who) == (7, 2):
        assert [q for q in triples if not sums_that_read(who, q, k)] == [(1, 3, 4), (1, 3, 5), (1, 4, 5), (3, 4, 5)]


def test_special_frequencies_at_uncounted_sites_change_nothing(ctx):
    """population `who` below minind at the planted sites — a middle population, A, or O: no triple that reads it counts them"""
    k, n = 6, si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c0 = si.pops_clean_columns(n, k, 9200, planted=sites)
    for who in (1, 0, k - 1):
        c = [x.copy() for x in c0]
        c[who][list(sites)] = si.POPS_MININD - 1
        f = [x.copy() for x in f0]
        for s, v in PLANTED.items():
            f[who][s] = v
        for name, win in si.pops_tables(n, planted=sites):
            crow, ctot = call(ctx, tp, f0, c, si.POPS_MININD, win)
            got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
            assert got.tobytes() == crow.tobytes() and tot.tobytes() == ctot.tobytes(), (who, name)
            assert all(np.all(np.isfinite(got[fld])) for fld in SUMS), (who, name)


@pytest.mark.parametrize("k", [5, 7])
def test_frequencies_at_the_edge_of_the_range_are_ordinary_values(ctx, k):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f0, c = si.pops_clean_columns(n, k, 9300 + k)
    m = len(si.POPS_PLANTED)
    edge = np.array(si.POPS_EDGE_VALUES)
    f = si.pops_plant(f0, {0: edge[np.arange(m) % edge.size], 1: edge[(np.arange(m) + 3) % edge.size], k - 1: edge[(np.arange(m) + 1) % edge.size]})
    for name, win in si.pops_tables(n):
        got, tot = call(ctx, tp, f, c, si.POPS_MININD, win)
        assert all(np.all(np.isfinite(got[fld])) for fld in SUMS), name
        assert_against_the_definition(got, tot, f, c, si.POPS_MININD, win, f"f4ratio K={k} edge values, table {name}")


@pytest.mark.parametrize("minind", si.POPS_MININDS)
def test_counts_over_the_whole_int32_range_decide_the_predicate_only(ctx, minind):
    """nInd of INT32_MIN, -1, 0, minind - 1, minind and INT32_MAX: a signed compare, and no count enters a value — the rows are
    those of the same columns with every counted site's count replaced by minind and every other by 0.  (Five populations must
    pass at a counted site: A and O get a passing count at three sites in four, so that every triple keeps some.)"""
    k, n = 6, si.POPS_N
    assert si.POPS_MININDS == (1, 20, si.I32_MAX)
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns("f4ratio", k, minind)
    rng = np.random.default_rng([32, minind % 1000])
    for who in (0, k - 1):
        c[who] = np.where(rng.random(n) < 0.75, rng.choice(np.array([minind, si.I32_MAX], dtype=np.int32), n), c[who]).astype(np.int32)
    present = set(np.concatenate(c).tolist())
    assert {si.I32_MIN, -1, 0, si.I32_MAX} <= present and minind in present
    flat = [np.where(x >= np.int32(minind), np.int32(minind), np.int32(0)).astype(np.int32) for x in c]
    for name, win in si.pops_tables(n):
        got, tot = call(ctx, tp, f, c, minind, win)
        assert_against_the_definition(got, tot, f, c, minind, win, f"f4ratio minind={minind} table {name}")
        same, same_t = call(ctx, tp, f, flat, minind, win)
        assert got.tobytes() == same.tobytes() and tot.tobytes() == same_t.tobytes(), (minind, name)
        assert np.all(tot["neff"] > 0) and np.all(tot["nskip"] > 0)  # both kinds of site, for every triple
