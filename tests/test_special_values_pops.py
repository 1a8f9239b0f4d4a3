"""GPU: the K-population kernels (pgt_dxy_pops / fst_pops / fst_hudson_pops / pi_pops / dstat_pops / fd_pops _reduce_dev and
pgt_dstat_jackknife_dev) on NaN, infinite and edge frequencies AT COUNTED SITES, on rows whose sums are denormal or zero, on
counts and minind over the whole int32 range and on jackknife weights of 2^32 - 1 (include/pgtwin.h, "Values the columns admit").

The yardstick is the per-site definition — the per-site functions of the NumPy models, float64 with every operation rounded on
its own — summed per window by special_inputs.window_sums, which carries NaN and infinities (the models' prefix sums cannot).
Comparison (special_inputs.assert_sums): the NaN mask and the +-inf bits of a sum exact; a finite sum within 1e-9 A + 1e-12, A
the window's Σ|term| (any order of n <= 9e6 additions stays inside n 2^-53 A); a one-site window bit for bit the definition's
value + 0.0 (Weir-Cockerham excepted: its kernel evaluates an identity of the definition and is held to exact rationals);
counts exact; a ratio bit for bit the stated function of the row's own sums; every window WITHOUT a planted site, and every row
of an item that holds no planted population, bit for bit the row of the same call on the clean columns.
tests/test_special_values_pops_cpu.py shows, without a GPU, that the inputs have the shapes claimed here and that the float64
models meet these tolerances against exact rationals.

Sizes: 8192 + 513 sites (leaf 512, level-2 tile 8192, a ragged last tile, n mod 4 = 1); 524288 + 8192 + 5 for the two level-3
cases; 301 sites for the denormal rows; 129 and 4097 blocks for the jackknife."""
import numpy as np
import pytest

import special_inputs as si
from helpers import rows_equal
from popgenomicstools_amd.window_scan import rows_from_device, table_hints, windows_to_device

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(_dev())


def call(ctx, stat, tp, f, c, minind, win):
    """one <stat>_pops_reduce_dev call -> (rows[items, n_win], totals[items])"""
    import torch
    out, tot, _ = getattr(ctx, f"{stat}_pops_reduce_dev")(tp, [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    row, total = si.pops_dtypes(stat)
    T = len(si.pops_items(stat, len(f)))
    return rows_from_device(out, row)[: T * win.size].reshape(T, win.size).copy(), rows_from_device(tot, total)[:T].copy()


def check_counts(stat, row, tot, ok, lo, hi, pos, what):
    """coordinates and counts of one item's rows and genome-wide line, exact against the predicate"""
    cnt = np.concatenate(([0], np.cumsum(ok)))
    neff = (cnt[hi] - cnt[lo]).astype(np.uint32)
    start, end = pos[lo], pos[hi - 1]
    assert np.array_equal(row["start"], start) and np.array_equal(row["end"], end), (what, "coordinates")
    if "neff" in row.dtype.names:
        assert np.array_equal(row["neff"], neff) and np.array_equal(row["nskip"], (hi - lo).astype(np.uint32) - neff), (what, "neff / nskip")
    else:
        assert np.array_equal(row["n"], neff), (what, "n")
        assert np.array_equal(row["mid"], ((start.astype(np.uint64) + end.astype(np.uint64)) & 0xFFFFFFFF) // 2), (what, "mid")
    assert (int(tot["neff"]), int(tot["nskip"])) == (int(ok.sum()), int(ok.size - ok.sum())), (what, "genome-wide neff / nskip", tot)


def check_items(stat, items, got, tot, f, c, minind, win, pos, what, one_site_bits=True):
    """the rows and genome-wide lines of the items [(index, populations)] against the per-site definition"""
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    one = hi - lo == 1
    for t, item in items:
        w = f"{what} item {item}"
        ok = si.pops_counted(item, c, minind)
        check_counts(stat, got[t], tot[t], ok, lo, hi, pos, w)
        for fld, x in zip(si.POPS_SUMS[stat], si.pops_site_terms(stat, item, f, c)):
            x = np.where(ok, x, 0.0)
            want, A, _ = si.window_sums(x, lo, hi)
            si.assert_sums(got[t][fld], want, A, f"{w} {fld}")
            if one_site_bits and one.any():
                si.assert_float_column(got[t][fld][one], want[one], f"{w} {fld}, one-site windows")
            whole, A_all, _ = si.window_sums(x, [0], [ok.size])
            si.assert_sums([tot[t][fld]], whole, A_all, f"{w} genome-wide {fld}")
        for fld, q in si.pops_ratios(stat, got[t]):
            si.assert_float_column(got[t][fld], q, f"{w} {fld} from the row's own sums")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a special frequency at a counted site reaches exactly its items and windows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat,k", si.POPS_SECTION1)
def test_special_frequency_at_a_counted_site_reaches_exactly_its_items_and_windows(ctx, stat, k):
    """NaN in one ingroup population (for f_d as P1, P2 and P3 of trio 0), NaN in the outgroup (trio kernels), +inf, and the edge
    frequencies -0.0, 5e-324, 2^-1022, 1 - 2^-53, 0, 1, at sites 0, 511 | 512, 4000, 4001 (one quad), 8191 | 8192 and n - 1, all
    counted: through the build's reduce-scatter, the query's whole-quad loads, the level-2 nodes and the build waves' partials,
    an item that holds the population has the definition's sums in exactly the windows that hold such a site, and nothing else
    changes by a bit.  For f_d the definition selects OPERANDS by comparisons that are all false with a NaN: NaN in P2 leaves
    fd_den finite, NaN in P1 leaves fdm_den finite."""
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f0, c = si.pops_clean_columns(n, k, 100 * k + len(stat))
    planted = np.array(si.POPS_PLANTED)
    items = si.pops_items(stat, k)
    tables = si.pops_tables()
    clean = {name: call(ctx, stat, tp, f0, c, si.POPS_MININD, win) for name, win in tables}
    for run, plan in si.pops_runs(stat, k):
        f = si.pops_plant(f0, plan)
        asym = {"fd_den": False, "fdm_den": False}
        for name, win in tables:
            what = f"{stat} K={k}, {run}, table {name}"
            got, tot = call(ctx, stat, tp, f, c, si.POPS_MININD, win)
            crow, ctot = clean[name]
            unhit = si.windows_without(win["lo"], win["hi"], planted)
            holders = [(t, item) for t, item in enumerate(items) if set(item) & set(plan)]
            assert holders
            for t, item in enumerate(items):
                if (t, item) in holders:
                    rows_equal(got[t][unhit], crow[t][unhit], f"{what} item {item}: windows without a planted site")
                else:
                    rows_equal(got[t], crow[t], f"{what} item {item}, which holds no planted population")
                    assert tot[t].tobytes() == ctot[t].tobytes(), (what, item, "genome-wide line")
            check_items(stat, holders, got, tot, f, c, si.POPS_MININD, win, pos, what)
            if stat == "fd":
                r = got[0][~unhit]
                for fld in asym:
                    asym[fld] |= bool(np.any(np.isfinite(r[fld]) & np.isnan(r["num"])))
        if stat == "fd" and run.startswith("NaN"):
            want = {"NaN in population 0": (False, True), "NaN in population 1": (True, False)}.get(run, (False, False))
            assert (asym["fd_den"], asym["fdm_den"]) == want, (run, asym)


@pytest.mark.parametrize("stat,k", [("fd", 4), ("fst_hudson", 3)])
def test_nan_on_both_sides_of_a_level3_edge(ctx, stat, k):
    """524288 + 8192 + 5 sites: one level-3 node, NaN in population 1 at its last site and at the first site after it.  Windows
    that are the node, that miss its first site, that miss its last site, the rest of the column with and without the planted
    site, and the whole column: the two windows that avoid both sites keep the bits of the clean run."""
    n = si.POPS_L3_N
    pos = np.arange(1, n + 1, dtype=np.uint32)
    tp = _t(pos)
    planted = np.array(si.POPS_L3_PLANTED)
    f0, c = si.pops_clean_columns(n, k, 900 + k, planted=si.POPS_L3_PLANTED)
    f = si.pops_plant(f0, {1: si.NAN}, planted=si.POPS_L3_PLANTED)
    win = si.windows_of(si.POPS_L3_WINDOWS)
    unhit = si.windows_without(win["lo"], win["hi"], planted)
    assert int(unhit.sum()) == 2
    got, tot = call(ctx, stat, tp, f, c, si.POPS_MININD, win)
    crow, ctot = call(ctx, stat, tp, f0, c, si.POPS_MININD, win)
    items = si.pops_items(stat, k)
    holders = [(t, item) for t, item in enumerate(items) if 1 in item]
    for t, item in enumerate(items):
        if (t, item) in holders:
            rows_equal(got[t][unhit], crow[t][unhit], f"{stat} level 3 item {item}: windows without a planted site")
            fld = si.POPS_SUMS[stat][0]  # (f_d's fd_den stays finite with NaN in P2: check_items holds every sum to the definition)
            assert np.isnan(got[t][fld][~unhit]).all() and np.isfinite(crow[t][fld]).all(), (item, fld)
        else:
            rows_equal(got[t], crow[t], f"{stat} level 3 item {item}")
            assert tot[t].tobytes() == ctot[t].tobytes()
    check_items(stat, holders, got, tot, f, c, si.POPS_MININD, win, pos, f"{stat} level 3")
    check_items(stat, list(enumerate(items)), crow, ctot, f0, c, si.POPS_MININD, win, pos, f"{stat} level 3, clean columns")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. denormal and zero sums in a row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat,k", si.DENORMAL_CASES)
def test_denormal_and_zero_sums(ctx, stat, k):
    """Frequencies 2^-1074 ... 2^-1 and 0 (special_inputs.denormal_columns): sums that are denormal, that underflow to 0, and
    rows with den == 0 and num == 0 (ratio 0.0, not NaN).  One-site sums carry the definition's bits; a 7-site sum stays within
    the bound (exactly +0.0 where every term is a zero); the ratio is ONE correctly rounded division of the row's own sums,
    denormal quotients included."""
    f, c = si.denormal_columns(k)
    pos = np.arange(1, si.DENORMAL_N + 1, dtype=np.uint32)
    tp = _t(pos)
    items = list(enumerate(si.pops_items(stat, k)))
    tiny = 2.0 ** -1022
    denormal = 0
    for name, win in si.denormal_tables():
        got, tot = call(ctx, stat, tp, f, c, si.POPS_MININD, win)
        check_items(stat, items, got, tot, f, c, si.POPS_MININD, win, pos, f"{stat} K={k} denormal rows, {name}")
        for fld in si.POPS_SUMS[stat]:
            assert np.isfinite(got[fld]).all()
            denormal += int(np.count_nonzero((np.abs(got[fld]) < tiny) & (got[fld] != 0)))
    assert denormal > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. counts at their extremes
# ---------------------------------------------------------------------------------------------------------------------------
PREDICATE_CASES = [(s, k, m) for s, k in si.POPS_SMALLEST_LARGEST if s not in si.POPS_VALUE_STATS for m in si.POPS_MININDS]
VALUE_CASES = [(s, k, m) for s, k in si.POPS_SMALLEST_LARGEST if s in si.POPS_VALUE_STATS for m in si.POPS_MININDS + ("realistic",)]


def _ones_where_counted(c, minind):
    return [(x >= np.int32(minind)).astype(np.int32) for x in c]


@pytest.mark.parametrize("stat,k,minind", PREDICATE_CASES)
def test_extreme_counts_decide_nothing_but_the_predicate(ctx, stat, k, minind):
    """dxy, D, f_d with counts from {INT32_MIN, -1, 0, minind - 1, minind, INT32_MAX}: n / neff / nskip are the signed int32
    predicate's, and every row and genome-wide line is bit for bit that of counts 1 where counted, 0 where not, and minind 1."""
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns(stat, k, minind)
    ones = _ones_where_counted(c, minind)
    items = si.pops_items(stat, k)
    for name, win in si.pops_tables(with_one_site=False):
        what = f"{stat} K={k} minind={minind} table {name}"
        got, tot = call(ctx, stat, tp, f, c, minind, win)
        ref, rtot = call(ctx, stat, tp, f, ones, 1, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        for t, item in enumerate(items):
            ok = si.pops_counted(item, c, minind)
            assert 0 < int(ok.sum()) < n, (what, item)
            check_counts(stat, got[t], tot[t], ok, lo, hi, pos, f"{what} item {item}")
            rows_equal(got[t], ref[t], f"{what} item {item}")
        assert tot.tobytes() == rtot.tobytes(), what


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("minind", [0, -1, si.I32_MIN])
def test_dxy_pops_minind_below_one(ctx, k, minind):
    """pgt_dxy_pops_reduce_dev accepts minind < 1.  A site beyond n, whose count the build loads as 0, would pass such a
    predicate: only its mask keeps it out.  With minind = INT32_MIN every real site counts and no padded one: neff == hi - lo in
    every row, nskip == 0 in the genome-wide lines, the sums those of all-ones counts and minind 1.  The host-buffer form
    agrees, bit for bit under the hint it derives from the table."""
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns("dxy", k, minind)
    ones = _ones_where_counted(c, minind)
    items = si.pops_items("dxy", k)
    for name, win in si.pops_tables(with_one_site=False):
        what = f"dxy K={k} minind={minind} table {name}"
        got, tot = call(ctx, "dxy", tp, f, c, minind, win)
        ref, rtot = call(ctx, "dxy", tp, f, ones, 1, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        for t, item in enumerate(items):
            ok = si.pops_counted(item, c, minind)
            check_counts("dxy", got[t], tot[t], ok, lo, hi, pos, f"{what} item {item}")
            rows_equal(got[t], ref[t], f"{what} item {item}")
            if minind == si.I32_MIN:
                assert ok.all() and all(x.all() for x in ones)
                assert np.array_equal(got[t]["neff"], (hi - lo).astype(np.uint32)) and not got[t]["nskip"].any(), (what, item)
                assert (int(tot[t]["neff"]), int(tot[t]["nskip"])) == (n, 0), (what, item, tot[t])
            else:
                assert 0 < int(ok.sum()) < n, (what, item)
        assert tot.tobytes() == rtot.tobytes(), what
        check_items("dxy", list(enumerate(items)), got, tot, f, c, minind, win, pos, what)
        host, host_tot = ctx.dxy_pops_reduce(pos, f, c, minind, win)
        with ctx.hints(table_hints(win)[0], 0, 0):
            hinted, hinted_tot = call(ctx, "dxy", tp, f, c, minind, win)
        for t, item in enumerate(items):
            rows_equal(np.ascontiguousarray(host[t]), hinted[t], f"{what} item {item}, host-buffer form")
        assert host_tot.tobytes() == hinted_tot.tobytes(), (what, "host-buffer form, genome-wide lines")
        check_items("dxy", list(enumerate(items)), host, host_tot, f, c, minind, win, pos, what + ", host-buffer form")


@pytest.mark.parametrize("stat,k,minind", VALUE_CASES)
def test_extreme_and_realistic_counts_as_values(ctx, stat, k, minind):
    """Weir-Cockerham, Hudson and pi read the counts as VALUES: the signed compare at INT32_MIN / -1 / INT32_MAX, (double)nind at
    INT32_MAX, the reciprocal of a divisor up to 2^96 (Weir-Cockerham) and 2 nind - 1 (Hudson, pi).  Rows and genome-wide
    lines against the float64 per-site model summed directly; one-site windows at counted sites against the header's definition
    in exact rationals (Hudson and pi also bit for bit against the float64 model).  "realistic": counts uniform in
    1 ... 100 000, the same checks."""
    realistic = minind == "realistic"
    minind = si.REALISTIC_MININD if realistic else minind
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns(stat, k, minind, realistic)
    items = list(enumerate(si.pops_items(stat, k)))
    for t, item in items:
        assert 0 < int(si.pops_counted(item, c, minind).sum()) < n, item
    for name, win in si.pops_tables(with_one_site=False):
        got, tot = call(ctx, stat, tp, f, c, minind, win)
        check_items(stat, items, got, tot, f, c, minind, win, pos, f"{stat} K={k} minind={minind} table {name}")
    win = si.counted_site_table(stat, k, c, minind)
    at = win["lo"].astype(np.int64)
    got, tot = call(ctx, stat, tp, f, c, minind, win)
    what = f"{stat} K={k} minind={minind} one-site windows"
    check_items(stat, items, got, tot, f, c, minind, win, pos, what, one_site_bits=stat != "fst")
    for t, item in items:
        ok = si.pops_counted(item, c, minind)[at]
        assert ok.any()
        for w in np.flatnonzero(ok).tolist():
            exact = si.exact_site(stat, [f[x][at[w]] for x in item], [c[x][at[w]] for x in item])
            si.assert_within_exact([got[t][fld][w] for fld in si.POPS_SUMS[stat]], exact, f"{what} item {item} site {at[w]}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. jackknife weights beyond 2^32
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", si.JACK_U32_N_WIN)
def test_jackknife_weights_of_u32_max(ctx, n_win):
    """Every used block weighs 0xFFFFFFFF, one block in seven is unused (n = 0, NaN sums): Σn is kept in u64 and passes 2^32 at
    the second block.  n_sites and n_blocks exact; d, d_jack, se against the exact-rational model under the bound of
    tests/test_dstat_jack.py; z the quotient of the call's own d_jack and se."""
    from test_dstat_jack import assert_item, jack_dev
    rows = si.jack_u32_rows(n_win)
    got = jack_dev(ctx, rows)
    want = si.jack_u32_exact(n_win)
    for t in range(si.JACK_U32_TRIOS):
        used = int((rows["n"][t] > 0).sum())
        for c in range(3):
            assert want[t][c]["n_sites"] == used * 0xFFFFFFFF > 2 ** 32 and want[t][c]["n_blocks"] == used
            assert_item(got[t, c], want[t][c], f"n_win={n_win} trio {t} topology {c}")
