"""CPU: the expectations of tests/test_special_values_pops.py hold by the models alone.

The GPU tests expect, for the K-population kernels, what the per-site definitions (the models' per-site functions) give at a
counted site that holds NaN, an infinity or an edge frequency, summed by special_inputs.window_sums.  Here the very inputs of
those tests are checked to have the shapes the tests claim, the direct-sum helper is held to the prefix-sum models on clean
inputs, and the float64 models are held to exact rationals wherever the GPU tests use them as the reference for a tolerance."""
import numpy as np
import pytest

import dstat_jack_model
import dstat_pops_model
import fd_pops_model
import fst_hudson_model
import fst_pops_model
import helpers
import pi_pops_model
import special_inputs as si

MODELS = {"fst": fst_pops_model, "fst_hudson": fst_hudson_model, "pi": pi_pops_model, "dstat": dstat_pops_model, "fd": fd_pops_model}


def _terms(stat, item, f, c, minind):
    ok = si.pops_counted(item, c, minind)
    return ok, [np.where(ok, x, 0.0) for x in si.pops_site_terms(stat, item, f, c)]


# ---- the helper ----------------------------------------------------------------------------------------------------------------
def test_window_sums_rule():
    t = np.array([1.0, np.nan, 2.0, np.inf, 3.0, -np.inf, -0.0, 0.0, 0.5, np.inf, np.inf, 2.0 ** -1074, -(2.0 ** -1074)])
    lo = np.array([0, 0, 2, 2, 3, 4, 5, 6, 6, 9, 11, 11, 8, 3])
    hi = np.array([1, 2, 3, 5, 6, 5, 6, 8, 9, 11, 12, 13, 8, 4])
    want, A, finite = si.window_sums(t, lo, hi)
    expect = np.array([1.0, np.nan, 2.0, np.inf, np.nan, 3.0, -np.inf, 0.0, 0.5, np.inf, 2.0 ** -1074, 0.0, 0.0, np.inf])
    si.assert_float_column(want, expect, "window_sums")  # -0.0 + 0.0 and the empty window are +0.0
    assert np.array_equal(finite, np.isfinite(expect))
    assert np.array_equal(A == 0, np.array([0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1], dtype=bool))
    assert A[3] == 5.0 and A[11] == 2.0 ** -1073
    with pytest.raises(AssertionError):
        si.window_sums(np.array([1.0, 9.0]), [0], [2])
    # the comparison rule refuses what it must
    si.assert_sums(want, expect, A, "itself")
    for i, v in ((0, np.nan), (1, 1.0), (3, -np.inf), (3, 1e308), (7, -0.0), (2, 2.0 + 1e-8), (10, 2e-12)):
        bad = want.copy()
        bad[i] = v
        with pytest.raises(AssertionError):
            si.assert_sums(bad, expect, A, "a wrong sum")
    ok = want.copy()
    ok[2] += 1e-9
    si.assert_sums(ok, expect, A, "inside the bound")


@pytest.mark.parametrize("stat,k", [("dxy", 3), ("fst", 3), ("fst_hudson", 8), ("pi", 2), ("dstat", 5), ("fd", 5)])
def test_direct_sums_equal_the_prefix_sum_models_on_clean_columns(stat, k):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    f, c = si.pops_clean_columns(n, k, 400 + k)
    model, fields = (fst_hudson_model, ("bsum",)) if stat == "dxy" else (MODELS[stat], si.POPS_SUMS[stat])  # Hudson's denominator IS dxy
    for name, win in si.pops_tables():
        res = model.model(pos, f, c, si.POPS_MININD, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        for t, item in enumerate(si.pops_items(stat, k)):
            ok, terms = _terms(stat, item, f, c, si.POPS_MININD)
            cnt = np.concatenate(([0], np.cumsum(ok)))
            assert np.array_equal(res[0][t]["neff" if stat == "pi" else "n"], cnt[hi] - cnt[lo])
            for fld, x in zip(fields, terms):
                want, A, finite = si.window_sums(x, lo, hi)
                assert finite.all()
                si.assert_sums(res[0][t][fld], want, A, f"{stat} K={k} {name} item {item} {fld}")
                whole, A_all, _ = si.window_sums(x, [0], [n])
                si.assert_sums([res[1][t][fld]], whole, A_all, f"{stat} K={k} item {item} genome-wide {fld}")


# ---- section 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat,k", si.POPS_SECTION1)
def test_planted_columns_have_the_shapes_the_gpu_test_claims(stat, k):
    """Every finite term is at most 8 (window_sums asserts it; with at most 532 485 sites no partial sum can overflow, so no
    window mixes an infinity made by overflow with a planted one); every table but the whole-column window has windows with and
    without a planted site; the planted sites are counted; NaN reaches every window of a holder that holds a planted site; the
    edge values leave every term finite."""
    n = si.POPS_N
    planted = np.array(si.POPS_PLANTED)
    f0, c = si.pops_clean_columns(n, k, 100 * k + len(stat))
    tables = si.pops_tables()
    for name, win in tables:
        hit = ~si.windows_without(win["lo"], win["hi"], planted)
        assert hit.any() and (name == "(0,n)" or (~hit).any()), name
    assert planted[3] + 1 == planted[4] and planted[3] // 4 == planted[4] // 4 and (n - 1) // 4 * 4 + 4 > n
    for run, plan in si.pops_runs(stat, k):
        f = si.pops_plant(f0, plan)
        for item in si.pops_items(stat, k):
            if not set(item) & set(plan):
                continue
            ok, terms = _terms(stat, item, f, c, si.POPS_MININD)
            assert ok[planted].all()
            for name, win in tables:
                hit = ~si.windows_without(win["lo"], win["hi"], planted)
                for x in terms:
                    want, A, finite = si.window_sums(x, win["lo"], win["hi"])
                    assert np.isfinite(A).all() and finite[~hit].all()
                    if run == "edge values":
                        assert finite.all()
                    if run.startswith("NaN") and stat != "fd":
                        assert np.array_equal(np.isnan(want), hit), (run, item, name)


def test_fd_asymmetries_of_the_definition_occur():
    """NaN in P2 leaves fd_den finite (H = L = P3: every comparison is false) while num and fdm_den are NaN; NaN in P1 leaves
    fdm_den finite (G = S = P3) while num and fd_den are NaN; NaN in P3 or in the outgroup poisons all three."""
    k, n = 4, si.POPS_N
    f0, c = si.pops_clean_columns(n, k, 100 * k + 2)
    planted = np.array(si.POPS_PLANTED)
    for who, finite_sum in ((0, "fdm_den"), (1, "fd_den"), (2, None), (3, None)):
        f = si.pops_plant(f0, {who: si.NAN})
        ok, terms = _terms("fd", (0, 1, 2, 3), f, c, si.POPS_MININD)
        for fld, x in zip(si.POPS_SUMS["fd"], terms):
            assert np.array_equal(np.isnan(x[planted]), np.full(planted.size, fld != finite_sum)), (who, fld)
            assert np.isfinite(np.delete(x, planted)).all()


# ---- section 2 -------------------------------------------------------------------------------------------------------------------
def test_denormal_columns_reach_denormal_sums_zero_denominators_and_denormal_quotients():
    """Per kernel: some sums are denormal, some are 0 in a window that has counted sites, and (where the row has a ratio) some
    denominator is 0 with its numerator 0.  A denormal QUOTIENT needs a numerator sum far smaller than its denominator sum: the
    terms of D's and Hudson's two sums are of one magnitude site by site, so only f_d, whose numerator term cancels to 0 at a
    site where its denominator terms do not, can and does produce one."""
    tiny = 2.0 ** -1022
    for stat, k in si.DENORMAL_CASES:
        f, c = si.denormal_columns(k)
        for x in f:
            nz = x[x != 0]
            assert np.all((x >= 0) & (x <= 0.5)) and np.array_equal(np.ldexp(1.0, np.round(np.log2(nz)).astype(int)), nz)
        seen = {"denormal sum": False, "zero sum": False, "zero denominator": False, "denormal quotient": False}
        for name, win in si.denormal_tables():
            lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
            for item in si.pops_items(stat, k):
                ok, terms = _terms(stat, item, f, c, si.POPS_MININD)
                cnt = np.concatenate(([0], np.cumsum(ok)))
                some = cnt[hi] > cnt[lo]
                sums = {}
                for fld, x in zip(si.POPS_SUMS[stat], terms):
                    sums[fld], _, finite = si.window_sums(x, lo, hi)
                    assert finite.all()
                    seen["denormal sum"] |= bool(np.any((np.abs(sums[fld]) < tiny) & (sums[fld] != 0)))
                    seen["zero sum"] |= bool(np.any((sums[fld] == 0) & some))
                row = np.zeros(lo.size, dtype=si.pops_dtypes(stat)[0])
                for fld in sums:
                    row[fld] = sums[fld]
                den = {"fst_hudson": "bsum", "fd": "fd_den"}.get(stat)
                if stat == "dstat":
                    seen["zero denominator"] |= bool(np.any((row["abba"] + row["baba"] == 0) & some))
                elif den:
                    seen["zero denominator"] |= bool(np.any((row[den] == 0) & (row[si.POPS_SUMS[stat][0]] == 0) & some))
                for fld, q in si.pops_ratios(stat, row):
                    assert np.isfinite(q).all()
                    seen["denormal quotient"] |= bool(np.any((np.abs(q) < tiny) & (q != 0)))
        assert seen["denormal sum"] and seen["zero sum"], (stat, seen)
        assert seen["zero denominator"] == (stat != "dxy"), (stat, seen)
        assert seen["denormal quotient"] == (stat == "fd"), (stat, seen)


# ---- section 3 -------------------------------------------------------------------------------------------------------------------
def test_extreme_counts_k_draws_the_six_values():
    for minind in si.POPS_MININDS + (0, -1, si.I32_MIN):
        c = si.extreme_counts_k(np.random.default_rng(1), 4000, minind, 3)
        want = {si.I32_MIN, -1, 0, max(minind - 1, si.I32_MIN), minind, si.I32_MAX}
        assert len(c) == 3 and all(x.dtype == np.int32 and set(x.tolist()) == want for x in c)


@pytest.mark.parametrize("realistic", [False, True])
@pytest.mark.parametrize("stat,k", [(s, k) for s, k in si.POPS_SMALLEST_LARGEST if s in si.POPS_VALUE_STATS])
def test_float64_models_meet_the_bound_against_exact_rationals(stat, k, realistic):
    """At the counted one-site windows the GPU test uses, the float64 per-site model of each statistic whose per-site function
    reads the counts is within 1e-9 scale + 1e-12 of the header's definition in exact rationals — at counts of INT32_MAX too —
    so the reference alone meets the tolerance asked of the kernel; and every window has 0 < neff < n."""
    for minind in ((si.REALISTIC_MININD,) if realistic else si.POPS_MININDS):
        f, c = si.count_case_columns(stat, k, minind, realistic)
        win = si.counted_site_table(stat, k, c, minind)
        at = win["lo"].astype(np.int64)
        assert 300 <= at.size <= 600
        for item in si.pops_items(stat, k):
            ok, terms = _terms(stat, item, f, c, minind)
            assert 0 < int(ok.sum()) < si.POPS_N and np.isfinite(np.stack(terms)).all() and np.abs(np.stack(terms)).max() <= 8
            for s in at[ok[at]].tolist():
                exact = si.exact_site(stat, [f[x][s] for x in item], [c[x][s] for x in item])
                si.assert_within_exact([x[s] for x in terms], exact, f"{stat} K={k} minind={minind} item {item} site {s}")


@pytest.mark.parametrize("stat,k", [(s, k) for s, k in si.POPS_SMALLEST_LARGEST if s not in si.POPS_VALUE_STATS])
def test_extreme_counts_leave_counted_and_uncounted_sites_for_every_item(stat, k):
    for minind in si.POPS_MININDS + ((0, -1, si.I32_MIN) if stat == "dxy" else ()):
        f, c = si.count_case_columns(stat, k, minind)
        for item in si.pops_items(stat, k):
            neff = int(si.pops_counted(item, c, minind).sum())
            assert (neff == si.POPS_N) if minind == si.I32_MIN else (0 < neff < si.POPS_N), (stat, k, minind, item, neff)


# ---- section 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", si.JACK_U32_N_WIN)
def test_jackknife_float_model_meets_the_bound_at_weights_of_u32_max(n_win):
    rows = si.jack_u32_rows(n_win)
    used = rows["n"] > 0
    assert set(np.unique(rows["n"]).tolist()) == {0, 0xFFFFFFFF} and np.isnan(rows["abba"][~used]).all()
    assert 0.05 < np.mean(~used) < 0.25 and int(rows["n"][0].astype(np.uint64).sum()) > 2 ** 32
    exact = si.jack_u32_exact(n_win)
    for t in range(si.JACK_U32_TRIOS):
        for c, (e, fl) in enumerate(zip(exact[t], dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_float))):
            assert e["n_sites"] == fl["n_sites"] == int(used[t].sum()) * 0xFFFFFFFF and e["n_blocks"] == fl["n_blocks"] == int(used[t].sum())
            for key in ("d", "d_jack", "se"):
                assert helpers.close(fl[key], e[key]), (n_win, t, c, key, fl[key], e[key])


def test_the_recorded_exact_jackknife_is_the_models():
    """one trio of tests/golden/dstat_jack_u32_exact.json evaluated again"""
    n_win = si.JACK_U32_GOLDEN_N_WIN
    again = dstat_jack_model.jack_rows(si.jack_u32_rows(n_win)[1], dstat_jack_model.jack_exact)
    for e, a in zip(si.jack_u32_exact(n_win)[1], again):
        assert all(e[key] == a[key] for key in ("d", "d_jack", "se", "z", "n_sites", "n_blocks")), (e, a)
