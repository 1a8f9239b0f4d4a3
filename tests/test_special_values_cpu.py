"""CPU: the expectations of tests/test_special_values.py hold by the reference's rules alone.

The GPU tests expect the oracle's rows on columns that carry NaN and infinities.  Here the oracle itself is held, on those very
columns, to a few lines of numpy that restate the reference's rule for the extreme score ("the window's first site, unless a
later key is strictly greater", ihsWindow.cpp:194-201), and the inputs are checked to have the shapes the GPU tests claim."""
import numpy as np

import special_inputs as si


def test_extreme_expectations_are_the_first_site_rule(oracle):
    chr_ids, pos, chr_len = si.extreme_layout()
    seen = set()
    for W, rot in si.EXT_RUNS:
        for cl in (chr_len, None):
            table = oracle.extreme_scan(chr_ids, pos, np.zeros(si.EXT_N), W, 0, 2.0, cl)  # the table depends on pos alone
            lo, hi = table["lo"].astype(np.int64), table["hi"].astype(np.int64)
            score, used = si.extreme_scores(lo, hi, rot)
            seen |= used
            for mode, cutoff in si.EXT_MODES:
                ref = oracle.extreme_scan(chr_ids, pos, score, W, mode, cutoff, cl)
                assert np.array_equal(ref["lo"], table["lo"]) and np.array_equal(ref["hi"], table["hi"])
                at, nbig = si.extreme_model(score, lo, hi, mode, cutoff)
                some = at >= 0
                assert np.array_equal(ref["nsites"], hi - lo) and np.array_equal(some, ref["nsites"] > 0)
                assert np.array_equal(ref["nbig"], nbig), (W, rot, mode)
                assert np.array_equal(ref["position"], np.where(some, pos[np.maximum(at, 0)], 0)), (W, rot, mode)
                si.assert_selected_column(ref["value"], np.where(some, score[np.maximum(at, 0)], 0.0), f"W={W} rot={rot} mode={mode}")
            if W == 64:  # the shapes the GPU test names are really there
                key_nan = np.isnan(score)
                first_nan = np.array([b > a and key_nan[a] for a, b in zip(lo, hi)])
                all_nan = np.array([b > a and key_nan[a:b].all() for a, b in zip(lo, hi)])
                later_only = np.array([b > a and not key_nan[a] and key_nan[a:b].any() for a, b in zip(lo, hi)])
                one_site_nan = np.array([b - a == 1 and key_nan[a] for a, b in zip(lo, hi)])
                all_ninf = np.array([b - a >= 4 and np.all(score[a:b] == -np.inf) for a, b in zip(lo, hi)])
                all_pinf = np.array([b - a >= 4 and np.all(score[a:b] == np.inf) for a, b in zip(lo, hi)])
                assert first_nan.any() and all_nan.any() and later_only.any() and one_site_nan.any() and all_ninf.any() and all_pinf.any()
    assert seen == set(si.EXT_SHAPES)


def test_the_probe_of_eight_sites(oracle):
    """scores [nan, 1, 3 | 1, nan, .5 | nan, nan] in three 10-bp windows, |iHS| with cutoff 2: the literal known answer."""
    pos = np.array([1, 2, 3, 11, 12, 13, 21, 22], dtype=np.uint32)
    score = np.array([np.nan, 1, 3, 1, np.nan, .5, np.nan, np.nan])
    ref = oracle.extreme_scan(np.zeros(8, np.uint32), pos, score, 10, 0, 2.0, None)
    assert [(int(r["nsites"]), int(r["nbig"]), int(r["position"])) for r in ref] == [(3, 1, 1), (3, 0, 11), (2, 0, 21)]
    assert np.isnan(ref["value"][0]) and ref["value"][1] == 1.0 and np.isnan(ref["value"][2])


def test_special_fst_columns_sum_the_same_in_any_order(oracle):
    """The oracle adds a window's sites first to last; the query strategies add them in other orders.  On the planted columns
    the sum must not depend on the order: forwards, backwards and pairwise (numpy) agree under the comparison rule."""
    for n, tables in ((si.FST_N, ((300, 1), (5, 2), (1000, 250))), (si.FST_GROUP_N, ((20_000, 100),))):
        a, b, planted, a0, b0 = si.fst_special_columns(n, 5)
        assert planted.size == 10 and np.isnan(a[planted]).sum() + np.isnan(b[planted]).sum() == 3
        chr_ids, pos = si.two_chromosomes(n)
        for W, S in tables:
            ref = oracle.fst_scan(chr_ids, pos, a, b, W, S)
            clean = si.windows_without(ref["lo"], ref["hi"], planted)
            assert clean.any() and (~clean).any()
            with np.errstate(all="ignore"):
                for col, name in ((a, "num"), (b, "den")):
                    back = np.array([col[int(l):int(h)][::-1].cumsum()[-1] + 0.0 for l, h in zip(ref["lo"], ref["hi"])], dtype=np.float64)
                    pairwise = np.array([col[int(l):int(h)].sum() + 0.0 for l, h in zip(ref["lo"], ref["hi"])])
                    si.assert_float_column(back, ref[name], f"n={n} W={W} S={S} {name} summed backwards")
                    si.assert_float_column(pairwise, ref[name], f"n={n} W={W} S={S} {name} summed pairwise")
            ref0 = oracle.fst_scan(chr_ids, pos, a0, b0, W, S)
            for f in ("value", "num", "den"):
                assert np.array_equal(si.bits(ref[f][clean]), si.bits(ref0[f][clean]))


def test_het_bytes_and_division_inputs_cover_what_they_claim():
    g = si.het_bytes_column()
    assert g.dtype == np.int8 and g.size == si.HET_N and np.unique(g).size == 256
    for short in (True, False):
        lo, hi = si.het_windows(si.HET_N, short)
        assert {int(x) % 16 for x in lo} == set(range(16)) and {int(x) % 16 for x in hi} == set(range(16))
        assert int((hi - lo).max()) < 65536 if short else int((hi - lo).max()) == si.HET_N
    a, b = si.division_columns()
    with np.errstate(all="ignore"):
        q = a / b
    tiny = np.ldexp(1.0, -1022)
    assert a.size == b.size < 30_000
    assert (np.abs(a[a != 0]) < tiny).any() and ((b < tiny) & (b > 0)).any()          # denormal numerators, denominators
    assert ((np.abs(q) < tiny) & (q != 0)).any() and ((q == 0) & (a != 0) & np.isfinite(b)).any()  # quotients that underflow
    assert (np.isinf(q) & np.isfinite(a) & (b != 0)).any() and np.isnan(q).any()       # quotients that overflow; inf / inf
