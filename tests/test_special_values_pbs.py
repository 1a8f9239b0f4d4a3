"""GPU: pgt_pbs_pops_reduce_dev / pgt_pbs_hudson_pops_reduce_dev on NaN, infinite, denormal and edge-of-range frequencies and on
counts over the whole int32 range (include/pgtwin.h, "Values the columns admit"), with the patterns of
tests/test_special_values_f3.py and tests/test_special_values_f4ratio.py.

PBS is two walks (the numerators, then the denominators) whose scratch rows a third kernel merges and closes with a logarithm,
and it reads the counts as VALUES through pgt_fst_site.h.  One NaN, one +inf, one -inf and one denormal frequency are planted in
ONE population, each at one COUNTED site: only the rows of the trios that hold that population, of them only the windows that
hold such a site, and of a row only the four sums of the two pairs that read the population, change; every other row, and the
pair WITHOUT the population in every window and in the genome-wide line, keeps the bits of the clean run.

What the changed sums are:
  Hudson            the per-site definition on the IEEE operands (pbs_pops_model.site_values, every operation rounded on its
                    own) summed by special_inputs.window_sums, compared by assert_sums (the NaN mask and the infinities exact, a
                    finite sum within 1e-9 A + 1e-12), one-site windows bit for bit.  At a frequency of +-inf the definition
                    gives num = +inf and den = NaN.
  Weir-Cockerham    the kernel evaluates an identity of the definition with ONE reciprocal per pair (pgt_fst_site.h): at a
                    frequency of +-inf its written form gives a = +inf where the model's division form gives NaN, so the class
                    of a non-finite sum is not the model's to decide.  The rule the header states is the one held here: a window
                    that holds the NaN site is NaN; a window that holds only +-inf sites is NON-FINITE, its class unspecified;
                    every other window is within 1e-9 A + 1e-12 of the model.
The finishing arithmetic of every row goes through test_pbs_pops.assert_finish (the model's finishing lines on the row's own
sums); all three pbs_* are NaN wherever a holder's window contains the NaN site.
The same values planted at UNcounted sites change nothing at all.  Frequencies at the edge of [0, 1] are ordinary values.
Denormal and zero sums: a counted row whose three denominators are 0 has pbs_* = +0.0 by its bits (fst = 0, T = -log(1) = -0.0,
and the + 0.0 that closes the finishing lines).  Counts from INT32_MIN to INT32_MAX: one-site windows against the header's
definition in exact rationals, and the third population of a pair decides membership only.
tests/test_pbs_pops_cpu.py shows, without a GPU, that the inputs have the shapes claimed here.

Sizes: 8192 + 513 sites (leaf 512, level-2 tile 8192, a ragged last tile, n mod 4 = 1); 524288 + 8192 + 5 for the level-3 case;
301 sites for the denormal rows; K = 3 and 6 (both build occupancies, both query launch bounds)."""
import numpy as np
import pytest

import pbs_pops_model
import special_inputs as si
from helpers import rows_equal
from pbs_pops_model import PAIRS, PBS, SUMS, all_trio_order, pairs_of
from popgenomicstools_amd._lib import PBS_ROW_DTYPE, PBS_TOTAL_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, windows_to_device
from test_pbs_pops import assert_finish, bits
from test_special_values_f3 import PLANTED, _dev, _t  # NaN, +inf, -inf, a denormal: a leaf's last site, inside a quad, a tile's first, the last
from test_special_values_pops import check_counts

pytestmark = pytest.mark.gpu
STAT = {"wc": "pbs", "hudson": "pbs_hudson"}
assert si.POPS_SUMS["pbs"] == si.POPS_SUMS["pbs_hudson"] == SUMS
NAN_SITE = [s for s, v in PLANTED.items() if np.isnan(v)]
INF_SITES = [s for s, v in PLANTED.items() if np.isinf(v)]


def call(ctx, est, tp, f, c, minind, win):
    import torch
    out, tot, _ = ctx.pbs_pops_reduce_dev(tp, [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()), estimator=est)
    torch.cuda.synchronize()
    T = len(all_trio_order(len(f)))
    return rows_from_device(out, PBS_ROW_DTYPE)[: T * win.size].reshape(T, win.size).copy(), rows_from_device(tot, PBS_TOTAL_DTYPE)[:T].copy()


def sums_that_read(who, ijk):
    """the sums of a trio's row whose per-site value reads population `who`: those of the two pairs that hold it"""
    return [f"{half}_{name}" for half in ("num", "den") for name, pair in zip(PAIRS, pairs_of(*ijk)) if who in pair]


def holds(lo, hi, sites):
    return ~si.windows_without(lo, hi, np.array(sorted(sites), dtype=np.int64))


def assert_sum(est, got, total, x, lo, hi, what, loose=False):
    """One sum of one trio against its per-site terms x (uncounted sites already 0.0).  loose (Weir-Cockerham with NaN and +-inf
    frequencies planted): NaN where the window holds the NaN site, non-finite where it holds only +-inf sites, the bound elsewhere."""
    n = x.size
    lo_all, hi_all = np.concatenate((lo, [0])), np.concatenate((hi, [n]))  # the genome-wide line is the window (0, n)
    got_all = np.concatenate((got, [total]))
    if loose:
        has_nan, has_inf = holds(lo_all, hi_all, NAN_SITE), holds(lo_all, hi_all, INF_SITES)
        assert np.isnan(got_all[has_nan]).all(), (what, "a window with the NaN site must be NaN")
        assert not np.isfinite(got_all[has_inf & ~has_nan]).any(), (what, "a window with an infinite frequency must not be finite")
        rest = ~(has_nan | has_inf)
        x = x.copy()
        x[NAN_SITE + INF_SITES] = 0.0  # in no window that is compared below
        want, A, _ = si.window_sums(x, lo_all[rest], hi_all[rest])
        si.assert_sums(got_all[rest], want, A, what)
        return
    want, A, _ = si.window_sums(x, lo_all, hi_all)
    si.assert_sums(got_all, want, A, what)
    one = hi_all - lo_all == 1
    if est == "hudson" and one.any():
        si.assert_float_column(got_all[one], want[one], f"{what}, one-site windows")


def assert_against_the_definition(est, got, tot, f, c, minind, win, pos, what, trios=None, loose=()):
    """the rows and genome-wide lines of the trios [(index, populations)] against the per-site definition on the IEEE operands;
    loose: the sums held to the Weir-Cockerham rule for non-finite frequencies"""
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    for t, ijk in (list(enumerate(all_trio_order(len(f)))) if trios is None else trios):
        w = f"{what} trio {ijk}"
        ok = si.pops_counted(ijk, c, minind)
        assert np.array_equal(ok, pbs_pops_model.counted(c, *ijk, np.int32(minind)))
        check_counts(STAT[est], got[t], tot[t], ok, lo, hi, pos, w)
        for fld, x in zip(SUMS, si.pops_site_terms(STAT[est], ijk, f, c)):
            assert_sum(est, got[t][fld], tot[t][fld], np.where(ok, x, 0.0), lo, hi, f"{w} {fld}", loose=fld in loose)
        assert_finish(got[t], w)
        assert_finish(tot[t:t + 1], w + " genome-wide")


# ---- planted at counted sites ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est,k,who", [("hudson", 3, 1), ("hudson", 6, 1), ("wc", 6, 4), ("wc", 3, 0)])
def test_special_frequencies_at_counted_sites_reach_exactly_their_trios_windows_and_pairs(ctx, est, k, who):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c = si.pops_clean_columns(n, k, 7100 + 10 * k + who, planted=sites)  # the planted sites are counted for every population
    f = [x.copy() for x in f0]
    for s, v in PLANTED.items():
        f[who][s] = v
    trios = all_trio_order(k)
    for name, win in si.pops_tables(n, planted=sites):
        what = f"pbs {est} K={k} population {who} table {name}"
        crow, ctot = call(ctx, est, tp, f0, c, si.POPS_MININD, win)
        got, tot = call(ctx, est, tp, f, c, si.POPS_MININD, win)
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        unhit = si.windows_without(lo, hi, np.array(sites))
        with_nan = holds(lo, hi, NAN_SITE)
        assert unhit.any() or name == "(0,n)"
        assert (~unhit).any() and with_nan.any()
        for t, ijk in enumerate(trios):
            hit = sums_that_read(who, ijk)
            if not hit:
                rows_equal(got[t], crow[t], f"{what} trio {ijk}, which does not hold population {who}")
                assert tot[t].tobytes() == ctot[t].tobytes(), (what, ijk, "genome-wide line")
                continue
            assert len(hit) == 4
            rows_equal(got[t][unhit], crow[t][unhit], f"{what} trio {ijk}: windows without a planted site")
            assert got[t][~unhit].tobytes() != crow[t][~unhit].tobytes(), (what, ijk, "the planted values must show")
            for fld in ("start", "end", "mid", "n"):  # the values decide no count
                assert np.array_equal(got[t][fld], crow[t][fld]), (what, ijk, fld)
            assert (int(tot[t]["neff"]), int(tot[t]["nskip"])) == (int(ctot[t]["neff"]), int(ctot[t]["nskip"]))
            for fld in SUMS:
                if fld in hit:
                    assert np.isnan(tot[t][fld]), (what, ijk, fld)  # the NaN site is in every genome-wide line that reads the population
                    assert np.isfinite(crow[t][fld]).all()
                else:  # the pair without the population: neither of its two walks saw the values
                    assert got[t][fld].tobytes() == crow[t][fld].tobytes() and tot[t][fld].tobytes() == ctot[t][fld].tobytes(), (what, ijk, fld)
            for fld in PBS:  # every pbs_* reads all three branches
                assert np.isnan(got[t][fld][with_nan]).all() and np.isnan(tot[t][fld]), (what, ijk, fld)
        for t, ijk in enumerate(trios):  # Hudson: every sum as the definition gives it; Weir-Cockerham: the rule for the sums that read `who`
            assert_against_the_definition(est, got, tot, f, c, si.POPS_MININD, win, pos, what, trios=[(t, ijk)],
                                          loose=sums_that_read(who, ijk) if est == "wc" else ())
    assert sum(1 for ijk in trios if who in ijk) == (k - 1) * (k - 2) // 2


@pytest.mark.parametrize("est", ["wc", "hudson"])
def test_special_frequencies_at_uncounted_sites_change_nothing(ctx, est):
    """population `who` below minind at the planted sites: no trio that reads it counts them, in either walk"""
    k, n = 6, si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    sites = tuple(PLANTED)
    f0, c0 = si.pops_clean_columns(n, k, 7200, planted=sites)
    for who in (1, k - 1):
        c = [x.copy() for x in c0]
        c[who][list(sites)] = si.POPS_MININD - 1
        f = [x.copy() for x in f0]
        for s, v in PLANTED.items():
            f[who][s] = v
        for name, win in si.pops_tables(n, planted=sites):
            crow, ctot = call(ctx, est, tp, f0, c, si.POPS_MININD, win)
            got, tot = call(ctx, est, tp, f, c, si.POPS_MININD, win)
            assert got.tobytes() == crow.tobytes() and tot.tobytes() == ctot.tobytes(), (est, who, name)
            assert all(np.all(np.isfinite(got[fld])) and np.all(np.isfinite(tot[fld])) for fld in SUMS), (est, who, name)


def test_nan_on_both_sides_of_a_level3_edge(ctx):
    """524288 + 8192 + 5 sites: one level-3 node, NaN in population 1 at its last site and at the first site after it.  The two
    windows that avoid both sites keep the bits of the clean run; the others hold NaN in the four sums that read the population,
    and the pair (0, 2) keeps its bits everywhere."""
    est, k, n = "hudson", 3, si.POPS_L3_N
    pos = np.arange(1, n + 1, dtype=np.uint32)
    tp = _t(pos)
    planted = np.array(si.POPS_L3_PLANTED)
    f0, c = si.pops_clean_columns(n, k, 7300, planted=si.POPS_L3_PLANTED)
    f = si.pops_plant(f0, {1: si.NAN}, planted=si.POPS_L3_PLANTED)
    win = si.windows_of(si.POPS_L3_WINDOWS)
    unhit = si.windows_without(win["lo"], win["hi"], planted)
    assert int(unhit.sum()) == 2
    got, tot = call(ctx, est, tp, f, c, si.POPS_MININD, win)
    crow, ctot = call(ctx, est, tp, f0, c, si.POPS_MININD, win)
    rows_equal(got[0][unhit], crow[0][unhit], "pbs level 3: windows without a planted site")
    hit = sums_that_read(1, (0, 1, 2))
    assert hit == ["num_ij", "num_jk", "den_ij", "den_jk"]
    for fld in SUMS:
        if fld in hit:
            assert np.isnan(got[0][fld][~unhit]).all() and np.isnan(tot[0][fld]) and np.isfinite(crow[0][fld]).all(), fld
        else:
            assert got[0][fld].tobytes() == crow[0][fld].tobytes() and tot[0][fld].tobytes() == ctot[0][fld].tobytes(), fld
    assert_against_the_definition(est, got, tot, f, c, si.POPS_MININD, win, pos, "pbs level 3")
    assert_against_the_definition(est, crow, ctot, f0, c, si.POPS_MININD, win, pos, "pbs level 3, clean columns")


@pytest.mark.parametrize("est", ["wc", "hudson"])
@pytest.mark.parametrize("k", [3, 6])
def test_frequencies_at_the_edge_of_the_range_are_ordinary_values(ctx, k, est):
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f0, c = si.pops_clean_columns(n, k, 7400 + k)
    m = len(si.POPS_PLANTED)
    edge = np.array(si.POPS_EDGE_VALUES)
    f = si.pops_plant(f0, {0: edge[np.arange(m) % edge.size], 1: edge[(np.arange(m) + 3) % edge.size], k - 1: edge[(np.arange(m) + 1) % edge.size]})
    for name, win in si.pops_tables(n):
        got, tot = call(ctx, est, tp, f, c, si.POPS_MININD, win)
        assert all(np.all(np.isfinite(got[fld])) and np.all(np.isfinite(tot[fld])) for fld in SUMS), name
        assert_against_the_definition(est, got, tot, f, c, si.POPS_MININD, win, pos, f"pbs {est} K={k} edge values, table {name}")


# ---- denormal and zero sums --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["wc", "hudson"])
def test_denormal_and_zero_sums(ctx, est):
    """Frequencies 2^-1074 ... 2^-1 and 0 (special_inputs.denormal_columns): sums that are denormal, that underflow to 0 (exactly
    +0.0 where every term is a zero), and counted rows whose three denominators are 0: fst = 0, T = -0.0, pbs_* = +0.0 by
    its bits, never NaN."""
    k = 3
    f, c = si.denormal_columns(k)
    pos = np.arange(1, si.DENORMAL_N + 1, dtype=np.uint32)
    tp = _t(pos)
    tiny = 2.0 ** -1022
    denormal = zero_den = 0
    for name, win in si.denormal_tables():
        got, tot = call(ctx, est, tp, f, c, si.POPS_MININD, win)
        assert_against_the_definition(est, got, tot, f, c, si.POPS_MININD, win, pos, f"pbs {est} denormal rows, {name}")
        r = got[0]
        for fld in SUMS:
            assert np.isfinite(r[fld]).all()
            denormal += int(np.count_nonzero((np.abs(r[fld]) < tiny) & (r[fld] != 0)))
        z = (r["n"] > 0) & (r["den_ij"] == 0) & (r["den_ik"] == 0) & (r["den_jk"] == 0)
        zero_den += int(z.sum())
        for fld in PBS:
            assert np.isfinite(r[fld]).all(), (name, fld)
            assert np.all(bits(r[fld][z]) == 0), (name, fld, "+0.0 where the three denominators are 0")
    assert denormal > 0 and zero_den > 0


# ---- counts as values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minind", si.POPS_MININDS + ("realistic",))
@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("est", ["wc", "hudson"])
def test_extreme_and_realistic_counts_as_values(ctx, est, k, minind):
    """PBS reads the counts as VALUES through pgt_fst_site.h: the signed compare at INT32_MIN / -1 / INT32_MAX, (double)nind at
    INT32_MAX, the reciprocal of a divisor up to 2^96 (Weir-Cockerham) and 2 nind - 1 (Hudson).  Rows and genome-wide lines
    against the float64 per-site model summed directly; one-site windows at counted sites against the header's definition in exact
    rationals for each of the trio's pairs (Hudson also bit for bit against the float64 model).  The third population of a pair
    decides membership only: with population r's count replaced by INT32_MAX where it passes and INT32_MIN where it fails, the
    sums of the pair without r keep their bits in every trio that holds r, and every other trio keeps all of its bits."""
    realistic = minind == "realistic"
    minind = si.REALISTIC_MININD if realistic else minind
    n = si.POPS_N
    _, pos = si.two_chromosomes(n)
    tp = _t(pos)
    f, c = si.count_case_columns("pbs", k, minind, realistic)
    trios = all_trio_order(k)
    for ijk in trios:
        assert 0 < int(si.pops_counted(ijk, c, minind).sum()) < n, ijk
    what = f"pbs {est} K={k} minind={minind}"
    for name, win in si.pops_tables(with_one_site=False):
        got, tot = call(ctx, est, tp, f, c, minind, win)
        assert_against_the_definition(est, got, tot, f, c, minind, win, pos, f"{what} table {name}")
        assert np.all(tot["neff"] > 0) and np.all(tot["nskip"] > 0)
        for r in (0, 1, k - 1):
            flat = list(c)
            flat[r] = np.where(c[r] >= np.int32(minind), np.int32(si.I32_MAX), np.int32(si.I32_MIN)).astype(np.int32)
            same, same_t = call(ctx, est, tp, f, flat, minind, win)
            for t, ijk in enumerate(trios):
                if r not in ijk:
                    rows_equal(same[t], got[t], f"{what} table {name}: trio {ijk} without population {r}")
                    assert same_t[t].tobytes() == tot[t].tobytes()
                    continue
                kept = [s for s in SUMS if s not in sums_that_read(r, ijk)]
                assert len(kept) == 2
                for fld in kept + ["start", "end", "mid", "n"]:
                    assert same[t][fld].tobytes() == got[t][fld].tobytes(), (what, name, ijk, r, fld)
                for fld in kept + ["neff", "nskip"]:
                    assert same_t[t][fld].tobytes() == tot[t][fld].tobytes(), (what, name, ijk, r, fld)
    win = si.counted_site_table("pbs", k, c, minind, m=300 if k == 3 else 100)  # K = 6: 20 trios of three pairs each
    at = win["lo"].astype(np.int64)
    got, tot = call(ctx, est, tp, f, c, minind, win)
    assert_against_the_definition(est, got, tot, f, c, minind, win, pos, f"{what} one-site windows")
    pair_stat = si.PBS_PAIR_STAT[STAT[est]]
    for t, ijk in enumerate(trios):
        ok = si.pops_counted(ijk, c, minind)[at]
        assert ok.any()
        for w in np.flatnonzero(ok).tolist():
            for pname, (a, b) in zip(PAIRS, pairs_of(*ijk)):
                exact = si.exact_site(pair_stat, [f[a][at[w]], f[b][at[w]]], [c[a][at[w]], c[b][at[w]]])
                si.assert_within_exact([got[t][f"num_{pname}"][w], got[t][f"den_{pname}"][w]], exact, f"{what} trio {ijk} pair {(a, b)} site {at[w]}")
