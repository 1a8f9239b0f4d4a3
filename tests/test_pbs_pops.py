"""GPU: the population branch statistic of all trios of 3 ... 6 populations, every population of a trio as the focal one, from
per-population (freq, nInd) columns (pgt_pbs_pops_reduce_dev / pgt_pbs_hudson_pops_reduce_dev and their host-buffer forms).

The yardsticks are the float64 NumPy model of the definition (tests/pbs_pops_model.py), the pair sums of
pgt_fst_pops_reduce_dev / pgt_fst_hudson_pops_reduce_dev on the same columns and the definition's own properties — never the
code under test.  Tolerance: counts, coordinates and mid exact; each of the six sums within |x - y| <= 1e-9 A + 1e-12, A the
window's sum of the absolute values of the terms a site's value is built from (any summation order of n <= 9e6 doubles stays
within n 2^-53 A < 1e-9 A).  The finishing arithmetic is held to the model's finishing lines applied to the row's OWN sums: the
arguments of the logarithm are then the same bits, the two logarithms are each within 1 ulp, and three branches are added:
|x - y| <= 1e-13 (|T_ij| + |T_ik| + |T_jk|) + 1e-18, about 200 times that; infinities and NaN must agree in class and sign."""
import ctypes as C

import numpy as np
import pytest

import pbs_pops_model
import synth
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from pbs_pops_model import PAIRS, PBS, SUMS, all_trio_order, pairs_of
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import FST_ROW_DTYPE, PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, WIN_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, run_lengths, windows_to_device
from test_fst_pops import MININD, SIZES, _dev, _t, random_pops, tables_for

pytestmark = pytest.mark.gpu
REL_A, ABS = 1e-9, 1e-12
ESTIMATORS = ("wc", "hudson")


def n_trios(k):
    return len(all_trio_order(k))


def pops_dev(ctx, tp, tf, tn, minind, win, est, **kw):
    """-> (rows[n_trios, n_win], totals[n_trios] or None) of one pbs_pops_reduce_dev call"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.pbs_pops_reduce_dev(tp, tf, tn, minind, wd, estimator=est, **kw)
    T = n_trios(len(tf))
    rows = rows_from_device(out, PBS_ROW_DTYPE)[: T * win.size].reshape(T, win.size)
    return rows, (rows_from_device(tot, PBS_TOTAL_DTYPE)[:T] if tot is not None else None)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def excess(x, y, A, slack=1.0):
    """max of |x - y| - slack (1e-9 A + 1e-12): <= 0 when every entry is within the bound"""
    x, y, A = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, y, A))
    return -1.0 if x.size == 0 else float(np.max(np.abs(x - y) - slack * (REL_A * A + ABS)))


def assert_finish(got, what):
    """pbs_i, pbs_j, pbs_k of `got` (rows or totals) against the model's finishing lines on got's own six sums"""
    got = np.atleast_1d(got)
    want, T = pbs_pops_model.finish_rows(got)
    mag = sum(np.where(np.isfinite(t), np.abs(t), 0.0) for t in T)
    for fld, w in zip(PBS, want):
        g = got[fld]
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, fld, "NaN where the model has none, or the reverse")
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(np.sign(g[np.isinf(w)]), np.sign(w[np.isinf(w)])), (what, fld, "infinities")
        assert np.all(np.abs(g[fin] - w[fin]) <= 1e-13 * mag[fin] + 1e-18), (what, fld, float(np.max(np.abs(g[fin] - w[fin]) - 1e-13 * mag[fin])))
    empty = got["n" if "n" in got.dtype.names else "neff"] == 0
    for fld in PBS + SUMS:
        assert np.all(bits(got[fld][empty]) == 0), (what, fld, "+0.0 without a counted site")


def assert_rows(got, want, A, t, what, quiet=True):
    assert got.size == want.size, what
    for fld in ("start", "end", "mid", "n"):
        assert np.array_equal(got[fld], want[fld]), (what, fld)
    for fld in SUMS:
        e = excess(got[fld], want[fld], A[fld][t])
        if not quiet:
            print(f"{what} {fld}: excess over the bound {e:.3e}")
        assert e <= 0.0, (what, fld, e)
    assert_finish(got, what)


def assert_totals(got, want, A_tot, what):
    for fld in ("neff", "nskip"):
        assert np.array_equal(got[fld], want[fld]), (what, fld)
    for fld in SUMS:
        assert excess(got[fld], want[fld], A_tot[fld]) <= 0.0, (what, fld, got[fld], want[fld])
    assert_finish(got, what)


def one_site_table(n):
    win = np.zeros(n, dtype=WIN_DTYPE)
    win["lo"] = np.arange(n)
    win["hi"] = win["lo"] + 1
    return win


# ---- rows and genome-wide lines against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("k", [3, 4, 6])
def test_rows_and_totals_against_the_numpy_model(pgt, ctx, k, est):
    for si, n in enumerate(SIZES):
        rng = np.random.default_rng(5300 * k + si)
        chr_ids, pos = synth.chromosomes(rng, n, min(1 + (si + k) % 3, n), equal=False)
        f, c = random_pops(rng, n, k)
        tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
        for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est)
            want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est)
            for t, ijk in enumerate(all_trio_order(k)):
                assert_rows(rows[t], want[t], A, t, f"{est} K={k} n={n} {name} trio {ijk}", quiet=n < 8193 or t > 0)
            assert_totals(tot, want_t, A_tot, f"{est} K={k} n={n} {name} totals")


@pytest.mark.parametrize("est", ESTIMATORS)
def test_level3_nodes_are_built_and_used(pgt, ctx, est):
    n, W, k = 600_001, 550_000, 3
    rng = np.random.default_rng(5333)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, 10_000)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.any(-(-lo // (8192 * 64)) < hi // (8192 * 64)), "a window must contain a level-3 node"
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est)
    for hint in (0, W, 50_000):  # 50 000: too small a hint for these windows, answered from level 2
        with ctx.hints(hint, 0, 0):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est)
        assert_rows(rows[0], want[0], A, 0, f"{est} level 3, hint {hint}", quiet=False)
        assert_totals(tot, want_t, A_tot, f"{est} level 3, hint {hint}")


# ---- one-site windows: the definition's bits, +inf, NaN and +0.0 ------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
@pytest.mark.parametrize("k", [3, 6])
def test_one_site_windows(pgt, ctx, k, est):
    """Hudson: all six sums carry the definition's bits (every operation of its per-site lines is a float64 operation of its
    own); wc: within the bound (the kernel's one reciprocal per pair is not the model's divisions).  Sites with p = 0 against
    p = 1 pin T = +inf and the NaN of inf - inf; a window without a counted site is +0.0 in every double."""
    n = 8193
    rng = np.random.default_rng(5450 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    for x in f:  # exact 0 and 1, and ties between neighbours, among the sites
        x[rng.integers(0, n, 200)] = 0.0
        x[rng.integers(0, n, 200)] = 1.0
    for a in range(k - 1):
        at = rng.integers(0, n, 300)
        f[a + 1][at] = f[a][at]
    fixed = np.arange(100, 160)  # populations 0 / 1 / 2 hold 0 / 1 / 1 (two fixed pairs), then 0 / 1 / 0.5 (one), all counted
    f[0][fixed], f[1][fixed] = 0.0, 1.0
    f[2][fixed[:30]], f[2][fixed[30:]] = 1.0, 0.5
    for x in c[:3]:
        x[fixed] = 20
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    win = one_site_table(n)
    for minind in (1, 5):
        rows, tot = pops_dev(ctx, tp, tf, tn, minind, win, est)
        want, _, A, _ = pbs_pops_model.model(pos, f, c, minind, win, est)
        for t, (i, j, kk) in enumerate(all_trio_order(k)):
            what = f"{est} K={k} minind={minind} trio {(i, j, kk)}"
            ok = pbs_pops_model.counted(c, i, j, kk, minind)
            assert np.array_equal(rows[t]["n"], ok.astype(np.uint32)), what
            assert np.array_equal(rows[t]["start"], pos) and np.array_equal(rows[t]["end"], pos) and np.array_equal(rows[t]["mid"], pos), what
            for name, (a, b) in zip(PAIRS, pairs_of(i, j, kk)):
                num, den = pbs_pops_model.site_values(est, f[a], f[b], c[a], c[b])
                for fld, x in ((f"num_{name}", num), (f"den_{name}", den)):
                    x = np.where(ok, x, 0.0) + 0.0
                    if est == "hudson":
                        assert np.array_equal(bits(rows[t][fld]), bits(x)), (what, fld)
                    else:
                        assert excess(rows[t][fld], x, A[fld][t]) <= 0.0, (what, fld)
            assert_finish(rows[t], what)
            for fld in PBS + SUMS:  # no counted site: +0.0 by its bits
                assert np.all(bits(rows[t][fld][~ok]) == 0), (what, fld)
            assert np.any(~ok)
            assert int(tot[t]["neff"]) == int(ok.sum()) and int(tot[t]["nskip"]) == n - int(ok.sum())
        r = rows[0]  # trio (0, 1, 2)
        two, one = fixed[:30], fixed[30:]
        assert np.all(np.isposinf(r["pbs_i"][two])) and np.all(np.isnan(r["pbs_j"][two])) and np.all(np.isnan(r["pbs_k"][two])), est
        assert np.all(r["num_ij"][fixed] == 1.0) and np.all(r["den_ij"][fixed] == 1.0), est
        assert np.all(np.isposinf(r["pbs_i"][one])) and np.all(np.isposinf(r["pbs_j"][one])) and np.all(np.isneginf(r["pbs_k"][one])), est


# ---- the trio's site set against the pair's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
def test_the_pair_sums_of_the_fst_call_where_the_third_population_is_counted_everywhere(pgt, ctx, est):
    """K = 3 with the third population's nInd >= minind everywhere: trio (0,1,2) counts exactly the sites pair (0,1) counts, and
    n, num_ij, den_ij are n, asum, bsum of pair (0,1) of the all-pairs FST call of the same estimator, within the bound of both
    rows.  With the third population short of data on every seventh site the trio counts fewer sites than the pair."""
    n, k = 2 * 8192 + 700, 3
    rng = np.random.default_rng(5550)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    c[2] = np.maximum(c[2], MININD).astype(np.int32)
    fst_dev = ctx.fst_pops_reduce_dev if est == "wc" else ctx.fst_hudson_pops_reduce_dev
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    short = c[2].copy()
    short[::7] = 0
    for name, win in [("one site", one_site_table(n))] + tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est)
        out, _, _ = fst_dev(tp, tf, tn, MININD, windows_to_device(win, _dev()), tot=False)
        pair = rows_from_device(out, FST_ROW_DTYPE)[: 3 * win.size].reshape(3, win.size)[0]  # pair (0, 1)
        _, _, A, _ = pbs_pops_model.model(pos, f, c, MININD, win, est)
        assert np.array_equal(rows[0]["n"], pair["n"]) and np.any(pair["n"] > 0), name
        for mine, theirs in (("num_ij", "asum"), ("den_ij", "bsum")):
            e = excess(rows[0][mine], pair[theirs], A[mine][0], slack=2.0)
            print(f"{est} {name}: {mine} against the pair's {theirs}, excess over the bound {e:.3e}")
            assert e <= 0.0, (name, mine, e)
        fewer, _ = pops_dev(ctx, tp, tf, [tn[0], tn[1], _t(short)], MININD, win, est)
        assert np.all(fewer[0]["n"] <= pair["n"]) and int(fewer[0]["n"].sum()) < int(pair["n"].sum()), name
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        lost = np.concatenate(([0], np.cumsum((np.arange(n) % 7 == 0) & (c[0] >= MININD) & (c[1] >= MININD))))
        assert np.array_equal(pair["n"].astype(np.int64) - fewer[0]["n"], lost[hi] - lost[lo]), name


# ---- trio isolation and reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
def test_trios_do_not_see_the_other_populations_and_calls_repeat(pgt, ctx, est):
    n, k = 2 * 8192 + 700, 6
    rng = np.random.default_rng(5650)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    f2, c2 = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), W, S) for W, S in ((7, 3), (5000, 1000))])
    tp = _t(pos)
    rows, tot = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win, est)
    again, again_t = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win, est)
    assert again.tobytes() == rows.tobytes() and again_t.tobytes() == tot.tobytes()  # two calls give the same bits
    for t, sel in enumerate(all_trio_order(k)):  # (0,1,2), (0,2,4), (3,4,5): the K = 3 call on those columns
        if sel in ((0, 1, 2), (0, 2, 4), (3, 4, 5)):
            three, three_t = pops_dev(ctx, tp, [_t(f[x]) for x in sel], [_t(c[x]) for x in sel], MININD, win, est)
            rows_equal(np.ascontiguousarray(rows[t]), three[0], f"{est} trio {sel} of the K = 6 call against the K = 3 call")
            assert three_t[0].tobytes() == tot[t].tobytes()
    for r in (0, 3, 5):  # population r replaced: every trio without it keeps its bits
        fr, cr = list(f), list(c)
        fr[r], cr[r] = f2[r], c2[r]
        got, got_t = pops_dev(ctx, tp, [_t(x) for x in fr], [_t(x) for x in cr], MININD, win, est)
        kept = 0
        for t, ijk in enumerate(all_trio_order(k)):
            if r not in ijk:
                rows_equal(np.ascontiguousarray(got[t]), np.ascontiguousarray(rows[t]), f"{est} population {r} replaced, trio {ijk}")
                assert got_t[t].tobytes() == tot[t].tobytes()
                kept += 1
            else:
                assert got[t].tobytes() != rows[t].tobytes()
        assert kept == n_trios(k - 1)


@pytest.mark.parametrize("est", ESTIMATORS)
def test_uncounted_sites_may_hold_anything_and_a_counted_nan_stays_in_its_sums(pgt, ctx, est):
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(5750)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    win = np.concatenate([one_site_table(n)[:3000]] + [w for _, w in tables_for(pgt, pos, run_lengths(chr_ids))])
    tp = _t(pos)
    tame, tame_t = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win, est)
    wild_f, wild_c = [x.copy() for x in f], [x.copy() for x in c]
    junk_f = np.array([np.nan, np.inf, -np.inf, 2.0])
    junk_c = np.array([0, -1, np.iinfo(np.int32).min], dtype=np.int32)
    for p in range(k):
        low = np.flatnonzero(c[p] < MININD)
        assert low.size > 1000
        wild_f[p][low] = junk_f[rng.integers(0, junk_f.size, low.size)]
        wild_c[p][low] = junk_c[rng.integers(0, junk_c.size, low.size)]
    wild, wild_t = pops_dev(ctx, tp, [_t(x) for x in wild_f], [_t(x) for x in wild_c], MININD, win, est)
    for t in range(n_trios(k)):
        rows_equal(np.ascontiguousarray(wild[t]), np.ascontiguousarray(tame[t]), f"{est} trio {t}: wild values at uncounted sites")
        assert all(np.all(np.isfinite(wild[t][s])) for s in SUMS)
    assert wild_t.tobytes() == tame_t.tobytes()
    # a NaN frequency of population 1 at ONE site that every population counts: NaN in exactly the sums of the pairs that hold
    # population 1, of the trios that hold it, in the windows that hold the site; every other sum keeps its bits
    site = int(np.flatnonzero(np.all([x >= MININD for x in c], axis=0) & (np.arange(n) > 1000))[0])
    nan_f = [x.copy() for x in f]
    nan_f[1][site] = np.nan
    got, got_t = pops_dev(ctx, tp, [_t(x) for x in nan_f], [_t(x) for x in c], MININD, win, est)
    holds = (win["lo"] <= site) & (site < win["hi"])
    assert holds.sum() > 3 and not holds.all()
    for t, ijk in enumerate(all_trio_order(k)):
        for name, pair in zip(PAIRS, pairs_of(*ijk)):
            for fld in (f"num_{name}", f"den_{name}"):
                if 1 in pair:
                    assert np.all(np.isnan(got[t][fld][holds])) and np.isnan(got_t[t][fld]), (est, ijk, fld)
                    assert np.array_equal(bits(got[t][fld][~holds]), bits(tame[t][fld][~holds])), (est, ijk, fld)
                else:
                    assert np.array_equal(bits(got[t][fld]), bits(tame[t][fld])) and bits(got_t[t][fld]) == bits(tame_t[t][fld]), (est, ijk, fld)
        assert np.array_equal(got[t]["n"], tame[t]["n"])
        assert_finish(got[t], f"{est} NaN at a counted site, trio {ijk}")


# ---- workspace contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,est", [(513, 3, "wc"), (8193, 6, "hudson"), (8193, 5, "wc"), (600_001, 4, "hudson")])
def test_rows_under_every_hint_poison_and_guard(pgt, ctx, n, k, est):
    W = 550_000 if n > 100_000 else 5000
    rng = np.random.default_rng(5850 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    fb, cb = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), min(W, n), max(1, min(W, n) // 4)),
                          pgt.build_windows_sites(run_lengths(chr_ids), min(1000, n), min(333, n))])
    want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est)
    dev = _dev()
    tf, tn = [padded_column(x, float("nan"), dev) for x in f], [padded_column(x, 1000, dev) for x in c]
    tp, wd = _t(pos), windows_to_device(win, dev)
    T = n_trios(k)
    wb = ctx.pbs_pops_work_bytes(k, n, win.size)
    _, _, foreign = ctx.pbs_pops_reduce_dev(tp, [_t(x) for x in fb], [_t(x) for x in cb], MININD, wd, estimator=est)
    assert foreign.numel() == wb
    g = GuardedBuffers([wb, T * win.size * PBS_ROW_DTYPE.itemsize, T * PBS_TOTAL_DTYPE.itemsize], 47 + k, dev)
    work, out, tot = g.bufs
    for hint in (0, W, 50_000):  # 50 000: at 600 001 sites too small a hint, the level-3 windows answered from level 2
        first = None
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):  # the tree, the scratch rows and the scratch totals all lie in `work`
                poison_tree(work, kind, other=foreign)
                out.fill_(0xFF)
                tot.fill_(0xFF)
                ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd, estimator=est, out=out, tot=tot, work=work)
                what = f"{est} n={n} K={k} hint={hint} poison={kind}"
                g.check(what)
                got = rows_from_device(out, PBS_ROW_DTYPE).reshape(T, win.size).copy()
                got_t = rows_from_device(tot, PBS_TOTAL_DTYPE).copy()
                if first is None:
                    first = (got, got_t)
                    for t in range(T):
                        assert_rows(got[t], want[t], A, t, what + f" trio {t}")
                    assert_totals(got_t, want_t, A_tot, what)
                else:  # identical under one hint, whatever the workspace held
                    assert got.tobytes() == first[0].tobytes() and got_t.tobytes() == first[1].tobytes(), what
    # tot=None (no genome-wide lines: the totals buffer stays as it was), the global-only form (n_win = 0: no row is written) and
    # the tree-only call (n_win = 0 without tot: both passes build, nothing is finished, PGT_OK as for every other statistic),
    # under the last hint of the loop above, whose rows `first` holds; the workspace starts from 0xFF every time
    with ctx.hints(hint, 0, 0):
        for buf in (work, out, tot):
            buf.fill_(0xFF)
        ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd, estimator=est, out=out, tot=False, work=work)
        g.check("tot = NULL")
        assert rows_from_device(out, PBS_ROW_DTYPE).reshape(T, win.size).tobytes() == first[0].tobytes()
        assert bool((tot == 0xFF).all()), "tot = NULL: the totals buffer is not written"
        for buf in (work, out, tot):
            buf.fill_(0xFF)
        ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd[:0], estimator=est, out=out, tot=tot, work=work)
        g.check("n_win = 0")
        assert bool((out == 0xFF).all()), "n_win = 0: no row is written"
        assert rows_from_device(tot, PBS_TOTAL_DTYPE).tobytes() == first[1].tobytes()
        for buf in (work, out, tot):
            buf.fill_(0xFF)
        ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd[:0], estimator=est, out=out, tot=False, work=work)  # raises unless PGT_OK
        g.check("n_win = 0 and tot = NULL")
        assert bool((out == 0xFF).all()) and bool((tot == 0xFF).all()), "the tree-only call writes no row and no total"


def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    import torch
    n, k, est = 2 * 8192 + 700, 4, "wc"
    rng = np.random.default_rng(5950)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    A_, B_ = random_pops(rng, n, k), random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 100)
    dev = _dev()
    wd, tp = windows_to_device(win, dev), _t(pos)
    tf, tn = [_t(x) for x in A_[0]], [_t(x) for x in A_[1]]
    T = n_trios(k)
    g = GuardedBuffers([ctx.pbs_pops_work_bytes(k, n, win.size), T * win.size * PBS_ROW_DTYPE.itemsize, T * PBS_TOTAL_DTYPE.itemsize], 3, dev)
    work, out, tot = g.bufs
    with ctx.hints(5000, 100, 0):
        ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd, estimator=est, out=out, tot=tot, work=work)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # one call on one stream: a chain of kernels, no parallel branches
            ctx.pbs_pops_reduce_dev(tp, tf, tn, MININD, wd, estimator=est, out=out, tot=tot, work=work)
    for name, src in (("B", B_), ("A", A_)):
        for t, x in zip(tf + tn, src[0] + src[1]):
            t.copy_(torch.from_numpy(x))
        for buf in (work, out, tot):
            buf.fill_(0xFF)
        graph.replay()
        g.check("pbs_pops graph replay")
        want, want_t, A, A_tot = pbs_pops_model.model(pos, src[0], src[1], MININD, win, est)
        got = rows_from_device(out, PBS_ROW_DTYPE).reshape(T, win.size)
        for t in range(T):
            assert_rows(got[t], want[t], A, t, f"replay {name} trio {t}")
        assert_totals(rows_from_device(tot, PBS_TOTAL_DTYPE), want_t, A_tot, f"replay {name}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
def test_refusals_name_the_argument_and_write_nothing(pgt, ctx, est):
    import torch
    n, k = 10_000, 3
    rng = np.random.default_rng(6050)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 1000, 500)
    wd = windows_to_device(win, _dev())
    T = 1
    wb = ctx.pbs_pops_work_bytes(k, n, win.size)
    g = GuardedBuffers([wb, T * win.size * PBS_ROW_DTYPE.itemsize, T * PBS_TOTAL_DTYPE.itemsize], 5, _dev())
    work, out, tot = g.bufs
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    lib, h = ctx._lib, ctx._ctx
    dev_fn = lib.pgt_pbs_pops_reduce_dev if est == "wc" else lib.pgt_pbs_hudson_pops_reduce_dev
    host_fn = lib.pgt_pbs_pops_reduce if est == "wc" else lib.pgt_pbs_hudson_pops_reduce
    before = [b.clone() for b in g.bufs]

    def call(freq=None, nind=None, n_pops=k, minind=MININD, win_p=wd.data_ptr(), out_p=out.data_ptr(), out_bytes=out.numel(),
             work_p=work.data_ptr(), work_bytes=work.numel(), freq_null=False, nind_null=False, pos_p=tp.data_ptr()):
        fp = [t.data_ptr() for t in tf] if freq is None else freq
        npn = [t.data_ptr() for t in tn] if nind is None else nind
        pf = (C.c_void_p * 8)(*(fp + [None] * (8 - len(fp))))
        pn = (C.c_void_p * 8)(*(npn + [None] * (8 - len(npn))))
        return dev_fn(h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, n, minind, win_p, win.size,
                      out_p, out_bytes, tot.data_ptr(), work_p, work_bytes, None)

    fp, npp = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    refusals = [
        (dict(minind=0), "minind must be at least 1"), (dict(minind=-3), "minind"),
        (dict(pos_p=None), "pos"), (dict(freq_null=True), "freq"), (dict(nind_null=True), "nind"), (dict(work_p=None), "work is NULL"), (dict(win_p=None), "win"),
        (dict(out_p=None), "out"), (dict(n_pops=2), "n_pops must be 3 ... 6"), (dict(n_pops=7), "n_pops must be 3 ... 6"), (dict(n_pops=0), "n_pops"),
        (dict(freq=[fp[0], None, fp[2]]), "freq[1]"), (dict(nind=[npp[0], npp[1], None]), "nind[2]"),
        (dict(freq=[fp[0], fp[1] + 8, fp[2]]), "freq[1] is not 16-byte aligned"), (dict(nind=[npp[0], npp[1], npp[2] + 8]), "nind[2]"),
        (dict(nind=[npp[0] + 4, npp[1], npp[2]]), "nind[0]"), (dict(work_p=work.data_ptr() + 8, work_bytes=wb), "work is not 16-byte aligned"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(work_bytes=wb - 1), "work_bytes too small"),
        (dict(work_bytes=ctx.f3_pops_tree_bytes(k, n)), "work_bytes too small"),  # the tree alone is not enough: the scratch rows lie behind it
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_pbs_pops_reduce: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    want, _, A, _ = pbs_pops_model.model(pos, f, c, MININD, win, est)
    assert_rows(rows_from_device(out, PBS_ROW_DTYPE).reshape(T, win.size)[0], want[0], A, 0, "accepted call", quiet=False)

    # the host-buffer form refuses in the same words and returns before any upload
    rows_h, tot_h = np.zeros(win.size, dtype=PBS_ROW_DTYPE), np.zeros(1, dtype=PBS_TOTAL_DTYPE)
    hf = (C.c_void_p * 8)(*([x.ctypes.data for x in f] + [None] * 5))
    hn = (C.c_void_p * 8)(*([x.ctypes.data for x in c] + [None] * 5))
    for n_pops, minind, name in ((2, MININD, "n_pops must be 3 ... 6"), (7, MININD, "n_pops must be 3 ... 6"), (3, 0, "minind must be at least 1")):
        rc = host_fn(h, pos.ctypes.data, hf, hn, n_pops, n, minind, win.ctypes.data, win.size, rows_h.ctypes.data, tot_h.ctypes.data)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_pbs_pops_reduce: "), (n_pops, minind, msg)
    assert not rows_h.view(np.uint8).any() and not tot_h.view(np.uint8).any()

    # the Python wrappers refuse by name
    who = "pbs_pops_reduce" if est == "wc" else "pbs_hudson_pops_reduce"
    with pytest.raises(_lib.PgtError, match=f"{who}_dev: 3 ... 6 populations"):
        ctx.pbs_pops_reduce_dev(tp, tf[:2], tn[:2], 1, wd, estimator=est)
    with pytest.raises(_lib.PgtError, match="3 ... 6 populations"):
        ctx.pbs_pops_reduce(pos, f * 3, c * 3, MININD, win, estimator=est)
    with pytest.raises(_lib.PgtError, match="minind"):
        ctx.pbs_pops_reduce_dev(tp, tf, tn, 0, wd, estimator=est)
    with pytest.raises(_lib.PgtError, match='pbs_pops_reduce_dev: estimator must be "wc" or "hudson"'):
        ctx.pbs_pops_reduce_dev(tp, tf, tn, 1, wd, estimator="reynolds")
    with pytest.raises(_lib.PgtError, match=f"{who}_dev: work"):
        ctx.pbs_pops_reduce_dev(tp, tf, tn, 1, wd, estimator=est, work=torch.empty(wb - 1, dtype=torch.uint8, device=_dev()))
    torch.cuda.synchronize()


# ---- host-buffer form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ESTIMATORS)
def test_host_buffer_form_equals_the_device_form_twice_in_a_row(pgt, ctx, est):
    n, k = 2 * 8192 + 700, 4
    for seed in (93, 94):  # different data through the one context: nothing of the cached workspace may survive
        rng = np.random.default_rng(seed)
        chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
        f, c = random_pops(rng, n, k)
        win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 1000)
        rows, tot = ctx.pbs_pops_reduce(pos, f, c, MININD, win, estimator=est)
        hints = pgt.window_scan.table_hints(win)
        with ctx.hints(hints[0], 0, 0):  # the host-buffer form derives the longest-window hint from the table
            want, want_t = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], MININD, win, est)
        assert rows.shape == want.shape == (4, win.size)
        for t in range(rows.shape[0]):
            rows_equal(np.ascontiguousarray(rows[t]), np.ascontiguousarray(want[t]), f"{est} seed {seed} trio {t}")
        assert tot.tobytes() == want_t.tobytes()
    res = pgt.pbs_window_pops(chr_ids, pos, f, c, 5000, 1000, MININD, 1, estimator=est, ctx=ctx)
    assert list(res) == pgt.all_trio_order(k) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    for t, ijk in enumerate(pgt.all_trio_order(k)):
        rows_equal(np.ascontiguousarray(res[ijk].rows), np.ascontiguousarray(want[t]), f"{est} pbs_window_pops trio {ijk}")
        assert res[ijk].total.tobytes() == want_t[t].tobytes()
    # -skip_missing drops a trio's rows without counted sites from that trio alone
    c0 = [x.copy() for x in c]
    c0[1][:6000] = 0
    full = pgt.pbs_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, estimator=est, ctx=ctx)
    kept = pgt.pbs_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, skip_missing=1, estimator=est, ctx=ctx)
    assert np.any(full[(0, 1, 2)].rows["n"] == 0)
    assert kept[(0, 1, 2)].rows.size == np.count_nonzero(full[(0, 1, 2)].rows["n"]) < full[(0, 1, 2)].rows.size
    assert kept[(0, 2, 3)].rows.size == np.count_nonzero(full[(0, 2, 3)].rows["n"]) > kept[(0, 1, 2)].rows.size
