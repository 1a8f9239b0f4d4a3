"""GPU: f_d (Martin et al. 2015) and f_dM (Malinsky et al. 2015) of all ingroup trios against an outgroup from per-population
(freq, nInd) columns (pgt_fd_pops_reduce_dev / pgt_fd_pops_reduce).

The yardsticks are the float64 NumPy model of the definition (tests/fd_pops_model.py), the exact-rational fixture
(tests/golden/fd_exact.json), the D rows of the same columns and the definition's own properties — never the code under test.
Tolerance: counts, coordinates and mid exact; num, fd_den, fdm_den within |x - y| <= 1e-9 A + 1e-12, A the window's Σ|site
term| (num's site terms have both signs — a 7-site window cancels to 9e-4 of Σ|term| — so a bound relative to |y| would be
wrong; any summation order of n <= 9e6 doubles stays within n 2^-53 A < 1e-9 A); fd and fdm bit for bit the stated function
of the row's own sums; one-site windows bit for bit."""
import ctypes as C

import numpy as np
import pytest

import dstat_pops_model
import fd_pops_model
import helpers
import pops_grid_shapes as shapes
import synth
from fd_pops_model import SUMS
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import DSTAT_ROW_DTYPE, FD_ROW_DTYPE, FD_TOTAL_DTYPE, WIN_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, run_lengths, trio_order, windows_to_device
from test_fst_pops import MININD, SIZES, _dev, _t, random_pops, tables_for

pytestmark = pytest.mark.gpu
REL_A, ABS = 1e-9, 1e-12


def n_trios(k):
    return len(trio_order(k))


def uniform_pops(rng, n, k):
    """input set 2: ALL frequencies uniform in [0, 1] rounded to 6 decimals (the outgroup polymorphic too), nInd uniform in 0 .. 20"""
    return [np.round(rng.uniform(0, 1, n), 6) for _ in range(k)], [rng.integers(0, 21, n, dtype=np.int32) for _ in range(k)]


INPUTS = {"project": random_pops, "uniform": uniform_pops}


def pops_dev(ctx, tp, tf, tn, minind, win, **kw):
    """-> (rows[n_trios, n_win], totals[n_trios] or None) of one fd_pops_reduce_dev call"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.fd_pops_reduce_dev(tp, tf, tn, minind, wd, **kw)
    T = n_trios(len(tf))
    rows = rows_from_device(out, FD_ROW_DTYPE)[: T * win.size].reshape(T, win.size)
    return rows, (rows_from_device(tot, FD_TOTAL_DTYPE)[:T] if tot is not None else None)


def dstat_dev(ctx, tp, tf, tn, minind, win):
    out, _, _ = ctx.dstat_pops_reduce_dev(tp, tf, tn, minind, windows_to_device(win, _dev()), tot=False)
    T = n_trios(len(tf))
    return rows_from_device(out, DSTAT_ROW_DTYPE)[: T * win.size].reshape(T, win.size)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def excess(x, y, A):
    """max of |x - y| - (1e-9 A + 1e-12): <= 0 when every entry is within the bound"""
    x, y, A = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, y, A))
    return -1.0 if x.size == 0 else float(np.max(np.abs(x - y) - (REL_A * A + ABS)))


def assert_ratios_are_their_definition(rows, what):
    """fd and fdm, bit for bit, are the stated function of the row's own sums"""
    assert np.array_equal(bits(rows["fd"]), bits(fd_pops_model.ratio(rows["num"], rows["fd_den"]))), (what, "fd")
    assert np.array_equal(bits(rows["fdm"]), bits(fd_pops_model.ratio(rows["num"], rows["fdm_den"]))), (what, "fdm")


def assert_rows(got, want, A, t, what, quiet=False):
    assert got.size == want.size, what
    for fld in ("start", "end", "mid", "n"):
        assert np.array_equal(got[fld], want[fld]), (what, fld)
    for fld in SUMS:
        e = excess(got[fld], want[fld], A[fld][t])
        if not quiet:
            print(f"{what} {fld}: excess over the bound {e:.3e}")
        assert e <= 0.0, (what, fld, e)
    assert_ratios_are_their_definition(got, what)


def assert_totals(got, want, A_tot, what):
    for fld in ("neff", "nskip"):
        assert np.array_equal(got[fld], want[fld]), (what, fld)
    for fld in SUMS:
        assert excess(got[fld], want[fld], A_tot[fld]) <= 0.0, (what, fld, got[fld], want[fld])


def one_site_table(n):
    win = np.zeros(n, dtype=WIN_DTYPE)
    win["lo"] = np.arange(n)
    win["hi"] = win["lo"] + 1
    return win


# ---- 1, 3b, 4: rows and genome-wide lines against the model; coordinates and counts are the D rows'; num against abba - baba ----
@pytest.mark.parametrize("inputs", ["project", "uniform"])
@pytest.mark.parametrize("k", [4, 5, 7])
def test_rows_and_totals_against_the_numpy_model_and_the_d_rows(pgt, ctx, k, inputs):
    for si, n in enumerate(SIZES):
        rng = np.random.default_rng(1300 * k + si + (50 if inputs == "uniform" else 0))
        chr_ids, pos = synth.chromosomes(rng, n, min(1 + (si + k) % 3, n), equal=False)
        f, c = INPUTS[inputs](rng, n, k)
        tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
        for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
            want, want_t, A, A_tot = fd_pops_model.model(pos, f, c, MININD, win)
            d = dstat_dev(ctx, tp, tf, tn, MININD, win)
            for t, ijk in enumerate(trio_order(k)):
                what = f"K={k} {inputs} n={n} {name} trio {ijk}"
                assert_rows(rows[t], want[t], A, t, what, quiet=True)
                for fld in ("start", "end", "mid", "n"):  # those of pgt_dstat_pops_reduce_dev on the same call arguments
                    assert np.array_equal(rows[t][fld], d[t][fld]), (what, fld, "against the D rows")
                gap = np.abs(rows[t]["num"] - (d[t]["abba"] - d[t]["baba"]))
                assert np.all(gap <= 1e-9 * (d[t]["abba"] + d[t]["baba"]) + 1e-12), (what, "num against abba - baba", float(gap.max()))
                assert np.all(rows[t]["fdm_den"] >= 0) and np.all(np.abs(rows[t]["fdm"]) <= 1 + 1e-9), what
            assert_totals(tot, want_t, A_tot, f"K={k} {inputs} n={n} {name} totals")


def test_the_uniform_inputs_reach_both_signs_and_both_branches():
    """input set 2 gives a negative fd_den site term at >= 10 % of the sites and each f_dM branch at >= 40 %"""
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        f, _ = uniform_pops(rng, 8193, 4)
        _, fd_den, _ = fd_pops_model.site_terms(*f)
        neg, ge, le = np.mean(fd_den < 0), np.mean(f[1] >= f[0]), np.mean(f[1] <= f[0])
        print(f"seed {seed}: fd_den < 0 at {100 * neg:.1f} %, p_j >= p_i at {100 * ge:.1f} %, p_j <= p_i at {100 * le:.1f} %")
        assert neg >= 0.10 and ge >= 0.40 and le >= 0.40


def test_level3_nodes_are_built_and_used(pgt, ctx):
    n, W, k = 600_001, 550_000, 4
    rng = np.random.default_rng(33)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = uniform_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, 10_000)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.any(-(-lo // (8192 * 64)) < hi // (8192 * 64)), "a window must contain a level-3 node"
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = fd_pops_model.model(pos, f, c, MININD, win)
    for hint in (0, W, 50_000):  # 50 000: too small a hint for these windows, answered from level 2
        with ctx.hints(hint, 0, 0):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        assert_rows(rows[0], want[0], A, 0, f"level 3, hint {hint}")
        assert_totals(tot, want_t, A_tot, f"level 3, hint {hint}")


# ---- 2: the exact fixture -----------------------------------------------------------------------------------------------------
def test_rows_against_the_exact_rational_fixture(pgt, ctx):
    k = helpers.load_golden("fd_exact.json")
    pos = np.array(k["pos"], dtype=np.uint32)
    f = [np.array(x, dtype=np.float64) for x in k["freq"]]
    c = [np.array(x, dtype=np.int32) for x in k["nind"]]
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    fixed = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    fixed["lo"], fixed["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    whole = k["windows"].index([0, int(pos.size)])
    assert [c["minind"] for c in k["cases"]] == [1, 5]
    for case in k["cases"]:
        rows, tot = pops_dev(ctx, tp, tf, tn, case["minind"], fixed)
        _, _, A, A_tot = fd_pops_model.model(pos, f, c, case["minind"], fixed)  # the bound's A only
        assert [tuple(tr["trio"]) for tr in case["trios"]] == trio_order(5)
        for t, tr in enumerate(case["trios"]):
            what = f"fixture minind={case['minind']} trio {tr['trio']}"
            assert np.array_equal(rows[t]["n"], np.array(tr["n"], dtype=np.uint32)), what
            for fld in SUMS:
                e = excess(rows[t][fld], tr[fld], A[fld][t])
                print(f"{what} {fld}: excess over the bound {e:.3e}")
                assert e <= 0, (what, fld, e)
                assert excess(tot[t][fld], tr[fld][whole], A_tot[fld][t]) <= 0, (what, fld)
            assert_ratios_are_their_definition(rows[t], what)
            assert int(tot[t]["neff"]) == tr["n"][whole] and int(tot[t]["nskip"]) == pos.size - tr["n"][whole]


# ---- 3: one-site windows carry the definition's bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 7])
def test_one_site_windows_carry_the_bits_of_the_definition(pgt, ctx, k):
    n = 8193
    rng = np.random.default_rng(1450 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    for x in f:  # exact 0 and 1, and ties between neighbours, among the sites
        x[rng.integers(0, n, 200)] = 0.0
        x[rng.integers(0, n, 200)] = 1.0
    for a in range(k - 2):
        at = rng.integers(0, n, 300)
        f[a + 1][at] = f[a][at]
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    win = one_site_table(n)
    for minind in (1, 5):
        rows, tot = pops_dev(ctx, tp, tf, tn, minind, win)
        for t, (i, j, kk) in enumerate(trio_order(k)):
            what = f"K={k} minind={minind} trio {(i, j, kk)}"
            ok = fd_pops_model.counted(c, i, j, kk, minind)
            assert np.array_equal(rows[t]["n"], ok.astype(np.uint32)), what
            assert np.array_equal(rows[t]["start"], pos) and np.array_equal(rows[t]["end"], pos) and np.array_equal(rows[t]["mid"], pos), what
            for fld, x in zip(SUMS, fd_pops_model.site_terms(f[i], f[j], f[kk], f[k - 1])):
                assert np.array_equal(bits(rows[t][fld]), bits(np.where(ok, x, 0.0) + 0.0)), (what, fld)
            assert_ratios_are_their_definition(rows[t], what)
            assert int(tot[t]["neff"]) == int(ok.sum()) and int(tot[t]["nskip"]) == n - int(ok.sum())


# ---- 5: properties that need no model ---------------------------------------------------------------------------------------------
def test_swapping_p1_and_p2_negates_num_and_fdm_and_keeps_fdm_den(pgt, ctx):
    n, k = 8193, 4
    rng = np.random.default_rng(1650)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = uniform_pops(rng, n, k)
    win = one_site_table(n)
    tp = _t(pos)
    a, _ = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    order = [1, 0, 2, 3]
    b, _ = pops_dev(ctx, tp, [_t(f[x]) for x in order], [_t(c[x]) for x in order], MININD, win)
    a, b = a[0], b[0]
    assert np.array_equal(a["n"], b["n"]) and np.any(a["n"] > 0)
    nz = a["num"] != 0
    assert np.count_nonzero(nz) > 1000 and np.array_equal(nz, b["num"] != 0)
    assert np.array_equal(bits(a["num"][nz]), bits(-b["num"][nz])) and np.all(bits(a["num"][~nz]) == 0) and np.all(bits(b["num"][~nz]) == 0)
    assert np.array_equal(bits(a["fdm_den"]), bits(b["fdm_den"]))
    assert np.array_equal(bits(a["fdm"][nz]), bits(-b["fdm"][nz])) and np.array_equal(a["fdm"], -b["fdm"])
    assert np.any(a["fdm"] > 0) and np.any(a["fdm"] < 0)


def test_p3_equal_to_p2_gives_fd_one(pgt, ctx):
    """With P3 = P2 the site's num and fd_den are the same number, (p_j - p_i)(p_j - p_o) in exact arithmetic, computed by two
    groupings: they differ by a few 2^-53 of products <= 1.  The inputs keep that number above 0.09 at every site (p_i <= 0.3,
    p_o <= 0.2, p_j >= 0.6), so every term of both sums is positive and the ratio is 1 within 1e-14 — far inside the 1e-9 asked
    for; with p_j within 1e-6 of p_i or p_o the same few 2^-53 would be 1e-4 of the value, which no bound on fd could cover."""
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(1651)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    f[0] = np.round(rng.uniform(0.0, 0.3, n), 6)
    f[1] = np.round(rng.uniform(0.6, 1.0, n), 6)
    f[3] = np.where(rng.uniform(0, 1, n) < 0.6, 0.0, np.round(rng.uniform(0.0, 0.2, n), 6))
    f[2], c[2] = f[1].copy(), c[1].copy()
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    seen = 0
    for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, _ = pops_dev(ctx, tp, tf, tn, MININD, win)
        r = rows[0][rows[0]["n"] > 0]
        worst = float(np.max(np.abs(r["fd"] - 1.0)))
        print(f"{name}: largest |fd - 1| {worst:.3e}")
        assert worst <= 1e-9, (name, worst)
        seen += r.size
    assert seen > 5000


def test_fixed_outgroup_and_p2_above_p1_make_the_two_denominators_one(pgt, ctx):
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(1652)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    f[0], f[1] = np.minimum(f[0], f[1]), np.maximum(f[0], f[1])
    f[3] = np.zeros(n)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        assert np.array_equal(bits(rows[0]["fdm_den"]), bits(rows[0]["fd_den"])) and np.any(rows[0]["fd_den"] != 0), name
        assert np.array_equal(bits(rows[0]["fdm"]), bits(rows[0]["fd"])), name
        assert bits(tot["fdm_den"])[0] == bits(tot["fd_den"])[0]


def test_identical_sister_populations_give_zero(pgt, ctx):
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(1653)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    f[1], c[1] = f[0].copy(), c[0].copy()
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    for name, win in [("one site", one_site_table(n))] + tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        for fld in ("num", "fd", "fdm"):
            assert np.all(bits(rows[0][fld]) == 0), (name, fld)
        assert np.any(rows[0]["fd_den"] > 0) and np.all(rows[0]["fd_den"] >= 0) and bits(tot["num"])[0] == 0, name


# ---- 6: trio isolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 7])
def test_trios_do_not_see_the_other_populations(pgt, ctx, k):
    n = 2 * 8192 + 700
    rng = np.random.default_rng(1750 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    f2, c2 = uniform_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), W, S) for W, S in ((7, 3), (5000, 1000))])
    tp = _t(pos)
    rows, tot = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    for r in (0, (k - 1) // 2, k - 2):  # ingroup population r replaced: every trio without it keeps its bits
        fr, cr = list(f), list(c)
        fr[r], cr[r] = f2[r], c2[r]
        got, got_t = pops_dev(ctx, tp, [_t(x) for x in fr], [_t(x) for x in cr], MININD, win)
        kept = 0
        for t, ijk in enumerate(trio_order(k)):
            if r not in ijk:
                rows_equal(got[t], rows[t], f"K={k}, population {r} replaced, trio {ijk}")
                assert got_t[t].tobytes() == tot[t].tobytes()
                kept += 1
            else:
                assert got[t].tobytes() != rows[t].tobytes()
        assert kept == n_trios(k - 1)
    _, _, A, A_tot = fd_pops_model.model(pos, f, c, MININD, win)  # the bound's A
    for t, (i, j, kk) in enumerate(trio_order(k)):  # a trio's table from the K-population call = the four-population call's
        sel = (i, j, kk, k - 1)
        four, four_t = pops_dev(ctx, tp, [_t(f[x]) for x in sel], [_t(c[x]) for x in sel], MININD, win)
        assert_rows(rows[t], four[0], A, t, f"K={k} trio {(i, j, kk)} against the four-population call", quiet=True)
        assert_totals(tot[t:t + 1], four_t, {s: A_tot[s][t:t + 1] for s in SUMS}, f"K={k} trio {(i, j, kk)} totals")


# ---- 7: uncounted sites may hold anything -----------------------------------------------------------------------------------------
def test_uncounted_sites_may_hold_anything(pgt, ctx):
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(1850)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = uniform_pops(rng, n, k)
    win = np.concatenate([one_site_table(n)[:3000]] + [w for _, w in tables_for(pgt, pos, run_lengths(chr_ids))])
    tp = _t(pos)
    tame, tame_t = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    wild_f, wild_c = [x.copy() for x in f], [x.copy() for x in c]
    junk_f = np.array([np.nan, np.inf, -np.inf, 2.0])
    junk_c = np.array([0, -1, np.iinfo(np.int32).min], dtype=np.int32)
    for p in range(k):
        low = np.flatnonzero(c[p] < MININD)
        assert low.size > 1000
        wild_f[p][low] = junk_f[rng.integers(0, junk_f.size, low.size)]
        wild_c[p][low] = junk_c[rng.integers(0, junk_c.size, low.size)]
    wild, wild_t = pops_dev(ctx, tp, [_t(x) for x in wild_f], [_t(x) for x in wild_c], MININD, win)
    for t in range(n_trios(k)):
        rows_equal(wild[t], tame[t], f"trio {t}: wild values at uncounted sites")
        assert all(np.all(np.isfinite(wild[t][s])) for s in SUMS + ("fd", "fdm"))
    assert wild_t.tobytes() == tame_t.tobytes()
    assert all(np.all(np.isfinite(wild_t[s])) for s in SUMS)


# ---- 8: workspace contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(513, 4), (8193, 7), (600_001, 5)])
def test_rows_under_every_hint_poison_and_guard(pgt, ctx, n, k):
    W = 550_000 if n > 100_000 else 5000
    rng = np.random.default_rng(1950 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = uniform_pops(rng, n, k)
    fb, cb = uniform_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), min(W, n), max(1, min(W, n) // 4)),
                          pgt.build_windows_sites(run_lengths(chr_ids), min(1000, n), min(333, n))])
    want, want_t, A, A_tot = fd_pops_model.model(pos, f, c, MININD, win)
    dev = _dev()
    tf, tn = [padded_column(x, float("nan"), dev) for x in f], [padded_column(x, 1000, dev) for x in c]
    tp, wd = _t(pos), windows_to_device(win, dev)
    T = n_trios(k)
    tb = ctx.fd_pops_tree_bytes(k, n)
    _, _, foreign = ctx.fd_pops_reduce_dev(tp, [_t(x) for x in fb], [_t(x) for x in cb], MININD, wd)
    g = GuardedBuffers([tb, T * win.size * FD_ROW_DTYPE.itemsize, T * FD_TOTAL_DTYPE.itemsize], 41 + k, dev)
    tree, out, tot = g.bufs
    for hint in (0, W, 4 * W, 50_000):  # 50 000: at 600 001 sites too small a hint, the level-3 windows answered from level 2
        first = None
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):
                poison_tree(tree, kind, other=foreign)
                out.fill_(0xFF)
                tot.fill_(0xFF)
                ctx.fd_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
                what = f"n={n} K={k} hint={hint} poison={kind}"
                g.check(what)
                got = rows_from_device(out, FD_ROW_DTYPE).reshape(T, win.size).copy()
                got_t = rows_from_device(tot, FD_TOTAL_DTYPE).copy()
                if first is None:
                    first = (got, got_t)
                    for t in range(T):
                        assert_rows(got[t], want[t], A, t, what + f" trio {t}", quiet=True)
                    assert_totals(got_t, want_t, A_tot, what)
                else:  # identical under one hint, whatever the workspace held
                    assert got.tobytes() == first[0].tobytes() and got_t.tobytes() == first[1].tobytes(), what


# ---- 9: graph capture --------------------------------------------------------------------------------------------------------------
def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    import torch
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(2050)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    A_, B_ = uniform_pops(rng, n, k), uniform_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 100)
    dev = _dev()
    wd, tp = windows_to_device(win, dev), _t(pos)
    tf, tn = [_t(x) for x in A_[0]], [_t(x) for x in A_[1]]
    T = n_trios(k)
    g = GuardedBuffers([ctx.fd_pops_tree_bytes(k, n), T * win.size * FD_ROW_DTYPE.itemsize, T * FD_TOTAL_DTYPE.itemsize], 3, dev)
    tree, out, tot = g.bufs
    with ctx.hints(5000, 100, 0):
        ctx.fd_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # one call on one stream: a chain of kernels, no parallel branches
            ctx.fd_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
    for name, src in (("B", B_), ("A", A_)):
        for t, x in zip(tf + tn, src[0] + src[1]):
            t.copy_(torch.from_numpy(x))
        for buf in (tree, out, tot):
            buf.fill_(0xFF)
        graph.replay()
        g.check("fd_pops graph replay")
        want, want_t, A, A_tot = fd_pops_model.model(pos, src[0], src[1], MININD, win)
        got = rows_from_device(out, FD_ROW_DTYPE).reshape(T, win.size)
        for t in range(T):
            assert_rows(got[t], want[t], A, t, f"replay {name} trio {t}", quiet=True)
        assert_totals(rows_from_device(tot, FD_TOTAL_DTYPE), want_t, A_tot, f"replay {name}")


# ---- 10: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(pgt, ctx):
    import torch
    n, k = 10_000, 4
    rng = np.random.default_rng(2150)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = uniform_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 1000, 500)
    wd = windows_to_device(win, _dev())
    T = 1
    tb = ctx.fd_pops_tree_bytes(k, n)
    g = GuardedBuffers([tb, T * win.size * FD_ROW_DTYPE.itemsize, T * FD_TOTAL_DTYPE.itemsize], 5, _dev())
    tree, out, tot = g.bufs
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    lib, h = ctx._lib, ctx._ctx
    before = [b.clone() for b in g.bufs]

    def call(freq=None, nind=None, n_pops=k, minind=MININD, win_p=wd.data_ptr(), out_p=out.data_ptr(), out_bytes=out.numel(),
             tree_p=tree.data_ptr(), tree_bytes=tree.numel(), freq_null=False, nind_null=False, pos_p=tp.data_ptr()):
        fp = [t.data_ptr() for t in tf] if freq is None else freq
        npn = [t.data_ptr() for t in tn] if nind is None else nind
        pf = (C.c_void_p * 8)(*(fp + [None] * (8 - len(fp))))
        pn = (C.c_void_p * 8)(*(npn + [None] * (8 - len(npn))))
        return lib.pgt_fd_pops_reduce_dev(h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, n, minind, win_p, win.size,
                                          out_p, out_bytes, tot.data_ptr(), tree_p, tree_bytes, None)

    fp, npp = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    refusals = [
        (dict(minind=0), "minind"), (dict(minind=-3), "minind"),
        (dict(pos_p=None), "pos"), (dict(freq_null=True), "freq"), (dict(nind_null=True), "nind"), (dict(tree_p=None), "tree"), (dict(win_p=None), "win"),
        (dict(out_p=None), "out"), (dict(n_pops=3), "n_pops must be 4 ... 7"), (dict(n_pops=8), "n_pops must be 4 ... 7"), (dict(n_pops=0), "n_pops"),
        (dict(freq=[fp[0], None, fp[2], fp[3]]), "freq[1]"), (dict(nind=[npp[0], npp[1], npp[2], None]), "nind[3]"),
        (dict(freq=[fp[0], fp[1] + 8, fp[2], fp[3]]), "freq[1]"), (dict(nind=[npp[0], npp[1], npp[2] + 8, npp[3]]), "nind[2]"),
        (dict(nind=[npp[0] + 4, npp[1], npp[2], npp[3]]), "nind[0]"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(tree_bytes=tb - 1), "tree_bytes"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_fd_pops_reduce: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    want, _, A, _ = fd_pops_model.model(pos, f, c, MININD, win)
    assert_rows(rows_from_device(out, FD_ROW_DTYPE).reshape(T, win.size)[0], want[0], A, 0, "accepted call")

    # the host-buffer form refuses in the same words and returns before any upload
    rows_h, tot_h = np.zeros(win.size, dtype=FD_ROW_DTYPE), np.zeros(1, dtype=FD_TOTAL_DTYPE)
    hf = (C.c_void_p * 8)(*([x.ctypes.data for x in f] + [None] * 4))
    hn = (C.c_void_p * 8)(*([x.ctypes.data for x in c] + [None] * 4))
    for n_pops, minind, name in ((3, MININD, "n_pops must be 4 ... 7"), (8, MININD, "n_pops must be 4 ... 7"), (4, 0, "minind must be at least 1")):
        rc = lib.pgt_fd_pops_reduce(h, pos.ctypes.data, hf, hn, n_pops, n, minind, win.ctypes.data, win.size, rows_h.ctypes.data, tot_h.ctypes.data)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_fd_pops_reduce: "), (n_pops, minind, msg)
    rc = lib.pgt_fd_pops_reduce(h, pos.ctypes.data, None, hn, 4, n, MININD, win.ctypes.data, win.size, rows_h.ctypes.data, tot_h.ctypes.data)
    assert rc == _lib.PGT_EARG and "NULL" in _lib.last_error(h) and _lib.last_error(h).startswith("pgt_fd_pops_reduce: ")
    assert not rows_h.view(np.uint8).any() and not tot_h.view(np.uint8).any()

    # the Python wrappers refuse the population count, misaligned views and differing lengths by name
    m = 1000
    fcols = [torch.zeros(m + 4, dtype=torch.float64, device=_dev()) for _ in range(4)]
    ccols = [torch.ones(m + 4, dtype=torch.int32, device=_dev()) for _ in range(4)]
    posm = torch.arange(1, m + 1, dtype=torch.int32, device=_dev())
    w1 = windows_to_device(pgt.build_windows_sites(np.array([m], np.uint64), 100, 100), _dev())
    good_f, good_c = [t[4:4 + m] for t in fcols], [t[4:4 + m] for t in ccols]
    ctx.fd_pops_reduce_dev(posm, good_f, good_c, 1, w1)
    with pytest.raises(_lib.PgtError, match="fd_pops_reduce_dev: 4 ... 7 populations"):
        ctx.fd_pops_reduce_dev(posm, good_f[:3], good_c[:3], 1, w1)
    with pytest.raises(_lib.PgtError, match="4 ... 7 populations"):
        ctx.fd_pops_reduce_dev(posm, good_f * 2, good_c * 2, 1, w1)
    with pytest.raises(_lib.PgtError, match="4 ... 7 populations"):
        ctx.fd_pops_reduce(pos, f[:3], c[:3], MININD, win)
    with pytest.raises(_lib.PgtError, match=r"freqs\[1\]"):
        ctx.fd_pops_reduce_dev(posm, [good_f[0], fcols[1][1:1 + m], good_f[2], good_f[3]], good_c, 1, w1)
    with pytest.raises(_lib.PgtError, match=r"ninds\[2\]"):
        ctx.fd_pops_reduce_dev(posm, good_f, [good_c[0], good_c[1], ccols[2][2:2 + m], good_c[3]], 1, w1)
    with pytest.raises(_lib.PgtError, match="column lengths differ"):
        ctx.fd_pops_reduce_dev(posm, [good_f[0], good_f[1][:-4], good_f[2], good_f[3]], good_c, 1, w1)
    with pytest.raises(_lib.PgtError, match="column lengths differ"):
        ctx.fd_pops_reduce(pos, [f[0], f[1][:-1], f[2], f[3]], c, MININD, win)
    with pytest.raises(_lib.PgtError, match="minind"):
        ctx.fd_pops_reduce_dev(posm, good_f, good_c, 0, w1)
    torch.cuda.synchronize()


# ---- 11: host-buffer form -----------------------------------------------------------------------------------------------------------
def test_host_buffer_form_equals_the_device_form_twice_in_a_row(pgt, ctx):
    n, k = 2 * 8192 + 700, 5
    for seed in (73, 74):  # different data through the one context: nothing of the cached workspace may survive
        rng = np.random.default_rng(seed)
        chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
        f, c = uniform_pops(rng, n, k)
        win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 1000)
        rows, tot = ctx.fd_pops_reduce(pos, f, c, MININD, win)
        hints = pgt.window_scan.table_hints(win)
        with ctx.hints(hints[0], 0, 0):  # the host-buffer form derives the longest-window hint from the table
            want, want_t = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], MININD, win)
        assert rows.shape == want.shape == (4, win.size)
        for t in range(rows.shape[0]):
            rows_equal(np.ascontiguousarray(rows[t]), want[t], f"seed {seed} trio {t}")
        assert tot.tobytes() == want_t.tobytes()
    res = pgt.fd_window_pops(chr_ids, pos, f, c, 5000, 1000, MININD, 1, ctx=ctx)
    assert list(res) == trio_order(k) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    for t, ijk in enumerate(trio_order(k)):
        rows_equal(np.ascontiguousarray(res[ijk].rows), want[t], f"fd_window_pops trio {ijk}")
        assert res[ijk].total.tobytes() == want_t[t].tobytes()
    # -skip_missing drops a trio's rows without counted sites from that trio alone
    c0 = [x.copy() for x in c]
    c0[1][:6000] = 0
    full = pgt.fd_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, ctx=ctx)
    kept = pgt.fd_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, skip_missing=1, ctx=ctx)
    assert np.any(full[(0, 1, 2)].rows["n"] == 0)
    assert kept[(0, 1, 2)].rows.size == np.count_nonzero(full[(0, 1, 2)].rows["n"]) < full[(0, 1, 2)].rows.size
    assert kept[(0, 2, 3)].rows.size == np.count_nonzero(full[(0, 2, 3)].rows["n"]) > kept[(0, 1, 2)].rows.size
    assert np.all(kept[(0, 1, 2)].rows["n"] > 0) and kept[(0, 1, 2)].win.size == kept[(0, 1, 2)].rows.size


# ---- 12: a build wave's second tile ---------------------------------------------------------------------------------------------------
def test_a_build_waves_second_tile(pgt, ctx):
    """K = 5 takes the one-wave build (kOneWaveFrom = 5, held to csrc/ by tests/test_fd_pops_cpu.py): 1025 tiles are walked by
    516 waves in two rounds, so tile 516 is wave 0's second.  The explicit ranges of pops_grid_shapes.second_round_windows
    against the model."""
    k, tiles = 5, 1025
    rounds, waves, n_waves = shapes.pops_build(tiles, k)
    assert (rounds, waves, n_waves) == (2, 513, 516) and shapes.tiles_of_wave(tiles, n_waves).max() == 2
    n = shapes.ragged_n(tiles)
    rng = np.random.default_rng(2250)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = uniform_pops(rng, n, k)
    win, names = shapes.second_round_windows(n, tiles, n_waves)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
    want, want_t, A, A_tot = fd_pops_model.model(pos, f, c, MININD, win)
    lo = win["lo"].astype(np.int64)
    one = (win["hi"] - win["lo"]) == 1
    for t, (i, j, kk) in enumerate(trio_order(k)):
        assert_rows(rows[t], want[t], A, t, f"second tile, trio {(i, j, kk)}")
        ok = fd_pops_model.counted(c, i, j, kk, MININD)[lo[one]]
        for fld, x in zip(SUMS, fd_pops_model.site_terms(f[i][lo[one]], f[j][lo[one]], f[kk][lo[one]], f[k - 1][lo[one]])):
            assert np.array_equal(bits(rows[t][fld][one]), bits(np.where(ok, x, 0.0) + 0.0)), (names, fld)
    assert_totals(tot, want_t, A_tot, "second tile, totals")
