"""GPU: f4 of all quartets of 4 ... 6 populations, every quartet in its three pairings, from per-population (freq, nInd)
columns (pgt_f4_pops_reduce_dev / pgt_f4_pops_reduce).

The yardsticks are the float64 NumPy model of the definition (tests/f4_pops_model.py), the exact-rational fixture
(tests/golden/f4_exact.json), the ABBA-BABA sums of pgt_dstat_pops_reduce_dev on the same columns and the definition's own
properties — never the code under test.
Tolerance: counts, coordinates and mid exact; the three sums within |x - y| <= 1e-9 A + 1e-12, A the window's Σ|product| of the
same pairing (the site terms have both signs, so a bound relative to |y| would be wrong; any summation order of n <= 9e6
doubles stays within n 2^-53 A < 1e-9 A); reserved_ +0.0; one-site windows bit for bit."""
import ctypes as C

import numpy as np
import pytest

import f4_pops_model
import helpers
import synth
from f4_pops_model import SUMS, all_quartet_order
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import DSTAT_ROW_DTYPE, F4_ROW_DTYPE, F4_TOTAL_DTYPE, WIN_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, run_lengths, windows_to_device
from test_fst_pops import MININD, SIZES, _dev, _t, random_pops, tables_for

pytestmark = pytest.mark.gpu
REL_A, ABS = 1e-9, 1e-12


def n_quartets(k):
    return len(all_quartet_order(k))


def pops_dev(ctx, tp, tf, tn, minind, win, **kw):
    """-> (rows[n_quartets, n_win], totals[n_quartets] or None) of one f4_pops_reduce_dev call"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.f4_pops_reduce_dev(tp, tf, tn, minind, wd, **kw)
    Q = n_quartets(len(tf))
    rows = rows_from_device(out, F4_ROW_DTYPE)[: Q * win.size].reshape(Q, win.size)
    return rows, (rows_from_device(tot, F4_TOTAL_DTYPE)[:Q] if tot is not None else None)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def excess(x, y, A):
    """max of |x - y| - (1e-9 A + 1e-12): <= 0 when every entry is within the bound"""
    x, y, A = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x, y, A))
    return -1.0 if x.size == 0 else float(np.max(np.abs(x - y) - (REL_A * A + ABS)))


def assert_rows(got, want, A, t, what, quiet=True):
    assert got.size == want.size, what
    for fld in ("start", "end", "mid", "n"):
        assert np.array_equal(got[fld], want[fld]), (what, fld)
    assert np.all(bits(got["reserved_"]) == 0), (what, "reserved_ is +0.0")
    for fld in SUMS:
        e = excess(got[fld], want[fld], A[fld][t])
        if not quiet:
            print(f"{what} {fld}: excess over the bound {e:.3e}")
        assert e <= 0.0, (what, fld, e)


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


# ---- rows and genome-wide lines against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 5, 6])
def test_rows_and_totals_against_the_numpy_model(pgt, ctx, k):
    for si, n in enumerate(SIZES):
        rng = np.random.default_rng(4400 * k + si)
        chr_ids, pos = synth.chromosomes(rng, n, min(1 + (si + k) % 3, n), equal=False)
        f, c = random_pops(rng, n, k)
        tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
        for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
            want, want_t, A, A_tot = f4_pops_model.model(pos, f, c, MININD, win)
            for t, q in enumerate(all_quartet_order(k)):
                assert_rows(rows[t], want[t], A, t, f"K={k} n={n} {name} quartet {q}", quiet=n < 8193 or t > 0)
            assert_totals(tot, want_t, A_tot, f"K={k} n={n} {name} totals")


def test_the_exact_fixture_through_the_host_buffer_form(pgt, ctx):
    """tests/golden/f4_exact.json: every sum within 1e-9 A + 1e-12 of the exact rational (A from the model, which
    tests/test_f4_pops_cpu.py holds to the same fixture), counts exact, one-site windows within one rounding of the product."""
    k = helpers.load_golden("f4_exact.json")
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    empty = win["lo"] == win["hi"]  # the host-buffer form takes an empty window only with coordinates of its own
    assert empty.sum() == 1
    win["flags"][empty], win["start"][empty], win["end"][empty] = 1, 77, 99
    whole = k["windows"].index([0, len(k["sets"][0]["pos"])])
    for s in k["sets"]:
        pos = np.array(s["pos"], dtype=np.uint32)
        f, c = [np.array(x, dtype=np.float64) for x in s["freq"]], [np.array(x, dtype=np.int32) for x in s["nind"]]
        for case in s["cases"]:
            rows, tot = ctx.f4_pops_reduce(pos, f, c, case["minind"], win)
            _, _, A, A_tot = f4_pops_model.model(pos, f, c, case["minind"], win)
            assert rows.shape == (len(case["quartets"]), win.size)
            for t, q in enumerate(case["quartets"]):
                what = f"K={s['n_pops']} minind={case['minind']} quartet {q['quartet']}"
                assert tuple(q["quartet"]) == all_quartet_order(s["n_pops"])[t]
                assert np.array_equal(rows[t]["n"], np.array(q["n"], dtype=np.uint32)), what
                assert int(tot[t]["neff"]) == q["n"][whole] and int(tot[t]["nskip"]) == pos.size - q["n"][whole], what
                assert np.all(bits(rows[t]["reserved_"]) == 0), what
                assert [int(rows[t][x][empty][0]) for x in ("start", "end", "mid", "n")] == [77, 99, 88, 0], what
                for fld in SUMS:
                    e = excess(rows[t][fld], np.array(q[fld]), A[fld][t])
                    assert e <= 0.0, (what, fld, e)
                    assert excess(tot[t][fld], q[fld][whole], A_tot[fld][t]) <= 0.0, (what, fld)


def test_level3_nodes_are_built_and_used(pgt, ctx):
    n, W, k = 600_001, 550_000, 4
    rng = np.random.default_rng(4433)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, 10_000)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.any(-(-lo // (8192 * 64)) < hi // (8192 * 64)), "a window must contain a level-3 node"
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = f4_pops_model.model(pos, f, c, MININD, win)
    for hint in (0, W, 50_000):  # 50 000: too small a hint for these windows, answered from level 2
        with ctx.hints(hint, 0, 0):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        assert_rows(rows[0], want[0], A, 0, f"level 3, hint {hint}", quiet=False)
        assert_totals(tot, want_t, A_tot, f"level 3, hint {hint}")


# ---- one-site windows carry the definition's bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 6])
def test_one_site_windows_carry_the_bits_of_the_definition(pgt, ctx, k):
    n = 8193
    rng = np.random.default_rng(4450 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    for x in f:  # exact 0 and 1, and ties between neighbours, among the sites
        x[rng.integers(0, n, 200)] = 0.0
        x[rng.integers(0, n, 200)] = 1.0
    for a in range(k - 1):
        at = rng.integers(0, n, 300)
        f[a + 1][at] = f[a][at]
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    win = one_site_table(n)
    for minind in (1, 5):
        rows, tot = pops_dev(ctx, tp, tf, tn, minind, win)
        for t, (i, j, kk, l) in enumerate(all_quartet_order(k)):
            what = f"K={k} minind={minind} quartet {(i, j, kk, l)}"
            ok = f4_pops_model.counted(c, i, j, kk, l, minind)
            assert np.array_equal(rows[t]["n"], ok.astype(np.uint32)), what
            assert np.array_equal(rows[t]["start"], pos) and np.array_equal(rows[t]["end"], pos) and np.array_equal(rows[t]["mid"], pos), what
            assert np.all(bits(rows[t]["reserved_"]) == 0), what
            terms, _ = f4_pops_model.site_terms(f[i], f[j], f[kk], f[l])
            for fld, x in zip(SUMS, terms):
                assert np.array_equal(bits(rows[t][fld]), bits(np.where(ok, x, 0.0) + 0.0)), (what, fld)
            assert int(tot[t]["neff"]) == int(ok.sum()) and int(tot[t]["nskip"]) == n - int(ok.sum())


# ---- the identity of the three pairings ----------------------------------------------------------------------------------------
def test_the_three_sums_of_a_row_cancel(pgt, ctx):
    """In real arithmetic s0 - s1 + s2 = 0 at every site.  Each of a row's three sums lies within 1e-9 A_c + 1e-12 of its exact
    value, so |Σs0 - Σs1 + Σs2| <= 1e-9 (A_0 + A_1 + A_2) + 3e-12 <= 3 (1e-9 A + 1e-12) with A the largest of the three."""
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(4460)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        _, _, A, A_tot = f4_pops_model.model(pos, f, c, MININD, win)
        for t in range(n_quartets(k)):
            r = rows[t]
            Amax = np.maximum(np.maximum(A[SUMS[0]][t], A[SUMS[1]][t]), A[SUMS[2]][t])
            gap = np.abs(r[SUMS[0]] - r[SUMS[1]] + r[SUMS[2]])
            assert np.all(gap <= 3 * (REL_A * Amax + ABS)), (name, t, float(gap.max()))
            assert np.any(r[SUMS[0]] != 0)
            g = tot[t]
            assert abs(g[SUMS[0]] - g[SUMS[1]] + g[SUMS[2]]) <= 3 * (REL_A * max(A_tot[s][t] for s in SUMS) + ABS)


# ---- against the ABBA-BABA sums of the other entry point ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 5, 6])
def test_against_the_d_kernel_with_the_last_population_as_the_outgroup(pgt, ctx, k):
    """pgt_dstat_pops_reduce_dev on the same columns, O = K-1 the outgroup, trio (i, j, k) and quartet (i, j, k, O): both count
    the sites where all four populations have minind individuals, so n is equal.  With q = 1 - p, the D call's per-site patterns
        bbaa = p_i p_j q_k q_o + q_i q_j p_k p_o,  abba = q_i p_j p_k q_o + p_i q_j q_k p_o,  baba = p_i q_j p_k q_o + q_i p_j q_k p_o
    give     abba - baba = (q_i p_j - p_i q_j)(p_k q_o - q_k p_o) = (p_j - p_i)(p_k - p_o) = -d_ij d_ko = -s0
             bbaa - abba = (p_i q_k - q_i p_k)(p_j q_o - q_j p_o) = (p_i - p_k)(p_j - p_o) =  d_ik d_jo =  s1
             bbaa - baba = (p_j q_k - q_j p_k)(p_i q_o - q_i p_o) = (p_j - p_k)(p_i - p_o) =  d_jk d_io =  s2
    (x q_y - q_x p_y = p_x - p_y).  So Σs0 = Σbaba - Σabba, Σs1 = Σbbaa - Σabba, Σs2 = Σbbaa - Σbaba up to the rounding of both
    calls: within 1e-9 (the two D sums involved + A) + 1e-12, the D sums being sums of non-negative terms at these inputs."""
    n = 2 * 8192 + 700
    rng = np.random.default_rng(4470 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    quartets = all_quartet_order(k)
    trios = pgt.trio_order(k)
    for name, win in [("one site", one_site_table(n)[:2000])] + tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        out, _, _ = ctx.dstat_pops_reduce_dev(tp, tf, tn, MININD, windows_to_device(win, _dev()), tot=False)
        d = rows_from_device(out, DSTAT_ROW_DTYPE)[: len(trios) * win.size].reshape(len(trios), win.size)
        _, _, A, _ = f4_pops_model.model(pos, f, c, MININD, win)
        for td, (i, j, kk) in enumerate(trios):
            t = quartets.index((i, j, kk, k - 1))
            what = f"K={k} {name} trio {(i, j, kk)}"
            assert np.array_equal(rows[t]["n"], d[td]["n"]) and np.any(d[td]["n"] > 0), what
            for fld, plus, minus in ((SUMS[0], "baba", "abba"), (SUMS[1], "bbaa", "abba"), (SUMS[2], "bbaa", "baba")):
                gap = np.abs(rows[t][fld] - (d[td][plus] - d[td][minus]))
                bound = REL_A * (np.abs(d[td][plus]) + np.abs(d[td][minus]) + A[fld][t]) + ABS
                assert np.all(gap <= bound), (what, fld, float(np.max(gap - bound)))


# ---- quartet isolation, the allele flip and reproducibility --------------------------------------------------------------------------
def test_quartets_do_not_see_the_other_populations_and_calls_repeat(pgt, ctx):
    n, k = 2 * 8192 + 700, 6
    rng = np.random.default_rng(4650)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), W, S) for W, S in ((7, 3), (5000, 1000))])
    tp = _t(pos)
    rows, tot = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    again, again_t = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    assert again.tobytes() == rows.tobytes() and again_t.tobytes() == tot.tobytes()  # two calls give the same bits
    # quartet (0,1,2,3) of the K = 6 call has the bits of the K = 4 call on those columns — and so have the others
    for t, sel in enumerate(all_quartet_order(k)):
        if t in (0, 7, 14):
            four, four_t = pops_dev(ctx, tp, [_t(f[x]) for x in sel], [_t(c[x]) for x in sel], MININD, win)
            rows_equal(np.ascontiguousarray(rows[t]), four[0], f"quartet {sel} of the K = 6 call against the K = 4 call")
            assert four_t[0].tobytes() == tot[t].tobytes()
    # populations 4 and 5 poisoned with NaN (their counts kept, so the sites still count): (0,1,2,3) keeps its bits, and every
    # quartet that holds 4 or 5 and counts a site turns NaN
    fp = [x.copy() for x in f]
    fp[4][:] = np.nan
    fp[5][:] = np.nan
    got, got_t = pops_dev(ctx, tp, [_t(x) for x in fp], [_t(x) for x in c], MININD, win)
    for t, q in enumerate(all_quartet_order(k)):
        if 4 not in q and 5 not in q:
            assert q == (0, 1, 2, 3)
            rows_equal(np.ascontiguousarray(got[t]), np.ascontiguousarray(rows[t]), "populations 4 and 5 are NaN, quartet (0,1,2,3)")
            assert got_t[t].tobytes() == tot[t].tobytes()
        else:
            assert np.array_equal(got[t]["n"], rows[t]["n"])
            assert all(np.all(np.isnan(got[t][s][rows[t]["n"] > 0])) for s in SUMS) and np.isnan(got_t[t][SUMS[0]])


def test_flipping_the_allele_in_all_populations_keeps_the_bits(pgt, ctx):
    """Frequencies that are multiples of 2^-10: 1 - p is exact and every difference only changes its sign, so every product,
    and with it every sum, keeps its bits under p -> 1 - p in ALL columns."""
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(4660)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f = [rng.integers(0, 1025, n) / 1024.0 for _ in range(k)]
    c = [rng.integers(0, 21, n, dtype=np.int32) for _ in range(k)]
    win = np.concatenate([one_site_table(n)[:3000]] + [w for _, w in tables_for(pgt, pos, run_lengths(chr_ids))])
    tp, tn = _t(pos), [_t(x) for x in c]
    a, a_t = pops_dev(ctx, tp, [_t(x) for x in f], tn, MININD, win)
    b, b_t = pops_dev(ctx, tp, [_t(1.0 - x) for x in f], tn, MININD, win)
    assert a.tobytes() == b.tobytes() and a_t.tobytes() == b_t.tobytes()
    assert np.any(a[0][SUMS[0]] < 0) and np.any(a[0][SUMS[0]] > 0)


def test_uncounted_sites_may_hold_anything(pgt, ctx):
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(4750)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
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
    for t in range(n_quartets(k)):
        rows_equal(np.ascontiguousarray(wild[t]), np.ascontiguousarray(tame[t]), f"quartet {t}: wild values at uncounted sites")
        assert all(np.all(np.isfinite(wild[t][s])) for s in SUMS)
    assert wild_t.tobytes() == tame_t.tobytes()


# ---- workspace and output contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(513, 4), (8193, 6), (600_001, 5)])
def test_rows_under_every_hint_poison_and_guard(pgt, ctx, n, k):
    W = 550_000 if n > 100_000 else 5000
    rng = np.random.default_rng(4850 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    fb, cb = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), min(W, n), max(1, min(W, n) // 4)),
                          pgt.build_windows_sites(run_lengths(chr_ids), min(1000, n), min(333, n))])
    want, want_t, A, A_tot = f4_pops_model.model(pos, f, c, MININD, win)
    dev = _dev()
    tf, tn = [padded_column(x, float("nan"), dev) for x in f], [padded_column(x, 1000, dev) for x in c]
    tp, wd = _t(pos), windows_to_device(win, dev)
    Q = n_quartets(k)
    tb = ctx.f4_pops_tree_bytes(k, n)
    _, _, foreign = ctx.f4_pops_reduce_dev(tp, [_t(x) for x in fb], [_t(x) for x in cb], MININD, wd)
    g = GuardedBuffers([tb, Q * win.size * F4_ROW_DTYPE.itemsize, Q * F4_TOTAL_DTYPE.itemsize], 47 + k, dev)
    tree, out, tot = g.bufs
    for hint in (0, W, 50_000):  # 50 000: at 600 001 sites too small a hint, the level-3 windows answered from level 2
        first = None
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):
                poison_tree(tree, kind, other=foreign)
                out.fill_(0xFF)
                tot.fill_(0xFF)
                ctx.f4_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
                what = f"n={n} K={k} hint={hint} poison={kind}"
                g.check(what)
                got = rows_from_device(out, F4_ROW_DTYPE).reshape(Q, win.size).copy()
                got_t = rows_from_device(tot, F4_TOTAL_DTYPE).copy()
                if first is None:
                    first = (got, got_t)
                    for t in range(Q):
                        assert_rows(got[t], want[t], A, t, what + f" quartet {t}")
                    assert_totals(got_t, want_t, A_tot, what)
                else:  # identical under one hint, whatever the workspace held
                    assert got.tobytes() == first[0].tobytes() and got_t.tobytes() == first[1].tobytes(), what
    # tot=None (no genome-wide lines: the totals buffer stays as it was) and the global-only form (n_win = 0: no row is written),
    # under the last hint of the loop above, whose rows `first` holds
    out.fill_(0xFF)
    tot.fill_(0xFF)
    with ctx.hints(hint, 0, 0):
        ctx.f4_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=False, tree=tree)
        g.check("tot = NULL")
        assert rows_from_device(out, F4_ROW_DTYPE).reshape(Q, win.size).tobytes() == first[0].tobytes()
        assert bool((tot == 0xFF).all()), "tot = NULL: the totals buffer is not written"
        out.fill_(0xFF)
        ctx.f4_pops_reduce_dev(tp, tf, tn, MININD, wd[:0], out=out, tot=tot, tree=tree)
        g.check("n_win = 0")
        assert bool((out == 0xFF).all()), "n_win = 0: no row is written"
        assert rows_from_device(tot, F4_TOTAL_DTYPE).tobytes() == first[1].tobytes()


def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    import torch
    n, k = 2 * 8192 + 700, 5
    rng = np.random.default_rng(4950)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    A_, B_ = random_pops(rng, n, k), random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 100)
    dev = _dev()
    wd, tp = windows_to_device(win, dev), _t(pos)
    tf, tn = [_t(x) for x in A_[0]], [_t(x) for x in A_[1]]
    Q = n_quartets(k)
    g = GuardedBuffers([ctx.f4_pops_tree_bytes(k, n), Q * win.size * F4_ROW_DTYPE.itemsize, Q * F4_TOTAL_DTYPE.itemsize], 3, dev)
    tree, out, tot = g.bufs
    with ctx.hints(5000, 100, 0):
        ctx.f4_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)  # warm-up outside the capture
        torch.cuda.synchronize()
        direct = (rows_from_device(out, F4_ROW_DTYPE).tobytes(), rows_from_device(tot, F4_TOTAL_DTYPE).tobytes())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # one call on one stream: a chain of kernels, no parallel branches
            ctx.f4_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
    for name, src in (("B", B_), ("A", A_)):
        for t, x in zip(tf + tn, src[0] + src[1]):
            t.copy_(torch.from_numpy(x))
        for buf in (tree, out, tot):
            buf.fill_(0xFF)
        graph.replay()
        g.check("f4_pops graph replay")
        want, want_t, A, A_tot = f4_pops_model.model(pos, src[0], src[1], MININD, win)
        got = rows_from_device(out, F4_ROW_DTYPE).reshape(Q, win.size)
        for t in range(Q):
            assert_rows(got[t], want[t], A, t, f"replay {name} quartet {t}")
        assert_totals(rows_from_device(tot, F4_TOTAL_DTYPE), want_t, A_tot, f"replay {name}")
    # the replay on the first columns has the bits of the direct call on them
    assert (rows_from_device(out, F4_ROW_DTYPE).tobytes(), rows_from_device(tot, F4_TOTAL_DTYPE).tobytes()) == direct


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(pgt, ctx):
    import torch
    n, k = 10_000, 4
    rng = np.random.default_rng(5050)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 1000, 500)
    wd = windows_to_device(win, _dev())
    Q = 1
    tb = ctx.f4_pops_tree_bytes(k, n)
    g = GuardedBuffers([tb, Q * win.size * F4_ROW_DTYPE.itemsize, Q * F4_TOTAL_DTYPE.itemsize], 5, _dev())
    tree, out, tot = g.bufs
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    lib, h = ctx._lib, ctx._ctx
    before = [b.clone() for b in g.bufs]

    def call(dstat=False, freq=None, nind=None, n_pops=k, minind=MININD, win_p=wd.data_ptr(), out_p=out.data_ptr(), out_bytes=out.numel(),
             tree_p=tree.data_ptr(), tree_bytes=tree.numel(), freq_null=False, nind_null=False, pos_p=tp.data_ptr()):
        fp = [t.data_ptr() for t in tf] if freq is None else freq
        npn = [t.data_ptr() for t in tn] if nind is None else nind
        pf = (C.c_void_p * 8)(*(fp + [None] * (8 - len(fp))))
        pn = (C.c_void_p * 8)(*(npn + [None] * (8 - len(npn))))
        fn = lib.pgt_dstat_pops_reduce_dev if dstat else lib.pgt_f4_pops_reduce_dev
        return fn(h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, n, minind, win_p, win.size,
                  out_p, out_bytes, tot.data_ptr(), tree_p, tree_bytes, None)

    fp, npp = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    refusals = [
        (dict(minind=0), "minind must be at least 1"), (dict(minind=-3), "minind"),
        (dict(pos_p=None), "pos"), (dict(freq_null=True), "freq"), (dict(nind_null=True), "nind"), (dict(tree_p=None), "tree"), (dict(win_p=None), "win"),
        (dict(out_p=None), "out"), (dict(n_pops=3), "n_pops must be 4 ... 6"), (dict(n_pops=7), "n_pops must be 4 ... 6"), (dict(n_pops=0), "n_pops"),
        (dict(freq=[fp[0], None, fp[2], fp[3]]), "freq[1]"), (dict(nind=[npp[0], npp[1], npp[2], None]), "nind[3]"),
        (dict(freq=[fp[0], fp[1] + 8, fp[2], fp[3]]), "freq[1] is not 16-byte aligned"), (dict(nind=[npp[0], npp[1], npp[2] + 8, npp[3]]), "nind[2]"),
        (dict(nind=[npp[0] + 4, npp[1], npp[2], npp[3]]), "nind[0]"), (dict(tree_p=tree.data_ptr() + 8), "tree is not 16-byte aligned"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(tree_bytes=tb - 1), "tree_bytes"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f4_pops_reduce: "), (kw, rc, msg)
    for minind in (0, -3, -2 ** 31):  # a minind the D call refuses is refused here, in the D call's words
        assert call(dstat=True, minind=minind) == _lib.PGT_EARG
        d_msg = _lib.last_error(h)
        assert call(minind=minind) == _lib.PGT_EARG
        assert _lib.last_error(h) == d_msg.replace("pgt_dstat_pops_reduce: ", "pgt_f4_pops_reduce: ") != d_msg
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    want, _, A, _ = f4_pops_model.model(pos, f, c, MININD, win)
    assert_rows(rows_from_device(out, F4_ROW_DTYPE).reshape(Q, win.size)[0], want[0], A, 0, "accepted call", quiet=False)

    # the host-buffer form refuses in the same words and returns before any upload
    rows_h, tot_h = np.zeros(win.size, dtype=F4_ROW_DTYPE), np.zeros(1, dtype=F4_TOTAL_DTYPE)
    hf = (C.c_void_p * 8)(*([x.ctypes.data for x in f] + [None] * 4))
    hn = (C.c_void_p * 8)(*([x.ctypes.data for x in c] + [None] * 4))
    for n_pops, minind, name in ((3, MININD, "n_pops must be 4 ... 6"), (7, MININD, "n_pops must be 4 ... 6"), (4, 0, "minind must be at least 1")):
        rc = lib.pgt_f4_pops_reduce(h, pos.ctypes.data, hf, hn, n_pops, n, minind, win.ctypes.data, win.size, rows_h.ctypes.data, tot_h.ctypes.data)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f4_pops_reduce: "), (n_pops, minind, msg)
    assert not rows_h.view(np.uint8).any() and not tot_h.view(np.uint8).any()

    # the Python wrappers refuse the population count by name
    with pytest.raises(_lib.PgtError, match="f4_pops_reduce_dev: 4 ... 6 populations"):
        ctx.f4_pops_reduce_dev(tp, tf[:3], tn[:3], 1, wd)
    with pytest.raises(_lib.PgtError, match="4 ... 6 populations"):
        ctx.f4_pops_reduce(pos, f * 2, c * 2, MININD, win)
    with pytest.raises(_lib.PgtError, match="minind"):
        ctx.f4_pops_reduce_dev(tp, tf, tn, 0, wd)
    torch.cuda.synchronize()


# ---- host-buffer form and the Python mirror -------------------------------------------------------------------------------------
def test_host_buffer_form_equals_the_device_form_twice_in_a_row(pgt, ctx):
    n, k = 2 * 8192 + 700, 5
    for seed in (93, 94):  # different data through the one context: nothing of the cached workspace may survive
        rng = np.random.default_rng(seed)
        chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
        f, c = random_pops(rng, n, k)
        win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 1000)
        rows, tot = ctx.f4_pops_reduce(pos, f, c, MININD, win)
        hints = pgt.window_scan.table_hints(win)
        with ctx.hints(hints[0], 0, 0):  # the host-buffer form derives the longest-window hint from the table
            want, want_t = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], MININD, win)
        assert rows.shape == want.shape == (5, win.size)
        for t in range(rows.shape[0]):
            rows_equal(np.ascontiguousarray(rows[t]), np.ascontiguousarray(want[t]), f"seed {seed} quartet {t}")
        assert tot.tobytes() == want_t.tobytes()
    res = pgt.f4_window_pops(chr_ids, pos, f, c, 5000, 1000, MININD, 1, ctx=ctx)
    assert list(res) == pgt.all_quartet_order(k) == [(0, 1, 2, 3), (0, 1, 2, 4), (0, 1, 3, 4), (0, 2, 3, 4), (1, 2, 3, 4)]
    for t, q in enumerate(pgt.all_quartet_order(k)):
        rows_equal(np.ascontiguousarray(res[q].rows), np.ascontiguousarray(want[t]), f"f4_window_pops quartet {q}")
        assert res[q].total.tobytes() == want_t[t].tobytes()
    # -skip_missing drops a quartet's rows without counted sites from that quartet alone
    c0 = [x.copy() for x in c]
    c0[1][:6000] = 0
    full = pgt.f4_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, ctx=ctx)
    kept = pgt.f4_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, skip_missing=1, ctx=ctx)
    assert np.any(full[(0, 1, 2, 3)].rows["n"] == 0)
    assert kept[(0, 1, 2, 3)].rows.size == np.count_nonzero(full[(0, 1, 2, 3)].rows["n"]) < full[(0, 1, 2, 3)].rows.size
    assert kept[(0, 2, 3, 4)].rows.size == np.count_nonzero(full[(0, 2, 3, 4)].rows["n"]) > kept[(0, 1, 2, 3)].rows.size
    # jackknife=True on disjoint windows: the same rows, and the items of the device jackknife on them
    plain = pgt.f4_window_pops(chr_ids, pos, f, c, 5000, 5000, MININD, 1, ctx=ctx)
    jk = pgt.f4_window_pops(chr_ids, pos, f, c, 5000, 5000, MININD, 1, jackknife=True, ctx=ctx)
    assert set(jk) == set(plain) | {"jackknife"} and list(jk["jackknife"]) == pgt.all_quartet_order(k)
    for q in pgt.all_quartet_order(k):
        rows_equal(np.ascontiguousarray(jk[q].rows), np.ascontiguousarray(plain[q].rows), f"jackknife=True rows of quartet {q}")
        host = ctx.f4_jackknife(plain[q].rows[None, :])[0]
        assert host.tobytes() == jk["jackknife"][q].tobytes()
        assert jk["jackknife"][q]["n_blocks"][0] == np.count_nonzero(plain[q].rows["n"])
