"""GPU: f3 of all trios of 3 ... 6 populations, every population of a trio as the target, from per-population (freq, nInd)
columns (pgt_f3_pops_reduce_dev / pgt_f3_pops_reduce).

The yardsticks are the float64 NumPy model of the definition (tests/f3_pops_model.py), Hudson's numerator from
pgt_fst_hudson_pops_reduce_dev on the same columns and the definition's own properties — never the code under test.
Tolerance: counts, coordinates and mid exact; f3_i, f3_j, f3_k within |x - y| <= 1e-9 A + 1e-12, A the window's
Σ(|product| + |h|) (the site terms have both signs, so a bound relative to |y| would be wrong; any summation order of n <= 9e6
doubles stays within n 2^-53 A < 1e-9 A); reserved_ +0.0; one-site windows bit for bit."""
import ctypes as C

import numpy as np
import pytest

import f3_pops_model
import synth
from f3_pops_model import SUMS, all_trio_order
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import F3_ROW_DTYPE, F3_TOTAL_DTYPE, FST_ROW_DTYPE, WIN_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device, run_lengths, windows_to_device
from test_fst_pops import MININD, SIZES, _dev, _t, random_pops, tables_for

pytestmark = pytest.mark.gpu
REL_A, ABS = 1e-9, 1e-12


def n_trios(k):
    return len(all_trio_order(k))


def pops_dev(ctx, tp, tf, tn, minind, win, **kw):
    """-> (rows[n_trios, n_win], totals[n_trios] or None) of one f3_pops_reduce_dev call"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.f3_pops_reduce_dev(tp, tf, tn, minind, wd, **kw)
    T = n_trios(len(tf))
    rows = rows_from_device(out, F3_ROW_DTYPE)[: T * win.size].reshape(T, win.size)
    return rows, (rows_from_device(tot, F3_TOTAL_DTYPE)[:T] if tot is not None else None)


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
@pytest.mark.parametrize("k", [3, 4, 6])
def test_rows_and_totals_against_the_numpy_model(pgt, ctx, k):
    for si, n in enumerate(SIZES):
        rng = np.random.default_rng(3300 * k + si)
        chr_ids, pos = synth.chromosomes(rng, n, min(1 + (si + k) % 3, n), equal=False)
        f, c = random_pops(rng, n, k)
        tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
        for name, win in tables_for(pgt, pos, run_lengths(chr_ids)):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
            want, want_t, A, A_tot = f3_pops_model.model(pos, f, c, MININD, win)
            for t, ijk in enumerate(all_trio_order(k)):
                assert_rows(rows[t], want[t], A, t, f"K={k} n={n} {name} trio {ijk}", quiet=n < 8193 or t > 0)
            assert_totals(tot, want_t, A_tot, f"K={k} n={n} {name} totals")


def test_level3_nodes_are_built_and_used(pgt, ctx):
    n, W, k = 600_001, 550_000, 3
    rng = np.random.default_rng(3333)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, 10_000)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.any(-(-lo // (8192 * 64)) < hi // (8192 * 64)), "a window must contain a level-3 node"
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = f3_pops_model.model(pos, f, c, MININD, win)
    for hint in (0, W, 50_000):  # 50 000: too small a hint for these windows, answered from level 2
        with ctx.hints(hint, 0, 0):
            rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        assert_rows(rows[0], want[0], A, 0, f"level 3, hint {hint}", quiet=False)
        assert_totals(tot, want_t, A_tot, f"level 3, hint {hint}")


# ---- one-site windows carry the definition's bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 6])
def test_one_site_windows_carry_the_bits_of_the_definition(pgt, ctx, k):
    n = 8193
    rng = np.random.default_rng(3450 + k)
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
        for t, (i, j, kk) in enumerate(all_trio_order(k)):
            what = f"K={k} minind={minind} trio {(i, j, kk)}"
            ok = f3_pops_model.counted(c, i, j, kk, minind)
            assert np.array_equal(rows[t]["n"], ok.astype(np.uint32)), what
            assert np.array_equal(rows[t]["start"], pos) and np.array_equal(rows[t]["end"], pos) and np.array_equal(rows[t]["mid"], pos), what
            assert np.all(bits(rows[t]["reserved_"]) == 0), what
            terms, _ = f3_pops_model.site_terms(f[i], f[j], f[kk], c[i], c[j], c[kk])
            for fld, x in zip(SUMS, terms):
                assert np.array_equal(bits(rows[t][fld]), bits(np.where(ok, x, 0.0) + 0.0)), (what, fld)
            assert int(tot[t]["neff"]) == int(ok.sum()) and int(tot[t]["nskip"]) == n - int(ok.sum())


# ---- s0 + s1 against Hudson's numerator from the other entry point -----------------------------------------------------------------
def test_the_first_two_targets_add_up_to_hudsons_numerator_of_the_pair(pgt, ctx):
    """K = 3 with the third population's nInd >= minind everywhere: trio (0,1,2) counts exactly the sites pair (0,1) counts, and
    f3_i + f3_j is Σ[(p_0 - p_1)^2 - h_0 - h_1] up to rounding: asum of pair (0,1) of pgt_fst_hudson_pops_reduce_dev on the same
    columns, within the bound of both rows (1e-9 A + 1e-12 each, A of the two f3 sums added: it dominates Hudson's Σ|term|)."""
    n, k = 2 * 8192 + 700, 3
    rng = np.random.default_rng(3550)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    c[2] = np.maximum(c[2], MININD).astype(np.int32)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    for name, win in [("one site", one_site_table(n))] + tables_for(pgt, pos, run_lengths(chr_ids)):
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
        out, _, _ = ctx.fst_hudson_pops_reduce_dev(tp, tf, tn, MININD, windows_to_device(win, _dev()), tot=False)
        hud = rows_from_device(out, FST_ROW_DTYPE)[: 3 * win.size].reshape(3, win.size)[0]  # pair (0, 1)
        _, _, A, _ = f3_pops_model.model(pos, f, c, MININD, win)
        assert np.array_equal(rows[0]["n"], hud["n"]) and np.any(hud["n"] > 0), name
        e = excess(rows[0]["f3_i"] + rows[0]["f3_j"], hud["asum"], A["f3_i"][0] + A["f3_j"][0])
        print(f"{name}: f3_i + f3_j against Hudson's asum, excess over the bound {e:.3e}")
        assert e <= 0.0, (name, e)


# ---- trio isolation and reproducibility ------------------------------------------------------------------------------------------
def test_trios_do_not_see_the_other_populations_and_calls_repeat(pgt, ctx):
    n, k = 2 * 8192 + 700, 6
    rng = np.random.default_rng(3650)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, c = random_pops(rng, n, k)
    f2, c2 = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), W, S) for W, S in ((7, 3), (5000, 1000))])
    tp = _t(pos)
    rows, tot = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    again, again_t = pops_dev(ctx, tp, [_t(x) for x in f], [_t(x) for x in c], MININD, win)
    assert again.tobytes() == rows.tobytes() and again_t.tobytes() == tot.tobytes()  # two calls give the same bits
    # trio (0,1,2) of the K = 6 call has the bits of the K = 3 call on those columns — and so has every other trio
    for t, sel in enumerate(all_trio_order(k)):
        if t in (0, 7, 19):
            three, three_t = pops_dev(ctx, tp, [_t(f[x]) for x in sel], [_t(c[x]) for x in sel], MININD, win)
            rows_equal(np.ascontiguousarray(rows[t]), three[0], f"trio {sel} of the K = 6 call against the K = 3 call")
            assert three_t[0]["neff"] == tot[t]["neff"] and three_t[0]["nskip"] == tot[t]["nskip"]
    for r in (0, 3, 5):  # population r replaced: every trio without it keeps its bits
        fr, cr = list(f), list(c)
        fr[r], cr[r] = f2[r], c2[r]
        got, got_t = pops_dev(ctx, tp, [_t(x) for x in fr], [_t(x) for x in cr], MININD, win)
        kept = 0
        for t, ijk in enumerate(all_trio_order(k)):
            if r not in ijk:
                rows_equal(np.ascontiguousarray(got[t]), np.ascontiguousarray(rows[t]), f"population {r} replaced, trio {ijk}")
                assert got_t[t].tobytes() == tot[t].tobytes()
                kept += 1
            else:
                assert got[t].tobytes() != rows[t].tobytes()
        assert kept == n_trios(k - 1)


def test_uncounted_sites_may_hold_anything(pgt, ctx):
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(3750)
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
    for t in range(n_trios(k)):
        rows_equal(np.ascontiguousarray(wild[t]), np.ascontiguousarray(tame[t]), f"trio {t}: wild values at uncounted sites")
        assert all(np.all(np.isfinite(wild[t][s])) for s in SUMS)
    assert wild_t.tobytes() == tame_t.tobytes()


# ---- workspace contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(513, 3), (8193, 6), (600_001, 4)])
def test_rows_under_every_hint_poison_and_guard(pgt, ctx, n, k):
    W = 550_000 if n > 100_000 else 5000
    rng = np.random.default_rng(3850 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    fb, cb = random_pops(rng, n, k)
    win = np.concatenate([pgt.build_windows_sites(run_lengths(chr_ids), min(W, n), max(1, min(W, n) // 4)),
                          pgt.build_windows_sites(run_lengths(chr_ids), min(1000, n), min(333, n))])
    want, want_t, A, A_tot = f3_pops_model.model(pos, f, c, MININD, win)
    dev = _dev()
    tf, tn = [padded_column(x, float("nan"), dev) for x in f], [padded_column(x, 1000, dev) for x in c]
    tp, wd = _t(pos), windows_to_device(win, dev)
    T = n_trios(k)
    tb = ctx.f3_pops_tree_bytes(k, n)
    _, _, foreign = ctx.f3_pops_reduce_dev(tp, [_t(x) for x in fb], [_t(x) for x in cb], MININD, wd)
    g = GuardedBuffers([tb, T * win.size * F3_ROW_DTYPE.itemsize, T * F3_TOTAL_DTYPE.itemsize], 43 + k, dev)
    tree, out, tot = g.bufs
    for hint in (0, W, 50_000):  # 50 000: at 600 001 sites too small a hint, the level-3 windows answered from level 2
        first = None
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):
                poison_tree(tree, kind, other=foreign)
                out.fill_(0xFF)
                tot.fill_(0xFF)
                ctx.f3_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
                what = f"n={n} K={k} hint={hint} poison={kind}"
                g.check(what)
                got = rows_from_device(out, F3_ROW_DTYPE).reshape(T, win.size).copy()
                got_t = rows_from_device(tot, F3_TOTAL_DTYPE).copy()
                if first is None:
                    first = (got, got_t)
                    for t in range(T):
                        assert_rows(got[t], want[t], A, t, what + f" trio {t}")
                    assert_totals(got_t, want_t, A_tot, what)
                else:  # identical under one hint, whatever the workspace held
                    assert got.tobytes() == first[0].tobytes() and got_t.tobytes() == first[1].tobytes(), what


def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    import torch
    n, k = 2 * 8192 + 700, 4
    rng = np.random.default_rng(3950)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    A_, B_ = random_pops(rng, n, k), random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 100)
    dev = _dev()
    wd, tp = windows_to_device(win, dev), _t(pos)
    tf, tn = [_t(x) for x in A_[0]], [_t(x) for x in A_[1]]
    T = n_trios(k)
    g = GuardedBuffers([ctx.f3_pops_tree_bytes(k, n), T * win.size * F3_ROW_DTYPE.itemsize, T * F3_TOTAL_DTYPE.itemsize], 3, dev)
    tree, out, tot = g.bufs
    with ctx.hints(5000, 100, 0):
        ctx.f3_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # one call on one stream: a chain of kernels, no parallel branches
            ctx.f3_pops_reduce_dev(tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree)
    for name, src in (("B", B_), ("A", A_)):
        for t, x in zip(tf + tn, src[0] + src[1]):
            t.copy_(torch.from_numpy(x))
        for buf in (tree, out, tot):
            buf.fill_(0xFF)
        graph.replay()
        g.check("f3_pops graph replay")
        want, want_t, A, A_tot = f3_pops_model.model(pos, src[0], src[1], MININD, win)
        got = rows_from_device(out, F3_ROW_DTYPE).reshape(T, win.size)
        for t in range(T):
            assert_rows(got[t], want[t], A, t, f"replay {name} trio {t}")
        assert_totals(rows_from_device(tot, F3_TOTAL_DTYPE), want_t, A_tot, f"replay {name}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(pgt, ctx):
    import torch
    n, k = 10_000, 3
    rng = np.random.default_rng(4050)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 1000, 500)
    wd = windows_to_device(win, _dev())
    T = 1
    tb = ctx.f3_pops_tree_bytes(k, n)
    g = GuardedBuffers([tb, T * win.size * F3_ROW_DTYPE.itemsize, T * F3_TOTAL_DTYPE.itemsize], 5, _dev())
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
        return lib.pgt_f3_pops_reduce_dev(h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, n, minind, win_p, win.size,
                                          out_p, out_bytes, tot.data_ptr(), tree_p, tree_bytes, None)

    fp, npp = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    refusals = [
        (dict(minind=0), "minind must be at least 1"), (dict(minind=-3), "minind"),
        (dict(pos_p=None), "pos"), (dict(freq_null=True), "freq"), (dict(nind_null=True), "nind"), (dict(tree_p=None), "tree"), (dict(win_p=None), "win"),
        (dict(out_p=None), "out"), (dict(n_pops=2), "n_pops must be 3 ... 6"), (dict(n_pops=7), "n_pops must be 3 ... 6"), (dict(n_pops=0), "n_pops"),
        (dict(freq=[fp[0], None, fp[2]]), "freq[1]"), (dict(nind=[npp[0], npp[1], None]), "nind[2]"),
        (dict(freq=[fp[0], fp[1] + 8, fp[2]]), "freq[1] is not 16-byte aligned"), (dict(nind=[npp[0], npp[1], npp[2] + 8]), "nind[2]"),
        (dict(nind=[npp[0] + 4, npp[1], npp[2]]), "nind[0]"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(tree_bytes=tb - 1), "tree_bytes"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f3_pops_reduce: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    want, _, A, _ = f3_pops_model.model(pos, f, c, MININD, win)
    assert_rows(rows_from_device(out, F3_ROW_DTYPE).reshape(T, win.size)[0], want[0], A, 0, "accepted call", quiet=False)

    # the host-buffer form refuses in the same words and returns before any upload
    rows_h, tot_h = np.zeros(win.size, dtype=F3_ROW_DTYPE), np.zeros(1, dtype=F3_TOTAL_DTYPE)
    hf = (C.c_void_p * 8)(*([x.ctypes.data for x in f] + [None] * 5))
    hn = (C.c_void_p * 8)(*([x.ctypes.data for x in c] + [None] * 5))
    for n_pops, minind, name in ((2, MININD, "n_pops must be 3 ... 6"), (7, MININD, "n_pops must be 3 ... 6"), (3, 0, "minind must be at least 1")):
        rc = lib.pgt_f3_pops_reduce(h, pos.ctypes.data, hf, hn, n_pops, n, minind, win.ctypes.data, win.size, rows_h.ctypes.data, tot_h.ctypes.data)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f3_pops_reduce: "), (n_pops, minind, msg)
    assert not rows_h.view(np.uint8).any() and not tot_h.view(np.uint8).any()

    # the Python wrappers refuse the population count by name
    with pytest.raises(_lib.PgtError, match="f3_pops_reduce_dev: 3 ... 6 populations"):
        ctx.f3_pops_reduce_dev(tp, tf[:2], tn[:2], 1, wd)
    with pytest.raises(_lib.PgtError, match="3 ... 6 populations"):
        ctx.f3_pops_reduce(pos, f * 3, c * 3, MININD, win)
    with pytest.raises(_lib.PgtError, match="minind"):
        ctx.f3_pops_reduce_dev(tp, tf, tn, 0, wd)
    torch.cuda.synchronize()


# ---- host-buffer form -----------------------------------------------------------------------------------------------------------
def test_host_buffer_form_equals_the_device_form_twice_in_a_row(pgt, ctx):
    n, k = 2 * 8192 + 700, 4
    for seed in (83, 84):  # different data through the one context: nothing of the cached workspace may survive
        rng = np.random.default_rng(seed)
        chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
        f, c = random_pops(rng, n, k)
        win = pgt.build_windows_sites(run_lengths(chr_ids), 5000, 1000)
        rows, tot = ctx.f3_pops_reduce(pos, f, c, MININD, win)
        hints = pgt.window_scan.table_hints(win)
        with ctx.hints(hints[0], 0, 0):  # the host-buffer form derives the longest-window hint from the table
            want, want_t = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], MININD, win)
        assert rows.shape == want.shape == (4, win.size)
        for t in range(rows.shape[0]):
            rows_equal(np.ascontiguousarray(rows[t]), np.ascontiguousarray(want[t]), f"seed {seed} trio {t}")
        assert tot.tobytes() == want_t.tobytes()
    res = pgt.f3_window_pops(chr_ids, pos, f, c, 5000, 1000, MININD, 1, ctx=ctx)
    assert list(res) == pgt.all_trio_order(k) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    for t, ijk in enumerate(pgt.all_trio_order(k)):
        rows_equal(np.ascontiguousarray(res[ijk].rows), np.ascontiguousarray(want[t]), f"f3_window_pops trio {ijk}")
        assert res[ijk].total.tobytes() == want_t[t].tobytes()
    # -skip_missing drops a trio's rows without counted sites from that trio alone
    c0 = [x.copy() for x in c]
    c0[1][:6000] = 0
    full = pgt.f3_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, ctx=ctx)
    kept = pgt.f3_window_pops(chr_ids, pos, f, c0, 5000, 1000, MININD, 1, skip_missing=1, ctx=ctx)
    assert np.any(full[(0, 1, 2)].rows["n"] == 0)
    assert kept[(0, 1, 2)].rows.size == np.count_nonzero(full[(0, 1, 2)].rows["n"]) < full[(0, 1, 2)].rows.size
    assert kept[(0, 2, 3)].rows.size == np.count_nonzero(full[(0, 2, 3)].rows["n"]) > kept[(0, 1, 2)].rows.size
    # jackknife=True on disjoint windows: the same rows, and the items of the device jackknife on them
    plain = pgt.f3_window_pops(chr_ids, pos, f, c, 5000, 5000, MININD, 1, ctx=ctx)
    jk = pgt.f3_window_pops(chr_ids, pos, f, c, 5000, 5000, MININD, 1, jackknife=True, ctx=ctx)
    assert set(jk) == set(plain) | {"jackknife"} and list(jk["jackknife"]) == pgt.all_trio_order(k)
    for ijk in pgt.all_trio_order(k):
        rows_equal(np.ascontiguousarray(jk[ijk].rows), np.ascontiguousarray(plain[ijk].rows), f"jackknife=True rows of trio {ijk}")
        host = ctx.f3_jackknife(plain[ijk].rows[None, :])[0]
        assert host.tobytes() == jk["jackknife"][ijk].tobytes()
        assert jk["jackknife"][ijk]["n_blocks"][0] == np.count_nonzero(plain[ijk].rows["n"])
