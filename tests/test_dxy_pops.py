"""GPU: dxy of all population pairs from per-population columns (pgt_dxy_pops_reduce_dev / pgt_dxy_pops_reduce).

The yardsticks are the two-population path (Context.dxy_reduce_dev on each pair's columns), the CPU restatement
(oracle.dxy_scan on each pair's columns), the hand-walked / known-answer fixtures and integer prefix sums of exact data —
never the code under test."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import synth
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, WIN_DTYPE
from popgenomicstools_amd.window_scan import pair_order, rows_from_device, run_lengths, windows_to_device

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x).to(_dev())


def random_pops(rng, n, k):
    """6-decimal frequencies, counts 0 .. 20 (tests/synth.dxy_columns, per population)"""
    return [np.round(rng.uniform(0, 1, n), 6) for _ in range(k)], [rng.integers(0, 21, n, dtype=np.int32) for _ in range(k)]


def pops_dev(ctx, tp, tf, tn, minind, win, **kw):
    """-> (rows[n_pairs, n_win], totals[n_pairs] or None) of one dxy_pops_reduce_dev call"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.dxy_pops_reduce_dev(tp, tf, tn, minind, wd, **kw)
    n_pairs = len(tf) * (len(tf) - 1) // 2
    rows = rows_from_device(out, DXY_ROW_DTYPE)[: n_pairs * win.size].reshape(n_pairs, win.size)
    return rows, (rows_from_device(tot, DXY_TOTAL_DTYPE)[:n_pairs] if tot is not None else None)


def pair_dev(ctx, tp, tf, tn, i, j, minind, win):
    """the parent's two-population path on pair (i, j)"""
    wd = windows_to_device(win, _dev())
    out, tot, _ = ctx.dxy_reduce_dev(tp, tf[i], tf[j], tn[i], tn[j], minind, wd)
    return rows_from_device(out, DXY_ROW_DTYPE)[: win.size], rows_from_device(tot, DXY_TOTAL_DTYPE)[0]


def worst_excess(x, y):
    """max over all entries of |x - y| - (REL |y| + ABS) (<= 0: every entry within the project's standing bound) and the
    largest relative difference"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.size == 0:
        return -1.0, 0.0
    d = np.abs(x - y)
    rel = float(np.max(d / np.maximum(np.abs(y), 1e-300)))
    return float(np.max(d - (helpers.REL * np.abs(y) + helpers.ABS))), rel


# ---- 3: per-site bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
def test_per_site_rows_carry_the_pair_paths_bits(pgt, ctx, k):
    """-fixedsite 1 -winsize 1 -stepsize 1: every row of every pair is bit for bit the two-population path's."""
    rng = np.random.default_rng(100 + k)
    n = 20_011
    chr_ids, pos = synth.chromosomes(rng, n, 2)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), 1, 1)
    assert win.size == n
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    for minind in (1, 5):
        rows, tot = pops_dev(ctx, tp, tf, tn, minind, win)
        for p, (i, j) in enumerate(pair_order(k)):
            want, want_t = pair_dev(ctx, tp, tf, tn, i, j, minind, win)
            rows_equal(rows[p], want, f"K={k} minind={minind} pair {(i, j)}")
            assert int(tot[p]["neff"]) == int(want_t["neff"]) and int(tot[p]["nskip"]) == int(want_t["nskip"])


# ---- 4: against the pair path and the oracle, any table ---------------------------------------------------------------------
SIZES = [1, 127, 128, 129, 511, 513, 8191, 8192, 8193, 65537, 300_017, 8192 * 64 + 15, 1_600_001]
SITE_TABLES = [(1, 1), (50, 7), (1000, 1000), (50_000, 10_000)]


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_rows_against_the_pair_path_and_the_oracle(pgt, ctx, oracle, k):
    """Every K crossed with every size; per (K, size) ALL four site tables and one base-pair table (W = 2000 bp, S = 500 bp:
    about 67 sites per window); 1 - 4 chromosomes (cycled with the size's index, so every count meets every K; with two or
    more the site tables contain the Q1 carry windows); BOTH minind values, 1 and 5, on every (K, size, table).  EVERY row of
    EVERY pair is compared: coordinates and counts exactly, sums by |x - y| <= 1e-9 |y| + 1e-12 against BOTH references, the genome-wide lines included.
    Largest relative difference seen on an MI355X: profiles/r07/dxy_pops.md."""
    worst = 0.0
    for si, n in enumerate(SIZES):
        rng = np.random.default_rng(1000 * k + si)
        n_chr = min(1 + (si + k) % 4, n)
        chr_ids, pos = synth.chromosomes(rng, n, n_chr, equal=False)
        rl = run_lengths(chr_ids)
        f, c = random_pops(rng, n, k)
        tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
        ends = np.cumsum(rl).astype(np.int64)
        chr_len = (pos[ends - 1].astype(np.int64) + 17).astype(np.uint32)
        tables = [("site", W, S) for W, S in SITE_TABLES] + [("bp", 2000, 500)]
        for ti, (kind, W, S) in enumerate(tables):
            fixed = 1 if kind == "site" else 0
            win = pgt.build_windows_sites(rl, W, S) if fixed else pgt.build_windows_bp(pos, rl, chr_len, W, S)
            for minind in (1, 5):
                rows, tot = pops_dev(ctx, tp, tf, tn, minind, win)
                for p, (i, j) in enumerate(pair_order(k)):
                    what = f"K={k} n={n} {kind} W={W} S={S} minind={minind} pair {(i, j)}"
                    want, want_t = pair_dev(ctx, tp, tf, tn, i, j, minind, win)
                    ref, rtot = oracle.dxy_scan(chr_ids, pos, f[i], f[j], c[i], c[j], W, S, minind, fixed, 0, None if fixed else chr_len)
                    ref = ref[ref["printed"] == 1]
                    got = rows[p]
                    assert got.size == want.size == ref.size, what
                    for fld in ("start", "end", "neff", "nskip"):
                        assert np.array_equal(got[fld], want[fld]), (what, fld)
                    assert np.array_equal(got["start"], ref["start"]) and np.array_equal(got["end"], ref["end"]), what
                    assert np.array_equal(got["neff"], ref["n"]) and np.array_equal(got["nskip"], ref["nskip"]), what
                    for name, y in (("pair path", want["sum"]), ("oracle", ref["value"])):
                        excess, rel = worst_excess(got["sum"], y)
                        worst = max(worst, rel)
                        assert excess <= 0.0, (what, name, excess, rel)
                    assert int(tot[p]["neff"]) == int(want_t["neff"]) == int(rtot["neff"]), what
                    assert int(tot[p]["nskip"]) == int(want_t["nskip"]) == int(rtot["nskip"]), what
                    for name, y in (("pair path", want_t["sum"]), ("oracle", rtot["sum"])):
                        excess, rel = worst_excess([tot[p]["sum"]], [y])
                        worst = max(worst, rel)
                        assert excess <= 0.0, (what, "total", name, excess, rel)
    print(f"\ndxy_pops K={k}: largest relative difference of a sum against either reference = {worst:.3e}")


# ---- 5: fixtures ------------------------------------------------------------------------------------------------------------
def _lines(names, res):
    lines = "".join(f"{names[int(w['label_run'])]}\t{int(r['start'])}\t{int(r['end'])}\t{helpers.fmt_g(r['sum'])}\t{int(r['neff'])}\t{int(r['nskip'])}\n"
                    for w, r in zip(res.win, res.rows))
    total = f"{helpers.fmt_g(res.total['sum'])}\t{int(res.total['neff'])}\t{int(res.total['nskip'])}\n"
    return lines, total


def _kat_columns():
    k = helpers.load_golden("dxy_kat.json")
    names = [r[0] for r in k["sizes"]]
    chr_ids = np.array([names.index(r[0]) for r in k["pop1"]], dtype=np.uint32)
    pos = np.array([r[1] for r in k["pop1"]], dtype=np.uint32)
    p1 = np.array([r[2] for r in k["pop1"]]); n1 = np.array([r[3] for r in k["pop1"]], dtype=np.int32)
    p2 = np.array([r[2] for r in k["pop2"]]); n2 = np.array([r[3] for r in k["pop2"]], dtype=np.int32)
    chr_len = np.array([r[1] for r in k["sizes"]], dtype=np.uint32)
    return k, names, chr_ids, pos, p1, p2, n1, n2, chr_len


def test_two_populations_reproduce_the_known_answers(pgt, ctx):
    k, names, chr_ids, pos, p1, p2, n1, n2, chr_len = _kat_columns()
    for c in k["cases"]:
        res = pgt.dxy_window_pops(chr_ids, pos, [p1, p2], [n1, n2], c["winsize"], c["stepsize"], k["minind"], c["fixedsite"],
                                  chr_len, c["skip_missing"], ctx=ctx)
        assert list(res) == [(0, 1)]
        lines, total = _lines(names, res[(0, 1)])
        if c["winsize"] == 0:
            assert total == c["stdout"] and lines == ""
        else:
            assert lines == c["stdout"] and total == c["stderr"]


def test_two_populations_reproduce_the_hand_walked_cases(pgt, ctx):
    k = helpers.load_golden("dxy_hand_walked.json")
    done = 0
    for c in k["cases"]:
        names = []
        for r in c["pop1"]:
            if not names or names[-1] != r[0]:
                names.append(r[0])
        key2 = {(r[0], r[1]): r for r in c["pop2"]}
        both = [(r, key2[(r[0], r[1])]) for r in c["pop1"] if (r[0], r[1]) in key2]
        if not both:
            continue
        chr_ids = np.array([names.index(a[0]) for a, _ in both], dtype=np.uint32)
        pos = np.array([a[1] for a, _ in both], dtype=np.uint32)
        p1 = np.array([a[2] for a, _ in both]); n1 = np.array([a[3] for a, _ in both], dtype=np.int32)
        p2 = np.array([b[2] for _, b in both]); n2 = np.array([b[3] for _, b in both], dtype=np.int32)
        sizes = dict(c["sizes"] or [])
        for r in c["runs"]:
            want_out, want_err = helpers.hand_walked_product_expectation(c, r)
            chr_len = None if r["fixedsite"] else np.array([sizes[nm] for nm in names], dtype=np.uint32)
            res = pgt.dxy_window_pops(chr_ids, pos, [p1, p2], [n1, n2], r["winsize"], r["stepsize"], c["minind"], r["fixedsite"],
                                      chr_len, r["skip_missing"], ctx=ctx)
            lines, total = _lines(names, res[(0, 1)])
            if r["winsize"] == 0:
                assert total == want_out and lines == "", c["name"]
            else:
                assert lines == want_out, (c["name"], r, lines)
                assert total == want_err, (c["name"], r, total)
            done += 1
    assert done >= 11


def test_a_copied_population_gives_equal_pairs_and_the_heterozygosity_sum(pgt, ctx):
    """K = 3 with population 2 a copy of population 0: pairs (0,1) and (1,2) are the same sites and the same two products
    (added in the other order: an addition commutes bit for bit); pair (0,2) is Σ 2p(1-p) over population 0's counted sites."""
    k, names, chr_ids, pos, p1, p2, n1, n2, chr_len = _kat_columns()
    for c in k["cases"]:
        if c["winsize"] == 0 or c["skip_missing"]:
            continue
        res = pgt.dxy_window_pops(chr_ids, pos, [p1, p2, p1.copy()], [n1, n2, n1.copy()], c["winsize"], c["stepsize"], k["minind"],
                                  c["fixedsite"], chr_len, 0, ctx=ctx)
        rows_equal(res[(0, 1)].rows, res[(1, 2)].rows, "pairs (0,1) and (1,2)")
        assert np.array([res[(0, 1)].total]).tobytes() == np.array([res[(1, 2)].total]).tobytes()
        h = np.where(n1 >= k["minind"], 2.0 * p1 * (1.0 - p1), 0.0)
        for w, r in zip(res[(0, 2)].win, res[(0, 2)].rows):
            lo, hi = int(w["lo"]), int(w["hi"])
            assert int(r["neff"]) == int((n1[lo:hi] >= k["minind"]).sum()) and int(r["nskip"]) == hi - lo - int(r["neff"])
            assert helpers.close(float(r["sum"]), math.fsum(h[lo:hi])), (c, lo, hi)


# ---- 6: exact data ----------------------------------------------------------------------------------------------------------
class ExactPops:
    """frequencies k/1024 and counts 0 .. 20: d = (k_i (1024 - k_j) + k_j (1024 - k_i)) 2^-20 exactly, every partial sum of
    fewer than 2^30 sites exact in f64 in any order — rows are integer prefix sums, bit for bit"""

    def __init__(self, seed, n, k, n_chr=3, minind=5):
        rng = np.random.default_rng(seed)
        self.n, self.k, self.minind = n, k, minind
        self.chr_ids, self.pos = synth.chromosomes(rng, n, min(n_chr, n), equal=False)
        self.run_len = run_lengths(self.chr_ids)
        self.f, self.ks = synth.exact_freq_columns(rng, n, k)
        self.c = [rng.integers(0, 21, n, dtype=np.int32) for _ in range(k)]
        self.pre_d, self.pre_n = [], []
        for i, j in pair_order(k):
            ok = (self.c[i] >= minind) & (self.c[j] >= minind)
            d = np.where(ok, self.ks[i] * (1024 - self.ks[j]) + self.ks[j] * (1024 - self.ks[i]), 0)
            self.pre_d.append(np.concatenate(([0], np.cumsum(d))))
            self.pre_n.append(np.concatenate(([0], np.cumsum(ok.astype(np.int64)))))

    def expect(self, win):
        lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
        rows = np.zeros((len(self.pre_d), win.size), dtype=DXY_ROW_DTYPE)
        tot = np.zeros(len(self.pre_d), dtype=DXY_TOTAL_DTYPE)
        for p in range(len(self.pre_d)):
            rows[p]["start"] = self.pos[np.minimum(lo, self.n - 1)]
            rows[p]["end"] = self.pos[np.maximum(hi, 1) - 1]
            rows[p]["neff"] = self.pre_n[p][hi] - self.pre_n[p][lo]
            rows[p]["nskip"] = (hi - lo) - (self.pre_n[p][hi] - self.pre_n[p][lo])
            rows[p]["sum"] = (self.pre_d[p][hi] - self.pre_d[p][lo]).astype(np.float64) * synth.EXACT_UNIT
            tot[p]["sum"] = float(self.pre_d[p][-1]) * synth.EXACT_UNIT
            tot[p]["neff"] = self.pre_n[p][-1]
            tot[p]["nskip"] = self.n - self.pre_n[p][-1]
        return rows, tot

    def padded(self):
        dev = _dev()
        return [padded_column(x, float("nan"), dev) for x in self.f], [padded_column(x, 1000, dev) for x in self.c]


LEVEL3 = 8192 * 64  # sites of a level-3 node


def _contains_level3_node(win):
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    return (-(-lo // LEVEL3)) < (hi // LEVEL3)


def _exact_table(pgt, d, W):
    """windows of W sites (step W/4) and short ones beside them by the tools' rules, and — where the size has level-3 nodes
    (524 288 sites) — explicit ranges that CONTAIN one, two and all of them with ragged ends on every level below (a table is
    any list of ranges; these cross chromosome boundaries, which the reduction does not look at)"""
    parts = [pgt.build_windows_sites(d.run_len, max(1, min(W, d.n)), max(1, min(W, d.n) // 4)),
             pgt.build_windows_sites(d.run_len, max(1, min(1000, d.n)), max(1, min(333, d.n)))]
    extra = [(LEVEL3 - 7, 2 * LEVEL3 + 13), (LEVEL3, 2 * LEVEL3), (LEVEL3 - 100, 3 * LEVEL3 + 5), (0, 3 * LEVEL3), (0, d.n),
             (700, 2 * LEVEL3 + 8192 + 513), (2 * LEVEL3 - 8192 * 3 - 129, d.n - 1)]
    extra = [(lo, hi) for lo, hi in extra if 0 <= lo < hi <= d.n]
    if extra:
        e = np.zeros(len(extra), dtype=WIN_DTYPE)
        e["lo"], e["hi"] = [x[0] for x in extra], [x[1] for x in extra]
        parts.append(e)
    return np.concatenate(parts)


@pytest.mark.parametrize("n,k", [(1, 2), (513, 3), (513, 6), (8193, 7), (8193, 8), (65_537, 5), (300_017, 4), (1_600_001, 8)])
def test_exact_rows_under_every_hint_poison_and_guard(pgt, ctx, n, k):
    """Rows and totals of every pair equal the integer prefix sums BITWISE: under the hints 0 / W / 4 W, with the tree
    workspace poisoned three ways before every call, tree / out / tot between seeded guards, and the columns as views into
    padding that would show (NaN frequencies, counts of 1000).  At 1 600 001 sites the table holds windows that contain one,
    two and all three level-3 nodes (asserted below): under the hints 0 / W / 4 W level 3 is built by pops_up_kernel and
    read by the query; under the fourth hint (50 000: no level above 2) the same windows are answered from level 2."""
    W = 600_000
    A, B = ExactPops(21 + k, n, k), ExactPops(22 + k, n, k)
    win = _exact_table(pgt, A, W)
    if n >= 3 * LEVEL3:
        assert int(_contains_level3_node(win).sum()) >= 5, "the table must contain level-3 nodes"
    want, want_t = A.expect(win)
    tf, tn = A.padded()
    tp = _t(A.pos)
    n_pairs = k * (k - 1) // 2
    tb = ctx.dxy_pops_tree_bytes(k, n)
    # a foreign tree: fully built from another dataset of the same size
    wd = windows_to_device(win, _dev())
    _, _, foreign = ctx.dxy_pops_reduce_dev(_t(B.pos), [_t(x) for x in B.f], [_t(x) for x in B.c], B.minind, wd)
    g = GuardedBuffers([tb, n_pairs * win.size * DXY_ROW_DTYPE.itemsize, n_pairs * DXY_TOTAL_DTYPE.itemsize], 31 + k, _dev())
    tree, out, tot = g.bufs
    for hint in (0, W, 4 * W, 50_000):
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):
                poison_tree(tree, kind, other=foreign)
                out.fill_(0xFF)
                tot.fill_(0xFF)
                ctx.dxy_pops_reduce_dev(tp, tf, tn, A.minind, wd, out=out, tot=tot, tree=tree)
                what = f"n={n} K={k} hint={hint} poison={kind}"
                g.check(what)
                got = rows_from_device(out, DXY_ROW_DTYPE).reshape(n_pairs, win.size)
                for p in range(n_pairs):
                    rows_equal(got[p], want[p], what + f" pair {p}")
                assert rows_from_device(tot, DXY_TOTAL_DTYPE).tobytes() == want_t.tobytes(), what


# ---- 7: totals on random data -----------------------------------------------------------------------------------------------
def test_genome_wide_lines_are_pinned_to_the_exact_sums(pgt, ctx):
    rng = np.random.default_rng(77)
    n, k, minind = 1_000_003, 4, 5
    chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
    f, c = random_pops(rng, n, k)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    win = pgt.build_windows_sites(run_lengths(chr_ids), 50_000, 10_000)
    _, t1 = pops_dev(ctx, tp, tf, tn, minind, win)
    _, t2 = pops_dev(ctx, tp, tf, tn, minind, win)
    _, t3 = pops_dev(ctx, tp, tf, tn, minind, np.zeros(0, dtype=WIN_DTYPE))  # the global-only form
    assert t1.tobytes() == t2.tobytes() == t3.tobytes()
    for p, (i, j) in enumerate(pair_order(k)):
        ok = (c[i] >= minind) & (c[j] >= minind)
        d = f[i] * (1.0 - f[j]) + f[j] * (1.0 - f[i])  # numpy f64: the same three roundings per site as the device
        exact = math.fsum(d[ok])
        assert int(t1[p]["neff"]) == int(ok.sum()) and int(t1[p]["nskip"]) == n - int(ok.sum())
        assert abs(float(t1[p]["sum"]) - exact) <= 1e-13 * exact, (p, float(t1[p]["sum"]), exact)


# ---- 8: shards --------------------------------------------------------------------------------------------------------------
def test_sharded_tables_give_the_single_calls_rows(pgt, ctx):
    rng = np.random.default_rng(88)
    n, k, minind, W, S = 1_600_001, 3, 5, 50_000, 10_000
    chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
    f, c = random_pops(rng, n, k)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, S)
    with ctx.hints(W, S, 0):
        whole, _ = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], minind, win)
        for n_ranks in (2, 3, 8):
            parts = []
            for sh in pgt.plan_shards(win, n_ranks):
                a, b, s0, s1 = int(sh["win_begin"]), int(sh["win_end"]), int(sh["site_lo"]), int(sh["site_hi"])
                w = win[a:b].copy()
                w["lo"] -= s0
                w["hi"] -= s0
                if b > a:
                    assert s0 % 65536 == 0
                    rows, _ = pops_dev(ctx, _t(pos[s0:s1]), [_t(x[s0:s1]) for x in f], [_t(x[s0:s1]) for x in c], minind, w, tot=False)
                else:
                    rows = np.zeros((3, 0), dtype=DXY_ROW_DTYPE)
                parts.append(rows)
            got = np.concatenate(parts, axis=1)
            for p in range(3):
                rows_equal(np.ascontiguousarray(got[p]), whole[p], f"{n_ranks} shards, pair {p}")


# ---- 9: graph capture -------------------------------------------------------------------------------------------------------
def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    import torch
    n, k = 500_003, 4
    A, B = ExactPops(41, n, k), ExactPops(42, n, k)
    win = pgt.build_windows_sites(A.run_len, 50_000, 100)
    wd = windows_to_device(win, _dev())
    tf, tn = A.padded()
    tp = _t(A.pos)
    n_pairs = k * (k - 1) // 2
    g = GuardedBuffers([ctx.dxy_pops_tree_bytes(k, n), n_pairs * win.size * DXY_ROW_DTYPE.itemsize, n_pairs * DXY_TOTAL_DTYPE.itemsize], 3, _dev())
    tree, out, tot = g.bufs
    with ctx.hints(50_000, 100, 0):
        ctx.dxy_pops_reduce_dev(tp, tf, tn, A.minind, wd, out=out, tot=tot, tree=tree)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ctx.dxy_pops_reduce_dev(tp, tf, tn, A.minind, wd, out=out, tot=tot, tree=tree)
    for src in (B, A, B):
        # (A and B share n and the window table; the positions are the capture's: rows carry A's coordinates)
        for t, x in zip(tf + tn, src.f + src.c):
            t.copy_(torch.from_numpy(x))
        for buf in (tree, out, tot):
            buf.fill_(0xFF)
        graph.replay()
        g.check("dxy_pops graph replay")
        want, want_t = src.expect(win)
        want["start"], want["end"] = A.expect(win)[0]["start"], A.expect(win)[0]["end"]
        got = rows_from_device(out, DXY_ROW_DTYPE).reshape(n_pairs, win.size)
        for p in range(n_pairs):
            rows_equal(got[p], want[p], f"replay pair {p}")
        assert rows_from_device(tot, DXY_TOTAL_DTYPE).tobytes() == want_t.tobytes()


# ---- 10: argument checks ----------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(pgt, ctx):
    import torch
    n, k = 10_000, 3
    d = ExactPops(51, n, k)
    win = pgt.build_windows_sites(d.run_len, 1000, 500)
    wd = windows_to_device(win, _dev())
    n_pairs = 3
    tb = ctx.dxy_pops_tree_bytes(k, n)
    g = GuardedBuffers([tb, n_pairs * win.size * DXY_ROW_DTYPE.itemsize, n_pairs * DXY_TOTAL_DTYPE.itemsize], 5, _dev())
    tree, out, tot = g.bufs
    tp, tf, tn = _t(d.pos), [_t(x) for x in d.f], [_t(x) for x in d.c]
    lib, h = ctx._lib, ctx._ctx
    before = [b.clone() for b in g.bufs]

    def call(freq=None, nind=None, n_pops=k, win_p=wd.data_ptr(), out_p=out.data_ptr(), out_bytes=out.numel(), tree_p=tree.data_ptr(),
             tree_bytes=tree.numel(), freq_null=False, nind_null=False, pos_p=tp.data_ptr()):
        fp = [t.data_ptr() for t in tf] if freq is None else freq
        npn = [t.data_ptr() for t in tn] if nind is None else nind
        pf = (C.c_void_p * 8)(*(fp + [None] * (8 - len(fp))))
        pn = (C.c_void_p * 8)(*(npn + [None] * (8 - len(npn))))
        return lib.pgt_dxy_pops_reduce_dev(h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, n, 5, win_p, win.size,
                                           out_p, out_bytes, tot.data_ptr(), tree_p, tree_bytes, None)

    f_ptrs, n_ptrs = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    refusals = [
        (dict(pos_p=None), "pos"), (dict(freq_null=True), "freq"), (dict(nind_null=True), "nind"), (dict(tree_p=None), "tree"), (dict(win_p=None), "win"),
        (dict(out_p=None), "out"), (dict(n_pops=1), "n_pops"), (dict(n_pops=9), "n_pops"),
        (dict(freq=[f_ptrs[0], None, f_ptrs[2]]), "freq[1]"), (dict(nind=[n_ptrs[0], n_ptrs[1], None]), "nind[2]"),
        (dict(freq=[f_ptrs[0], f_ptrs[1] + 8, f_ptrs[2]]), "freq[1]"), (dict(nind=[n_ptrs[0], n_ptrs[1], n_ptrs[2] + 8]), "nind[2]"),
        (dict(nind=[n_ptrs[0] + 4, n_ptrs[1], n_ptrs[2]]), "nind[0]"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(tree_bytes=tb - 1), "tree_bytes"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg, (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    torch.cuda.synchronize()
    want, _ = d.expect(win)
    got = rows_from_device(out, DXY_ROW_DTYPE).reshape(n_pairs, win.size)
    for p in range(n_pairs):
        rows_equal(got[p], want[p], f"accepted call, pair {p}")

    # the Python wrapper refuses misaligned views by name
    m = 1000
    fcols = [torch.zeros(m + 4, dtype=torch.float64, device=_dev()) for _ in range(3)]
    ccols = [torch.ones(m + 4, dtype=torch.int32, device=_dev()) for _ in range(3)]
    posm = torch.arange(1, m + 1, dtype=torch.int32, device=_dev())
    w1 = windows_to_device(pgt.build_windows_sites(np.array([m], np.uint64), 100, 100), _dev())
    good_f, good_c = [t[4:4 + m] for t in fcols], [t[4:4 + m] for t in ccols]
    ctx.dxy_pops_reduce_dev(posm, good_f, good_c, 1, w1)
    with pytest.raises(_lib.PgtError, match=r"freqs\[1\]"):
        ctx.dxy_pops_reduce_dev(posm, [good_f[0], fcols[1][1:1 + m], good_f[2]], good_c, 1, w1)
    with pytest.raises(_lib.PgtError, match=r"ninds\[2\]"):
        ctx.dxy_pops_reduce_dev(posm, good_f, [good_c[0], good_c[1], ccols[2][2:2 + m]], 1, w1)
    with pytest.raises(_lib.PgtError, match="column lengths differ"):
        ctx.dxy_pops_reduce_dev(posm, [good_f[0], good_f[1][:-4], good_f[2]], good_c, 1, w1)
    torch.cuda.synchronize()


# ---- 11: host-buffer form ---------------------------------------------------------------------------------------------------
def test_host_buffer_form_equals_the_device_form_twice_in_a_row(pgt, ctx):
    n, k, minind = 300_017, 4, 5
    for seed in (61, 62):  # different data through the one context: nothing of the cached workspace may survive
        rng = np.random.default_rng(seed)
        chr_ids, pos = synth.chromosomes(rng, n, 4, equal=False)
        f, c = random_pops(rng, n, k)
        win = pgt.build_windows_sites(run_lengths(chr_ids), 20_000, 3_333)
        rows, tot = ctx.dxy_pops_reduce(pos, f, c, minind, win)
        hints = pgt.window_scan.table_hints(win)
        with ctx.hints(hints[0], 0, 0):  # the host-buffer form derives the longest-window hint from the table
            want, want_t = pops_dev(ctx, _t(pos), [_t(x) for x in f], [_t(x) for x in c], minind, win)
        assert rows.shape == want.shape
        for p in range(rows.shape[0]):
            rows_equal(np.ascontiguousarray(rows[p]), want[p], f"seed {seed} pair {p}")
        assert tot.tobytes() == want_t.tobytes()
