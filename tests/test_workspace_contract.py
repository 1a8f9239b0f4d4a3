"""GPU: what the device reductions READ and WRITE besides their inputs and rows.

The parity tests check values; these check the workspace contract of every *_dev entry point (and of the host-buffer path,
whose workspace the context caches):

  * nothing the tree workspace held before the call reaches the rows — it is poisoned three ways (0xFF bytes, the fully
    built tree of a different dataset of the same size, zeros) under every hint, so a query that reads a level the build
    skipped (pgt_set_max_window) shows;
  * nothing outside the buffers a call was given changes — tree, out and tot lie between seeded guards (helpers.GuardedBuffers);
  * nothing outside [0, n) of a column is read — columns are views into padding that would show (NaN for f64 values, 1000
    for the count columns, 1 for genotypes, 1e300 for scores);
  * on dyadic data (synth.exact_*: every partial sum exact in any order) every strategy gives the SAME bits, equal to integer
    prefix sums — where the parity tests can only compare strategies to 1e-9, a site dropped or counted twice shows here.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import synth
from helpers import GuardedBuffers, padded_column, poison_tree, rows_equal
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import (DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, EXT_ROW_DTYPE, FST_ROW_DTYPE, HET_ROW_DTYPE, PGT_STAT_DXY,
                                       PGT_STAT_EXT, PGT_STAT_FST, PGT_STAT_HET, WIN_DTYPE)
from popgenomicstools_amd.window_scan import rows_from_device, table_hints, windows_to_device

pytestmark = pytest.mark.gpu

UNIT = synth.EXACT_UNIT
MININD = 5
POS_PAD = 2_000_000_000  # in range of a position, never an address
SIZES = [1, 127, 129, 511, 513, 8191, 8193, 65535, 65537, 500_003, 1_600_001]  # 1.6e6: f64 trees with level-3 nodes


def _dev():
    import torch
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------
# data and exact expectations
# ---------------------------------------------------------------------------------------------------------------------------
class Data:
    """One exact dataset of n sites (host columns + their padded device views, made on first use)."""

    def __init__(self, seed, n, layout):
        self.n = n
        self.chr_ids, self.pos = synth.chromosomes(np.random.default_rng(layout), n, min(3, n), equal=False)
        rng = np.random.default_rng(seed)
        self.run_len = np.diff(np.concatenate(([0], np.flatnonzero(np.diff(self.chr_ids)) + 1, [n]))).astype(np.uint64)
        self.a, self.b, self.ka, self.kb = synth.exact_fst_columns(rng, n)
        self.p1, self.p2, self.n1, self.n2, self.k1, self.k2 = synth.exact_dxy_columns(rng, n)
        self.g = synth.het_column(rng, n).astype(np.int8)
        self.score = synth.tied_scores(rng, n)
        self.freqs, self.kf = synth.exact_freq_columns(rng, n, 8)
        self._t = {}

    def t(self, name, fill=None):
        """padded device view of a column"""
        key = (name, fill)
        if key not in self._t:
            x = {"pos": self.pos.view(np.int32)}.get(name)
            if x is None:
                x = getattr(self, name)
            if fill is None:
                fill = {"pos": POS_PAD, "n1": 1000, "n2": 1000, "g": 1}.get(name, float("nan"))
            self._t[key] = padded_column(x, fill, _dev())
        return self._t[key]

    def freq_t(self, k):
        key = ("freq", k)
        if key not in self._t:
            self._t[key] = padded_column(self.freqs[k], float("nan"), _dev())
        return self._t[key]

    @functools.cached_property
    def prefix(self):
        P = lambda x: np.concatenate(([0], np.cumsum(x, dtype=np.int64)))  # noqa: E731
        keep = (self.n1 >= MININD) & (self.n2 >= MININD)
        d = self.k1 * (1024 - self.k2) + self.k2 * (1024 - self.k1)  # units of 2^-20
        return {"a": P(self.ka), "b": P(self.kb), "nm": P(self.g >= 0), "nh": P(self.g == 1), "d": P(np.where(keep, d, 0)),
                "neff": P(keep), "nskip": P(~keep)}


@functools.lru_cache(maxsize=8)
def data(seed, n, layout=0):
    """datasets of the same n and layout share their positions and chromosome runs (one window table serves them)"""
    return Data(seed, n, layout)


def _lohi(win):
    return win["lo"].astype(np.int64), win["hi"].astype(np.int64)


def coords(pos, win):
    """start / end of every row: the table's where PGT_WIN_COORDS is set, else pos[lo], pos[hi - 1] (0 for an empty window)"""
    lo, hi = _lohi(win)
    some = hi > lo
    start = np.where(some, pos[np.minimum(lo, pos.size - 1)], 0).astype(np.uint32)
    end = np.where(some, pos[np.maximum(hi - 1, 0)], 0).astype(np.uint32)
    given = (win["flags"] & _lib.PGT_WIN_COORDS) != 0
    return np.where(given, win["start"], start), np.where(given, win["end"], end)


def wsum(P, win):
    lo, hi = _lohi(win)
    return P[hi] - P[lo]


def ratio(x, y):
    return np.divide(x, y, out=np.zeros_like(x), where=y != 0)


def fst_expect(d, win):
    r = np.zeros(win.size, FST_ROW_DTYPE)
    r["start"], r["end"] = coords(d.pos, win)
    r["mid"] = ((r["start"].astype(np.uint64) + r["end"]) & 0xFFFFFFFF) // 2
    r["n"] = win["hi"] - win["lo"]
    r["asum"] = wsum(d.prefix["a"], win).astype(np.float64) * synth.FST_UNIT
    r["bsum"] = wsum(d.prefix["b"], win).astype(np.float64) * synth.FST_UNIT
    r["fst"] = ratio(r["asum"], r["bsum"])
    return r


def het_expect(d, win, g=None):
    P = lambda x: np.concatenate(([0], np.cumsum(x, dtype=np.int64)))  # noqa: E731
    r = np.zeros(win.size, HET_ROW_DTYPE)
    r["start"], r["end"] = coords(d.pos, win)
    r["mid"] = ((r["start"].astype(np.uint64) + r["end"]) & 0xFFFFFFFF) // 2
    r["nonmissing"] = wsum(d.prefix["nm"] if g is None else P(g >= 0), win)
    r["nhet"] = wsum(d.prefix["nh"] if g is None else P(g == 1), win)
    r["h"] = ratio(r["nhet"].astype(np.float64), r["nonmissing"].astype(np.float64))
    return r


def dxy_expect(d, win):
    r = np.zeros(win.size, DXY_ROW_DTYPE)
    r["start"], r["end"] = coords(d.pos, win)
    r["neff"] = wsum(d.prefix["neff"], win)
    r["nskip"] = wsum(d.prefix["nskip"], win)
    r["sum"] = wsum(d.prefix["d"], win).astype(np.float64) * UNIT
    t = np.zeros(1, DXY_TOTAL_DTYPE)
    t["sum"] = float(d.prefix["d"][-1]) * UNIT
    t["neff"], t["nskip"] = d.prefix["neff"][-1], d.prefix["nskip"][-1]
    return r, t


def ext_key(score, mode):
    return np.abs(score) if mode == _lib.PGT_EXT_IHS else (score if mode == _lib.PGT_EXT_XP_MAX else -score)


def ext_expect(d, win, mode, cutoff):
    key = ext_key(d.score, mode)
    thr = -cutoff if mode == _lib.PGT_EXT_XP_MIN else cutoff  # xpehh below a negative cutoff: s < cutoff, i.e. -s > -cutoff
    big = np.concatenate(([0], np.cumsum(key > thr, dtype=np.int64)))
    r = np.zeros(win.size, EXT_ROW_DTYPE)
    r["start"], r["end"] = coords(d.pos, win)
    r["nsites"] = win["hi"] - win["lo"]
    r["nbig"] = wsum(big, win)
    for w, (lo, hi) in enumerate(zip(*_lohi(win))):
        if hi > lo:
            i = lo + int(np.argmax(key[lo:hi]))  # the first site attaining the maximum
            r["position"][w], r["value"][w] = d.pos[i], d.score[i]
    return r


def af_pairs(n_pops):
    return [(i, j) for i in range(n_pops) for j in range(i + 1, n_pops)]


def af_expect(d, win, n_pops, nsamp):
    """Σ2f(1-f) and Σ(f_i-f_j)^2 exact, then the kernel's closing formula (pgt_af_kernels.hip) in the same IEEE operations."""
    P = lambda x: np.concatenate(([0], np.cumsum(x, dtype=np.int64)))  # noqa: E731
    A = [wsum(P(2 * k * (1024 - k)), win).astype(np.float64) * UNIT for k in d.kf[:n_pops]]
    start, end = coords(d.pos, win)
    rows = []
    for i, j in af_pairs(n_pops):
        D = wsum(P((d.kf[i] - d.kf[j]) ** 2), win).astype(np.float64) * UNIT
        ni, nj = nsamp[i], nsamp[j]
        npool = ni + nj
        sb = (ni * A[i] + nj * A[j]) / (npool - 1.0)
        sa = D - sb * (npool / (4.0 * ni * nj))
        r = np.zeros(win.size, FST_ROW_DTYPE)
        r["start"], r["end"] = start, end
        r["mid"] = ((start.astype(np.uint64) + end) & 0xFFFFFFFF) // 2
        r["n"] = win["hi"] - win["lo"]
        r["asum"] = sa + 0.0
        r["bsum"] = (sa + sb) + 0.0
        r["fst"] = ratio(r["asum"], r["bsum"])
        rows.append(r)
    return np.stack(rows)


def af_rational_check(d, win, n_pops, nsamp, rows, max_windows=48):
    """The rows of (at most four) pairs against WCFst's window sums in exact rationals: betaAFOutlier.R:400-418 site by site for
    windows of up to 512 sites, the kernel header's closed form Σb = (n_i A_i + n_j A_j)/(npool-1), Σa = D_ij - Σb npool/(4 n_i n_j) on the exact sums
    for longer ones — within a few ulp of the component's scale, on a sample of windows that includes the first and the last."""
    idx = np.unique(np.linspace(0, win.size - 1, min(win.size, max_windows)).astype(np.int64))
    P = lambda x: np.concatenate(([0], np.cumsum(x, dtype=np.int64)))  # noqa: E731
    PA = [P(2 * k * (1024 - k)) for k in d.kf[:n_pops]]
    pairs = af_pairs(n_pops)
    for p in sorted({0, 1 % len(pairs), len(pairs) // 2, len(pairs) - 1}):
        i, j = pairs[p]
        ni, nj = Fraction(nsamp[i]), Fraction(nsamp[j])
        npool = ni + nj
        PD = P((d.kf[i] - d.kf[j]) ** 2)
        for w in idx:
            lo, hi = int(win["lo"][w]), int(win["hi"][w])
            if hi - lo <= 512:
                sa = sb = Fraction(0)
                for ki, kj in zip(d.kf[i][lo:hi].tolist(), d.kf[j][lo:hi].tolist()):
                    f1, f2 = Fraction(ki, 1024), Fraction(kj, 1024)
                    fpool = ni / npool * f1 + nj / npool * f2
                    b = (ni * 2 * f1 * (1 - f1) + nj * 2 * f2 * (1 - f2)) / (npool - 1)
                    sa += (4 * ni * (f1 - fpool) ** 2 + 4 * nj * (f2 - fpool) ** 2 - b) / (4 * ni * nj / npool)
                    sb += b
                scale = max(abs(sa), abs(sb))
            else:
                Ai, Aj = Fraction(int(PA[i][hi] - PA[i][lo]), 2 ** 20), Fraction(int(PA[j][hi] - PA[j][lo]), 2 ** 20)
                D = Fraction(int(PD[hi] - PD[lo]), 2 ** 20)
                sb = (ni * Ai + nj * Aj) / (npool - 1)
                sa = D - sb * npool / (4 * ni * nj)
                scale = max(abs(D), abs(sb * npool / (4 * ni * nj)), abs(sb))
            tol = 8 * 2.0 ** -52 * float(scale)
            r = rows[p][w]
            assert abs(float(r["asum"]) - float(sa)) <= tol, (p, w, float(r["asum"]), float(sa))
            assert abs(float(r["bsum"]) - float(sa + sb)) <= tol, (p, w, float(r["bsum"]), float(sa + sb))


# ---------------------------------------------------------------------------------------------------------------------------
# window tables and hints
# ---------------------------------------------------------------------------------------------------------------------------
def span_table(n, long_lengths=()):
    """Windows starting and ending on and next to multiples of 16, 128, 512, 1024, 8192 and 65536, in the column's last 16
    sites, of length 0 and 1 (the span recipe of test_fast_query_paths_equal_the_general_path_at_their_edges)."""
    edges = set()
    for m in (16, 128, 512, 1024, 8192, 65536):
        for k in (1, 2, 3, 7, n // m - 1, n // m):
            for dd in (-1, 0, 1):
                edges.add(k * m + dd)
    edges |= set(range(n - 16, n + 1)) | {0, 1, 15, 17}
    edges = sorted(e for e in edges if 0 <= e <= n)
    spans = set()
    for lo in edges:
        for length in (0, 1, 15, 16, 17, 127, 129, 511, 513, 1023, 1025, 8191, 8193, 49_999, 65_535, 65_536, 70_000) + tuple(long_lengths):
            if lo + length <= n:
                spans.add((lo, lo + length))
    for hi in edges:
        for length in (1, 16, 1000, 50_000):
            if hi - length >= 0:
                spans.add((hi - length, hi))
    spans = sorted(spans)
    win = np.zeros(len(spans), dtype=WIN_DTYPE)
    win["lo"] = [s[0] for s in spans]
    win["hi"] = [s[1] for s in spans]
    return win


def tables(pgt, d):
    """(name, host table, hint variants) for dataset d.  Hint variants: (max_window, step, typical) — none, the exact (W, S), a
    max-window hint that is too small, one much larger than W; bp tables also their typical length."""
    n = d.n
    out = []
    site = [(50_000, 10_000), (50_000, 100), (20_000, 777), (20_000, 33)]
    if n <= 600_000:
        site += [(300, 1), (5_000, 7)]  # per-window, group (with and without shared edge scans), sliding
    else:
        site += [(600_000, 150_000)]      # windows with level-3 nodes
    for W, S in site:
        out.append((f"sites W={W} S={S}", pgt.build_windows_sites(d.run_len, W, S),
                    [(0, 0, 0), (W, S, 0), (max(1, W // 4), S, 0), (64 * W, S, 0)]))
    ends = np.cumsum(d.run_len).astype(np.int64) - 1
    chr_len = (d.pos[ends].astype(np.int64) + 1000).astype(np.uint32)
    bp = pgt.build_windows_bp(d.pos, d.run_len, chr_len, 100_000, 25_000)
    mw, typ, st = table_hints(bp)
    st = 0 if st >= 2 ** 63 else st
    out.append(("bp W=100000 S=25000", bp, [(0, 0, 0), (mw, st, typ), (max(1, mw // 4), st, 0), (64 * mw, st, typ)]))
    out.append(("spans", span_table(n, (600_000,) if n > 600_000 else ()),
                [(0, 0, 0), (70_000, 1, 0), (65_536, 0, 0), (50_000, 1, 0), (5_000_000, 7, 0)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# one guarded, poisoned call per entry point
# ---------------------------------------------------------------------------------------------------------------------------
_other_trees = {}


def other_tree(key, build):
    """The fully built tree (no hints) of a different dataset of the same size: poison 2."""
    if key not in _other_trees:
        if len(_other_trees) > 16:
            _other_trees.clear()
        _other_trees[key] = build()
    return _other_trees[key]


def run_fst(ctx, d, win, wd, poison, other, seed):
    g = GuardedBuffers([ctx.tree_bytes(PGT_STAT_FST, d.n), win.size * FST_ROW_DTYPE.itemsize], seed, _dev())
    tree, out = g.bufs
    poison_tree(tree, poison, other)
    out.fill_(0xFF)
    ctx.fst_reduce_dev(d.t("pos"), d.t("a"), d.t("b"), wd, out=out, tree=tree)
    g.check("fst_reduce_dev")
    return rows_from_device(out, FST_ROW_DTYPE), tree


def run_het(ctx, d, win, wd, poison, other, seed):
    g = GuardedBuffers([ctx.tree_bytes(PGT_STAT_HET, d.n), win.size * HET_ROW_DTYPE.itemsize], seed, _dev())
    tree, out = g.bufs
    poison_tree(tree, poison, other)
    out.fill_(0xFF)
    ctx.het_reduce_dev(d.t("pos"), d.t("g"), wd, out=out, tree=tree)
    g.check("het_reduce_dev")
    return rows_from_device(out, HET_ROW_DTYPE), tree


def run_dxy(ctx, d, win, wd, poison, other, seed, with_tot=True):
    g = GuardedBuffers([ctx.tree_bytes(PGT_STAT_DXY, d.n), win.size * DXY_ROW_DTYPE.itemsize, DXY_TOTAL_DTYPE.itemsize], seed, _dev())
    tree, out, tot = g.bufs
    poison_tree(tree, poison, other)
    out.fill_(0xFF)
    tot.fill_(0xFF)
    ctx.dxy_reduce_dev(d.t("pos"), d.t("p1"), d.t("p2"), d.t("n1"), d.t("n2"), MININD, wd, out=out,
                       tot=tot if with_tot else False, tree=tree)
    g.check("dxy_reduce_dev")
    t = rows_from_device(tot, DXY_TOTAL_DTYPE)
    if not with_tot:
        assert tot.cpu().numpy().tobytes() == b"\xff" * DXY_TOTAL_DTYPE.itemsize  # tot=NULL: nothing written there
    return rows_from_device(out, DXY_ROW_DTYPE), t, tree


def check_three_statistics(pgt, ctx, d, other_d, name, win, hint_list, k0, oracle=None, site_wS=None):
    """fst, het and dxy rows of one table under every hint, the poison rotating with the hint (pairwise, not a cross product)."""
    wd = windows_to_device(win, _dev())
    want_f, want_h = fst_expect(d, win), het_expect(d, win)
    want_d, want_t = dxy_expect(d, win)
    if oracle is not None and site_wS is not None:  # the data premise: on exact data the oracle's sequential sums are these bits too
        W, S = site_wS
        ref = oracle.fst_scan(d.chr_ids, d.pos, d.a, d.b, W, S)
        assert ref.size == win.size
        assert np.array_equal(ref["num"], want_f["asum"]) and np.array_equal(ref["den"], want_f["bsum"])
        assert np.array_equal(ref["value"], want_f["fst"])
        ref = oracle.het_scan(d.chr_ids, d.pos, d.g, W, S)
        assert np.array_equal(ref["n"], want_h["nonmissing"]) and np.array_equal(ref["value"], want_h["h"])
        ref, rtot = oracle.dxy_scan(d.chr_ids, d.pos, d.p1, d.p2, d.n1, d.n2, W, S, MININD, 1, 0)
        assert np.array_equal(ref["value"], want_d["sum"]) and np.array_equal(ref["n"], want_d["neff"])
        assert float(rtot["sum"]) == float(want_t["sum"][0]) and int(rtot["neff"]) == int(want_t["neff"][0])
    others = {}
    for h, (mw, st, typ) in enumerate(hint_list):
        poison = (k0 + h) % 3
        if poison == 1 and not others:
            with ctx.hints(0, 0, 0):
                others["fst"] = other_tree(("fst", d.n, other_d.n), lambda: run_fst(ctx, other_d, win, wd, 2, None, 1)[1].clone())
                others["het"] = other_tree(("het", d.n, other_d.n), lambda: run_het(ctx, other_d, win, wd, 2, None, 2)[1].clone())
                others["dxy"] = other_tree(("dxy", d.n, other_d.n), lambda: run_dxy(ctx, other_d, win, wd, 2, None, 3)[2].clone())
        what = f"n={d.n} {name} hints={(mw, st, typ)} poison={poison}"
        with ctx.hints(mw, st, typ):
            rows, _ = run_fst(ctx, d, win, wd, poison, others.get("fst"), 10 + h)
            rows_equal(rows, want_f, "fst " + what)
            rows, _ = run_het(ctx, d, win, wd, poison, others.get("het"), 20 + h)
            rows_equal(rows, want_h, "het " + what)
            rows, tot, _ = run_dxy(ctx, d, win, wd, poison, others.get("dxy"), 30 + h, with_tot=(h % 2 == 0))
            rows_equal(rows, want_d, "dxy " + what)
            if h % 2 == 0:
                assert tot.tobytes() == want_t.tobytes(), ("dxy total, bit for bit", what, tot, want_t)


# ---------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_fst_het_dxy_rows_are_exact_whatever_the_workspace_held(pgt, ctx, oracle, n):
    """fst_reduce_dev / het_reduce_dev / dxy_reduce_dev (with and without the genome-wide total) on exact data: every table
    (per-window, group with and without shared edge scans, sliding, long windows, bp windows, hand-made spans at every node
    boundary), every hint, every poison — the rows of integer prefix sums bit for bit, no guard byte touched."""
    d, other = data(1, n), data(2, n)
    for k, (name, win, hint_list) in enumerate(tables(pgt, d)):
        site_wS = None
        if name.startswith("sites") and (n <= 65537 or k == 0):
            site_wS = tuple(int(x.split("=")[1]) for x in name.split()[1:])
        check_three_statistics(pgt, ctx, d, other, name, win, hint_list, k, oracle, site_wS)


def test_genotype_tree_with_level_3_nodes(pgt, ctx):
    """het_reduce_dev at 9e6 sites (the int8 tree's level 3: 4.2e6-site nodes) with windows that contain them, and the hinted
    builds that skip its level 2 (W < 65536) on a poisoned workspace."""
    n = 9_000_017
    d, other = data(3, n), data(4, n)
    wins = [("sites W=5000000 S=1000000", pgt.build_windows_sites(d.run_len, 5_000_000, 1_000_000),
             [(0, 0, 0), (5_000_000, 1_000_000, 0), (50_000, 1_000_000, 0), (5_000_000, 100, 0)]),
            ("sites W=50000 S=10000", pgt.build_windows_sites(d.run_len, 50_000, 10_000),
             [(50_000, 10_000, 0), (50_000, 100, 0), (0, 0, 0)]),
            ("spans", span_table(n, (4_300_000, 8_500_000)), [(70_000, 1, 0), (0, 0, 0), (65_535, 0, 0)])]
    for k, (name, win, hint_list) in enumerate(wins):
        wd = windows_to_device(win, _dev())
        want = het_expect(d, win)
        with ctx.hints(0, 0, 0):
            full = run_het(ctx, other, win, wd, 2, None, 5)[1].clone()
        for h, (mw, st, typ) in enumerate(hint_list):
            poison = (k + h) % 3
            with ctx.hints(mw, st, typ):
                rows, _ = run_het(ctx, d, win, wd, poison, full, 40 + h)
            rows_equal(rows, want, f"het n={n} {name} hints={(mw, st, typ)} poison={poison}")


@pytest.mark.parametrize("n_pairs", [2, 33])
def test_batched_pairs_rows_are_exact(pgt, ctx, n_pairs):
    """fst_reduce_pairs_dev: 2 pairs, and 33 (two launch batches, each with its own tree region) — every pair's rows exact under
    every poison and hint, nothing written outside the n_pairs trees and the rows."""
    n = 65_537 if n_pairs == 33 else 500_003
    ds = [data(10 + s, n) for s in range(3)]  # one layout: one position column serves every pair
    win = pgt.build_windows_sites(ds[0].run_len, 20_000, 33) if n_pairs == 2 else span_table(n)
    wd = windows_to_device(win, _dev())
    wants = [fst_expect(d, win) for d in ds]
    tb = ctx.tree_bytes(PGT_STAT_FST, n)

    def call(shift, poison, other, seed):
        g = GuardedBuffers([n_pairs * tb, n_pairs * win.size * FST_ROW_DTYPE.itemsize], seed, _dev())
        tree, out = g.bufs
        poison_tree(tree, poison, other)
        out.fill_(0xFF)
        sel = [ds[(p + shift) % 3] for p in range(n_pairs)]
        ctx.fst_reduce_pairs_dev(ds[0].t("pos"), [s.t("a") for s in sel], [s.t("b") for s in sel], wd, out=out, tree=tree)
        g.check(f"fst_reduce_pairs_dev n_pairs={n_pairs}")
        return rows_from_device(out, FST_ROW_DTYPE).reshape(n_pairs, win.size), tree

    with ctx.hints(0, 0, 0):
        other = call(1, 2, None, 1)[1].clone()
    for h, hint in enumerate([(0, 0, 0), (20_000, 33, 0), (5_000, 33, 0), (70_000, 1, 0), (1_000_000, 777, 0)]):
        poison = h % 3
        with ctx.hints(*hint):
            rows, _ = call(0, poison, other, 10 + h)
        for p in range(n_pairs):
            rows_equal(rows[p], wants[p % 3], f"pair {p} of {n_pairs} hints={hint} poison={poison}")


@pytest.mark.parametrize("n", [129, 8193, 65_537, 500_003])
def test_fused_dxy_het_rows_are_exact(pgt, ctx, n):
    """pgt_dxy_het_reduce_dev (the C entry point: its wrapper allocates the outputs itself): the combined tree poisoned, the
    four outputs guarded, the rows those of the exact expectation."""
    import torch
    lib = _lib.load()
    d, other_d = data(5, n), data(6, n)
    d2 = data(7, n)  # the second genotype column
    g2 = padded_column(d2.g, 1, _dev())
    tree_bytes = ctx.tree_bytes(PGT_STAT_DXY, n) + 2 * ctx.tree_bytes(PGT_STAT_HET, n)
    for k, (name, win, hint_list) in enumerate(tables(pgt, d)):
        if n > 8193 and name not in ("spans", "sites W=50000 S=100", "sites W=20000 S=33"):
            continue
        wd = windows_to_device(win, _dev())
        want_d, want_t = dxy_expect(d, win)
        want_h1, want_h2 = het_expect(d, win), het_expect(d, win, d2.g)

        def call(cols, poison, other, seed):
            g = GuardedBuffers([tree_bytes, win.size * DXY_ROW_DTYPE.itemsize, DXY_TOTAL_DTYPE.itemsize,
                                win.size * HET_ROW_DTYPE.itemsize, win.size * HET_ROW_DTYPE.itemsize], seed, _dev())
            tree, out, tot, h1, h2 = g.bufs
            poison_tree(tree, poison, other)
            for b in (out, tot, h1, h2):
                b.fill_(0xFF)
            rc = lib.pgt_dxy_het_reduce_dev(ctx._ctx, cols.t("pos").data_ptr(), cols.t("p1").data_ptr(), cols.t("p2").data_ptr(),
                                            cols.t("n1").data_ptr(), cols.t("n2").data_ptr(), cols.t("g").data_ptr(), g2.data_ptr(),
                                            n, MININD, wd.data_ptr(), win.size, out.data_ptr(), out.numel(), tot.data_ptr(),
                                            h1.data_ptr(), h2.data_ptr(), h1.numel(), tree.data_ptr(), tree.numel(), None)
            assert rc == _lib.PGT_OK, lib.pgt_last_error(ctx._ctx)
            g.check("dxy_het_reduce_dev")
            return [rows_from_device(x, dt) for x, dt in ((out, DXY_ROW_DTYPE), (tot, DXY_TOTAL_DTYPE), (h1, HET_ROW_DTYPE),
                                                            (h2, HET_ROW_DTYPE))], tree

        with ctx.hints(0, 0, 0):
            other = call(other_d, 2, None, 1)[1].clone()
        for h, hint in enumerate(hint_list):
            poison = (k + h) % 3
            what = f"n={n} {name} hints={hint} poison={poison}"
            with ctx.hints(*hint):
                (rd, rt, r1, r2), _ = call(d, poison, other, 10 + h)
            rows_equal(rd, want_d, "fused dxy " + what)
            assert rt.tobytes() == want_t.tobytes(), ("fused dxy total", what)
            rows_equal(r1, want_h1, "fused het 1 " + what)
            rows_equal(r2, want_h2, "fused het 2 " + what)
        torch.cuda.synchronize()


@pytest.mark.parametrize("n_pops,n", [(2, 1), (2, 511), (2, 500_003), (3, 513), (3, 65_537), (4, 513), (5, 8193), (6, 65_537), (7, 8193), (8, 8193), (8, 1_600_001)])
def test_af_front_end_rows_are_exact(pgt, ctx, n_pops, n):
    """fst_af_reduce_dev with every NP in 2 ... 8 (each is its own instantiation of the reduce-scatter): exact frequency columns make the window sums exact, so every strategy, hint and
    poison gives the same bytes — those of the kernel's closing formula on the exact sums, and within a few ulp of the
    component's scale of WCFst evaluated in rationals."""
    d, other_d = data(8, n), data(9, n)
    nsamp = [12.0, 20.0, 7.0, 33.0, 9.0, 15.0, 40.0, 5.0][:n_pops]
    tb = int(_lib.load().pgt_af_tree_bytes(n_pops, n))
    n_pairs = n_pops * (n_pops - 1) // 2
    checked = False
    for k, (name, win, hint_list) in enumerate(tables(pgt, d)):
        if n > 65_537 and not (name.startswith("spans") or "S=33" in name or "150000" in name or "S=10000" in name):
            continue
        wd = windows_to_device(win, _dev())
        want = af_expect(d, win, n_pops, nsamp)

        def call(cols, poison, other, seed):
            g = GuardedBuffers([tb, n_pairs * win.size * FST_ROW_DTYPE.itemsize], seed, _dev())
            tree, out = g.bufs
            poison_tree(tree, poison, other)
            out.fill_(0xFF)
            ctx.fst_af_reduce_dev(cols.t("pos"), [cols.freq_t(q) for q in range(n_pops)], nsamp, wd, out=out, tree=tree)
            g.check(f"fst_af_reduce_dev NP={n_pops}")
            return rows_from_device(out, FST_ROW_DTYPE).reshape(n_pairs, win.size), tree

        with ctx.hints(0, 0, 0):
            other = call(other_d, 2, None, 1)[1].clone()
        for h, hint in enumerate(hint_list):
            poison = (k + h) % 3
            with ctx.hints(*hint):
                rows, _ = call(d, poison, other, 10 + h)
            for p in range(n_pairs):
                rows_equal(rows[p], want[p], f"AF NP={n_pops} pair {p} n={n} {name} hints={hint} poison={poison}")
        if not checked or name.startswith("spans"):
            af_rational_check(d, win, n_pops, nsamp, want, max_windows=12 if n_pops == 8 else 24)
            checked = True


@pytest.mark.parametrize("n", [1, 127, 129, 511, 513, 8193, 65_537, 500_003, 1_600_001])
def test_extreme_rows_are_exact(pgt, ctx, n):
    """extreme_reduce_dev in ihs and xpehh modes (ties included): value, position, nbig and nsites equal a numpy max / first
    argmax / count over [lo, hi); the tree poisoned with nodes that would win any maximum they enter (never 0xFF bytes: the
    query dereferences pos[node.idx]) and the score padding +-1e300, so a stale node or a read outside the column shows."""
    d, other_d = data(11, n), data(12, n)
    ends = np.cumsum(d.run_len).astype(np.int64) - 1
    chr_len = (d.pos[ends].astype(np.int64) + 5000).astype(np.uint32)
    wins = []
    for W in (100_000, 1_000_000, 40_000_000):
        win = pgt.build_windows_extreme(d.pos, d.run_len, chr_len if W != 1_000_000 else None, W)
        mw, typ, st = table_hints(win)
        st = 0 if st >= 2 ** 63 else st
        wins.append((f"extreme W={W}", win, [(0, 0, 0), (mw, st, typ), (max(1, mw // 4), st, 0)]))
    wins.append(("spans", span_table(n, (1_100_000,) if n > 1_100_000 else ()), [(0, 0, 0), (70_000, 1, 0), (65_536, 0, 0)]))
    tb = ctx.tree_bytes(PGT_STAT_EXT, n)
    for mode, cutoff in ((_lib.PGT_EXT_IHS, 2.0), (_lib.PGT_EXT_XP_MAX, 2.0), (_lib.PGT_EXT_XP_MIN, -2.0)):
        score = d.t("score", -1e300 if mode == _lib.PGT_EXT_XP_MIN else 1e300)
        oscore = other_d.t("score", 1e300)

        def call(pos, s, wd, nwin, poison, other, seed):
            g = GuardedBuffers([tb, nwin * EXT_ROW_DTYPE.itemsize], seed, _dev())
            tree, out = g.bufs
            poison_tree(tree, poison, other, ext=True)
            out.fill_(0xFF)
            ctx.extreme_reduce_dev(pos, s, mode, cutoff, wd, out=out, tree=tree)
            g.check(f"extreme_reduce_dev mode={mode}")
            return rows_from_device(out, EXT_ROW_DTYPE), tree

        for k, (name, win, hint_list) in enumerate(wins):
            wd = windows_to_device(win, _dev())
            want = ext_expect(d, win, mode, cutoff)
            with ctx.hints(0, 0, 0):
                other = call(other_d.t("pos"), oscore, wd, win.size, 2, None, 1)[1].clone()
            for h, hint in enumerate(hint_list):
                poison = (k + h + mode) % 3
                with ctx.hints(*hint):
                    rows, _ = call(d.t("pos"), score, wd, win.size, poison, other, 10 + h)
                rows_equal(rows, want, f"extreme mode={mode} n={n} {name} hints={hint} poison={poison}")


def test_graph_replay_rebuilds_from_new_columns(pgt, ctx):
    """A captured build + query (hints set at capture, one stream) replayed after the columns were overwritten in place with
    another exact dataset and the tree filled with 0xFF: every replay gives that dataset's exact rows (fst and dxy)."""
    import torch
    n = 500_003
    A, B = data(13, n), data(14, n)
    win = pgt.build_windows_sites(A.run_len, 50_000, 100)
    wd = windows_to_device(win, _dev())
    cols = {c: padded_column(getattr(A, c), {"n1": 1000, "n2": 1000}.get(c, float("nan")), _dev())
            for c in ("a", "b", "p1", "p2", "n1", "n2")}
    tp = A.t("pos")
    gf = GuardedBuffers([ctx.tree_bytes(PGT_STAT_FST, n), win.size * FST_ROW_DTYPE.itemsize], 1, _dev())
    gd = GuardedBuffers([ctx.tree_bytes(PGT_STAT_DXY, n), win.size * DXY_ROW_DTYPE.itemsize, DXY_TOTAL_DTYPE.itemsize], 2, _dev())
    ftree, fout = gf.bufs
    dtree, dout, dtot = gd.bufs
    with ctx.hints(50_000, 100, 0):
        ctx.fst_reduce_dev(tp, cols["a"], cols["b"], wd, out=fout, tree=ftree)  # warm-up outside the capture
        ctx.dxy_reduce_dev(tp, cols["p1"], cols["p2"], cols["n1"], cols["n2"], MININD, wd, out=dout, tot=dtot, tree=dtree)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.fst_reduce_dev(tp, cols["a"], cols["b"], wd, out=fout, tree=ftree)
            ctx.dxy_reduce_dev(tp, cols["p1"], cols["p2"], cols["n1"], cols["n2"], MININD, wd, out=dout, tot=dtot, tree=dtree)
    for src in (B, A, B):
        for c, t in cols.items():
            t.copy_(torch.from_numpy(getattr(src, c)))
        for buf in (ftree, dtree, fout, dout, dtot):
            buf.fill_(0xFF)
        g.replay()
        gf.check("fst graph replay")
        gd.check("dxy graph replay")
        rows_equal(rows_from_device(fout, FST_ROW_DTYPE), fst_expect(src, win), "fst replay")
        want_d, want_t = dxy_expect(src, win)
        rows_equal(rows_from_device(dout, DXY_ROW_DTYPE), want_d, "dxy replay")
        assert rows_from_device(dtot, DXY_TOTAL_DTYPE).tobytes() == want_t.tobytes()


def test_host_buffer_path_never_answers_from_the_cached_workspace(pgt, ctx):
    """The host-buffer entry points keep a per-context workspace that a test cannot poison: two different exact datasets of the
    same size alternate through fst / het / dxy / extreme_reduce and the *_reduce_tab calls over a device-built table, under
    every hint state, then a large call is followed by a small one — every result is its own dataset's exact rows."""
    n = 300_001
    A, B = data(15, n), data(16, n)
    win = pgt.build_windows_sites(A.run_len, 20_000, 33)
    ewin = pgt.build_windows_extreme(A.pos, A.run_len, None, 200_000)
    tab = ctx.window_table_sites(A.run_len, 5_000, 7)
    twin = pgt.build_windows_sites(A.run_len, 5_000, 7)
    try:
        for hint in [(0, 0, 0), (20_000, 33, 0), (5_000, 33, 0), (1_500_000, 7, 0)]:
            with ctx.hints(*hint):
                for d in (A, B, A):
                    what = f"hints={hint} seed-dataset {d is A}"
                    rows_equal(ctx.fst_reduce(d.pos, d.a, d.b, win), fst_expect(d, win), "fst_reduce " + what)
                    rows_equal(ctx.het_reduce(d.pos, d.g, win), het_expect(d, win), "het_reduce " + what)
                    rows, tot = ctx.dxy_reduce(d.pos, d.p1, d.p2, d.n1, d.n2, MININD, win)
                    want, want_t = dxy_expect(d, win)
                    rows_equal(rows, want, "dxy_reduce " + what)
                    assert np.array([tot]).tobytes() == want_t.tobytes(), what
                    rows_equal(ctx.extreme_reduce(d.pos, d.score, _lib.PGT_EXT_IHS, 2.0, ewin),
                               ext_expect(d, ewin, _lib.PGT_EXT_IHS, 2.0), "extreme_reduce " + what)
                    rows_equal(ctx.fst_reduce_tab(d.pos, d.a, d.b, tab), fst_expect(d, twin), "fst_reduce_tab " + what)
                    rows_equal(ctx.het_reduce_tab(d.pos, d.g, tab), het_expect(d, twin), "het_reduce_tab " + what)
                    rows, tot = ctx.dxy_reduce_tab(d.pos, d.p1, d.p2, d.n1, d.n2, MININD, tab)
                    want, want_t = dxy_expect(d, twin)
                    rows_equal(rows, want, "dxy_reduce_tab " + what)
                    assert np.array([tot]).tobytes() == want_t.tobytes(), what
    finally:
        tab.free()
    big, small = data(17, 2_000_003), data(18, 1_001)
    for d in (big, small, big, small):
        w = pgt.build_windows_sites(d.run_len, 50_000, 1_000)
        rows_equal(ctx.fst_reduce(d.pos, d.a, d.b, w), fst_expect(d, w), f"fst_reduce n={d.n}")
        rows_equal(ctx.het_reduce(d.pos, d.g, w), het_expect(d, w), f"het_reduce n={d.n}")
        rows, tot = ctx.dxy_reduce(d.pos, d.p1, d.p2, d.n1, d.n2, MININD, w)
        want, want_t = dxy_expect(d, w)
        rows_equal(rows, want, f"dxy_reduce n={d.n}")
        assert np.array([tot]).tobytes() == want_t.tobytes()
        ew = pgt.build_windows_extreme(d.pos, d.run_len, None, 300_000)
        rows_equal(ctx.extreme_reduce(d.pos, d.score, _lib.PGT_EXT_XP_MIN, -2.0, ew),
                   ext_expect(d, ew, _lib.PGT_EXT_XP_MIN, -2.0), f"extreme_reduce n={d.n}")
