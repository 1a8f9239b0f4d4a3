"""GPU: the all-pairs front ends (pgt_dxy_pops_reduce_dev, pgt_fst_pops_reduce_dev, pgt_fst_hudson_pops_reduce_dev,
pgt_dstat_pops_reduce_dev, pgt_fst_af_reduce_dev; pgt_pi_pops_reduce_dev for its build) at the sizes where a build wave walks
a SECOND level-2 tile and a query wave answers a SECOND item — the grid strides every other test leaves at one turn.  The
sizes come from the launch arithmetic restated in tests/pops_grid_shapes.py (tests/test_pops_grid_stride_cpu.py holds it to
the sources).

Section 1: the smallest column that reaches a second round of tiles, with a ragged last tile that is some wave's second; a
table of a few hundred windows that read second-round tiles; the tree poisoned three ways before every call, rows and totals
prefilled with 0xFF, all three buffers between guards, NaN / large-count padding around the columns; hints 0 and 50 000 (too
small for the level-3 window).  Section 2: 270 000 sites and tables of 262 143 / 262 144 / 262 149 windows, with and without
the genome-wide lines.

The yardsticks are never the code under test: the NumPy models (tests/*_model.py; dxy_model below, the definition of
dxyWindow.cpp:381 with x87 prefix sums), the CPU oracle's dxy scan on each pair's columns and, for the allele-frequency front
end, the oracle's WCFst() columns and its fstWindow scan.  All pairs and trios are compared with the full models (no subset).
Bounds: counts, start / end / mid exact; sums within helpers.REL |y| + helpers.ABS; fst and d as the pops modules assert them;
one-site windows bit for bit for dxy, Hudson, dstat and pi; the allele-frequency rows by the bounds of
test_af_front_end_vs_oracle (asum against the scale of bsum, fst within 1e-9).

The table of section 2 departs from "one-site table, then windows of 7 sites" in one respect: 270 000 one-site rows would fill
all 262 149 rows, so the two kinds alternate in blocks (pops_grid_shapes.strided_query_table) and both occur among the
second items.

Measured on an MI355X: the module takes 39 s, nearly all of it the host's models and column generation (at most 5.6 s per
case); the six GPU calls of a case take 1 ... 23 ms together."""
import time

import numpy as np
import pytest

import dstat_pops_model
import fst_hudson_model
import fst_pops_model
import helpers
import pi_pops_model
import pops_grid_shapes as shapes
import synth
import test_dstat_pops
import test_fst_pops
import test_pi_pops
from helpers import GuardedBuffers, padded_column, poison_tree
from popgenomicstools_amd._lib import (DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, FST_ROW_DTYPE,
                                       FST_TOTAL_DTYPE)
from popgenomicstools_amd.window_scan import pair_order, rows_from_device, run_lengths, trio_order, windows_to_device
from test_fst_pops import _dev, _t, excess, random_pops

pytestmark = pytest.mark.gpu

MININD = 5
W_SITES = 50_000   # the site windows of section 1 (W = S), and the too-small hint
HINTS = (0, W_SITES)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def log(msg):
    print(f"[grid stride] {msg}", flush=True)


# ---- references ----------------------------------------------------------------------------------------------------------------
def _coords(pos, win):
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.all(hi > lo) and not np.any(win["flags"] & 1)
    return lo, hi, pos[lo], pos[hi - 1]


def dxy_model(pos, freqs, ninds, minind, win):
    """dxyWindow.cpp:381 per pair: a site counts when both populations have minind individuals and then adds
    d = p_i (1 - p_j) + p_j (1 - p_i), every operation a float64 operation of its own; window sums are differences of x87
    prefix sums, a one-site window is the site's value itself.  -> (rows[n_pairs, n_win], totals[n_pairs])"""
    assert np.finfo(np.longdouble).eps < 2e-19
    lo, hi, start, end = _coords(pos, win)
    pairs = pair_order(len(freqs))
    rows, tot = np.zeros((len(pairs), win.size), dtype=DXY_ROW_DTYPE), np.zeros(len(pairs), dtype=DXY_TOTAL_DTYPE)
    one = hi - lo == 1
    for p, (i, j) in enumerate(pairs):
        ok = (ninds[i] >= minind) & (ninds[j] >= minind)
        v = np.where(ok, freqs[i] * (1.0 - freqs[j]) + freqs[j] * (1.0 - freqs[i]), 0.0)
        ps = np.concatenate(([0], np.cumsum(v.astype(np.longdouble))))
        pn = np.concatenate(([0], np.cumsum(ok.astype(np.int64))))
        r = rows[p]
        r["start"], r["end"] = start, end
        r["neff"] = pn[hi] - pn[lo]
        r["nskip"] = (hi - lo) - (pn[hi] - pn[lo])
        r["sum"] = (ps[hi] - ps[lo]).astype(np.float64)
        r["sum"][one] = v[lo[one]]
        tot[p] = (float(ps[-1]), int(pn[-1]), pos.size - int(pn[-1]))
    return rows, tot


def dstat_model(pos, freqs, ninds, minind, win):
    """tests/dstat_pops_model.py, with the one-site windows set to the sites' own values (a prefix difference rounds them
    again) and d to the stated function of those"""
    rows, tot = dstat_pops_model.model(pos, freqs, ninds, minind, win)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    one = hi - lo == 1
    site = lo[one]
    o = len(freqs) - 1
    for t, (i, j, k) in enumerate(trio_order(len(freqs))):
        ok = dstat_pops_model.counted(ninds, i, j, k, minind)[site]
        for fld, x in zip(test_dstat_pops.SUMS, dstat_pops_model.site_components(freqs[i][site], freqs[j][site], freqs[k][site], freqs[o][site])):
            rows[t][fld][one] = np.where(ok, x, 0.0)
        rows[t]["d"][one] = dstat_pops_model.d_of(rows[t]["abba"][one], rows[t]["baba"][one])
    return rows, tot


def af_model(oracle, pos, freqs, nsamp, win, scan=None):
    """WCFst() per pair by the CPU oracle (a, a + b per site), window sums as differences of x87 prefix sums
    -> rows[n_pairs, n_win]; with scan = (chr_ids, W, S) also the oracle's fstWindow rows (sequential sums) of every pair"""
    lo, hi, start, end = _coords(pos, win)
    pairs = pair_order(len(freqs))
    rows, scans = np.zeros((len(pairs), win.size), dtype=FST_ROW_DTYPE), []
    for p, (i, j) in enumerate(pairs):
        a, ab = oracle.wcfst_columns(freqs[i], freqs[j], nsamp[i], nsamp[j])
        r = rows[p]
        r["start"], r["end"] = start, end
        r["mid"] = ((start.astype(np.uint64) + end.astype(np.uint64)) & 0xFFFFFFFF) // 2
        r["n"] = hi - lo
        for fld, x in (("asum", a), ("bsum", ab)):
            px = np.concatenate(([0], np.cumsum(x.astype(np.longdouble))))
            r[fld] = (px[hi] - px[lo]).astype(np.float64)
            del px
        with np.errstate(all="ignore"):
            r["fst"] = np.where(r["bsum"] != 0, r["asum"] / np.where(r["bsum"] != 0, r["bsum"], 1.0), 0.0)
        if scan is not None:
            scans.append(oracle.fst_scan(scan[0], pos, a, ab, scan[1], scan[2]))
    return rows if scan is None else (rows, scans)


# ---- assertions ------------------------------------------------------------------------------------------------------------------
def assert_one_site_bits(got, want, win, fields, what):
    one = (win["hi"] - win["lo"]) == 1
    assert one.any(), what
    for fld in fields:
        same = bits(got[fld][one]) == bits(want[fld][one])
        assert same.all(), (what, fld, "one-site rows", np.flatnonzero(one)[~same][:4].tolist())


def dxy_assert_rows(got, want, what):
    assert got.size == want.size, what
    for fld in ("start", "end", "neff", "nskip"):
        assert np.array_equal(got[fld], want[fld]), (what, fld, np.flatnonzero(got[fld] != want[fld])[:4].tolist())
    e = excess(got["sum"], want["sum"])
    assert e <= 0.0, (what, "sum", e, np.flatnonzero(~(np.abs(got["sum"] - want["sum"]) <= helpers.REL * np.abs(want["sum"]) + helpers.ABS))[:4].tolist())


def dxy_assert_totals(got, want, what):
    for fld in ("neff", "nskip"):
        assert np.array_equal(got[fld], want[fld]), (what, fld, got[fld], want[fld])
    assert excess(got["sum"], want["sum"]) <= 0.0, (what, got["sum"], want["sum"])


def af_assert_rows(got, want, what):
    """the bounds of test_af_front_end_vs_oracle: Σ(a+b) relative; Σa cancels, so its error and the ratio's are measured
    against Σ(a+b)"""
    assert got.size == want.size, what
    for fld in ("start", "end", "mid", "n"):
        assert np.array_equal(got[fld], want[fld]), (what, fld, np.flatnonzero(got[fld] != want[fld])[:4].tolist())
    assert excess(got["bsum"], want["bsum"]) <= 0.0, (what, "bsum")
    assert np.all(np.abs(got["asum"] - want["asum"]) <= 1e-9 * np.abs(want["bsum"]) + 1e-12), (what, "asum")
    assert np.all(np.abs(got["fst"] - want["fst"]) <= 1e-9), (what, "fst")


def all_of(*checks):
    """run every check and report all that fail: a truncated build shows in the rows AND in the genome-wide lines"""
    failed = []
    for check in checks:
        try:
            check()
        except AssertionError as e:
            failed.append(e)
            log(f"FAILED: {str(e)[:500]}")
    assert not failed, failed


class Stat:
    """what is particular to one entry point: its call, buffers, tables, model and assertions"""

    def __init__(self, name, row, total, order, model, assert_rows, assert_totals, bit_fields):
        self.name, self.row, self.total, self.order, self.model = name, row, total, order, model
        self.assert_rows, self.assert_totals, self.bit_fields = assert_rows, assert_totals, bit_fields

    def call(self, ctx):
        return getattr(ctx, f"{self.name}_reduce_dev")

    def tree_bytes(self, ctx, k, n):
        return getattr(ctx, f"{self.name}_tree_bytes")(k, n)


STATS = {
    "dxy_pops": Stat("dxy_pops", DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, pair_order, dxy_model, dxy_assert_rows, dxy_assert_totals, ("sum",)),
    "fst_pops": Stat("fst_pops", FST_ROW_DTYPE, FST_TOTAL_DTYPE, pair_order, fst_pops_model.model, test_fst_pops.assert_rows,
                     test_fst_pops.assert_totals, ()),
    "fst_hudson_pops": Stat("fst_hudson_pops", FST_ROW_DTYPE, FST_TOTAL_DTYPE, pair_order, fst_hudson_model.model, test_fst_pops.assert_rows,
                            test_fst_pops.assert_totals, ("asum", "bsum", "fst")),
    "dstat_pops": Stat("dstat_pops", DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, trio_order, dstat_model, test_dstat_pops.assert_rows,
                       test_dstat_pops.assert_totals, ("bbaa", "abba", "baba", "d")),
    "pi_pops": Stat("pi_pops", DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, lambda k: list(range(k)), pi_pops_model.model, test_pi_pops.assert_rows,
                    test_pi_pops.assert_totals, ("sum",)),
}


# ---- section 1: a wave's second build tile -------------------------------------------------------------------------------------
class Columns:
    """one set of columns per (tiles, populations): generated once, shared by the tests of that shape (only the latest is kept)"""
    _last = (None, None)

    @classmethod
    def get(cls, tiles, k, seed):
        if cls._last[0] != (tiles, k, seed):
            cls._last = (None, None)  # let go of the previous shape first
            cls._last = ((tiles, k, seed), cls(tiles, k, seed))
        return cls._last[1]

    def __init__(self, tiles, k, seed):
        t0 = time.perf_counter()
        rng = np.random.default_rng(seed)
        self.tiles, self.n = tiles, shapes.ragged_n(tiles)
        self.chr_ids, self.pos = synth.chromosomes(rng, self.n, 1)
        self.f, self.c = random_pops(rng, self.n, k)
        dev = _dev()
        self.tp = _t(self.pos)
        self.tf = [padded_column(x, float("nan"), dev) for x in self.f]
        self.tn = [padded_column(x, 1000, dev) for x in self.c]
        self.sites = None
        log(f"columns of {k} populations x {self.n} sites ({tiles} tiles): {time.perf_counter() - t0:.1f} s on the host")

    def table(self, pgt, n_waves):
        """site windows W = S = 50 000 over the whole column, then the ranges that read the second round"""
        if self.sites is None:
            self.sites = pgt.build_windows_sites(run_lengths(self.chr_ids), W_SITES, W_SITES)
        special, names = shapes.second_round_windows(self.n, self.tiles, n_waves)
        return np.concatenate([self.sites, special]), self.sites.size, names

    def pops(self, sel):
        """(freq, nInd host columns, device views) of the populations `sel`"""
        return [self.f[q] for q in sel], [self.c[q] for q in sel], [self.tf[q] for q in sel], [self.tn[q] for q in sel]

    def foreign(self, tcols):
        """different columns of the same shape for the foreign tree: the next population's, rotated by half a tile and a bit"""
        import torch
        return [torch.roll(tcols[(q + 1) % len(tcols)], 4099).contiguous() for q in range(len(tcols))]


def poisoned_runs(ctx, call, foreign_tree, sizes, dtypes, shape, check, what):
    """Under each hint: the tree poisoned three ways, the outputs prefilled with 0xFF, all buffers between guards; the first
    run goes to check(rows, totals, what), the other two must repeat its bytes.  -> seconds spent on the GPU calls"""
    import torch
    g = GuardedBuffers(sizes, 97, _dev())
    tree, outs = g.bufs[0], g.bufs[1:]
    gpu = 0.0
    for hint in HINTS:
        first = None
        with ctx.hints(hint, 0, 0):
            for kind in (0, 1, 2):
                poison_tree(tree, kind, other=foreign_tree)
                for b in outs:
                    b.fill_(0xFF)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(tree, *outs)
                torch.cuda.synchronize()
                gpu += time.perf_counter() - t0
                tag = f"{what} hint={hint} poison={kind}"
                g.check(tag)
                got = [rows_from_device(b, dt).reshape(sh).copy() for b, dt, sh in zip(outs, dtypes, shape)]
                if first is None:
                    first = got
                    check(*got, tag)
                else:  # identical under one hint, whatever the workspace held
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, first)), tag
    return gpu


def run_build_case(pgt, ctx, oracle, entry, k, tiles, sel, n_cols):
    st = STATS[entry]
    rounds, waves, n_waves = shapes.grid_of(entry, k, tiles)
    assert rounds == 2
    cols = Columns.get(tiles, n_cols, 7000 + tiles + n_cols)
    f, c, tf, tn = cols.pops(sel)
    win, n_site_rows, names = cols.table(pgt, n_waves)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.any((-(-lo // shapes.LEVEL3) < hi // shapes.LEVEL3) & (lo > n_waves * shapes.TILE)), "a level-3 node of the second round"
    tables = st.order(k)
    t0 = time.perf_counter()
    want, want_t = st.model(cols.pos, f, c, MININD, win)
    host = time.perf_counter() - t0
    wd = windows_to_device(win, _dev())
    _, _, foreign = st.call(ctx)(cols.tp, cols.foreign(tf), cols.foreign(tn), MININD, wd)
    what = f"{entry} K={k} n={cols.n}"

    def check_rows(rows, tag):
        for p, key in enumerate(tables):
            st.assert_rows(rows[p], want[p], f"{tag} {key}")
            if st.bit_fields:
                assert_one_site_bits(rows[p], want[p], win, st.bit_fields, f"{tag} {key}")

    def check(rows, tot, tag):
        all_of(lambda: check_rows(rows, tag), lambda: st.assert_totals(tot, want_t, f"{tag} totals"))
        if entry == "dxy_pops":  # the CPU oracle's scan of each pair's columns: the W = S rows and the genome-wide line
            for p, (i, j) in enumerate(tables):
                ref, rtot = oracle.dxy_scan(cols.chr_ids, cols.pos, f[i], f[j], c[i], c[j], W_SITES, W_SITES, MININD, 1, 0)
                ref = ref[ref["printed"] == 1]
                got = rows[p][:n_site_rows]
                assert got.size == ref.size, tag
                assert np.array_equal(got["start"], ref["start"]) and np.array_equal(got["end"], ref["end"]), (tag, i, j)
                assert np.array_equal(got["neff"], ref["n"]) and np.array_equal(got["nskip"], ref["nskip"]), (tag, i, j)
                assert excess(got["sum"], ref["value"]) <= 0.0, (tag, i, j, "oracle")
                assert int(tot[p]["neff"]) == int(rtot["neff"]) and int(tot[p]["nskip"]) == int(rtot["nskip"]), (tag, i, j)
                assert excess(tot[p]["sum"], rtot["sum"]) <= 0.0, (tag, i, j, "oracle total")

    sizes = [st.tree_bytes(ctx, k, cols.n), len(tables) * win.size * st.row.itemsize, len(tables) * st.total.itemsize]
    gpu = poisoned_runs(ctx, lambda tree, out, tot: st.call(ctx)(cols.tp, tf, tn, MININD, wd, out=out, tot=tot, tree=tree), foreign, sizes,
                        (st.row, st.total), ((len(tables), win.size), (len(tables),)), check, what)
    log(f"{what}: {win.size} windows, {len(tables)} tables; model {host:.1f} s on the host, {2 * 3} GPU calls {gpu:.3f} s")


# one wave per SIMD (5 populations: `*_build_kernel_w1`), 1025 tiles: 516 waves, waves 0 .. 508 walk two tiles
@pytest.mark.parametrize("entry", ["dxy_pops", "fst_pops", "fst_hudson_pops", "dstat_pops"])
def test_second_build_tile_one_wave_per_simd(pgt, ctx, oracle, entry):
    run_build_case(pgt, ctx, oracle, entry, 5, 1025, [0, 1, 2, 3, 4], 5)


# two waves per SIMD, 2049 tiles: 1028 waves, waves 0 .. 1020 walk two tiles.  The columns are those of four populations;
# the three-population calls take populations 0, 1 and 3, so that pair (0, K-1) is the close pair with a negative throughout
@pytest.mark.parametrize("entry,k,sel", [("dxy_pops", 3, [0, 1, 3]), ("fst_pops", 3, [0, 1, 3]), ("fst_hudson_pops", 3, [0, 1, 3]),
                                         ("dstat_pops", 4, [0, 1, 2, 3]), ("pi_pops", 1, [1])],
                         ids=["dxy_pops-K3", "fst_pops-K3", "fst_hudson_pops-K3", "dstat_pops-K4", "pi_pops-K1"])
def test_second_build_tile_two_waves_per_simd(pgt, ctx, oracle, entry, k, sel):
    run_build_case(pgt, ctx, oracle, entry, k, 2049, sel, 4)


def run_af_build_case(pgt, ctx, oracle, k, tiles, cols, freqs, tfreqs):
    rounds, waves, n_waves = shapes.grid_of("fst_af", k, tiles)
    assert rounds >= 2
    nsamp = [12.0, 20.0, 7.0][:k]
    win, n_site_rows, names = cols.table(pgt, n_waves)
    pairs = pair_order(k)
    t0 = time.perf_counter()
    want, scans = af_model(oracle, cols.pos, freqs, nsamp, win, scan=(cols.chr_ids, W_SITES, W_SITES))
    host = time.perf_counter() - t0
    wd = windows_to_device(win, _dev())
    _, foreign = ctx.fst_af_reduce_dev(cols.tp, cols.foreign(tfreqs), nsamp[::-1], wd)
    what = f"fst_af K={k} n={cols.n}"

    def check(rows, tag):
        for p, (i, j) in enumerate(pairs):
            af_assert_rows(rows[p], want[p], f"{tag} pair {(i, j)}")
            ref, r = scans[p], rows[p][:n_site_rows]  # fstWindow (the oracle) on the pair's (a, a + b) columns: the W = S rows
            assert r.size == ref.size, tag
            for fld in ("start", "end", "mid", "n"):
                assert np.array_equal(r[fld], ref[fld]), (tag, fld)
            assert excess(r["bsum"], ref["den"]) <= 0.0, (tag, i, j)
            assert np.all(np.abs(r["asum"] - ref["num"]) <= 1e-9 * np.abs(ref["den"]) + 1e-12), (tag, i, j)
            assert np.all(np.abs(r["fst"] - ref["value"]) <= 1e-9), (tag, i, j)

    tb = int(ctx._lib.pgt_af_tree_bytes(k, cols.n))
    gpu = poisoned_runs(ctx, lambda tree, out: ctx.fst_af_reduce_dev(cols.tp, tfreqs, nsamp, wd, out=out, tree=tree), foreign,
                        [tb, len(pairs) * win.size * FST_ROW_DTYPE.itemsize], (FST_ROW_DTYPE,), ((len(pairs), win.size),), check, what)
    log(f"{what}: {win.size} windows, {rounds} rounds; model {host:.1f} s on the host, {2 * 3} GPU calls {gpu:.3f} s")


def test_second_build_tile_af_two_populations(pgt, ctx, oracle):
    """cap of 512 workgroups: 2049 tiles in two rounds over 1028 waves (populations 0 and 1 of the 2049-tile columns)"""
    cols = Columns.get(2049, 4, 7000 + 2049 + 4)
    run_af_build_case(pgt, ctx, oracle, 2, 2049, cols, cols.f[:2], cols.tf[:2])


class FreqColumns(Columns):
    def __init__(self, tiles, k, seed):
        rng = np.random.default_rng(seed)
        self.tiles, self.n = tiles, shapes.ragged_n(tiles)
        self.chr_ids, self.pos = synth.chromosomes(rng, self.n, 1)
        self.f = [np.round(rng.uniform(0, 1, self.n), 6) for _ in range(k)]
        self.tp = _t(self.pos)
        self.tf = [padded_column(x, float("nan"), _dev()) for x in self.f]
        self.sites = None


def test_second_build_tile_af_three_populations(pgt, ctx, oracle):
    """cap of 2048 workgroups: 8193 tiles (67.1 M sites, 1.6 GB of columns) are the fewest that need more than one round; the
    launch takes five (pops_grid_shapes.BUILD_CASES), 1640 waves of five or four tiles each"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 8e9:
        pytest.skip("needs 8 GB of free HBM")
    Columns._last = (None, None)
    cols = FreqColumns(8193, 3, 7000 + 8193)
    run_af_build_case(pgt, ctx, oracle, 3, 8193, cols, cols.f, cols.tf)


# ---- section 2: a wave's second query item ---------------------------------------------------------------------------------------
N_QUERY_SITES = 270_000


@pytest.fixture(scope="module")
def stride(pgt):
    rng = np.random.default_rng(9100)
    chr_ids, pos = synth.chromosomes(rng, N_QUERY_SITES, 3, equal=False)
    f, c = random_pops(rng, N_QUERY_SITES, 8)
    table = shapes.strided_query_table(pgt.build_windows_sites(run_lengths(chr_ids), 7, 1))
    assert table.size == shapes.QUERY_N_WIN[-1]
    return {"pos": pos, "f": f, "c": c, "table": table, "tp": _t(pos), "tf": [_t(x) for x in f], "tn": [_t(x) for x in c]}


def strided_runs(n_tables, row, total, call, check_full, check_totals, what):
    """The largest table first (its rows are checked against the model), then the two shorter ones: every row they share is
    the same bytes (a row does not depend on the table's other rows, nor on the genome-wide item).  Rows are prefilled with
    0xFF and end at a guard; without `tot` the totals stay 0xFF."""
    import torch
    full, gpu = None, 0.0
    for n_win in sorted(shapes.QUERY_N_WIN, reverse=True):
        for with_tot in ((True, False) if total is not None else (False,)):
            g = GuardedBuffers([n_tables * n_win * row.itemsize, n_tables * (total.itemsize if total is not None else 8)], 11 + n_win % 7, _dev())
            out, tot = g.bufs
            out.fill_(0xFF)
            tot.fill_(0xFF)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(n_win, out, tot if with_tot else False)
            torch.cuda.synchronize()
            gpu += time.perf_counter() - t0
            tag = f"{what} n_win={n_win} tot={with_tot}"
            g.check(tag)
            got = rows_from_device(out, row).reshape(n_tables, n_win)

            def totals():
                if with_tot:
                    check_totals(rows_from_device(tot, total).copy(), f"{tag} totals")
                else:
                    assert bool(torch.all(tot == 0xFF)), (tag, "the totals were written without being asked for")

            def rows():
                if full is None:
                    check_full(got, tag)
                else:
                    assert got.tobytes() == np.ascontiguousarray(full[:, :n_win]).tobytes(), (tag, "rows differ from the longest table's")

            all_of(rows, totals)
            if full is None:
                full = got.copy()
    return gpu


@pytest.mark.parametrize("entry,k", [("dxy_pops", 3), ("dxy_pops", 8), ("fst_pops", 3), ("fst_pops", 5), ("fst_hudson_pops", 3),
                                     ("fst_hudson_pops", 5), ("dstat_pops", 4), ("dstat_pops", 6)])
def test_second_query_item(pgt, ctx, stride, entry, k):
    st = STATS[entry]
    sel = list(range(k - 1)) + [7]  # the last population is the close one: a of pair (0, K-1) negative throughout
    pos, table = stride["pos"], stride["table"]
    f, c = [stride["f"][q] for q in sel], [stride["c"][q] for q in sel]
    tf, tn = [stride["tf"][q] for q in sel], [stride["tn"][q] for q in sel]
    tables = st.order(k)
    t0 = time.perf_counter()
    want, want_t = st.model(pos, f, c, MININD, table)
    host = time.perf_counter() - t0
    what = f"{entry} K={k}"

    def call(n_win, out, tot):
        st.call(ctx)(stride["tp"], tf, tn, MININD, windows_to_device(table[:n_win], _dev()), out=out, tot=tot)

    def check_full(rows, tag):
        for p, key in enumerate(tables):
            st.assert_rows(rows[p], want[p], f"{tag} {key}")
            if st.bit_fields:
                assert_one_site_bits(rows[p], want[p], table, st.bit_fields, f"{tag} {key}")

    gpu = strided_runs(len(tables), st.row, st.total, call, check_full, lambda t, tag: st.assert_totals(t, want_t, tag), what)
    log(f"{what}: {len(tables)} tables of up to {table.size} rows; model {host:.1f} s on the host, 6 GPU calls {gpu:.3f} s")


@pytest.mark.parametrize("k", [3, 8])
def test_second_query_item_af(pgt, ctx, oracle, stride, k):
    pos, table = stride["pos"], stride["table"]
    f, tf = stride["f"][:k], stride["tf"][:k]
    nsamp = [12.0, 20.0, 7.0, 31.0, 5.0, 16.0, 9.0, 25.0][:k]
    pairs = pair_order(k)
    t0 = time.perf_counter()
    want = af_model(oracle, pos, f, nsamp, table)
    host = time.perf_counter() - t0

    def call(n_win, out, tot):
        ctx.fst_af_reduce_dev(stride["tp"], tf, nsamp, windows_to_device(table[:n_win], _dev()), out=out)

    def check_full(rows, tag):
        for p, ij in enumerate(pairs):
            af_assert_rows(rows[p], want[p], f"{tag} pair {ij}")

    gpu = strided_runs(len(pairs), FST_ROW_DTYPE, None, call, check_full, None, f"fst_af K={k}")
    log(f"fst_af K={k}: {len(pairs)} tables of up to {table.size} rows; model {host:.1f} s on the host, 3 GPU calls {gpu:.3f} s")
