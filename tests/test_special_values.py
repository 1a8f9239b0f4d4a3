"""GPU: every reduction on NaN, infinite and full-range column values (include/pgtwin.h, "Values the columns admit").

Every assertion is exact.  Finite inputs are dyadic (synth.exact_*_columns, synth.tied_scores), so every sum is exact in any
order, and the specials are planted so sparsely that no order of the additions can change a result
(special_inputs.fst_special_columns; checked on the CPU in test_special_values_cpu.py).  The comparison rule is
special_inputs.assert_float_column: integers and coordinates bitwise; a float column has the expected NaN mask and, everywhere
else (+-inf, +-0, finite), the expected bits; a SELECTED value (pgt_ext_row.value) is a copy of the input and is compared bit
for bit, NaN included.

Sizes are the smallest that reach every code path: 2 * 8192 + 77 sites for fst and dxy (leaf 128, level-2 tile 8192),
16384 + 300 for the extreme scores (leaf 256, level-2 tile 16384), 65536 + 8192 + 1029 for het (leaf 1024, work item 8192,
level-2 tile 65536), 8192 + 513 for the all-pairs front ends (leaf 512, level-2 tile 8192), 60 000 for the group query."""
import numpy as np
import pytest

import special_inputs as si
import synth
from helpers import rows_equal
from popgenomicstools_amd._lib import (DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, EXT_ROW_DTYPE, FST_ROW_DTYPE, FST_TOTAL_DTYPE, HET_ROW_DTYPE,
                                       PGT_EXT_IHS, PGT_EXT_XP_MAX, PGT_EXT_XP_MIN, WIN_DTYPE)
from popgenomicstools_amd.window_scan import pair_order, rows_from_device, run_lengths, windows_to_device

pytestmark = pytest.mark.gpu

assert (PGT_EXT_IHS, PGT_EXT_XP_MAX, PGT_EXT_XP_MIN) == tuple(m for m, _ in si.EXT_MODES)
POPS_N = 8192 + 513


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _t(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(_dev())


def _one_chromosome(n):
    return np.zeros(n, dtype=np.uint32), np.arange(1, n + 1, dtype=np.uint32)


def _fst_rows_match_oracle(rows, ref, what):
    assert rows.size == ref.size, (what, rows.size, ref.size)
    si.assert_int_columns(rows, ref, (("start", "start"), ("end", "end"), ("mid", "mid"), ("n", "n")), what)
    si.assert_float_column(rows["asum"], ref["num"], what + " asum")
    si.assert_float_column(rows["bsum"], ref["den"], what + " bsum")
    si.assert_float_column(rows["fst"], ref["value"], what + " fst")


# ---------------------------------------------------------------------------------------------------------------------------
# fst
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,W,S", [(si.FST_N, 300, 1), (si.FST_N, 5, 2),   # the sliding query (scan tables; per-lane direct sums)
                                   (si.FST_N, 1000, 250),                   # one wave per window
                                   (si.FST_GROUP_N, 20_000, 100)])          # the group query: windows of >= two level-2 tiles
def test_fst_specials_reach_exactly_their_windows(pgt, ctx, oracle, n, W, S):
    """NaN, +inf, -inf, an (+inf, -inf) pair, +-1.797e308 pairs that overflow and -0.0 at sites 0 and n - 1, on both sides of a
    leaf edge (127 | 128) and of a level-2 edge (8191 | 8192) and in the ragged last tile: the rows are the oracle's (fst
    itself included: NaN where bsum is NaN, +-inf, 0 where bsum == 0), and every window WITHOUT a planted site has, bit for
    bit, the row of the same call with 0.0 at the planted sites — no special leaks through a scan table or a shared sum."""
    chr_ids, pos = si.two_chromosomes(n)
    a, b, planted, a0, b0 = si.fst_special_columns(n, 5)
    ref = oracle.fst_scan(chr_ids, pos, a, b, W, S)
    res = pgt.fst_window(chr_ids, pos, a, b, W, S, ctx=ctx)
    assert np.array_equal(res.win["lo"], ref["lo"]) and np.array_equal(res.win["hi"], ref["hi"])
    _fst_rows_match_oracle(res.rows, ref, f"fst n={n} W={W} S={S}")
    clean = si.windows_without(ref["lo"], ref["hi"], planted)
    assert clean.any() and (~clean).any()
    zeroed = pgt.fst_window(chr_ids, pos, a0, b0, W, S, ctx=ctx).rows
    rows_equal(res.rows[clean], zeroed[clean], f"fst n={n} W={W} S={S}: windows without a planted site")
    assert np.isfinite(zeroed["asum"]).all() and np.isfinite(zeroed["bsum"]).all()


def test_fst_specials_sharded_table(pgt, ctx, oracle):
    """The multi-GPU plan on one GPU (as test_sharded_equals_single_bitwise): every shard reduced on its own columns gives the
    oracle's rows, and, concatenated, the single call's under the comparison rule."""
    from popgenomicstools_amd.distributed import shard_windows
    n, W, S = si.FST_N, 1000, 250
    chr_ids, pos = si.two_chromosomes(n)
    a, b, _, _, _ = si.fst_special_columns(n, 5)
    ref = oracle.fst_scan(chr_ids, pos, a, b, W, S)
    win = pgt.build_windows_sites(run_lengths(chr_ids), W, S)
    single = ctx.fst_reduce(pos, a, b, win)
    _fst_rows_match_oracle(single, ref, "single")
    for world in (2, 3):
        parts = []
        for rank in range(world):
            s, local, _ = shard_windows(win, rank, world)
            lo, hi = int(s["site_lo"]), int(s["site_hi"])
            parts.append(ctx.fst_reduce(pos[lo:hi], a[lo:hi], b[lo:hi], local))
        _fst_rows_match_oracle(np.concatenate(parts), ref, f"{world} shards")


def _fst_dev(ctx, pos, a, b, win):
    import torch
    out, _ = ctx.fst_reduce_dev(_t(pos), _t(a), _t(b), windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    return rows_from_device(out, FST_ROW_DTYPE)


def test_fst_one_division_correctly_rounded_over_the_full_range(pgt, ctx):
    """W = S = 1: asum and bsum are the inputs (-0.0 -> +0.0: the reference's sums start at +0.0, fstWindow.cpp:76-77) and
    fst is ONE correctly rounded division asum / bsum, 0.0 where bsum == 0 (fstWindow.cpp:85) — denormal operands, quotients
    that underflow to a denormal or to 0, quotients that overflow.  Once by the sliding query's per-lane direct sums (the
    host-buffer call derives step 1 from the table) and once by the per-window query under a longest-window hint of 1."""
    a, b = si.division_columns()
    n = a.size
    _, pos = _one_chromosome(n)
    win = pgt.build_windows_sites(np.array([n], dtype=np.uint64), 1, 1)
    with np.errstate(all="ignore"):
        asum, bsum = a + 0.0, b + 0.0
        fst = np.where(bsum != 0.0, asum / bsum, 0.0)
    assert np.array_equal(si.bits(asum)[a != 0], si.bits(a)[a != 0]) and not np.signbit(asum[a == 0]).any()
    with ctx.hints(1, 0):
        per_window = _fst_dev(ctx, pos, a, b, win)
    for what, rows in (("lane-direct", ctx.fst_reduce(pos, a, b, win)), ("per-window", per_window)):
        assert rows.size == n and np.array_equal(rows["n"], np.ones(n, np.uint32))
        si.assert_float_column(rows["asum"], asum, what + " asum")
        si.assert_float_column(rows["bsum"], bsum, what + " bsum")
        si.assert_float_column(rows["fst"], fst, what + " fst")


def test_fst_sum_of_x_and_minus_x_is_plus_zero(pgt, ctx):
    m = 4001
    x = np.ldexp(1.0 + np.arange(m) / 4096.0, np.linspace(-1074, 1023, m).astype(np.int64))
    y = np.ldexp(1.5, np.linspace(1023, -1074, m).astype(np.int64))
    a = np.stack([x, -x], axis=1).ravel()
    a[: 2 * (m // 2)] *= -1.0  # (-x, x) in the first half
    b = np.stack([y, -y], axis=1).ravel()
    n = a.size
    _, pos = _one_chromosome(n)
    win = pgt.build_windows_sites(np.array([n], dtype=np.uint64), 2, 2)
    with ctx.hints(2, 0):
        per_window = _fst_dev(ctx, pos, a, b, win)
    for what, rows in (("lane-direct", ctx.fst_reduce(pos, a, b, win)), ("per-window", per_window)):
        assert rows.size == m
        for f in ("asum", "bsum", "fst"):
            assert not si.bits(rows[f]).any(), (what, f)  # +0.0, never -0.0


# ---------------------------------------------------------------------------------------------------------------------------
# extreme scores
# ---------------------------------------------------------------------------------------------------------------------------
def _check_extreme(pgt, ctx, oracle, chr_ids, pos, score, W, mode, cutoff, chr_len, what):
    ref = oracle.extreme_scan(chr_ids, pos, score, W, mode, cutoff, chr_len)
    if mode == PGT_EXT_IHS:
        res = pgt.ihs_window(chr_ids, pos, score, W, cutoff, chr_len, ctx=ctx)
    else:
        res = pgt.xpehh_window(chr_ids, pos, score, cutoff, W, chr_len, ctx=ctx)
    r = res.rows
    assert r.size == ref.size, what
    assert np.array_equal(res.win["lo"], ref["lo"]) and np.array_equal(res.win["hi"], ref["hi"]), what
    assert np.array_equal(res.win["label_run"], ref["label"]), what
    si.assert_int_columns(r, ref, [(f, f) for f in ("start", "end", "nsites", "nbig", "position")], what)
    si.assert_selected_column(r["value"], ref["value"], what)
    return r


@pytest.mark.parametrize("W,rot", si.EXT_RUNS)
def test_extreme_nan_and_infinity_rules(pgt, ctx, oracle, W, rot):
    """The reference's rule, all three modes: the window's first site is the running extreme unconditionally and a later site
    replaces it only by a strict `>` (ihsWindow.cpp:194-201) — a window whose first key is NaN reports that site (value NaN,
    its bits, with its position), a NaN key at a later site never wins and is never beyond the cutoff.  Window shapes
    (special_inputs.EXT_SHAPES): first site NaN, NaN only later, all NaN, all -inf (the extreme under PGT_EXT_XP_MAX is
    -inf, first site), all +inf (likewise under PGT_EXT_XP_MIN), a +inf tie (first occurrence), NaN on both sides of 255 | 256
    and of 16383 | 16384, at the last site of the partial tile, and a one-site window that is NaN; W = 64 bp keeps every
    window inside a leaf, 1000 spans leaves, 10^6 makes one window per chromosome (level-2 node, then the partial tile)."""
    chr_ids, pos, chr_len = si.extreme_layout()
    for cl in (chr_len, None):
        table = oracle.extreme_scan(chr_ids, pos, np.zeros(si.EXT_N), W, 0, 2.0, cl)
        score, _ = si.extreme_scores(table["lo"], table["hi"], rot)
        for mode, cutoff in si.EXT_MODES:
            _check_extreme(pgt, ctx, oracle, chr_ids, pos, score, W, mode, cutoff, cl, f"W={W} rot={rot} mode={mode} chr_len={cl is not None}")


def test_extreme_probe_of_eight_sites(pgt, ctx):
    """Known answer: scores [nan, 1, 3 | 1, nan, .5 | nan, nan] at positions 1 2 3 | 11 12 13 | 21 22, W = 10, |iHS| with cutoff 2
    -> (nsites, nbig, value, position) = (3, 1, nan, 1), (3, 0, 1.0, 11), (2, 0, nan, 21)."""
    pos = np.array([1, 2, 3, 11, 12, 13, 21, 22], dtype=np.uint32)
    score = np.array([np.nan, 1, 3, 1, np.nan, .5, np.nan, np.nan])
    r = pgt.ihs_window(np.zeros(8, np.uint32), pos, score, 10, 2.0, None, ctx=ctx).rows
    assert [(int(x["nsites"]), int(x["nbig"]), int(x["position"])) for x in r] == [(3, 1, 1), (3, 0, 11), (2, 0, 21)]
    si.assert_selected_column(r["value"], np.array([np.nan, 1.0, np.nan]), "probe")


def test_extreme_specials_sharded_equal_single(pgt, ctx, oracle):
    """Shard by shard (pgt_plan_shards, as test_extreme_sharded_equals_single_with_long_windows): concatenated shards == the
    single call, bit for bit, == the oracle."""
    import torch
    from popgenomicstools_amd.distributed import shard_windows
    chr_ids, pos, _ = si.extreme_layout()
    W = 1000
    win = pgt.build_windows_extreme(pos, run_lengths(chr_ids), None, W)
    score, _ = si.extreme_scores(win["lo"], win["hi"], 0)
    tp, ts = _t(pos), _t(score)
    for mode, cutoff in si.EXT_MODES:
        ref = oracle.extreme_scan(chr_ids, pos, score, W, mode, cutoff, None)
        single, _ = ctx.extreme_reduce_dev(tp, ts, mode, cutoff, windows_to_device(win, _dev()))
        torch.cuda.synchronize()
        single = rows_from_device(single, EXT_ROW_DTYPE)
        si.assert_int_columns(single, ref, [(f, f) for f in ("start", "end", "nsites", "nbig", "position")], f"mode {mode}")
        si.assert_selected_column(single["value"], ref["value"], f"mode {mode}")
        for world in (2, 3, 5):
            parts = []
            for rank in range(world):
                s, local, _ = shard_windows(win, rank, world)
                if local.size == 0:
                    continue
                lo, hi = int(s["site_lo"]), int(s["site_hi"])
                o, _ = ctx.extreme_reduce_dev(tp[lo:hi], ts[lo:hi], mode, cutoff, windows_to_device(local, _dev()))
                torch.cuda.synchronize()
                parts.append(rows_from_device(o, EXT_ROW_DTYPE))
            rows_equal(np.concatenate(parts), single, f"mode {mode}, {world} shards")


# ---------------------------------------------------------------------------------------------------------------------------
# het
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short_only", [True, False])
def test_het_every_byte_value(pgt, ctx, short_only):
    """All 256 int8 values at every offset of a 16-byte word, runs of 0x01 beside 0x81 / 0x00 / 0x7F / 0x80 / 0xFF, windows that
    start and end at every offset mod 16 near both ends of the column: nonmissing = #(g >= 0), nhet = #(g == 1)
    (hetWindow.cpp:78-80), h their one division.  short_only: windows below 65536 sites under the matching hint, so that the
    tree has one level and the two ragged ends are counted together; otherwise the whole tree.  Both once with one wave per
    window (device call, step unknown) and once with the hints the host-buffer call derives from the table."""
    import torch
    g = si.het_bytes_column()
    n = g.size
    _, pos = _one_chromosome(n)
    lo, hi = si.het_windows(n, short_only)
    win = np.zeros(lo.size, dtype=WIN_DTYPE)
    win["lo"], win["hi"] = lo, hi
    c_nm = np.concatenate(([0], np.cumsum(g >= 0)))
    c_nh = np.concatenate(([0], np.cumsum(g == 1)))
    nm = (c_nm[hi.astype(np.int64)] - c_nm[lo.astype(np.int64)]).astype(np.uint32)
    nh = (c_nh[hi.astype(np.int64)] - c_nh[lo.astype(np.int64)]).astype(np.uint32)
    with np.errstate(all="ignore"):
        h = np.where(nm != 0, nh.astype(np.float64) / np.maximum(nm, 1).astype(np.float64), 0.0)
    with ctx.hints(int((hi - lo).max()), 0):
        out, _ = ctx.het_reduce_dev(_t(pos), _t(g), windows_to_device(win, _dev()))
        torch.cuda.synchronize()
    for what, rows in (("one wave per window", rows_from_device(out, HET_ROW_DTYPE)), ("derived hints", ctx.het_reduce(pos, g, win))):
        assert np.array_equal(rows["nonmissing"], nm), what
        assert np.array_equal(rows["nhet"], nh), what
        assert np.array_equal(rows["start"], pos[lo.astype(np.int64)]) and np.array_equal(rows["end"], pos[hi.astype(np.int64) - 1]), what
        si.assert_float_column(rows["h"], h, what + " h")


# ---------------------------------------------------------------------------------------------------------------------------
# dxy
# ---------------------------------------------------------------------------------------------------------------------------
def _dxy_dev(ctx, pos, p1, p2, n1, n2, minind, win):
    import torch
    out, tot, _ = ctx.dxy_reduce_dev(_t(pos), _t(p1), _t(p2), _t(n1), _t(n2), minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    return rows_from_device(out, DXY_ROW_DTYPE), rows_from_device(tot, DXY_TOTAL_DTYPE)


def _dxy_het_dev(ctx, pos, p1, p2, n1, n2, g1, g2, minind, win):
    import torch
    out, tot, h1, h2, _ = ctx.dxy_het_reduce_dev(_t(pos), _t(p1), _t(p2), _t(n1), _t(n2), _t(g1), _t(g2), minind,
                                                 windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    return rows_from_device(out, DXY_ROW_DTYPE), rows_from_device(tot, DXY_TOTAL_DTYPE), rows_from_device(h1, HET_ROW_DTYPE), \
        rows_from_device(h2, HET_ROW_DTYPE)


@pytest.mark.parametrize("minind", si.MININDS)
def test_dxy_counts_at_their_extremes(pgt, ctx, oracle, minind):
    """n1, n2 from {INT32_MIN, -1, 0, minind - 1, minind, INT32_MAX}: a site counts when both are >= minind, as signed 32-bit
    integers (dxyWindow.cpp:381).  Exact dyadic frequencies: neff, nskip, sum and the genome-wide line equal the oracle's."""
    n = si.FST_N
    rng = np.random.default_rng(17 + minind % 1000)
    chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
    p1, p2, _, _, _, _ = synth.exact_dxy_columns(rng, n)
    n1, n2 = si.extreme_counts(rng, n, minind)
    g1, g2 = synth.het_column(rng, n).astype(np.int8), synth.het_column(rng, n).astype(np.int8)
    for W, S in ((1000, 250), (5, 2)):
        ref, rtot = oracle.dxy_scan(chr_ids, pos, p1, p2, n1, n2, W, S, minind, 1, 0)
        ref = ref[ref["printed"] == 1]
        assert 0 < int(rtot["neff"]) < n
        win = pgt.build_windows_sites(run_lengths(chr_ids), W, S)
        fused = _dxy_het_dev(ctx, pos, p1, p2, n1, n2, g1, g2, minind, win)
        for what, (rows, tot) in (("host buffers", ctx.dxy_reduce(pos, p1, p2, n1, n2, minind, win)),
                                  ("device", _dxy_dev(ctx, pos, p1, p2, n1, n2, minind, win)), ("fused with het", fused[:2])):
            what = f"dxy minind={minind} W={W} S={S} {what}"
            tot = np.atleast_1d(tot)[0]
            assert rows.size == ref.size, what
            si.assert_int_columns(rows, ref, (("start", "start"), ("end", "end"), ("neff", "n"), ("nskip", "nskip")), what)
            si.assert_float_column(rows["sum"], ref["value"], what + " sum")
            assert (int(tot["neff"]), int(tot["nskip"])) == (int(rtot["neff"]), int(rtot["nskip"])), what
            si.assert_float_column([tot["sum"]], [rtot["sum"]], what + " genome-wide sum")
        for g, hrows in ((g1, fused[2]), (g2, fused[3])):
            href = oracle.het_scan(chr_ids, pos, g.astype(np.int32), W, S)
            assert np.array_equal(hrows["nonmissing"], href["n"]) and np.array_equal(hrows["nhet"], href["num"].astype(np.uint32))
            si.assert_float_column(hrows["h"], href["value"], "fused het h")


def _uncounted(rng, n, k, minind):
    """exact frequencies and counts of k populations; at about one site in 16 one population's count is below minind and its
    frequency there is garbage (NaN, +inf, -inf, -5.0, 7.0) in the first result, 0.5 in the second"""
    f, _ = synth.exact_freq_columns(rng, n, k)
    c = [rng.integers(minind, 41, n, dtype=np.int32) for _ in range(k)]
    sites = np.flatnonzero(rng.random(n) < 1 / 16)
    sites = np.union1d(sites, [0, 511, 512, 8191, 8192, n - 1])
    who = rng.integers(0, k, sites.size)
    bad, half = [x.copy() for x in f], [x.copy() for x in f]
    for j in range(k):
        s = sites[who == j]
        c[j][s] = rng.integers(-3, minind, s.size)
        bad[j][s] = rng.choice(np.array(si.GARBAGE), s.size)
        half[j][s] = 0.5
    return bad, half, c


def test_uncounted_site_frequency_decides_nothing_two_populations(pgt, ctx):
    n, minind = si.FST_N, 5
    rng = np.random.default_rng(91)
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    bad, half, c = _uncounted(rng, n, 2, minind)
    g1, g2 = synth.het_column(rng, n).astype(np.int8), synth.het_column(rng, n).astype(np.int8)
    for W, S in ((1000, 250), (7, 3), (300, 1)):
        win = pgt.build_windows_sites(run_lengths(chr_ids), W, S)
        with ctx.hints(W, S):
            got, want = _dxy_dev(ctx, pos, *bad, *c, minind, win), _dxy_dev(ctx, pos, *half, *c, minind, win)
            fgot = _dxy_het_dev(ctx, pos, *bad, *c, g1, g2, minind, win)
            fwant = _dxy_het_dev(ctx, pos, *half, *c, g1, g2, minind, win)
        assert 0 < int(want[1]["nskip"][0]) < n and np.isfinite(want[0]["sum"]).all()
        rows_equal(got[0], want[0], f"dxy rows W={W} S={S}")
        rows_equal(got[1], want[1], f"dxy genome-wide line W={W} S={S}")
        for k, name in enumerate(("rows", "genome-wide line", "het rows 1", "het rows 2")):
            rows_equal(fgot[k], fwant[k], f"fused dxy + het {name} W={W} S={S}")
        rows_equal(fgot[0], got[0], f"fused rows == plain rows W={W} S={S}")


def _pops_dev(ctx, which, pos, f, c, minind, win, row_dtype, tot_dtype):
    import torch
    call = ctx.dxy_pops_reduce_dev if which == "dxy" else ctx.fst_pops_reduce_dev
    out, tot, _ = call(_t(pos), [_t(x) for x in f], [_t(x) for x in c], minind, windows_to_device(win, _dev()))
    torch.cuda.synchronize()
    n_pairs = len(f) * (len(f) - 1) // 2
    return rows_from_device(out, row_dtype)[: n_pairs * win.size].reshape(n_pairs, win.size), rows_from_device(tot, tot_dtype)[:n_pairs]


@pytest.mark.parametrize("which,k", [("dxy", 3), ("dxy", 8), ("fst", 3), ("fst", 8)])
def test_uncounted_site_frequency_decides_nothing_all_pairs(pgt, ctx, which, k):
    """pgt_dxy_pops_reduce_dev / pgt_fst_pops_reduce_dev: a population below minind at a site takes its pairs out of that site;
    whatever its frequency column holds there, every row and every genome-wide line keeps its bits."""
    n, minind = POPS_N, 5
    rng = np.random.default_rng(100 * k + len(which))
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    bad, half, c = _uncounted(rng, n, k, minind)
    dt = (DXY_ROW_DTYPE, DXY_TOTAL_DTYPE) if which == "dxy" else (FST_ROW_DTYPE, FST_TOTAL_DTYPE)
    for W, S in ((7, 3), (512, 512), (3000, 1000), (n, n)):
        win = pgt.build_windows_sites(run_lengths(chr_ids), W, S) if W < n else np.array([(0, n, 0, 0, 0, 0)], dtype=WIN_DTYPE)
        got = _pops_dev(ctx, which, pos, bad, c, minind, win, *dt)
        want = _pops_dev(ctx, which, pos, half, c, minind, win, *dt)
        val = "sum" if which == "dxy" else "bsum"
        assert np.isfinite(want[0][val]).all() and np.isfinite(want[1][val]).all() and int(want[1]["nskip"].min()) > 0
        for p, ij in enumerate(pair_order(k)):
            rows_equal(got[0][p], want[0][p], f"{which} K={k} W={W} S={S} pair {ij}")
        rows_equal(got[1], want[1], f"{which} K={k} W={W} S={S} genome-wide lines")


@pytest.mark.parametrize("which,k", [("af", 5), ("af", 8), ("pops", 5), ("pops", 8)])
def test_nan_in_one_population_stays_in_its_pairs(pgt, ctx, which, k):
    """pgt_fst_af_reduce_dev / pgt_fst_pops_reduce_dev: NaN in ONE population's frequency at a few counted sites, on both sides
    of a leaf edge (511 | 512) and of a level-2 edge (8191 | 8192).  Pairs without that population keep every bit; pairs with
    it are NaN (asum, bsum, fst) in exactly the windows that hold such a site, their counts unchanged."""
    import torch
    n, minind, who = POPS_N, 5, 2
    rng = np.random.default_rng(7 * k + len(which))
    chr_ids, pos = synth.chromosomes(rng, n, 2, equal=False)
    f, _ = synth.exact_freq_columns(rng, n, k)
    c = [rng.integers(0, 41, n, dtype=np.int32) for _ in range(k)]
    sites = np.array([0, 511, 512, 4000, 8191, 8192, n - 1], dtype=np.int64)
    for j in range(k):
        c[j][sites] = 9  # counted for every pair
    fn = [x.copy() for x in f]
    fn[who][sites] = np.nan
    nsamp = [float(x) for x in rng.integers(5, 40, k)]

    def call(freqs, win):
        if which == "pops":
            return _pops_dev(ctx, "fst", pos, freqs, c, minind, win, FST_ROW_DTYPE, FST_TOTAL_DTYPE)
        out, _ = ctx.fst_af_reduce_dev(_t(pos), [_t(x) for x in freqs], nsamp, windows_to_device(win, _dev()))
        torch.cuda.synchronize()
        return rows_from_device(out, FST_ROW_DTYPE).reshape(k * (k - 1) // 2, win.size), None

    for W, S in ((7, 3), (512, 512), (3000, 1000), (n, n)):
        win = pgt.build_windows_sites(run_lengths(chr_ids), W, S) if W < n else np.array([(0, n, 0, 0, 0, 0)], dtype=WIN_DTYPE)
        hit = ~si.windows_without(win["lo"], win["hi"], sites)
        assert hit.any() and (W == n or (~hit).any())
        (got, gtot), (want, wtot) = call(fn, win), call(f, win)
        for p, (i, j) in enumerate(pair_order(k)):
            what = f"{which} K={k} W={W} S={S} pair {(i, j)}"
            if who not in (i, j):
                rows_equal(got[p], want[p], what)
                continue
            si.assert_int_columns(got[p], want[p], [(x, x) for x in ("start", "end", "mid", "n")], what)
            for fld in ("asum", "bsum", "fst"):
                assert np.isfinite(want[p][fld]).all(), what
                assert np.array_equal(np.isnan(got[p][fld]), hit), (what, fld)
                assert np.array_equal(si.bits(got[p][fld][~hit]), si.bits(want[p][fld][~hit])), (what, fld)
            if gtot is not None:
                assert (int(gtot[p]["neff"]), int(gtot[p]["nskip"])) == (int(wtot[p]["neff"]), int(wtot[p]["nskip"])), what
                assert np.isnan(gtot[p]["asum"]) and np.isnan(gtot[p]["bsum"]), what
        if gtot is not None:
            keep = np.array([who not in ij for ij in pair_order(k)])
            rows_equal(gtot[keep], wtot[keep], f"{which} K={k} W={W} S={S} genome-wide lines of the other pairs")
