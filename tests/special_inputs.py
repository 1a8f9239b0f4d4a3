"""Inputs with NaN, infinite and full-range values for tests/test_special_values.py and tests/test_special_values_pops.py
(GPU) and the CPU checks of their expectations (tests/test_special_values_cpu.py, tests/test_special_values_pops_cpu.py).
numpy, host side; nothing here touches the product."""
import numpy as np

import synth

NAN = np.float64(np.nan)
INF = np.float64(np.inf)
# quiet NaNs with a payload and with the sign set: a SELECTED value is a copy of the input, so these bits must come back
NAN_PAYLOAD = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
NAN_NEGATIVE = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
HUGE = np.float64(1.797e308)  # HUGE + HUGE overflows; HUGE + (any sum of the dyadic columns) == HUGE


# ---- comparison rule -------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_float_column(got, want, what):
    """THE comparison rule for a float column: the NaN masks are equal; everywhere else (+-inf, +-0, finite) the bits are
    equal.  Sign and payload of a COMPUTED NaN are not part of the contract (x86 gives a sign-set NaN for inf - inf and
    inf / inf, the GPU need not)."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = int(np.flatnonzero(gn != wn)[0])
        raise AssertionError(f"{what}: NaN masks differ at {int((gn != wn).sum())} of {got.size} entries; first at {i}: "
                             f"got {got.flat[i]!r}, want {want.flat[i]!r}")
    bad = (bits(got) != bits(want)) & ~wn
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} entries differ in their bits; first at {i}: "
                             f"got {got.flat[i]!r} ({bits(got).flat[i]:#018x}), want {want.flat[i]!r} ({bits(want).flat[i]:#018x})")


def assert_selected_column(got, want, what):
    """A SELECTED value (pgt_ext_row.value) is a copy of the input: every bit is compared, NaN included."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        i = int(np.flatnonzero(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} selected values differ; first at {i}: got "
                             f"{np.asarray(got).flat[i]!r} ({g.flat[i]:#018x}), want {np.asarray(want).flat[i]!r} ({w.flat[i]:#018x})")


def assert_int_columns(got, want, pairs, what):
    for g, w in pairs:
        if not np.array_equal(got[g], want[w]):
            i = int(np.flatnonzero(got[g] != want[w])[0])
            raise AssertionError(f"{what}: column {g} differs at {int((got[g] != want[w]).sum())} rows; first at {i}: got "
                                 f"{got[g][i]}, want {want[w][i]}")


# ---- fst: specials at the edges of the leaves (128 sites) and of the level-2 tiles (8192 sites) ----------------------------------
FST_N = 2 * 8192 + 77
FST_GROUP_N = 60_000


def two_chromosomes(n):
    """-> (chr_ids, pos): two chromosomes of (n + 1) // 2 and n // 2 sites, positions 3, 6, 9, ... in each"""
    n0 = (n + 1) // 2
    chr_ids = (np.arange(n) >= n0).astype(np.uint32)
    pos = (3 * (np.arange(n) - n0 * chr_ids.astype(np.int64) + 1)).astype(np.uint32)
    return chr_ids, pos


def fst_special_columns(n, seed):
    """-> (a, b, planted site indices, a0, b0): exact dyadic columns (synth.exact_fst_columns) with 13 specials, and the same
    columns with 0.0 at the planted sites.

    Every window sum is the same in ANY order of the additions, so the oracle's sequential sum is the expectation for every
    query strategy: the finite values are dyadic (exact partial sums), HUGE absorbs them, and per column the specials are
    chosen so that no order can give another result —
      a: NaN, +inf, (+inf, -inf) 40 sites apart (both in a window: NaN in any order), -0.0, and a (-HUGE, -HUGE) pair across
         the level-2 boundary 8191 | 8192 that overflows to -inf (a window that also holds the +inf of site 127 or 3000 holds
         the -inf of site 3040 as well: NaN in any order);
      b: NaN, +inf, -0.0 and a (+HUGE, +HUGE) pair in the ragged last tile that overflows to +inf; nothing negative."""
    rng = np.random.default_rng(seed)
    a0, b0, _, _ = synth.exact_fst_columns(rng, n)
    a, b = a0.copy(), b0.copy()
    rag = (n // 8192) * 8192 + 50  # inside the ragged last level-2 tile
    assert rag + 1 < n - 1
    plant_a = {0: NAN, 127: INF, 128: -0.0, 3000: INF, 3040: -INF, 8191: -HUGE, 8192: -HUGE, n - 1: NAN}
    plant_b = {127: NAN, 128: -0.0, 8191: INF, rag: HUGE, rag + 1: HUGE}
    for i, v in plant_a.items():
        a[i] = v
    for i, v in plant_b.items():
        b[i] = v
    planted = np.array(sorted(set(plant_a) | set(plant_b)), dtype=np.int64)
    a0, b0 = a0.copy(), b0.copy()
    a0[planted] = 0.0
    b0[planted] = 0.0
    return a, b, planted, a0, b0


def windows_without(lo, hi, planted):
    """mask of the windows [lo, hi) that hold none of the planted sites"""
    cnt = np.searchsorted(planted, np.asarray(hi, dtype=np.int64)) - np.searchsorted(planted, np.asarray(lo, dtype=np.int64))
    return cnt == 0


def division_columns():
    """(a, b) for the one division per row over the full range: a = +-m 2^i, b = m' 2^j with the exponents sweeping
    -1074 ... 1023 (denormal numerators and denominators, quotients that underflow to a denormal or to 0, quotients that
    overflow), a few mantissas with a full 53 bits, zero denominators of both signs, zero numerators of both signs and
    infinite operands."""
    e = sorted(set(range(-1074, 1024, 41)) | {-1074, -1073, -1023, -1022, -1021, -53, -1, 0, 1, 52, 970, 1022, 1023})
    m = np.array([1.0, 1.5, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 4.0 / 3.0])
    ei, ej, mi = np.meshgrid(np.array(e), np.array(e), np.arange(m.size), indexing="ij")
    ei, ej, mi = ei.ravel(), ej.ravel(), mi.ravel()
    sign = np.where(np.arange(ei.size) % 3 == 1, -1.0, 1.0)
    a = sign * np.ldexp(m[mi], ei)
    b = np.ldexp(m[(mi * 2 + np.arange(ei.size) // 7) % m.size], ej)
    # quotients around the edges of the range: i - j near -1075 (rounds to 0 or to the smallest denormal), -1022, 1024
    extra_a, extra_b = [], []
    for d in (-1077, -1076, -1075, -1074, -1073, -1024, -1023, -1022, -1021, 1022, 1023, 1024, 1025):
        for j in (-1074, -1050, -1022, -600, -51, 0):
            i = d + j
            if -1074 <= i <= 1023:
                for x in m:
                    for y in m:
                        extra_a.append(np.ldexp(x, i))
                        extra_b.append(np.ldexp(y, j))
    tail_a = [1.0, -1.0, 0.0, -0.0, 0.0, -0.0, INF, -INF, INF, 1.0, 5e-324, -5e-324, HUGE, -0.0]
    tail_b = [0.0, -0.0, 0.0, -0.0, 2.0, 2.0, 1.0, 5e-324, INF, INF, 0.0, -0.0, 5e-324, -INF]
    a = np.concatenate([a, np.array(extra_a), np.array(tail_a)])
    b = np.concatenate([b, np.array(extra_b), np.array(tail_b)])
    return a, b


# ---- extreme scores (leaf 256 sites, level-2 tile 16384 sites) --------------------------------------------------------------------
EXT_N = 16384 + 300
EXT_MODES = ((0, 2.0), (1, 2.0), (2, -2.0))  # (PGT_EXT_IHS, cutoff), (PGT_EXT_XP_MAX, cutoff), (PGT_EXT_XP_MIN, cutoff)
EXT_RUNS = ((64, 0), (64, 3), (1000, 0), (1000, 5), (1_000_000, 0), (1_000_000, 1), (1_000_000, 5))  # (W in bp, rotation of the shapes)
EXT_SHAPES = ("first_nan", "later_nan", "all_nan", "all_ninf", "all_pinf", "pinf_tie", "first_nan_then_pinf", "first_ninf")
EXT_LONE_SITE = 5000


def extreme_layout():
    """Two chromosomes (16384 + 200 and 100 sites), consecutive positions but for one site that lies 200 bp from both its
    neighbours (alone in a 64-bp window).  -> (chr_ids, pos, chr_len)"""
    n0 = 16384 + 200
    gaps = np.ones(EXT_N, dtype=np.int64)
    gaps[EXT_LONE_SITE] = gaps[EXT_LONE_SITE + 1] = 200
    pos = np.concatenate([np.cumsum(gaps[:n0]), np.cumsum(gaps[n0:])]).astype(np.uint32)
    chr_ids = np.concatenate([np.zeros(n0, np.uint32), np.ones(EXT_N - n0, np.uint32)])
    chr_len = np.array([int(pos[n0 - 1]) + 37, int(pos[-1]) + 150], dtype=np.uint32)
    return chr_ids, pos, chr_len


def extreme_scores(lo, hi, rot, seed=7):
    """synth.tied_scores with NaN / +inf / -inf planted by window shape: every third window of at least four sites of the
    table (lo, hi) gets one of EXT_SHAPES in turn (starting at `rot`), windows of one site become NaN, and the sites on both
    sides of a leaf edge (255 | 256), of a level-2 edge (16383 | 16384) and the last site of the partial tile are NaN."""
    s = synth.tied_scores(np.random.default_rng(seed), EXT_N).astype(np.float64)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    used = set()
    for j, k in enumerate(np.flatnonzero(hi - lo >= 4)[::3]):
        shape = EXT_SHAPES[(j + rot) % len(EXT_SHAPES)]
        used.add(shape)
        a, b = int(lo[k]), int(hi[k])
        if shape == "first_nan":
            s[a] = (NAN, NAN_PAYLOAD, NAN_NEGATIVE)[j % 3]
        elif shape == "later_nan":
            s[a + 1], s[b - 1] = NAN_NEGATIVE, NAN
        elif shape == "all_nan":
            s[a:b] = NAN
            s[a + 1] = NAN_PAYLOAD
        elif shape == "all_ninf":
            s[a:b] = -INF
        elif shape == "all_pinf":
            s[a:b] = INF
        elif shape == "pinf_tie":
            s[a + 1] = s[b - 1] = INF
        elif shape == "first_nan_then_pinf":
            s[a], s[a + 2] = NAN_PAYLOAD, INF
        elif shape == "first_ninf":
            s[a] = -INF
    for k in np.flatnonzero(hi - lo == 1):
        s[int(lo[k])] = NAN
    for i in (255, 256, 16383, 16384, EXT_N - 1):
        s[i] = NAN
    return s, used


def extreme_model(score, lo, hi, mode, cutoff):
    """The reference's rule (ihsWindow.cpp:194-205, xpehhWindow.cpp:210-216) restated on one window table: the window's first
    site is the running extreme unconditionally, a later site replaces it only when its key is strictly greater; a key counts
    when it is beyond the cutoff.  -> (index of the reported site or -1, nbig) per window."""
    key = np.abs(score) if mode == 0 else (score if mode == 1 else -score)
    thr = -cutoff if mode == 2 else cutoff
    at, nbig = np.full(len(lo), -1, dtype=np.int64), np.zeros(len(lo), dtype=np.int64)
    for w, (a, b) in enumerate(zip(lo, hi)):
        if b > a:
            k = key[a:b]
            # a NaN first key is never replaced (nothing is > NaN); otherwise NaN keys never win: the first maximum of the rest
            at[w] = a if np.isnan(k[0]) else a + int(np.argmax(np.where(np.isnan(k), -np.inf, k)))
            nbig[w] = int(np.count_nonzero(k > thr))
    return at, nbig


# ---- het: every byte value --------------------------------------------------------------------------------------------------
HET_N = 65536 + 8192 + 1029


def het_bytes_column():
    """All 256 int8 values, every value at every offset 0 ... 15 of a 16-byte word (the value at site i is i + i // 256 mod
    256: the cycle shifts by one per 256 sites), with runs of 0x01 next to 0x81, 0x00, 0x7F, 0x80 and 0xFF (the neighbours a
    carry of the packed byte count would come from) at every alignment inside a 4-byte word, near both ends of the column,
    in whole work items and in the ragged tail."""
    i = np.arange(HET_N, dtype=np.int64)
    g = ((i + i // 256) % 256).astype(np.uint8)
    run = np.array([1, 1, 1, 0x81, 1, 1, 0x00, 1, 1, 1, 0x7F, 1, 1, 0x80, 1, 1, 1, 0xFF, 1, 1, 0xFF, 1, 0x80, 1, 0x7F, 1, 0x81, 1, 1], dtype=np.uint8)
    for start in (3, 1030, 20_000, 65_530, 65536 + 8192 + 5, HET_N - 4 * (run.size + 1) - 1):
        for k in range(4):  # the next copy starts one byte later inside its 4-byte word
            at = start + k * (run.size + 1 - (run.size + 1) % 4 + 1)
            g[at:at + run.size] = run
    seen = np.zeros((256, 16), dtype=bool)
    seen[g, i % 16] = True
    assert seen.all()
    return g.view(np.int8)


def het_windows(n, short_only):
    """(lo, hi) pairs that start and end at every offset mod 16 near both ends of the column and around the edges of the
    1024-site leaves, the 8192-site work items and the 65536-site level-2 tile; short_only: nothing of 65536 sites or more
    (the tree is then built to one level and windows with a whole leaf take the two-ranges path)."""
    out = set()
    lengths = (1, 2, 3, 15, 16, 17, 100, 1023, 1024, 1025, 1030, 2100, 9000, 40_000) + (() if short_only else (65_536, 70_001, n))
    for k in range(0, 34):
        for L in lengths:
            out.add((k, min(n, k + L)))
            out.add((max(0, n - k - L), n - k))
        out.add((k, n - (k * 7) % 18))
        for edge in (1024, 8192, 65536, 65536 + 8192):
            out.add((edge - k, min(n, edge + 1024 + (k * 5) % 17)))
            out.add((edge - 1024 - (k * 3) % 16, edge + k))
    out = sorted((a, b) for a, b in out if 0 <= a < b <= n and (not short_only or b - a < 65_536))
    return np.array([a for a, _ in out], dtype=np.uint64), np.array([b for _, b in out], dtype=np.uint64)


# ---- counts at their extremes -----------------------------------------------------------------------------------------------
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MININDS = (0, 1, 20, I32_MAX)


def extreme_counts(rng, n, minind):
    vals = np.array(sorted({I32_MIN, -1, 0, max(minind - 1, I32_MIN), minind, I32_MAX}), dtype=np.int64).astype(np.int32)
    return rng.choice(vals, size=n), rng.choice(vals, size=n)


GARBAGE = (NAN, INF, -INF, -5.0, 7.0)


# ---- the K-population kernels (tests/test_special_values_pops.py on the GPU, tests/test_special_values_pops_cpu.py for the expectations) ----
# dxy_pops, fst_pops (Weir-Cockerham), fst_hudson_pops, pi_pops, dstat_pops, fd_pops: leaf 512 sites, level-2 tile 8192 sites,
# level-3 node 64 tiles.  A special value sits at a COUNTED site here, so the expectation is the per-site definition itself
# (the models' per-site functions) summed by window_sums below, which carries NaN and infinities where a difference of prefix
# sums cannot.
POPS_N = 8192 + 513          # a ragged last tile, n mod 4 == 1
POPS_L3_N = 524288 + 8192 + 5
POPS_L3_PLANTED = (524287, 524288)
POPS_L3_WINDOWS = ((0, 524288), (1, 524288), (0, 524287), (524288, POPS_L3_N), (524289, POPS_L3_N), (0, POPS_L3_N))
POPS_MININD = 5
POPS_TABLES = ((7, 3), (512, 512), (3000, 1000))
# both sides of a leaf edge and of a tile edge, two neighbours inside one quad, the column's first site and its last quad
POPS_PLANTED = (0, 511, 512, 4000, 4001, 8191, 8192, POPS_N - 1)
POPS_EDGE_VALUES = (-0.0, 5e-324, 2.0 ** -1022, 1.0 - 2.0 ** -53, 0.0, 1.0)  # inside the contract: frequencies in [0, 1]
POPS_SUMS = {"dxy": ("sum",), "pi": ("sum",), "fst": ("asum", "bsum"), "fst_hudson": ("asum", "bsum"),
             "dstat": ("bbaa", "abba", "baba"), "fd": ("num", "fd_den", "fdm_den")}
# the population branch statistic (tests/test_special_values_pbs.py): a trio's six sums, the pair values of "fst" / "fst_hudson"
POPS_SUMS["pbs"] = POPS_SUMS["pbs_hudson"] = ("num_ij", "num_ik", "num_jk", "den_ij", "den_ik", "den_jk")
PBS_PAIR_STAT = {"pbs": "fst", "pbs_hudson": "fst_hudson"}
POPS_SECTION1 = [("dxy", 3), ("dxy", 8), ("fst_hudson", 3), ("fst_hudson", 8), ("pi", 2), ("pi", 8), ("dstat", 4), ("dstat", 7),
                 ("fd", 4), ("fd", 5), ("fd", 7)]  # fd: the two-wave build, the one-wave build without recompute, kRecompute
POPS_SMALLEST_LARGEST = [("dxy", 2), ("dxy", 8), ("fst", 2), ("fst", 8), ("fst_hudson", 2), ("fst_hudson", 8), ("pi", 1), ("pi", 8),
                         ("dstat", 4), ("dstat", 7), ("fd", 4), ("fd", 7)]
POPS_VALUE_STATS = ("fst", "fst_hudson", "pi")  # the counts are VALUES of the per-site function, not only its predicate
POPS_MININDS = (1, 20, I32_MAX)
REL_A, ABS_A = 1e-9, 1e-12  # helpers.REL / ABS against the scale A = Σ|term| (tests/test_fd_pops.py derives the bound)


def pops_dtypes(stat):
    from popgenomicstools_amd import _lib
    return {"dxy": (_lib.DXY_ROW_DTYPE, _lib.DXY_TOTAL_DTYPE), "pi": (_lib.DXY_ROW_DTYPE, _lib.DXY_TOTAL_DTYPE),
            "fst": (_lib.FST_ROW_DTYPE, _lib.FST_TOTAL_DTYPE), "fst_hudson": (_lib.FST_ROW_DTYPE, _lib.FST_TOTAL_DTYPE),
            "dstat": (_lib.DSTAT_ROW_DTYPE, _lib.DSTAT_TOTAL_DTYPE), "fd": (_lib.FD_ROW_DTYPE, _lib.FD_TOTAL_DTYPE),
            "pbs": (_lib.PBS_ROW_DTYPE, _lib.PBS_TOTAL_DTYPE), "pbs_hudson": (_lib.PBS_ROW_DTYPE, _lib.PBS_TOTAL_DTYPE)}[stat]


def pops_items(stat, k):
    """the populations every item of the call holds, in the order of the row tables: a population (pi), a pair, a trio with
    the outgroup (the last population) as its fourth, or (pbs) a trio i < j < k of all populations"""
    from popgenomicstools_amd.window_scan import pair_order, trio_order
    if stat in PBS_PAIR_STAT:
        from f3_pops_model import all_trio_order
        return [tuple(t) for t in all_trio_order(k)]
    if stat == "pi":
        return [(i,) for i in range(k)]
    if stat in ("dstat", "fd"):
        return [tuple(t) + (k - 1,) for t in trio_order(k)]
    return [tuple(p) for p in pair_order(k)]


def pops_counted(item, c, minind):
    """the predicate as the header states it: every population of the item has nind >= minind, compared as signed int32"""
    ok = np.ones(len(c[0]), dtype=bool)
    for x in item:
        assert c[x].dtype == np.int32
        ok &= c[x] >= np.int32(minind)
    return ok


def pops_site_terms(stat, item, f, c):
    """-> the item's per-site terms (one array per sum of POPS_SUMS[stat]) by the models' per-site functions: float64, every
    operation rounded on its own, whatever they are at a site that is not counted"""
    import dstat_pops_model
    import fd_pops_model
    import fst_hudson_model
    import fst_pops_model
    import pi_pops_model
    with np.errstate(all="ignore"):
        if stat == "dxy":
            i, j = item
            return (f[i] * (1.0 - f[j]) + f[j] * (1.0 - f[i]),)
        if stat == "pi":
            return (pi_pops_model.site_pi(f[item[0]], c[item[0]]),)
        if stat == "fst":
            i, j = item
            return fst_pops_model.site_components(f[i], f[j], c[i], c[j])
        if stat == "fst_hudson":
            i, j = item
            return fst_hudson_model.site_components(f[i], f[j], c[i], c[j])
        if stat in PBS_PAIR_STAT:  # the pair's two values for (i, j), (i, k), (j, k): the numerators, then the denominators
            i, j, k = item
            pairs = [pops_site_terms(PBS_PAIR_STAT[stat], p, f, c) for p in ((i, j), (i, k), (j, k))]
            return tuple(x[0] for x in pairs) + tuple(x[1] for x in pairs)
        fn = dstat_pops_model.site_components if stat == "dstat" else fd_pops_model.site_terms
        return fn(*(f[x] for x in item))


def pops_ratios(stat, row):
    """-> [(field, the stated function of the row's own sums)]"""
    import dstat_pops_model
    import fd_pops_model
    if stat in ("fst", "fst_hudson"):
        with np.errstate(all="ignore"):
            return [("fst", np.where(row["bsum"] != 0, row["asum"] / np.where(row["bsum"] != 0, row["bsum"], 1.0), 0.0))]
    if stat == "dstat":
        return [("d", dstat_pops_model.d_of(row["abba"], row["baba"]))]
    if stat == "fd":
        return [("fd", fd_pops_model.ratio(row["num"], row["fd_den"])), ("fdm", fd_pops_model.ratio(row["num"], row["fdm_den"]))]
    return []


def window_sums(terms, lo, hi):
    """The window expectation that survives non-finite terms.  terms: an item's per-site terms with the sites that are not
    counted already 0.0 (selected away by the predicate); (lo, hi): the table.  -> (want, A, finite) per window: A is
    Σ|finite terms|, and want follows the rule that holds in ANY order of the additions — a NaN term gives NaN, +inf and -inf
    together give NaN, infinities of one sign give that infinity, otherwise the correctly rounded sum (math.fsum) plus +0.0.
    Every finite term is at most 8 in magnitude, so no partial sum of at most 2^50 of them can overflow."""
    import math
    t = np.ascontiguousarray(terms, dtype=np.float64)
    fin = np.isfinite(t)
    assert np.all(np.abs(t[fin]) <= 8.0), "a finite term above 8: partial sums could overflow in some order"
    val, mag = np.where(fin, t, 0.0), np.where(fin, np.abs(t), 0.0)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)

    def count(mask):
        c = np.concatenate(([0], np.cumsum(mask)))
        return c[hi] - c[lo]

    n_nan, n_pos, n_neg, n_nonzero = count(np.isnan(t)), count(t == np.inf), count(t == -np.inf), count(mag != 0)
    # A is a scale, not a value: a difference of extended-precision prefix sums (summed directly where that difference would
    # lose a window of tiny terms), and exactly 0 where every term is a zero
    pa = np.concatenate(([0], np.cumsum(mag.astype(np.longdouble))))
    A = np.where(n_nonzero > 0, np.maximum((pa[hi] - pa[lo]).astype(np.float64), 0.0), 0.0)
    vals, mags = val.tolist(), mag.tolist()
    for w in np.flatnonzero((n_nonzero > 0) & (A < 1e-30)).tolist():
        A[w] = math.fsum(mags[lo[w]:hi[w]])
    want = np.where((n_nan > 0) | ((n_pos > 0) & (n_neg > 0)), np.nan, np.where(n_pos > 0, np.inf, np.where(n_neg > 0, -np.inf, 0.0)))
    for w in np.flatnonzero(want == 0.0).tolist():
        want[w] = math.fsum(vals[lo[w]:hi[w]]) + 0.0
    return want, A, np.isfinite(want)


def assert_sums(got, want, A, what):
    """THE comparison rule for a column of window sums: the NaN mask and the +-inf bits exact; a finite sum within
    1e-9 A + 1e-12, and exactly +0.0 where the window has no term but zeros (A == 0)."""
    got, want, A = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, want, A))
    assert got.shape == want.shape == A.shape, (what, got.shape, want.shape, A.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = int(np.flatnonzero(gn != wn)[0])
        raise AssertionError(f"{what}: NaN masks differ at {int((gn != wn).sum())} of {got.size} windows; first at {i}: got {got[i]!r}, want {want[i]!r}")
    exact = (np.isinf(want) | np.isinf(got) | (A == 0)) & ~wn
    bad = exact & (bits(got) != bits(want))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} infinite or all-zero sums differ in their bits; first at {i}: got {got[i]!r}, want {want[i]!r}")
    rest = ~wn & ~exact
    over = np.abs(got[rest] - want[rest]) - (REL_A * A[rest] + ABS_A)
    if over.size and over.max() > 0:
        i = int(np.flatnonzero(rest)[int(np.argmax(over))])
        raise AssertionError(f"{what}: {int((over > 0).sum())} sums beyond 1e-9 A + 1e-12; worst at {i}: got {got[i]!r}, want {want[i]!r}, A {A[i]!r}")


def windows_of(pairs):
    from popgenomicstools_amd._lib import WIN_DTYPE
    win = np.zeros(len(pairs), dtype=WIN_DTYPE)
    if len(pairs):
        win["lo"], win["hi"] = [a for a, _ in pairs], [b for _, b in pairs]
    return win


def site_windows(n, W, S):
    """windows of W sites every S sites that never cross the chromosome edge of two_chromosomes(n); the last ones are shorter"""
    n0 = (n + 1) // 2
    return windows_of([(a, min(a + W, end)) for start, end in ((0, n0), (n0, n)) for a in range(start, end, S)])


def one_site_windows(sites):
    return windows_of([(int(s), int(s) + 1) for s in sites])


def pops_tables(n=POPS_N, planted=POPS_PLANTED, with_one_site=True):
    """-> [(name, table)]: POPS_TABLES, the single window (0, n) and the one-site windows at the planted sites and their neighbours"""
    out = [(f"({W},{S})", site_windows(n, W, S)) for W, S in POPS_TABLES] + [("(0,n)", windows_of([(0, n)]))]
    if with_one_site:
        near = sorted({s + d for s in planted for d in (-1, 0, 1) if 0 <= s + d < n})
        out.append(("(1,1)", one_site_windows(near)))
    return out


def pops_clean_columns(n, k, seed, planted=POPS_PLANTED, count_hi=41):
    """frequencies j/1024 (synth.exact_freq_columns) and counts 0 ... 40; the planted sites are counted for every population;
    where a population is below POPS_MININD, one frequency in four is GARBAGE (NaN, +-inf, -5, 7): a site that is not counted
    is selected away, never multiplied by 0, in the clean run and in every planted one"""
    rng = np.random.default_rng(seed)
    f, _ = synth.exact_freq_columns(rng, n, k)
    c = [rng.integers(0, count_hi, n, dtype=np.int32) for _ in range(k)]
    for x, y in zip(c, f):
        x[list(planted)] = 9
        wild = np.flatnonzero((x < POPS_MININD) & (rng.random(n) < 0.25))
        y[wild] = rng.choice(np.array(GARBAGE), wild.size)
    return f, c


def pops_plant(f, plan, planted=POPS_PLANTED):
    """plan: {population: a value, or one value per planted site} -> a copy of the columns with them planted"""
    out = [x.copy() for x in f]
    for who, v in plan.items():
        out[who][list(planted)] = v
    return out


def pops_runs(stat, k):
    """-> [(name, plan)] of section 1 for one kernel: NaN in one ingroup population (for f_d as P1, P2 and P3 of trio 0), for the
    trio kernels NaN in the outgroup, +inf in population 1, and the in-contract edge values cycled over the planted sites of
    populations 0 and 1 (from different starts, so that a site's two values differ)"""
    m = len(POPS_PLANTED)
    edge = np.array(POPS_EDGE_VALUES)
    runs = [(f"NaN in population {who}", {who: NAN}) for who in ((0, 1, 2) if stat == "fd" else (1 if k > 1 else 0,))]
    if stat in ("dstat", "fd"):
        runs.append(("NaN in the outgroup", {k - 1: NAN}))
    runs.append(("+inf in population 1", {min(1, k - 1): INF}))
    runs.append(("edge values", {0: edge[np.arange(m) % edge.size], min(1, k - 1): edge[(np.arange(m) + 3) % edge.size]} if k > 1
                 else {0: edge[np.arange(m) % edge.size]}))
    return runs


# ---- denormal and zero sums in a row -----------------------------------------------------------------------------------------
DENORMAL_CASES = [("dstat", 4), ("fd", 4), ("fst_hudson", 3), ("dxy", 3)]
DENORMAL_N = 7 * 43  # 43 windows of 7 sites


def denormal_columns(k, seed=0):
    """Frequencies that are powers of two from 2^-1074 to 2^-1, or exactly 0, in groups of 7 sites (one 7-site window each), the
    groups cycling through five shapes: (0) exponents from the whole range; (1) every frequency at most 2^-1030: sums are
    denormal or underflow to 0; (2) every frequency 0: numerator and denominator sums are 0 and the ratio is 0.0, not NaN;
    (3) one site with P1 = P2 = 2^-3, P3 = 2^-1 and the outgroup 2^-2 — its f_d numerator term is exactly 0, its
    denominator terms are not — among sites of shape (1): a denormal numerator sum over a normal denominator sum, the quotient
    denormal; (4) exponents around -540: products of two frequencies are denormal, of three are 0.  Counts 5 ... 40, one site in
    eight uncounted for one population.  -> (f, c)"""
    rng = np.random.default_rng([seed, k])
    n = DENORMAL_N
    f = [np.zeros(n) for _ in range(k)]
    for g in range(n // 7):
        s = slice(7 * g, 7 * g + 7)
        shape = g % 5
        for p in range(k):
            if shape == 0:
                e = rng.choice(np.array([-1074, -1073, -1060, -1023, -1022, -1021, -600, -537, -300, -52, -20, -3, -2, -1]), 7)
            elif shape in (1, 3):
                e = rng.integers(-1074, -1029, 7)
            elif shape == 4:
                e = rng.integers(-545, -530, 7)
            else:
                e = None
            if e is not None:
                f[p][s] = np.ldexp(1.0, e)
                if shape != 3:
                    f[p][s][rng.random(7) < 0.2] = 0.0
        if shape == 3:
            at = 7 * g + int(rng.integers(0, 7))
            for p in range(k):
                f[p][at] = 2.0 ** -2
            f[0][at] = f[1][at] = 2.0 ** -3
            f[2 if k > 3 else 1][at] = 2.0 ** -1
    c = [rng.integers(5, 41, n, dtype=np.int32) for _ in range(k)]
    for i in np.flatnonzero(rng.random(n) < 1 / 8):
        c[int(rng.integers(0, k))][i] = 2
    return f, c


def denormal_tables():
    n = DENORMAL_N
    return [("one site", one_site_windows(range(n))), ("7 sites", windows_of([(a, a + 7) for a in range(0, n, 7)]))]


# ---- counts at their extremes, K populations -------------------------------------------------------------------------------
def extreme_counts_k(rng, n, minind, k):
    """extreme_counts for k columns: every count from {INT32_MIN, -1, 0, minind - 1, minind, INT32_MAX}"""
    vals = np.array(sorted({I32_MIN, -1, 0, max(minind - 1, I32_MIN), minind, I32_MAX}), dtype=np.int64).astype(np.int32)
    return [rng.choice(vals, size=n) for _ in range(k)]


REALISTIC_MININD = 1000


def realistic_counts_k(rng, n, k):
    """sample sizes of a large cohort: uniform in 1 ... 100 000 (about one count in a hundred is below REALISTIC_MININD)"""
    return [rng.integers(1, 100_001, n, dtype=np.int32) for _ in range(k)]


def count_case_columns(stat, k, minind, realistic=False):
    """-> (f, c) of section 3 for one kernel: frequencies j/1024, counts at their extremes (or realistic ones)"""
    rng = np.random.default_rng([31, k, minind % 1000, len(stat), int(realistic)])
    f, _ = synth.exact_freq_columns(rng, POPS_N, k)
    return f, (realistic_counts_k(rng, POPS_N, k) if realistic else extreme_counts_k(rng, POPS_N, minind, k))


def counted_site_table(stat, k, c, minind, m=300):
    """one-site windows at up to m sites counted for the call's first item and up to m counted for its last"""
    items = pops_items(stat, k)
    sites = set()
    for item in (items[0], items[-1]):
        at = np.flatnonzero(pops_counted(item, c, minind))
        sites |= set(at[np.linspace(0, at.size - 1, min(m, at.size)).astype(np.int64)].tolist()) if at.size else set()
    return one_site_windows(sorted(sites))


def exact_site(stat, fs, cs):
    """The header's per-site definition of a VALUE statistic in exact rationals, for one counted site of one item.  fs, cs: the
    item's frequencies (floats, taken at their exact value) and counts.  -> [(value, scale)] per sum of POPS_SUMS[stat], the
    scale being the Σ|.| of the definition's subterms"""
    from fractions import Fraction
    p = [Fraction(float(x)) for x in fs]
    n = [int(x) for x in cs]
    if stat == "pi":
        v = (2 * p[0]) * (1 - p[0]) * Fraction(2 * n[0], 2 * n[0] - 1)
        return [(v, abs(v))]
    if stat == "fst_hudson":
        h = [p[x] * (1 - p[x]) / (2 * n[x] - 1) for x in (0, 1)]
        d2 = (p[0] - p[1]) ** 2
        x, y = p[0] * (1 - p[1]), p[1] * (1 - p[0])
        return [(d2 - h[0] - h[1], d2 + abs(h[0]) + abs(h[1])), (x + y, abs(x) + abs(y))]
    assert stat == "fst"
    n1, n2 = n
    f1, f2 = p
    npool = n1 + n2
    fpool = (n1 * f1 + n2 * f2) / npool
    b = (n1 * 2 * f1 * (1 - f1) + n2 * 2 * f2 * (1 - f2)) / (npool - 1)
    div = Fraction(4 * n1 * n2, npool)
    t = [4 * n1 * (f1 - fpool) ** 2 / div, 4 * n2 * (f2 - fpool) ** 2 / div, b / div]
    a, sa = t[0] + t[1] - t[2], abs(t[0]) + abs(t[1]) + abs(t[2])
    return [(a, sa), (a + b, sa + abs(b))]


def assert_within_exact(got, exact, what):
    """got: floats; exact: [(value, scale)] of exact_site -> every |got - value| <= 1e-9 scale + 1e-12, in exact arithmetic"""
    from fractions import Fraction
    for i, (g, (v, s)) in enumerate(zip(got, exact)):
        g = float(g)
        assert g == g and abs(g) != float("inf"), (what, i, g)
        assert abs(Fraction(g) - v) <= Fraction(REL_A) * s + Fraction(ABS_A), (what, i, g, float(v), float(s))


# ---- jackknife weights beyond 2^32 ---------------------------------------------------------------------------------------------
JACK_U32_N_WIN = (129, 64 * 64 + 1)  # dstat_jack_shapes.N_WIN_PARTIALS_ABOVE_64
JACK_U32_TRIOS = 4
_jack_u32 = {}


def jack_u32_rows(n_win, n_trios=JACK_U32_TRIOS):
    """dstat_jack_shapes.synth_rows with every used block's weight n = 0xFFFFFFFF (about one block in seven unused: n = 0, NaN
    sums): Σn passes 2^32 at the second used block.  Equal weights on purpose: h_j = g for every block and amplifies no
    rounding.  Read-only, made once."""
    import dstat_jack_shapes
    if (n_win, n_trios) not in _jack_u32:
        rows = dstat_jack_shapes.synth_rows(n_win, n_trios, seed=1).copy()
        rows["n"] = np.where(rows["n"] > 0, 0xFFFFFFFF, 0).astype(np.uint32)
        rows.setflags(write=False)
        _jack_u32[(n_win, n_trios)] = rows
    return _jack_u32[(n_win, n_trios)]


JACK_U32_GOLDEN_N_WIN = JACK_U32_N_WIN[1]  # recorded by tests/golden/make_dstat_jack_u32_exact.py
_jack_u32_exact = {}


def jack_u32_exact(n_win):
    """[JACK_U32_TRIOS][3] dicts (d, d_jack, se, z, n_sites, n_blocks) of jack_u32_rows(n_win) from the exact-rational model:
    evaluated here for 129 blocks, read from tests/golden/dstat_jack_u32_exact.json (the same evaluation, recorded) for 4 097."""
    import dstat_jack_model
    import helpers
    if n_win not in _jack_u32_exact:
        if n_win == JACK_U32_GOLDEN_N_WIN:
            rec = helpers.load_golden("dstat_jack_u32_exact.json")
            assert rec["n_win"] == n_win and rec["n_trios"] == JACK_U32_TRIOS and rec["seed"] == 1
            _jack_u32_exact[n_win] = [[{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in item.items()} for item in trio]
                                      for trio in rec["items"]]
        else:
            rows = jack_u32_rows(n_win)
            _jack_u32_exact[n_win] = [[{k: v for k, v in item.items() if k != "var"} for item in dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_exact)]
                                      for t in range(JACK_U32_TRIOS)]
    return _jack_u32_exact[n_win]
