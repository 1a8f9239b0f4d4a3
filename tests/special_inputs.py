"""Inputs with NaN, infinite and full-range values for tests/test_special_values.py (GPU) and the CPU check of their
expectations (tests/test_special_values_cpu.py).  numpy, host side; nothing here touches the product."""
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
