"""Seeded synthetic inputs shaped as BASELINE.md defines them (numpy, host side)."""
import numpy as np


def chromosomes(rng, n_sites, n_chr, equal=True):
    """-> (chr_ids u32[n], pos u32[n]); pos = running sum of U{1..59} gaps per chromosome."""
    if equal:
        base = n_sites // n_chr
        lens = np.full(n_chr, base, dtype=np.int64)
        lens[: n_sites - base * n_chr] += 1
    else:
        cuts = np.sort(rng.choice(np.arange(1, n_sites), size=n_chr - 1, replace=False)) if n_chr > 1 else np.array([], dtype=np.int64)
        lens = np.diff(np.concatenate(([0], cuts, [n_sites])))
    lens = lens[lens > 0]
    chr_ids = np.repeat(np.arange(lens.size, dtype=np.uint32), lens)
    gaps = rng.integers(1, 60, size=n_sites, dtype=np.int64)
    csum = np.cumsum(gaps)
    starts = np.concatenate(([0], np.cumsum(lens)[:-1]))
    offset = np.repeat(np.concatenate(([0], csum[np.cumsum(lens)[:-1] - 1])), lens)
    pos = (csum - offset).astype(np.uint32)
    return chr_ids, pos


def fst_columns(rng, n):
    b = np.round(rng.uniform(0.0, 0.3, n), 6)
    a = np.round(b * rng.uniform(-0.1, 0.6, n), 6)
    return a, b


def het_column(rng, n):
    return rng.choice(np.array([0, 1, 2, -1], dtype=np.int32), size=n, p=[0.5, 0.3, 0.15, 0.05])


def dxy_columns(rng, n):
    p1 = np.round(rng.uniform(0, 1, n), 6)
    p2 = np.round(rng.uniform(0, 1, n), 6)
    n1 = rng.integers(0, 21, n, dtype=np.int32)
    n2 = rng.integers(0, 21, n, dtype=np.int32)
    return p1, p2, n1, n2


# ---- exact (dyadic) columns: every partial sum is exact in any order, so every query strategy, hint and workspace content must
# give the same bits, equal to integer prefix sums.  The integer arrays are in units of EXACT_UNIT (FST_UNIT for the fst columns).
EXACT_UNIT = 2.0 ** -20
FST_UNIT = 2.0 ** -24


def exact_fst_columns(rng, n):
    """a = k/4096 (k in [-600, 2400]) and b = k/4096 >= 0 (zero at about one site in eight); at about one site in 64, and at the
    last site, a and b are instead a few units of 2^-24: below 1e-9 of the sum of any window of a few thousand sites, so only
    an exact comparison sees such a site dropped or counted twice.  Partial sums stay below 2^29: exact.
    -> (a, b, ka, kb) with a = ka * 2^-24, b = kb * 2^-24."""
    ka = rng.integers(-600, 2401, n).astype(np.int64) * 4096
    kb = rng.integers(0, 2401, n).astype(np.int64) * 4096
    kb[rng.random(n) < 0.125] = 0
    tiny = rng.random(n) < 1 / 64
    tiny[-1:] = True
    ka[tiny] = rng.integers(-3, 4, int(tiny.sum()))
    kb[tiny] = rng.integers(0, 4, int(tiny.sum()))
    return ka * FST_UNIT, kb * FST_UNIT, ka, kb


def exact_dxy_columns(rng, n):
    """p1, p2 = k/1024: p1(1-p2) + p2(1-p1) is exact (20 fractional bits).  -> (p1, p2, n1, n2, k1, k2)"""
    k1 = rng.integers(0, 1025, n).astype(np.int64)
    k2 = rng.integers(0, 1025, n).astype(np.int64)
    n1 = rng.integers(0, 21, n, dtype=np.int32)
    n2 = rng.integers(0, 21, n, dtype=np.int32)
    return k1 / 1024.0, k2 / 1024.0, n1, n2, k1, k2


def exact_freq_columns(rng, n, n_pops):
    """Allele frequencies k/1024: 2f(1-f) and (f_i - f_j)^2 are exact.  -> (list of f64 columns, list of int64 k)"""
    ks = [rng.integers(0, 1025, n).astype(np.int64) for _ in range(n_pops)]
    return [k / 1024.0 for k in ks], ks


def tied_scores(rng, n):
    """Scores k/16 in [-5, 5]: many ties, in value and in |value|, and values equal to the cutoffs 2 and -2."""
    return rng.integers(-80, 81, n) / 16.0
