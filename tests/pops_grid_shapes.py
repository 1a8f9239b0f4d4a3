"""The launch arithmetic of the all-pairs front ends, restated in Python: which column lengths make a build wave take a second
level-2 tile and which table sizes make a query wave take a second item (tests/test_pops_grid_stride.py runs them on the GPU,
tests/test_pops_grid_stride_cpu.py holds the constants below to the literal definitions in csrc/).

Build (pgt_*_pops_kernels.hip, pgt_af_kernels.hip, pi_build_kernel): `for (t = wave0; t < n_l2; t += n_waves)`, n_waves the
waves of the GRID (4 per workgroup), so the waves that pad the last workgroup take a first-round tile like any other.
Query: `for (w = wave0; w < n_items; w += n_waves)` with n_items = n_win + (tot ? 1 : 0)."""
import numpy as np

from popgenomicstools_amd._lib import WIN_DTYPE

TILE = 8192                 # sites of a level-2 tile (tree_layout(PGT_STAT_FST, n): 128-site leaves, radix 64)
LEAF = 512                  # sites of a level-1 node of the all-pairs trees
LEVEL3 = TILE * 64          # sites of a level-3 node
MAX_BUILD_WAVES = 2048      # kMaxBuildWaves (pgt_internal.h): the two-waves-per-SIMD build, and 4 * kFstBuildBlocks of pi_build_kernel
ONE_WAVE_BUILD_WAVES = 1024  # pops_build_grid (pgt_pops_common.h), one wave per SIMD
POPS_ONE_WAVE_FROM = 5      # kOneWaveFrom of the three (freq, nInd) front ends
QUERY_MAX_BLOCKS = 65536    # wave_grid (pgt_pops_common.h)
QUERY_WAVES = 4 * QUERY_MAX_BLOCKS  # 262 144: from this many items on a query wave takes a second one
AF_CAP_BLOCKS = {True: 512, False: 2048}  # launch_af_np: `NP == 2 ? 512 : 2048`
AF_ONE_WAVE_FROM = 4        # af_one_wave_from()'s default: resident workgroups 256 from there, 512 below
AF_ROUND_CANDIDATES = 4     # launch_af_np tries r0 .. r0 + 3 rounds
AF_FILL_MARGIN = 0.02       # and takes a longer round only for a last generation fuller by this much


def ragged_n(tiles):
    """the column length of `tiles` level-2 tiles whose last tile is partial and ends four sites into its ninth leaf"""
    return tiles * TILE - TILE + 4097 + 3


def _grid(tiles, rounds):
    waves = -(-tiles // rounds)
    return rounds, waves, 4 * (-(-waves // 4))


def balanced_build(tiles, max_waves):
    """pops_build_grid / build_grid -> (rounds, waves asked for, waves of the grid)"""
    return _grid(tiles, -(-tiles // max_waves))


def pops_build(tiles, n_pops):
    return balanced_build(tiles, ONE_WAVE_BUILD_WAVES if n_pops >= POPS_ONE_WAVE_FROM else MAX_BUILD_WAVES)


def generic_build(tiles):
    return balanced_build(tiles, MAX_BUILD_WAVES)


def af_build(tiles, n_pops):
    """launch_af_np's round chooser: among r0 .. r0 + 3 rounds the one whose last generation of resident workgroups is fullest"""
    max_waves = 4 * AF_CAP_BLOCKS[n_pops == 2]
    resident = 256 if n_pops >= AF_ONE_WAVE_FROM else 512
    r0 = -(-tiles // max_waves)
    rounds, best = r0, -1.0
    for r in range(r0, r0 + AF_ROUND_CANDIDATES):
        wg = -(-(-(-tiles // r)) // 4)
        gens = -(-wg // resident)
        fill = wg / (gens * resident)
        if fill > best + AF_FILL_MARGIN:
            best, rounds = fill, r
    return _grid(tiles, rounds)


def tiles_of_wave(tiles, n_waves):
    """how many tiles each wave of the grid walks"""
    return np.array([len(range(w, tiles, n_waves)) for w in range(n_waves)])


# section 1 of the GPU module: (entry point, populations, tiles, grid function, rounds, waves asked for, waves of the grid)
BUILD_CASES = [
    ("dxy_pops", 5, 1025, pops_build, 2, 513, 516),
    ("fst_pops", 5, 1025, pops_build, 2, 513, 516),
    ("fst_hudson_pops", 5, 1025, pops_build, 2, 513, 516),
    ("dstat_pops", 5, 1025, pops_build, 2, 513, 516),
    ("dxy_pops", 3, 2049, pops_build, 2, 1025, 1028),
    ("fst_pops", 3, 2049, pops_build, 2, 1025, 1028),
    ("fst_hudson_pops", 3, 2049, pops_build, 2, 1025, 1028),
    ("dstat_pops", 4, 2049, pops_build, 2, 1025, 1028),
    ("fst_af", 2, 2049, af_build, 2, 1025, 1028),
    # 8193 tiles are the fewest that pass the cap of 2048 workgroups (r0 = 2); of 2 .. 5 rounds the chooser takes 5: 410
    # workgroups fill 80 % of the one generation of 512, where 2 rounds fill 67 % of three
    ("fst_af", 3, 8193, af_build, 5, 1639, 1640),
    ("pi_pops", 1, 2049, lambda tiles, n_pops: generic_build(tiles), 2, 1025, 1028),
]


def grid_of(entry, n_pops, tiles):
    for e, k, t, fn, *_ in BUILD_CASES:
        if (e, k, t) == (entry, n_pops, tiles):
            return fn(tiles, n_pops)
    raise KeyError((entry, n_pops, tiles))


def _table(ranges):
    win = np.zeros(len(ranges), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [r[0] for r in ranges], [r[1] for r in ranges]
    return win


def second_round_windows(n, tiles, n_waves):
    """The explicit ranges of section 1, from the launch arithmetic: tile `n_waves` is the first tile of the second round
    (wave 0's second).  -> (table, names)"""
    first = n_waves * TILE  # the first site a second-round tile holds
    assert tiles > n_waves + 1 and n == ragged_n(tiles)
    node3 = -(-first // LEVEL3)  # the first level-3 node that lies in the second round as a whole
    assert (node3 + 1) * LEVEL3 + 1313 <= n
    named = [("the last site of a first-round tile", first - 1, first), ("the first site of the second round", first, first + 1),
             ("the last site", n - 1, n)]
    named += [(f"one site of leaf {q} of tile {n_waves}", first + q * LEAF + (37 * q + 5) % LEAF, first + q * LEAF + (37 * q + 5) % LEAF + 1)
              for q in range(TILE // LEAF)]
    named += [(f"tile {n_waves} alone", first, first + TILE),
              (f"tiles {n_waves - 1} .. {n_waves + 1} and 100 sites on each side", first - TILE - 100, first + 2 * TILE + 100),
              (f"level-3 node {node3} and ragged ends", node3 * LEVEL3 - 777, (node3 + 1) * LEVEL3 + 1313),
              ("the whole column", 0, n), ("the partial last tile", (tiles - 1) * TILE, n)]
    return _table([(lo, hi) for _, lo, hi in named]), [name for name, _, _ in named]


def one_site_table(sites):
    sites = np.asarray(sites, dtype=np.uint64)
    win = np.zeros(sites.size, dtype=WIN_DTYPE)
    win["lo"], win["hi"] = sites, sites + 1
    return win


def strided_query_table(w7):
    """Section 2: 262 149 rows of which the last five are second items of waves 0 .. 4.  The two kinds of window alternate
    in blocks, so that one-site rows AND windows of 7 sites (w7: build_windows_sites(run_len, 7, 1)) lie on both sides of row
    262 144: rows 0 .. 131 072 one site each, then 131 073 windows of 7 sites (rows 262 144 and 262 145 are the last two), then
    one-site rows again."""
    half = QUERY_WAVES // 2 + 1
    assert w7.size >= half
    table = np.concatenate([one_site_table(np.arange(half)), w7[:half], one_site_table(np.arange(half, half + 64))])
    return table[:QUERY_WAVES + 5]


QUERY_N_WIN = (QUERY_WAVES - 1, QUERY_WAVES, QUERY_WAVES + 5)
