"""The selection between the two fst build kernels, restated in Python (fst_build_launch in csrc/pgt_kernels.hip; the constants
are held to the literal definitions of the sources by tests/test_fst_deep_stage_cpu.py).

The fst build walks level-2 tiles of 8192 sites with build_grid(tiles, cap): r = ceil(tiles / (4 cap)) rounds, ceil(tiles / r)
waves asked for, whole workgroups of 4 waves launched.  cap is kFstBuildBlocks unless PGT_FST_BUILD_BLOCKS (read when a context is
opened) lowers it.  More than kFstStage rounds: the deep-stage kernel (FstDeepStage: kFstDeepLdsRows rows in LDS, kFstDeepBlocks
register blocks of kFstDeepBlockRows rows).  With the knob at 1 the grid is one workgroup, so 4 waves walk the column and a wave
walks `rounds` tiles of a column of 4 * rounds tiles."""
TILE = 8192
FST_BUILD_BLOCKS = 512   # kFstBuildBlocks
FST_STAGE = 16           # kFstStage: rounds up to which fst_build_kernel<> runs
DEEP_LDS_ROWS = 20       # kFstDeepLdsRows
DEEP_BLOCKS = 4          # kFstDeepBlocks
DEEP_BLOCK_ROWS = 11     # kFstDeepBlockRows
DEEP_ROWS = DEEP_LDS_ROWS + DEEP_BLOCKS * DEEP_BLOCK_ROWS  # C = kFstDeepStage: rows a wave holds before it has to write
KNOB = "PGT_FST_BUILD_BLOCKS"


def cap_of(knob=None):
    """fst_build_cap: the knob's value where it lies in 1 .. kFstBuildBlocks - 1, else kFstBuildBlocks"""
    return knob if knob is not None and 1 <= knob < FST_BUILD_BLOCKS else FST_BUILD_BLOCKS


def tiles_of(n):
    return max(1, -(-n // TILE))


def rounds_of(n, knob=None):
    """build_rounds: the most tiles a wave walks"""
    return -(-tiles_of(n) // (4 * cap_of(knob)))


def grid_waves(n, knob=None):
    """waves of the launched grid (the stride of a wave's walk)"""
    tiles = tiles_of(n)
    waves = -(-tiles // rounds_of(n, knob))
    return 4 * (-(-waves // 4))


def deep(n, knob=None):
    return rounds_of(n, knob) > FST_STAGE


def tiles_of_wave(n, knob=None):
    tiles, nw = tiles_of(n), grid_waves(n, knob)
    return [len(range(w, tiles, nw)) for w in range(nw)]


def full_n(rounds):
    """the column with which each of the knob's 4 waves walks exactly `rounds` whole tiles"""
    return 4 * rounds * TILE


def ragged_n(rounds):
    """4 * rounds - 1 tiles (the last wave walks rounds - 1), the last tile partial: it ends 4 sites into its 33rd leaf, so n is a
    multiple neither of 8192 nor of 128"""
    return (4 * rounds - 2) * TILE + 32 * 128 + 4


# rounds per wave with the knob at 1.  16: the last size of fst_build_kernel<>; 17: the first of the deep kernel (one block
# parked, 6 rows in LDS).  A block is parked when the LDS rows hold kFstDeepBlockRows rows (after rows 11, 22, 33 and 44): at 22, 33
# and 44 the final flush finds 2, 3 and 4 blocks and no row in LDS, at 23, 34 and 45 one row in LDS behind them; 49: where a layout
# of 16-row blocks would park its third.  C - 1 and C rows: the final flush alone (C fills the LDS rows and is written by the flush
# in put()); C + 1 and 2C + 3: one and two full flushes, then a partial one.
ROUNDS = (16, 17, 22, 23, 33, 34, 44, 45, 49, DEEP_ROWS - 1, DEEP_ROWS, DEEP_ROWS + 1, 2 * DEEP_ROWS + 3)
RAGGED_ROUNDS = (17, DEEP_ROWS + 1)
PAIRS_ROUNDS = 33
