"""No GPU: the shapes of tests/test_pops_grid_stride.py are derived from caps that csrc/ defines (tests/pops_grid_shapes.py
restates them).  If a cap changes, the GPU tests would silently drop back to one tile per build wave or one item per query
wave; this module fails instead and names the shapes to update."""
import os
import re

import numpy as np
import pytest

import pops_grid_shapes as shapes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "popgenomicstools_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _has(text, literal):
    """the literal with any run of blanks between its tokens"""
    return re.search(r"\s+".join(re.escape(tok) for tok in literal.split()), text) is not None


def test_the_caps_are_the_literal_definitions_of_the_sources():
    internal, common, af = _src("pgt_internal.h"), _src("pgt_pops_common.h"), _src("pgt_af_kernels.hip")
    kernels = _src("pgt_kernels.hip")
    update = "update tests/pops_grid_shapes.py and the sizes of tests/test_pops_grid_stride.py"
    assert _has(internal, f"kMaxBuildWaves = {shapes.MAX_BUILD_WAVES};"), update
    assert _has(common, f"one_wave_per_simd ? {shapes.ONE_WAVE_BUILD_WAVES}"), update
    assert _has(common, f"b > {shapes.QUERY_MAX_BLOCKS} ? {shapes.QUERY_MAX_BLOCKS}"), update
    assert _has(af, f"NP == 2 ? {shapes.AF_CAP_BLOCKS[True]} : {shapes.AF_CAP_BLOCKS[False]}"), update
    # what else the restated arithmetic rests on
    assert _has(af, f'env_int("PGT_AF_ONE_WAVE_FROM", {shapes.AF_ONE_WAVE_FROM})'), update
    assert _has(af, "resident = w1 ? 256 : 512"), update
    assert _has(af, f"r < r0 + {shapes.AF_ROUND_CANDIDATES}") and _has(af, f"fill > best + {shapes.AF_FILL_MARGIN}"), update
    assert _has(kernels, f"kFstBuildBlocks = {shapes.MAX_BUILD_WAVES // 4};"), update
    for name in ("pgt_dxy_pops_kernels.hip", "pgt_fst_pops_kernels.hip", "pgt_dstat_pops_kernels.hip"):
        assert _has(_src(name), f"constexpr int kOneWaveFrom = {shapes.POPS_ONE_WAVE_FROM};"), (name, update)
    assert shapes.TILE == 128 * 64 and shapes.LEAF * 16 == shapes.TILE and shapes.QUERY_WAVES == 262_144


@pytest.mark.parametrize("entry,n_pops,tiles,grid,rounds,waves,n_waves", shapes.BUILD_CASES,
                         ids=[f"{c[0]}-K{c[1]}-{c[2]}" for c in shapes.BUILD_CASES])
def test_every_build_case_reaches_a_second_tile(entry, n_pops, tiles, grid, rounds, waves, n_waves):
    assert grid(tiles, n_pops) == (rounds, waves, n_waves)
    assert rounds >= 2 and (rounds == 2 or (entry, n_pops) == ("fst_af", 3))
    assert grid(tiles - 1, n_pops)[0] == 1, "one tile fewer is the last size of one round: the case is the smallest"
    # the padding of the last workgroup: 3 waves (1 at the AF front end's 1639 waves).  The loops stride by the waves of
    # the GRID, so these waves are not idle: they take a first-round tile and no later one
    assert n_waves - waves == (1 if (entry, n_pops) == ("fst_af", 3) else 3)
    per_wave = shapes.tiles_of_wave(tiles, n_waves)
    assert per_wave.sum() == tiles and per_wave.min() >= rounds - 1 and per_wave.max() == rounds
    assert np.all(per_wave[waves:] == rounds - 1)
    assert per_wave[(tiles - 1) % n_waves] == rounds and (tiles - 1) // n_waves == rounds - 1, "the partial last tile is a wave's last of several"
    n = shapes.ragged_n(tiles)
    assert -(-n // shapes.TILE) == tiles and n % shapes.TILE == 4100 and n % shapes.LEAF == 4
    win, names = shapes.second_round_windows(n, tiles, n_waves)
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert np.all((0 <= lo) & (lo < hi) & (hi <= n)) and len(names) == win.size == 24
    first = n_waves * shapes.TILE
    assert np.count_nonzero((hi - lo == 1) & (lo >= first) & (hi <= first + shapes.TILE)) == 17, "a site in every leaf of the tile"
    assert np.any((lo == first) & (hi == first + shapes.TILE))
    assert np.any((-(-lo // shapes.LEVEL3) < hi // shapes.LEVEL3) & (lo > first) & (hi < n)), "a level-3 node of the second round"


def test_the_query_table_strides():
    n = 270_000
    w7 = shapes.one_site_table(np.arange(n - 6))
    w7["hi"] += 6
    table = shapes.strided_query_table(w7)
    assert table.size == shapes.QUERY_N_WIN[-1] == shapes.QUERY_WAVES + 5
    assert shapes.QUERY_N_WIN == (262_143, 262_144, 262_149)
    length = (table["hi"] - table["lo"]).astype(np.int64)
    second = length[shapes.QUERY_WAVES:]
    assert set(second.tolist()) == {1, 7} and set(length[:shapes.QUERY_WAVES].tolist()) == {1, 7}
    assert int(table["hi"].max()) <= n
