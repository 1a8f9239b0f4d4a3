"""GPU: pgt_pbs_pops_reduce_dev / pgt_pbs_hudson_pops_reduce_dev at the sizes where a build wave walks a SECOND level-2 tile
and a query wave answers a SECOND item — the grid strides of pgt_pops_walk.h that the other PBS tests leave at one turn (their
longest column has 74 tiles, their largest table a few thousand rows).  PBS walks the columns twice through that walk: the
second pass rebuilds the tree the first one left and writes its own scratch rows, so a stale node or a skipped tile of the second
pass shows in the den_* sums alone — all six sums are compared, never num_ij only.  The sizes come from the launch arithmetic
restated in tests/pops_grid_shapes.py, taken at PbsPass' own kOneWaveFrom = 5 and kQueryOneWaveFrom = 6
(tests/test_pbs_pops_cpu.py holds the constants to the literals in csrc/).

Build: the smallest tile counts that give two rounds at both occupancies — 1025 at the one-wave K = 5 (1024 build waves at
most), 2049 at the two-wave K = 3 (2048) — crossed once with the two estimators (the estimator changes site(), not the walk),
with a ragged last tile, the table pops_grid_shapes.second_round_windows, and the model evaluated on those ranges only.
Query: QUERY_N_WIN[-1] = QUERY_WAVES + 5 rows of pops_grid_shapes.strided_query_table, so that five waves answer a second item
(six with the genome-wide line) and pbs_finish_kernel runs 262 150 threads over scratch rows written on that second turn; K = 3
(T = 1) under both estimators, and K = 6 (the query kernel at one wave per SIMD, T = 20 scratch tables) once.
Bounds as tests/test_pbs_pops.py: counts and coordinates exact, sums within 1e-9 A + 1e-12, the finishing arithmetic through
assert_finish, one-site rows bit for bit under Hudson."""
import numpy as np
import pytest

import pbs_pops_model
import pops_grid_shapes as shapes
import synth
from pbs_pops_model import SUMS, all_trio_order
from popgenomicstools_amd.window_scan import run_lengths
from test_fst_pops import MININD, _t, random_pops
from test_pbs_pops import assert_rows, assert_totals, bits, pops_dev

pytestmark = pytest.mark.gpu
ONE_WAVE_FROM = 5        # PbsPass::kOneWaveFrom
QUERY_ONE_WAVE_FROM = 6  # PbsPass::kQueryOneWaveFrom


def build_grid(tiles, k):
    return shapes.balanced_build(tiles, shapes.ONE_WAVE_BUILD_WAVES if k >= ONE_WAVE_FROM else shapes.MAX_BUILD_WAVES)


def assert_one_site_bits(rows, want, one, est, what):
    """Hudson: every operation of the per-site lines is a float64 operation of its own, so a one-site row carries the model's bits"""
    if est == "hudson":
        for fld in SUMS:
            assert np.array_equal(bits(rows[fld][one]), bits(want[fld][one])), (what, fld)


@pytest.mark.parametrize("est,k,tiles,grid", [("wc", 5, 1025, (2, 513, 516)), ("hudson", 3, 2049, (2, 1025, 1028))],
                         ids=["wc-one-wave-K5", "hudson-two-wave-K3"])
def test_a_build_waves_second_tile(pgt, ctx, est, k, tiles, grid):
    rounds, waves, n_waves = build_grid(tiles, k)
    assert (rounds, waves, n_waves) == grid and shapes.tiles_of_wave(tiles, n_waves).max() == 2
    assert build_grid(tiles - 1, k)[0] == 1  # the smallest count with two rounds at this occupancy
    n = shapes.ragged_n(tiles)
    rng = np.random.default_rng(5250 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win, names = shapes.second_round_windows(n, tiles, n_waves)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est)
    want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est, ranges_only=True)
    one = (win["hi"] - win["lo"]) == 1
    assert one.sum() >= 19
    for t, ijk in enumerate(all_trio_order(k)):
        assert_rows(rows[t], want[t], A, t, f"{est} K={k} second tile, trio {ijk}", quiet=t > 0)  # all six sums: both passes
        assert_one_site_bits(rows[t], want[t], one, est, (names, ijk))
        assert np.any(rows[t]["n"][one] > 0), ijk
    assert_totals(tot, want_t, A_tot, f"{est} K={k} second tile, totals")


def query_inputs(pgt, k, seed):
    n = 270_000
    rng = np.random.default_rng(seed)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = shapes.strided_query_table(pgt.build_windows_sites(run_lengths(chr_ids), 7, 1))
    assert win.size == shapes.QUERY_WAVES + 5 == shapes.QUERY_N_WIN[-1]
    return pos, f, c, win


@pytest.mark.parametrize("est", ["wc", "hudson"])
def test_a_query_waves_second_item(pgt, ctx, est):
    k = 3
    assert k < QUERY_ONE_WAVE_FROM
    pos, f, c, win = query_inputs(pgt, k, 5350)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est)
    one = (win["hi"] - win["lo"]) == 1
    tail = slice(shapes.QUERY_WAVES, None)
    for with_tot in (True, False):  # with the genome-wide lines the total is one more item: a sixth wave's second
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est, **({} if with_tot else {"tot": False}))
        assert_rows(rows[0], want[0], A, 0, f"{est} second item, totals {with_tot}", quiet=False)
        assert_one_site_bits(rows[0], want[0], one, est, f"second item, totals {with_tot}")
        assert np.any(rows[0]["n"][tail] > 0) and np.any(~one[tail]) and np.any(one[tail])
        if with_tot:
            assert_totals(tot, want_t, A_tot, f"{est} second item, totals")
        else:
            assert tot is None


def test_a_query_waves_second_item_at_one_wave_per_simd(pgt, ctx):
    """K = 6: the query kernel compiled from kQueryOneWaveFrom, 20 scratch tables of 262 149 rows per pass"""
    k, est = 6, "hudson"
    assert k >= QUERY_ONE_WAVE_FROM
    pos, f, c, win = query_inputs(pgt, k, 5356)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, est)
    want, want_t, A, A_tot = pbs_pops_model.model(pos, f, c, MININD, win, est)
    one = (win["hi"] - win["lo"]) == 1
    tail = slice(shapes.QUERY_WAVES, None)
    trios = all_trio_order(k)
    for t, ijk in enumerate(trios):
        assert np.array_equal(rows[t]["n"], want[t]["n"]), ijk
        assert np.any(rows[t]["n"][tail] > 0), ijk
    for t in (0, len(trios) - 1):
        assert_rows(rows[t], want[t], A, t, f"{est} K={k} second item, trio {trios[t]}", quiet=False)
        assert_one_site_bits(rows[t], want[t], one, est, trios[t])
    assert_totals(tot, want_t, A_tot, f"{est} K={k} second item, totals")
