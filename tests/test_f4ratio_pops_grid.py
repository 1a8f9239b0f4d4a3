"""GPU: pgt_f4ratio_pops_reduce_dev at the sizes where a build wave walks a SECOND level-2 tile and a query wave answers a
SECOND item — the grid strides the other f4-ratio tests leave at one turn.  The sizes come from the launch arithmetic restated
in tests/pops_grid_shapes.py, taken at F4RatioPops' own kOneWaveFrom = 6 (tests/test_f4ratio_pops_cpu.py holds the constants to
the literal in csrc/).

Build: the smallest tile counts that give two rounds at both occupancies — 1025 at the one-wave K = 6 (1024 build waves at
most), 2049 at the two-wave K = 5 (2048) — with a ragged last tile, the table pops_grid_shapes.second_round_windows, and the
model evaluated on those ranges only.
Query: QUERY_N_WIN[-1] = QUERY_WAVES + 5 rows of pops_grid_shapes.strided_query_table, so that five waves answer a second item.
Bounds as tests/test_f4ratio_pops.py: counts and coordinates exact, sums within 1e-9 A + 1e-12, one-site rows bit for bit."""
import numpy as np
import pytest

import f4ratio_pops_model as model
import pops_grid_shapes as shapes
import synth
from f4ratio_pops_model import SUMS, middle_triple_order
from popgenomicstools_amd.window_scan import run_lengths
from test_f4ratio_pops import assert_rows, assert_totals, bits, pops_dev
from test_fst_pops import MININD, _t, random_pops

pytestmark = pytest.mark.gpu
ONE_WAVE_FROM = 6  # F4RatioPops::kOneWaveFrom


def build_grid(tiles, k):
    return shapes.balanced_build(tiles, shapes.ONE_WAVE_BUILD_WAVES if k >= ONE_WAVE_FROM else shapes.MAX_BUILD_WAVES)


@pytest.mark.parametrize("k,tiles,grid", [(6, 1025, (2, 513, 516)), (5, 2049, (2, 1025, 1028))], ids=["one-wave-K6", "two-wave-K5"])
def test_a_build_waves_second_tile(pgt, ctx, k, tiles, grid):
    rounds, waves, n_waves = build_grid(tiles, k)
    assert (rounds, waves, n_waves) == grid and shapes.tiles_of_wave(tiles, n_waves).max() == 2
    assert build_grid(tiles - 1, k)[0] == 1  # the smallest count with two rounds at this occupancy
    n = shapes.ragged_n(tiles)
    rng = np.random.default_rng(8250 + k)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win, names = shapes.second_round_windows(n, tiles, n_waves)
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win)
    want, want_t, A, A_tot = model.model(pos, f, c, MININD, win, ranges_only=True)
    one = (win["hi"] - win["lo"]) == 1
    assert one.sum() >= 19
    for t, q in enumerate(middle_triple_order(k)):
        assert_rows(rows[t], want[t], A, t, f"K={k} second tile, triple {q}", quiet=t > 0)
        for fld in SUMS:
            assert np.array_equal(bits(rows[t][fld][one]), bits(want[t][fld][one])), (names, q, fld)
    assert_totals(tot, want_t, A_tot, f"K={k} second tile, totals")


def test_a_query_waves_second_item(pgt, ctx):
    n, k = 270_000, 5
    rng = np.random.default_rng(8350)
    chr_ids, pos = synth.chromosomes(rng, n, 1)
    f, c = random_pops(rng, n, k)
    win = shapes.strided_query_table(pgt.build_windows_sites(run_lengths(chr_ids), 7, 1))
    assert win.size == shapes.QUERY_WAVES + 5 == shapes.QUERY_N_WIN[-1]
    tp, tf, tn = _t(pos), [_t(x) for x in f], [_t(x) for x in c]
    want, want_t, A, A_tot = model.model(pos, f, c, MININD, win)
    for with_tot in (True, False):  # with the genome-wide lines the total is one more item: a sixth wave's second
        rows, tot = pops_dev(ctx, tp, tf, tn, MININD, win, **({} if with_tot else {"tot": False}))
        assert_rows(rows[0], want[0], A, 0, f"second item, totals {with_tot}", quiet=False)
        one = (win["hi"] - win["lo"]) == 1
        for fld in SUMS:
            assert np.array_equal(bits(rows[0][fld][one]), bits(want[0][fld][one])), fld
        tail = slice(shapes.QUERY_WAVES, None)
        assert np.any(rows[0]["n"][tail] > 0) and np.any(~one[tail]) and np.any(one[tail])
        if with_tot:
            assert_totals(tot, want_t, A_tot, "second item, totals")
