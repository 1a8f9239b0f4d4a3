"""CPU: the block jackknife of the f4-ratio (pgt_f4ratio_jackknife*, `f4ratioWindowPops -jackknife 1`) without a device — the two
restatements of tests/f4ratio_jack_model.py held to hand cases that are exact in f64 and to each other, the synthetic tables the
GPU test uploads, the item count as a constant of the estimator in csrc/, and the block counts tests/test_f4ratio_jack.py runs
at against the launch arithmetic of tests/dstat_jack_shapes.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dstat_jack_shapes as shapes
import f4ratio_jack_model as model
import helpers
from popgenomicstools_amd._lib import DSTAT_ROW_DTYPE, F4RATIO_JACK_DTYPE, F4RATIO_ROW_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "popgenomicstools_amd", "csrc")


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_both_models_give_the_hand_cases(name, blocks, want):
    """(num, den, m) per block: two blocks (1,2,1), (3,2,1) give alpha = 1, alpha_jack = 1, se = 0.5, z = 2; one block; no block;
    an unused block with NaN sums between two used ones; a deletion that leaves a zero denominator; 64 identical blocks."""
    num, den, m = ([b[c] for b in blocks] for c in range(3))
    got = model.jack_float(num, den, m)
    assert model.same_item(got, want), (name, got, want)
    exact = model.jack_exact(num, den, m)
    assert model.same_item(exact, want), (name, exact, want)
    # the rows the GPU test uploads for the case read the same values through items 5 = q(S0, S1) and 3 = q(S0, -S2)
    rows = model.hand_rows(blocks)
    items = model.jack_rows(rows[0])
    assert model.same_item(items[5], want) and model.same_item(items[3], want), (name, items)


def test_the_hand_cases_cover_what_they_must():
    names = [c[0] for c in model.HAND_CASES]
    assert names == ["two blocks", "64 identical blocks", "one block", "an unused block between two used ones",
                     "a deletion that leaves a zero denominator", "no block"]
    two = dict(zip(names, model.HAND_CASES))["two blocks"]
    assert two[1] == [(1, 2, 1), (3, 2, 1)] and two[2] == dict(alpha=1.0, alpha_jack=1.0, se=0.5, z=2.0, n_blocks=2, n_sites=2)
    used = sorted(len([b for b in c[1] if b[2] > 0]) for c in model.HAND_CASES)
    assert used == [0, 1, 2, 2, 2, 64]
    zero = dict(zip(names, model.HAND_CASES))["a deletion that leaves a zero denominator"][1]
    assert sum(b[1] for b in zero) - zero[1][1] == 0  # the denominator without the second block
    same = dict(zip(names, model.HAND_CASES))["64 identical blocks"][2]
    assert same["se"] == 0.0 and same["z"] != same["z"]


def test_the_float_model_agrees_with_the_exact_model_on_the_synthetic_tables():
    """|x - y| <= 1e-9 |y| + 1e-12 for alpha, alpha_jack and se at every small table size: the sums are positive, so N, D and every
    D - d_j are sums of like-signed terms (kappa = 1) and the float evaluation loses about n 2^-53."""
    for n_win in shapes.SMALL_N_WIN:
        n_triples = 3 if n_win <= 129 else 1
        rows = model.synth_rows(n_win, n_triples)
        assert rows.shape == (n_triples, n_win) and rows.dtype == F4RATIO_ROW_DTYPE
        used = rows["n"] > 0
        assert all(np.all(rows[f][used] > 0) for f in model.FIELDS) and (n_win < 63 or (~used).any())
        exact, flt = model.exact_reference(n_win, n_triples), model.float_reference(n_win, n_triples)
        for t in range(n_triples):
            for c in range(model.ITEMS):
                e, f = exact[t][c], flt[t][c]
                assert e["n_blocks"] == f["n_blocks"] == int(used[t].sum()) and e["n_sites"] == f["n_sites"] == int(rows["n"][t].sum())
                for k in ("alpha", "alpha_jack", "se"):
                    assert (e[k] != e[k]) == (f[k] != f[k]) and (e[k] != e[k] or helpers.close(f[k], e[k])), (n_win, t, c, k, f[k], e[k])
                if e["n_blocks"] >= 2:
                    assert e["se"] > 0 and np.sign(e["alpha"]) == (-1 if c in (2, 3) else 1)


def test_the_exact_models_shortcuts_are_the_definition():
    """fsum adds what sum adds, and the expanded variance is the definition's sum of squares, in rationals."""
    rng = np.random.default_rng(7800)
    xs = [Fraction(int(a), int(b)) for a, b in zip(rng.integers(-99, 99, 37), rng.integers(1, 99, 37))]
    assert model.fsum(xs) == sum(xs, Fraction(0)) and model.fsum([]) == 0 and model.fsum(xs[:1]) == xs[0]
    num, den, m = rng.integers(1, 50, 9) / 4.0, rng.integers(1, 50, 9) / 4.0, rng.integers(1, 9, 9)
    got = model.jack_exact(num, den, m)
    n, g = int(m.sum()), 9
    N, D = Fraction(float(num.sum())), Fraction(float(den.sum()))
    theta = N / D
    th = [(N - Fraction(float(a))) / (D - Fraction(float(b))) for a, b in zip(num, den)]
    theta_j = g * theta - sum(Fraction(n - int(mj), n) * t for mj, t in zip(m, th))
    var = sum((theta + Fraction(n - int(mj), int(mj)) * (theta - t) - theta_j) ** 2 / Fraction(n - int(mj), int(mj)) for mj, t in zip(m, th)) / g
    assert got["alpha"] == float(theta) and got["alpha_jack"] == float(theta_j) and abs(got["se"] - float(var) ** 0.5) <= 1e-15 * got["se"]


def test_the_synthetic_tables_are_the_d_jackknifes_through_a_view():
    assert F4RATIO_ROW_DTYPE.itemsize == DSTAT_ROW_DTYPE.itemsize == 48 and F4RATIO_JACK_DTYPE.itemsize == 48
    for a, b in zip(model.FIELDS, ("bbaa", "abba", "baba")):
        assert F4RATIO_ROW_DTYPE.fields[a][1] == DSTAT_ROW_DTYPE.fields[b][1]
    assert F4RATIO_ROW_DTYPE.fields["n"][1] == DSTAT_ROW_DTYPE.fields["n"][1]
    d = shapes.synth_rows(65, model.MAX_TRIPLES)
    v = model.synth_rows(65)
    assert v.shape == (10, 65) and np.array_equal(v["n"], d["n"]) and v["g_jk"].tobytes() == d["baba"].tobytes()
    assert model.MAX_TRIPLES == 10 == 5 * 4 * 3 // 6 <= shapes.MAX_TRIOS


def test_the_item_counts_and_the_workspace_sizes_they_give():
    """D, F3Mean and F4Mean stay at three items and keep their workspace; Ratio has six, and its workspace is larger by that."""
    from popgenomicstools_amd import _lib
    lib = _lib.load()
    internal = open(os.path.join(CSRC, "pgt_internal.h")).read()
    assert re.search(r"constexpr int kJackTopologies = 3;", internal) and re.search(r"constexpr int kJackRatioItems = 6;", internal)
    assert model.ITEMS == 6 and model.WORDS_PER_PARTIAL - shapes.WORDS_PER_PARTIAL == 2 * (6 - 3)
    for n_win in (1, 64, 65, 4097, 65537, 10**6):
        for t in (1, 4, 10):
            three = lib.pgt_dstat_jackknife_work_bytes(t, n_win)
            assert three == lib.pgt_f3_jackknife_work_bytes(t, n_win) == lib.pgt_f4_jackknife_work_bytes(t, n_win) == shapes.work_bytes(t, n_win)
            assert lib.pgt_f4ratio_jackknife_work_bytes(t, n_win) == model.work_bytes(t, n_win) >= three
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    assert "1 <= n_triples <= 10" in text and "theta_-j(c) = q(N_c - n_cj, D_c - d_cj)" in text


def test_the_block_counts_of_the_gpu_test():
    assert shapes.SMALL_N_WIN == (0, 1, 2, 3, 63, 64, 65, 127, 129, 4096) and shapes.EXACT_UP_TO == 4096
    assert shapes.LARGE_N_WIN == (4097, 65537)
    assert shapes.plan(4097)[2] == 65 and shapes.plan(65537)[:2] == (1025, 2)  # more than 64 partials; a wave's second chunk
