"""CPU: the block jackknife of a mean (pgt_f3_jackknife*, `f3WindowPops -jackknife 1`) without a device — the hand-checkable
cases on both models, the NumPy model against the exact-rational one (the tolerance the GPU tests then use), and the workspace
size, which is D's."""
import numpy as np
import pytest

import dstat_jack_shapes as shapes
import f3_jack_model as model
import helpers
from popgenomicstools_amd import _lib

N_BLOCKS = (2, 3, 63, 64, 65, 129, 1000, 4096)


# ---- hand-checkable cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_hand_checkable_cases(name, blocks, want):
    x, m = [float(b[0]) for b in blocks], [int(b[1]) for b in blocks]
    for fn in (model.jack_float, model.jack_exact):
        if fn is model.jack_exact:  # finite inputs only: it never looks at an unused block
            x = [0.0 if v != v else v for v in x]
        got = fn(np.array(x), np.array(m, dtype=np.uint32))
        assert model.same_item(got, want), (name, fn.__name__, got, want)


def test_the_hand_cases_are_the_ones_the_definition_gives():
    cases = {c[0]: c for c in model.HAND_CASES}
    assert cases["two blocks"][1] == [(3, 1), (1, 1)] and cases["two blocks"][2] == dict(f3=2.0, f3_jack=2.0, se=1.0, z=2.0, n_blocks=2, n_sites=2)
    assert cases["64 identical blocks"][1] == [(3, 8)] * 64 and cases["64 identical blocks"][2]["f3"] == 0.375
    assert cases["64 identical blocks"][2]["se"] == 0.0 and cases["64 identical blocks"][2]["z"] != cases["64 identical blocks"][2]["z"]
    assert len(cases["one block"][1]) == 1 and cases["no block"][1] == []
    used = [b for b in cases["an unused block between two used ones"][1] if b[1] > 0]
    assert used == cases["two blocks"][1] and cases["an unused block between two used ones"][2] == cases["two blocks"][2]


# ---- the float model against the exact evaluation ---------------------------------------------------------------------------
def test_the_table_has_signed_sums_and_unused_blocks_with_nan_sums():
    rows = model.synth_rows(4096)
    empty = rows["n"] == 0
    assert 0.13 < empty.mean() < 0.15 and all(np.isnan(rows[f][empty]).all() and not np.isnan(rows[f][~empty]).any() for f in model.FIELDS)
    assert rows["n"].max() == 512 and rows["n"][~empty].min() == 1
    x = rows["f3_i"][~empty]
    assert np.mean(x < 0) > 0.5 and np.mean(x > 0) > 0.3 and np.array_equal(x * 2.0 ** 20, np.round(x * 2.0 ** 20))
    per_site = x / rows["n"][~empty]
    assert abs(per_site.mean() + 0.004) < 0.001 and 0.015 < per_site.std() < 0.025
    assert not rows["reserved_"].any()
    assert model.synth_rows(4096, 4).tobytes() == rows[:4].tobytes()  # fewer trios: a prefix


@pytest.mark.parametrize("n_win", N_BLOCKS)
def test_float_model_stays_within_the_project_tolerance_of_the_exact_one(n_win):
    """f3, f3_jack and se of the first trios' items: 1e-9 |y| + 1e-12 (helpers.REL / ABS) — and below 1 % of that bound, so
    the bound is the one to use on the GPU too.  The worst share of the bound is printed."""
    n_trios = 20 if n_win <= 129 else 3
    exact, flt = model.exact_reference(n_win, n_trios), model.float_reference(n_win, n_trios)
    worst = {"f3": 0.0, "f3_jack": 0.0, "se": 0.0}
    for t in range(n_trios):
        for c in range(3):
            e, f = exact[t][c], flt[t][c]
            assert e["n_blocks"] == f["n_blocks"] and e["n_sites"] == f["n_sites"], (n_win, t, c)
            for k in worst:
                if e[k] != e[k]:
                    assert f[k] != f[k], (n_win, t, c, k)
                    continue
                assert helpers.close(f[k], e[k]), (n_win, t, c, k, f[k], e[k])
                worst[k] = max(worst[k], abs(f[k] - e[k]) / (helpers.REL * abs(e[k]) + helpers.ABS))
            assert (e["z"] != e["z"]) == (f["z"] != f["z"])
    print(f"n_win={n_win}: largest share of the bound the float model uses against the exact one: {worst}")
    assert max(worst.values()) < 0.01, worst


def test_an_unused_block_changes_nothing_but_is_not_counted():
    rows = model.synth_rows(129)[3]
    used = rows["n"] > 0
    assert not used.all()
    a = model.jack_float(rows["f3_j"], rows["n"])
    b = model.jack_float(rows["f3_j"][used], rows["n"][used])
    assert a == b and a["n_blocks"] == int(used.sum()) < rows.size


# ---- the workspace -----------------------------------------------------------------------------------------------------------
def test_work_bytes_are_those_of_the_d_jackknife():
    lib = _lib.load()
    import popgenomicstools_amd as pgt
    sizes = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 131073, 10**6, 10**8)
    for t in (0, 1, 4, 20, 21, 1000):
        for n in sizes:
            b = lib.pgt_f3_jackknife_work_bytes(t, n)
            assert b == lib.pgt_dstat_jackknife_work_bytes(t, n) == shapes.work_bytes(t, n), (t, n, b)
            assert b == pgt.Context.f3_jackknife_work_bytes(t, n)
    assert model.MAX_TRIOS == shapes.MAX_TRIOS == 20
