"""CPU: the f4-ratio front end (pgt_f4ratio_pops_reduce*, pgt_f4ratio_jackknife*, f4ratioWindowPops) without a device — the
exact-rational fixture, the NumPy model the GPU tests compare against, the cancellation of the three sums on the grid, the
orders, the workspace sizes, the declarations, the constants the build-grid test depends on, and the refusals of the Python
mirror and of the command line that come before the device is opened.

Ratios are compared only where the denominator's condition kappa = Σ|term| / |Σ term| is at most 8, which every test asserts of
its own inputs: with n <= 1024 sites per window the float64 model's ratio then lies within 2 kappa n 2^-53 < 2e-12 of the exact
one, far inside the 1e-9 relative bound used."""
import itertools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import f4ratio_jack_model
import f4ratio_pops_model as model
import helpers
from f4ratio_pops_model import KAPPA_CAP, SUMS
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
CSRC = os.path.join(ROOT, "popgenomicstools_amd", "csrc")
sys.path.insert(0, helpers.GOLDEN)


def unhex(xs):
    return np.array([float.fromhex(x) for x in xs], dtype=np.float64)


def fixture_sets():
    """-> (the fixture, its window table, [(set, pos, freqs, ninds)])"""
    k = helpers.load_golden("f4ratio_exact.json")
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    sets = [(s, np.array(s["pos"], dtype=np.uint32), [unhex(f) for f in s["freq"]], [np.array(c, dtype=np.int32) for c in s["nind"]]) for s in k["sets"]]
    return k, win, sets


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/f4ratio_exact.json is reproducible, holds data only, its frequencies lie on the 2^-10 grid, its inputs reach
    sites below minind, and every denominator of a recorded ratio has kappa <= 8."""
    import make_f4ratio_exact as gen
    k, win, sets = fixture_sets()
    assert set(k) == {"source", "windows", "ratio_windows", "sets"} and [s["n_pops"] for s in k["sets"]] == [6]
    assert gen.windows() == k["windows"] and [0, gen.N_SITES] in k["windows"] and gen.ratio_windows() == k["ratio_windows"]
    assert len(k["ratio_windows"]) >= 4 and all(hi - lo >= 256 for lo, hi in (k["windows"][n] for n in k["ratio_windows"]))
    assert gen.KAPPA_CAP == KAPPA_CAP == 8 and gen.RATIOS == model.RATIOS == f4ratio_jack_model.RATIOS
    worst = Fraction(0)
    for (s, pos, freqs, ninds), (n_pops, seed) in zip(sets, gen.SETS):
        gpos, gf, gn = gen.inputs(s["n_pops"], seed)
        assert n_pops == s["n_pops"] and gpos == s["pos"] and gn == s["nind"]
        assert [[float.fromhex(x) for x in col] for col in s["freq"]] == gf
        assert all(np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= 0 and x.max() <= 1 for x in freqs)
        assert set(s) == {"n_pops", "pos", "freq", "nind", "cases"} and [c["minind"] for c in s["cases"]] == [1, 5]
        for case in s["cases"]:
            assert [tuple(q["triple"]) for q in case["triples"]] == model.middle_triple_order(s["n_pops"]) == gen.triples_of(s["n_pops"])
            for q in case["triples"]:
                assert set(q) == {"triple", "n", "alpha"} | set(SUMS)
                sites = gen.exact_sites(gf, gn, q["triple"], case["minind"])
                for w, (lo, hi) in enumerate(k["windows"]):
                    r = gen.exact_window(sites, lo, hi)
                    assert gen.hexes(gen.nearest(x) for x in r[:3]) == [q[f][w] for f in SUMS] and r[3] == q["n"][w]
                    if w in k["ratio_windows"]:
                        assert gen.hexes(gen.nearest(x) for x in gen.exact_ratios(r[:3])) == q["alpha"][k["ratio_windows"].index(w)]
                        for c in range(3):  # the condition cap, asserted of the exact sums
                            assert r[c] != 0 and r[4 + c] <= KAPPA_CAP * abs(r[c])
                            worst = max(worst, r[4 + c] / abs(r[c]))
                ok = np.array([x is not None for x in sites])
                if case["minind"] == 5:
                    assert 0 < ok.sum() < ok.size  # sites with nInd below minind, and sites above
    print(f"largest kappa of a compared denominator in the fixture: {float(worst):.3f}")


def test_the_three_sums_cancel_exactly_on_the_grid():
    """s0 - s1 + s2 = 0 in rationals at every counted site; on the 2^-10 grid the float64 terms are exact (a product of two
    11-bit differences), so the three float64 site terms cancel exactly too, and so do the model's sums of a 320-site window
    (sums of multiples of 2^-20 below 2^10: exact)."""
    import make_f4ratio_exact as gen
    k, win, sets = fixture_sets()
    seen = 0
    for s, pos, freqs, ninds in sets:
        for triple in gen.triples_of(s["n_pops"]):
            sites = gen.exact_sites([list(x) for x in freqs], s["nind"], triple, 1)
            for x in sites:
                if x is not None:
                    assert x[0] - x[1] + x[2] == 0 and all(isinstance(v, Fraction) for v in x)
                    seen += 1
            for lo, hi in k["windows"]:
                r = gen.exact_window(sites, lo, hi)
                assert r[0] - r[1] + r[2] == 0
            i, j, kk = triple
            (t0, t1, t2), _ = model.site_terms(freqs[0], freqs[-1], freqs[i], freqs[j], freqs[kk])
            assert np.all(t0 - t1 + t2 == 0) and np.any(t0 != 0)
        rows, tot, A, A_tot = model.model(pos, freqs, ninds, 1, win)
        assert np.all(rows[SUMS[0]] - rows[SUMS[1]] + rows[SUMS[2]] == 0) and np.all(tot[SUMS[0]] - tot[SUMS[1]] + tot[SUMS[2]] == 0)
    assert seen > 500


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """On the grid every term and every sum of the fixture's windows is exact in float64: the model's sums ARE the fixture's,
    bit for bit, counts included; its six ratios are one correctly rounded division of exact operands, so they are the
    fixture's bit for bit as well — and within the 1e-9 relative bound the GPU tests use, a fortiori."""
    k, win, sets = fixture_sets()
    whole = k["windows"].index([0, 320])
    rw = k["ratio_windows"]
    for s, pos, freqs, ninds in sets:
        for case in s["cases"]:
            rows, tot, A, A_tot = model.model(pos, freqs, ninds, case["minind"], win)
            r2, t2, A2, At2 = model.model(pos, freqs, ninds, case["minind"], win, ranges_only=True)
            assert r2.tobytes() == rows.tobytes() and t2.tobytes() == tot.tobytes()
            for t, q in enumerate(case["triples"]):
                what = (s["n_pops"], case["minind"], q["triple"])
                assert np.array_equal(rows[t]["n"], np.array(q["n"], dtype=np.uint32)), what
                assert int(tot[t]["neff"]) == q["n"][whole] and int(tot[t]["nskip"]) == pos.size - q["n"][whole]
                assert not rows[t]["reserved_"].any()
                for fld in SUMS:
                    assert np.array_equal(rows[t][fld], unhex(q[fld])), what + (fld,)
                    assert float(tot[t][fld]) == float.fromhex(q[fld][whole]) and A_tot[fld][t] == A[fld][t][whole]
                    assert np.all(model.kappa(rows[t][fld][rw], A[fld][t][rw]) <= KAPPA_CAP), what + (fld, "kappa")
                got = model.alphas_of(rows[t][rw])
                want = np.array([unhex(a) for a in q["alpha"]])
                assert got.shape == want.shape == (len(rw), 6)
                assert np.array_equal(got, want), what
                assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want))
                assert np.array_equal(model.alphas_of(tot[t:t + 1])[0], want[rw.index(whole)])
    # the ratios of the admixture tree come out where the recipe puts them: alpha(B = M1, X = M2, C = M3) at K = 6 is the share of
    # M1-like ancestry in M2, (0.633 - 0.367) / (0.9 - 0.367) = 0.5 in expectation
    s, pos, freqs, ninds = sets[0]
    rows, tot, _, _ = model.model(pos, freqs, ninds, 1, win)
    assert abs(model.alphas_of(tot)[0, 0] - 0.5) < 0.1


def test_the_condition_cap_holds_for_the_recipe_at_the_sizes_the_gpu_tests_use():
    """kappa <= 8 for every sum of every triple, windows of 256, 512 and 1024 sites and the whole column, m = 3, 4, 5."""
    worst = 0.0
    for seed in range(4):
        for k in (5, 6, 7):
            rng = np.random.default_rng([7700, seed, k])
            n = 4096
            f, c = model.admixture_inputs(rng, n, k, lo_count=3)
            pos = np.arange(1, n + 1, dtype=np.uint32)
            win = np.zeros(0, dtype=WIN_DTYPE)
            for W in (256, 512, 1024, n):
                w = np.zeros(n // W, dtype=WIN_DTYPE)
                w["lo"] = np.arange(n // W) * W
                w["hi"] = w["lo"] + W
                win = np.concatenate([win, w])
            rows, tot, A, A_tot = model.model(pos, f, c, 5, win)
            for fld in SUMS:
                kap = model.kappa(rows[fld], A[fld])
                worst = max(worst, float(kap.max()))
                assert np.all(kap <= KAPPA_CAP), (seed, k, fld, float(kap.max()))
    print(f"largest kappa over the recipe's windows: {worst:.3f}")


def test_orders_against_itertools():
    import popgenomicstools_amd as pgt
    for k in range(0, 10):
        want = list(itertools.combinations(range(1, max(k - 1, 1)), 3))
        assert pgt.middle_triple_order(k) == want == model.middle_triple_order(k), k
    assert [len(pgt.middle_triple_order(k)) for k in (5, 6, 7)] == [1, 4, 10]
    assert pgt.middle_triple_order(5) == [(1, 2, 3)] and pgt.middle_triple_order(6)[:2] == [(1, 2, 3), (1, 2, 4)]
    for t in itertools.combinations(range(1, 6), 3):
        i, j, k = t
        got = pgt.ratio_order(*t)
        assert got == [(i, j, k), (j, i, k), (i, k, j), (k, i, j), (j, k, i), (k, j, i)] == model.ratio_order(*t)
        assert sorted(got) == sorted(itertools.permutations(t))  # every (B, X, C) once
        # the table of the definition: alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C), with f4(A,O; x,y) = -f4(A,O; y,x) and the sums
        # S0, S1, S2 = f4(A,O; i,j), (i,k), (j,k) up to the common factor n
        f4 = {(i, j): (+1, 0), (i, k): (+1, 1), (j, k): (+1, 2), (j, i): (-1, 0), (k, i): (-1, 1), (k, j): (-1, 2)}
        for c, (B, X, C) in enumerate(got):
            (sn, a), (sd, b) = f4[X, C], f4[B, C]
            (tn, ta), (td, tb) = model.RATIOS[c]
            assert (a, b) == (ta, tb) and sn * sd == tn * td, (t, c)  # the same two sums, the same sign of the quotient
    assert {"f4ratio_window_pops", "f4ratio_alphas", "middle_triple_order", "ratio_order"} <= set(pgt.__all__)
    rows = np.zeros(3, dtype=_lib.F4RATIO_ROW_DTYPE)
    rows["g_ij"], rows["g_ik"], rows["g_jk"] = [1.0, 2.0, 0.0], [2.0, 0.0, 0.0], [4.0, -1.0, 0.0]
    assert np.array_equal(pgt.f4ratio_alphas(rows), model.alphas_of(rows))
    assert pgt.f4ratio_alphas(rows)[0].tolist() == [2.0, 0.5, -4.0, -0.25, 2.0, 0.5] and not pgt.f4ratio_alphas(rows)[2].any()
    assert pgt.f4ratio_alphas(rows)[1].tolist() == [0.0, -0.0, 0.5, 2.0, 0.0, 0.0]


def test_tree_bytes_only_for_five_to_seven_populations_and_work_bytes_for_one_to_ten_triples():
    """0 outside 5 ... 7; inside, the tree of f4 (three sums per item) with C(K-2, 3) items.  The jackknife workspace: 0 outside
    1 ... 10 triples; inside, tests/dstat_jack_shapes.py's arithmetic with 5 + 6 + 6 words per partial where the three-item
    estimators have 5 + 3 + 3 (restated in tests/f4ratio_jack_model.py)."""
    lib = _lib.load()
    import dstat_jack_shapes as shapes
    import popgenomicstools_amd as pgt
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        for k in range(0, 12):
            b = lib.pgt_f4ratio_pops_tree_bytes(k, n)
            assert (b > 0) == (5 <= k <= 7), (k, n, b)
        # one item of three sums: f4 at 4 populations; four items: f3 at 4 populations; ten: f3 at 5 populations
        assert lib.pgt_f4ratio_pops_tree_bytes(5, n) == lib.pgt_f4_pops_tree_bytes(4, n)
        assert lib.pgt_f4ratio_pops_tree_bytes(6, n) == lib.pgt_f3_pops_tree_bytes(4, n)
        assert lib.pgt_f4ratio_pops_tree_bytes(7, n) == lib.pgt_f3_pops_tree_bytes(5, n)
    assert pgt.Context.f4ratio_pops_tree_bytes(6, 12345) == lib.pgt_f4ratio_pops_tree_bytes(6, 12345) > 0
    assert pgt.Context.f4ratio_pops_tree_bytes(8, 12345) == 0 and pgt.Context.f4ratio_pops_tree_bytes(4, 12345) == 0
    sizes = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 131073, 10**6, 10**8)
    for t in (0, 1, 4, 10, 11, 15, 20, 21, 1000):
        for n in sizes:
            b = lib.pgt_f4ratio_jackknife_work_bytes(t, n)
            assert b == f4ratio_jack_model.work_bytes(t, n) == pgt.Context.f4ratio_jackknife_work_bytes(t, n), (t, n, b)
            assert (b > 0) == (1 <= t <= 10)
            if 1 <= t <= 10:  # the three-item estimators keep their size; this one is larger by its six items
                assert lib.pgt_f4_jackknife_work_bytes(t, n) == shapes.work_bytes(t, n) <= b
    src = open(os.path.join(CSRC, "pgt_internal.h")).read()
    assert re.search(r"constexpr uint32_t kJackMaxTriples = 10;", src) and re.search(r"constexpr int kJackRatioItems = 6;", src)
    assert f4ratio_jack_model.WORDS_PER_PARTIAL == 17 and shapes.WORDS_PER_PARTIAL == 11


def test_header_binding_and_dtypes():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_f4ratio_pops_tree_bytes", "pgt_f4ratio_pops_reduce_dev", "pgt_f4ratio_pops_reduce", "pgt_f4ratio_jackknife_work_bytes",
             "pgt_f4ratio_jackknife_dev", "pgt_f4ratio_jackknife")
    for name in names:
        assert name + "(" in text
    assert "} pgt_f4ratio_row;" in text and "} pgt_f4ratio_total;" in text and "} pgt_f4ratio_jack;" in text
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_f4ratio_row, pgt_f4ratio_total, pgt_f4ratio_jack" in text
    for line in ("e    = p_0 - p_{K-1}", "d_ab = p_a - p_b", "s0 = e * d_ij", "s1 = e * d_ik", "s2 = e * d_jk", "out[t * n_win + w]",
                 "pgt_f4ratio_row (48 bytes)", "pgt_f4ratio_total (40 bytes", "pgt_f4ratio_jackknife_dev (48 bytes, the layout of pgt_f4_jack)",
                 "1e-9 * A + 1e-12", "1 <= n_triples <= 10", "5 <= n_pops <= 7", "User-chosen quintet lists", "q(a, b) = b != 0 ? a / b : 0",
                 "Nothing is clamped", "FIVE populations", 'messages begin "pgt_f4ratio_jackknife: "', '"pgt_f4ratio_pops_reduce: "',
                 "u = 6 t + c"):
        assert line in text, line
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    row, tot, jack = _lib.F4RATIO_ROW_DTYPE, _lib.F4RATIO_TOTAL_DTYPE, _lib.F4RATIO_JACK_DTYPE
    assert row.names == ("start", "end", "mid", "n", "reserved_") + SUMS and row.itemsize == 48
    assert [row.fields[f][1] for f in row.names] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert tot.names == SUMS + ("neff", "nskip") and tot.itemsize == 40 and [tot.fields[f][1] for f in tot.names] == [0, 8, 16, 24, 32]
    assert jack.names == ("alpha", "alpha_jack", "se", "z", "n_sites", "n_blocks", "pad_") and jack.itemsize == 48
    assert [jack.fields[f][1] for f in jack.names] == [0, 8, 16, 24, 32, 40, 44]
    for a, b in zip(SUMS, ("f4_ij_kl", "f4_ik_jl", "f4_il_jk")):  # the jackknife's row loader serves both row types
        assert row.fields[a][1] == _lib.F4_ROW_DTYPE.fields[b][1]
    assert [jack.fields[f][1] for f in jack.names] == [_lib.F4_JACK_DTYPE.fields[f][1] for f in _lib.F4_JACK_DTYPE.names]
    # the C compiler's view of the same structs, and the loader's
    api = open(os.path.join(CSRC, "pgt_api.cpp")).read()
    assert "sizeof(pgt_f4ratio_row) == 48 && offsetof(pgt_f4ratio_row, reserved_) == 16 && offsetof(pgt_f4ratio_row, g_ij) == offsetof(pgt_f4_row, f4_ij_kl)" in api
    assert "init_f4ratio_pops_kernels(&init_err)" in api


def test_the_build_grid_constants_are_the_ones_the_gpu_test_assumes():
    """tests/test_f4ratio_pops_grid.py takes its tile counts from this statistic's own kOneWaveFrom: K = 5 is a two-wave K
    (2048 build waves at most), K = 6 a one-wave K (1024)."""
    import pops_grid_shapes as shapes
    src = open(os.path.join(CSRC, "pgt_f4ratio_pops_kernels.hip")).read()
    m = re.search(r"static constexpr int kOneWaveFrom = (\d+);", src)
    assert m and int(m.group(1)) == 6
    assert re.search(r"static constexpr int kQueryOneWaveFrom = 7;", src) and re.search(r"kMinPops = 5, kMaxPops = 7;", src)
    assert "static constexpr const char *kOneWaveKnob = nullptr;" in src and "using Counts = CountBits;" in src
    assert shapes.balanced_build(1025, shapes.ONE_WAVE_BUILD_WAVES) == (2, 513, 516) and shapes.balanced_build(2049, shapes.MAX_BUILD_WAVES) == (2, 1025, 1028)
    assert shapes.balanced_build(1024, shapes.ONE_WAVE_BUILD_WAVES)[0] == 1 and shapes.balanced_build(2048, shapes.MAX_BUILD_WAVES)[0] == 1
    walk = open(os.path.join(CSRC, "pgt_pops_walk.h")).read()
    assert "constexpr int middle_triple_count(int np) { return (np - 2) * (np - 3) * (np - 4) / 6; }" in walk


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (4, 8):
        with pytest.raises(_lib.PgtError, match="f4ratio_window_pops: 5 ... 7 populations, one frequency and one count column each") as e:
            pgt.f4ratio_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1)
        assert e.value.code == _lib.PGT_EARG
        with pytest.raises(_lib.PgtError, match="f4ratio_window_pops: 5 ... 7 populations"):
            pgt.f4ratio_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1, jackknife=True)
    with pytest.raises(_lib.PgtError, match="5 ... 7 populations"):
        pgt.f4ratio_window_pops(ids, pos, [z] * 5, [c] * 4, 2, 2, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.f4ratio_window_pops(ids, pos, [z] * 5, [c] * 5, 2, 2, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.f4ratio_window_pops(ids, pos, [z] * 5, [c] * 5, 2, 2, 1, 0)
    for W, S in ((4, 2), (0, 0)):
        with pytest.raises(_lib.PgtError, match="f4ratio_window_pops: the block jackknife needs disjoint windows") as e:
            pgt.f4ratio_window_pops(ids, pos, [z] * 5, [c] * 5, W, S, 1, 1, jackknife=True)
        assert e.value.code == _lib.PGT_EARG and f"winsize {W}" in str(e.value) and f"stepsize {S}" in str(e.value)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "f4ratioWindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_states_the_definition_and_what_is_left_out(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("f4ratioWindowPops [options] -out PREFIX <maf A> <maf M1> ... <maf Mm> <maf O>", "5 <= K <= 7",
                 "alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C)", "(p_A - p_O)(p_x - p_y)",          # the definition
                 "The FIRST file is A", "the LAST file is the outgroup O",                            # the roles
                 "ALL files must report the frequency of the SAME allele",                            # one allele
                 "ALL FIVE populations", "over the same sites",                                       # five populations
                 "NOT clamped",                                                                       # no clamp
                 "denominator is exactly zero is printed as 0",                                       # the zero-denominator convention
                 "user-chosen quintet lists", "K = 8", "qpAdm-style multi-source fits",               # not computed
                 "-jackknife", "-skip_missing", "-sizefile", "-fixedsite", "numerator and denominator together",
                 "PREFIX.pop<i>_pop<j>_pop<k>.f4ratio", "PREFIX.global", "PREFIX.jackknife", "(1) B\n(2) X\n(3) C",
                 "One GPU is used", "No passes mode", "PGT_DXY_SYNC=reference is not offered"):
        assert word in r.stdout, word
    # f4WindowPops points here and keeps its own words
    r4 = run([os.path.join(BIN, "f4WindowPops")])
    assert "f4-ratio admixture proportions (see f4ratioWindowPops)" in r4.stdout


def test_the_refusals_that_need_no_device(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(9)]
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    f4 = os.path.join(BIN, "f4WindowPops")
    for k in (4, 8):
        r = run([tool] + head + missing[:k])
        assert r.returncode == 255 and r.stdout == "", (k, r.returncode)
        assert f"f4ratioWindowPops: between 5 and 7 MAF files are needed ({k} given)" in r.stderr and "Unable to open" not in r.stderr, r.stderr
    cases = [
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-jackknife", "1"], "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0"], "-jackknife 1 needs windows as its blocks"),
        (["-jackknife", "2", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "-jackknife must be 0 or 1 (given: 2)"),
        (["-fd", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "Unknown command"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + ["-out", out] + missing[:5])
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
        r4 = run([f4] + opts + ["-out", out] + missing[:5])  # f4WindowPops refuses the same options in the same words
        assert r4.returncode == 255 and r4.stderr == r.stderr, (opts, r4.stderr, r.stderr)
    # without a refusal the run gets as far as the files
    r = run([tool, "-jackknife", "1"] + head + missing[:5])
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
