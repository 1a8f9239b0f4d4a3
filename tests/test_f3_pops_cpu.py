"""CPU: the f3 front end (pgt_f3_pops_reduce*, f3WindowPops) without a device — the exact-rational fixture, the NumPy model the
GPU tests compare against, the model's identity with Hudson's numerator, the allele symmetry of the definition, the workspace
size, the declarations, the constants the build-grid test depends on, and the refusals of the Python mirror and of the command
line that come before the device is opened."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import f3_pops_model
import fst_hudson_model
import helpers
from f3_pops_model import SUMS
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)


def fixture_sets():
    """-> (the fixture, its window table, [(set, pos, freqs, ninds)])"""
    k = helpers.load_golden("f3_exact.json")
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    sets = [(s, np.array(s["pos"], dtype=np.uint32), [np.array(f, dtype=np.float64) for f in s["freq"]],
             [np.array(c, dtype=np.int32) for c in s["nind"]]) for s in k["sets"]]
    return k, win, sets


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/f3_exact.json is reproducible, holds data only, and its inputs reach ties, 0 and 1 at counted sites."""
    import make_f3_exact as gen
    k, win, sets = fixture_sets()
    assert set(k) == {"source", "windows", "sets"} and [s["n_pops"] for s in k["sets"]] == [3, 4]
    assert gen.windows() == k["windows"] and [0, gen.N_SITES] in k["windows"]
    for (s, pos, freqs, ninds), seed in zip(sets, (20261020, 20261021)):
        gpos, gf, gn = gen.inputs(s["n_pops"], seed)
        assert gpos == s["pos"] and gf == s["freq"] and gn == s["nind"]
        assert set(s) == {"n_pops", "pos", "freq", "nind", "cases"} and [c["minind"] for c in s["cases"]] == [1, 5]
        for case in s["cases"]:
            assert [tuple(tr["trio"]) for tr in case["trios"]] == f3_pops_model.all_trio_order(s["n_pops"])
            for tr in case["trios"]:
                assert set(tr) == {"trio", "n"} | set(SUMS)
                sites = gen.exact_sites(s["freq"], s["nind"], tr["trio"], case["minind"])
                for w, (lo, hi) in enumerate(k["windows"]):
                    a, b, c, n = gen.exact_window(sites, lo, hi)
                    assert (gen.nearest(a), gen.nearest(b), gen.nearest(c), n) == (tr["f3_i"][w], tr["f3_j"][w], tr["f3_k"][w], tr["n"][w])
                ok = np.array([x is not None for x in sites])
                i, j, kk = tr["trio"]
                assert 0 < ok.sum() < ok.size
                for what, m in (("p_i == p_j", freqs[i] == freqs[j]), ("p_i == p_k", freqs[i] == freqs[kk]), ("p_j == p_k", freqs[j] == freqs[kk])):
                    assert np.any(m & ok), (case["minind"], tr["trio"], what)
                for x in (i, j, kk):
                    assert np.any(((freqs[x] == 0) | (freqs[x] == 1)) & ok), (case["minind"], tr["trio"], x)
                assert any(v < 0 for v in tr["f3_i"]) and any(v > 0 for v in tr["f3_i"])  # both signs among the windows


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site lines of the definition, summed: within 1e-12 A + 1e-15 (hi - lo) of the exact rationals, A the window's
    Σ(|product| + |h|), counts exact.  The per-site floor: a term is a product of two differences of values <= 1 minus a
    quotient <= 1/4, five roundings of 2^-53 of values <= 1: below 1e-15 per site."""
    k, win, sets = fixture_sets()
    length = (win["hi"] - win["lo"]).astype(np.float64)
    whole = k["windows"].index([0, 96])
    worst = 0.0
    for s, pos, freqs, ninds in sets:
        for case in s["cases"]:
            rows, tot, A, A_tot = f3_pops_model.model(pos, freqs, ninds, case["minind"], win)
            # the ranges-only evaluation is the same model with float64 pairwise sums: 1e-13 of A apart at most
            r2, t2, A2, At2 = f3_pops_model.model(pos, freqs, ninds, case["minind"], win, ranges_only=True)
            assert np.array_equal(r2["n"], rows["n"]) and np.array_equal(t2["neff"], tot["neff"]) and np.array_equal(t2["nskip"], tot["nskip"])
            for f in SUMS:
                assert np.all(np.abs(r2[f] - rows[f]) <= 1e-13 * A[f]) and np.all(np.abs(A2[f] - A[f]) <= 1e-13 * A[f])
                assert np.all(np.abs(t2[f] - tot[f]) <= 1e-13 * A_tot[f]) and np.all(np.abs(At2[f] - A_tot[f]) <= 1e-13 * A_tot[f])
            for t, tr in enumerate(case["trios"]):
                assert np.array_equal(rows[t]["n"], np.array(tr["n"], dtype=np.uint32))
                assert int(tot[t]["neff"]) == tr["n"][whole] and int(tot[t]["nskip"]) == pos.size - tr["n"][whole]
                assert not rows[t]["reserved_"].any()
                for fld in SUMS:
                    err = np.abs(rows[t][fld] - np.array(tr[fld]))
                    worst = max(worst, float(err[length == 1].max()))
                    assert np.all(err <= 1e-12 * A[fld][t] + 1e-15 * length), (s["n_pops"], case["minind"], tr["trio"], fld)
                    assert abs(float(tot[t][fld]) - tr[fld][whole]) <= 1e-12 * A_tot[fld][t] + 1e-15 * pos.size
                    assert A_tot[fld][t] == A[fld][t][whole]
    print(f"largest one-site error of the model against the exact value: {worst:.3e}")


def test_the_first_two_targets_add_up_to_hudsons_numerator():
    """s0 + s1 = d_ij (d_ik - d_jk) - h_i - h_j = (p_i - p_j)^2 - h_i - h_j: per site within a few 2^-53 of values <= 1, and
    exactly so in rationals — fst_hudson_model's numerator on the same sites."""
    import make_f3_exact as gen
    k, win, sets = fixture_sets()
    worst = 0.0
    for s, pos, freqs, ninds in sets:
        for i, j, kk in f3_pops_model.all_trio_order(s["n_pops"]):
            (s0, s1, _), _ = f3_pops_model.site_terms(freqs[i], freqs[j], freqs[kk], ninds[i], ninds[j], ninds[kk])
            num, _ = fst_hudson_model.site_components(freqs[i], freqs[j], ninds[i], ninds[j])
            ok = f3_pops_model.counted(ninds, i, j, kk, 1)
            worst = max(worst, float(np.max(np.abs((s0 + s1) - num)[ok])))
            for site in np.flatnonzero(ok):
                p = [Fraction(float(freqs[x][site])) for x in (i, j, kk)]
                n = [int(ninds[x][site]) for x in (i, j, kk)]
                e = gen.f3_site(p, n)
                assert e[0] + e[1] == (p[0] - p[1]) ** 2 - p[0] * (1 - p[0]) / (2 * n[0] - 1) - p[1] * (1 - p[1]) / (2 * n[1] - 1)
    print(f"largest per-site |s0 + s1 - Hudson's numerator|: {worst:.3e}")
    assert worst <= 1e-15


def test_flipping_the_allele_in_all_populations_keeps_the_bits():
    """Frequencies that are multiples of 2^-10: 1 - p is exact, the differences only change sign (and a product of two of them
    keeps its bits), p (1 - p) commutes: the three terms keep their bits under p -> 1 - p in ALL populations."""
    rng = np.random.default_rng(3100)
    n = 4096
    p = [rng.integers(0, 1025, n) / 1024.0 for _ in range(3)]
    c = [rng.integers(1, 21, n).astype(np.int32) for _ in range(3)]
    a, _ = f3_pops_model.site_terms(*p, *c)
    b, _ = f3_pops_model.site_terms(*[1.0 - x for x in p], *c)
    for x, y in zip(a, b):
        assert np.array_equal((x + 0.0).view(np.uint64), (y + 0.0).view(np.uint64))
    assert np.any(a[0] < 0) and np.any(a[0] > 0)


def test_tree_bytes_only_for_three_to_six_populations():
    lib = _lib.load()
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        for k in range(0, 12):
            b = lib.pgt_f3_pops_tree_bytes(k, n)
            assert (b > 0) == (3 <= k <= 6), (k, n, b)
            if 3 <= k <= 6:
                assert b == lib.pgt_dstat_pops_tree_bytes(k + 1, n)  # C(k, 3) trios of three sums: the D node at one population more
        sizes = [lib.pgt_f3_pops_tree_bytes(k, n) for k in (3, 4, 5, 6)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    import popgenomicstools_amd as pgt
    assert pgt.Context.f3_pops_tree_bytes(5, 12345) == lib.pgt_f3_pops_tree_bytes(5, 12345)
    assert pgt.Context.f3_pops_tree_bytes(7, 12345) == 0 and pgt.Context.f3_pops_tree_bytes(2, 12345) == 0


def test_header_binding_and_orders():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_f3_pops_tree_bytes", "pgt_f3_pops_reduce_dev", "pgt_f3_pops_reduce", "pgt_f3_jackknife_work_bytes", "pgt_f3_jackknife_dev",
             "pgt_f3_jackknife")
    for name in names:
        assert name + "(" in text
    assert "} pgt_f3_row;" in text and "} pgt_f3_total;" in text and "} pgt_f3_jack;" in text
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_f3_row, pgt_f3_total, pgt_f3_jack" in text
    for line in ("h_x  = (p_x * (1 - p_x)) / (2*n_x - 1)", "d_ab = p_a - p_b", "s0 = d_ij*d_ik - h_i", "s1 = (-d_ij)*d_jk - h_j",
                 "s2 = d_ik*d_jk - h_k", "out[t * n_win + w]", "mean(a, b)  = b != 0 ? a / b : 0", "theta_-j    = mean(X - x_j, n - m_j)",
                 "f4, user-chosen trio lists"):
        assert line in text, line
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.F3_ROW_DTYPE.names == ("start", "end", "mid", "n", "reserved_", "f3_i", "f3_j", "f3_k") and _lib.F3_ROW_DTYPE.itemsize == 48
    assert _lib.F3_TOTAL_DTYPE.names == ("f3_i", "f3_j", "f3_k", "neff", "nskip") and _lib.F3_TOTAL_DTYPE.itemsize == 40
    assert _lib.F3_JACK_DTYPE.names == ("f3", "f3_jack", "se", "z", "n_sites", "n_blocks", "pad_") and _lib.F3_JACK_DTYPE.itemsize == 48
    for a, b in zip(SUMS, ("bbaa", "abba", "baba")):  # the jackknife's row loader serves both row types
        assert _lib.F3_ROW_DTYPE.fields[a][1] == _lib.DSTAT_ROW_DTYPE.fields[b][1]
    import popgenomicstools_amd as pgt
    for k in range(3, 7):
        assert pgt.all_trio_order(k) == f3_pops_model.all_trio_order(k) and len(pgt.all_trio_order(k)) == (1, 4, 10, 20)[k - 3]
    assert pgt.all_trio_order(4) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    assert pgt.target_order(0, 2, 5) == [(0, 2, 5), (2, 0, 5), (5, 0, 2)]
    assert {"f3_window_pops", "all_trio_order", "target_order"} <= set(pgt.__all__)


def test_the_build_grid_constants_are_the_ones_the_gpu_test_assumes():
    """tests/test_f3_pops_grid.py takes its cases from tests/pops_grid_shapes.py, whose POPS_ONE_WAVE_FROM must be this
    statistic's kOneWaveFrom; K = 3 is a two-wave K and K = 5 a one-wave K."""
    import pops_grid_shapes as shapes
    src = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_f3_pops_kernels.hip")).read()
    m = re.search(r"static constexpr int kOneWaveFrom = (\d+);", src)
    assert m and int(m.group(1)) == shapes.POPS_ONE_WAVE_FROM == 5
    assert re.search(r"static constexpr int kQueryOneWaveFrom = 6;", src) and re.search(r"kMinPops = 3, kMaxPops = 6;", src)
    assert shapes.pops_build(1025, 5) == (2, 513, 516) and shapes.pops_build(2049, 3) == (2, 1025, 1028)
    assert shapes.pops_build(1024, 5)[0] == 1 and shapes.pops_build(2048, 3)[0] == 1  # the smallest counts with two rounds


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (2, 7):
        with pytest.raises(_lib.PgtError, match="f3_window_pops: 3 ... 6 populations, one frequency and one count column each") as e:
            pgt.f3_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1)
        assert e.value.code == _lib.PGT_EARG
    with pytest.raises(_lib.PgtError, match="3 ... 6 populations"):
        pgt.f3_window_pops(ids, pos, [z] * 3, [c] * 2, 2, 2, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.f3_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.f3_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 1, 0)
    for W, S in ((4, 2), (0, 0)):
        with pytest.raises(_lib.PgtError, match="f3_window_pops: the block jackknife needs disjoint windows") as e:
            pgt.f3_window_pops(ids, pos, [z] * 3, [c] * 3, W, S, 1, 1, jackknife=True)
        assert e.value.code == _lib.PGT_EARG and f"winsize {W}" in str(e.value) and f"stepsize {S}" in str(e.value)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "f3WindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_states_the_definition_and_what_is_left_out(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("f3WindowPops [options] -out PREFIX", "(3 <= K <= 6)", "(p_x - p_a)(p_x - p_b) - p_x (1 - p_x)/(2 n_x - 1)", "MEAN",
                 "ALL files must report the frequency of the SAME allele", "NEGATIVE", "admixed", "Outgroup f3", "-jackknife",
                 "PREFIX.pop<i>_pop<j>_pop<k>.f3", "PREFIX.global", "PREFIX.jackknife", "(1) target\n(2) source 1\n(3) source 2",
                 "normalised by the target's heterozygosity", "f4", "user-chosen trio lists", "One GPU is used"):
        assert word in r.stdout, word


def test_the_refusals_that_need_no_device(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(7)]
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    for k in (2, 7):
        r = run([tool] + head + missing[:k])
        assert r.returncode == 255 and r.stdout == "", (k, r.returncode)
        assert f"f3WindowPops: between 3 and 6 MAF files are needed ({k} given)" in r.stderr and "Unable to open" not in r.stderr, r.stderr
    cases = [
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-jackknife", "1"], "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0"], "-jackknife 1 needs windows as its blocks"),
        (["-jackknife", "2", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "-jackknife must be 0 or 1 (given: 2)"),
        (["-fd", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "Unknown command"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + ["-out", out] + missing[:3])
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
    # without a refusal the run gets as far as the files
    r = run([tool, "-jackknife", "1"] + head + missing[:3])
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
