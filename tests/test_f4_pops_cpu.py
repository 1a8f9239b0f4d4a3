"""CPU: the f4 front end (pgt_f4_pops_reduce*, f4WindowPops) without a device — the exact-rational fixture, the NumPy model the
GPU tests compare against, the identity of the three pairings, the allele symmetry of the definition, the orders, the workspace
size, the declarations, the constants the build-grid test depends on, and the refusals of the Python mirror and of the command
line that come before the device is opened."""
import itertools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import f4_pops_model
import helpers
from f4_pops_model import SUMS
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)


def fixture_sets():
    """-> (the fixture, its window table, [(set, pos, freqs, ninds)])"""
    k = helpers.load_golden("f4_exact.json")
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    sets = [(s, np.array(s["pos"], dtype=np.uint32), [np.array(f, dtype=np.float64) for f in s["freq"]],
             [np.array(c, dtype=np.int32) for c in s["nind"]]) for s in k["sets"]]
    return k, win, sets


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/f4_exact.json is reproducible, holds data only, and its inputs reach sites below minind, ties, 0 and 1."""
    import make_f4_exact as gen
    k, win, sets = fixture_sets()
    assert set(k) == {"source", "windows", "sets"} and [s["n_pops"] for s in k["sets"]] == [4, 5]
    assert gen.windows() == k["windows"] and [0, gen.N_SITES] in k["windows"]
    for (s, pos, freqs, ninds), (n_pops, seed) in zip(sets, gen.SETS):
        gpos, gf, gn = gen.inputs(s["n_pops"], seed)
        assert n_pops == s["n_pops"] and gpos == s["pos"] and gf == s["freq"] and gn == s["nind"]
        assert set(s) == {"n_pops", "pos", "freq", "nind", "cases"} and [c["minind"] for c in s["cases"]] == [1, 5]
        for case in s["cases"]:
            assert [tuple(q["quartet"]) for q in case["quartets"]] == f4_pops_model.all_quartet_order(s["n_pops"])
            for q in case["quartets"]:
                assert set(q) == {"quartet", "n"} | set(SUMS)
                sites = gen.exact_sites(s["freq"], s["nind"], q["quartet"], case["minind"])
                for w, (lo, hi) in enumerate(k["windows"]):
                    a, b, c, n = gen.exact_window(sites, lo, hi)
                    assert (gen.nearest(a), gen.nearest(b), gen.nearest(c), n) == (q[SUMS[0]][w], q[SUMS[1]][w], q[SUMS[2]][w], q["n"][w])
                ok = np.array([x is not None for x in sites])
                assert 0 < ok.sum() < ok.size  # sites with nInd below minind, and sites above
                for a, b in itertools.combinations(q["quartet"], 2):
                    assert np.any((freqs[a] == freqs[b]) & ok), (case["minind"], q["quartet"], "equal frequencies", a, b)
                for x in q["quartet"]:
                    assert np.any(((freqs[x] == 0) | (freqs[x] == 1)) & ok), (case["minind"], q["quartet"], x)
                assert any(v < 0 for v in q[SUMS[0]]) and any(v > 0 for v in q[SUMS[0]])  # both signs among the windows


def test_the_three_pairings_cancel_exactly_in_the_fixture():
    """s0 - s1 + s2 = 0 in rationals, at every counted site and so in every window of the fixture."""
    import make_f4_exact as gen
    k, win, sets = fixture_sets()
    seen = 0
    for s, pos, freqs, ninds in sets:
        for quartet in gen.quartets_of(s["n_pops"]):
            sites = gen.exact_sites(s["freq"], s["nind"], quartet, 1)
            for x in sites:
                if x is not None:
                    assert x[0] - x[1] + x[2] == 0 and all(isinstance(v, Fraction) for v in x)
                    seen += 1
            for lo, hi in k["windows"]:
                a, b, c, _ = gen.exact_window(sites, lo, hi)
                assert a - b + c == 0
    assert seen > 100


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site lines of the definition, summed: within 1e-12 A + 1e-15 (hi - lo) of the exact rationals, A the window's
    Σ|product|, counts exact.  The per-site floor: a term is a product of two differences of values <= 1, three roundings of
    2^-53 of values <= 1: below 1e-15 per site."""
    k, win, sets = fixture_sets()
    length = (win["hi"] - win["lo"]).astype(np.float64)
    whole = k["windows"].index([0, 64])
    worst = 0.0
    for s, pos, freqs, ninds in sets:
        for case in s["cases"]:
            rows, tot, A, A_tot = f4_pops_model.model(pos, freqs, ninds, case["minind"], win)
            # the ranges-only evaluation is the same model with float64 pairwise sums: 1e-13 of A apart at most
            r2, t2, A2, At2 = f4_pops_model.model(pos, freqs, ninds, case["minind"], win, ranges_only=True)
            assert np.array_equal(r2["n"], rows["n"]) and np.array_equal(t2["neff"], tot["neff"]) and np.array_equal(t2["nskip"], tot["nskip"])
            for f in SUMS:
                assert np.all(np.abs(r2[f] - rows[f]) <= 1e-13 * A[f]) and np.all(np.abs(A2[f] - A[f]) <= 1e-13 * A[f])
                assert np.all(np.abs(t2[f] - tot[f]) <= 1e-13 * A_tot[f]) and np.all(np.abs(At2[f] - A_tot[f]) <= 1e-13 * A_tot[f])
            for t, q in enumerate(case["quartets"]):
                assert np.array_equal(rows[t]["n"], np.array(q["n"], dtype=np.uint32))
                assert int(tot[t]["neff"]) == q["n"][whole] and int(tot[t]["nskip"]) == pos.size - q["n"][whole]
                assert not rows[t]["reserved_"].any()
                for fld in SUMS:
                    err = np.abs(rows[t][fld] - np.array(q[fld]))
                    worst = max(worst, float(err[length == 1].max()))
                    assert np.all(err <= 1e-12 * A[fld][t] + 1e-15 * length), (s["n_pops"], case["minind"], q["quartet"], fld)
                    assert abs(float(tot[t][fld]) - q[fld][whole]) <= 1e-12 * A_tot[fld][t] + 1e-15 * pos.size
                    assert A_tot[fld][t] == A[fld][t][whole]
    print(f"largest one-site error of the model against the exact value: {worst:.3e}")


def test_flipping_the_allele_in_all_populations_keeps_the_bits():
    """Frequencies that are multiples of 2^-10: 1 - p is exact, the differences only change sign, and a product of two of them
    keeps its bits: the three terms keep their bits under p -> 1 - p in ALL populations."""
    rng = np.random.default_rng(4100)
    n = 4096
    p = [rng.integers(0, 1025, n) / 1024.0 for _ in range(4)]
    a, _ = f4_pops_model.site_terms(*p)
    b, _ = f4_pops_model.site_terms(*[1.0 - x for x in p])
    for x, y in zip(a, b):
        assert np.array_equal((x + 0.0).view(np.uint64), (y + 0.0).view(np.uint64))
    assert np.any(a[0] < 0) and np.any(a[0] > 0)


def test_orders_against_itertools():
    import popgenomicstools_amd as pgt
    for k in range(0, 9):
        want = list(itertools.combinations(range(k), 4))
        assert pgt.all_quartet_order(k) == want == f4_pops_model.all_quartet_order(k)
    assert [len(pgt.all_quartet_order(k)) for k in (4, 5, 6)] == [1, 5, 15]
    for q in itertools.combinations(range(6), 4):
        i, j, k, l = q
        got = pgt.pairing_order(*q)
        assert got == (((i, j), (k, l)), ((i, k), (j, l)), ((i, l), (j, k)))
        # the three ways to split four populations into two pairs, each once, the pair with i first
        splits = {frozenset((frozenset(a), frozenset(set(q) - set(a)))) for a in itertools.combinations(q, 2)}
        assert {frozenset((frozenset(a), frozenset(b))) for a, b in got} == splits and len(splits) == 3
    assert {"f4_window_pops", "all_quartet_order", "pairing_order"} <= set(pgt.__all__)


def test_tree_bytes_only_for_four_to_six_populations():
    """0 outside 4 ... 6; inside, the bytes of the tree layout: per level a node array of 3 Q doubles and one of Q u32, each
    padded to 256 bytes — level 1 has 512-site nodes, level 2 8192-site nodes, 64 children per node above — and behind the
    levels the same two arrays with one node per build wave.  The level-2 and higher node counts and the number of build waves
    are read off a sibling of the same layout: pgt_dxy_pops_tree_bytes at 2 populations is that layout with ONE double and
    one u32 per node, pgt_fst_pops_tree_bytes at 2 populations with TWO doubles and one u32."""
    lib = _lib.load()

    def pad(b):
        return (b + 255) // 256 * 256

    def node_counts(n):
        """-> the node counts of the levels, level 1 first: 8192-site level-2 nodes (one at least), 16 level-1 nodes of 512 sites
        under each, and 64 children per node above while a level has more than 64 nodes"""
        counts = [max(1, -(-n // 8192)) * 16, max(1, -(-n // 8192))]
        while counts[-1] > 64:
            counts.append(-(-counts[-1] // 64))
        return counts

    def layout(n, items, sums, waves):
        return sum(pad(c * items * 8 * sums) + pad(c * items * 4) for c in node_counts(n)) + pad(waves * items * 8 * sums) + pad(waves * items * 4)

    # the build waves the workspace reserves, from the sibling with the smallest node
    waves = next(w for w in (1024, 2048, 4096) if layout(0, 1, 1, w) == lib.pgt_dxy_pops_tree_bytes(2, 0))
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        if layout(n, 1, 1, waves) != lib.pgt_dxy_pops_tree_bytes(2, n) or layout(n, 1, 2, waves) != lib.pgt_fst_pops_tree_bytes(2, n):
            pytest.fail(f"the test's restatement of the tree layout does not give the siblings' sizes at n = {n}")
        for k in range(0, 12):
            b = lib.pgt_f4_pops_tree_bytes(k, n)
            assert (b > 0) == (4 <= k <= 6), (k, n, b)
            if 4 <= k <= 6:
                q = len(list(itertools.combinations(range(k), 4)))
                assert b == layout(n, q, 3, waves), (k, n, b)
        assert lib.pgt_f4_pops_tree_bytes(4, n) == lib.pgt_f3_pops_tree_bytes(3, n)  # one item of three sums either way
        sizes = [lib.pgt_f4_pops_tree_bytes(k, n) for k in (4, 5, 6)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    import popgenomicstools_amd as pgt
    assert pgt.Context.f4_pops_tree_bytes(5, 12345) == lib.pgt_f4_pops_tree_bytes(5, 12345)
    assert pgt.Context.f4_pops_tree_bytes(7, 12345) == 0 and pgt.Context.f4_pops_tree_bytes(3, 12345) == 0
    for q in range(0, 20):
        assert (lib.pgt_f4_jackknife_work_bytes(q, 1000) > 0) == (1 <= q <= 15)
        if 1 <= q <= 15:
            assert lib.pgt_f4_jackknife_work_bytes(q, 1000) == lib.pgt_f3_jackknife_work_bytes(q, 1000) == pgt.Context.f4_jackknife_work_bytes(q, 1000)


def test_header_binding_and_dtypes():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_f4_pops_tree_bytes", "pgt_f4_pops_reduce_dev", "pgt_f4_pops_reduce", "pgt_f4_jackknife_work_bytes", "pgt_f4_jackknife_dev",
             "pgt_f4_jackknife")
    for name in names:
        assert name + "(" in text
    assert "} pgt_f4_row;" in text and "} pgt_f4_total;" in text and "} pgt_f4_jack;" in text
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_f4_row, pgt_f4_total, pgt_f4_jack" in text
    for line in ("d_ab = p_a - p_b", "s0 = d_ij * d_kl", "s1 = d_ik * d_jl", "s2 = d_il * d_jk", "out[q * n_win + w]", "pgt_f4_row (48 bytes)",
                 "pgt_f4_total (40 bytes", "pgt_f4_jackknife_dev (48 bytes, the layout of pgt_f3_jack)", "1e-9 * A + 1e-12", "1 <= n_quartets <= 15", "user-chosen quartet lists"):
        assert line in text, line
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    row, tot, jack = _lib.F4_ROW_DTYPE, _lib.F4_TOTAL_DTYPE, _lib.F4_JACK_DTYPE
    assert row.names == ("start", "end", "mid", "n", "reserved_") + SUMS and row.itemsize == 48
    assert [row.fields[f][1] for f in row.names] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert tot.names == SUMS + ("neff", "nskip") and tot.itemsize == 40 and [tot.fields[f][1] for f in tot.names] == [0, 8, 16, 24, 32]
    assert jack.names == ("f4", "f4_jack", "se", "z", "n_sites", "n_blocks", "pad_") and jack.itemsize == 48
    assert [jack.fields[f][1] for f in jack.names] == [0, 8, 16, 24, 32, 40, 44]
    for a, b in zip(SUMS, ("f3_i", "f3_j", "f3_k")):  # the jackknife's row loader serves both row types
        assert row.fields[a][1] == _lib.F3_ROW_DTYPE.fields[b][1]
    assert [jack.fields[f][1] for f in jack.names] == [_lib.F3_JACK_DTYPE.fields[f][1] for f in _lib.F3_JACK_DTYPE.names]
    # the C compiler's view of the same structs
    api = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_api.cpp")).read()
    assert "sizeof(pgt_f4_row) == 48 && offsetof(pgt_f4_row, reserved_) == 16 && offsetof(pgt_f4_row, f4_ij_kl) == offsetof(pgt_f3_row, f3_i)" in api


def test_the_build_grid_constants_are_the_ones_the_gpu_test_assumes():
    """tests/test_f4_pops_grid.py takes its cases from tests/pops_grid_shapes.py, whose POPS_ONE_WAVE_FROM must be this
    statistic's kOneWaveFrom; K = 4 is a two-wave K and K = 5 a one-wave K."""
    import pops_grid_shapes as shapes
    src = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_f4_pops_kernels.hip")).read()
    m = re.search(r"static constexpr int kOneWaveFrom = (\d+);", src)
    assert m and int(m.group(1)) == shapes.POPS_ONE_WAVE_FROM == 5
    assert re.search(r"static constexpr int kQueryOneWaveFrom = 6;", src) and re.search(r"kMinPops = 4, kMaxPops = 6;", src)
    assert "static constexpr const char *kOneWaveKnob = nullptr;" in src and "using Counts = CountBits;" in src
    assert shapes.pops_build(1025, 5) == (2, 513, 516) and shapes.pops_build(2049, 4) == (2, 1025, 1028)
    assert shapes.pops_build(1024, 5)[0] == 1 and shapes.pops_build(2048, 4)[0] == 1  # the smallest counts with two rounds
    walk = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_pops_walk.h")).read()
    assert "constexpr int all_quartet_count(int np) { return np * (np - 1) * (np - 2) * (np - 3) / 24; }" in walk


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (3, 7):
        with pytest.raises(_lib.PgtError, match="f4_window_pops: 4 ... 6 populations, one frequency and one count column each") as e:
            pgt.f4_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1)
        assert e.value.code == _lib.PGT_EARG
        with pytest.raises(_lib.PgtError, match="f4_window_pops: 4 ... 6 populations"):
            pgt.f4_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1, jackknife=True)
    with pytest.raises(_lib.PgtError, match="4 ... 6 populations"):
        pgt.f4_window_pops(ids, pos, [z] * 4, [c] * 3, 2, 2, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.f4_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 2, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.f4_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 2, 1, 0)
    for W, S in ((4, 2), (0, 0)):
        with pytest.raises(_lib.PgtError, match="f4_window_pops: the block jackknife needs disjoint windows") as e:
            pgt.f4_window_pops(ids, pos, [z] * 4, [c] * 4, W, S, 1, 1, jackknife=True)
        assert e.value.code == _lib.PGT_EARG and f"winsize {W}" in str(e.value) and f"stepsize {S}" in str(e.value)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "f4WindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_states_the_definition_and_what_is_left_out(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("f4WindowPops [options] -out PREFIX", "(4 <= K <= 6)", "f4(a,b; c,d) = (p_a - p_b)(p_c - p_d)", "MEAN",
                 "ALL files must report the frequency of the SAME allele", "|Z| above about 3 rejects", "the tree ((a,b),(c,d))",
                 "f4(i,j; k,O) is the numerator of Patterson's D", "-jackknife", "-skip_missing", "-sizefile", "-fixedsite",
                 "PREFIX.pop<i>_pop<j>_pop<k>_pop<l>.f4", "PREFIX.global", "PREFIX.jackknife", "(1) a\n(2) b\n(3) c\n(4) d",
                 "f4-ratio admixture proportions", "user-chosen quartet lists", "K = 7", "One GPU is used", "No passes mode",
                 "PGT_DXY_SYNC=reference is not offered"):
        assert word in r.stdout, word


def test_the_refusals_that_need_no_device(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(7)]
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    f3 = os.path.join(BIN, "f3WindowPops")
    for k in (3, 7):
        r = run([tool] + head + missing[:k])
        assert r.returncode == 255 and r.stdout == "", (k, r.returncode)
        assert f"f4WindowPops: between 4 and 6 MAF files are needed ({k} given)" in r.stderr and "Unable to open" not in r.stderr, r.stderr
    cases = [
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-jackknife", "1"], "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0"], "-jackknife 1 needs windows as its blocks"),
        (["-jackknife", "2", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "-jackknife must be 0 or 1 (given: 2)"),
        (["-fd", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "Unknown command"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + ["-out", out] + missing[:4])
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
        r3 = run([f3] + opts + ["-out", out] + missing[:4])  # f3WindowPops refuses the same options in the same words
        assert r3.returncode == 255 and r3.stderr == r.stderr, (opts, r3.stderr, r.stderr)
    # without a refusal the run gets as far as the files
    r = run([tool, "-jackknife", "1"] + head + missing[:4])
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
