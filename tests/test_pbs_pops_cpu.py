"""CPU: the PBS front end (pgt_pbs_pops_reduce*, pbsWindowPops) without a device — the exact-rational fixture, the NumPy model the
GPU tests compare against, the model's identity with the pair models where the third population is counted everywhere, the
workspace size, the declarations, and the refusals of the Python mirror and of the command line that come before the device is
opened."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fst_hudson_model
import fst_pops_model
import helpers
import pbs_pops_model
import special_inputs as si
from pbs_pops_model import PAIRS, PBS, SUMS
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)
PAIR_MODELS = {"wc": fst_pops_model, "hudson": fst_hudson_model}


def fixture_sets():
    """-> (the fixture, its window table, [(set, pos, freqs, ninds)])"""
    k = helpers.load_golden("pbs_exact.json")
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    sets = [(s, np.array(s["pos"], dtype=np.uint32), [np.array(f, dtype=np.float64) for f in s["freq"]],
             [np.array(c, dtype=np.int32) for c in s["nind"]]) for s in k["sets"]]
    return k, win, sets


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/pbs_exact.json is reproducible, holds data only, its inputs reach ties, 0 and 1 at counted sites, and every
    trio has sites that one of its pairs counts and the trio does not."""
    import make_pbs_exact as gen
    k, win, sets = fixture_sets()
    assert set(k) == {"source", "windows", "sets"} and [s["n_pops"] for s in k["sets"]] == [3, 4]
    assert gen.windows() == k["windows"] and [0, gen.N_SITES] in k["windows"]
    for (s, pos, freqs, ninds), (n_pops, seed) in zip(sets, gen.SEEDS):
        gpos, gf, gn = gen.inputs(n_pops, seed)
        assert s["n_pops"] == n_pops and gpos == s["pos"] and gf == s["freq"] and gn == s["nind"]
        assert set(s) == {"n_pops", "pos", "freq", "nind", "cases"}
        assert [(c["estimator"], c["minind"]) for c in s["cases"]] == [("wc", 1), ("wc", 5), ("hudson", 1), ("hudson", 5)]
        for case in s["cases"]:
            assert [tuple(tr["trio"]) for tr in case["trios"]] == pbs_pops_model.all_trio_order(n_pops)
            for tr in case["trios"]:
                assert set(tr) == {"trio", "n"} | set(SUMS) and gen.FIELDS == SUMS
                sites = gen.exact_sites(s["freq"], s["nind"], tr["trio"], case["minind"], case["estimator"])
                for w, (lo, hi) in enumerate(k["windows"]):
                    r = gen.exact_window(sites, lo, hi)
                    assert tuple(gen.nearest(x) for x in r[:6]) + (r[6],) == tuple(tr[f][w] for f in SUMS) + (tr["n"][w],)
                ok = np.array([x is not None for x in sites])
                i, j, kk = tr["trio"]
                assert 0 < ok.sum() < ok.size
                for what, m in (("p_i == p_j", freqs[i] == freqs[j]), ("p_i == p_k", freqs[i] == freqs[kk]), ("p_j == p_k", freqs[j] == freqs[kk])):
                    assert np.any(m & ok), (case["minind"], tr["trio"], what)
                for x in (i, j, kk):
                    assert np.any(((freqs[x] == 0) | (freqs[x] == 1)) & ok), (case["minind"], tr["trio"], x)
                for a, b in pbs_pops_model.pairs_of(i, j, kk):  # the pair's own site set is larger than the trio's
                    pair_ok = (ninds[a] >= case["minind"]) & (ninds[b] >= case["minind"])
                    assert np.any(pair_ok & ~ok), (case["minind"], tr["trio"], (a, b))
                assert any(v < 0 for v in tr["num_ij"]) and any(v > 0 for v in tr["num_ij"])  # both signs among the windows


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site lines of the pair models, summed over the trio's sites: within 1e-12 A + 1e-15 (hi - lo) of the exact
    rationals, A the window's sum of the absolute values of the terms a site's value is built from, counts exact."""
    k, win, sets = fixture_sets()
    length = (win["hi"] - win["lo"]).astype(np.float64)
    whole = k["windows"].index([0, 96])
    worst = 0.0
    for s, pos, freqs, ninds in sets:
        for case in s["cases"]:
            rows, tot, A, A_tot = pbs_pops_model.model(pos, freqs, ninds, case["minind"], win, case["estimator"])
            r2, t2, A2, At2 = pbs_pops_model.model(pos, freqs, ninds, case["minind"], win, case["estimator"], ranges_only=True)
            assert np.array_equal(r2["n"], rows["n"]) and np.array_equal(t2["neff"], tot["neff"]) and np.array_equal(t2["nskip"], tot["nskip"])
            for f in SUMS:
                assert np.all(np.abs(r2[f] - rows[f]) <= 1e-13 * A[f]) and np.all(np.abs(A2[f] - A[f]) <= 1e-13 * A[f])
                assert np.all(np.abs(t2[f] - tot[f]) <= 1e-13 * A_tot[f])
            for t, tr in enumerate(case["trios"]):
                assert np.array_equal(rows[t]["n"], np.array(tr["n"], dtype=np.uint32))
                assert int(tot[t]["neff"]) == tr["n"][whole] and int(tot[t]["nskip"]) == pos.size - tr["n"][whole]
                for fld in SUMS:
                    err = np.abs(rows[t][fld] - np.array(tr[fld]))
                    worst = max(worst, float((err[length == 1] / np.maximum(A[fld][t][length == 1], 1e-300)).max()))
                    assert np.all(err <= 1e-12 * A[fld][t] + 1e-15 * length), (s["n_pops"], case, tr["trio"], fld)
                    assert abs(float(tot[t][fld]) - tr[fld][whole]) <= 1e-12 * A_tot[fld][t] + 1e-15 * pos.size
                    assert A_tot[fld][t] == A[fld][t][whole]
    print(f"largest one-site error of the model against the exact value, relative to A: {worst:.3e}")


def test_the_finishing_lines():
    """No counted site: every pbs is +0.0 by its bits.  A negative FST gives a negative T, FST = 1 an infinite one, two of them
    NaN; the three statistics of a trio are the three half-sums of its branches."""
    z = np.zeros(1)
    pbs, T = pbs_pops_model.finish([z, z, z], [z, z, z])
    assert all(np.array_equal(x.view(np.uint64), np.zeros(1, dtype=np.uint64)) for x in pbs)
    pbs, T = pbs_pops_model.finish([-0.1, 0.5, 0.2], [1.0, 1.0, 1.0])
    assert T[0] < 0 < T[1] and np.isclose(pbs[0], (T[0] + T[1] - T[2]) / 2) and np.isclose(pbs[1] + pbs[2], T[2])
    pbs, T = pbs_pops_model.finish([1.0, 0.5, 0.2], [1.0, 1.0, 1.0])
    assert np.isposinf(T[0]) and np.isposinf(pbs[0]) and np.isposinf(pbs[1]) and np.isneginf(pbs[2])
    pbs, T = pbs_pops_model.finish([1.0, 1.0, 0.2], [1.0, 1.0, 1.0])
    assert np.isposinf(pbs[0]) and np.isnan(pbs[1]) and np.isnan(pbs[2])


@pytest.mark.parametrize("estimator", ["wc", "hudson"])
def test_with_the_third_population_counted_everywhere_the_trio_sums_are_the_pair_sums(estimator):
    """Where every population of the trio's complement has data at every site, the trio's site set is each pair's own: the
    model's sums equal the pair model's asum / bsum bit for bit (the same per-site lines, the same prefix sums)."""
    rng = np.random.default_rng(1807)
    n, K = 3000, 4
    pos = np.cumsum(rng.integers(1, 30, n)).astype(np.uint32)
    freqs = [np.round(rng.random(n), 6) for _ in range(K)]
    ninds = [rng.integers(5, 21, n).astype(np.int32) for _ in range(K)]  # all >= minind = 5
    win = np.zeros(40, dtype=WIN_DTYPE)
    win["lo"] = np.sort(rng.integers(0, n - 300, 40))
    win["hi"] = win["lo"] + rng.integers(7, 300, 40)
    rows, tot, _, _ = pbs_pops_model.model(pos, freqs, ninds, 5, win, estimator)
    prow, ptot = PAIR_MODELS[estimator].model(pos, freqs, ninds, 5, win)
    from popgenomicstools_amd.window_scan import pair_order
    index = {p: x for x, p in enumerate(pair_order(K))}
    for t, trio in enumerate(pbs_pops_model.all_trio_order(K)):
        for name, pair in zip(PAIRS, pbs_pops_model.pairs_of(*trio)):
            p = index[pair]
            assert np.array_equal(rows[t]["n"], prow[p]["n"])
            assert np.array_equal(rows[t][f"num_{name}"], prow[p]["asum"] + 0.0) and np.array_equal(rows[t][f"den_{name}"], prow[p]["bsum"] + 0.0)
            assert tot[t][f"num_{name}"] == ptot[p]["asum"] and tot[t]["neff"] == ptot[p]["neff"]
    # and with the third population short of data at some sites the trio counts fewer
    ninds[2][::7] = 0
    rows2, _, _, _ = pbs_pops_model.model(pos, freqs, ninds, 5, win, estimator)
    assert np.all(rows2[0]["n"] < rows[0]["n"])  # trio (0, 1, 2): every window holds at least seven sites, one of them without population 2
    assert np.array_equal(rows2[1]["n"], rows[1]["n"])  # trio (0, 1, 3) does not hold population 2


def test_work_bytes_only_for_three_to_six_populations():
    lib = _lib.load()
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        for n_win in (0, 1, 1000):
            for k in range(0, 12):
                b = lib.pgt_pbs_pops_work_bytes(k, n, n_win)
                assert (b > 0) == (3 <= k <= 6), (k, n, n_win, b)
                if 3 <= k <= 6:
                    T = k * (k - 1) * (k - 2) // 6
                    # the tree of one pass (f3's), two passes' scratch rows and scratch totals of 40 bytes
                    assert b >= lib.pgt_f3_pops_tree_bytes(k, n) + 2 * T * n_win * 40 + 2 * T * 40 and b % 256 == 0
                    assert b <= lib.pgt_f3_pops_tree_bytes(k, n) + 2 * T * n_win * 40 + 2 * T * 40 + 5 * 256
            sizes = [lib.pgt_pbs_pops_work_bytes(k, n, n_win) for k in (3, 4, 5, 6)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    import popgenomicstools_amd as pgt
    assert pgt.Context.pbs_pops_work_bytes(5, 12345, 17) == lib.pgt_pbs_pops_work_bytes(5, 12345, 17)
    assert pgt.Context.pbs_pops_work_bytes(7, 12345, 17) == 0 and pgt.Context.pbs_pops_work_bytes(2, 12345, 17) == 0


def test_header_binding_and_sizes():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_pbs_pops_work_bytes", "pgt_pbs_pops_reduce_dev", "pgt_pbs_hudson_pops_reduce_dev", "pgt_pbs_pops_reduce", "pgt_pbs_hudson_pops_reduce")
    for name in names:
        assert name + "(" in text
    assert "} pgt_pbs_row;" in text and "} pgt_pbs_total;" in text
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_pbs_row, pgt_pbs_total" in text
    for line in ("fst_xy = den_xy != 0 ? num_xy / den_xy : 0", "T_xy   = -log(1 - fst_xy)", "pbs_i  = ((T_ij + T_ik) - T_jk) * 0.5 + 0.0",
                 "pbs_j  = ((T_ij + T_jk) - T_ik) * 0.5 + 0.0", "pbs_k  = ((T_ik + T_jk) - T_ij) * 0.5 + 0.0", "NOTHING IS CLAMPED",
                 "inf - inf gives NaN", "out[t * n_win + w]", "offsets 40, 48, 56", "offsets 72, 80", "PBSn1"):
        assert line in text, line
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.PBS_ROW_DTYPE.names == ("start", "end", "mid", "n") + PBS + SUMS and _lib.PBS_ROW_DTYPE.itemsize == 88
    assert _lib.PBS_TOTAL_DTYPE.names == PBS + SUMS + ("neff", "nskip") and _lib.PBS_TOTAL_DTYPE.itemsize == 88
    assert _lib.PBS_ROW_DTYPE.fields["pbs_i"][1] == 16 and _lib.PBS_ROW_DTYPE.fields["num_ij"][1] == 40 and _lib.PBS_ROW_DTYPE.fields["den_jk"][1] == 80
    assert _lib.PBS_TOTAL_DTYPE.fields["num_ij"][1] == 24 and _lib.PBS_TOTAL_DTYPE.fields["neff"][1] == 72
    import popgenomicstools_amd as pgt
    assert "pbs_window_pops" in pgt.__all__ and callable(pgt.pbs_window_pops)
    for k in range(3, 7):
        assert pgt.all_trio_order(k) == pbs_pops_model.all_trio_order(k)


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (2, 7):
        with pytest.raises(_lib.PgtError, match="pbs_window_pops: 3 ... 6 populations, one frequency and one count column each") as e:
            pgt.pbs_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1)
        assert e.value.code == _lib.PGT_EARG
    with pytest.raises(_lib.PgtError, match="3 ... 6 populations"):
        pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 2, 2, 2, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 1, 0)
    for bad in ("reynolds", None, 1):
        with pytest.raises(_lib.PgtError, match='pbs_window_pops: estimator must be "wc" or "hudson"') as e:
            pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 1, 1, estimator=bad)
        assert e.value.code == _lib.PGT_EARG


# ---- what the GPU modules of the grid strides and of the special values assume ---------------------------------------------------
def test_the_grid_constants_are_the_ones_the_gpu_test_assumes():
    """tests/test_pbs_pops_grid.py takes its tile counts from PbsPass' own kOneWaveFrom: K = 5 is a one-wave K with 1024 build
    waves at most, K = 3 a two-wave K with 2048; the query kernel takes one wave per SIMD from K = 6."""
    import pops_grid_shapes as shapes
    src = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_pbs_pops_kernels.hip")).read()
    m = re.search(r"static constexpr int kOneWaveFrom = (\d+);", src)
    assert m and int(m.group(1)) == 5 and src.count("kOneWaveFrom = ") == 1
    assert re.search(r"static constexpr int kQueryOneWaveFrom = 6;", src) and re.search(r"kMinPops = 3, kMaxPops = 6;", src)
    assert re.search(r"static constexpr const char \*kOneWaveKnob = nullptr;", src)  # no environment knob moves the occupancy
    assert shapes.balanced_build(1025, shapes.ONE_WAVE_BUILD_WAVES) == (2, 513, 516)   # wc, K = 5
    assert shapes.balanced_build(2049, shapes.MAX_BUILD_WAVES) == (2, 1025, 1028)      # hudson, K = 3
    assert shapes.balanced_build(1024, shapes.ONE_WAVE_BUILD_WAVES)[0] == 1 and shapes.balanced_build(2048, shapes.MAX_BUILD_WAVES)[0] == 1
    assert shapes.tiles_of_wave(1025, 516).max() == 2 and shapes.tiles_of_wave(2049, 1028).max() == 2
    assert shapes.QUERY_N_WIN[-1] == shapes.QUERY_WAVES + 5 == 262_149


def _trio_terms(stat, ijk, f, c, minind):
    ok = si.pops_counted(ijk, c, minind)
    return ok, [np.where(ok, x, 0.0) for x in si.pops_site_terms(stat, ijk, f, c)]


def test_the_special_value_inputs_have_the_shapes_the_gpu_test_claims():
    """The very inputs of tests/test_special_values_pbs.py, without a device: the planted sites are counted and the clean terms
    finite and at most 8 (special_inputs.window_sums asserts it); the model's classes at a frequency of +-inf; every trio of the
    count cases has counted and uncounted sites, the fewest counted as recorded, every counted term finite and at most 1; the
    denormal columns reach denormal sums and counted rows with all three denominators 0, whose pbs is +0.0 by the model."""
    from test_special_values_f3 import PLANTED
    n = si.POPS_N
    assert si.POPS_SUMS["pbs"] == si.POPS_SUMS["pbs_hudson"] == SUMS and si.pops_dtypes("pbs") == (_lib.PBS_ROW_DTYPE, _lib.PBS_TOTAL_DTYPE)
    for k in (3, 6):
        assert si.pops_items("pbs", k) == si.pops_items("pbs_hudson", k) == pbs_pops_model.all_trio_order(k)
    sites = np.array(sorted(PLANTED))
    # planted at counted sites: Hudson's sums are the definition's on the IEEE operands
    for k, who in ((3, 1), (6, 1)):
        f0, c = si.pops_clean_columns(n, k, 7100 + 10 * k + who, planted=tuple(PLANTED))
        f = [x.copy() for x in f0]
        for s, v in PLANTED.items():
            f[who][s] = v
        for ijk in pbs_pops_model.all_trio_order(k):
            ok, terms = _trio_terms("pbs_hudson", ijk, f, c, si.POPS_MININD)
            assert ok[sites].all()
            for fld, x in zip(SUMS, terms):
                _, A, _ = si.window_sums(x, [0], [n])  # finite terms at most 8
                reads = who in dict(zip(pbs_pops_model.PAIRS, pbs_pops_model.pairs_of(*ijk)))[fld[4:]]
                assert np.isfinite(np.delete(x, sites)).all() and np.isfinite(A).all()
                if not reads:
                    assert np.isfinite(x).all()
                    continue
                assert np.isnan(x[511]) and np.isfinite(x[n - 1])  # the NaN site; the denormal is an ordinary value
                for s in (4001, 8192):  # +inf and -inf: num = +inf, den = NaN
                    assert np.isposinf(x[s]) if fld.startswith("num") else np.isnan(x[s]), (ijk, fld, s)
    # the division form of the Weir-Cockerham model gives NaN for both values at a frequency of +-inf, where the kernel's identity
    # with a reciprocal gives a = +inf: the class of such a sum is left open, and the GPU test asks for a non-finite one
    nine = np.array([9, 9], dtype=np.int32)
    for v in (np.inf, -np.inf):
        num, den = pbs_pops_model.site_values("wc", np.array([v, 0.25]), np.array([0.25, v]), nine, nine)
        assert np.isnan(num).all() and np.isnan(den).all()
        num, den = pbs_pops_model.site_values("hudson", np.array([v, 0.25]), np.array([0.25, v]), nine, nine)
        assert np.isposinf(num).all() and np.isnan(den).all()
    # counts as values
    fewest = {(3, 1): 565, (3, 20): 302, (3, si.I32_MAX): 68, (6, 1): 503, (6, 20): 294, (6, si.I32_MAX): 62, (3, "realistic"): 8454, (6, "realistic"): 8427}
    for (k, minind), want in fewest.items():
        real = minind == "realistic"
        m = si.REALISTIC_MININD if real else minind
        f, c = si.count_case_columns("pbs", k, m, real)
        counted = []
        for ijk in pbs_pops_model.all_trio_order(k):
            for stat in ("pbs", "pbs_hudson"):
                ok, terms = _trio_terms(stat, ijk, f, c, m)
                assert np.isfinite(np.stack(terms)).all() and np.abs(np.stack(terms)).max() <= 1.0, (k, minind, ijk, stat)
            counted.append(int(ok.sum()))
        assert 0 < min(counted) == want and max(counted) < n, (k, minind, min(counted), max(counted))
    # denormal and zero sums
    tiny = 2.0 ** -1022
    f, c = si.denormal_columns(3)
    name, win = si.denormal_tables()[0]
    lo, hi = win["lo"].astype(np.int64), win["hi"].astype(np.int64)
    assert name == "one site"
    for stat, n_denormal in (("pbs", 646), ("pbs_hudson", 643)):
        ok, terms = _trio_terms(stat, (0, 1, 2), f, c, si.POPS_MININD)
        row = np.zeros(lo.size, dtype=_lib.PBS_ROW_DTYPE)
        row["n"] = ok[lo]
        for fld, x in zip(SUMS, terms):
            row[fld], _, finite = si.window_sums(x, lo, hi)
            assert finite.all()
        assert sum(int(np.count_nonzero((np.abs(row[fld]) < tiny) & (row[fld] != 0))) for fld in SUMS) == n_denormal
        zero = [(row["n"] > 0) & (row[f"den_{p}"] == 0) for p in pbs_pops_model.PAIRS]
        # 182 zero denominators among the counted rows' pairs; in 56 of the 266 counted rows all three are 0
        assert sum(int(z.sum()) for z in zero) == 182 and int((zero[0] & zero[1] & zero[2]).sum()) == 56 and int(ok.sum()) == 266
        pbs, _ = pbs_pops_model.finish_rows(row)
        for x in pbs:
            assert np.isfinite(x).all() and not x[zero[0] & zero[1] & zero[2]].view(np.uint64).any()


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "pbsWindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_states_the_site_rule_the_ieee_results_and_what_is_left_out(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("pbsWindowPops [options] -out PREFIX", "(3 <= K <= 6)", "-estimator", "wc (Weir-Cockerham components) or hudson",
                 "ALL THREE of its populations have at least -minind individuals", "The .fst files of fstWindowPops",
                 "wherever the third population lacks data", "T = -log(1 - FST)", "(T_xa + T_xb - T_ab) / 2", "Nothing is clamped",
                 "inf:", "nan:", "PREFIX.pop<i>_pop<j>_pop<k>.pbs", "PREFIX.global", "PBSn1", "block jackknife", "user-chosen trio lists",
                 "One GPU is used", "No passes mode"):
        assert word in r.stdout, word


def test_the_refusals_that_need_no_device(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(7)]
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4"]
    for k in (2, 7):
        r = run([tool] + head + ["-out", out] + missing[:k])
        assert r.returncode == 255 and r.stdout == "", (k, r.returncode)
        assert f"pbsWindowPops: between 3 and 6 MAF files are needed ({k} given)" in r.stderr and "Unable to open" not in r.stderr, r.stderr
    cases = [
        (head + ["-estimator", "reynolds", "-out", out], "-estimator must be wc or hudson (given: reynolds)"),
        (head, "Must supply -out PREFIX"),
        (head + ["-jackknife", "1", "-out", out], "Unknown command"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + missing[:3])
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
    # without a refusal the run gets as far as the files, with either estimator
    for est in ("wc", "hudson"):
        r = run([tool, "-estimator", est] + head + ["-out", out] + missing[:3])
        assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
