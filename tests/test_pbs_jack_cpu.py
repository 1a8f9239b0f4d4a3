"""CPU: the block jackknife of PBS and PBSn1 (pgt_pbs_jackknife*, `pbsWindowPops -blockjack 1`, `-pbsn1 1`, pbsn1_of) without a
device — the two restatements of tests/pbs_jack_model.py held to each other and to the hand cases, the recorded 60-digit
reference, the header, the binding and the workspace size against the library, and every refusal that needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import dstat_jack_shapes as shapes
import helpers
import pbs_jack_model as model
from popgenomicstools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "popgenomicstools_amd", "csrc")
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")


def tenth(x, y):
    """a tenth of the project's jackknife tolerance (helpers.REL / helpers.ABS)"""
    return abs(x - y) <= 0.1 * (helpers.REL * abs(y) + helpers.ABS)


# ---- the models ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [5, 65, 129, 4097, 65537])
def test_the_float_model_stays_within_a_tenth_of_the_tolerance_of_the_60_digit_model(n_win):
    n_trios = 2 if n_win != 4097 else 1
    rows = model.synth_rows(n_win, n_trios)
    used = rows["n"] > 0
    # what keeps the estimator tame: every FST in (0, 0.5), and so is every FST of the sums with a block left out
    for a, b in zip(model.NUM, model.DEN):
        assert np.all(rows[a][used] > 0) and np.all(rows[a][used] < 12.5) and np.all(rows[b][used] >= 25) and np.all(rows[b][used] < 50)
    assert n_win < 65 or ((~used).any() and all(np.isnan(rows[f][~used]).all() for f in model.PBS + model.SUMS))
    ref, flt = model.ref_reference(n_win, n_trios), model.float_reference(n_win, n_trios)
    worst = 0.0
    for t in range(n_trios):
        for c in range(model.ITEMS):
            e, f = ref[t][c], flt[t][c]
            assert e["n_blocks"] == f["n_blocks"] == int(used[t].sum()) >= 2 and e["n_sites"] == f["n_sites"] == int(rows["n"][t].sum())
            for k in ("stat", "stat_jack", "se"):
                worst = max(worst, abs(f[k] - e[k]) / (helpers.REL * abs(e[k]) + helpers.ABS))
                assert tenth(f[k], e[k]), (n_win, t, c, k, f[k], e[k])
            assert e["se"] > 0 and e["stat"] > -1.0
    print(f"n_win={n_win}: worst |float - ref| / tolerance = {worst:.4f}")


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_both_models_give_the_hand_cases(name, blocks, want):
    sums = np.array([s for s, _ in blocks], dtype=np.float64).reshape(-1, 6)
    m = np.array([w for _, w in blocks], dtype=np.uint64)
    got = model.jack_float(sums, m)
    ref = model.jack_ref(sums, m)
    rows = model.hand_rows(blocks)
    by_rows = model.jack_rows(rows[0])
    for c in range(model.ITEMS):
        model.check_hand_item(name, c, got[c], blocks, want, helpers.close)
        model.check_hand_item(name, c, by_rows[c], blocks, want, helpers.close)
        model.check_hand_item(name, c, ref[c], blocks, want, helpers.close, rounded_late=True)


def test_the_hand_cases_cover_what_they_must():
    names = [c[0] for c in model.HAND_CASES]
    assert names == ["no block", "unused blocks only", "all numerators zero", "one block", "two identical blocks around an unused one"]
    assert sorted(len([b for b in c[1] if b[1] > 0]) for c in model.HAND_CASES) == [0, 0, 1, 2, 3]
    zero = dict(zip(names, model.HAND_CASES))["all numerators zero"]
    assert all(s[:3] == (0, 0, 0) for s, m in zero[1] if m > 0) and zero[2]["stat"] == 0.0 and zero[2]["se"] == 0.0
    # E of one block's sums: the three pbs are those of tests/pbs_pops_model.py, and PBSn1 is pbs / (1 + sum)
    import pbs_pops_model
    e = model.hand_stat(dict(zip(names, model.HAND_CASES))["one block"][1])
    pbs, _ = pbs_pops_model.finish([1.0, 2.0, 3.0], [8.0, 8.0, 8.0])
    assert [model.bits(x) for x in e[:3]] == [model.bits(x) for x in pbs]
    assert np.array_equal(e[3:], e[:3] / (1.0 + ((e[0] + e[1]) + e[2]))) and np.all(e[3:] != e[:3])


def test_the_recorded_reference_is_the_evaluation_it_claims():
    """one deletion of the recorded table re-derived: stat of the record is E of the used blocks' sums at 60 digits"""
    import decimal
    rows = model.synth_rows(model.GOLDEN_N_WIN, 1)[0]
    used = rows["n"] > 0
    rec = model.ref_reference(model.GOLDEN_N_WIN, 1)[0]
    with decimal.localcontext() as ctx:
        ctx.prec = model.DIGITS
        S = [sum((decimal.Decimal(float(x)) for x in rows[f][used]), decimal.Decimal(0)) for f in model.SUMS]
        e = model._estimator_ref(S)
    for c in range(model.ITEMS):
        assert rec[c]["stat"] == float(e[c]) and rec[c]["n_blocks"] == int(used.sum()) and rec[c]["n_sites"] == int(rows["n"][used].sum())
    assert os.path.getsize(model.GOLDEN) < 8192


# ---- header, binding, workspace --------------------------------------------------------------------------------------------------
def test_header_binding_dtype_and_work_bytes():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_pbs_jackknife_work_bytes", "pgt_pbs_jackknife_dev", "pgt_pbs_jackknife")
    lib = _lib.load()
    for name in names:
        assert name + "(" in text and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "} pgt_pbs_jack;" in text and "#define PGT_ABI_VERSION 6" in text
    assert "Still 6: pgt_pbs_jack, pgt_pbs_jackknife_work_bytes / pgt_pbs_jackknife_dev / pgt_pbs_jackknife added" in text
    for line in ("pbsn1_x = pbs_x / (1.0 + s)", "s       = (pbs_i + pbs_j) + pbs_k", "theta_-j(c) = E(S_total - s_j)[c]", "u = 6 t + c",
                 "n_trios must be 1 ... 20", "rows is not 8-byte aligned", "makes all six items of its trio NaN"):
        assert line in text, line
    assert "Not computed: PBSn1" not in text and "a block jackknife, user-chosen" not in text
    d = _lib.PBS_JACK_DTYPE
    assert d.names == ("stat", "stat_jack", "se", "z", "n_sites", "n_blocks", "pad_") and d.itemsize == 48
    assert [d.fields[k][1] for k in d.names] == [_lib.F4_JACK_DTYPE.fields[k][1] for k in _lib.F4_JACK_DTYPE.names] == [0, 8, 16, 24, 32, 40, 44]
    internal = open(os.path.join(CSRC, "pgt_internal.h")).read()
    assert re.search(r"constexpr int kJackPbsItems = 6;", internal) and re.search(r"constexpr int kJackPbsSums = 6;", internal)
    assert re.search(r"constexpr int kJackTotalWords = 5;", internal)
    assert model.WORDS_PER_PARTIAL == 20 and model.ITEMS == 6 and model.MAX_TRIOS == shapes.MAX_TRIOS == 20
    import popgenomicstools_amd as pgt
    for n_win in (0, 1, 64, 65, 4096, 4097, 65536, 65537, 10**6):
        for t in (1, 4, 20):
            got = lib.pgt_pbs_jackknife_work_bytes(t, n_win)
            assert got == model.work_bytes(t, n_win) == pgt.Context.pbs_jackknife_work_bytes(t, n_win) and got % 256 == 0
            assert got >= lib.pgt_f4ratio_jackknife_work_bytes(min(t, 10), n_win) and lib.pgt_dstat_jackknife_work_bytes(t, n_win) == shapes.work_bytes(t, n_win)
    assert model.work_bytes(2, 65537) == -(-(2 * 1024 * 8 * 20) // 256) * 256
    for t in (0, 21, 40):
        assert lib.pgt_pbs_jackknife_work_bytes(t, 100) == 0 == model.work_bytes(t, 100)
    assert {"pbs_window_pops", "pbsn1_of", "pbs_item_order"} <= set(pgt.__all__)
    assert pgt.pbs_item_order(0, 2, 5) == [("pbs", 0), ("pbs", 2), ("pbs", 5), ("pbsn1", 0), ("pbsn1", 2), ("pbsn1", 5)]
    for method in ("pbs_jackknife", "pbs_jackknife_dev", "pbs_jackknife_work_bytes"):
        assert callable(getattr(pgt.Context, method))


def test_the_phases_are_one_copy_with_a_fourth_estimator():
    src = open(os.path.join(CSRC, "pgt_dstat_jack_kernels.hip")).read()
    for kernel in ("jack_totals_kernel", "jack_drop_kernel", "jack_var_kernel", "jack_close_kernel"):
        assert len(re.findall(r"__global__ __launch_bounds__\(256\) void " + kernel + r"\(", src)) == 1, kernel
    assert "struct Pbs {" in src and "struct RowsPbs {" in src and "struct Rows48 {" in src and "atomic" not in src.replace("No atomics", "")
    from popgenomicstools_amd import build
    assert "pgt_dstat_jack_kernels.hip" in build.LIB_SOURCES and len(build.LIB_SOURCES) == 15


def test_pbsn1_of_is_the_formula_in_its_order():
    import popgenomicstools_amd as pgt
    rng = np.random.default_rng(2016)
    rows = np.zeros((3, 7), dtype=_lib.PBS_ROW_DTYPE)
    for f in model.PBS:
        rows[f] = rng.normal(0.1, 0.2, rows.shape)
    rows["pbs_i"][0, 0], rows["pbs_j"][0, 1] = np.inf, np.nan
    rows["pbs_i"][1, 0], rows["pbs_j"][1, 0], rows["pbs_k"][1, 0] = -0.5, -0.25, -0.25  # 1 + s = 0
    got = pgt.pbsn1_of(rows)
    assert got.shape == (3, 7, 3) and got.dtype == np.float64
    with np.errstate(all="ignore"):
        one_s = 1.0 + ((rows["pbs_i"] + rows["pbs_j"]) + rows["pbs_k"])
        for c, f in enumerate(model.PBS):
            want = rows[f] / one_s
            assert np.array_equal(got[..., c], want, equal_nan=True)
    assert np.isnan(got[0, 0, 0]) and got[0, 0, 1] == 0.0 and np.isnan(got[0, 1]).all() and np.isinf(got[1, 0]).all()
    tot = np.zeros(2, dtype=_lib.PBS_TOTAL_DTYPE)
    tot["pbs_i"], tot["pbs_j"], tot["pbs_k"] = 0.5, 0.25, 0.25
    assert np.array_equal(pgt.pbsn1_of(tot), [[0.25, 0.125, 0.125]] * 2)
    assert np.array_equal(pgt.pbsn1_of(np.zeros(4, dtype=_lib.PBS_ROW_DTYPE)), np.zeros((4, 3)))


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for W, S in ((0, 0), (4, 2), (4, 3)):
        with pytest.raises(_lib.PgtError, match="pbs_window_pops: the block jackknife needs disjoint windows as its blocks") as e:
            pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, W, S, 1, 1, jackknife=True)
        assert e.value.code == _lib.PGT_EARG and f"winsize {W} must be positive and stepsize {S} at least the winsize" in str(e.value)
    with pytest.raises(_lib.PgtError, match='pbs_window_pops: estimator must be "wc" or "hudson"'):
        pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 1, 1, estimator="reynolds", jackknife=True)
    for k in (2, 7):
        with pytest.raises(_lib.PgtError, match="pbs_window_pops: 3 ... 6 populations"):
            pgt.pbs_window_pops(ids, pos, [z] * k, [c] * k, 2, 2, 1, 1, jackknife=True)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.pbs_window_pops(ids, pos, [z] * 3, [c] * 3, 2, 2, 0, 1, jackknife=True)
    with pytest.raises(_lib.PgtError, match="column lengths differ"):
        pgt.pbs_window_pops(ids, pos, [z, z, np.zeros(3)], [c] * 3, 2, 2, 1, 1, jackknife=True)


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "pbsWindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_describes_the_two_options(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("-blockjack", "-pbsn1", "PBSn1", "block jackknife", "PREFIX.jackknife", "PREFIX.pbsn1.global", "PREFIX.pop<i>_pop<j>_pop<k>.pbsn1",
                 "PBS_x / (1 + PBS_i + PBS_j + PBS_k)", "Malaspinas et al. 2016", "The block jackknife is -blockjack, not -jackknife",
                 "-stepsize not below -winsize", "(1) pbs or pbsn1", "Not computed: FST truncated at 0, user-chosen trio lists"):
        assert word in r.stdout, word
    assert "Not computed: PBSn1" not in r.stdout and "a block jackknife of PBS, user" not in r.stdout


def test_the_option_refusals_come_before_any_file_is_opened(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(3)]
    out = str(tmp_path / "o")
    sites = ["-fixedsite", "1"]
    cases = [
        (sites + ["-winsize", "4", "-stepsize", "4", "-blockjack", "2"], "-blockjack must be 0 or 1 (given: 2)"),
        (sites + ["-winsize", "4", "-stepsize", "4", "-blockjack", "yes"], "-blockjack must be 0 or 1 (given: yes)"),
        (sites + ["-winsize", "4", "-stepsize", "4", "-pbsn1", "2"], "-pbsn1 must be 0 or 1 (given: 2)"),
        (sites + ["-winsize", "4", "-stepsize", "4", "-pbsn1", "on"], "-pbsn1 must be 0 or 1 (given: on)"),
        (sites + ["-winsize", "0", "-blockjack", "1"], "-blockjack 1 needs windows as its blocks: -winsize must be > 0"),
        (sites + ["-blockjack", "1"], "-blockjack 1 needs windows as its blocks: -winsize must be > 0"),
        (sites + ["-winsize", "4", "-stepsize", "2", "-blockjack", "1"], "-blockjack 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        # the last value of -winsize / -stepsize counts, wherever -blockjack stands
        (sites + ["-blockjack", "1", "-winsize", "4", "-stepsize", "3"], "-blockjack 1 needs windows that do not overlap: -stepsize (3) must not be below -winsize (4)"),
        (sites + ["-winsize", "4", "-stepsize", "4", "-jackknife", "1"], "Unknown command"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + ["-out", out] + missing)
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
        assert "-jackknife 1 needs" not in r.stderr
    # accepted option values get as far as the files: both options at 0, at 1, and -pbsn1 1 without windows
    for opts in (["-blockjack", "0", "-pbsn1", "0"], ["-blockjack", "1", "-pbsn1", "1"], []):
        r = run([tool] + sites + ["-winsize", "4", "-stepsize", "4"] + opts + ["-out", out] + missing)
        assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr, (opts, r.stderr)
    r = run([tool] + sites + ["-winsize", "0", "-pbsn1", "1", "-blockjack", "0", "-out", out] + missing)
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []


def test_the_other_tools_keep_their_jackknife_messages(tool, tmp_path):
    """JackknifeOption takes the option's name; with its default the texts of tests/golden/pops_cli_texts.json stand"""
    f3 = os.path.join(BIN, "f3WindowPops")
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(3)]
    r = run([f3, "-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-jackknife", "1", "-out", str(tmp_path / "o")] + missing)
    assert r.returncode == 255 and "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)" in r.stderr
    r = run([f3, "-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-jackknife", "2", "-out", str(tmp_path / "o")] + missing)
    assert r.returncode == 255 and "-jackknife must be 0 or 1 (given: 2)" in r.stderr
