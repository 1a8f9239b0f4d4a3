"""CPU: the all-pairs FST front end over per-population (freq, nInd) columns — the exact-rational fixture, the NumPy model
the GPU tests compare against, the workspace size, and bin/fstWindowPops' refusals that come before the device is opened."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)


def fixture_columns():
    k = helpers.load_golden("wcfst_nind_exact.json")
    pos = np.array(k["pos"], dtype=np.uint32)
    freqs = [np.array(f, dtype=np.float64) for f in k["freq"]]
    ninds = [np.array(c, dtype=np.int32) for c in k["nind"]]
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    return k, pos, freqs, ninds, win


def test_the_fixture_is_what_its_generator_writes(tmp_path):
    """tests/golden/wcfst_nind_exact.json is reproducible: the generator gives the committed inputs and sums again."""
    import make_wcfst_nind_exact as gen
    k, pos, freqs, ninds, win = fixture_columns()
    gpos, gf, gn = gen.inputs()
    assert np.array_equal(gpos, pos) and all(np.array_equal(a, b) for a, b in zip(gf + gn, freqs + ninds))
    assert [list(w) for w in gen.windows()] == k["windows"]
    assert len(freqs) == 3 and pos.size <= 200 and [c["minind"] for c in k["cases"]] == [1, 5]
    for case in k["cases"]:
        for pr in case["pairs"]:
            i, j = pr["pair"]
            sites = gen.exact_sites(freqs, ninds, i, j, case["minind"])
            for w, (lo, hi) in enumerate(k["windows"]):
                a, b, n = gen.exact_window(sites, lo, hi)
                assert (float(a), float(b), n) == (pr["asum"][w], pr["bsum"][w], pr["n"][w])
    # pair (0, 2): frequencies about 1e-3 apart, a negative at every counted site
    one_site = [w for w, (lo, hi) in enumerate(k["windows"]) if hi == lo + 1]
    p02 = k["cases"][0]["pairs"][1]
    assert p02["pair"] == [0, 2] and all(p02["asum"][w] < 0 for w in one_site if p02["n"][w])


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site components in the literal form of the R lines, summed: within 1e-12 relative of the exact rationals
    (one-site windows included), counts exact."""
    import fst_pops_model
    k, pos, freqs, ninds, win = fixture_columns()
    for case in k["cases"]:
        rows, tot = fst_pops_model.model(pos, freqs, ninds, case["minind"], win)
        for p, pr in enumerate(case["pairs"]):
            assert np.array_equal(rows[p]["n"], np.array(pr["n"], dtype=np.uint32))
            for fld in ("asum", "bsum"):
                want = np.array(pr[fld])
                assert np.all(np.abs(rows[p][fld] - want) <= 1e-12 * np.abs(want)), (case["minind"], pr["pair"], fld)
            whole = k["windows"].index([0, int(pos.size)])
            assert int(tot[p]["neff"]) == pr["n"][whole] and int(tot[p]["nskip"]) == pos.size - pr["n"][whole]
            assert abs(float(tot[p]["asum"]) - pr["asum"][whole]) <= 1e-12 * abs(pr["asum"][whole])
            assert abs(float(tot[p]["bsum"]) - pr["bsum"][whole]) <= 1e-12 * abs(pr["bsum"][whole])


def test_the_identity_form_agrees_per_site():
    """a = (f1-f2)^2 - b npool/(4 n1 n2) (pgt_af_kernels.hip:12-15), the form the kernel evaluates, against the literal lines"""
    import fst_pops_model
    rng = np.random.default_rng(5)
    n = 50_000
    f1, f2 = np.round(rng.uniform(0, 1, n), 6), np.round(rng.uniform(0, 1, n), 6)
    n1, n2 = rng.integers(1, 21, n).astype(np.float64), rng.integers(1, 21, n).astype(np.float64)
    a, ab = fst_pops_model.site_components(f1, f2, n1, n2)
    b = (n1 * 2 * f1 * (1 - f1) + n2 * 2 * f2 * (1 - f2)) / (n1 + n2 - 1)
    a2 = (f1 - f2) ** 2 - b * (n1 + n2) / (4 * n1 * n2)
    assert np.max(np.abs(a2 - a)) < 1e-15 and np.max(np.abs((a2 + b) - ab)) < 1e-15


def test_tree_bytes():
    lib = _lib.load()
    assert lib.pgt_fst_pops_tree_bytes(1, 1000) == 0 and lib.pgt_fst_pops_tree_bytes(9, 1000) == 0 and lib.pgt_fst_pops_tree_bytes(0, 1000) == 0
    for k in range(2, 9):
        prev = 0
        for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8, 10**9):
            tb = lib.pgt_fst_pops_tree_bytes(k, n)
            assert tb >= prev and tb > 0 and tb % 256 == 0
            prev = tb
        assert lib.pgt_fst_pops_tree_bytes(k, 10**9) < 0.02 * 12 * k * 10**9 + (1 << 20)


def test_header_declares_the_entry_points_and_the_total():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    for name in ("pgt_fst_pops_tree_bytes", "pgt_fst_pops_reduce_dev", "pgt_fst_pops_reduce", "pgt_fst_total"):
        assert name in text
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_fst_total" in text
    lib = _lib.load()
    for name in ("pgt_fst_pops_tree_bytes", "pgt_fst_pops_reduce_dev", "pgt_fst_pops_reduce"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.FST_TOTAL_DTYPE.itemsize == 32 and _lib.FST_TOTAL_DTYPE.names == ("asum", "bsum", "neff", "nskip")


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.fst_window_pops(ids, pos, [z, z], [c, c], 2, 1, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.fst_window_pops(ids, pos, [z, z], [c, c], 2, 1, 1, 0)
    with pytest.raises(_lib.PgtError, match="2 ... 8 populations"):
        pgt.fst_window_pops(ids, pos, [z], [c], 2, 1, 1, 1)


# ---- bin/fstWindowPops: the command line ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "fstWindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_and_argument_refusals(tool, tmp_path):
    r = run([tool])
    assert r.returncode == 0 and "-out" in r.stdout and "-minind" in r.stdout and ".fst" in r.stdout
    assert "One GPU" in r.stdout and "No passes mode" in r.stdout and "PGT_DXY_SYNC" in r.stdout
    m = [str(tmp_path / f"p{k}.mafs") for k in range(9)]
    for p in m:
        open(p, "w").write("chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\nc1\t1\tA\tC\tA\t0.500000\t5\n")
    base = [tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", str(tmp_path / "o")]
    cases = [
        (base + m[:1], "fstWindowPops: between 2 and 8 MAF files are needed (1 given)"),
        (base + m, "fstWindowPops: between 2 and 8 MAF files are needed (9 given)"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1"] + m[:2], "Must supply -out PREFIX"),
        ([tool, "-minind", "0", "-out", "o"] + m[:2], "-minind must be at least 1"),
        ([tool, "-winsize", "2", "-stepsize", "1", "-out", "o"] + m[:2], "Must supply size file unless -fixedsite 1"),
        ([tool, "-bogus", "1", "-out", "o"] + m[:2], "Unknown command: -bogus"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "3", "-out", "o"] + m[:2], "-stepsize must not exceed -winsize"),
    ]
    for cmd, text in cases:
        r = run(cmd)
        assert r.returncode == 255 and text in r.stderr and r.stdout == "", (cmd, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "o.global"))
