"""CPU: the ABBA-BABA front end (pgt_dstat_pops_reduce*, dstatWindowPops) — the exact-rational fixture, the NumPy model the GPU
tests compare against, the allele symmetry of the definition, the workspace size, the declarations, and the refusals of the
Python mirror and of the command line that come before the device is opened."""
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
    k = helpers.load_golden("dstat_exact.json")
    pos = np.array(k["pos"], dtype=np.uint32)
    freqs = [np.array(f, dtype=np.float64) for f in k["freq"]]
    ninds = [np.array(c, dtype=np.int32) for c in k["nind"]]
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    return k, pos, freqs, ninds, win


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/dstat_exact.json is reproducible: the generator gives the committed inputs and sums again."""
    import make_dstat_exact as gen
    k, pos, freqs, ninds, win = fixture_columns()
    gpos, gf, gn = gen.inputs()
    assert np.array_equal(gpos, pos) and all(np.array_equal(a, b) for a, b in zip(gf + gn, freqs + ninds))
    assert [list(w) for w in gen.windows()] == k["windows"]
    assert len(freqs) == 5 and pos.size <= 200 and [c["minind"] for c in k["cases"]] == [1, 5]
    assert all(c.min() == 0 and c.max() == 20 and np.any(c == 1) for c in ninds)
    assert all(np.array_equal(f, np.round(f, 6)) for f in freqs)
    assert [0, int(pos.size)] in k["windows"] and sum(hi == lo + 1 for lo, hi in k["windows"]) >= pos.size
    assert abs(float(np.max(np.abs(freqs[4] - freqs[0]))) - 1e-3) < 3e-4  # the outgroup about 1e-3 from population 0
    from popgenomicstools_amd.window_scan import trio_order
    for case in k["cases"]:
        assert [tuple(tr["trio"]) for tr in case["trios"]] == trio_order(5) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
        for tr in case["trios"]:
            sites = gen.exact_sites(freqs, ninds, *tr["trio"], case["minind"])
            for w, (lo, hi) in enumerate(k["windows"]):
                b, a, c, n = gen.exact_window(sites, lo, hi)
                assert (float(b), float(a), float(c), n) == (tr["bbaa"][w], tr["abba"][w], tr["baba"][w], tr["n"][w])
    # the fixture holds data only
    assert set(k) == {"source", "pos", "freq", "nind", "windows", "cases"}


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site lines of the definition, summed: within 1e-12 |y| + 1e-15 (hi - lo) of the exact rationals, counts
    exact.  The per-site floor: a pattern is a sum of two products of four factors <= 1, each product chain and the sum rounded
    at most four times by 2^-53 of a value <= 1 (the subtractions 1 - p are exact on 6-decimal inputs to within half an ulp
    and enter the same bound): below 1e-15 per site; measured on these 200 sites, 1.1e-16."""
    import dstat_pops_model
    k, pos, freqs, ninds, win = fixture_columns()
    length = (win["hi"] - win["lo"]).astype(np.float64)
    worst = 0.0
    for case in k["cases"]:
        rows, tot = dstat_pops_model.model(pos, freqs, ninds, case["minind"], win)
        for t, tr in enumerate(case["trios"]):
            assert np.array_equal(rows[t]["n"], np.array(tr["n"], dtype=np.uint32))
            whole = k["windows"].index([0, int(pos.size)])
            assert int(tot[t]["neff"]) == tr["n"][whole] and int(tot[t]["nskip"]) == pos.size - tr["n"][whole]
            for fld in ("bbaa", "abba", "baba"):
                want = np.array(tr[fld])
                err = np.abs(rows[t][fld] - want)
                worst = max(worst, float(err[length == 1].max()))
                assert np.all(err <= 1e-12 * np.abs(want) + 1e-15 * length), (case["minind"], tr["trio"], fld)
                assert abs(float(tot[t][fld]) - tr[fld][whole]) <= 1e-12 * abs(tr[fld][whole]) + 1e-15 * pos.size
            assert np.array_equal(rows[t]["d"], dstat_pops_model.d_of(rows[t]["abba"], rows[t]["baba"]))
    print(f"largest one-site error of the model against the exact value: {worst:.3e}")


def test_the_patterns_do_not_depend_on_the_reported_allele():
    """p -> 1 - p in all four populations swaps the two terms of every line: the three patterns stay, within 1e-15 per site
    (the flipped frequency 1 - p is itself rounded once); exactly so in rationals."""
    import dstat_pops_model
    import make_dstat_exact as gen
    from fractions import Fraction
    k, pos, freqs, ninds, win = fixture_columns()
    worst = 0.0
    for i, j, kk in gen.TRIOS:
        cols = [freqs[x] for x in (i, j, kk, 4)]
        a = dstat_pops_model.site_components(*cols)
        b = dstat_pops_model.site_components(*[1.0 - c for c in cols])
        worst = max(worst, max(float(np.max(np.abs(x - y))) for x, y in zip(a, b)))
    print(f"largest per-site change under the allele flip: {worst:.3e}")
    assert worst <= 1e-15
    p = [Fraction(float(freqs[x][17])) for x in (0, 1, 2, 4)]
    assert gen.dstat_site(*p) == gen.dstat_site(*[1 - x for x in p])


def test_tree_bytes_only_for_four_to_seven_populations():
    lib = _lib.load()
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        for k in range(0, 12):
            b = lib.pgt_dstat_pops_tree_bytes(k, n)
            assert (b > 0) == (4 <= k <= 7), (k, n, b)
        sizes = [lib.pgt_dstat_pops_tree_bytes(k, n) for k in (4, 5, 6, 7)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    import popgenomicstools_amd as pgt
    assert pgt.Context.dstat_pops_tree_bytes(5, 12345) == lib.pgt_dstat_pops_tree_bytes(5, 12345)
    assert pgt.Context.dstat_pops_tree_bytes(8, 12345) == 0 and pgt.Context.dstat_pops_tree_bytes(3, 12345) == 0


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_dstat_pops_tree_bytes", "pgt_dstat_pops_reduce_dev", "pgt_dstat_pops_reduce")
    for name in names:
        assert name + "(" in text
    assert "} pgt_dstat_row;" in text and "} pgt_dstat_total;" in text
    assert "#define PGT_ABI_VERSION 6" in text
    assert ("Still 6: pgt_dstat_row, pgt_dstat_total, pgt_dstat_pops_tree_bytes / pgt_dstat_pops_reduce_dev / pgt_dstat_pops_reduce "
            "added (additive as well).") in text
    for line in ("bbaa = (p_i*p_j)*(q_k*q_o) + (q_i*q_j)*(p_k*p_o)", "abba = (q_i*p_j)*(p_k*q_o) + (p_i*q_j)*(q_k*p_o)",
                 "baba = (p_i*q_j)*(p_k*q_o) + (q_i*p_j)*(q_k*p_o)", "d = (abba + baba) != 0 ? (abba - baba) / (abba + baba) : 0",
                 "(bbaa - baba) / (bbaa + baba)", "(bbaa - abba) / (bbaa + abba)"):
        assert line in text, line
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.DSTAT_ROW_DTYPE.names == ("start", "end", "mid", "n", "d", "bbaa", "abba", "baba") and _lib.DSTAT_ROW_DTYPE.itemsize == 48
    assert _lib.DSTAT_TOTAL_DTYPE.names == ("bbaa", "abba", "baba", "neff", "nskip") and _lib.DSTAT_TOTAL_DTYPE.itemsize == 40


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    assert pgt.trio_order(4) == [(0, 1, 2)] and len(pgt.trio_order(7)) == 20 and pgt.trio_order(5)[1] == (0, 1, 3)
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (3, 8):
        with pytest.raises(_lib.PgtError, match="4 ... 7 populations, one frequency and one count column each") as e:
            pgt.dstat_window_pops(ids, pos, [z] * k, [c] * k, 2, 1, 1, 1)
        assert e.value.code == _lib.PGT_EARG
    with pytest.raises(_lib.PgtError, match="4 ... 7 populations"):
        pgt.dstat_window_pops(ids, pos, [z] * 4, [c] * 3, 2, 1, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.dstat_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 1, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.dstat_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 1, 1, 0)
    with pytest.raises(_lib.PgtError, match="2 ... 8 populations"):  # the other statistics keep their message
        pgt.fst_window_pops(ids, pos, [z], [c], 2, 1, 1, 1)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bin_dir():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return BIN


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_and_the_refusals_of_the_command_line(bin_dir, tmp_path):
    tool = os.path.join(bin_dir, "dstatWindowPops")
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("-out", "outgroup", "4 <= K <= 7", "SAME allele", "(BBAA - BABA)/(BBAA + BABA)", "(BBAA - ABBA)/(BBAA + ABBA)", "jackknife", "Limits:"):
        assert word in r.stdout, word
    m = [str(tmp_path / f"p{k}.mafs") for k in range(8)]
    for p in m:
        open(p, "w").write("chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\nc1\t1\tA\tC\tA\t0.500000\t5\n")
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", out]
    for k in (3, 8):
        r = run([tool] + head + m[:k])
        assert r.returncode == 255 and r.stdout == "" and f"between 4 and 7 MAF files are needed ({k} given)" in r.stderr, (k, r.stderr)
    r = run([tool, "-estimator", "hudson"] + head + m[:4])
    assert r.returncode == 255 and r.stdout == "" and "Unknown command: -estimator" in r.stderr, r.stderr
    r = run([tool, "-winsize", "2", "-stepsize", "1", "-fixedsite", "1"] + m[:4])
    assert r.returncode == 255 and r.stdout == "" and "-out" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
    # the other tools keep their limit and its message
    r = run([os.path.join(bin_dir, "piWindowPops")] + head + m[:8] + [m[0]])
    assert r.returncode == 255 and "between 1 and 8 MAF files are needed (9 given)" in r.stderr
