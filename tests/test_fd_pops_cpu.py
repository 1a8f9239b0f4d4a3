"""CPU: the f_d / f_dM front end (pgt_fd_pops_reduce*, `dstatWindowPops -fd 1`) — the exact-rational fixture, the NumPy model
the GPU tests compare against, the allele symmetry of the definition, its indifference to the choice at ties, the workspace
size, the declarations, the constant the build-grid test depends on, and the refusals of the Python mirror and of the command
line that come before the device is opened."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import helpers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)
SUMS = ("num", "fd_den", "fdm_den")


def fixture_columns():
    k = helpers.load_golden("fd_exact.json")
    pos = np.array(k["pos"], dtype=np.uint32)
    freqs = [np.array(f, dtype=np.float64) for f in k["freq"]]
    ninds = [np.array(c, dtype=np.int32) for c in k["nind"]]
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    return k, pos, freqs, ninds, win


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/fd_exact.json is reproducible, and its inputs hold what the definition's selects can go wrong on."""
    import make_fd_exact as gen
    from popgenomicstools_amd.window_scan import trio_order
    k, pos, freqs, ninds, win = fixture_columns()
    gpos, gf, gn = gen.inputs()
    assert np.array_equal(gpos, pos) and all(np.array_equal(a, b) for a, b in zip(gf + gn, freqs + ninds))
    assert [list(w) for w in gen.windows()] == k["windows"]
    assert len(freqs) == 5 and pos.size <= 200 and [c["minind"] for c in k["cases"]] == [1, 5]
    assert all(np.array_equal(f, np.round(f, 6)) for f in freqs)
    assert [0, int(pos.size)] in k["windows"] and sum(hi == lo + 1 for lo, hi in k["windows"]) >= pos.size
    o = 4
    for case in k["cases"]:
        assert [tuple(tr["trio"]) for tr in case["trios"]] == trio_order(5) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
        for tr in case["trios"]:
            i, j, kk = tr["trio"]
            sites = gen.exact_sites(freqs, ninds, i, j, kk, case["minind"])
            for w, (lo, hi) in enumerate(k["windows"]):
                a, b, c, n = gen.exact_window(sites, lo, hi)
                assert (float(a), float(b), float(c), n) == (tr["num"][w], tr["fd_den"][w], tr["fdm_den"][w], tr["n"][w])
            ok = np.array([s is not None for s in sites])
            pi, pj, pk, po = freqs[i], freqs[j], freqs[kk], freqs[o]
            # ties of all three kinds, 0 and 1 in every role, and both branches of every select: at COUNTED sites of every trio
            for what, m in (("p_i == p_j", pi == pj), ("p_j == p_k", pj == pk), ("p_i == p_k", pi == pk),
                            ("p_j > p_k", pj > pk), ("p_j < p_k", pj < pk), ("p_i > p_k", pi > pk), ("p_i < p_k", pi < pk),
                            ("p_j > p_i", pj > pi), ("p_j < p_i", pj < pi)):
                assert np.any(m & ok), (case["minind"], tr["trio"], what)
            for role, p in (("i", pi), ("j", pj), ("k", pk), ("o", po)):
                assert np.any((p == 0) & ok) and np.any((p == 1) & ok), (case["minind"], tr["trio"], role)
            assert np.any((po > 0) & (po < 1) & ok)
    assert set(k) == {"source", "pos", "freq", "nind", "windows", "cases"}  # the fixture holds data only
    assert all(set(tr) == {"trio", "n"} | set(SUMS) for case in k["cases"] for tr in case["trios"])


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site lines of the definition, summed: within 1e-12 A + 1e-15 (hi - lo) of the exact rationals, A the
    window's Σ|site term| (the terms have both signs), counts exact.  The per-site floor: a term is a difference or sum of
    four products of four factors <= 1, each chain rounded at most four times by 2^-53 of a value <= 1, then at most two
    more additions of values <= 2: below 1e-15 per site."""
    import fd_pops_model
    k, pos, freqs, ninds, win = fixture_columns()
    length = (win["hi"] - win["lo"]).astype(np.float64)
    whole = k["windows"].index([0, int(pos.size)])
    worst = 0.0
    for case in k["cases"]:
        rows, tot, A, A_tot = fd_pops_model.model(pos, freqs, ninds, case["minind"], win)
        for t, tr in enumerate(case["trios"]):
            assert np.array_equal(rows[t]["n"], np.array(tr["n"], dtype=np.uint32))
            assert int(tot[t]["neff"]) == tr["n"][whole] and int(tot[t]["nskip"]) == pos.size - tr["n"][whole]
            for fld in SUMS:
                want = np.array(tr[fld])
                err = np.abs(rows[t][fld] - want)
                worst = max(worst, float(err[length == 1].max()))
                assert np.all(err <= 1e-12 * A[fld][t] + 1e-15 * length), (case["minind"], tr["trio"], fld)
                assert abs(float(tot[t][fld]) - tr[fld][whole]) <= 1e-12 * A_tot[fld][t] + 1e-15 * pos.size
                assert A_tot[fld][t] == A[fld][t][whole]
            assert np.array_equal(rows[t]["fd"], fd_pops_model.ratio(rows[t]["num"], rows[t]["fd_den"]))
            assert np.array_equal(rows[t]["fdm"], fd_pops_model.ratio(rows[t]["num"], rows[t]["fdm_den"]))
    print(f"largest one-site error of the model against the exact value: {worst:.3e}")


def test_the_terms_do_not_depend_on_the_reported_allele():
    """p -> 1 - p in all four populations swaps the two halves of every line (and the larger with the smaller): the three
    per-site values stay, within 1e-15 per site (the flipped frequency 1 - p is itself rounded once); exactly so in rationals."""
    import fd_pops_model
    import make_fd_exact as gen
    k, pos, freqs, ninds, win = fixture_columns()
    worst = 0.0
    for i, j, kk in gen.TRIOS:
        cols = [freqs[x] for x in (i, j, kk, 4)]
        a = fd_pops_model.site_terms(*cols)
        b = fd_pops_model.site_terms(*[1.0 - c for c in cols])
        worst = max(worst, max(float(np.max(np.abs(x - y))) for x, y in zip(a, b)))
        for s in range(pos.size):
            p = [Fraction(float(c[s])) for c in cols]
            assert gen.fd_site(*p) == gen.fd_site(*[1 - x for x in p]), ((i, j, kk), s)
    print(f"largest per-site change under the allele flip: {worst:.3e}")
    assert worst <= 1e-15


def test_either_choice_at_a_tie_gives_the_same_bits():
    """Equal p give equal q and the products commute: on the fixture's tie sites H, L, G and S may be chosen either way."""
    import fd_pops_model
    import make_fd_exact as gen
    k, pos, freqs, ninds, win = fixture_columns()
    ties = 0
    for i, j, kk in gen.TRIOS:
        pi, pj, pk, po = (freqs[x] for x in (i, j, kk, 4))
        a = fd_pops_model.site_terms(pi, pj, pk, po)
        other = {"H_is_j": pj > pk, "L_is_j": pj < pk, "G_is_i": pi > pk, "S_is_i": pi < pk}  # the other branch at every tie
        b = fd_pops_model.site_terms(pi, pj, pk, po, choose=other)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (i, j, kk)
        assert np.any(pj == pk) and np.any(pi == pk) and np.any(pi == pj)
        ties += int(np.count_nonzero(pj == pk)) + int(np.count_nonzero(pi == pk))
    assert ties >= 8 * gen.TIE_RUN


def test_tree_bytes_only_for_four_to_seven_populations():
    lib = _lib.load()
    for n in (0, 1, 511, 512, 513, 8192, 8193, 10**6, 10**8):
        for k in range(0, 12):
            b = lib.pgt_fd_pops_tree_bytes(k, n)
            assert (b > 0) == (4 <= k <= 7), (k, n, b)
            assert b == lib.pgt_dstat_pops_tree_bytes(k, n)  # the tool reuses the D tree's buffer
        sizes = [lib.pgt_fd_pops_tree_bytes(k, n) for k in (4, 5, 6, 7)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    import popgenomicstools_amd as pgt
    assert pgt.Context.fd_pops_tree_bytes(5, 12345) == lib.pgt_fd_pops_tree_bytes(5, 12345)
    assert pgt.Context.fd_pops_tree_bytes(8, 12345) == 0 and pgt.Context.fd_pops_tree_bytes(3, 12345) == 0


def test_header_declares_the_entry_points_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_fd_pops_tree_bytes", "pgt_fd_pops_reduce_dev", "pgt_fd_pops_reduce")
    for name in names:
        assert name + "(" in text
    assert "} pgt_fd_row;" in text and "} pgt_fd_total;" in text
    assert "#define PGT_ABI_VERSION 6" in text
    assert ("Still 6: pgt_fd_row, pgt_fd_total, pgt_fd_pops_tree_bytes / pgt_fd_pops_reduce_dev / pgt_fd_pops_reduce "
            "added (additive as well).") in text
    for line in ("num  = abba - baba",
                 "H = (p_j >= p_k) ? j : k        L = (p_j <= p_k) ? j : k",
                 "G = (p_i >= p_k) ? i : k        S = (p_i <= p_k) ? i : k",
                 "B1 = (q_i*p_H)*(p_H*q_o) - (p_i*q_H)*(p_H*q_o)",
                 "A1 = (p_i*q_L)*(q_L*p_o) - (q_i*p_L)*(q_L*p_o)",
                 "B2 = (p_G*q_j)*(p_G*q_o) - (q_G*p_j)*(p_G*q_o)",
                 "A2 = (q_S*p_j)*(q_S*p_o) - (p_S*q_j)*(q_S*p_o)",
                 "fd_den  = B1 + A1",
                 "fdm_den = (p_j >= p_i ? B1 : B2) + (p_j <= p_i ? A1 : A2)",
                 "fd = fd_den != 0 ? num / fd_den : 0", "fdm = fdm_den != 0 ? num / fdm_den : 0",
                 "out[t * n_win + w]", "f_d is meant for windows with D >= 0", "f_dM covers both directions",
                 "Only the topology ((i,j),k) is computed"):
        assert line in text, line
    assert "f_d / f_dM and user-chosen trio lists are not" not in text  # the sentence now points to the new entry point
    assert "f_d / f_dM of the same trios come from" in text and "pgt_fd_pops_reduce_dev below" in text
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.FD_ROW_DTYPE.names == ("start", "end", "mid", "n", "fd", "fdm", "num", "fd_den", "fdm_den") and _lib.FD_ROW_DTYPE.itemsize == 56
    assert _lib.FD_TOTAL_DTYPE.names == ("num", "fd_den", "fdm_den", "neff", "nskip") and _lib.FD_TOTAL_DTYPE.itemsize == 40


def test_the_build_grid_constant_is_the_one_the_gpu_test_assumes():
    """tests/test_fd_pops.py takes its second-tile case from tests/pops_grid_shapes.py, whose POPS_ONE_WAVE_FROM must be the
    new statistic's kOneWaveFrom."""
    import pops_grid_shapes as shapes
    src = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_fd_pops_kernels.hip")).read()
    m = re.search(r"static constexpr int kOneWaveFrom = (\d+);", src)
    assert m and int(m.group(1)) == shapes.POPS_ONE_WAVE_FROM == 5
    assert shapes.pops_build(1025, 5) == (2, 513, 516)


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    assert "fd_window_pops" in pgt.__all__
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    for k in (3, 8):
        with pytest.raises(_lib.PgtError, match="fd_window_pops: 4 ... 7 populations, one frequency and one count column each") as e:
            pgt.fd_window_pops(ids, pos, [z] * k, [c] * k, 2, 1, 1, 1)
        assert e.value.code == _lib.PGT_EARG
    with pytest.raises(_lib.PgtError, match="4 ... 7 populations"):
        pgt.fd_window_pops(ids, pos, [z] * 4, [c] * 3, 2, 1, 1, 1)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.fd_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 1, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.fd_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 1, 1, 0)
    with pytest.raises(TypeError):  # dstat_window_pops's arguments minus jackknife
        pgt.fd_window_pops(ids, pos, [z] * 4, [c] * 4, 2, 1, 1, 1, jackknife=True)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bin_dir():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return BIN


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_names_the_option_and_both_formats_and_other_values_are_refused(bin_dir, tmp_path):
    tool = os.path.join(bin_dir, "dstatWindowPops")
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("-fd", "PREFIX.pop<i>_pop<j>_pop<k>.fd", "PREFIX.fd.global", "(5) f_d of ((i,j),k)\n(6) f_dM of ((i,j),k)\n(7) num (sum)\n(8) fd_den (sum)\n(9) fdm_den (sum)",
                 "(4) f_d\n(5) f_dM\n(6) num\n(7) fd_den\n(8) fdm_den", "f_d is meant for windows with D >= 0", "f_dM covers both directions",
                 "Only the topology ((i,j),k) is computed", "Martin", "Malinsky", "-jackknife"):
        assert word in r.stdout, word
    m = [str(tmp_path / f"p{k}.mafs") for k in range(4)]
    for p in m:
        open(p, "w").write("chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\nc1\t1\tA\tC\tA\t0.500000\t5\n")
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", out]
    for bad in ("2", "yes", "01"):
        r = run([tool] + head + ["-fd", bad] + m)
        assert r.returncode == 255 and r.stdout == "" and f"-fd must be 0 or 1 (given: {bad})" in r.stderr, (bad, r.returncode, r.stderr)
    r = run([tool] + head + ["-jackknife", "2"] + m)  # the words -jackknife uses
    assert r.returncode == 255 and "-jackknife must be 0 or 1 (given: 2)" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
