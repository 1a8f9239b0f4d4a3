"""CPU: the per-population nucleotide-diversity front end (pgt_pi_pops_*) — the exact-rational fixture, the NumPy model the GPU
tests compare against, the workspace size, the header as plain C, the Python mirror's refusals that come before the device is opened, and
bin/piWindowPops' usage text."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import pi_pops_model
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import WIN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
sys.path.insert(0, helpers.GOLDEN)


def fixture_columns():
    k = helpers.load_golden("pi_exact.json")
    pos = np.array(k["pos"], dtype=np.uint32)
    freqs = [np.array(f, dtype=np.float64) for f in k["freq"]]
    ninds = [np.array(c, dtype=np.int32) for c in k["nind"]]
    win = np.zeros(len(k["windows"]), dtype=WIN_DTYPE)
    win["lo"], win["hi"] = [w[0] for w in k["windows"]], [w[1] for w in k["windows"]]
    return k, pos, freqs, ninds, win


def test_the_fixture_is_what_its_generator_writes():
    """tests/golden/pi_exact.json is reproducible: the generator gives the committed inputs and sums again."""
    import make_pi_exact as gen
    k, pos, freqs, ninds, win = fixture_columns()
    gpos, gf, gn = gen.inputs()
    assert np.array_equal(gpos, pos) and all(np.array_equal(a, b) for a, b in zip(gf + gn, freqs + ninds))
    assert [list(w) for w in gen.windows()] == k["windows"]
    assert len(freqs) == 3 and pos.size <= 200 and [c["minind"] for c in k["cases"]] == [1, 5]
    for case in k["cases"]:
        for pop in case["pops"]:
            sites = gen.exact_sites(freqs[pop["pop"]], ninds[pop["pop"]], case["minind"])
            for w, (lo, hi) in enumerate(k["windows"]):
                s, neff = gen.exact_window(sites, lo, hi)
                assert (float(s), neff) == (pop["sum"][w], pop["neff"][w])
    assert any(0 < x < 5 for x in k["cases"][0]["pops"][2]["neff"]), "population 2 has the small counts"


def test_the_numpy_model_agrees_with_the_exact_fixture():
    """float64 per-site values in the literal order of the spec, summed: inside the project's bound for these sums (1e-9
    relative + 1e-12) and, every term being >= 0 (no cancellation: four roundings per site, one per addition), far inside it:
    within 1e-13 relative.  Counts exact."""
    k, pos, freqs, ninds, win = fixture_columns()
    whole = k["windows"].index([0, int(pos.size)])
    for case in k["cases"]:
        rows, tot = pi_pops_model.model(pos, freqs, ninds, case["minind"], win)
        for pop in case["pops"]:
            r, want = rows[pop["pop"]], np.array(pop["sum"])
            what = (case["minind"], pop["pop"])
            assert np.array_equal(r["neff"], np.array(pop["neff"], dtype=np.uint32)), what
            assert np.array_equal(r["nskip"], (win["hi"] - win["lo"]).astype(np.uint32) - r["neff"]), what
            assert np.all(np.abs(r["sum"] - want) <= helpers.REL * np.abs(want) + helpers.ABS), what
            assert np.all(np.abs(r["sum"] - want) <= 1e-13 * np.abs(want)), what
            assert np.all(r["sum"] >= 0) and not np.any(np.signbit(r["sum"])), what
            t = tot[pop["pop"]]
            assert int(t["neff"]) == pop["neff"][whole] and int(t["nskip"]) == pos.size - pop["neff"][whole]
            assert abs(float(t["sum"]) - want[whole]) <= 1e-13 * abs(want[whole])


def test_the_model_per_site():
    """the finite-sample factor from the doubles: no integer overflow at INT32_MAX, nothing used where a site is not counted"""
    p = np.array([0.5, 0.5, 0.25, np.nan, 0.5, 0.5])
    c = np.array([1, 2, 2**31 - 1, 0, -7, -2**31], dtype=np.int32)
    v = pi_pops_model.site_pi(p, c)
    assert v[0] == 1.0 and v[1] == 0.5 * (4.0 / 3.0) and v[2] == 0.375 * (4294967294.0 / 4294967293.0)
    pos = np.arange(1, 7, dtype=np.uint32)
    win = np.zeros(7, dtype=WIN_DTYPE)
    win["lo"][:6], win["hi"][:6] = np.arange(6), np.arange(1, 7)
    win["hi"][6] = 6
    rows, tot = pi_pops_model.model(pos, [p], [c], 1, win)
    assert np.array_equal(rows[0]["neff"], [1, 1, 1, 0, 0, 0, 3]) and np.array_equal(rows[0]["nskip"], [0, 0, 0, 1, 1, 1, 3])
    assert np.array_equal(rows[0]["sum"][:6], [v[0], v[1], v[2], 0.0, 0.0, 0.0]) and np.isfinite(rows[0]["sum"][6])
    assert (float(tot[0]["sum"]), int(tot[0]["neff"]), int(tot[0]["nskip"])) == (float(rows[0]["sum"][6]), 3, 3)


def test_tree_bytes():
    lib = _lib.load()
    assert lib.pgt_pi_pops_tree_bytes(0, 1000) == 0 and lib.pgt_pi_pops_tree_bytes(9, 1000) == 0
    sizes = (0, 1, 127, 128, 129, 8192, 8193, 10**6, 10**8, 10**9)
    for k in range(1, 9):
        prev = 0
        for n in sizes:
            tb = lib.pgt_pi_pops_tree_bytes(k, n)
            assert tb >= prev and tb > 0 and tb % 256 == 0
            prev = tb
            if k > 1:  # monotone in the number of populations: one tree each
                assert tb > lib.pgt_pi_pops_tree_bytes(k - 1, n)
            assert tb == k * lib.pgt_tree_bytes(_lib.PGT_STAT_DXY, n)
        assert lib.pgt_pi_pops_tree_bytes(k, 10**9) < 0.02 * 12 * k * 10**9 + (1 << 20)


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "pgtwin.h"\n'
                   "size_t f(void) { return pgt_pi_pops_tree_bytes(1, 1000); }\n"
                   "int g(pgt_ctx *c, const uint32_t *pos, const double *const *fr, const int32_t *const *ni, const pgt_win *w, pgt_dxy_row *o,\n"
                   "      pgt_dxy_total *t, void *tree) {\n"
                   "    return pgt_pi_pops_reduce_dev(c, pos, fr, ni, 1, 10, 1, w, 1, o, sizeof *o, t, tree, 0, 0) + pgt_pi_pops_reduce(c, pos, fr, ni, 1, 10, 1, w, 1, o, t);\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    assert "#define PGT_ABI_VERSION 6" in text and "Still 6: pgt_pi_pops_tree_bytes" in text
    for name in ("pgt_pi_pops_tree_bytes", "pgt_pi_pops_reduce_dev", "pgt_pi_pops_reduce"):
        assert name in _lib.SYMBOLS


def test_the_python_mirror_refuses_before_any_device_use():
    import popgenomicstools_amd as pgt
    z = np.zeros(4)
    c = np.ones(4, dtype=np.int32)
    ids, pos = np.zeros(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):
        pgt.pi_window_pops(ids, pos, [z], [c], 2, 1, 0, 1)
    with pytest.raises(_lib.PgtError, match="size file"):
        pgt.pi_window_pops(ids, pos, [z], [c], 2, 1, 1, 0)
    with pytest.raises(_lib.PgtError, match="1 ... 8 populations"):
        pgt.pi_window_pops(ids, pos, [], [], 2, 1, 1, 1)
    with pytest.raises(_lib.PgtError, match="1 ... 8 populations"):
        pgt.pi_window_pops(ids, pos, [z] * 9, [c] * 9, 2, 1, 1, 1)


# ---- bin/piWindowPops: the usage text (the refusals are in tests/test_cli_pi_pops.py) --------------------------------------------
def test_usage_text():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    r = subprocess.run([os.path.join(BIN, "piWindowPops")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "-out" in r.stdout and "-minind" in r.stdout and ".pi" in r.stdout and "1 <= K <= 8" in r.stdout
    assert "One GPU" in r.stdout and "No passes mode" in r.stdout and "PGT_DXY_SYNC" in r.stdout
