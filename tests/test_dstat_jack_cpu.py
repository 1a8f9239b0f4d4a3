"""CPU: the block jackknife of dstatWindowPops without a device — the NumPy model against the exact-rational one (the
tolerance the GPU tests then use), the hand-checkable cases, the header / library / binding, the launch arithmetic, and the
refusals of the Python mirror and of the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import dstat_jack_model as model
import dstat_jack_shapes as shapes
import helpers
from popgenomicstools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")


# ---- the float model against the exact evaluation ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", shapes.SMALL_N_WIN)
def test_float_model_stays_within_the_project_tolerance_of_the_exact_one(n_win):
    """d, d_jack and se of all 60 items of the shared table: 1e-9 relative + 1e-12 (helpers.REL / ABS, the tolerance the dstat
    contract states), so the reference alone passes the GPU tests' tolerance.  The worst error is printed."""
    exact, flt = shapes.exact_reference(n_win), shapes.float_reference(n_win)
    worst = {"d": 0.0, "d_jack": 0.0, "se": 0.0}
    for t in range(shapes.MAX_TRIOS):
        for c in range(3):
            e, f = exact[t][c], flt[t][c]
            assert e["n_blocks"] == f["n_blocks"] and e["n_sites"] == f["n_sites"], (n_win, t, c)
            for k in worst:
                if e[k] != e[k]:
                    assert f[k] != f[k], (n_win, t, c, k)
                    continue
                worst[k] = max(worst[k], abs(f[k] - e[k]) / max(abs(e[k]), 1e-300))
                assert helpers.close(f[k], e[k]), (n_win, t, c, k, f[k], e[k])
            assert (e["z"] != e["z"]) == (f["z"] != f["z"])
    print(f"n_win={n_win}: worst relative error of the float model against the exact one: {worst}")


def test_the_recorded_exact_values_are_what_the_exact_model_gives():
    """tests/golden/dstat_jack_exact.json against a fresh evaluation of one of its 60 items (each takes a second)."""
    rows = shapes.synth_rows(shapes.GOLDEN_N_WIN)
    t, c = 7, 1
    fx, fy = model.TOPOLOGY_FIELDS[c]
    fresh = model.jack_exact(rows[fx][t], rows[fy][t], rows["n"][t])
    rec = shapes.exact_reference(shapes.GOLDEN_N_WIN)[t][c]
    for k in ("d", "d_jack", "se", "z", "n_sites", "n_blocks"):
        assert fresh[k] == rec[k], (k, fresh[k], rec[k])


def test_the_table_has_unused_blocks_with_nan_sums():
    rows = shapes.synth_rows(4096)
    empty = rows["n"] == 0
    assert 0.1 < empty.mean() < 0.2 and np.isnan(rows["abba"][empty]).all() and not np.isnan(rows["abba"][~empty]).any()
    assert rows["n"].max() == 512 and rows["bbaa"][~empty].min() > 0 and rows["bbaa"][~empty].max() < 50
    assert shapes.synth_rows(4096, 4).tobytes() == rows[:4].tobytes()  # fewer trios: a prefix


# ---- hand-checkable cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocks,want", shapes.HAND_CASES, ids=[c[0] for c in shapes.HAND_CASES])
def test_hand_checkable_cases(name, blocks, want):
    x, y, m = ([float(b[k]) for b in blocks] for k in range(3))
    m = [int(v) for v in m]
    for fn in (model.jack_float, model.jack_exact):
        if fn is model.jack_exact:  # finite inputs only: it never looks at an unused block
            x, y = [0.0 if v != v else v for v in x], [0.0 if v != v else v for v in y]
        got = fn(np.array(x), np.array(y), np.array(m, dtype=np.uint32))
        assert shapes.same_item(got, want), (name, fn.__name__, got, want)


def test_an_unused_block_changes_nothing_but_is_not_counted():
    rows = shapes.synth_rows(129)[3]
    used = rows["n"] > 0
    assert not used.all()
    a = model.jack_float(rows["abba"], rows["baba"], rows["n"])
    b = model.jack_float(rows["abba"][used], rows["baba"][used], rows["n"][used])
    assert a == b and a["n_blocks"] == int(used.sum()) < rows.size


# ---- header, library, binding -----------------------------------------------------------------------------------------------
def test_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    names = ("pgt_dstat_jackknife_work_bytes", "pgt_dstat_jackknife_dev", "pgt_dstat_jackknife")
    for name in names:
        assert name + "(" in text
    assert "} pgt_dstat_jack;" in text and "#define PGT_ABI_VERSION 6" in text
    assert "Still 6: pgt_dstat_jack, pgt_dstat_jackknife_work_bytes / pgt_dstat_jackknife_dev / pgt_dstat_jackknife added" in text
    assert "jackknife Z scores, f_d" not in text  # the sentence that said they are not computed
    lib = _lib.load()
    assert lib.pgt_abi_version() == 6
    for name in names:
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.DSTAT_JACK_DTYPE.itemsize == 48
    assert _lib.DSTAT_JACK_DTYPE.names == ("d", "d_jack", "se", "z", "n_sites", "n_blocks", "pad_")
    import popgenomicstools_amd as pgt
    assert pgt.topology_order(0, 2, 5) == [(0, 2, 5), (0, 5, 2), (2, 5, 0)]
    assert [(fx, fy) for fx, fy in model.TOPOLOGY_FIELDS] == [("abba", "baba"), ("bbaa", "baba"), ("bbaa", "abba")]


def test_work_bytes_and_the_launch_arithmetic():
    """work_bytes: 0 outside 1 ... 20 trios, monotone in n_win, and exactly what the restated plan gives — which ties
    tests/dstat_jack_shapes.py (and the two table sizes the GPU test derives from it) to jack_plan / jack_work."""
    lib = _lib.load()
    src = open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", "pgt_internal.h")).read()
    for name, value in (("kJackChunk", shapes.CHUNK), ("kJackMaxPartials", shapes.MAX_PARTIALS), ("kJackMaxTrios", shapes.MAX_TRIOS)):
        assert re.search(rf"constexpr uint32_t {name} = {value};", src), name
    assert re.search(r"constexpr int kJackTotalWords = 5;", src) and re.search(r"constexpr int kJackTopologies = 3;", src)
    sizes = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 131072, 131073, 10**6, 10**8, 10**8 + 1)
    for t in (0, 21, 1000):
        assert all(lib.pgt_dstat_jackknife_work_bytes(t, n) == 0 for n in sizes)
    import popgenomicstools_amd as pgt
    for t in (1, 4, 20):
        prev = 0
        for n in sizes:
            b = lib.pgt_dstat_jackknife_work_bytes(t, n)
            assert b == shapes.work_bytes(t, n) == pgt.Context.dstat_jackknife_work_bytes(t, n) and b >= prev and b >= 256 and b % 256 == 0, (t, n, b)
            prev = b
    assert shapes.plan(10**8) == (1562500, 1526, 1024) and shapes.plan(64) == (1, 1, 1) and shapes.plan(65) == (2, 1, 2)
    assert all(shapes.plan(n)[2] <= shapes.MAX_PARTIALS for n in sizes)
    assert shapes.LARGE_N_WIN == (4097, 65537)


# ---- the Python mirror ------------------------------------------------------------------------------------------------------
def test_the_python_mirror_refuses_overlapping_windows_before_any_device_use():
    import popgenomicstools_amd as pgt
    z, c = np.full(8, 0.5), np.full(8, 5, dtype=np.int32)
    ids, pos = np.zeros(8, dtype=np.uint32), np.arange(1, 9, dtype=np.uint32)
    for W, S in ((4, 2), (4, 3), (0, 0)):
        with pytest.raises(_lib.PgtError, match="jackknife") as e:  # no device here: reaching Context() would raise PGT_EDEVICE
            pgt.dstat_window_pops(ids, pos, [z] * 4, [c] * 4, W, S, 1, 1, jackknife=True)
        assert e.value.code == _lib.PGT_EARG and f"winsize {W}" in str(e.value) and f"stepsize {S}" in str(e.value)
    with pytest.raises(_lib.PgtError, match="-minind must be at least 1"):  # the other refusals keep their turn
        pgt.dstat_window_pops(ids, pos, [z] * 4, [c] * 4, 4, 4, 0, 1, jackknife=True)


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "dstatWindowPops")


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_help_describes_the_option(tool):
    r = run([tool])
    assert r.returncode == 0 and r.stderr == ""
    for word in ("-jackknife", "PREFIX.jackknife", "blocks are the", "windows without an analyzed site are left out", "equal weight",
                 "standard error", "number of blocks"):
        assert word in r.stdout, word
    assert "No Z scores are computed" not in r.stdout


def test_the_refusals_come_before_any_file_is_opened(tool, tmp_path):
    missing = [str(tmp_path / f"missing{k}.mafs") for k in range(4)]
    out = str(tmp_path / "o")
    cases = [
        (["-jackknife", "2", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "-jackknife must be 0 or 1"),
        (["-jackknife", "yes", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4"], "-jackknife must be 0 or 1"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0"], "-jackknife 1 needs windows as its blocks"),
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-jackknife", "1"], "-jackknife 1 needs windows that do not overlap"),
        (["-jackknife", "1", "-sizefile", str(tmp_path / "missing.sizes"), "-winsize", "400", "-stepsize", "100"],
         "-jackknife 1 needs windows that do not overlap"),
    ]
    for opts, msg in cases:
        r = run([tool] + opts + ["-out", out] + missing)
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr and "Unable to open" not in r.stderr, (opts, r.stderr)
    # without a refusal the run gets as far as the files
    r = run([tool, "-jackknife", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out] + missing)
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    r = run([tool, "-jackknife", "0", "-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-out", out] + missing)
    assert r.returncode == 255 and "Unable to open Pop1 MAF file" in r.stderr
    assert [f for f in os.listdir(tmp_path) if f.startswith("o")] == []
