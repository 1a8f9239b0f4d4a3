"""CPU: the block jackknife of a mean over f4 rows (pgt_f4_jackknife*, `f4WindowPops -jackknife 1`) without a device — the
workspace size (D's, for 1 ... 15 quartets), the constant the refusals state against its literal in csrc/, the one estimator body
behind both mean entry points, the layouts that let the f3 jackknife's tables and models serve (tests/f3_jack_model.py), and the
block counts tests/test_f4_jack.py runs at against the launch arithmetic of tests/dstat_jack_shapes.py."""
import os
import re

import numpy as np

import dstat_jack_shapes as shapes
import f3_jack_model as model
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import F3_JACK_DTYPE, F3_ROW_DTYPE, F4_JACK_DTYPE, F4_ROW_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "popgenomicstools_amd", "csrc")
MAX_QUARTETS = 15  # C(6, 4)


def test_work_bytes_are_those_of_the_d_jackknife_for_one_to_fifteen_quartets():
    lib = _lib.load()
    import popgenomicstools_amd as pgt
    sizes = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 131073, 10**6, 10**8)
    for q in (0, 1, 4, 15, 16, 20, 21, 1000):
        for n in sizes:
            b = lib.pgt_f4_jackknife_work_bytes(q, n)
            want = shapes.work_bytes(q, n) if q <= MAX_QUARTETS else 0
            assert b == want == pgt.Context.f4_jackknife_work_bytes(q, n), (q, n, b)
            if 1 <= q <= MAX_QUARTETS:
                assert b == lib.pgt_dstat_jackknife_work_bytes(q, n) == lib.pgt_f3_jackknife_work_bytes(q, n) > 0


def test_the_largest_quartet_count_is_the_literal_in_csrc():
    src = open(os.path.join(CSRC, "pgt_internal.h")).read()
    m = re.search(r"constexpr uint32_t kJackMaxQuartets = (\d+);", src)
    assert m and int(m.group(1)) == MAX_QUARTETS == 6 * 5 * 4 * 3 // 24
    m = re.search(r"constexpr uint32_t kJackMaxTrios = (\d+);", src)
    assert m and int(m.group(1)) == shapes.MAX_TRIOS >= MAX_QUARTETS  # the workspace arithmetic is sized by the larger
    api = open(os.path.join(CSRC, "pgt_api.cpp")).read()
    assert "static_assert(kJackMaxQuartets <= kJackMaxTrios" in api
    text = open(os.path.join(ROOT, "include", "pgtwin.h")).read()
    assert "1 <= n_quartets <= 15" in text and 'messages begin "pgt_f4_jackknife: "' in text


def test_one_estimator_body_serves_both_mean_entry_points():
    """The mean estimator is one template over (Row, Out); the phases are not copied: each phase kernel is defined once."""
    src = open(os.path.join(CSRC, "pgt_dstat_jack_kernels.hip")).read()
    assert "template <class RowT, class OutT>\nstruct Mean {" in src
    assert "using F3Mean = Mean<pgt_f3_row, pgt_f3_jack>;" in src and "using F4Mean = Mean<pgt_f4_row, pgt_f4_jack>;" in src
    assert src.count("static __device__ __forceinline__ double theta_drop(") == 2  # D's and the mean's
    for kernel in ("jack_totals_kernel", "jack_drop_kernel", "jack_var_kernel", "jack_close_kernel"):
        assert len(re.findall(r"__global__ __launch_bounds__\(256\) void " + kernel + r"\(", src)) == 1, kernel
    assert "launch_jackknife<F4Mean>" in src and "launch_jackknife<F3Mean>" in src and "launch_jackknife<D>" in src
    assert "offsetof(pgt_f4_row, f4_ij_kl) == offsetof(pgt_f3_row, f3_i)" in src


def test_the_f3_tables_and_models_serve_through_a_view():
    assert F4_ROW_DTYPE.itemsize == F3_ROW_DTYPE.itemsize == 48 and F4_JACK_DTYPE.itemsize == F3_JACK_DTYPE.itemsize == 48
    assert [F4_ROW_DTYPE.fields[n][1] for n in F4_ROW_DTYPE.names] == [F3_ROW_DTYPE.fields[n][1] for n in F3_ROW_DTYPE.names]
    assert [F4_JACK_DTYPE.fields[n][1] for n in F4_JACK_DTYPE.names] == [F3_JACK_DTYPE.fields[n][1] for n in F3_JACK_DTYPE.names]
    assert F4_JACK_DTYPE.names == ("f4", "f4_jack", "se", "z", "n_sites", "n_blocks", "pad_")
    rows = model.synth_rows(65, MAX_QUARTETS)
    v = np.ascontiguousarray(rows).view(F4_ROW_DTYPE).reshape(rows.shape)
    assert v.shape == (MAX_QUARTETS, 65) and np.array_equal(v["n"], rows["n"])
    for a, b in zip(("f4_ij_kl", "f4_ik_jl", "f4_il_jk"), model.FIELDS):
        assert v[a].tobytes() == rows[b].tobytes()
    assert (rows["n"] == 0).any() and np.isnan(v["f4_ij_kl"][rows["n"] == 0]).all()
    assert MAX_QUARTETS <= model.MAX_TRIOS
    used = sorted(len([b for b in c[1] if b[1] > 0]) for c in model.HAND_CASES)
    assert used[:4] == [0, 1, 2, 2]  # g = 0, 1, 2 among the hand cases, one of them with an unused NaN block


def test_the_block_counts_of_the_gpu_test():
    assert [shapes.plan(n)[:2] for n in (63, 64, 65)] == [(1, 1), (1, 1), (2, 1)]  # around one chunk
    assert shapes.plan(65535) == (1024, 1, 1024) and shapes.plan(65536) == (1024, 1, 1024)  # around 1024 chunks
    assert shapes.plan(65537)[:2] == (1025, 2) and shapes.N_WIN_SECOND_CHUNK == 65537  # chunks_per_wave = 2
    assert shapes.plan(shapes.N_WIN_PARTIALS_ABOVE_64)[2] == 65
