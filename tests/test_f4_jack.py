"""GPU: the block jackknife of a mean over f4 rows (pgt_f4_jackknife_dev / pgt_f4_jackknife) on row tables that are synthesised
and uploaded directly (tests/f3_jack_model.py's tables, viewed as F4_ROW_DTYPE: the two row types are one layout).

The yardsticks are the two restatements of the mean jackknife in tests/f3_jack_model.py — the exact-rational one at the small
tables, the float64 one at the large ones — and the EXISTING pgt_f3_jackknife_dev on the same bytes, which must give the same
bits; never the code under test.  Block counts (tests/dstat_jack_shapes.py: the estimators share the plan): around one chunk
(63, 64, 65), around 1024 chunks (65 535, 65 536) and the smallest with two chunks per wave (65 537).  Tolerance: n_blocks and
n_sites exact; f4, f4_jack and se within |x - y| <= 1e-9 |y| + 1e-12 (helpers.REL / ABS: the f3 jackknife's contract); z is,
bit for bit, the quotient of the call's own f4_jack and se."""
import numpy as np
import pytest

import dstat_jack_shapes as shapes
import f3_jack_model as model
import helpers
from helpers import GuardedBuffers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import F3_JACK_DTYPE, F3_ROW_DTYPE, F4_JACK_DTYPE, F4_ROW_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device

pytestmark = pytest.mark.gpu
ROW = F4_ROW_DTYPE.itemsize
ITEM = F4_JACK_DTYPE.itemsize
PAD_ROWS = 128  # rows of padding on each side of an uploaded table: two whole chunks
MAX_QUARTETS = 15
FIELDS = ("f4_ij_kl", "f4_ik_jl", "f4_il_jk")
ONE_CHUNK = (63, 64, 65)
LARGE = (shapes.N_WIN_SECOND_CHUNK - 2, shapes.N_WIN_SECOND_CHUNK - 1, shapes.N_WIN_SECOND_CHUNK)  # 65 535, 65 536, 65 537


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def f4_rows(n_win, n_quartets=MAX_QUARTETS):
    """the f3 jackknife tests' synthetic table (signed sums, one block in seven unused with NaN sums) as F4_ROW_DTYPE"""
    return np.ascontiguousarray(model.synth_rows(n_win, n_quartets)).view(F4_ROW_DTYPE).reshape(n_quartets, n_win)


def upload(rows):
    """[n_quartets, n_win] rows as a uint8 CUDA view into a larger tensor whose PAD_ROWS rows before and after would show in any
    result: n = 1000 and NaN sums.  16-byte aligned (a row is 48 bytes)."""
    import torch
    pad = np.zeros(PAD_ROWS, dtype=rows.dtype)
    pad["n"] = 1000
    for f in rows.dtype.names[5:]:
        pad[f] = np.nan
    flat = np.concatenate([pad, np.ascontiguousarray(rows).reshape(-1), pad])
    full = torch.from_numpy(flat.view(np.uint8).copy()).to(_dev())
    view = full[PAD_ROWS * ROW: (PAD_ROWS + rows.size) * ROW]
    assert view.data_ptr() % 16 == 0
    return view


def jack_dev(ctx, rows, **kw):
    """one pgt_f4_jackknife_dev call on a [n_quartets, n_win] host table -> [n_quartets, 3] F4_JACK_DTYPE"""
    n_quartets, n_win = rows.shape
    out, _ = ctx.f4_jackknife_dev(upload(rows), n_win, n_quartets, **kw)
    return rows_from_device(out, F4_JACK_DTYPE)[: 3 * n_quartets].reshape(n_quartets, 3).copy()


def f3_jack_dev(ctx, rows):
    """the same bytes as pgt_f3_row through the existing pgt_f3_jackknife_dev -> [n, 3] F3_JACK_DTYPE"""
    n_trios, n_win = rows.shape
    out, _ = ctx.f3_jackknife_dev(upload(rows.view(F3_ROW_DTYPE).reshape(rows.shape)), n_win, n_trios)
    return rows_from_device(out, F3_JACK_DTYPE)[: 3 * n_trios].reshape(n_trios, 3).copy()


def bits(x):
    return np.float64(x).tobytes()


def assert_item(got, want, what, quiet=True):
    """want: a dict of tests/f3_jack_model.py (its f3 / f3_jack are the mean and its jackknife estimate)"""
    assert int(got["n_blocks"]) == want["n_blocks"] and int(got["n_sites"]) == want["n_sites"], (what, got, want)
    assert int(got["pad_"]) == 0, what
    for k, kw in (("f4", "f3"), ("f4_jack", "f3_jack"), ("se", "se")):
        g, w = float(got[k]), float(want[kw])
        if not quiet:
            print(f"{what} {k}: got {g!r} want {w!r} |diff| {abs(g - w):.3e}")
        assert (g != g) == (w != w), (what, k, g, w)
        assert w != w or helpers.close(g, w), (what, k, g, w)
    z, se = float(got["z"]), float(got["se"])
    if se > 0:
        assert bits(z) == bits(np.float64(got["f4_jack"]) / np.float64(got["se"])), (what, "z", got)
    else:
        assert z != z, (what, "z", got)


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", ONE_CHUNK)
def test_items_against_the_exact_model_and_the_f3_entry_point(ctx, n_win):
    rows = f4_rows(n_win)
    got = jack_dev(ctx, rows)  # all 15 quartets in the call, every one an independent draw
    want = model.exact_reference(n_win, MAX_QUARTETS)
    for q in range(MAX_QUARTETS):
        for c in range(3):
            assert_item(got[q, c], want[q][c], f"n_win={n_win} quartet {q} pairing {c}", quiet=q > 0)
    assert got.tobytes() == f3_jack_dev(ctx, rows).tobytes(), "the same bytes through pgt_f3_jackknife_dev"


@pytest.mark.parametrize("n_win", LARGE)
def test_items_against_the_float_model_and_the_f3_entry_point(ctx, n_win):
    assert LARGE == (65535, 65536, 65537) and [shapes.plan(n)[1] for n in LARGE] == [1, 1, 2] and shapes.plan(65536)[0] == 1024
    n_quartets = 2
    rows = f4_rows(n_win, n_quartets)
    got = jack_dev(ctx, rows)
    want = model.float_reference(n_win, n_quartets)  # tests/test_f3_jack_cpu.py holds it to the exact model
    for q in range(n_quartets):
        for c in range(3):
            assert_item(got[q, c], want[q][c], f"n_win={n_win} quartet {q} pairing {c}", quiet=False)
    assert got.tobytes() == f3_jack_dev(ctx, rows).tobytes(), "the same bytes through pgt_f3_jackknife_dev"


def hand_rows(blocks):
    """one quartet whose three pairings see x, 2 x and -x of the case (all exact)"""
    rows = np.zeros((1, len(blocks)), dtype=F4_ROW_DTYPE)
    for j, (x, m) in enumerate(blocks):
        rows[0, j] = (100 * j + 1, 100 * j + 100, 100 * j + 50, m, 0.0, x, 2.0 * x, -x)
    return rows


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_no_one_two_and_a_few_used_blocks_bit_for_bit(ctx, name, blocks, want):
    """g = 0 ("no block"), g = 1 ("one block"), g = 2 ("two blocks", and again with an unused NaN block between them), 64"""
    assert {len([b for b in c[1] if b[1] > 0]) for c in model.HAND_CASES} >= {0, 1, 2}
    got = jack_dev(ctx, hand_rows(blocks))
    for c, scale in ((0, 1.0), (1, 2.0), (2, -1.0)):  # a mean, its jackknife and Z scale with x exactly by a power of two or a sign; se by |scale|
        item = got[0, c]
        assert int(item["n_blocks"]) == want["n_blocks"] and int(item["n_sites"]) == want["n_sites"], (name, c, item)
        for k, kw, s in (("f4", "f3", scale), ("f4_jack", "f3_jack", scale), ("se", "se", abs(scale)), ("z", "z", np.sign(scale))):
            g, w = float(item[k]), want[kw] * s
            assert (g != g and w != w) or g == w, (name, c, k, g, w)
            if c == 0:
                assert (g != g and w != w) or bits(g) == bits(w), (name, k, g, w)


def test_an_unused_block_with_nan_sums_is_selected_away_and_nan_in_a_used_one_stays_in_its_item(ctx):
    rows = f4_rows(129, 4).copy()
    unused = rows["n"] == 0
    assert unused.any() and all(np.isnan(rows[f][unused]).all() for f in FIELDS)
    clean = jack_dev(ctx, rows)
    assert all(np.isfinite(clean[k]).all() for k in ("f4", "f4_jack", "se", "z"))
    tame = rows.copy()
    for f in FIELDS:  # the unused blocks' sums replaced by finite values: nothing changes
        tame[f][unused] = 12345.0
    assert jack_dev(ctx, tame).tobytes() == clean.tobytes()
    j = int(np.flatnonzero(rows["n"][1] > 0)[5])
    rows["f4_ik_jl"][1, j] = np.nan
    got = jack_dev(ctx, rows)
    for q in range(4):
        for c in range(3):
            if (q, c) == (1, 1):
                assert all(np.isnan(got[q, c][k]) for k in ("f4", "f4_jack", "se", "z")) and got[q, c]["n_blocks"] == clean[q, c]["n_blocks"]
            else:
                assert got[q, c].tobytes() == clean[q, c].tobytes(), (q, c)


# ---- isolation and reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [129, shapes.N_WIN_PARTIALS_ABOVE_64])
def test_an_items_bits_do_not_depend_on_n_quartets(ctx, n_win):
    rows = f4_rows(n_win)
    all15 = jack_dev(ctx, rows)
    assert all15.tobytes() == jack_dev(ctx, rows).tobytes(), "two calls on the same input"
    alone = jack_dev(ctx, np.ascontiguousarray(rows[2:3]))
    assert alone[0].tobytes() == all15[2].tobytes(), (alone[0], all15[2])
    assert jack_dev(ctx, np.ascontiguousarray(rows[:4])).tobytes() == all15[:4].tobytes()
    other = rows.copy()  # every quartet but quartet 2 gets other sums and other weights
    for f in FIELDS:
        other[f][:2] *= 3.0
        other[f][3:] *= 0.5
    other["n"][3:] = np.where(other["n"][3:] > 0, 7, 0)
    assert jack_dev(ctx, other)[2].tobytes() == all15[2].tobytes(), "the other quartets' rows changed"


def test_nothing_of_the_workspace_survives_and_nothing_outside_is_touched(ctx):
    n_win, n_quartets = shapes.N_WIN_PARTIALS_ABOVE_64, 4
    rows = f4_rows(n_win, n_quartets)
    wb = ctx.f4_jackknife_work_bytes(n_quartets, n_win)
    assert wb == ctx.dstat_jackknife_work_bytes(n_quartets, n_win) == shapes.work_bytes(n_quartets, n_win)
    want = jack_dev(ctx, rows)
    rt = upload(rows)
    for poison in (0x00, 0xFF):
        g = GuardedBuffers([wb, 3 * n_quartets * ITEM], 10 + poison, _dev())
        work, out = g.bufs
        work.fill_(poison)
        out.fill_(0xFF)
        ctx.f4_jackknife_dev(rt, n_win, n_quartets, out=out, work=work)
        g.check(f"f4_jackknife_dev poison {poison}")
        assert rows_from_device(out, F4_JACK_DTYPE).tobytes() == want.tobytes(), poison


def test_host_buffer_form_gives_the_bytes_of_the_device_form(ctx):
    for n_win, n_quartets in ((0, 3), (1, 1), (129, 15), (shapes.N_WIN_PARTIALS_ABOVE_64, 4), (65, 2)):
        rows = np.ascontiguousarray(f4_rows(n_win, n_quartets))
        assert ctx.f4_jackknife(rows).tobytes() == jack_dev(ctx, rows).tobytes(), (n_win, n_quartets)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import torch
    n_win, n_quartets = 129, 4
    rows = f4_rows(n_win, n_quartets)
    rt = upload(rows)
    wb = ctx.f4_jackknife_work_bytes(n_quartets, n_win)
    g = GuardedBuffers([wb, 3 * n_quartets * ITEM], 7, _dev())
    work, out = g.bufs
    before = [b.clone() for b in g.bufs]
    lib, h = ctx._lib, ctx._ctx

    def call(rows_p=rt.data_ptr(), n_win_=n_win, n_quartets_=n_quartets, out_p=out.data_ptr(), out_bytes=out.numel(), work_p=work.data_ptr(),
             work_bytes=work.numel()):
        return lib.pgt_f4_jackknife_dev(h, rows_p, n_win_, n_quartets_, out_p, out_bytes, work_p, work_bytes, None)

    refusals = [
        (dict(rows_p=None), "rows is NULL"), (dict(out_p=None), "out is NULL"), (dict(work_p=None), "work is NULL"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(out_bytes=0), "out_bytes"),
        (dict(work_bytes=wb - 1), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
        (dict(rows_p=rt.data_ptr() + 8), "rows is not 16-byte aligned"), (dict(work_p=work.data_ptr() + 8), "work is not 16-byte aligned"),
        (dict(out_p=out.data_ptr() + 4), "out is not 8-byte aligned"),
        (dict(n_quartets_=0), "n_quartets must be 1 ... 15"), (dict(n_quartets_=16), "n_quartets must be 1 ... 15"),
        (dict(n_quartets_=20), "n_quartets must be 1 ... 15"), (dict(n_win_=2 ** 62), "n_win"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f4_jackknife: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    g.check("accepted call")
    assert rows_from_device(out, F4_JACK_DTYPE).reshape(n_quartets, 3).tobytes() == jack_dev(ctx, rows).tobytes()
    # the host-buffer form and the Python wrappers
    host = np.ascontiguousarray(rows)
    res = np.zeros((n_quartets, 3), dtype=F4_JACK_DTYPE)
    for args, name in (((host.ctypes.data, n_win, 0, res.ctypes.data), "n_quartets"), ((host.ctypes.data, n_win, 16, res.ctypes.data), "n_quartets"),
                       ((None, n_win, n_quartets, res.ctypes.data), "NULL"), ((host.ctypes.data, n_win, n_quartets, None), "NULL")):
        assert lib.pgt_f4_jackknife(h, *args) == _lib.PGT_EARG and name in _lib.last_error(h), (args, _lib.last_error(h))
        assert _lib.last_error(h).startswith("pgt_f4_jackknife: ")
    assert not res.view(np.uint8).any()
    assert ctx.f4_jackknife_work_bytes(0, n_win) == 0 == ctx.f4_jackknife_work_bytes(16, n_win)
    with pytest.raises(_lib.PgtError, match="f4_jackknife_dev: n_quartets must be 1 ... 15"):
        ctx.f4_jackknife_dev(rt, 1, 16)
    with pytest.raises(_lib.PgtError, match="rows: buffer holds"):
        ctx.f4_jackknife_dev(rt, n_win + 1, n_quartets)
