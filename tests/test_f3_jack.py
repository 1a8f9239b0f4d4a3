"""GPU: the block jackknife of a mean (pgt_f3_jackknife_dev / pgt_f3_jackknife) on row tables that are synthesised and uploaded
directly (tests/f3_jack_model.py: no f3 reduction is needed to test it).

The yardsticks are the two restatements of the definition in tests/f3_jack_model.py — the exact-rational one at the small
tables of dstat_jack_shapes.SMALL_N_WIN (the two estimators share the plan, so the sizes at which the kernels take another path
are the same), the float64 one at 4 097 and 65 537 blocks — never the code under test.  Tolerance: n_blocks and n_sites exact;
f3, f3_jack and se within |x - y| <= 1e-9 |y| + 1e-12 (helpers.REL / ABS), of which tests/test_f3_jack_cpu.py shows the float
model to use less than 1 % against the exact one; z is, bit for bit, the quotient of the call's own f3_jack and se."""
import numpy as np
import pytest

import dstat_jack_shapes as shapes
import f3_jack_model as model
import helpers
from helpers import GuardedBuffers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import F3_JACK_DTYPE, F3_ROW_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device

pytestmark = pytest.mark.gpu
ROW = F3_ROW_DTYPE.itemsize
ITEM = F3_JACK_DTYPE.itemsize
PAD_ROWS = 128  # rows of padding on each side of an uploaded table: two whole chunks
EXACT_TRIOS = 4  # trios of a table held to the exact model (every trio of it is an independent draw)


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def upload(rows):
    """[n_trios, n_win] rows as a uint8 CUDA view into a larger tensor whose PAD_ROWS rows before and after would show in any
    result: n = 1000 and NaN sums.  16-byte aligned (a row is 48 bytes)."""
    import torch
    pad = np.zeros(PAD_ROWS, dtype=F3_ROW_DTYPE)
    pad["n"] = 1000
    for f in model.FIELDS:
        pad[f] = np.nan
    flat = np.concatenate([pad, np.ascontiguousarray(rows).reshape(-1), pad])
    full = torch.from_numpy(flat.view(np.uint8).copy()).to(_dev())
    view = full[PAD_ROWS * ROW: (PAD_ROWS + rows.size) * ROW]
    assert view.data_ptr() % 16 == 0
    return view


def jack_dev(ctx, rows, **kw):
    """one pgt_f3_jackknife_dev call on a [n_trios, n_win] host table -> [n_trios, 3] F3_JACK_DTYPE"""
    n_trios, n_win = rows.shape
    out, _ = ctx.f3_jackknife_dev(upload(rows), n_win, n_trios, **kw)
    return rows_from_device(out, F3_JACK_DTYPE)[: 3 * n_trios].reshape(n_trios, 3).copy()


def bits(x):
    return np.float64(x).tobytes()


def assert_item(got, want, what, quiet=True):
    assert int(got["n_blocks"]) == want["n_blocks"] and int(got["n_sites"]) == want["n_sites"], (what, got, want)
    assert int(got["pad_"]) == 0, what
    for k in ("f3", "f3_jack", "se"):
        g, w = float(got[k]), float(want[k])
        if not quiet:
            print(f"{what} {k}: got {g!r} want {w!r} |diff| {abs(g - w):.3e}")
        assert (g != g) == (w != w), (what, k, g, w)
        assert w != w or helpers.close(g, w), (what, k, g, w)
    z, se = float(got["z"]), float(got["se"])
    if se > 0:
        assert bits(z) == bits(np.float64(got["f3_jack"]) / np.float64(got["se"])), (what, "z", got)
    else:
        assert z != z, (what, "z", got)


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", shapes.SMALL_N_WIN)
def test_items_against_the_exact_model(ctx, n_win):
    rows = model.synth_rows(n_win)
    got = jack_dev(ctx, rows)  # all 20 trios in the call; the first EXACT_TRIOS and the last are held to the exact model
    n_exact = EXACT_TRIOS if n_win > 129 else model.MAX_TRIOS
    want = model.exact_reference(n_win, n_exact)
    for t in range(n_exact):
        for c in range(3):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} trio {t} target {c}", quiet=t > 0)
    flt = model.float_reference(n_win)
    for t in range(n_exact, model.MAX_TRIOS):  # the others to the float model, which the CPU test holds to the exact one
        for c in range(3):
            assert_item(got[t, c], flt[t][c], f"n_win={n_win} trio {t} target {c} (float model)")


@pytest.mark.parametrize("n_win", shapes.LARGE_N_WIN)
def test_items_against_the_float_model(ctx, n_win):
    assert shapes.LARGE_N_WIN == (4097, 65537)
    n_trios = 4
    rows = model.synth_rows(n_win, n_trios)
    got = jack_dev(ctx, rows)
    want = model.float_reference(n_win, n_trios)
    for t in range(n_trios):
        for c in range(3):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} trio {t} target {c}", quiet=False)


def hand_rows(blocks):
    """one trio whose three targets see x, 2 x and -x of the case (all exact)"""
    rows = np.zeros((1, len(blocks)), dtype=F3_ROW_DTYPE)
    for j, (x, m) in enumerate(blocks):
        rows[0, j] = (100 * j + 1, 100 * j + 100, 100 * j + 50, m, 0.0, x, 2.0 * x, -x)
    return rows


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_hand_checkable_cases_bit_for_bit(ctx, name, blocks, want):
    got = jack_dev(ctx, hand_rows(blocks))
    for c, scale in ((0, 1.0), (1, 2.0), (2, -1.0)):  # a mean, its jackknife and Z scale with x exactly by a power of two or a sign; se by |scale|
        item = got[0, c]
        assert int(item["n_blocks"]) == want["n_blocks"] and int(item["n_sites"]) == want["n_sites"], (name, c, item)
        for k, s in (("f3", scale), ("f3_jack", scale), ("se", abs(scale)), ("z", np.sign(scale))):
            g, w = float(item[k]), want[k] * s
            assert (g != g and w != w) or g == w, (name, c, k, g, w)
            if c == 0:
                assert (g != g and w != w) or bits(g) == bits(w), (name, k, g, w)


def test_nan_in_a_used_row_reaches_its_own_item_only(ctx):
    rows = model.synth_rows(129)[:4].copy()
    j = int(np.flatnonzero(rows["n"][1] > 0)[5])
    rows["f3_j"][1, j] = np.nan
    got, clean = jack_dev(ctx, rows), jack_dev(ctx, model.synth_rows(129)[:4])
    for t in range(4):
        for c in range(3):
            if (t, c) == (1, 1):
                assert all(np.isnan(got[t, c][k]) for k in ("f3", "f3_jack", "se", "z")) and got[t, c]["n_blocks"] == clean[t, c]["n_blocks"]
            else:
                assert got[t, c].tobytes() == clean[t, c].tobytes(), (t, c)


# ---- isolation and reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [129, shapes.N_WIN_PARTIALS_ABOVE_64])
def test_an_items_bits_do_not_depend_on_n_trios(ctx, n_win):
    rows = model.synth_rows(n_win)
    all20 = jack_dev(ctx, rows)
    assert all20.tobytes() == jack_dev(ctx, rows).tobytes(), "two calls on the same input"
    alone = jack_dev(ctx, np.ascontiguousarray(rows[2:3]))
    assert alone[0].tobytes() == all20[2].tobytes(), (alone[0], all20[2])
    assert jack_dev(ctx, np.ascontiguousarray(rows[:4])).tobytes() == all20[:4].tobytes()
    other = rows.copy()  # every trio but trio 2 gets other sums and other weights
    for f in model.FIELDS:
        other[f][:2] *= 3.0
        other[f][3:] *= 0.5
    other["n"][3:] = np.where(other["n"][3:] > 0, 7, 0)
    assert jack_dev(ctx, other)[2].tobytes() == all20[2].tobytes(), "the other trios' rows changed"


def test_nothing_of_the_workspace_survives_and_nothing_outside_is_touched(ctx):
    n_win, n_trios = shapes.N_WIN_PARTIALS_ABOVE_64, 4
    rows = model.synth_rows(n_win, n_trios)
    wb = ctx.f3_jackknife_work_bytes(n_trios, n_win)
    assert wb == ctx.dstat_jackknife_work_bytes(n_trios, n_win)
    want = jack_dev(ctx, rows)
    rt = upload(rows)
    for poison in (0x00, 0xFF):
        g = GuardedBuffers([wb, 3 * n_trios * ITEM], 10 + poison, _dev())
        work, out = g.bufs
        work.fill_(poison)
        out.fill_(0xFF)
        ctx.f3_jackknife_dev(rt, n_win, n_trios, out=out, work=work)
        g.check(f"f3_jackknife_dev poison {poison}")
        assert rows_from_device(out, F3_JACK_DTYPE).tobytes() == want.tobytes(), poison


def test_host_buffer_form_gives_the_bytes_of_the_device_form(ctx):
    for n_win, n_trios in ((0, 3), (1, 1), (129, 20), (shapes.N_WIN_PARTIALS_ABOVE_64, 4), (65, 2)):
        rows = np.ascontiguousarray(model.synth_rows(n_win, n_trios))
        assert ctx.f3_jackknife(rows).tobytes() == jack_dev(ctx, rows).tobytes(), (n_win, n_trios)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import torch
    n_win, n_trios = 129, 4
    rows = model.synth_rows(n_win, n_trios)
    rt = upload(rows)
    wb = ctx.f3_jackknife_work_bytes(n_trios, n_win)
    g = GuardedBuffers([wb, 3 * n_trios * ITEM], 7, _dev())
    work, out = g.bufs
    before = [b.clone() for b in g.bufs]
    lib, h = ctx._lib, ctx._ctx

    def call(rows_p=rt.data_ptr(), n_win_=n_win, n_trios_=n_trios, out_p=out.data_ptr(), out_bytes=out.numel(), work_p=work.data_ptr(),
             work_bytes=work.numel()):
        return lib.pgt_f3_jackknife_dev(h, rows_p, n_win_, n_trios_, out_p, out_bytes, work_p, work_bytes, None)

    refusals = [
        (dict(rows_p=None), "rows is NULL"), (dict(out_p=None), "out is NULL"), (dict(work_p=None), "work is NULL"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(out_bytes=0), "out_bytes"),
        (dict(work_bytes=wb - 1), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
        (dict(rows_p=rt.data_ptr() + 8), "rows is not 16-byte aligned"), (dict(work_p=work.data_ptr() + 8), "work is not 16-byte aligned"),
        (dict(out_p=out.data_ptr() + 4), "out is not 8-byte aligned"),
        (dict(n_trios_=0), "n_trios must be 1 ... 20"), (dict(n_trios_=21), "n_trios must be 1 ... 20"),
        (dict(n_win_=2 ** 62), "n_win"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f3_jackknife: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    g.check("accepted call")
    assert rows_from_device(out, F3_JACK_DTYPE).reshape(n_trios, 3).tobytes() == jack_dev(ctx, rows).tobytes()
    # the host-buffer form and the Python wrappers
    host = np.ascontiguousarray(rows)
    res = np.zeros((n_trios, 3), dtype=F3_JACK_DTYPE)
    for args, name in (((host.ctypes.data, n_win, 0, res.ctypes.data), "n_trios"), ((host.ctypes.data, n_win, 21, res.ctypes.data), "n_trios"),
                       ((None, n_win, n_trios, res.ctypes.data), "NULL"), ((host.ctypes.data, n_win, n_trios, None), "NULL")):
        assert lib.pgt_f3_jackknife(h, *args) == _lib.PGT_EARG and name in _lib.last_error(h), (args, _lib.last_error(h))
        assert _lib.last_error(h).startswith("pgt_f3_jackknife: ")
    assert not res.view(np.uint8).any()
    with pytest.raises(_lib.PgtError, match="f3_jackknife_dev: n_trios must be 1 ... 20"):
        ctx.f3_jackknife_dev(rt, 1, 21)
    with pytest.raises(_lib.PgtError, match="rows: buffer holds"):
        ctx.f3_jackknife_dev(rt, n_win + 1, n_trios)
