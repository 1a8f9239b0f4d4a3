"""GPU: the block jackknife of the f4-ratio (pgt_f4ratio_jackknife_dev / pgt_f4ratio_jackknife), six items per row, on row
tables that are synthesised and uploaded directly (tests/dstat_jack_shapes.py's tables viewed as F4RATIO_ROW_DTYPE: positive
sums, so no denominator, whole or with a block left out, vanishes or comes near it).

The yardsticks are the two restatements of the ratio jackknife in tests/f4ratio_jack_model.py — the exact-rational one up to
4096 blocks, the float64 one above (tests/test_f4ratio_jack_cpu.py holds it to the exact one) — the hand cases, and the EXISTING
pgt_f4_jackknife_dev on the same bytes, which must still give its own bits; never the code under test.  Block counts
(tests/dstat_jack_shapes.py: the estimators share the plan): 0 ... 3, around one and two chunks, 4096; 4097 (more than 64
partials) and 65 537 (a wave's second chunk).  Tolerance: n_blocks and n_sites exact; alpha, alpha_jack and se within
|x - y| <= 1e-9 |y| + 1e-12 (helpers.REL / ABS, as for f4); z is, bit for bit, the quotient of the call's own alpha_jack and se."""
import numpy as np
import pytest

import dstat_jack_shapes as shapes
import f4ratio_jack_model as model
import helpers
from helpers import GuardedBuffers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import F4_JACK_DTYPE, F4_ROW_DTYPE, F4RATIO_JACK_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device
from test_f4_jack import _dev, bits, upload  # upload: rows between two chunks of padding rows that would show in any result

pytestmark = pytest.mark.gpu
ITEM = F4RATIO_JACK_DTYPE.itemsize
ITEMS = model.ITEMS
MAX_TRIPLES = model.MAX_TRIPLES
FIELDS = model.FIELDS


def jack_dev(ctx, rows, **kw):
    """one pgt_f4ratio_jackknife_dev call on a [n_triples, n_win] host table -> [n_triples, 6] F4RATIO_JACK_DTYPE"""
    n_triples, n_win = rows.shape
    out, _ = ctx.f4ratio_jackknife_dev(upload(rows), n_win, n_triples, **kw)
    return rows_from_device(out, F4RATIO_JACK_DTYPE)[: ITEMS * n_triples].reshape(n_triples, ITEMS).copy()


def f4_jack_dev(ctx, rows):
    """the same bytes as pgt_f4_row through the existing pgt_f4_jackknife_dev -> [n, 3] F4_JACK_DTYPE"""
    n, n_win = rows.shape
    out, _ = ctx.f4_jackknife_dev(upload(rows.view(F4_ROW_DTYPE).reshape(rows.shape)), n_win, n)
    return rows_from_device(out, F4_JACK_DTYPE)[: 3 * n].reshape(n, 3).copy()


def assert_item(got, want, what, quiet=True):
    assert int(got["n_blocks"]) == want["n_blocks"] and int(got["n_sites"]) == want["n_sites"], (what, got, want)
    assert int(got["pad_"]) == 0, what
    for k in ("alpha", "alpha_jack", "se"):
        g, w = float(got[k]), float(want[k])
        if not quiet:
            print(f"{what} {k}: got {g!r} want {w!r} |diff| {abs(g - w):.3e}")
        assert (g != g) == (w != w), (what, k, g, w)
        assert w != w or helpers.close(g, w), (what, k, g, w)
    z, se = float(got["z"]), float(got["se"])
    if se > 0:
        assert bits(z) == bits(np.float64(got["alpha_jack"]) / np.float64(got["se"])), (what, "z", got)
    else:
        assert z != z, (what, "z", got)


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", shapes.SMALL_N_WIN)
def test_items_against_the_exact_model(ctx, n_win):
    assert shapes.SMALL_N_WIN == (0, 1, 2, 3, 63, 64, 65, 127, 129, 4096) and n_win <= shapes.EXACT_UP_TO
    n_triples = MAX_TRIPLES if n_win <= 129 else 2  # every triple an independent draw; at 4096 blocks two keep the exact model quick
    rows = model.synth_rows(n_win, n_triples)
    got = jack_dev(ctx, rows)
    want = model.exact_reference(n_win, n_triples)
    for t in range(n_triples):
        for c in range(ITEMS):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} triple {t} item {c}", quiet=t > 0 or n_win < 4096)
    if n_win == 0:
        assert all(float(x["alpha"]) == 0.0 == float(x["alpha_jack"]) and int(x["n_blocks"]) == 0 for x in got.reshape(-1))


@pytest.mark.parametrize("n_win", shapes.LARGE_N_WIN)
def test_items_against_the_float_model_and_the_f4_jackknife_keeps_its_bits(ctx, n_win):
    assert shapes.LARGE_N_WIN == (4097, 65537) and shapes.plan(4097)[2] == 65 and shapes.plan(65537)[1] == 2
    n_triples = 2
    rows = model.synth_rows(n_win, n_triples)
    got = jack_dev(ctx, rows)
    want = model.float_reference(n_win, n_triples)
    for t in range(n_triples):
        for c in range(ITEMS):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} triple {t} item {c}", quiet=c > 0)
    # the three-item mean on the same bytes: its own bits, before and after a call of the six-item estimator, and its values
    import f3_jack_model
    f4 = f4_jack_dev(ctx, rows)
    jack_dev(ctx, rows)
    assert f4_jack_dev(ctx, rows).tobytes() == f4.tobytes()
    for t in range(n_triples):
        for c, fld in enumerate(FIELDS):
            w = f3_jack_model.jack_float(rows[fld][t], rows["n"][t])
            assert int(f4[t, c]["n_blocks"]) == w["n_blocks"] and helpers.close(float(f4[t, c]["f4"]), w["f3"]) and helpers.close(float(f4[t, c]["se"]), w["se"])


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_the_hand_cases_bit_for_bit(ctx, name, blocks, want):
    """rows (S0, S1, S2) = (num, den, -den): item 5 = q(S0, S1) and item 3 = q(S0, -S2) both read the case"""
    got = jack_dev(ctx, model.hand_rows(blocks))
    for c in (5, 3):
        item = got[0, c]
        assert int(item["n_blocks"]) == want["n_blocks"] and int(item["n_sites"]) == want["n_sites"] and int(item["pad_"]) == 0, (name, c, item)
        for k in ("alpha", "alpha_jack", "se", "z"):
            g, w = float(item[k]), float(want[k])
            assert (g != g and w != w) or bits(g) == bits(w), (name, c, k, g, w)


def test_an_unused_block_with_nan_sums_is_selected_away_and_nan_in_a_used_one_stays_in_the_items_that_read_it(ctx):
    rows = model.synth_rows(129, 4).copy()
    unused = rows["n"] == 0
    assert unused.any() and all(np.isnan(rows[f][unused]).all() for f in FIELDS)
    clean = jack_dev(ctx, rows)
    assert all(np.isfinite(clean[k]).all() for k in ("alpha", "alpha_jack", "se", "z"))
    tame = rows.copy()
    for f in FIELDS:  # the unused blocks' sums replaced by finite values: nothing changes
        tame[f][unused] = 12345.0
    assert jack_dev(ctx, tame).tobytes() == clean.tobytes()
    j = int(np.flatnonzero(rows["n"][1] > 0)[5])
    rows["g_ik"][1, j] = np.nan  # S1 of triple 1: read by items 0, 1 (with S2) and 4, 5 (with S0), not by 2 and 3 (S2 and S0)
    reads_s1 = [c for c, ((_, a), (_, b)) in enumerate(model.RATIOS) if 1 in (a, b)]
    assert reads_s1 == [0, 1, 4, 5]
    got = jack_dev(ctx, rows)
    for t in range(4):
        for c in range(ITEMS):
            if t == 1 and c in reads_s1:
                assert all(np.isnan(got[t, c][k]) for k in ("alpha", "alpha_jack", "se", "z")) and got[t, c]["n_blocks"] == clean[t, c]["n_blocks"]
            else:
                assert got[t, c].tobytes() == clean[t, c].tobytes(), (t, c)


# ---- isolation and reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [129, shapes.N_WIN_PARTIALS_ABOVE_64])
def test_an_items_bits_do_not_depend_on_n_triples(ctx, n_win):
    rows = model.synth_rows(n_win)
    all10 = jack_dev(ctx, rows)
    assert all10.tobytes() == jack_dev(ctx, rows).tobytes(), "two calls on the same input"
    alone = jack_dev(ctx, np.ascontiguousarray(rows[2:3]))
    assert alone[0].tobytes() == all10[2].tobytes(), (alone[0], all10[2])
    assert jack_dev(ctx, np.ascontiguousarray(rows[:4])).tobytes() == all10[:4].tobytes()
    other = rows.copy()  # every triple but triple 2 gets other sums and other weights
    for f in FIELDS:
        other[f][:2] *= 3.0
        other[f][3:] *= 0.5
    other["n"][3:] = np.where(other["n"][3:] > 0, 7, 0)
    assert jack_dev(ctx, other)[2].tobytes() == all10[2].tobytes(), "the other triples' rows changed"


def test_the_workspace_is_fully_rewritten_and_nothing_outside_is_touched(ctx):
    n_win, n_triples = shapes.N_WIN_PARTIALS_ABOVE_64, 4
    rows = model.synth_rows(n_win, n_triples)
    wb = ctx.f4ratio_jackknife_work_bytes(n_triples, n_win)
    assert wb == model.work_bytes(n_triples, n_win) > ctx.f4_jackknife_work_bytes(n_triples, n_win) == shapes.work_bytes(n_triples, n_win)
    want = jack_dev(ctx, rows)
    rt = upload(rows)
    for poison in (0x00, 0xFF):
        g = GuardedBuffers([wb, ITEMS * n_triples * ITEM], 10 + poison, _dev())
        work, out = g.bufs
        work.fill_(poison)
        out.fill_(0xFF)
        ctx.f4ratio_jackknife_dev(rt, n_win, n_triples, out=out, work=work)
        g.check(f"f4ratio_jackknife_dev poison {poison}")
        assert rows_from_device(out, F4RATIO_JACK_DTYPE).tobytes() == want.tobytes(), poison


def test_host_buffer_form_gives_the_bytes_of_the_device_form(ctx):
    for n_win, n_triples in ((0, 3), (1, 1), (129, 10), (shapes.N_WIN_PARTIALS_ABOVE_64, 4), (65, 2)):
        rows = np.ascontiguousarray(model.synth_rows(n_win, n_triples))
        host = ctx.f4ratio_jackknife(rows)
        assert host.shape == (n_triples, ITEMS) and host.tobytes() == jack_dev(ctx, rows).tobytes(), (n_win, n_triples)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import torch
    n_win, n_triples = 129, 4
    rows = model.synth_rows(n_win, n_triples)
    rt = upload(rows)
    wb = ctx.f4ratio_jackknife_work_bytes(n_triples, n_win)
    g = GuardedBuffers([wb, ITEMS * n_triples * ITEM], 7, _dev())
    work, out = g.bufs
    before = [b.clone() for b in g.bufs]
    lib, h = ctx._lib, ctx._ctx

    def call(rows_p=rt.data_ptr(), n_win_=n_win, n_triples_=n_triples, out_p=out.data_ptr(), out_bytes=out.numel(), work_p=work.data_ptr(),
             work_bytes=work.numel()):
        return lib.pgt_f4ratio_jackknife_dev(h, rows_p, n_win_, n_triples_, out_p, out_bytes, work_p, work_bytes, None)

    refusals = [
        (dict(rows_p=None), "rows is NULL"), (dict(out_p=None), "out is NULL"), (dict(work_p=None), "work is NULL"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(out_bytes=3 * n_triples * ITEM), "out_bytes"), (dict(out_bytes=0), "out_bytes"),
        (dict(work_bytes=wb - 1), "work_bytes"), (dict(work_bytes=ctx.f4_jackknife_work_bytes(n_triples, n_win)), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
        (dict(rows_p=rt.data_ptr() + 8), "rows is not 16-byte aligned"), (dict(work_p=work.data_ptr() + 8), "work is not 16-byte aligned"),
        (dict(out_p=out.data_ptr() + 4), "out is not 8-byte aligned"),
        (dict(n_triples_=0), "n_triples must be 1 ... 10"), (dict(n_triples_=11), "n_triples must be 1 ... 10"),
        (dict(n_triples_=20), "n_triples must be 1 ... 10"), (dict(n_win_=2 ** 62), "n_win"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_f4ratio_jackknife: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    g.check("accepted call")
    assert rows_from_device(out, F4RATIO_JACK_DTYPE).reshape(n_triples, ITEMS).tobytes() == jack_dev(ctx, rows).tobytes()
    # the host-buffer form and the Python wrappers
    host = np.ascontiguousarray(rows)
    res = np.zeros((n_triples, ITEMS), dtype=F4RATIO_JACK_DTYPE)
    for args, name in (((host.ctypes.data, n_win, 0, res.ctypes.data), "n_triples"), ((host.ctypes.data, n_win, 11, res.ctypes.data), "n_triples"),
                       ((None, n_win, n_triples, res.ctypes.data), "NULL"), ((host.ctypes.data, n_win, n_triples, None), "NULL")):
        assert lib.pgt_f4ratio_jackknife(h, *args) == _lib.PGT_EARG and name in _lib.last_error(h), (args, _lib.last_error(h))
        assert _lib.last_error(h).startswith("pgt_f4ratio_jackknife: ")
    assert not res.view(np.uint8).any()
    assert ctx.f4ratio_jackknife_work_bytes(0, n_win) == 0 == ctx.f4ratio_jackknife_work_bytes(11, n_win)
    with pytest.raises(_lib.PgtError, match="f4ratio_jackknife_dev: n_triples must be 1 ... 10"):
        ctx.f4ratio_jackknife_dev(rt, 1, 11)
    with pytest.raises(_lib.PgtError, match="rows: buffer holds"):
        ctx.f4ratio_jackknife_dev(rt, n_win + 1, n_triples)
