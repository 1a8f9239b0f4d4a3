"""GPU: the block jackknife of Patterson's D (pgt_dstat_jackknife_dev / pgt_dstat_jackknife) on row tables that are synthesised
and uploaded directly (tests/dstat_jack_shapes.py: no ABBA-BABA reduction is needed to test it), and through
dstat_window_pops(..., jackknife=True).

The yardsticks are the two restatements of the definition in tests/dstat_jack_model.py — the exact-rational one up to 4 096
blocks (evaluated once per table and shared; the 4 096-block values are recorded in tests/golden/dstat_jack_exact.json), the
float64 one beyond — never the code under test.  Tolerance: n_blocks and n_sites exact; d, d_jack and se within
|x - y| <= 1e-9 |y| + 1e-12 (helpers.REL / ABS), which tests/test_dstat_jack_cpu.py shows the float model itself to meet
against the exact one at every shape used here; z is, bit for bit, the quotient of the call's own d_jack and se."""

import numpy as np
import pytest

import dstat_jack_model as model
import dstat_jack_shapes as shapes
import helpers
import synth
from helpers import GuardedBuffers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import DSTAT_JACK_DTYPE, DSTAT_ROW_DTYPE
from popgenomicstools_amd.window_scan import RowBuffer, rows_from_device, trio_order

pytestmark = pytest.mark.gpu
ROW = DSTAT_ROW_DTYPE.itemsize
ITEM = DSTAT_JACK_DTYPE.itemsize
PAD_ROWS = 128  # rows of padding on each side of an uploaded table: two whole chunks


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


_uploaded = {}


def upload(rows):
    """[n_trios, n_win] rows as a uint8 CUDA view into a larger tensor whose PAD_ROWS rows before and after would show in any
    result: n = 1000 and NaN sums.  16-byte aligned (a row is 48 bytes)."""
    import torch
    key = id(rows)
    if key not in _uploaded or _uploaded[key][0] is not rows:
        pad = np.zeros(PAD_ROWS, dtype=DSTAT_ROW_DTYPE)
        pad["n"] = 1000
        for f in ("d", "bbaa", "abba", "baba"):
            pad[f] = np.nan
        flat = np.concatenate([pad, np.ascontiguousarray(rows).reshape(-1), pad])
        full = torch.from_numpy(flat.view(np.uint8).copy()).to(_dev())
        view = full[PAD_ROWS * ROW: (PAD_ROWS + rows.size) * ROW]
        assert view.data_ptr() % 16 == 0
        if len(_uploaded) > 8:
            _uploaded.clear()
        _uploaded[key] = (rows, view)
    return _uploaded[key][1]


def jack_dev(ctx, rows, **kw):
    """one pgt_dstat_jackknife_dev call on a [n_trios, n_win] host table -> [n_trios, 3] DSTAT_JACK_DTYPE"""
    n_trios, n_win = rows.shape
    out, _ = ctx.dstat_jackknife_dev(upload(rows), n_win, n_trios, **kw)
    return rows_from_device(out, DSTAT_JACK_DTYPE)[: 3 * n_trios].reshape(n_trios, 3)


def bits(x):
    return np.float64(x).tobytes()


def assert_item(got, want, what):
    assert int(got["n_blocks"]) == want["n_blocks"] and int(got["n_sites"]) == want["n_sites"], (what, got, want)
    assert int(got["pad_"]) == 0, what
    for k in ("d", "d_jack", "se"):
        g, w = float(got[k]), float(want[k])
        print(f"{what} {k}: got {g!r} want {w!r} |diff| {abs(g - w):.3e}")
        assert (g != g) == (w != w), (what, k, g, w)
        assert w != w or helpers.close(g, w), (what, k, g, w)
    z, se = float(got["z"]), float(got["se"])
    if se > 0:
        assert bits(z) == bits(np.float64(got["d_jack"]) / np.float64(got["se"])), (what, "z", got)
    else:
        assert z != z, (what, "z", got)


def reference(n_win, n_trios):
    if n_win <= shapes.EXACT_UP_TO:
        return shapes.exact_reference(n_win)[:n_trios]
    return shapes.float_reference(n_win, n_trios)


# ---- 1: values -------------------------------------------------------------------------------------------------------------------
CASES = [(n_win, t) for n_win in shapes.SMALL_N_WIN for t in (1, 4, 20)] + [(n_win, 4) for n_win in shapes.LARGE_N_WIN]


@pytest.mark.parametrize("n_win,n_trios", CASES)
def test_items_against_the_models(ctx, n_win, n_trios):
    rows = shapes.synth_rows(n_win)[:n_trios] if n_win <= shapes.EXACT_UP_TO else shapes.synth_rows(n_win, n_trios)
    got = jack_dev(ctx, rows)
    want = reference(n_win, n_trios)
    for t in range(n_trios):
        for c in range(3):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} n_trios={n_trios} trio {t} topology {c}")


def hand_rows(blocks):
    """one trio whose topologies 0 and 1 both see (x, y): abba = bbaa = x, baba = y"""
    rows = np.zeros((1, len(blocks)), dtype=DSTAT_ROW_DTYPE)
    for j, (x, y, m) in enumerate(blocks):
        rows[0, j] = (100 * j + 1, 100 * j + 100, 100 * j + 50, m, 0.0, x, x, y)
    return rows


@pytest.mark.parametrize("name,blocks,want", shapes.HAND_CASES, ids=[c[0] for c in shapes.HAND_CASES])
def test_hand_checkable_cases_bit_for_bit(ctx, name, blocks, want):
    got = jack_dev(ctx, hand_rows(blocks))
    for c in (0, 1):
        item = got[0, c]
        assert int(item["n_blocks"]) == want["n_blocks"] and int(item["n_sites"]) == want["n_sites"], (name, c, item)
        for k in ("d", "d_jack", "se", "z"):
            g, w = float(item[k]), want[k]
            assert (g != g and w != w) or bits(g) == bits(w), (name, c, k, g, w)
    if blocks:  # topology 2 takes (bbaa, abba) = (x, x): D = 0 wherever x is not 0
        assert float(got[0, 2]["d"]) == 0.0


def test_nan_in_a_used_row_reaches_its_own_items_only(ctx):
    rows = shapes.synth_rows(129)[:4].copy()
    j = int(np.flatnonzero(rows["n"][1] > 0)[5])
    rows["bbaa"][1, j] = np.nan  # trio 1: topologies 1 and 2 read bbaa, topology 0 does not
    got, clean = jack_dev(ctx, rows), jack_dev(ctx, shapes.synth_rows(129)[:4])
    for t in range(4):
        for c in range(3):
            if t == 1 and c in (1, 2):
                assert all(np.isnan(got[t, c][k]) for k in ("d", "d_jack", "se", "z")) and got[t, c]["n_blocks"] == clean[t, c]["n_blocks"]
            else:
                assert got[t, c].tobytes() == clean[t, c].tobytes(), (t, c)


# ---- 2: isolation and reproducibility -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [129, shapes.N_WIN_PARTIALS_ABOVE_64])
def test_an_item_depends_on_its_own_trio_alone(ctx, n_win):
    rows = shapes.synth_rows(n_win)
    all20 = jack_dev(ctx, rows)
    again = jack_dev(ctx, rows)
    assert all20.tobytes() == again.tobytes(), "two calls on the same input"
    alone = jack_dev(ctx, np.ascontiguousarray(rows[2:3]))
    assert alone[0].tobytes() == all20[2].tobytes(), (alone[0], all20[2])
    other = rows.copy()  # every trio but trio 2 gets other sums and other weights
    for f in ("bbaa", "abba", "baba"):
        other[f][:2] *= 3.0
        other[f][3:] *= 0.5
    other["n"][3:] = np.where(other["n"][3:] > 0, 7, 0)
    assert jack_dev(ctx, other)[2].tobytes() == all20[2].tobytes(), "the other trios' rows changed"


# ---- 3: the workspace contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win,n_trios", [(129, 20), (shapes.N_WIN_PARTIALS_ABOVE_64, 4), (shapes.N_WIN_SECOND_CHUNK, 4)])
def test_nothing_of_the_workspace_survives_and_nothing_outside_is_touched(ctx, n_win, n_trios):
    """work poisoned three ways (the splitmix pattern of pgt_rowbuf_fill, 0xFF bytes, the workspace another table of the same
    size left), out and work between seeded guards, rows a view into padding that would show: the same bytes every time."""
    import torch
    rows = shapes.synth_rows(n_win, n_trios) if n_win > shapes.EXACT_UP_TO else shapes.synth_rows(n_win)[:n_trios]
    other = shapes.synth_rows(n_win, n_trios, seed=1)
    wb = ctx.dstat_jackknife_work_bytes(n_trios, n_win)
    want = jack_dev(ctx, rows)
    g0 = GuardedBuffers([wb, 3 * n_trios * ITEM], 3, _dev())
    ctx.dstat_jackknife_dev(upload(other), n_win, n_trios, out=g0.bufs[1], work=g0.bufs[0])
    g0.check("the other table")
    left = g0.bufs[0].clone()
    assert rows_from_device(g0.bufs[1], DSTAT_JACK_DTYPE).tobytes() != want.tobytes()
    for poison in range(3):
        g = GuardedBuffers([wb, 3 * n_trios * ITEM], 10 + poison, _dev())
        work, out = g.bufs
        if poison == 0:
            ctx.rowbuf_fill(RowBuffer(work.data_ptr(), wb, owner=work), 99)
        elif poison == 1:
            work.fill_(0xFF)
        else:
            work.copy_(left)
        out.fill_(0xFF)
        ctx.dstat_jackknife_dev(upload(rows), n_win, n_trios, out=out, work=work)
        g.check(f"dstat_jackknife_dev poison {poison}")
        assert rows_from_device(out, DSTAT_JACK_DTYPE).tobytes() == want.tobytes(), (n_win, n_trios, poison)
    torch.cuda.synchronize()


def test_host_buffer_form_gives_the_bytes_of_the_device_form(ctx):
    for n_win, n_trios in ((0, 3), (1, 1), (129, 20), (shapes.N_WIN_PARTIALS_ABOVE_64, 4), (65, 2)):
        rows = np.ascontiguousarray(shapes.synth_rows(n_win)[:n_trios]) if n_win <= shapes.EXACT_UP_TO else shapes.synth_rows(n_win, n_trios)
        assert ctx.dstat_jackknife(rows).tobytes() == jack_dev(ctx, rows).tobytes(), (n_win, n_trios)


def test_profiling_reports_the_call_as_query_time(ctx):
    rows = shapes.synth_rows(shapes.N_WIN_PARTIALS_ABOVE_64, 4)
    ctx.set_profiling(True)
    try:
        jack_dev(ctx, rows)
        build_ms, query_ms = ctx.last_kernel_ms()
    finally:
        ctx.set_profiling(False)
    assert build_ms == 0.0 and query_ms > 0.0


def test_graph_replay_follows_the_rows(ctx):
    """captured once (no allocation, no attribute call inside), replayed after the rows were overwritten in place"""
    import torch
    n_win, n_trios = 129, 4
    a, b = shapes.synth_rows(n_win)[:n_trios], shapes.synth_rows(n_win, n_trios, seed=1)
    want = {id(a): jack_dev(ctx, a), id(b): jack_dev(ctx, b)}
    buf = upload(a).clone()
    out = torch.empty(3 * n_trios * ITEM, dtype=torch.uint8, device=_dev())
    work = torch.empty(ctx.dstat_jackknife_work_bytes(n_trios, n_win), dtype=torch.uint8, device=_dev())
    ctx.dstat_jackknife_dev(buf, n_win, n_trios, out=out, work=work)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.dstat_jackknife_dev(buf, n_win, n_trios, out=out, work=work)
    for src in (b, a, b):
        buf.copy_(upload(src))
        out.fill_(0xFF)
        work.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert rows_from_device(out, DSTAT_JACK_DTYPE).reshape(n_trios, 3).tobytes() == want[id(src)].tobytes()


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ctx):
    import torch
    n_win, n_trios = 129, 4
    rows = shapes.synth_rows(n_win)[:n_trios]
    rt = upload(rows)
    wb = ctx.dstat_jackknife_work_bytes(n_trios, n_win)
    g = GuardedBuffers([wb, 3 * n_trios * ITEM], 7, _dev())
    work, out = g.bufs
    before = [b.clone() for b in g.bufs]
    lib, h = ctx._lib, ctx._ctx

    def call(rows_p=rt.data_ptr(), n_win_=n_win, n_trios_=n_trios, out_p=out.data_ptr(), out_bytes=out.numel(), work_p=work.data_ptr(),
             work_bytes=work.numel()):
        return lib.pgt_dstat_jackknife_dev(h, rows_p, n_win_, n_trios_, out_p, out_bytes, work_p, work_bytes, None)

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
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_dstat_jackknife: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    g.check("accepted call")
    assert rows_from_device(out, DSTAT_JACK_DTYPE).reshape(n_trios, 3).tobytes() == jack_dev(ctx, rows).tobytes()
    # the host-buffer form and the Python wrappers
    host = np.ascontiguousarray(rows)
    res = np.zeros((n_trios, 3), dtype=DSTAT_JACK_DTYPE)
    for args, name in (((host.ctypes.data, n_win, 0, res.ctypes.data), "n_trios"), ((host.ctypes.data, n_win, 21, res.ctypes.data), "n_trios"),
                       ((None, n_win, n_trios, res.ctypes.data), "NULL"), ((host.ctypes.data, n_win, n_trios, None), "NULL")):
        assert lib.pgt_dstat_jackknife(h, *args) == _lib.PGT_EARG and name in _lib.last_error(h), (args, _lib.last_error(h))
    with pytest.raises(_lib.PgtError, match="n_trios must be 1 ... 20"):
        ctx.dstat_jackknife_dev(rt, 1, 21)
    with pytest.raises(_lib.PgtError, match="rows: buffer holds"):
        ctx.dstat_jackknife_dev(rt, n_win + 1, n_trios)
    with pytest.raises(_lib.PgtError, match="work: buffer holds"):
        ctx.dstat_jackknife_dev(rt, n_win, n_trios, work=work[: wb - 1])


# ---- 5: end to end ----------------------------------------------------------------------------------------------------------------
def test_dstat_window_pops_with_the_jackknife(pgt, ctx):
    from test_fst_pops import MININD, random_pops
    n, k = 6_011, 5
    rng = np.random.default_rng(3100)
    chr_ids, pos = synth.chromosomes(rng, n, 3, equal=False)
    f, c = random_pops(rng, n, k)
    res = pgt.dstat_window_pops(chr_ids, pos, f, c, 64, 64, MININD, 1, ctx=ctx, jackknife=True)
    plain = pgt.dstat_window_pops(chr_ids, pos, f, c, 64, 64, MININD, 1, ctx=ctx)
    trios = trio_order(k)
    assert set(res) == set(trios) | {"jackknife"} and set(plain) == set(trios) and list(res["jackknife"]) == trios
    for ijk in trios:
        rows = np.ascontiguousarray(res[ijk].rows)
        assert rows.tobytes() == np.ascontiguousarray(plain[ijk].rows).tobytes() and rows.size > 90
        items = res["jackknife"][ijk]
        assert items.dtype == DSTAT_JACK_DTYPE and items.shape == (3,)
        want = model.jack_rows(rows, model.jack_float)
        for cc in range(3):
            assert_item(items[cc], want[cc], f"dstat_window_pops trio {ijk} topology {cc}")
        used = rows["n"] > 0
        assert int(items[0]["n_blocks"]) == int(used.sum()) > 60 and int(items[0]["n_sites"]) == int(rows["n"].sum())
        abba, baba = float(np.sum(rows["abba"][used])), float(np.sum(rows["baba"][used]))
        assert abs(float(items[0]["d"]) - (abba - baba) / (abba + baba)) <= 1e-12
        assert float(items[0]["se"]) > 0 and np.isfinite(items["z"]).all()
    # -skip_missing drops rows from the results, never blocks from the jackknife
    kept = pgt.dstat_window_pops(chr_ids, pos, f, c, 64, 64, MININD, 1, skip_missing=1, ctx=ctx, jackknife=True)
    for ijk in trios:
        assert kept["jackknife"][ijk].tobytes() == res["jackknife"][ijk].tobytes()
