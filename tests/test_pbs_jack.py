"""GPU: the block jackknife of PBS and PBSn1 (pgt_pbs_jackknife_dev / pgt_pbs_jackknife), six items per 88-byte row, on row
tables that are synthesised and uploaded directly (tests/pbs_jack_model.py: every FST, whole or with a block left out, in (0, 0.5)).

The yardsticks are the two restatements of tests/pbs_jack_model.py — the 60-digit one up to 4096 blocks and, recorded, at 65 537;
the float64 one at 4097 (tests/test_pbs_jack_cpu.py holds it to a tenth of the tolerance of the 60-digit one) — the hand cases,
the rows of the EXISTING pgt_pbs_pops_reduce_dev for one block, and pbsn1_of; never the code under test.  Block counts
(tests/dstat_jack_shapes.py: the estimators share the plan): 0 ... 3, around one and two chunks, 4096; 4097 (more than 64
partials) and 65 537 (a wave's second chunk).  Tolerance: n_blocks and n_sites exact; stat, stat_jack and se within
|x - y| <= 1e-9 |y| + 1e-12 (helpers.REL / ABS, as for every other jackknife); z is, bit for bit, the quotient of the call's own
stat_jack and se."""
import numpy as np
import pytest

import dstat_jack_shapes as shapes
import helpers
import pbs_jack_model as model
from helpers import GuardedBuffers
from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import PBS_JACK_DTYPE, PBS_ROW_DTYPE
from popgenomicstools_amd.window_scan import rows_from_device

pytestmark = pytest.mark.gpu
ROW = PBS_ROW_DTYPE.itemsize
ITEM = PBS_JACK_DTYPE.itemsize
ITEMS = model.ITEMS
MAX_TRIOS = model.MAX_TRIOS
PAD_ROWS = 128  # rows of padding on each side of an uploaded table: two whole chunks
VALUES = ("stat", "stat_jack", "se", "z")
bits = model.bits


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def upload(rows):
    """[n_trios, n_win] rows as a uint8 CUDA view into a larger tensor whose PAD_ROWS rows before and after would show in any
    result: n = 1000 and NaN in all nine doubles.  16-byte aligned (128 rows of 88 bytes)."""
    import torch
    pad = np.zeros(PAD_ROWS, dtype=PBS_ROW_DTYPE)
    pad["n"] = 1000
    for f in model.PBS + model.SUMS:
        pad[f] = np.nan
    flat = np.concatenate([pad, np.ascontiguousarray(rows).reshape(-1), pad])
    full = torch.from_numpy(flat.view(np.uint8).copy()).to(_dev())
    view = full[PAD_ROWS * ROW: (PAD_ROWS + rows.size) * ROW]
    assert view.data_ptr() % 16 == 0
    return view


def jack_dev(ctx, rows, **kw):
    """one pgt_pbs_jackknife_dev call on a [n_trios, n_win] host table -> [n_trios, 6] PBS_JACK_DTYPE"""
    n_trios, n_win = rows.shape
    out, _ = ctx.pbs_jackknife_dev(upload(rows), n_win, n_trios, **kw)
    return rows_from_device(out, PBS_JACK_DTYPE)[: ITEMS * n_trios].reshape(n_trios, ITEMS).copy()


def assert_item(got, want, what, quiet=True):
    assert int(got["n_blocks"]) == want["n_blocks"] and int(got["n_sites"]) == want["n_sites"], (what, got, want)
    assert int(got["pad_"]) == 0, what
    for k in ("stat", "stat_jack", "se"):
        g, w = float(got[k]), float(want[k])
        if not quiet:
            print(f"{what} {k}: got {g!r} want {w!r} |diff| {abs(g - w):.3e} of {helpers.REL * abs(w) + helpers.ABS:.3e}")
        assert (g != g) == (w != w), (what, k, g, w)
        assert w != w or helpers.close(g, w), (what, k, g, w)
    z, se = float(got["z"]), float(got["se"])
    if se > 0:
        assert bits(z) == bits(np.float64(got["stat_jack"]) / np.float64(got["se"])), (what, "z", got)
    else:
        assert z != z, (what, "z", got)


def assert_table(got, want, n_win, loud):
    for t in range(got.shape[0]):
        for c in range(ITEMS):
            assert_item(got[t, c], want[t][c], f"n_win={n_win} trio {t} item {c}", quiet=not (loud and t == 0))


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", shapes.SMALL_N_WIN)
def test_items_against_the_60_digit_model(ctx, n_win):
    assert shapes.SMALL_N_WIN == (0, 1, 2, 3, 63, 64, 65, 127, 129, 4096)
    n_trios = MAX_TRIOS if n_win <= 129 else 2  # every trio an independent draw; at 4096 blocks two keep the 60-digit model quick
    rows = model.synth_rows(n_win, n_trios)
    got = jack_dev(ctx, rows)
    assert_table(got, model.ref_reference(n_win, n_trios), n_win, loud=n_win == 4096)
    if n_win == 0:
        for x in got.reshape(-1):
            assert bits(x["stat"]) == 0 == bits(x["stat_jack"]) and int(x["n_blocks"]) == 0 == int(x["n_sites"]) and np.isnan(x["se"]) and np.isnan(x["z"])


def test_items_where_a_lane_re_adds_a_second_partial_against_the_float_model(ctx):
    n_win = shapes.N_WIN_PARTIALS_ABOVE_64
    assert n_win == 4097 and shapes.plan(n_win)[2] == 65
    assert_table(jack_dev(ctx, model.synth_rows(n_win, 2)), model.float_reference(n_win, 2), n_win, loud=True)


def test_items_at_a_waves_second_chunk_against_the_recorded_60_digit_model(ctx):
    n_win = shapes.N_WIN_SECOND_CHUNK
    assert n_win == 65537 == model.GOLDEN_N_WIN and shapes.plan(n_win)[:2] == (1025, 2)
    assert_table(jack_dev(ctx, model.synth_rows(n_win, 2)), model.ref_reference(n_win, 2), n_win, loud=True)


@pytest.mark.parametrize("name,blocks,want", model.HAND_CASES, ids=[c[0] for c in model.HAND_CASES])
def test_the_hand_cases_bit_for_bit(ctx, name, blocks, want):
    got = jack_dev(ctx, model.hand_rows(blocks))
    for c in range(ITEMS):
        assert int(got[0, c]["pad_"]) == 0
        model.check_hand_item(name, c, got[0, c], blocks, want, helpers.close)


@pytest.mark.parametrize("estimator", ["wc", "hudson"])
def test_one_used_block_carries_the_bits_of_the_row_the_reduction_writes(ctx, estimator):
    """a real pgt_pbs_pops_reduce call over a handful of sites: its one row, as the one used block of a table, gives stat of items
    0 ... 2 = the row's own pbs_i, pbs_j, pbs_k bit for bit (one text for the closing arithmetic), items 3 ... 5 = pbsn1_of the row"""
    import popgenomicstools_amd as pgt
    rng = np.random.default_rng(88)
    n = 11
    pos = np.arange(1, n + 1, dtype=np.uint32) * 7
    freqs = [rng.random(n) for _ in range(3)]
    ninds = [rng.integers(4, 12, n).astype(np.int32) for _ in range(3)]
    win = pgt.build_windows_sites(np.array([n], dtype=np.uint64), n, n)
    rows, _ = ctx.pbs_pops_reduce(pos, freqs, ninds, 1, win, estimator=estimator)
    assert rows.shape == (1, 1) and rows["n"][0, 0] == n and all(np.isfinite(rows[f][0, 0]) and rows[f][0, 0] != 0 for f in model.PBS)
    table = np.zeros((1, 3), dtype=PBS_ROW_DTYPE)
    table[0, 1] = rows[0, 0]
    for f in model.PBS + model.SUMS:  # two unused blocks around it
        table[f][0, 0] = table[f][0, 2] = np.nan
    got = jack_dev(ctx, table)
    n1 = pgt.pbsn1_of(rows[0, 0])
    for c in range(ITEMS):
        item = got[0, c]
        assert int(item["n_blocks"]) == 1 and int(item["n_sites"]) == n and np.isnan(item["se"]) and np.isnan(item["z"])
        assert bits(item["stat_jack"]) == bits(item["stat"])
        if c < 3:
            assert bits(item["stat"]) == bits(rows[model.PBS[c]][0, 0]), (c, item["stat"], rows[model.PBS[c]][0, 0])
        else:
            assert helpers.close(float(item["stat"]), float(n1[c - 3])), (c, item["stat"], n1[c - 3])


def test_items_3_to_5_are_pbsn1_of_items_0_to_2(ctx):
    import popgenomicstools_amd as pgt
    got = jack_dev(ctx, model.synth_rows(129, 4))
    as_rows = np.zeros(4, dtype=PBS_ROW_DTYPE)
    for c, f in enumerate(model.PBS):
        as_rows[f] = got["stat"][:, c]
    n1 = pgt.pbsn1_of(as_rows)
    for t in range(4):
        for c in range(3):
            assert helpers.close(float(got["stat"][t, 3 + c]), float(n1[t, c])), (t, c)


def test_64_identical_blocks_have_no_spread(ctx):
    blocks = [((1.5, 2.25, 3.0, 8.0, 9.0, 10.0), 8)] * 64
    got = jack_dev(ctx, model.hand_rows(blocks))
    want = model.hand_stat(blocks)
    for c in range(ITEMS):
        item = got[0, c]
        assert int(item["n_blocks"]) == 64 and int(item["n_sites"]) == 512
        assert helpers.close(float(item["stat"]), float(want[c])) and helpers.close(float(item["stat_jack"]), float(want[c]))
        assert 0.0 <= float(item["se"]) <= 1e-12, (c, item)


def test_an_unused_block_is_selected_away_and_a_nan_in_a_used_one_takes_its_trios_six_items(ctx):
    rows = model.synth_rows(129, 4).copy()
    unused = rows["n"] == 0
    assert unused.any() and all(np.isnan(rows[f][unused]).all() for f in model.PBS + model.SUMS)
    clean = jack_dev(ctx, rows)
    assert all(np.isfinite(clean[k]).all() for k in VALUES)
    tame = rows.copy()
    for f in model.SUMS:  # the unused blocks' sums replaced by finite values: nothing changes
        tame[f][unused] = 12345.0
    for f in model.PBS:  # ... and the fields that are never looked at, in every row
        tame[f] = -54321.0
    tame["start"] = tame["end"] = tame["mid"] = 0
    assert jack_dev(ctx, tame).tobytes() == clean.tobytes()
    j = int(np.flatnonzero(rows["n"][1] > 0)[5])
    for fld in ("den_ik", "num_ij"):  # one sum of one used block of trio 1: every item reads all six sums
        bad = rows.copy()
        bad[fld][1, j] = np.nan
        got = jack_dev(ctx, bad)
        for t in range(4):
            for c in range(ITEMS):
                if t == 1:
                    assert all(np.isnan(got[t, c][k]) for k in VALUES), (fld, c, got[t, c])
                    assert got[t, c]["n_blocks"] == clean[t, c]["n_blocks"] and got[t, c]["n_sites"] == clean[t, c]["n_sites"]
                else:
                    assert got[t, c].tobytes() == clean[t, c].tobytes(), (fld, t, c)


# ---- isolation and reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_win", [129, shapes.N_WIN_PARTIALS_ABOVE_64])
def test_an_items_bits_do_not_depend_on_n_trios(ctx, n_win):
    n_all = MAX_TRIOS if n_win == 129 else 5
    rows = model.synth_rows(n_win, n_all)
    every = jack_dev(ctx, rows)
    assert every.tobytes() == jack_dev(ctx, rows).tobytes(), "two calls on the same input"
    alone = jack_dev(ctx, np.ascontiguousarray(rows[2:3]))
    assert alone[0].tobytes() == every[2].tobytes(), (alone[0], every[2])
    assert jack_dev(ctx, np.ascontiguousarray(rows[:4])).tobytes() == every[:4].tobytes()
    other = rows.copy()  # every trio but trio 2 gets other sums and other weights
    for f in model.NUM:
        other[f][:2] *= 0.5
        other[f][3:] *= 1.5
    other["n"][3:] = np.where(other["n"][3:] > 0, 7, 0)
    assert jack_dev(ctx, other)[2].tobytes() == every[2].tobytes(), "the other trios' rows changed"


def test_the_workspace_is_fully_rewritten_and_nothing_outside_is_touched(ctx):
    n_win, n_trios = shapes.N_WIN_PARTIALS_ABOVE_64, 4
    rows = model.synth_rows(n_win, n_trios)
    wb = ctx.pbs_jackknife_work_bytes(n_trios, n_win)
    assert wb == model.work_bytes(n_trios, n_win) > ctx.f4_jackknife_work_bytes(n_trios, n_win) == shapes.work_bytes(n_trios, n_win)
    want = jack_dev(ctx, rows)
    rt = upload(rows)
    for poison in (0x00, 0xFF):
        g = GuardedBuffers([wb, ITEMS * n_trios * ITEM], 10 + poison, _dev())
        work, out = g.bufs
        work.fill_(poison)
        out.fill_(0xFF)
        ctx.pbs_jackknife_dev(rt, n_win, n_trios, out=out, work=work)
        g.check(f"pbs_jackknife_dev poison {poison}")
        assert rows_from_device(out, PBS_JACK_DTYPE).tobytes() == want.tobytes(), poison


def test_host_buffer_form_gives_the_bytes_of_the_device_form(ctx):
    for n_win, n_trios in ((0, 3), (1, 1), (129, 20), (shapes.N_WIN_PARTIALS_ABOVE_64, 3), (65, 2)):
        rows = np.ascontiguousarray(model.synth_rows(n_win, n_trios))
        host = ctx.pbs_jackknife(rows)
        assert host.shape == (n_trios, ITEMS) and host.tobytes() == jack_dev(ctx, rows).tobytes(), (n_win, n_trios)


def test_a_table_at_an_8_byte_aligned_address_gives_the_same_bytes(ctx):
    """an 88-byte row at an odd index is 8-byte aligned only: so may the table be"""
    import torch
    rows = model.synth_rows(129, 3)
    flat = np.ascontiguousarray(rows).reshape(-1).view(np.uint8)
    full = torch.zeros(flat.size + 64, dtype=torch.uint8, device=_dev())
    view = full[8: 8 + flat.size]
    assert view.data_ptr() % 16 == 8
    view.copy_(torch.from_numpy(flat.copy()))
    out, _ = ctx.pbs_jackknife_dev(view, 129, 3)
    assert rows_from_device(out, PBS_JACK_DTYPE)[: ITEMS * 3].reshape(3, ITEMS).tobytes() == jack_dev(ctx, rows).tobytes()


def test_the_other_four_jackknives_keep_their_bytes_around_a_pbs_call(ctx):
    from popgenomicstools_amd._lib import DSTAT_JACK_DTYPE, F3_JACK_DTYPE, F3_ROW_DTYPE, F4_JACK_DTYPE, F4_ROW_DTYPE, F4RATIO_JACK_DTYPE, F4RATIO_ROW_DTYPE
    from test_f4_jack import upload as upload48
    n_win, n = shapes.N_WIN_PARTIALS_ABOVE_64, 3
    d = np.ascontiguousarray(shapes.synth_rows(n_win, n))
    calls = [(ctx.dstat_jackknife_dev, d, DSTAT_JACK_DTYPE, 3), (ctx.f3_jackknife_dev, d.view(F3_ROW_DTYPE), F3_JACK_DTYPE, 3),
             (ctx.f4_jackknife_dev, d.view(F4_ROW_DTYPE), F4_JACK_DTYPE, 3), (ctx.f4ratio_jackknife_dev, d.view(F4RATIO_ROW_DTYPE), F4RATIO_JACK_DTYPE, 6)]

    def run_all():
        res = []
        for fn, rows, dtype, items in calls:
            out, _ = fn(upload48(rows.reshape(n, n_win)), n_win, n)
            res.append(rows_from_device(out, dtype)[: items * n].tobytes())
        return res

    before = run_all()
    pbs = jack_dev(ctx, model.synth_rows(n_win, n))
    assert run_all() == before
    assert jack_dev(ctx, model.synth_rows(n_win, n)).tobytes() == pbs.tobytes()
    # ... and their values are their models' (the mean of f3 on the first sum, as tests/test_f4ratio_jack.py holds it)
    import f3_jack_model
    f3 = np.frombuffer(before[1], dtype=F3_JACK_DTYPE).reshape(n, 3)
    w = f3_jack_model.jack_float(d["bbaa"][0], d["n"][0])
    assert int(f3[0, 0]["n_blocks"]) == w["n_blocks"] and helpers.close(float(f3[0, 0]["f3"]), w["f3"]) and helpers.close(float(f3[0, 0]["se"]), w["se"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import torch
    n_win, n_trios = 129, 4
    rows = model.synth_rows(n_win, n_trios)
    rt = upload(rows)
    wb = ctx.pbs_jackknife_work_bytes(n_trios, n_win)
    g = GuardedBuffers([wb, ITEMS * n_trios * ITEM], 7, _dev())
    work, out = g.bufs
    before = [b.clone() for b in g.bufs]
    lib, h = ctx._lib, ctx._ctx

    def call(rows_p=rt.data_ptr(), n_win_=n_win, n_trios_=n_trios, out_p=out.data_ptr(), out_bytes=out.numel(), work_p=work.data_ptr(),
             work_bytes=work.numel()):
        return lib.pgt_pbs_jackknife_dev(h, rows_p, n_win_, n_trios_, out_p, out_bytes, work_p, work_bytes, None)

    refusals = [
        (dict(rows_p=None), "rows is NULL"), (dict(out_p=None), "out is NULL"), (dict(work_p=None), "work is NULL"),
        (dict(out_bytes=out.numel() - 1), "out_bytes"), (dict(out_bytes=3 * n_trios * ITEM), "out_bytes"), (dict(out_bytes=0), "out_bytes"),
        (dict(work_bytes=wb - 1), "work_bytes"), (dict(work_bytes=ctx.f4ratio_jackknife_work_bytes(n_trios, n_win)), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
        (dict(rows_p=rt.data_ptr() + 4), "rows is not 8-byte aligned"), (dict(rows_p=rt.data_ptr() + 1), "rows is not 8-byte aligned"),
        (dict(work_p=work.data_ptr() + 8), "work is not 16-byte aligned"),
        (dict(out_p=out.data_ptr() + 4), "out is not 8-byte aligned"),
        (dict(n_trios_=0), "n_trios must be 1 ... 20"), (dict(n_trios_=21), "n_trios must be 1 ... 20"),
        (dict(n_trios_=40), "n_trios must be 1 ... 20"), (dict(n_win_=2 ** 62), "n_win"),
    ]
    for kw, name in refusals:
        rc = call(**kw)
        msg = _lib.last_error(h)
        assert rc == _lib.PGT_EARG and name in msg and msg.startswith("pgt_pbs_jackknife: "), (kw, rc, msg)
    g.check("refused calls")
    for b, was in zip(g.bufs, before):
        assert torch.equal(b, was), "a refused call wrote to a buffer"
    assert call() == _lib.PGT_OK  # the same arguments, unharmed, are accepted
    g.check("accepted call")
    assert rows_from_device(out, PBS_JACK_DTYPE).reshape(n_trios, ITEMS).tobytes() == jack_dev(ctx, rows).tobytes()
    # the host-buffer form and the Python wrappers
    host = np.ascontiguousarray(rows)
    res = np.zeros((n_trios, ITEMS), dtype=PBS_JACK_DTYPE)
    for args, name in (((host.ctypes.data, n_win, 0, res.ctypes.data), "n_trios"), ((host.ctypes.data, n_win, 21, res.ctypes.data), "n_trios"),
                       ((None, n_win, n_trios, res.ctypes.data), "NULL"), ((host.ctypes.data, n_win, n_trios, None), "NULL")):
        assert lib.pgt_pbs_jackknife(h, *args) == _lib.PGT_EARG and name in _lib.last_error(h), (args, _lib.last_error(h))
        assert _lib.last_error(h).startswith("pgt_pbs_jackknife: ")
    assert not res.view(np.uint8).any()
    assert ctx.pbs_jackknife_work_bytes(0, n_win) == 0 == ctx.pbs_jackknife_work_bytes(21, n_win)
    with pytest.raises(_lib.PgtError, match="pbs_jackknife_dev: n_trios must be 1 ... 20"):
        ctx.pbs_jackknife_dev(rt, 1, 21)
    with pytest.raises(_lib.PgtError, match="rows: buffer holds"):
        ctx.pbs_jackknife_dev(rt, n_win + 1, n_trios)


def test_graph_replay_follows_the_rows(ctx):
    """captured once (no allocation, no attribute call inside), replayed after the rows were overwritten in place"""
    import torch
    n_win, n_trios = 129, 4
    a, b = model.synth_rows(n_win, n_trios), model.synth_rows(127, 5).reshape(-1)[: n_trios * n_win].reshape(n_trios, n_win)
    want = {id(a): jack_dev(ctx, a), id(b): jack_dev(ctx, b)}
    assert want[id(a)].tobytes() != want[id(b)].tobytes()
    buf = upload(a).clone()
    out = torch.empty(ITEMS * n_trios * ITEM, dtype=torch.uint8, device=_dev())
    work = torch.empty(ctx.pbs_jackknife_work_bytes(n_trios, n_win), dtype=torch.uint8, device=_dev())
    ctx.pbs_jackknife_dev(buf, n_win, n_trios, out=out, work=work)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx.pbs_jackknife_dev(buf, n_win, n_trios, out=out, work=work)
    for src in (b, a, b):
        buf.copy_(upload(src))
        out.fill_(0xFF)
        work.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert rows_from_device(out, PBS_JACK_DTYPE).reshape(n_trios, ITEMS).tobytes() == want[id(src)].tobytes()


# ---- the Python mirror --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", ["wc", "hudson"])
def test_pbs_window_pops_with_jackknife_is_the_plain_result_plus_the_jackknife_of_its_rows(ctx, estimator):
    """pbs_window_pops(jackknife=True), both estimators (the Hudson reduction has another name than the jackknife): the trio
    results are those of jackknife=False byte for byte; "jackknife" holds, per trio, the bytes pgt_pbs_jackknife gives on the
    returned rows and holds to jack_float; skip_missing=1 drops rows from the results and leaves the blocks alone."""
    import popgenomicstools_amd as pgt
    rng = np.random.default_rng(1590)
    n, k, W, minind = 24_000, 4, 500, 5
    chr_ids = np.repeat(np.arange(2, dtype=np.uint32), n // 2)
    pos = np.concatenate([np.cumsum(rng.integers(1, 30, n // 2)) for _ in range(2)]).astype(np.uint32)
    freqs = [rng.random(n) for _ in range(k)]
    ninds = [rng.integers(0, 21, n).astype(np.int32) for _ in range(k)]
    ninds[1][: 3 * W] = 0  # three windows without a counted site for every trio that holds population 1
    plain = pgt.pbs_window_pops(chr_ids, pos, freqs, ninds, W, W, minind, 1, estimator=estimator, ctx=ctx)
    jk = pgt.pbs_window_pops(chr_ids, pos, freqs, ninds, W, W, minind, 1, estimator=estimator, ctx=ctx, jackknife=True)
    trios = pgt.all_trio_order(k)
    assert list(plain) == trios and set(jk) == set(plain) | {"jackknife"} and list(jk["jackknife"]) == trios
    other = pgt.pbs_window_pops(chr_ids, pos, freqs, ninds, W, W, minind, 1, estimator="hudson" if estimator == "wc" else "wc", ctx=ctx)
    for q in trios:
        rows = np.ascontiguousarray(plain[q].rows)
        assert rows.size == n // W and jk[q].rows.tobytes() == rows.tobytes() and jk[q].total.tobytes() == plain[q].total.tobytes(), q
        assert jk[q].win.tobytes() == plain[q].win.tobytes() and rows.tobytes() != other[q].rows.tobytes()
        assert (int(np.count_nonzero(rows["n"] == 0)) == 3) == (1 in q), q
        got = jk["jackknife"][q]
        assert got.dtype == PBS_JACK_DTYPE and got.shape == (ITEMS,)
        assert got.tobytes() == ctx.pbs_jackknife(rows[None, :])[0].tobytes(), q
        assert int(got["n_blocks"][0]) == np.count_nonzero(rows["n"]) and int(got["n_sites"][0]) == int(rows["n"].sum())
        for c, want in enumerate(model.jack_rows(rows, model.jack_float)):
            assert_item(got[c], want, f"{estimator} trio {q} item {c}")
            assert float(got[c]["se"]) > 0
    kept = pgt.pbs_window_pops(chr_ids, pos, freqs, ninds, W, W, minind, 1, skip_missing=1, estimator=estimator, ctx=ctx, jackknife=True)
    for q in trios:
        assert kept[q].rows.size == np.count_nonzero(plain[q].rows["n"]) and (kept[q].rows.size < plain[q].rows.size) == (1 in q)
        assert kept["jackknife"][q].tobytes() == jk["jackknife"][q].tobytes(), q
