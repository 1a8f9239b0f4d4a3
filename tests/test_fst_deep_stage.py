"""GPU: the deep-stage fst build (FstDeepStage, fst_build_kernel_deep in csrc/pgt_kernels.hip) against today's kernel.

Long columns (more than 16 tiles per wave) are built by a kernel that holds a wave's finished node rows in LDS and register
blocks and writes them after the wave's last tile.  With PGT_FST_BUILD_BLOCKS=1 in the environment when a context is opened
its fst build runs on one workgroup, so four waves walk the whole column and a few million sites reach any number of tiles
per wave; a context opened without the variable builds the same columns in one round with fst_build_kernel<>, which this
change leaves alone.  Tree (levels 1 and 2: what the build writes) and rows of the two contexts must be the same BYTES, on
poisoned workspaces, and the rows must agree with the CPU oracle.  The shapes are tests/fst_deep_shapes.py (checked without a
GPU by tests/test_fst_deep_stage_cpu.py)."""
import functools
import os

import numpy as np
import pytest

import fst_deep_shapes as shapes
import synth
from helpers import ABS, REL, poison_tree, rows_equal
from popgenomicstools_amd._lib import FST_ROW_DTYPE, PGT_STAT_FST
from popgenomicstools_amd.window_scan import rows_from_device, windows_to_device

pytestmark = pytest.mark.gpu

N_MAX = shapes.full_n(max(shapes.ROUNDS))
W_LONG, S_LONG, S_ONE = 50_000, 10_007, 9_973  # prime steps: window edges at every offset of a leaf and of a tile


def _dev():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def contexts(pgt):
    """(context with the knob at 1, default context): the variable is read when a context is opened"""
    saved = os.environ.pop(shapes.KNOB, None)
    try:
        plain = pgt.Context(0)
        os.environ[shapes.KNOB] = "1"
        knob = pgt.Context(0)
    finally:
        os.environ.pop(shapes.KNOB, None)
        if saved is not None:
            os.environ[shapes.KNOB] = saved
    yield knob, plain
    knob.close()
    plain.close()


@functools.lru_cache(maxsize=1)
def genome():
    """One seeded genome of the longest column; every case is a prefix of it (host columns and device tensors)."""
    import torch
    rng = np.random.default_rng(7_2026)
    chr_ids, pos = synth.chromosomes(rng, N_MAX, 3, equal=False)
    a, b = synth.fst_columns(rng, N_MAX)
    dev = _dev()
    t = {"pos": torch.from_numpy(pos.view(np.int32)).to(dev), "a": torch.from_numpy(a).to(dev), "b": torch.from_numpy(b).to(dev)}
    return chr_ids, pos, a, b, t


@functools.lru_cache(maxsize=None)
def case(pgt_mod, oracle, n):
    """-> (window table, device table, oracle rows) of the first n sites: windows of 50 000 sites every 10 007 and one-site windows
    every 9 973 sites, a few hundred of each at the largest n; their edges fall in tiles of every round of every wave"""
    chr_ids, pos, a, b, _ = genome()
    run_len = pgt_mod.run_lengths(chr_ids[:n])
    long_win = pgt_mod.build_windows_sites(run_len, W_LONG, S_LONG)
    long_ref = oracle.fst_scan(chr_ids[:n], pos[:n], a[:n], b[:n], W_LONG, S_LONG)
    assert long_win.size == long_ref.size and np.array_equal(long_win["lo"], long_ref["lo"]) and np.array_equal(long_win["hi"], long_ref["hi"])
    # one-site windows: every 9 973rd site, the two sites on each side of the last tile's start, the last site.  The oracle's row
    # of a one-site window depends on that site alone: it scans the picked sites as a column of their own with W = S = 1
    last_tile = (shapes.tiles_of(n) - 1) * shapes.TILE
    idx = np.unique(np.concatenate((np.arange(0, n, S_ONE), [last_tile - 1, last_tile, n - 1])))
    one_ref = oracle.fst_scan(chr_ids[idx], pos[idx], a[idx], b[idx], 1, 1)
    assert one_ref.size == idx.size and np.array_equal(one_ref["lo"], np.arange(idx.size))
    one_ref["lo"], one_ref["hi"] = idx, idx + 1
    one_win = np.zeros(idx.size, dtype=long_win.dtype)
    one_win["lo"], one_win["hi"], one_win["label_run"] = idx, idx + 1, chr_ids[idx]
    tables, ref = [long_win, one_win], [long_ref, one_ref]
    win = np.concatenate(tables)
    length = (win["hi"] - win["lo"]).astype(np.int64)
    assert np.count_nonzero(length == 1) >= n // S_ONE and np.count_nonzero(length == W_LONG) >= n // S_LONG // 2
    # edges in the first and the last tile of the column, i.e. in a wave's first and last round, and ragged on both sides
    assert int(win["lo"].min()) < shapes.TILE and int(win["hi"].max()) > n - shapes.TILE
    assert np.any(win["lo"] % 128 != 0) and np.any(win["hi"] % 128 != 0)
    return win, windows_to_device(win, _dev()), np.concatenate(ref)


def tree_levels(n):
    """byte ranges of level 1 and level 2 in an fst tree of n sites (tree_layout_for: 16-byte nodes, levels padded to 256 bytes)"""
    tiles = shapes.tiles_of(n)
    l1 = tiles * 64 * 16
    off2 = -(-l1 // 256) * 256
    return (0, l1), (off2, off2 + tiles * 16)


def run(ctx, n, win_t, pairs=1, cols=None):
    """one fst_reduce[_pairs]_dev on trees poisoned with 0xFF -> (rows per pair, tree bytes per pair)"""
    import torch
    _, _, _, _, t = genome()
    n_win = win_t.numel() // 32
    tb = ctx.tree_bytes(PGT_STAT_FST, n)
    tree = torch.empty(pairs * tb, dtype=torch.uint8, device=_dev())
    out = torch.full((pairs * n_win * FST_ROW_DTYPE.itemsize,), 0xFF, dtype=torch.uint8, device=_dev())
    poison_tree(tree, 0)
    if pairs == 1:
        ctx.fst_reduce_dev(t["pos"][:n], t["a"][:n], t["b"][:n], win_t, out=out, tree=tree)
    else:
        ctx.fst_reduce_pairs_dev(t["pos"][:n], [c[0][:n] for c in cols], [c[1][:n] for c in cols], win_t, out=out, tree=tree)
    torch.cuda.synchronize()
    rows = rows_from_device(out, FST_ROW_DTYPE).copy().reshape(pairs, n_win)
    return rows, tree.cpu().numpy().reshape(pairs, tb)


def same_tree(got, want, n, what):
    for name, (lo, hi) in zip(("level 1", "level 2"), tree_levels(n)):
        g, w = got[lo:hi], want[lo:hi]
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g != w).reshape(-1, 16).any(axis=1))
            per = 64 if name == "level 1" else 1
            raise AssertionError(f"{what}: {bad.size} nodes of {name} differ, first node {int(bad[0])} (tile {int(bad[0]) // per}, "
                                 f"round {int(bad[0]) // per // 4} of wave {int(bad[0]) // per % 4})")
    assert got.tobytes() == want.tobytes(), f"{what}: the upper levels differ"


def against_oracle(rows, ref, what):
    for f in ("start", "end", "mid", "n"):
        assert np.array_equal(rows[f], ref[f]), (what, f)
    assert np.array_equal(rows["n"], (ref["hi"] - ref["lo"]).astype(np.uint32)), what
    for f, r in (("fst", "value"), ("asum", "num"), ("bsum", "den")):
        bad = np.abs(rows[f] - ref[r]) > REL * np.abs(ref[r]) + ABS
        assert not bad.any(), (what, f, int(np.flatnonzero(bad)[0]), rows[f][bad][:3], ref[r][bad][:3])


def both(pgt, oracle, contexts, n, what):
    knob, plain = contexts
    win, win_t, ref = case(pgt, oracle, n)
    rows_k, tree_k = run(knob, n, win_t)
    rows_p, tree_p = run(plain, n, win_t)
    same_tree(tree_k[0], tree_p[0], n, what)
    rows_equal(rows_k[0], rows_p[0], what)
    against_oracle(rows_p[0], ref, what + " (default context)")
    against_oracle(rows_k[0], ref, what)


@pytest.mark.parametrize("rounds", shapes.ROUNDS)
def test_whole_tiles(pgt, oracle, contexts, rounds):
    """4 * rounds whole tiles: every wave walks `rounds` of them"""
    both(pgt, oracle, contexts, shapes.full_n(rounds), f"{rounds} rounds")


@pytest.mark.parametrize("rounds", shapes.RAGGED_ROUNDS)
def test_ragged_column(pgt, oracle, contexts, rounds):
    """the last wave walks one tile fewer, and the last tile is partial (the scalar path) and ends inside a leaf"""
    both(pgt, oracle, contexts, shapes.ragged_n(rounds), f"{rounds} rounds, ragged")


def test_two_pairs(pgt, oracle, contexts):
    """grid.y = 2: each pair's tree and rows are the default context's, and pair 0's are those of the one-pair call"""
    knob, plain = contexts
    n = shapes.full_n(shapes.PAIRS_ROUNDS)
    win, win_t, ref = case(pgt, oracle, n)
    _, _, _, _, t = genome()
    cols = [(t["a"], t["b"]), (t["b"], t["a"])]
    rows_k, tree_k = run(knob, n, win_t, 2, cols)
    rows_p, tree_p = run(plain, n, win_t, 2, cols)
    for p in range(2):
        same_tree(tree_k[p], tree_p[p], n, f"pair {p}")
        rows_equal(rows_k[p], rows_p[p], f"pair {p}")
    against_oracle(rows_k[0], ref, "pair 0")
    assert np.array_equal(rows_k[1]["asum"], rows_k[0]["bsum"]) and np.array_equal(rows_k[1]["bsum"], rows_k[0]["asum"])


def test_capture_and_replay(pgt, oracle, contexts):
    """one capture of fst_reduce_dev on the knob's context, replayed on a poisoned tree, equals the eager call bit for bit"""
    import torch
    knob, _ = contexts
    n = shapes.full_n(shapes.PAIRS_ROUNDS)
    _, win_t, _ = case(pgt, oracle, n)
    _, _, _, _, t = genome()
    rows_e, tree_e = run(knob, n, win_t)
    tree = torch.empty(knob.tree_bytes(PGT_STAT_FST, n), dtype=torch.uint8, device=_dev())
    out = torch.empty(rows_e.size * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
    pos, a, b = t["pos"][:n], t["a"][:n], t["b"][:n]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        knob.fst_reduce_dev(pos, a, b, win_t, out=out, tree=tree)
    poison_tree(tree, 0)
    out.fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    same_tree(tree.cpu().numpy(), tree_e[0], n, "replay")
    rows_equal(rows_from_device(out, FST_ROW_DTYPE), rows_e[0], "replay")
