"""GPU: the fused dxy + het build (dxy_het_build_kernel in csrc/pgt_kernels.hip) writes the trees of the separate builds.

pgt_dxy_het_reduce_dev builds the dxy tree and both genotype trees in one launch; its header comment promises node values and
tree layout of the separate kernels bit for bit.  Here the same columns go through pgt_dxy_het_reduce_dev, pgt_dxy_reduce_dev
and two pgt_het_reduce_dev calls of one context (the same hints), every workspace filled with 0xFF beforehand, and what the
builds write is compared byte for byte: levels 1 and 2 of the dxy tree, its per-wave partial sums, and level 1 of each
genotype tree (level 2 of a genotype tree comes from tree_up_kernel in both forms).

The column lengths: 129 = a lone ragged tile (one full leaf and one site); 8 193 = a full tile and one site; 20 481 = two full
tiles and half a tile whose genotype leaves end in mid-leaf; 500 003 = 62 tiles, every wave of the grid with one tile."""
import functools

import numpy as np
import pytest

import synth
from helpers import poison_tree
from popgenomicstools_amd._lib import PGT_STAT_DXY, PGT_STAT_HET, WIN_DTYPE
from popgenomicstools_amd.window_scan import windows_to_device

pytestmark = pytest.mark.gpu

SIZES = (129, 8_193, 20_481, 500_003)
MININD = 5
TILE = 8192  # sites per level-2 tile of the dxy tree = per work item of the het build


def pad256(b):
    return -(-b // 256) * 256


def dxy_ranges(n):
    """byte ranges (level 1, level 2, partial sums) of a dxy tree of n sites: tree_layout(PGT_STAT_DXY, n), 16-byte nodes, every
    level padded to 256 bytes, one partial per build wave behind the levels (as test_fst_deep_stage.tree_levels)"""
    tiles = max(1, -(-n // TILE))
    l1 = tiles * 64 * 16
    off2 = pad256(l1)
    end, c = off2 + pad256(tiles * 16), tiles
    while c > 64:  # the upper levels
        c = -(-c // 64)
        end += pad256(c * 16)
    assert tiles <= 2048  # one round: build_grid launches ceil(tiles / 4) workgroups of 4 waves, each wave leaves a partial
    waves = 4 * -(-tiles // 4)
    return (0, l1), (off2, off2 + tiles * 16), (end, end + waves * 16)


def het_level1(n):
    """byte range of level 1 of a genotype tree of n sites: 8-byte nodes of 1024 sites, 64 per level-2 node"""
    return 0, max(1, -(-n // (1024 * 64))) * 64 * 8


@functools.lru_cache(maxsize=1)
def columns():
    """one seeded set of columns of the longest case on the device; every case is a prefix"""
    import torch
    rng = np.random.default_rng(18_2026)
    n = max(SIZES)
    _, pos = synth.chromosomes(rng, n, 1)
    p1, p2, n1, n2 = synth.dxy_columns(rng, n)
    g = [synth.het_column(rng, n).astype(np.int8) for _ in range(2)]
    dev = torch.device("cuda:0")
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            for k, v in (("pos", pos.view(np.int32)), ("p1", p1), ("p2", p2), ("n1", n1), ("n2", n2), ("g1", g[0]), ("g2", g[1]))}


@pytest.mark.parametrize("n", SIZES)
def test_fused_trees_are_the_separate_builds(ctx, n):
    import torch
    c = {k: v[:n] for k, v in columns().items()}
    win = np.zeros(3, dtype=WIN_DTYPE)  # the whole column, its first sites, its last site (one chromosome: run 0)
    win["lo"], win["hi"] = (0, 0, n - 1), (n, min(n, 100), n)
    win_t = windows_to_device(win, c["p1"].device)
    db, hb = ctx.tree_bytes(PGT_STAT_DXY, n), ctx.tree_bytes(PGT_STAT_HET, n)

    def poisoned(nbytes):
        tree = torch.empty(nbytes, dtype=torch.uint8, device=c["p1"].device)
        poison_tree(tree, 0)
        return tree

    fused, dxy, het1, het2 = poisoned(db + 2 * hb), poisoned(db), poisoned(hb), poisoned(hb)
    ctx.dxy_het_reduce_dev(c["pos"], c["p1"], c["p2"], c["n1"], c["n2"], c["g1"], c["g2"], MININD, win_t, tree=fused)
    ctx.dxy_reduce_dev(c["pos"], c["p1"], c["p2"], c["n1"], c["n2"], MININD, win_t, tree=dxy)
    ctx.het_reduce_dev(c["pos"], c["g1"], win_t, tree=het1)
    ctx.het_reduce_dev(c["pos"], c["g2"], win_t, tree=het2)
    torch.cuda.synchronize()
    fused, dxy, het1, het2 = (t.cpu().numpy() for t in (fused, dxy, het1, het2))

    ranges = dxy_ranges(n)
    assert ranges[2][1] <= db
    for name, (lo, hi) in zip(("level 1", "level 2", "partial sums"), ranges):
        got, want = fused[lo:hi], dxy[lo:hi]
        assert not (want == 0xFF).all(), f"dxy {name}: the separate build wrote nothing"
        bad = np.flatnonzero((got != want).reshape(-1, 16).any(axis=1))
        assert bad.size == 0, f"n = {n}: {bad.size} nodes of the dxy tree's {name} differ, first node {int(bad[0])}"
    lo, hi = het_level1(n)
    assert hi <= hb
    for k, want in enumerate((het1, het2)):
        got = fused[db + k * hb + lo: db + k * hb + hi]
        assert not (want[lo:hi] == 0xFF).all(), f"genotype tree {k}: the separate build wrote nothing"
        bad = np.flatnonzero((got != want[lo:hi]).reshape(-1, 8).any(axis=1))
        assert bad.size == 0, f"n = {n}: {bad.size} level-1 nodes of genotype tree {k} differ, first node {int(bad[0])}"
