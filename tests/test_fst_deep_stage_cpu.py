"""No GPU: which sizes take the deep-stage fst build (tests/fst_deep_shapes.py restates fst_build_launch), and that the shapes of
tests/test_fst_deep_stage.py reach what they are named for.  If a constant of the sources changes, this module fails and names
what to update instead of the GPU tests silently running the other kernel."""
import os
import re

import fst_deep_shapes as shapes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "popgenomicstools_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _has(text, literal):
    """the literal with any run of blanks between its tokens"""
    return re.search(r"\s+".join(re.escape(tok) for tok in literal.split()), text) is not None


def test_the_constants_are_the_literal_definitions_of_the_sources():
    kernels, api = _src("pgt_kernels.hip"), _src("pgt_api.cpp")
    update = "update tests/fst_deep_shapes.py"
    assert _has(kernels, f"kFstBuildBlocks = {shapes.FST_BUILD_BLOCKS};"), update
    assert _has(kernels, f"kFstStage = {shapes.FST_STAGE};"), update
    assert _has(kernels, f"kFstDeepLdsRows = {shapes.DEEP_LDS_ROWS};"), update
    assert _has(kernels, f"kFstDeepBlocks = {shapes.DEEP_BLOCKS};"), update
    assert _has(kernels, f"kFstDeepBlockRows = {shapes.DEEP_BLOCK_ROWS};"), update
    assert _has(kernels, "kFstDeepStage = kFstDeepLdsRows + kFstDeepBlocks * kFstDeepBlockRows;"), update
    assert shapes.DEEP_ROWS >= 64, "the 60 rounds of 10^9 sites must fit a wave's stage with room"
    # the selection and the cap it is worked out with
    assert _has(kernels, "if (build_rounds(tl.count[1], cap) > (uint64_t)kFstStage)"), update
    assert _has(kernels, "hints.fst_build_blocks >= 1 && hints.fst_build_blocks < kFstBuildBlocks ? hints.fst_build_blocks : kFstBuildBlocks"), update
    assert _has(kernels, "const dim3 grid(build_grid(tl.count[1], cap), np);"), update
    # the knob: read where a context is opened, nowhere else
    assert api.count(f'"{shapes.KNOB}"') == 1 and _has(api, f'std::getenv("{shapes.KNOB}")'), update
    assert "getenv" not in kernels, "the kernel file reads no environment: the knob comes with the context's hints"
    assert _has(_src("pgt_internal.h"), "uint32_t fst_build_blocks = 0;"), update


def test_without_the_knob_the_cap_is_kFstBuildBlocks():
    assert shapes.cap_of(None) == shapes.FST_BUILD_BLOCKS == 512
    assert shapes.cap_of(0) == 512 and shapes.cap_of(512) == 512 and shapes.cap_of(100_000) == 512, "values outside 1 .. 511 change nothing"
    assert shapes.cap_of(1) == 1 and shapes.cap_of(511) == 511


def test_which_sizes_take_the_deep_stage():
    # the 8-GPU shard, the 28-pair workload and the extra configs: today's kernel, today's grid
    assert (shapes.rounds_of(100_000_000), shapes.deep(100_000_000)) == (6, False)
    assert (shapes.rounds_of(125_000_000), shapes.deep(125_000_000)) == (8, False)
    # "2.7e8 sites" is 16 rounds of 2048 waves = 268 435 456 sites: the last size of today's kernel.  (270 000 000 sites are
    # 32 959 tiles, 17 rounds: by the rule `rounds > kFstStage` the deep stage, like every size above the boundary.)
    boundary = shapes.FST_STAGE * 4 * shapes.FST_BUILD_BLOCKS * shapes.TILE
    assert boundary == 268_435_456
    assert (shapes.rounds_of(boundary), shapes.deep(boundary)) == (16, False)
    assert (shapes.rounds_of(boundary + 1), shapes.deep(boundary + 1)) == (17, True)
    assert (shapes.rounds_of(270_000_000), shapes.deep(270_000_000)) == (17, True)
    # the headline: 122 071 tiles, 60 rounds of 2035 waves, inside one stage
    assert (shapes.tiles_of(10**9), shapes.rounds_of(10**9), shapes.deep(10**9)) == (122_071, 60, True)
    assert shapes.grid_waves(10**9) == 2036 and 60 < shapes.DEEP_ROWS
    # beyond one stage (the overflow path): above C * 2048 tiles
    assert shapes.rounds_of(shapes.DEEP_ROWS * 2048 * shapes.TILE + 1) == shapes.DEEP_ROWS + 1


def test_the_gpu_shapes_reach_what_they_are_named_for():
    for r in shapes.ROUNDS:
        n = shapes.full_n(r)
        assert shapes.rounds_of(n, 1) == r and shapes.grid_waves(n, 1) == 4 and shapes.tiles_of_wave(n, 1) == [r] * 4
        assert shapes.deep(n, 1) == (r > 16)
        assert shapes.rounds_of(n) == 1 and not shapes.deep(n), "the default context takes one round: today's kernel"
    assert min(shapes.ROUNDS) == 16 and 17 in shapes.ROUNDS and max(shapes.ROUNDS) == 2 * shapes.DEEP_ROWS + 3
    assert {shapes.DEEP_ROWS - 1, shapes.DEEP_ROWS, shapes.DEEP_ROWS + 1, 33, 49} <= set(shapes.ROUNDS)
    for k in range(1, shapes.DEEP_BLOCKS + 1):  # one row past every park, and (from the second on) the park itself as the last row
        assert k * shapes.DEEP_BLOCK_ROWS + 1 in shapes.ROUNDS or k == 1
        assert k * shapes.DEEP_BLOCK_ROWS in shapes.ROUNDS or k == 1
    assert shapes.full_n(max(shapes.ROUNDS)) <= 4_300_000
    for r in shapes.RAGGED_ROUNDS:
        n = shapes.ragged_n(r)
        assert n % shapes.TILE != 0 and n % 128 != 0
        assert shapes.tiles_of(n) == 4 * r - 1 and shapes.rounds_of(n, 1) == r and shapes.deep(n, 1)
        assert shapes.tiles_of_wave(n, 1) == [r, r, r, r - 1]
        assert (shapes.tiles_of(n) - 1) % 4 == 2, "the partial tile is wave 2's last of r"
    assert shapes.PAIRS_ROUNDS in shapes.ROUNDS
