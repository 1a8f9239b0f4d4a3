"""GPU: pgt_sites_align / pgt_gather_dev against numpy (np.intersect1d per chromosome + np.searchsorted): index columns,
per-chromosome counts, n_common and gathered columns bit for bit, guard words around every buffer, poisoned workspaces."""
from functools import reduce

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def expected(files):
    """files[k] = list of (chromosome id, sorted unique u32 positions).  -> (idx per file, count per matched chromosome,
    matched ids): the sites of the chromosomes every file has, by np.intersect1d, located by np.searchsorted."""
    k = len(files)
    offs = [np.concatenate(([0], np.cumsum([len(p) for _, p in f]))).astype(np.int64) for f in files]
    ids = [[c for c, _ in f] for f in files]
    matched = [c for c in ids[0] if all(c in ids[j] for j in range(1, k))]
    idx = [[] for _ in range(k)]
    counts = []
    for c in matched:
        runs = [ids[j].index(c) for j in range(k)]
        common = reduce(np.intersect1d, [files[j][runs[j]][1] for j in range(k)])
        counts.append(common.size)
        for j in range(k):
            idx[j].append(offs[j][runs[j]] + np.searchsorted(files[j][runs[j]][1], common))
    cat = [np.concatenate(x).astype(np.uint32) if x else np.zeros(0, np.uint32) for x in idx]
    return cat, np.array(counts, dtype=np.uint64), matched


def device_pos(files_k, device, skew):
    """One file's position column on the device, `skew` elements past a 16-byte boundary (the kernels' aligned loads must
    cope with any 4-byte aligned column)."""
    import torch
    pos = np.concatenate([p for _, p in files_k]).astype(np.uint32) if files_k else np.zeros(0, np.uint32)
    full = torch.zeros(pos.size + 8, dtype=torch.int32, device=device)
    view = full[skew:skew + pos.size]
    view.copy_(torch.from_numpy(pos.view(np.int32).copy()))
    return pos, view


def check_case(pgt, ctx, files, seed, what):
    import torch
    dev = torch.device("cuda", ctx.device)
    k = len(files)
    want_idx, want_counts, matched = expected(files)
    n = int(want_idx[0].size)
    segs, chr_of = pgt.align_segments_runs([[c for c, _ in f] for f in files], [[len(p) for _, p in f] for f in files])
    assert chr_of.tolist() == matched, what
    host_pos, dev_pos = zip(*[device_pos(files[j], dev, (seed + j) % 4) for j in range(k)])
    wb = ctx.align_workspace_bytes(k, host_pos[0].size)
    assert wb <= 4 * (k + 1) * host_pos[0].size + (1 << 20)
    cap = n + (seed % 3)  # exactly enough, or a little more
    results = []
    for call in range(2):  # a second call into a differently poisoned workspace gives the same bits
        gb = helpers.GuardedBuffers([cap * 4] * k + [wb], seed=seed * 2 + call, device=dev)
        idx_bufs = [b.view(torch.int32) for b in gb.bufs[:k]]
        idx, counts, n_common = ctx.sites_align(list(dev_pos), segs, cap=cap, idx=idx_bufs, work=gb.bufs[k])
        gb.check(f"{what}: sites_align, call {call}")
        assert n_common == n, (what, n_common, n)
        assert counts.tolist() == want_counts.tolist(), what
        got = [t.cpu().numpy().view(np.uint32) for t in idx]
        for j in range(k):
            assert got[j].tobytes() == want_idx[j].tobytes(), (what, "idx", j, call)
            # behind the n_common rows nothing was written
            assert torch.equal(gb.bufs[j][n * 4:], gb.pattern[gb.spans[j][0] + n * 4: gb.spans[j][1]]), (what, "tail of idx", j)
        results.append(idx)
    # gathered columns: u32, f64, i32
    rng = np.random.default_rng(seed)
    for j in (0, k - 1):
        rows = host_pos[j].size
        cols = [host_pos[j].view(np.int32), rng.random(rows), rng.integers(-2**31, 2**31 - 1, rows, dtype=np.int32)]
        gb = helpers.GuardedBuffers([n * c.itemsize for c in cols], seed=seed + 77, device=dev)
        for c, buf in zip(cols, gb.bufs):
            src = torch.from_numpy(np.ascontiguousarray(c)).to(dev) if c is not cols[0] else dev_pos[j]
            out = ctx.gather_dev(src, results[0][j], out=buf.view(src.dtype))
            assert out.cpu().numpy().tobytes() == c[want_idx[j].astype(np.int64)].tobytes(), (what, "gather", j, c.dtype)
        gb.check(f"{what}: gather_dev")
    return n


def draw(rng, universe, keep):
    """a sorted random subset of `universe` holding about keep of it"""
    return universe[rng.random(universe.size) < keep]


def make_universe(rng, n, spread=7):
    return np.unique(rng.integers(1, n * spread + 2, n).astype(np.uint32))


@pytest.mark.parametrize("k", [2, 3, 8])
def test_alignment_is_exact(pgt, ctx, k):
    rng = np.random.default_rng(1000 + k)
    seed = 10 * k
    # identical lists
    u = [make_universe(rng, 5000), make_universe(rng, 300)]
    check_case(pgt, ctx, [[(0, u[0]), (1, u[1])] for _ in range(k)], seed, "identical")
    # nested either way: file 0 inside the others, the others inside file 0
    small = [draw(rng, x, 0.6) for x in u]
    assert check_case(pgt, ctx, [[(0, small[0]), (1, small[1])]] + [[(0, u[0]), (1, u[1])] for _ in range(k - 1)], seed + 1, "file 0 nested") > 0
    assert check_case(pgt, ctx, [[(0, u[0]), (1, u[1])]] + [[(0, small[0]), (1, small[1])] for _ in range(k - 1)], seed + 2, "others nested") > 0
    # random overlap of 50 ... 95 %
    for keep in (0.5, 0.8, 0.95):
        big = make_universe(rng, 40000)
        files = [[(5, draw(rng, big, keep)), (6, draw(rng, u[1], keep))] for _ in range(k)]
        assert check_case(pgt, ctx, files, seed + 3, f"overlap {keep}") > 0
    # one file empty in one chromosome (a run of no rows), and a chromosome missing from one file
    files = [[(0, draw(rng, u[0], 0.9)), (1, draw(rng, u[1], 0.9)), (2, draw(rng, u[1], 0.9))] for _ in range(k)]
    files[k - 1][1] = (1, np.zeros(0, np.uint32))
    check_case(pgt, ctx, files, seed + 4, "empty run in the last file")
    files[0][1] = (1, np.zeros(0, np.uint32))
    check_case(pgt, ctx, files, seed + 5, "empty run in the pivot")
    files = [[(0, draw(rng, u[0], 0.9)), (1, draw(rng, u[1], 0.9)), (2, draw(rng, u[1], 0.9))] for _ in range(k)]
    del files[k // 2][1]
    check_case(pgt, ctx, files, seed + 6, "chromosome missing from one file")
    files = [[(0, draw(rng, u[0], 0.9)), (1, draw(rng, u[1], 0.9)), (2, draw(rng, u[1], 0.9))] for _ in range(k)]
    files[1].insert(1, (77, u[1]))  # ... and one only one file has, in between
    check_case(pgt, ctx, files, seed + 7, "chromosome of one file only")
    # no common site at all: file 0 odd, file 1 even positions; no common chromosome
    files = [[(0, u[0][u[0] % 2 == (j == 0)])] for j in range(k)]
    assert check_case(pgt, ctx, files, seed + 8, "no common site") == 0
    assert check_case(pgt, ctx, [[(j, u[1])] for j in range(k)], seed + 9, "no common chromosome") == 0


@pytest.mark.parametrize("k", [2, 3])
def test_alignment_at_tile_and_segment_edges(pgt, ctx, k):
    rng = np.random.default_rng(2000 + k)
    for n in (1, 127, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193, 65537):
        uni = np.unique(np.concatenate([make_universe(rng, n + n // 4 + 2), [1]]).astype(np.uint32))
        pivot = uni[np.sort(rng.choice(uni.size, min(n, uni.size), replace=False))]
        # three chromosomes: exactly the pivot's n rows, a short one, n rows again — segment starts fall on every alignment
        files = [[(0, pivot), (1, pivot[:3]), (2, pivot)]] + [[(0, draw(rng, uni, 0.9)), (1, uni[:5]), (2, uni)] for _ in range(k - 1)]
        check_case(pgt, ctx, files, 100 + n % 50, f"n = {n}")


def test_alignment_large_and_uneven_density(pgt, ctx):
    rng = np.random.default_rng(3000)
    uni = make_universe(rng, 2_200_000, spread=4)
    assert uni.size > 1_600_000
    files = [[(0, draw(rng, uni[:900_000], 0.9)), (1, draw(rng, uni[900_000:], 0.9))] for _ in range(2)]
    assert sum(len(p) for _, p in files[0]) > 1_500_000
    assert check_case(pgt, ctx, files, 7, "1.6e6 rows, K = 2") > 1_000_000
    files8 = [[(0, draw(rng, uni[:400_000], 0.97))] for _ in range(8)]
    assert check_case(pgt, ctx, files8, 8, "K = 8, 4e5 rows") > 100_000
    # densities 1 : 200 — a tile of the sparse pivot spans far more rows of the dense file than the LDS stage holds ...
    sparse = uni[::200].copy()
    sparse[::7] += 1  # (some of them are no site of the dense file)
    sparse = np.unique(sparse)
    assert check_case(pgt, ctx, [[(3, sparse)], [(3, uni)]], 9, "sparse pivot, dense file") > 5000
    # ... and the other way round: a dense pivot whose tile brackets a handful of rows
    assert check_case(pgt, ctx, [[(3, uni)], [(3, sparse)]], 10, "dense pivot, sparse file") > 5000
    assert check_case(pgt, ctx, [[(3, sparse)], [(3, uni)], [(3, draw(rng, uni, 0.5))]], 11, "sparse pivot, two dense files") > 2000


def test_capacity_too_small(pgt, ctx):
    """PGT_ECAP: the needed count comes back, the first cap sites are written and nothing beyond."""
    import torch
    from popgenomicstools_amd import _lib
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(4000)
    uni = make_universe(rng, 30000)
    files = [[(0, draw(rng, uni, 0.9)), (1, draw(rng, uni, 0.8))] for _ in range(3)]
    want_idx, want_counts, _ = expected(files)
    n = want_idx[0].size
    segs, _ = pgt.align_segments_runs([[c for c, _ in f] for f in files], [[len(p) for _, p in f] for f in files])
    pos = [device_pos(f, dev, 0)[1] for f in files]
    for cap in (0, 1, 1000, n - 1):
        gb = helpers.GuardedBuffers([cap * 4] * 3 + [ctx.align_workspace_bytes(3, pos[0].numel())], seed=cap, device=dev)
        with pytest.raises(_lib.PgtError) as e:
            ctx.sites_align(pos, segs, cap=cap, idx=[b.view(torch.int32) for b in gb.bufs[:3]], work=gb.bufs[3])
        assert e.value.code == _lib.PGT_ECAP and e.value.n_common == n and e.value.counts.tolist() == want_counts.tolist()
        gb.check(f"cap = {cap}")
        for j in range(3):
            assert gb.bufs[j].cpu().numpy().tobytes() == want_idx[j][:cap].tobytes(), (cap, j)
    idx, counts, n_common = ctx.sites_align(pos, segs)  # default capacity: what the plan admits
    assert n_common == n and idx[2].cpu().numpy().view(np.uint32).tobytes() == want_idx[2].tobytes()


def test_argument_errors_by_name(pgt, ctx):
    import ctypes as C
    import torch
    from popgenomicstools_amd import _lib
    dev = torch.device("cuda", ctx.device)
    lib = _lib.load()
    pos = [torch.arange(1, 101, dtype=torch.int32, device=dev) for _ in range(2)]
    segs = np.array([(0, 100), (0, 101)], dtype=_lib.SEG_DTYPE).reshape(1, 2)
    with pytest.raises(_lib.PgtError) as e:
        ctx.sites_align(pos, segs)
    assert e.value.code == _lib.PGT_EARG and "file 1 runs beyond its 100 rows" in str(e.value)
    # the C ABI itself
    wb = ctx.align_workspace_bytes(2, 100)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    idx = [torch.empty(100, dtype=torch.int32, device=dev) for _ in range(2)]
    pp = (C.c_void_p * 2)(pos[0].data_ptr(), pos[1].data_ptr())
    pi = (C.c_void_p * 2)(idx[0].data_ptr(), idx[1].data_ptr())
    nr = (C.c_uint64 * 2)(100, 100)
    cnt = np.zeros(1, np.uint64)
    n_common = C.c_uint64(0)

    def call(pos_=pp, idx_=pi, seg_=segs, work_=work.data_ptr(), wb_=wb, k=2):
        return lib.pgt_sites_align(ctx._ctx, pos_, nr, k, seg_.ctypes.data, seg_.size, idx_, 100, cnt.ctypes.data, C.byref(n_common), work_, wb_, None)
    assert call() == _lib.PGT_EARG and "seg[1] runs beyond n_rows[1]" in _lib.last_error(ctx._ctx)
    good = np.array([(0, 100), (0, 100)], dtype=_lib.SEG_DTYPE)
    assert call(seg_=good, work_=None) == _lib.PGT_EARG and "work is NULL" in _lib.last_error(ctx._ctx)
    assert call(seg_=good, wb_=wb - 1) == _lib.PGT_EARG and "work_bytes too small" in _lib.last_error(ctx._ctx)
    assert call(seg_=good, pos_=None) == _lib.PGT_EARG and "pos is NULL" in _lib.last_error(ctx._ctx)
    assert call(seg_=good, pos_=(C.c_void_p * 2)(pos[0].data_ptr(), None)) == _lib.PGT_EARG and "pos[1] is NULL" in _lib.last_error(ctx._ctx)
    assert call(seg_=good, idx_=(C.c_void_p * 2)(None, idx[1].data_ptr())) == _lib.PGT_EARG and "idx[0] is NULL" in _lib.last_error(ctx._ctx)
    assert call(seg_=good, k=9) == _lib.PGT_EARG and "n_files must be 2 ... 8" in _lib.last_error(ctx._ctx)
    assert call(seg_=good) == _lib.PGT_OK and n_common.value == 100 and cnt[0] == 100
    src = torch.zeros(10, dtype=torch.float64, device=dev)
    for args, text in [((None, src.data_ptr(), idx[0].data_ptr(), 5, 8), "dst is NULL"), ((src.data_ptr(), None, idx[0].data_ptr(), 5, 8), "src is NULL"),
                       ((src.data_ptr(), src.data_ptr(), None, 5, 8), "idx is NULL"), ((src.data_ptr(), src.data_ptr(), idx[0].data_ptr(), 5, 2), "elem_bytes must be 4 or 8")]:
        assert lib.pgt_gather_dev(ctx._ctx, *args, None) == _lib.PGT_EARG and text in _lib.last_error(ctx._ctx), text
    with pytest.raises(_lib.PgtError) as e:
        ctx.gather_dev(torch.zeros(4, dtype=torch.int16, device=dev), idx[0][:2])
    assert "elements of 4 or 8 bytes" in str(e.value)


def test_align_sites_feeds_dxy_window_pops(pgt, ctx):
    """align_sites -> dxy_window_pops gives the rows of dxy_window_pops on columns aligned by numpy, bit for bit (same
    kernel, same input)."""
    rng = np.random.default_rng(5000)
    names = [11, 12, 13]
    uni = {c: make_universe(rng, 6000, spread=3) for c in names}
    chr_len = np.array([int(uni[c].max()) + 100 for c in names], np.uint32)
    for k in (2, 4):
        files = [[(c, draw(rng, uni[c], 0.85)) for c in names] for _ in range(k)]
        chr_ids = [np.concatenate([np.full(len(p), c, np.uint32) for c, p in f]) for f in files]
        pos = [np.concatenate([p for _, p in f]) for f in files]
        freq = [rng.random(p.size).round(6) for p in pos]
        nind = [rng.integers(0, 12, p.size).astype(np.int32) for p in pos]
        want_idx, counts, matched = expected(files)
        a_chr, a_pos, a_cols = pgt.align_sites(chr_ids, pos, [[f, c] for f, c in zip(freq, nind)], ctx=ctx)
        np_chr, np_pos = chr_ids[0][want_idx[0]], pos[0][want_idx[0]]
        assert a_chr.cpu().numpy().view(np.uint32).tobytes() == np_chr.tobytes()
        assert a_pos.cpu().numpy().view(np.uint32).tobytes() == np_pos.tobytes()
        np_freq = [freq[j][want_idx[j]] for j in range(k)]
        np_nind = [nind[j][want_idx[j]] for j in range(k)]
        for j in range(k):
            assert a_cols[j][0].cpu().numpy().tobytes() == np_freq[j].tobytes() and a_cols[j][1].cpu().numpy().tobytes() == np_nind[j].tobytes()
        for kw in (dict(W=50, S=25, fixedsite=1), dict(W=3000, S=1000, fixedsite=0, chr_len=chr_len), dict(W=0, S=0, fixedsite=1)):
            got = pgt.dxy_window_pops(a_chr, a_pos, [c[0] for c in a_cols], [c[1] for c in a_cols], minind=3, ctx=ctx, **kw)
            want = pgt.dxy_window_pops(np_chr, np_pos, np_freq, np_nind, minind=3, ctx=ctx, **kw)
            assert list(got) == pgt.pair_order(k)
            for ij in want:
                helpers.rows_equal(got[ij].rows, want[ij].rows, f"K = {k}, {kw}, pair {ij}")
                assert got[ij].win.tobytes() == want[ij].win.tobytes()
                assert np.asarray(got[ij].total).tobytes() == np.asarray(want[ij].total).tobytes()
