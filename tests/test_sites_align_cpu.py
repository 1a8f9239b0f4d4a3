"""CPU: the site-alignment entry points (pgt_align_segments, pgt_align_workspace_bytes) and the refusals of their Python
wrappers, as far as they can be checked without a GPU.  The model of the segment plan lives here: brute force over lists."""
import ctypes as C

import numpy as np
import pytest

from popgenomicstools_amd import _lib


def model_segments(run_chr, run_len):
    """Brute force: 'domain' or the list of (off, len) per (matched chromosome, file), chromosome-major, file 0's order."""
    k = len(run_chr)
    for ids in run_chr:
        if len(set(ids)) != len(ids):
            return "domain"
    matched = [c for c in run_chr[0] if all(c in run_chr[f] for f in range(1, k))]
    for f in range(k):
        if [c for c in run_chr[f] if c in matched] != matched:
            return "domain"
    out = []
    for c in matched:
        for f in range(k):
            r = run_chr[f].index(c)
            out.append((sum(run_len[f][:r]), run_len[f][r]))
    return out


def call_segments(run_chr, run_len, cap=None):
    """-> (rc, n_out, rows written into a buffer of cap entries behind which a canary sits)"""
    lib = _lib.load()
    k = len(run_chr)
    ids = [np.array(c, dtype=np.uint32) for c in run_chr]
    lens = [np.array(r, dtype=np.uint64) for r in run_len]
    pc = (C.c_void_p * k)(*[a.ctypes.data for a in ids])
    pl = (C.c_void_p * k)(*[a.ctypes.data for a in lens])
    nr = (C.c_size_t * k)(*[a.size for a in ids])
    n_out = C.c_size_t(12345)
    if cap is None:
        rc = lib.pgt_align_segments(pc, pl, nr, k, None, 0, C.byref(n_out))
        return rc, n_out.value, None
    buf = np.full(cap + 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64).repeat(2).view(_lib.SEG_DTYPE)
    rc = lib.pgt_align_segments(pc, pl, nr, k, buf.ctypes.data, cap, C.byref(n_out))
    assert (buf["off"][cap:] == 0xA5A5A5A5A5A5A5A5).all() and (buf["len"][cap:] == 0xA5A5A5A5A5A5A5A5).all(), "wrote beyond cap"
    return rc, n_out.value, buf[:cap]


def random_tables(rng):
    k = int(rng.integers(2, 9))
    universe = list(rng.permutation(50)[: int(rng.integers(1, 7))])
    run_chr, run_len = [], []
    for _ in range(k):
        ids = [int(c) for c in universe if rng.random() < 0.85]
        what = rng.random()
        if what < 0.08 and len(ids) >= 2:  # two chromosomes swapped: inconsistent order, if both are matched
            i, j = rng.choice(len(ids), 2, replace=False)
            ids[i], ids[j] = ids[j], ids[i]
        elif what < 0.14 and ids:  # an id in two runs
            ids.insert(int(rng.integers(0, len(ids) + 1)), ids[int(rng.integers(0, len(ids)))])
        elif what < 0.25:  # a chromosome of its own in between
            ids.insert(int(rng.integers(0, len(ids) + 1)), 1000 + len(run_chr))
        run_chr.append(ids)
        run_len.append([int(rng.integers(0, 40)) for _ in ids])
    return run_chr, run_len


def test_align_segments_against_brute_force():
    rng = np.random.default_rng(20240817)
    seen = {"domain": 0, "ok": 0, "empty": 0}
    for _ in range(4000):
        run_chr, run_len = random_tables(rng)
        want = model_segments(run_chr, run_len)
        rc, n, _ = call_segments(run_chr, run_len)
        if want == "domain":
            assert rc == _lib.PGT_EDOMAIN, (run_chr, rc)
            assert "chromosome id" in _lib.last_error(None)
            seen["domain"] += 1
            continue
        assert rc == _lib.PGT_OK and n == len(want), (run_chr, rc, n, len(want))
        rc, n, rows = call_segments(run_chr, run_len, cap=len(want))
        assert rc == _lib.PGT_OK and n == len(want)
        assert [(int(a), int(b)) for a, b in zip(rows["off"], rows["len"])] == want, (run_chr, run_len)
        seen["ok" if want else "empty"] += 1
    assert seen["domain"] > 100 and seen["ok"] > 1000, seen


def test_align_segments_both_refusals_by_name():
    rc, _, _ = call_segments([[3, 7, 3], [3, 7]], [[1, 1, 1], [1, 1]])
    assert rc == _lib.PGT_EDOMAIN and "chromosome id 3 has two runs in file 0" in _lib.last_error(None)
    rc, _, _ = call_segments([[3, 7], [7, 3]], [[1, 1], [1, 1]])
    assert rc == _lib.PGT_EDOMAIN and "chromosome id 7" in _lib.last_error(None) and "file 1" in _lib.last_error(None)
    # an unmatched chromosome in between does not disturb the order
    rc, n, _ = call_segments([[3, 9, 7], [8, 3, 7]], [[1, 1, 1], [1, 1, 1]])
    assert rc == _lib.PGT_OK and n == 4
    for bad_k in (0, 1, 9):
        lib = _lib.load()
        n_out = C.c_size_t(0)
        assert lib.pgt_align_segments(None, None, None, bad_k, None, 0, C.byref(n_out)) == _lib.PGT_EARG


def test_align_segments_capacity_protocol():
    """As pgt_build_windows_sites: out == NULL counts; a short buffer gets its first cap rows, PGT_ECAP and the needed count."""
    run_chr = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 2, 3]]
    run_len = [[5, 6, 7, 8], [1, 2, 3, 4], [9, 9, 9]]
    want = model_segments(run_chr, run_len)
    assert len(want) == 9
    for cap in (0, 1, 4, 8):
        rc, n, rows = call_segments(run_chr, run_len, cap=cap)
        assert rc == _lib.PGT_ECAP and n == 9
        assert [(int(a), int(b)) for a, b in zip(rows["off"], rows["len"])] == want[:cap]
    rc, n, rows = call_segments(run_chr, run_len, cap=20)
    assert rc == _lib.PGT_OK and n == 9
    assert [(int(a), int(b)) for a, b in zip(rows["off"][:9], rows["len"][:9])] == want


def test_align_workspace_bytes_bound():
    lib = _lib.load()
    for bad in (0, 1, 9, 100):
        assert lib.pgt_align_workspace_bytes(bad, 10**6) == 0
    for k in range(2, 9):
        prev = 0
        for n in (0, 1, 127, 128, 1023, 1024, 1025, 8193, 65537, 10**6, 10**8, 4 * 10**9):
            wb = lib.pgt_align_workspace_bytes(k, n)
            assert wb > 0 and wb >= prev, (k, n, wb)
            assert wb <= 4 * (k + 1) * n + (1 << 20), (k, n, wb)  # the bound include/pgtwin.h states
            prev = wb


def test_python_wrappers_refuse_before_the_device():
    """Argument refusals of align_segments / align_sites come before a context is opened: the same on a box without a GPU."""
    import popgenomicstools_amd as pgt
    chr_a, pos_a = np.zeros(5, np.uint32), np.arange(1, 6, dtype=np.uint32)
    f8, i4 = np.full(5, 0.5), np.full(5, 3, np.int32)
    cases = [
        (lambda: pgt.align_segments([chr_a]), _lib.PGT_EARG, "2 ... 8 files"),
        (lambda: pgt.align_segments([chr_a] * 9), _lib.PGT_EARG, "2 ... 8 files"),
        (lambda: pgt.align_segments_runs([[0, 1], [0]], [[1], [1]]), _lib.PGT_EARG, "file 0: 2 chromosome ids for 1 run lengths"),
        (lambda: pgt.align_segments([np.array([0, 1, 0]), np.array([0, 1])]), _lib.PGT_EDOMAIN, "chromosome id 0 has two runs"),
        (lambda: pgt.align_segments([np.array([0, 1]), np.array([1, 0])]), _lib.PGT_EDOMAIN, "chromosome id 1"),
        (lambda: pgt.align_sites([chr_a], [pos_a], [[f8]]), _lib.PGT_EARG, "2 ... 8 files"),
        (lambda: pgt.align_sites([chr_a, chr_a], [pos_a, pos_a], [[f8]]), _lib.PGT_EARG, "2 ... 8 files"),
        (lambda: pgt.align_sites([chr_a, chr_a[:4]], [pos_a, pos_a], [[f8], [f8]]), _lib.PGT_EARG, "file 1: 4 chromosome ids for 5 positions"),
        (lambda: pgt.align_sites([chr_a, chr_a], [pos_a, pos_a], [[f8, i4[:3]], [f8]]), _lib.PGT_EARG, "file 0: column 1 has 3 rows"),
        (lambda: pgt.align_sites([chr_a, chr_a], [pos_a, pos_a], [[f8], [i4.astype(np.int8)]]), _lib.PGT_EARG, "file 1: column 0: elements of 4 or 8 bytes"),
        (lambda: pgt.align_sites([np.array([0, 1, 0, 0, 0]), chr_a], [pos_a, pos_a], [[f8], [f8]]), _lib.PGT_EDOMAIN, "two runs"),
    ]
    for fn, code, text in cases:
        with pytest.raises(_lib.PgtError) as e:
            fn()
        assert e.value.code == code and text in str(e.value), str(e.value)


def test_align_segments_python_result():
    import popgenomicstools_amd as pgt
    segs, chr_of = pgt.align_segments([np.array([4, 4, 9, 9, 9, 2]), np.array([9, 9, 7, 2, 2])])
    assert segs.shape == (2, 2) and chr_of.tolist() == [9, 2]
    assert segs["off"].tolist() == [[2, 0], [5, 3]] and segs["len"].tolist() == [[3, 2], [1, 2]]
