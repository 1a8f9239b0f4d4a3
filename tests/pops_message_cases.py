"""The refused calls of the K-population entry points (dxy, fst and pi from per-population (freq, nInd) columns) whose return code
and FULL message tests/golden/pops_messages.json pins.  One list, issued twice: by tests/golden/make_pops_messages.py on the
commit the fixture is recorded from, and by tests/test_pops_messages*.py on the tree under test.

Every case is (key, thunk); a thunk returns [code, message].  A call through the C ABI gives its return code and
pgt_last_error (""  where it returns PGT_OK: the stale message of the call before says nothing); a call through the Python
wrappers gives PgtError.code and str(PgtError).  Shapes are those of the statistics' own refusal tests: 10 000 sites, K = 3, site
windows W = 1000 / S = 500 — the byte counts in the tree_bytes / out_bytes messages are functions of these alone."""
import ctypes as C

import numpy as np

from popgenomicstools_amd import _lib
from popgenomicstools_amd._lib import DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, FST_ROW_DTYPE, FST_TOTAL_DTYPE

STATS = ("dxy", "fst", "pi")
N, K, W, S, MININD = 10_000, 3, 1000, 500, 5
ROW = {"dxy": DXY_ROW_DTYPE, "fst": FST_ROW_DTYPE, "pi": DXY_ROW_DTYPE}
TOT = {"dxy": DXY_TOTAL_DTYPE, "fst": FST_TOTAL_DTYPE, "pi": DXY_TOTAL_DTYPE}
MIN_POPS = {"dxy": 2, "fst": 2, "pi": 1}


def tables(stat, k):
    return k if stat == "pi" else k * (k - 1) // 2


def _raised(fn):
    try:
        fn()
    except _lib.PgtError as e:
        return [e.code, str(e)]
    return [_lib.PGT_OK, ""]


def columns(n=N, k=K):
    """pos, K frequency and K count columns: the values play no part in a refusal"""
    pos = np.arange(1, n + 1, dtype=np.uint32)
    f = [np.full(n, 0.125 * (p + 1)) for p in range(k)]
    c = [np.full(n, 9, np.int32) for _ in range(k)]
    return pos, f, c


# ---- before a context is opened: no GPU --------------------------------------------------------------------------------------
def cpu_cases():
    import popgenomicstools_amd as pgt
    chr_ids = np.zeros(10, np.uint32)
    pos, f, c = columns(10, 3)
    window_args = [
        ("minind=0", dict(W=5, S=1, minind=0, fixedsite=1)),
        ("S=0,W>0", dict(W=5, S=0, minind=1, fixedsite=1)),
        ("no size file", dict(W=5, S=1, minind=1, fixedsite=0)),
        ("W=0 without fixedsite", dict(W=0, S=0, minind=1, fixedsite=0, chr_len=np.array([100], np.uint32))),
    ]
    ok = dict(W=5, S=1, minind=1, fixedsite=1)
    cases = []
    for what, kw in window_args:
        cases.append((f"dxy_window: {what}", lambda kw=kw: _raised(lambda: pgt.dxy_window(chr_ids, pos, f[0], f[1], c[0], c[1], **kw))))
    for stat in STATS:
        fn = getattr(pgt, f"{stat}_window_pops")
        for what, kw in window_args:
            cases.append((f"{stat}_window_pops: {what}", lambda fn=fn, kw=kw: _raised(lambda: fn(chr_ids, pos, f, c, **kw))))
        nine = (f * 3, c * 3)
        few = (f[: MIN_POPS[stat] - 1], c[: MIN_POPS[stat] - 1])
        for what, (ff, cc) in (("too few populations", few), ("9 populations", nine), ("one count column short", (f, c[:2]))):
            cases.append((f"{stat}_window_pops: {what}", lambda fn=fn, ff=ff, cc=cc: _raised(lambda: fn(chr_ids, pos, ff, cc, **ok))))
    return cases


def _wrapper_cases(pgt, ctx, stat, dev):
    """The refusals of Context.<stat>_pops_reduce_dev (a function of its own: every thunk keeps THIS statistic's tensors)."""
    import torch
    from popgenomicstools_amd.window_scan import windows_to_device
    wrap = getattr(ctx, f"{stat}_pops_reduce_dev")
    m = 1000
    fcols = [torch.zeros(m + 4, dtype=torch.float64, device=dev) for _ in range(3)]
    ccols = [torch.ones(m + 4, dtype=torch.int32, device=dev) for _ in range(3)]
    posm = torch.arange(1, m + 1, dtype=torch.int32, device=dev)
    w1 = windows_to_device(pgt.build_windows_sites(np.array([m], np.uint64), 100, 100), dev)
    good_f, good_c = [x[4:4 + m] for x in fcols], [x[4:4 + m] for x in ccols]
    lo = MIN_POPS[stat] - 1
    small = torch.zeros(tables(stat, 3) * 10 * ROW[stat].itemsize - 1, dtype=torch.uint8, device=dev)  # 10 windows of 100 sites: one byte short
    wrapped = [
        ("too few populations", lambda: wrap(posm, good_f[:lo], good_c[:lo], 1, w1)),
        ("9 populations", lambda: wrap(posm, good_f * 3, good_c * 3, 1, w1)),
        ("one count column short", lambda: wrap(posm, good_f, good_c[:2], 1, w1)),
        ("freqs[1] misaligned", lambda: wrap(posm, [good_f[0], fcols[1][1:1 + m], good_f[2]], good_c, 1, w1)),
        ("ninds[2] misaligned", lambda: wrap(posm, good_f, [good_c[0], good_c[1], ccols[2][2:2 + m]], 1, w1)),
        ("lengths differ", lambda: wrap(posm, [good_f[0], good_f[1][:-4], good_f[2]], good_c, 1, w1)),
        ("out too small", lambda: wrap(posm, good_f, good_c, 1, w1, out=small)),
    ]
    if stat != "dxy":
        wrapped.append(("minind=0", lambda: wrap(posm, good_f, good_c, 0, w1)))
    return [(f"Context.{stat}_pops_reduce_dev: {what}", lambda fn=fn: _raised(fn)) for what, fn in wrapped]


# ---- with a context: the C ABI's device and host forms, the Python device wrappers ------------------------------------------------
def gpu_cases(pgt, ctx):
    import torch
    from popgenomicstools_amd.window_scan import windows_to_device
    dev = torch.device("cuda", ctx.device)
    lib, h = ctx._lib, ctx._ctx
    pos, f, c = columns()
    win = pgt.build_windows_sites(np.array([N], np.uint64), W, S)
    wd = windows_to_device(win, dev)
    tp = torch.from_numpy(pos.view(np.int32)).to(dev)
    tf, tn = [torch.from_numpy(x).to(dev) for x in f], [torch.from_numpy(x).to(dev) for x in c]
    f_ptrs, n_ptrs = [t.data_ptr() for t in tf], [t.data_ptr() for t in tn]
    keep = [wd, tp, tf, tn, pos, f, c, win]  # what the thunks' raw pointers point into
    cases = []

    def c_call(fn, *args):
        rc = fn(*args)
        return [rc, _lib.last_error(h) if rc != _lib.PGT_OK else ""]

    for stat in STATS:
        row, t = ROW[stat].itemsize, tables(stat, K)
        tb = int(getattr(ctx, f"{stat}_pops_tree_bytes")(K, N))
        tree = torch.zeros(tb, dtype=torch.uint8, device=dev)
        out = torch.zeros(t * win.size * row, dtype=torch.uint8, device=dev)
        tot = torch.zeros(t * TOT[stat].itemsize, dtype=torch.uint8, device=dev)
        keep += [tree, out, tot]
        dev_fn = getattr(lib, f"pgt_{stat}_pops_reduce_dev")
        host_fn = getattr(lib, f"pgt_{stat}_pops_reduce")

        def dev_call(dev_fn=dev_fn, tree=tree, out=out, tot=tot, freq=None, nind=None, n_pops=K, minind=MININD, win_p=wd.data_ptr(),
                     out_bytes=None, tree_p=-1, tree_bytes=None, freq_null=False, nind_null=False, pos_p=tp.data_ptr(),
                     take_out=True):
            fp = f_ptrs if freq is None else freq
            npn = n_ptrs if nind is None else nind
            pf = (C.c_void_p * 9)(*(fp + [None] * (9 - len(fp))))
            pn = (C.c_void_p * 9)(*(npn + [None] * (9 - len(npn))))
            return c_call(dev_fn, h, pos_p, None if freq_null else pf, None if nind_null else pn, n_pops, N, minind, win_p, win.size,
                          out.data_ptr() if take_out else None, out.numel() if out_bytes is None else out_bytes, tot.data_ptr(),
                          tree.data_ptr() if tree_p == -1 else tree_p, tree.numel() if tree_bytes is None else tree_bytes, None)

        # the `refusals` list of test_{dxy,fst,pi}_pops.test_refusals_name_the_argument_and_launch_nothing
        refusals = []
        if stat != "dxy":
            refusals += [dict(minind=0), dict(minind=-3)]
        refusals += [dict(pos_p=None), dict(freq_null=True), dict(nind_null=True), dict(tree_p=None), dict(win_p=None), dict(take_out=False),
                     dict(n_pops=MIN_POPS[stat] - 1), dict(n_pops=9),
                     dict(freq=[f_ptrs[0], None, f_ptrs[2]]), dict(nind=[n_ptrs[0], n_ptrs[1], None]),
                     dict(freq=[f_ptrs[0], f_ptrs[1] + 8, f_ptrs[2]]), dict(nind=[n_ptrs[0], n_ptrs[1], n_ptrs[2] + 8]),
                     dict(nind=[n_ptrs[0] + 4, n_ptrs[1], n_ptrs[2]])]
        if stat == "pi":
            refusals += [dict(out_bytes=out.numel() - row)]
        refusals += [dict(out_bytes=out.numel() - 1), dict(tree_bytes=tb - 1)]
        names = {"pos_p": "pos", "freq_null": "freq", "nind_null": "nind", "tree_p": "tree", "win_p": "win", "take_out": "out"}
        for kw in refusals:
            (name, v), = kw.items()
            if name in names:
                what = f"{names[name]}=NULL"
            elif name in ("freq", "nind"):
                k = next(i for i, p in enumerate(v) if p is None or p % 16)
                what = f"{name}[{k}]=NULL" if v[k] is None else f"{name}[{k}] misaligned by {v[k] % 16}"
            elif name in ("out_bytes", "tree_bytes"):
                what = f"{name} short by {(out.numel() if name == 'out_bytes' else tb) - v}"
            else:
                what = f"{name}={v}"
            cases.append((f"pgt_{stat}_pops_reduce_dev: {what}", lambda dev_call=dev_call, kw=kw: dev_call(**kw)))

        # the host-buffer form
        def host_call(host_fn=host_fn, stat=stat, n_pops=K, minind=MININD, freq_null=False, freq=None, win_null=False):
            fp = [x.ctypes.data for x in f] if freq is None else freq
            pf = (C.c_void_p * 9)(*(fp + [None] * (9 - len(fp))))
            pn = (C.c_void_p * 9)(*([x.ctypes.data for x in c] + [None] * (9 - K)))
            rows = np.zeros((9 * 8, win.size), dtype=ROW[stat])  # room for any table count a wrong n_pops could stand for
            totals = np.zeros(9 * 8, dtype=TOT[stat])
            return c_call(host_fn, h, pos.ctypes.data, None if freq_null else pf, pn, n_pops, N, minind,
                          None if win_null else win.ctypes.data, win.size, rows.ctypes.data, totals.ctypes.data)

        host = [(f"n_pops={MIN_POPS[stat] - 1}", dict(n_pops=MIN_POPS[stat] - 1)), ("n_pops=9", dict(n_pops=9)), ("minind=0", dict(minind=0)),
                ("freq=NULL", dict(freq_null=True)), ("freq[1]=NULL", dict(freq=[f[0].ctypes.data, None, f[2].ctypes.data])),
                ("win=NULL", dict(win_null=True))]
        for what, kw in host:
            cases.append((f"pgt_{stat}_pops_reduce: {what}", lambda host_call=host_call, kw=kw: host_call(**kw)))

        cases += _wrapper_cases(pgt, ctx, stat, dev)
    return cases, keep  # the caller holds `keep` until the last thunk has run


def run(cases):
    out = {}
    for key, thunk in cases:
        assert key not in out, key
        out[key] = thunk()
    return out
