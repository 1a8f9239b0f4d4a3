"""Host-side mirror of the reference's three window tools over in-memory columns.

Reference interface mirrored (file:line in the reference tree):
  fstWindow  <file> [W] [S]            fstWindow.cpp:37-67,109-155   -> fst_window(chr, pos, a, b, W, S)
  hetWindow  <file> [W] [S]            hetWindow.cpp:34-64,107-153   -> het_window(chr, pos, g, W, S)
  dxyWindow  -winsize -stepsize -minind -fixedsite -sizefile -skip_missing <maf1> <maf2>
                                       dxyWindow.cpp:63-139,253-436  -> dxy_window(...)
Argument meaning, defaults (W=S=1 for fst/het; W=S=0, minind=1, fixedsite=0, skip_missing=0 for
dxy) and error behaviour (an exception where the tool exits 255) follow those lines.

All arithmetic happens in libpgtwin.so on the GPU.  This file only shapes buffers: numpy for
host columns, torch tensors for device-resident columns (torch is plumbing here: allocation,
streams, torch.distributed; it never computes a statistic).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (DSTAT_JACK_DTYPE, DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, EXT_ROW_DTYPE, F3_JACK_DTYPE, F3_ROW_DTYPE, F3_TOTAL_DTYPE, F4_JACK_DTYPE, F4_ROW_DTYPE, F4_TOTAL_DTYPE, F4RATIO_JACK_DTYPE, F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE, FD_ROW_DTYPE, FD_TOTAL_DTYPE, FST_ROW_DTYPE, FST_TOTAL_DTYPE, HET_ROW_DTYPE, PBS_JACK_DTYPE, PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, PGT_EXT_IHS,
                   PGT_EXT_XP_MAX, PGT_EXT_XP_MIN, PGT_STAT_DXY, PGT_STAT_EXT, PGT_STAT_FST, PGT_STAT_HET,
                   SEG_DTYPE, SHARD_DTYPE, WIN_DTYPE, PgtError, check)


# ---------------------------------------------------------------------------------------------
# window tables (host, no GPU)
# ---------------------------------------------------------------------------------------------
def run_lengths(chr_ids) -> np.ndarray:
    """Lengths of the runs of equal adjacent chromosome ids (the reference compares adjacent
    names only, fstWindow.cpp:132)."""
    c = np.asarray(chr_ids)
    if c.size == 0:
        return np.zeros(0, dtype=np.uint64)
    cuts = np.flatnonzero(c[1:] != c[:-1]) + 1
    edges = np.concatenate(([0], cuts, [c.size]))
    return np.diff(edges).astype(np.uint64)


def build_windows_sites(run_len, W: int, S: int) -> np.ndarray:
    lib = _lib.load()
    rl = np.ascontiguousarray(run_len, dtype=np.uint64)
    n_out = C.c_size_t(0)
    check(lib.pgt_build_windows_sites(rl.ctypes.data, rl.size, W, S, None, 0, C.byref(n_out)))
    out = np.zeros(n_out.value, dtype=WIN_DTYPE)
    check(lib.pgt_build_windows_sites(rl.ctypes.data, rl.size, W, S, out.ctypes.data, out.size, C.byref(n_out)))
    return out


def build_windows_bp(pos, run_len, chr_len, W: int, S: int) -> np.ndarray:
    lib = _lib.load()
    p = np.ascontiguousarray(pos, dtype=np.uint32)
    rl = np.ascontiguousarray(run_len, dtype=np.uint64)
    cl = np.ascontiguousarray(chr_len, dtype=np.uint32)
    if cl.size != rl.size or int(rl.sum()) != p.size:
        raise PgtError(_lib.PGT_EARG, "build_windows_bp: run_len / chr_len / pos sizes disagree")
    n_out = C.c_size_t(0)
    check(lib.pgt_build_windows_bp(p.ctypes.data, rl.ctypes.data, cl.ctypes.data, rl.size, W, S, None, 0, C.byref(n_out)))
    out = np.zeros(n_out.value, dtype=WIN_DTYPE)
    check(lib.pgt_build_windows_bp(p.ctypes.data, rl.ctypes.data, cl.ctypes.data, rl.size, W, S,
                                   out.ctypes.data, out.size, C.byref(n_out)))
    return out


def build_windows_extreme(pos, run_len, chr_len, W: int) -> np.ndarray:
    """ihsWindow / xpehhWindow window table (ihsWindow.cpp:147-218); chr_len[r] = 0 or None where the
    chromosome length is not given."""
    lib = _lib.load()
    p = np.ascontiguousarray(pos, dtype=np.uint32)
    rl = np.ascontiguousarray(run_len, dtype=np.uint64)
    cl = None if chr_len is None else np.ascontiguousarray(chr_len, dtype=np.uint32)
    if int(rl.sum()) != p.size or (cl is not None and cl.size != rl.size):
        raise PgtError(_lib.PGT_EARG, "build_windows_extreme: run_len / chr_len / pos sizes disagree")
    n_out = C.c_size_t(0)
    clp = cl.ctypes.data if cl is not None else None
    check(lib.pgt_build_windows_extreme(p.ctypes.data, rl.ctypes.data, clp, rl.size, W, None, 0, C.byref(n_out)))
    out = np.zeros(n_out.value, dtype=WIN_DTYPE)
    check(lib.pgt_build_windows_extreme(p.ctypes.data, rl.ctypes.data, clp, rl.size, W, out.ctypes.data, out.size,
                                        C.byref(n_out)))
    return out


def plan_shards(win: np.ndarray, n_ranks: int) -> np.ndarray:
    lib = _lib.load()
    w = np.ascontiguousarray(win, dtype=WIN_DTYPE)
    out = np.zeros(n_ranks, dtype=SHARD_DTYPE)
    check(lib.pgt_plan_shards(w.ctypes.data if w.size else None, w.size, n_ranks, out.ctypes.data))
    return out


def table_hints(win: np.ndarray):
    """(longest window, typical window, typical step) of a whole host table, as the host-buffer entry points derive them
    while the hints are unset (pgt_table_hints); the step is 2^64-1 where the table has no typical positive step."""
    import ctypes as C
    lib = _lib.load()
    w = np.ascontiguousarray(win, dtype=WIN_DTYPE)
    m, t, s = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib.pgt_table_hints(w.ctypes.data if w.size else None, w.size, C.byref(m), C.byref(t), C.byref(s)))
    return m.value, t.value, s.value


# ---------------------------------------------------------------------------------------------
# raw device memory handed out by the library (pgt_rowbuf_*): quacks like the uint8 tensors the
# *_dev wrappers take (data_ptr / numel), so it can be passed as `out=`
# ---------------------------------------------------------------------------------------------
def _runs_of(chr_ids):
    """(ids, lengths) of the runs of equal adjacent chromosome ids of one file."""
    c = _host_col(chr_ids, np.uint32)
    rl = run_lengths(c)
    starts = np.concatenate(([0], np.cumsum(rl)[:-1])).astype(np.int64) if rl.size else np.zeros(0, np.int64)
    return np.ascontiguousarray(c[starts], dtype=np.uint32), rl


def align_segments_runs(run_chr_list, run_len_list):
    """pgt_align_segments over run tables (per file: the chromosome id and the length of every run) -> (segs, chr):
    segs[m, k] (SEG_DTYPE) = the rows of matched chromosome m in file k, chr[m] = its id; file 0's order.  PgtError
    (PGT_EDOMAIN) when a file lists an id in two runs or the matched chromosomes come in different orders.  No GPU."""
    k = len(run_chr_list)
    if len(run_len_list) != k or not 2 <= k <= 8:
        raise PgtError(_lib.PGT_EARG, "align_segments: 2 ... 8 files, one run table each")
    ids = [np.ascontiguousarray(c, dtype=np.uint32) for c in run_chr_list]
    lens = [np.ascontiguousarray(r, dtype=np.uint64) for r in run_len_list]
    for f in range(k):
        if ids[f].ndim != 1 or ids[f].shape != lens[f].shape:
            raise PgtError(_lib.PGT_EARG, f"align_segments: file {f}: {ids[f].size} chromosome ids for {lens[f].size} run lengths")
    lib = _lib.load()
    pc = (C.c_void_p * k)(*[a.ctypes.data for a in ids])
    pl = (C.c_void_p * k)(*[a.ctypes.data for a in lens])
    nr = (C.c_size_t * k)(*[a.size for a in ids])
    n_out = C.c_size_t(0)
    check(lib.pgt_align_segments(pc, pl, nr, k, None, 0, C.byref(n_out)))
    segs = np.zeros(n_out.value, dtype=SEG_DTYPE)
    check(lib.pgt_align_segments(pc, pl, nr, k, segs.ctypes.data, segs.size, C.byref(n_out)))
    segs = segs.reshape(-1, k)
    # the matched chromosomes: file 0's ids that every file has (ids are unique per file, or the call above has refused)
    others = [set(a.tolist()) for a in ids[1:]]
    chr_of = np.array([c for c in ids[0].tolist() if all(c in o for o in others)], dtype=np.uint32)
    assert chr_of.size == segs.shape[0]
    return segs, chr_of


def align_segments(chr_ids_per_file):
    """The segment plan of Context.sites_align from per-SITE chromosome ids (one array per file, as the chr_ids of
    dxy_window; equal names must carry equal ids in every file) -> (segs[n_chr, n_files], chr[n_chr])."""
    if not 2 <= len(chr_ids_per_file) <= 8:
        raise PgtError(_lib.PGT_EARG, "align_segments: 2 ... 8 files, one chromosome-id column each")
    runs = [_runs_of(c) for c in chr_ids_per_file]
    return align_segments_runs([r[0] for r in runs], [r[1] for r in runs])


class RowBuffer:
    def __init__(self, ptr: int, nbytes: int, owner=None):
        self._ptr, self._nbytes, self._owner = int(ptr), int(nbytes), owner  # owner keeps the mapping alive

    def data_ptr(self) -> int:
        return self._ptr

    def numel(self) -> int:
        return self._nbytes

    def view(self, offset: int, nbytes: int) -> "RowBuffer":
        if offset < 0 or nbytes < 0 or offset + nbytes > self._nbytes:
            raise PgtError(_lib.PGT_EARG, "RowBuffer.view outside the buffer")
        return RowBuffer(self._ptr + offset, nbytes, self._owner or self)


class DeviceColumn:
    """A typed column in device memory that the library owns (pgt_ingest_column): accepted by the *_dev
    wrappers wherever a CUDA tensor of that dtype is."""

    def __init__(self, ptr: int, numel: int, dtype, owner):
        self._ptr, self._numel, self.dtype, self._owner = int(ptr), int(numel), dtype, owner

    def data_ptr(self) -> int:
        return self._ptr

    def numel(self) -> int:
        return self._numel


class Ingest:
    """Result of Context.ingest_text: parsed columns on the GPU + chromosome runs on the host."""

    def __init__(self, ctx, handle, text: bytes, tokens):
        self._ctx, self._h, self._text, self.tokens = ctx, handle, text, list(tokens)
        lib = ctx._lib
        self.rows = int(lib.pgt_ingest_rows(handle))
        self.bad_line = int(lib.pgt_ingest_bad_line(handle))
        rl, off, ln = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        n = int(lib.pgt_ingest_runs(handle, C.byref(rl), C.byref(off), C.byref(ln)))
        arr = lambda p, t: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,)).copy() if n else np.zeros(0, dtype=t)  # noqa: E731
        self.run_len = arr(rl, C.c_uint64)
        offs, lens = arr(off, C.c_uint64), arr(ln, C.c_uint32)
        self.run_names = [text[int(o): int(o) + int(k)].decode("latin-1") for o, k in zip(offs, lens)]

    def column(self, token: int):
        """Device column of token `token` (DeviceColumn), as the *_dev wrappers take it."""
        import torch
        dt = {_lib.PGT_TOK_U32: torch.int32, _lib.PGT_TOK_I32: torch.int32, _lib.PGT_TOK_F64: torch.float64,
              _lib.PGT_TOK_FREQ: torch.float64, _lib.PGT_TOK_I8: torch.int8}[self.tokens[token]]
        return DeviceColumn(self._ctx._lib.pgt_ingest_column(self._h, token), self.rows, dt, self)

    def column_np(self, token: int) -> np.ndarray:
        """Host copy of a column (u32 / i32 / f64 / i8 by token kind)."""
        dt = {_lib.PGT_TOK_U32: np.uint32, _lib.PGT_TOK_I32: np.int32, _lib.PGT_TOK_F64: np.float64,
              _lib.PGT_TOK_FREQ: np.float64, _lib.PGT_TOK_I8: np.int8}[self.tokens[token]]
        ptr = self._ctx._lib.pgt_ingest_column(self._h, token)
        raw = self._ctx.rowbuf_read(RowBuffer(ptr, self.rows * np.dtype(dt).itemsize)) if self.rows else np.zeros(0, np.uint8)
        return raw.view(dt)

    def free(self):
        if self._h:
            self._ctx._lib.pgt_ingest_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WindowTable:
    """A site-window table built on the GPU (pgt_wintab_sites): `n_win` windows, `first[r]` = index of run r's
    first window (n_runs + 1 values), `device()` = the table as a uint8 view usable as `win` of the *_dev calls."""

    def __init__(self, ctx, handle, n_runs):
        self._ctx, self._h = ctx, handle
        lib = ctx._lib
        self.n_win = int(lib.pgt_wintab_size(handle))
        self.first = np.ctypeslib.as_array(C.cast(lib.pgt_wintab_first(handle), C.POINTER(C.c_uint64)), shape=(n_runs + 1,)).copy()

    def device(self):
        return RowBuffer(self._ctx._lib.pgt_wintab_device(self._h) or 0, self.n_win * WIN_DTYPE.itemsize, owner=self)

    def to_host(self) -> np.ndarray:
        raw = self._ctx.rowbuf_read(self.device()) if self.n_win else np.zeros(0, np.uint8)
        return raw.view(WIN_DTYPE)

    def labels(self) -> np.ndarray:
        """label_run of every window, from `first` alone"""
        return (np.searchsorted(self.first, np.arange(self.n_win, dtype=np.uint64), side="right") - 1).astype(np.uint32)

    def free(self):
        if self._h:
            self._ctx._lib.pgt_wintab_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------
# the K-population statistics over per-population (freq, nInd) columns: what is particular to each.  Their wrappers
# (Context._pops_reduce, Context._pops_reduce_dev, _window_pops) are one body per form.
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class _PopsStat:
    name: str          # pgt_<name>_pops_reduce / _reduce_dev / _tree_bytes; <name>_pops_reduce* and <name>_window_pops in messages
    min_pops: int      # min_pops ... max_pops populations
    per_pair: bool     # one row table per pair i < j (pair_order), else one per population
    row: np.dtype
    total: np.dtype
    max_pops: int = 8
    per_trio: bool = False  # one row table per ingroup trio i < j < k (trio_order); the last population is the outgroup
    all_trios: bool = False  # one row table per trio i < j < k of ALL populations (all_trio_order): no outgroup
    all_quartets: bool = False  # one row table per quartet i < j < k < l of ALL populations (all_quartet_order)
    middle_triples: bool = False  # one row table per triple i < j < k of the populations between the first and the last (middle_triple_order)

    def tables(self, n_pops: int) -> int:
        if self.middle_triples:
            return (n_pops - 2) * (n_pops - 3) * (n_pops - 4) // 6
        if self.all_quartets:
            return n_pops * (n_pops - 1) * (n_pops - 2) * (n_pops - 3) // 24
        if self.all_trios:
            return n_pops * (n_pops - 1) * (n_pops - 2) // 6
        if self.per_trio:
            return (n_pops - 1) * (n_pops - 2) * (n_pops - 3) // 6
        return n_pops * (n_pops - 1) // 2 if self.per_pair else n_pops

    def check_count(self, who: str, freqs, ninds):
        if len(ninds) != len(freqs) or not self.min_pops <= len(freqs) <= self.max_pops:
            raise PgtError(_lib.PGT_EARG, f"{who}: {self.min_pops} ... {self.max_pops} populations, one frequency and one count column each")


_DXY_POPS = _PopsStat("dxy", 2, True, DXY_ROW_DTYPE, DXY_TOTAL_DTYPE)
_FST_POPS = _PopsStat("fst", 2, True, FST_ROW_DTYPE, FST_TOTAL_DTYPE)
_PI_POPS = _PopsStat("pi", 1, False, DXY_ROW_DTYPE, DXY_TOTAL_DTYPE)
_FST_HUDSON_POPS = _PopsStat("fst_hudson", 2, True, FST_ROW_DTYPE, FST_TOTAL_DTYPE)
_DSTAT_POPS = _PopsStat("dstat", 4, False, DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, max_pops=7, per_trio=True)
_FD_POPS = _PopsStat("fd", 4, False, FD_ROW_DTYPE, FD_TOTAL_DTYPE, max_pops=7, per_trio=True)
_F3_POPS = _PopsStat("f3", 3, False, F3_ROW_DTYPE, F3_TOTAL_DTYPE, max_pops=6, all_trios=True)
_F4_POPS = _PopsStat("f4", 4, False, F4_ROW_DTYPE, F4_TOTAL_DTYPE, max_pops=6, all_quartets=True)
_F4RATIO_POPS = _PopsStat("f4ratio", 5, False, F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE, max_pops=7, middle_triples=True)
_PBS_POPS = _PopsStat("pbs", 3, False, PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, max_pops=6, all_trios=True)
_PBS_HUDSON_POPS = _PopsStat("pbs_hudson", 3, False, PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, max_pops=6, all_trios=True)
_PBS_ESTIMATORS = {"wc": _PBS_POPS, "hudson": _PBS_HUDSON_POPS}  # pbs_window_pops(estimator=...), Context.pbs_pops_reduce*(estimator=...)
_FST_ESTIMATORS = {"wc": _FST_POPS, "hudson": _FST_HUDSON_POPS}  # fst_window_pops(estimator=...)


# ---------------------------------------------------------------------------------------------
# context
# ---------------------------------------------------------------------------------------------
class Context:
    """One GPU, one thread (include/pgtwin.h conventions).  Raises PgtError if no gfx950 device
    is usable: there is no CPU path."""

    def __init__(self, device: int = -1):
        self._lib = _lib.load()
        self._ctx = self._lib.pgt_open(device)
        if not self._ctx:
            raise PgtError(_lib.PGT_EDEVICE, _lib.last_error(None))
        if device < 0:  # "the current device": ask the runtime which one that was
            import torch
            device = torch.cuda.current_device()
        self.device = int(device)

    def close(self):
        if self._ctx:
            self._lib.pgt_close(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        check(rc, self._ctx)

    # ---- host buffers ------------------------------------------------------------------
    def prepare_host_io(self, expected_column_bytes: int = 0):
        """pgt_prepare_host_io: allocate the pinned staging ring of the host-buffer calls below (unless the expected upload is
        under 32 MiB; 0 = unknown) and make the runtime set up its first copies NOW (30 … 90 ms once per process) — worth
        calling from a thread that opens the device beside a long parse."""
        self._check(self._lib.pgt_prepare_host_io(self._ctx, int(expected_column_bytes)))

    def fst_reduce(self, pos, a, b, win) -> np.ndarray:
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        win = np.ascontiguousarray(win, dtype=WIN_DTYPE)
        if not (pos.size == a.size == b.size):
            raise PgtError(_lib.PGT_EARG, "fst_reduce: column lengths differ")
        out = np.zeros(win.size, dtype=FST_ROW_DTYPE)
        self._check(self._lib.pgt_fst_reduce(self._ctx, pos.ctypes.data, a.ctypes.data, b.ctypes.data, pos.size,
                                             win.ctypes.data, win.size, out.ctypes.data))
        return out

    def het_reduce(self, pos, g, win) -> np.ndarray:
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        g = np.ascontiguousarray(g, dtype=np.int8)
        win = np.ascontiguousarray(win, dtype=WIN_DTYPE)
        if pos.size != g.size:
            raise PgtError(_lib.PGT_EARG, "het_reduce: column lengths differ")
        out = np.zeros(win.size, dtype=HET_ROW_DTYPE)
        self._check(self._lib.pgt_het_reduce(self._ctx, pos.ctypes.data, g.ctypes.data, pos.size,
                                             win.ctypes.data, win.size, out.ctypes.data))
        return out

    def extreme_reduce(self, pos, score, mode, cutoff, win) -> np.ndarray:
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        score = np.ascontiguousarray(score, dtype=np.float64)
        win = np.ascontiguousarray(win, dtype=WIN_DTYPE)
        if pos.size != score.size:
            raise PgtError(_lib.PGT_EARG, "extreme_reduce: column lengths differ")
        out = np.zeros(win.size, dtype=EXT_ROW_DTYPE)
        self._check(self._lib.pgt_extreme_reduce(self._ctx, pos.ctypes.data, score.ctypes.data, pos.size, int(mode),
                                                 float(cutoff), win.ctypes.data, win.size, out.ctypes.data))
        return out

    def dxy_reduce(self, pos, p1, p2, n1, n2, minind, win):
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        p2 = np.ascontiguousarray(p2, dtype=np.float64)
        n1 = np.ascontiguousarray(n1, dtype=np.int32)
        n2 = np.ascontiguousarray(n2, dtype=np.int32)
        win = np.ascontiguousarray(win, dtype=WIN_DTYPE)
        if not (pos.size == p1.size == p2.size == n1.size == n2.size):
            raise PgtError(_lib.PGT_EARG, "dxy_reduce: column lengths differ")
        out = np.zeros(win.size, dtype=DXY_ROW_DTYPE)
        tot = np.zeros(1, dtype=DXY_TOTAL_DTYPE)
        self._check(self._lib.pgt_dxy_reduce(self._ctx, pos.ctypes.data, p1.ctypes.data, p2.ctypes.data,
                                             n1.ctypes.data, n2.ctypes.data, pos.size, int(minind),
                                             win.ctypes.data, win.size, out.ctypes.data, tot.ctypes.data))
        return out, tot[0]

    def _pops_reduce(self, st: _PopsStat, pos, freqs, ninds, minind, win):
        """The numpy form of a K-population statistic (pgt_<name>_pops_reduce) -> (rows[tables, n_win], totals[tables])."""
        who = f"{st.name}_pops_reduce"
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        freqs = [np.ascontiguousarray(f, dtype=np.float64) for f in freqs]
        ninds = [np.ascontiguousarray(k, dtype=np.int32) for k in ninds]
        win = np.ascontiguousarray(win, dtype=WIN_DTYPE)
        n_pops = len(freqs)
        st.check_count(who, freqs, ninds)
        if any(c.size != pos.size for c in freqs + ninds):
            raise PgtError(_lib.PGT_EARG, f"{who}: column lengths differ")
        out = np.zeros((st.tables(n_pops), win.size), dtype=st.row)
        tot = np.zeros(st.tables(n_pops), dtype=st.total)
        pf = (C.c_void_p * n_pops)(*[f.ctypes.data for f in freqs])
        pn = (C.c_void_p * n_pops)(*[k.ctypes.data for k in ninds])
        self._check(getattr(self._lib, f"pgt_{who}")(self._ctx, pos.ctypes.data, pf, pn, n_pops, pos.size, int(minind),
                                                     win.ctypes.data, win.size, out.ctypes.data, tot.ctypes.data))
        return out, tot

    def dxy_pops_reduce(self, pos, freqs, ninds, minind, win):
        """dxy rows of ALL pairs i<j of len(freqs) populations (pair_order) from per-population numpy columns, one pass:
        -> (rows[n_pairs, n_win], totals[n_pairs]) (pgt_dxy_pops_reduce)."""
        return self._pops_reduce(_DXY_POPS, pos, freqs, ninds, minind, win)

    def fst_pops_reduce(self, pos, freqs, ninds, minind, win):
        """FST rows of ALL pairs i<j of len(freqs) populations (pair_order) from per-population numpy (freq, nInd) columns, one
        pass: -> (rows[n_pairs, n_win], totals[n_pairs]) (pgt_fst_pops_reduce).  A row's n is the number of counted sites."""
        return self._pops_reduce(_FST_POPS, pos, freqs, ninds, minind, win)

    def fst_hudson_pops_reduce(self, pos, freqs, ninds, minind, win):
        """fst_pops_reduce with Hudson's estimator as a ratio of averages (pgt_fst_hudson_pops_reduce): a row's asum is
        Σ [(p1-p2)² - h1 - h2], h = p(1-p)/(2n-1), its bsum Σ dxy over the pair's counted sites, fst their ratio."""
        return self._pops_reduce(_FST_HUDSON_POPS, pos, freqs, ninds, minind, win)

    def pi_pops_reduce(self, pos, freqs, ninds, minind, win):
        """Nucleotide-diversity (pi) rows of EACH of len(freqs) populations (1 ... 8) from per-population numpy (freq, nInd)
        columns, one pass: -> (rows[n_pops, n_win], totals[n_pops]) (pgt_pi_pops_reduce).  A row's sum is Σ 2p(1-p) 2n/(2n-1) over
        its counted sites (nInd >= minind); divide by neff or by the window length."""
        return self._pops_reduce(_PI_POPS, pos, freqs, ninds, minind, win)

    def dstat_pops_reduce(self, pos, freqs, ninds, minind, win):
        """ABBA-BABA rows of ALL trios i<j<k of the first len(freqs) - 1 populations (trio_order) against the LAST one, the
        outgroup, from 4 ... 7 per-population numpy (freq, nInd) columns, one pass: -> (rows[n_trios, n_win], totals[n_trios])
        (pgt_dstat_pops_reduce).  A row carries Σbbaa, Σabba, Σbaba over its counted sites, their number n and Patterson's
        d = (abba - baba) / (abba + baba) for the topology ((i,j),k)."""
        return self._pops_reduce(_DSTAT_POPS, pos, freqs, ninds, minind, win)

    def fd_pops_reduce(self, pos, freqs, ninds, minind, win):
        """f_d / f_dM rows of ALL trios i<j<k of the first len(freqs) - 1 populations (trio_order), read as ((P1 = i, P2 = j),
        P3 = k), against the LAST one, the outgroup, from 4 ... 7 per-population numpy (freq, nInd) columns, one pass:
        -> (rows[n_trios, n_win], totals[n_trios]) (pgt_fd_pops_reduce).  A row carries Σnum, Σfd_den, Σfdm_den over its counted
        sites, their number n, fd = num / fd_den and fdm = num / fdm_den (0 where the denominator is 0)."""
        return self._pops_reduce(_FD_POPS, pos, freqs, ninds, minind, win)

    def f3_pops_reduce(self, pos, freqs, ninds, minind, win):
        """f3 rows of ALL trios i<j<k of len(freqs) populations (all_trio_order; no outgroup), every population of a trio as
        the target, from 3 ... 6 per-population numpy (freq, nInd) columns, one pass: -> (rows[n_trios, n_win], totals[n_trios])
        (pgt_f3_pops_reduce).  A row carries the three SUMS f3_i, f3_j, f3_k over its counted sites (target_order) and their
        number n; f3 of the window is sum / n."""
        return self._pops_reduce(_F3_POPS, pos, freqs, ninds, minind, win)

    def pbs_pops_reduce(self, pos, freqs, ninds, minind, win, estimator="wc"):
        """Population-branch-statistic rows of ALL trios i<j<k of len(freqs) populations (all_trio_order), every population of a
        trio as the focal one, from 3 ... 6 per-population numpy (freq, nInd) columns: -> (rows[n_trios, n_win], totals[n_trios])
        (pgt_pbs_pops_reduce; estimator="hudson": pgt_pbs_hudson_pops_reduce).  A row carries pbs_i, pbs_j, pbs_k, the six SUMS
        num_xy / den_xy of the trio's pairs over the sites counted for the whole trio, and their number n; fst_xy = num_xy / den_xy.
        Nothing is clamped: inf and nan are the IEEE results of FST = 1."""
        return self._pops_reduce(_pbs_estimator("pbs_pops_reduce", estimator), pos, freqs, ninds, minind, win)

    def f4_pops_reduce(self, pos, freqs, ninds, minind, win):
        """f4 rows of ALL quartets i<j<k<l of len(freqs) populations (all_quartet_order; no outgroup), every quartet in its three
        pairings, from 4 ... 6 per-population numpy (freq, nInd) columns, one pass: -> (rows[n_quartets, n_win], totals[n_quartets])
        (pgt_f4_pops_reduce).  A row carries the three SUMS f4_ij_kl, f4_ik_jl, f4_il_jk over its counted sites (pairing_order)
        and their number n; f4 of the window is sum / n."""
        return self._pops_reduce(_F4_POPS, pos, freqs, ninds, minind, win)

    def _jackknife(self, name: str, row: np.dtype, jack: np.dtype, rows, items: int = 3) -> np.ndarray:
        """The numpy form of a block jackknife (pgt_<name>_jackknife) -> [n_trios, items] of `jack`."""
        rows = np.ascontiguousarray(rows, dtype=row)
        if rows.ndim != 2:
            raise PgtError(_lib.PGT_EARG, f"{name}_jackknife: rows must be a [n_trios, n_win] table")
        n_trios, n_win = rows.shape
        out = np.zeros((n_trios, items), dtype=jack)
        self._check(getattr(self._lib, f"pgt_{name}_jackknife")(self._ctx, rows.ctypes.data if rows.size else None, n_win, n_trios, out.ctypes.data))
        return out

    def dstat_jackknife(self, rows) -> np.ndarray:
        """Block-jackknife D, standard error and Z of every trio and topology from a [n_trios, n_win] numpy table of
        DSTAT_ROW_DTYPE rows (what dstat_pops_reduce returns) over DISJOINT windows: every window is a block, used when its
        n > 0 and weighted by it (pgt_dstat_jackknife) -> [n_trios, 3] DSTAT_JACK_DTYPE, the topologies in topology_order."""
        return self._jackknife("dstat", DSTAT_ROW_DTYPE, DSTAT_JACK_DTYPE, rows)

    def f3_jackknife(self, rows) -> np.ndarray:
        """Block-jackknife f3 (the mean over the used blocks' sites), standard error and Z of every trio and target from a
        [n_trios, n_win] numpy table of F3_ROW_DTYPE rows (what f3_pops_reduce returns) over DISJOINT windows
        (pgt_f3_jackknife) -> [n_trios, 3] F3_JACK_DTYPE, the targets in target_order."""
        return self._jackknife("f3", F3_ROW_DTYPE, F3_JACK_DTYPE, rows)

    def f4_jackknife(self, rows) -> np.ndarray:
        """Block-jackknife f4 (the mean over the used blocks' sites), standard error and Z of every quartet and pairing from a
        [n_quartets, n_win] numpy table of F4_ROW_DTYPE rows (what f4_pops_reduce returns) over DISJOINT windows
        (pgt_f4_jackknife) -> [n_quartets, 3] F4_JACK_DTYPE, the pairings in pairing_order."""
        return self._jackknife("f4", F4_ROW_DTYPE, F4_JACK_DTYPE, rows)

    def f4ratio_pops_reduce(self, pos, freqs, ninds, minind, win):
        """The f4-ratio sums of ALL triples i<j<k of the middle populations 1 ... len(freqs) - 2 (middle_triple_order), between
        population 0 (A) and the last one (the outgroup O), from 5 ... 7 per-population numpy (freq, nInd) columns, one pass:
        -> (rows[n_triples, n_win], totals[n_triples]) (pgt_f4ratio_pops_reduce).  A row carries the three SUMS g_ij, g_ik, g_jk of
        (p_A - p_O)(p_x - p_y) over the sites where all FIVE populations have minind individuals, and their number n; the six
        admixture proportions of ratio_order(i, j, k) are ratios of two of them (f4ratio_alphas)."""
        return self._pops_reduce(_F4RATIO_POPS, pos, freqs, ninds, minind, win)

    def f4ratio_jackknife(self, rows) -> np.ndarray:
        """Block-jackknife admixture proportion (the ratio of two sums over the used blocks, both losing a block together),
        standard error and Z of every middle triple and each of its six (B, X, C) from a [n_triples, n_win] numpy table of
        F4RATIO_ROW_DTYPE rows (what f4ratio_pops_reduce returns) over DISJOINT windows (pgt_f4ratio_jackknife)
        -> [n_triples, 6] F4RATIO_JACK_DTYPE, in ratio_order."""
        return self._jackknife("f4ratio", F4RATIO_ROW_DTYPE, F4RATIO_JACK_DTYPE, rows, items=6)

    def pbs_jackknife(self, rows) -> np.ndarray:
        """Block-jackknife PBS and PBSn1 (the branch statistic of the six sums over the used blocks, each sum losing a block with
        one rounding), standard error and Z of every trio and focal population from a [n_trios, n_win] numpy table of
        PBS_ROW_DTYPE rows (what pbs_pops_reduce returns, either estimator) over DISJOINT windows (pgt_pbs_jackknife)
        -> [n_trios, 6] PBS_JACK_DTYPE, in pbs_item_order."""
        return self._jackknife("pbs", PBS_ROW_DTYPE, PBS_JACK_DTYPE, rows, items=6)

    # ---- device-resident columns (torch CUDA tensors) -------------------------------------
    @staticmethod
    def _stream(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    @staticmethod
    def tree_bytes(stat: int, n_sites: int) -> int:
        return int(_lib.load().pgt_tree_bytes(stat, n_sites))

    def _dev(self, t, dtype, name):
        import torch
        if isinstance(t, RowBuffer) and dtype == torch.uint8:
            return t.data_ptr()
        if isinstance(t, DeviceColumn) and t.dtype == dtype:
            return t.data_ptr() if t.numel() else None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype):
            raise PgtError(_lib.PGT_EARG, f"{name}: expected a contiguous CUDA tensor of {dtype}")
        if t.device.index != self.device:  # the kernels run on the context's GPU: memory of another one may not even be mapped there
            raise PgtError(_lib.PGT_EARG, f"{name}: tensor lives on cuda:{t.device.index}, the context on cuda:{self.device}")
        return t.data_ptr() if t.numel() else None  # an empty shard passes NULL columns (n == 0)

    def _col(self, t, dtype, name):
        """A COLUMN the build kernels stream: as _dev, plus the alignment the C ABI demands (16 bytes: every column is read
        by 16-byte loads; ABI 5 extended that to the i32 count columns).  A view that starts at an odd site offset is
        refused HERE, by name, with the offsets that work — the library's own message cannot name the tensor."""
        ptr = self._dev(t, dtype, name)
        if ptr is not None and ptr % 16:
            import torch
            per = 16 // torch.empty(0, dtype=dtype).element_size()
            raise PgtError(_lib.PGT_EARG, f"{name}: column starts {ptr % 16} bytes past a 16-byte boundary; slice columns at site offsets "
                                          f"that are multiples of {per} for {dtype} (or .clone() the view)")
        return ptr

    @staticmethod
    def _same_len(name, n, *cols):
        """The C ABI takes one n for all columns: a short column would be read out of bounds."""
        for c in cols:
            if c.numel() != n:
                raise PgtError(_lib.PGT_EARG, f"{name}: column lengths differ ({c.numel()} vs {n})")

    @staticmethod
    def _room(name, buf, need_bytes):
        """Early, readable refusal; the C ABI (version 4) checks the same capacities again before any launch."""
        if buf.numel() < need_bytes:
            raise PgtError(_lib.PGT_EARG, f"{name}: buffer holds {buf.numel()} bytes, {need_bytes} needed")

    # ---- device-side text ingest (pgt_ingest_*) ---------------------------------------------
    def ingest_text(self, text: bytes, tokens) -> Ingest:
        """Parse whitespace-separated text lines on the GPU.  tokens: PGT_TOK_* per column, the first being
        PGT_TOK_CHR (e.g. fstWindow: [CHR, U32, F64, F64]).  Raises PgtError(PGT_EDOMAIN) when the input
        has too many irregular lines for the device path."""
        toks = (C.c_uint8 * len(tokens))(*tokens)
        h = C.c_void_p(0)
        text = bytes(text)
        self._check(self._lib.pgt_ingest_text(self._ctx, text if text else None, len(text), toks, len(tokens), C.byref(h)))
        return Ingest(self, h, text, tokens)

    # ---- window tables built on the device (pgt_wintab_*) -----------------------------------
    def window_table_sites(self, run_len, W: int, S: int) -> WindowTable:
        run_len = np.ascontiguousarray(run_len, dtype=np.uint64)
        h = C.c_void_p(0)
        self._check(self._lib.pgt_wintab_sites(self._ctx, run_len.ctypes.data, run_len.size, int(W), int(S), C.byref(h)))
        return WindowTable(self, h, run_len.size)

    def fst_reduce_tab(self, pos, a, b, tab: WindowTable) -> np.ndarray:
        """Host columns + a device window table -> host rows (pgt_fst_reduce_tab)."""
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        if not (pos.size == a.size == b.size):
            raise PgtError(_lib.PGT_EARG, "fst_reduce_tab: column lengths differ")
        out = np.zeros(tab.n_win, dtype=FST_ROW_DTYPE)
        self._check(self._lib.pgt_fst_reduce_tab(self._ctx, pos.ctypes.data, a.ctypes.data, b.ctypes.data, pos.size, 0, tab._h,
                                                 out.ctypes.data, out.nbytes))
        return out

    def het_reduce_tab(self, pos, g, tab: WindowTable) -> np.ndarray:
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        g = np.ascontiguousarray(g, dtype=np.int8)
        if pos.size != g.size:
            raise PgtError(_lib.PGT_EARG, "het_reduce_tab: column lengths differ")
        out = np.zeros(tab.n_win, dtype=HET_ROW_DTYPE)
        self._check(self._lib.pgt_het_reduce_tab(self._ctx, pos.ctypes.data, g.ctypes.data, pos.size, 0, tab._h, out.ctypes.data,
                                                 out.nbytes))
        return out

    def dxy_reduce_tab(self, pos, p1, p2, n1, n2, minind, tab: WindowTable):
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        p2 = np.ascontiguousarray(p2, dtype=np.float64)
        n1 = np.ascontiguousarray(n1, dtype=np.int32)
        n2 = np.ascontiguousarray(n2, dtype=np.int32)
        if not (pos.size == p1.size == p2.size == n1.size == n2.size):
            raise PgtError(_lib.PGT_EARG, "dxy_reduce_tab: column lengths differ")
        out = np.zeros(tab.n_win, dtype=DXY_ROW_DTYPE)
        tot = np.zeros(1, dtype=DXY_TOTAL_DTYPE)
        self._check(self._lib.pgt_dxy_reduce_tab(self._ctx, pos.ctypes.data, p1.ctypes.data, p2.ctypes.data, n1.ctypes.data,
                                                 n2.ctypes.data, pos.size, int(minind), 0, tab._h, out.ctypes.data, out.nbytes,
                                                 tot.ctypes.data))
        return out, tot[0]

    # ---- multi-GPU row buffer (pgt_rowbuf_*) ------------------------------------------------
    def rowbuf_create(self, nbytes: int):
        """-> (RowBuffer on this GPU, 64-byte IPC handle to ship to the other ranks)."""
        ptr = C.c_void_p(0)
        handle = (C.c_ubyte * 64)()
        self._check(self._lib.pgt_rowbuf_create(self._ctx, int(nbytes), C.byref(ptr), handle))
        return RowBuffer(ptr.value, nbytes), bytes(handle)

    def peer_access(self, peer_device: int):
        """Raises PgtError unless this context's GPU can address memory of HIP device `peer_device`."""
        self._check(self._lib.pgt_peer_access(self._ctx, int(peer_device)))

    def rowbuf_open(self, handle: bytes, nbytes: int) -> RowBuffer:
        ptr = C.c_void_p(0)
        h = (C.c_ubyte * 64).from_buffer_copy(handle)
        self._check(self._lib.pgt_rowbuf_open(self._ctx, h, C.byref(ptr)))
        return RowBuffer(ptr.value, nbytes)

    def rowbuf_close(self, buf: RowBuffer, owner: bool):
        self._check(self._lib.pgt_rowbuf_close(self._ctx, C.c_void_p(buf.data_ptr()), int(owner)))

    def rowbuf_fill(self, buf: RowBuffer, seed: int, stream=None):
        """Store the test pattern of pgt_rowbuf_fill through `buf` (asynchronous); pattern_words() is what must read back."""
        self._check(self._lib.pgt_rowbuf_fill(self._ctx, C.c_void_p(buf.data_ptr()), buf.numel() // 8 * 8, int(seed),
                                              self._stream(stream)))

    @staticmethod
    def pattern_words(n_words: int, seed: int) -> np.ndarray:
        """The words pgt_rowbuf_fill writes: splitmix64(seed + i)."""
        with np.errstate(over="ignore"):
            z = np.arange(n_words, dtype=np.uint64) + np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))

    def rowbuf_read(self, buf: RowBuffer, nbytes: int | None = None, stream=None) -> np.ndarray:
        nbytes = buf.numel() if nbytes is None else int(nbytes)
        host = np.empty(nbytes, dtype=np.uint8)
        self._check(self._lib.pgt_rowbuf_read(self._ctx, host.ctypes.data, C.c_void_p(buf.data_ptr()), nbytes,
                                              self._stream(stream)))
        return host

    def fst_reduce_dev(self, pos, a, b, win, out=None, tree=None, stream=None):
        """pos u32-as-int32 [n], a/b float64 [n], win uint8 [n_win*32] (WIN_DTYPE bytes) on the GPU.
        Returns (out uint8 [n_win*40], tree).  Asynchronous on `stream`."""
        import torch
        n = a.numel()
        n_win = win.numel() // WIN_DTYPE.itemsize
        tb = self.tree_bytes(PGT_STAT_FST, n)
        if tree is None:
            tree = torch.empty(tb, dtype=torch.uint8, device=a.device)
        if out is None:
            out = torch.empty(n_win * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=a.device)
        self._same_len("fst_reduce_dev", n, pos, a, b)
        self._room("fst_reduce_dev: out", out, n_win * FST_ROW_DTYPE.itemsize)
        self._room("fst_reduce_dev: tree", tree, tb)
        self._check(self._lib.pgt_fst_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), self._col(a, torch.float64, "a"),
            self._col(b, torch.float64, "b"), n, self._dev(win, torch.uint8, "win"), n_win,
            self._dev(out, torch.uint8, "out"), out.numel(), self._dev(tree, torch.uint8, "tree"), tree.numel(),
            self._stream(stream)))
        return out, tree

    def fst_reduce_pairs_dev(self, pos, a_list, b_list, win, out=None, tree=None, stream=None):
        import torch
        n = a_list[0].numel()
        n_pairs = len(a_list)
        n_win = win.numel() // WIN_DTYPE.itemsize
        tb = self.tree_bytes(PGT_STAT_FST, n) * n_pairs
        if tree is None:
            tree = torch.empty(tb, dtype=torch.uint8, device=pos.device)
        if out is None:
            out = torch.empty(n_pairs * n_win * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=pos.device)
        self._same_len("fst_reduce_pairs_dev", n, pos, *a_list, *b_list)
        self._room("fst_reduce_pairs_dev: out", out, n_pairs * n_win * FST_ROW_DTYPE.itemsize)
        self._room("fst_reduce_pairs_dev: tree", tree, tb)
        pa = (C.c_void_p * n_pairs)(*[self._col(t, torch.float64, "a") for t in a_list])
        pb = (C.c_void_p * n_pairs)(*[self._col(t, torch.float64, "b") for t in b_list])
        self._check(self._lib.pgt_fst_reduce_pairs_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), pa, pb, n_pairs, n,
            self._dev(win, torch.uint8, "win"), n_win, self._dev(out, torch.uint8, "out"), out.numel(),
            self._dev(tree, torch.uint8, "tree"), tree.numel(), self._stream(stream)))
        return out, tree

    def het_reduce_dev(self, pos, g, win, out=None, tree=None, stream=None):
        import torch
        n = g.numel()
        n_win = win.numel() // WIN_DTYPE.itemsize
        if tree is None:
            tree = torch.empty(self.tree_bytes(PGT_STAT_HET, n), dtype=torch.uint8, device=g.device)
        if out is None:
            out = torch.empty(n_win * HET_ROW_DTYPE.itemsize, dtype=torch.uint8, device=g.device)
        self._same_len("het_reduce_dev", n, pos, g)
        self._room("het_reduce_dev: out", out, n_win * HET_ROW_DTYPE.itemsize)
        self._room("het_reduce_dev: tree", tree, self.tree_bytes(PGT_STAT_HET, n))
        self._check(self._lib.pgt_het_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), self._col(g, torch.int8, "g"), n,
            self._dev(win, torch.uint8, "win"), n_win, self._dev(out, torch.uint8, "out"), out.numel(),
            self._dev(tree, torch.uint8, "tree"), tree.numel(), self._stream(stream)))
        return out, tree

    def dxy_reduce_dev(self, pos, p1, p2, n1, n2, minind, win, out=None, tot=None, tree=None, stream=None):
        """tot: None = a fresh total buffer is allocated and filled; False = no genome-wide total is wanted (the C
        ABI's tot == NULL: only the tree levels the windows need are built, no whole-input query runs)."""
        import torch
        n = p1.numel()
        n_win = win.numel() // WIN_DTYPE.itemsize
        if tree is None:
            tree = torch.empty(self.tree_bytes(PGT_STAT_DXY, n), dtype=torch.uint8, device=p1.device)
        if out is None:
            out = torch.empty(n_win * DXY_ROW_DTYPE.itemsize, dtype=torch.uint8, device=p1.device)
        if tot is None:
            tot = torch.empty(DXY_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=p1.device)
        elif tot is False:
            tot = None
        self._same_len("dxy_reduce_dev", n, pos, p1, p2, n1, n2)
        self._room("dxy_reduce_dev: out", out, n_win * DXY_ROW_DTYPE.itemsize)
        self._room("dxy_reduce_dev: tree", tree, self.tree_bytes(PGT_STAT_DXY, n))
        self._check(self._lib.pgt_dxy_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), self._col(p1, torch.float64, "p1"),
            self._col(p2, torch.float64, "p2"), self._col(n1, torch.int32, "n1"), self._col(n2, torch.int32, "n2"),
            n, int(minind), self._dev(win, torch.uint8, "win") if n_win else None, n_win,
            self._dev(out, torch.uint8, "out") if n_win else None, out.numel(),
            self._dev(tot, torch.uint8, "tot") if tot is not None else None,
            self._dev(tree, torch.uint8, "tree"), tree.numel(), self._stream(stream)))
        return out, tot, tree

    def dxy_het_reduce_dev(self, pos, p1, p2, n1, n2, g1, g2, minind, win, tree=None, stream=None):
        """BASELINE config 3: dxy + het(g1) + het(g2) over one pos column / window table, two launches."""
        import torch
        n = p1.numel()
        n_win = win.numel() // WIN_DTYPE.itemsize
        dev = p1.device
        if tree is None:
            tree = torch.empty(self.tree_bytes(PGT_STAT_DXY, n) + 2 * self.tree_bytes(PGT_STAT_HET, n),
                               dtype=torch.uint8, device=dev)
        dxy_out = torch.empty(n_win * DXY_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        tot = torch.empty(DXY_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        h1 = torch.empty(n_win * HET_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        h2 = torch.empty(n_win * HET_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._same_len("dxy_het_reduce_dev", n, pos, p1, p2, n1, n2, g1, g2)
        self._room("dxy_het_reduce_dev: tree", tree, self.tree_bytes(PGT_STAT_DXY, n) + 2 * self.tree_bytes(PGT_STAT_HET, n))
        self._check(self._lib.pgt_dxy_het_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), self._col(p1, torch.float64, "p1"),
            self._col(p2, torch.float64, "p2"), self._col(n1, torch.int32, "n1"), self._col(n2, torch.int32, "n2"),
            self._col(g1, torch.int8, "g1"), self._col(g2, torch.int8, "g2"), n, int(minind),
            self._dev(win, torch.uint8, "win"), n_win, self._dev(dxy_out, torch.uint8, "dxy_out"), dxy_out.numel(),
            self._dev(tot, torch.uint8, "tot"), self._dev(h1, torch.uint8, "het_out1"),
            self._dev(h2, torch.uint8, "het_out2"), min(h1.numel(), h2.numel()), self._dev(tree, torch.uint8, "tree"),
            tree.numel(), self._stream(stream)))
        return dxy_out, tot, h1, h2, tree

    def fst_af_reduce_dev(self, pos, freqs, nsamp, win, out=None, tree=None, stream=None):
        """Allele frequencies of len(freqs) populations -> FST rows of all pairs i<j (pair-major),
        WCFst() of betaAFOutlier.R:400-418 + fstWindow's Σa/Σ(a+b).  freqs: float64 CUDA tensors."""
        import torch
        n_pops = len(freqs)
        n = freqs[0].numel()
        n_pairs = n_pops * (n_pops - 1) // 2
        n_win = win.numel() // WIN_DTYPE.itemsize
        tb = int(self._lib.pgt_af_tree_bytes(n_pops, n))
        if tree is None:
            tree = torch.empty(tb, dtype=torch.uint8, device=pos.device)
        if out is None:
            out = torch.empty(n_pairs * n_win * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=pos.device)
        self._same_len("fst_af_reduce_dev", n, pos, *freqs)
        self._room("fst_af_reduce_dev: out", out, n_pairs * n_win * FST_ROW_DTYPE.itemsize)
        self._room("fst_af_reduce_dev: tree", tree, tb)
        pf = (C.c_void_p * n_pops)(*[self._col(t, torch.float64, "freq") for t in freqs])
        ns = (C.c_double * n_pops)(*[float(x) for x in nsamp])
        self._check(self._lib.pgt_fst_af_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), pf, ns, n_pops, n, self._dev(win, torch.uint8, "win"),
            n_win, self._dev(out, torch.uint8, "out"), out.numel(), self._dev(tree, torch.uint8, "tree"), tree.numel(),
            self._stream(stream)))
        return out, tree

    def _pops_reduce_dev(self, st: _PopsStat, pos, freqs, ninds, minind, win, out, tot, tree, stream, work_bytes=None, work_word="tree"):
        """The device form of a K-population statistic (pgt_<name>_pops_reduce_dev) -> (out, tot, tree).  work_bytes(n_pops, n,
        n_win): the size of a workspace that holds more than the tree, named work_word in the messages."""
        import torch
        who = f"{st.name}_pops_reduce_dev"
        n_pops = len(freqs)
        st.check_count(who, freqs, ninds)
        n = freqs[0].numel()
        tables = st.tables(n_pops)
        n_win = win.numel() // WIN_DTYPE.itemsize
        tb = int(work_bytes(n_pops, n, n_win)) if work_bytes else int(getattr(self._lib, f"pgt_{st.name}_pops_tree_bytes")(n_pops, n))
        dev = pos.device
        if tree is None:
            tree = torch.empty(tb, dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty(tables * n_win * st.row.itemsize, dtype=torch.uint8, device=dev)
        if tot is None:
            tot = torch.empty(tables * st.total.itemsize, dtype=torch.uint8, device=dev)
        elif tot is False:
            tot = None
        self._same_len(who, n, pos, *freqs, *ninds)
        self._room(f"{who}: out", out, tables * n_win * st.row.itemsize)
        self._room(f"{who}: {work_word}", tree, tb)
        if tot is not None:
            self._room(f"{who}: tot", tot, tables * st.total.itemsize)
        pf = (C.c_void_p * n_pops)(*[self._col(t, torch.float64, f"freqs[{k}]") for k, t in enumerate(freqs)])
        pn = (C.c_void_p * n_pops)(*[self._col(t, torch.int32, f"ninds[{k}]") for k, t in enumerate(ninds)])
        self._check(getattr(self._lib, f"pgt_{who}")(
            self._ctx, self._dev(pos, torch.int32, "pos"), pf, pn, n_pops, n, int(minind),
            self._dev(win, torch.uint8, "win") if n_win else None, n_win,
            self._dev(out, torch.uint8, "out") if n_win else None, out.numel(),
            self._dev(tot, torch.uint8, "tot") if tot is not None else None,
            self._dev(tree, torch.uint8, work_word), tree.numel(), self._stream(stream)))
        return out, tot, tree

    @staticmethod
    def dxy_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_dxy_pops_tree_bytes(int(n_pops), int(n_sites)))

    def dxy_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """dxy rows of ALL pairs i<j of len(freqs) populations (pair-major, pair_order) in one pass over the populations'
        own columns.  freqs: float64 CUDA tensors, ninds: int32 CUDA tensors.  tot: None = a fresh buffer of n_pairs totals
        is allocated and filled; False = no genome-wide lines.  Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_DXY_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def fst_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_fst_pops_tree_bytes(int(n_pops), int(n_sites)))

    def fst_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """FST rows of ALL pairs i<j of len(freqs) populations (pair-major, pair_order) in one pass over the populations' own
        (freq, nInd) columns, with per-site sample sizes and the -minind predicate.  freqs: float64 CUDA tensors, ninds: int32
        CUDA tensors.  tot: None = a fresh buffer of n_pairs totals is allocated and filled; False = no genome-wide lines.
        Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_FST_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def fst_hudson_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_fst_hudson_pops_tree_bytes(int(n_pops), int(n_sites)))

    def fst_hudson_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """fst_pops_reduce_dev with Hudson's estimator as a ratio of averages (pgt_fst_hudson_pops_reduce_dev): the same
        arguments, buffers (the tree is fst_pops_tree_bytes large and may be reused between the two, one call at a time) and
        row layout; asum = Σ [(p1-p2)² - h1 - h2], bsum = Σ dxy.  Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_FST_HUDSON_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def pi_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_pi_pops_tree_bytes(int(n_pops), int(n_sites)))

    def pi_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """Nucleotide-diversity (pi) rows of EACH of len(freqs) populations (1 ... 8; population-major) in one pass over the
        populations' own (freq, nInd) columns.  freqs: float64 CUDA tensors, ninds: int32 CUDA tensors.  tot: None = a fresh
        buffer of n_pops totals is allocated and filled; False = no genome-wide lines.  All three hints of the context are
        honoured (the query strategies of dxy_reduce_dev).  Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_PI_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def dstat_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_dstat_pops_tree_bytes(int(n_pops), int(n_sites)))

    def dstat_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """ABBA-BABA rows of ALL ingroup trios (trio-major, trio_order) against the last population, the outgroup, in one pass
        over 4 ... 7 populations' own (freq, nInd) columns (pgt_dstat_pops_reduce_dev).  freqs: float64 CUDA tensors, ninds:
        int32 CUDA tensors.  tot: None = a fresh buffer of n_trios totals is allocated and filled; False = no genome-wide
        lines.  Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_DSTAT_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def fd_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_fd_pops_tree_bytes(int(n_pops), int(n_sites)))

    def fd_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """f_d / f_dM rows of ALL ingroup trios (trio-major, trio_order; ((P1 = i, P2 = j), P3 = k)) against the last population,
        the outgroup, in one pass over 4 ... 7 populations' own (freq, nInd) columns (pgt_fd_pops_reduce_dev): the arguments and
        buffers of dstat_pops_reduce_dev (the tree is dstat_pops_tree_bytes large and may be reused between the two, one call at
        a time), rows of FD_ROW_DTYPE, totals of FD_TOTAL_DTYPE.  Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_FD_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def dstat_jackknife_work_bytes(n_trios: int, n_win: int) -> int:
        return int(_lib.load().pgt_dstat_jackknife_work_bytes(int(n_trios), int(n_win)))

    def _jackknife_dev(self, name: str, row: np.dtype, jack: np.dtype, rows, n_win, n_trios, out, work, stream, items: int = 3):
        """The device form of a block jackknife (pgt_<name>_jackknife_dev) -> (out, work); `items` results per table."""
        import torch
        who = f"{name}_jackknife_dev"
        n_win, n_trios = int(n_win), int(n_trios)
        wb = int(getattr(self._lib, f"pgt_{name}_jackknife_work_bytes")(n_trios, n_win))
        if wb == 0:
            raise PgtError(_lib.PGT_EARG, f"{who}: n_quartets must be 1 ... 15" if name == "f4" else
                           (f"{who}: n_triples must be 1 ... 10" if name == "f4ratio" else f"{who}: n_trios must be 1 ... 20"))
        self._room(f"{who}: rows", rows, n_trios * n_win * row.itemsize)
        if out is None:
            out = torch.empty(items * n_trios * jack.itemsize, dtype=torch.uint8, device=rows.device)
        if work is None:
            work = torch.empty(wb, dtype=torch.uint8, device=rows.device)
        self._room(f"{who}: out", out, items * n_trios * jack.itemsize)
        self._room(f"{who}: work", work, wb)
        self._check(getattr(self._lib, f"pgt_{who}")(
            self._ctx, self._dev(rows, torch.uint8, "rows") if n_win else None, n_win, n_trios,
            self._dev(out, torch.uint8, "out"), out.numel(), self._dev(work, torch.uint8, "work"), work.numel(), self._stream(stream)))
        return out, work

    def dstat_jackknife_dev(self, rows, n_win, n_trios, out=None, work=None, stream=None):
        """Block-jackknife D, standard error and Z of n_trios trios x 3 topologies from the device rows of
        dstat_pops_reduce_dev (uint8 CUDA tensor, trio-major, n_trios * n_win rows; the windows must be disjoint)
        (pgt_dstat_jackknife_dev).  Returns (out, work): out holds 3 * n_trios DSTAT_JACK_DTYPE, item 3 t + c
        (rows_from_device(out, DSTAT_JACK_DTYPE)).  Asynchronous on `stream`; no allocation when out and work are given."""
        return self._jackknife_dev("dstat", DSTAT_ROW_DTYPE, DSTAT_JACK_DTYPE, rows, n_win, n_trios, out, work, stream)

    @staticmethod
    def f3_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_f3_pops_tree_bytes(int(n_pops), int(n_sites)))

    def f3_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """f3 rows of ALL trios of len(freqs) populations (trio-major, all_trio_order; no outgroup), every population of a trio
        as the target, in one pass over 3 ... 6 populations' own (freq, nInd) columns (pgt_f3_pops_reduce_dev).  freqs: float64
        CUDA tensors, ninds: int32 CUDA tensors.  Rows of F3_ROW_DTYPE carry SUMS (f3 = sum / n), totals are F3_TOTAL_DTYPE.
        tot: None = a fresh buffer of n_trios totals is allocated and filled; False = no genome-wide lines.
        Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_F3_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def pbs_pops_work_bytes(n_pops: int, n_sites: int, n_win: int) -> int:
        return int(_lib.load().pgt_pbs_pops_work_bytes(int(n_pops), int(n_sites), int(n_win)))

    def pbs_pops_reduce_dev(self, pos, freqs, ninds, minind, win, estimator="wc", out=None, tot=None, work=None, stream=None):
        """Population-branch-statistic rows of ALL trios of len(freqs) populations (trio-major, all_trio_order), every population
        of a trio as the focal one, from 3 ... 6 populations' own (freq, nInd) columns (pgt_pbs_pops_reduce_dev; estimator="hudson":
        pgt_pbs_hudson_pops_reduce_dev).  freqs: float64 CUDA tensors, ninds: int32 CUDA tensors.  Rows of PBS_ROW_DTYPE, totals of
        PBS_TOTAL_DTYPE.  work: pbs_pops_work_bytes(n_pops, n, n_win) bytes (the tree of one pass and the scratch rows of both).
        tot: None = a fresh buffer of n_trios totals is allocated and filled; False = no genome-wide lines.
        Returns (out, tot, work).  Asynchronous on `stream`: one chain of kernels."""
        st = _pbs_estimator("pbs_pops_reduce_dev", estimator)
        return self._pops_reduce_dev(st, pos, freqs, ninds, minind, win, out, tot, work, stream, self._lib.pgt_pbs_pops_work_bytes, "work")

    @staticmethod
    def f3_jackknife_work_bytes(n_trios: int, n_win: int) -> int:
        return int(_lib.load().pgt_f3_jackknife_work_bytes(int(n_trios), int(n_win)))

    def f3_jackknife_dev(self, rows, n_win, n_trios, out=None, work=None, stream=None):
        """Block-jackknife f3, standard error and Z of n_trios trios x 3 targets from the device rows of f3_pops_reduce_dev
        (uint8 CUDA tensor, trio-major, n_trios * n_win rows; the windows must be disjoint) (pgt_f3_jackknife_dev).
        Returns (out, work): out holds 3 * n_trios F3_JACK_DTYPE, item 3 t + c with c the target i / j / k
        (rows_from_device(out, F3_JACK_DTYPE)).  Asynchronous on `stream`; no allocation when out and work are given."""
        return self._jackknife_dev("f3", F3_ROW_DTYPE, F3_JACK_DTYPE, rows, n_win, n_trios, out, work, stream)

    @staticmethod
    def f4_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_f4_pops_tree_bytes(int(n_pops), int(n_sites)))

    def f4_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """f4 rows of ALL quartets of len(freqs) populations (quartet-major, all_quartet_order; no outgroup), every quartet in its
        three pairings, in one pass over 4 ... 6 populations' own (freq, nInd) columns (pgt_f4_pops_reduce_dev).  freqs: float64
        CUDA tensors, ninds: int32 CUDA tensors.  Rows of F4_ROW_DTYPE carry SUMS (f4 = sum / n), totals are F4_TOTAL_DTYPE.
        tot: None = a fresh buffer of n_quartets totals is allocated and filled; False = no genome-wide lines.
        Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_F4_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def f4_jackknife_work_bytes(n_quartets: int, n_win: int) -> int:
        return int(_lib.load().pgt_f4_jackknife_work_bytes(int(n_quartets), int(n_win)))

    def f4_jackknife_dev(self, rows, n_win, n_quartets, out=None, work=None, stream=None):
        """Block-jackknife f4, standard error and Z of n_quartets quartets x 3 pairings from the device rows of
        f4_pops_reduce_dev (uint8 CUDA tensor, quartet-major, n_quartets * n_win rows; the windows must be disjoint)
        (pgt_f4_jackknife_dev).  Returns (out, work): out holds 3 * n_quartets F4_JACK_DTYPE, item 3 q + c with c the pairing
        (ij;kl) / (ik;jl) / (il;jk) (rows_from_device(out, F4_JACK_DTYPE)).  Asynchronous on `stream`; no allocation when out
        and work are given."""
        return self._jackknife_dev("f4", F4_ROW_DTYPE, F4_JACK_DTYPE, rows, n_win, n_quartets, out, work, stream)

    @staticmethod
    def f4ratio_pops_tree_bytes(n_pops: int, n_sites: int) -> int:
        return int(_lib.load().pgt_f4ratio_pops_tree_bytes(int(n_pops), int(n_sites)))

    def f4ratio_pops_reduce_dev(self, pos, freqs, ninds, minind, win, out=None, tot=None, tree=None, stream=None):
        """The f4-ratio sums of ALL triples of the middle populations (triple-major, middle_triple_order) between population 0 (A)
        and the last one (the outgroup), in one pass over 5 ... 7 populations' own (freq, nInd) columns
        (pgt_f4ratio_pops_reduce_dev).  freqs: float64 CUDA tensors, ninds: int32 CUDA tensors.  Rows of F4RATIO_ROW_DTYPE carry
        SUMS over the sites all five populations cover (the ratios are the caller's: f4ratio_alphas), totals are
        F4RATIO_TOTAL_DTYPE.  tot: None = a fresh buffer of n_triples totals is allocated and filled; False = no genome-wide lines.
        Returns (out, tot, tree).  Asynchronous on `stream`."""
        return self._pops_reduce_dev(_F4RATIO_POPS, pos, freqs, ninds, minind, win, out, tot, tree, stream)

    @staticmethod
    def f4ratio_jackknife_work_bytes(n_triples: int, n_win: int) -> int:
        return int(_lib.load().pgt_f4ratio_jackknife_work_bytes(int(n_triples), int(n_win)))

    def f4ratio_jackknife_dev(self, rows, n_win, n_triples, out=None, work=None, stream=None):
        """Block-jackknife admixture proportion, standard error and Z of n_triples middle triples x 6 (B, X, C) from the device rows
        of f4ratio_pops_reduce_dev (uint8 CUDA tensor, triple-major, n_triples * n_win rows; the windows must be disjoint)
        (pgt_f4ratio_jackknife_dev).  Returns (out, work): out holds 6 * n_triples F4RATIO_JACK_DTYPE, item 6 t + c with c the
        position in ratio_order (rows_from_device(out, F4RATIO_JACK_DTYPE)).  Asynchronous on `stream`; no allocation when out and
        work are given."""
        return self._jackknife_dev("f4ratio", F4RATIO_ROW_DTYPE, F4RATIO_JACK_DTYPE, rows, n_win, n_triples, out, work, stream, items=6)

    @staticmethod
    def pbs_jackknife_work_bytes(n_trios: int, n_win: int) -> int:
        return int(_lib.load().pgt_pbs_jackknife_work_bytes(int(n_trios), int(n_win)))

    def pbs_jackknife_dev(self, rows, n_win, n_trios, out=None, work=None, stream=None):
        """Block-jackknife PBS and PBSn1, standard error and Z of n_trios trios x 6 items from the device rows of
        pbs_pops_reduce_dev, either estimator (uint8 CUDA tensor, trio-major, n_trios * n_win rows of 88 bytes; the windows must be
        disjoint) (pgt_pbs_jackknife_dev).  Returns (out, work): out holds 6 * n_trios PBS_JACK_DTYPE, item 6 t + c with c the
        position in pbs_item_order (rows_from_device(out, PBS_JACK_DTYPE)).  Asynchronous on `stream`; no allocation when out and
        work are given."""
        return self._jackknife_dev("pbs", PBS_ROW_DTYPE, PBS_JACK_DTYPE, rows, n_win, n_trios, out, work, stream, items=6)

    def extreme_reduce_dev(self, pos, score, mode, cutoff, win, out=None, tree=None, stream=None):
        """ihsWindow / xpehhWindow rows from a device-resident score column (mode: PGT_EXT_*)."""
        import torch
        n = score.numel()
        n_win = win.numel() // WIN_DTYPE.itemsize
        tb = self.tree_bytes(PGT_STAT_EXT, n)
        if tree is None:
            tree = torch.empty(tb, dtype=torch.uint8, device=score.device)
        if out is None:
            out = torch.empty(n_win * EXT_ROW_DTYPE.itemsize, dtype=torch.uint8, device=score.device)
        self._same_len("extreme_reduce_dev", n, pos, score)
        self._room("extreme_reduce_dev: out", out, n_win * EXT_ROW_DTYPE.itemsize)
        self._room("extreme_reduce_dev: tree", tree, tb)
        self._check(self._lib.pgt_extreme_reduce_dev(
            self._ctx, self._dev(pos, torch.int32, "pos"), self._col(score, torch.float64, "score"), n, int(mode),
            float(cutoff), self._dev(win, torch.uint8, "win"), n_win, self._dev(out, torch.uint8, "out"), out.numel(),
            self._dev(tree, torch.uint8, "tree"), tree.numel(), self._stream(stream)))
        return out, tree

    # ---- the sites common to K files (pgt_sites_align, pgt_gather_dev) -------------------------
    @staticmethod
    def align_workspace_bytes(n_files: int, n_rows_file0: int) -> int:
        return int(_lib.load().pgt_align_workspace_bytes(int(n_files), int(n_rows_file0)))

    def sites_align(self, pos_list, segs, cap=None, idx=None, work=None, stream=None):
        """The sites (chromosome, position) present in ALL of len(pos_list) files.  pos_list: int32 CUDA tensors (the u32
        position columns, strictly increasing inside a chromosome); segs: align_segments' plan.  Returns (idx, counts,
        n_common): idx[k] an int32 CUDA tensor, idx[k][m] = the row of common site m in file k; counts[c] = common sites of
        matched chromosome c (numpy u64).  cap: room per index column (default: the most the plan admits); a cap too small
        raises PgtError(PGT_ECAP) carrying .n_common and .counts.  Synchronous."""
        import torch
        k = len(pos_list)
        if not 2 <= k <= 8:
            raise PgtError(_lib.PGT_EARG, "sites_align: 2 ... 8 position columns")
        segs = np.ascontiguousarray(segs, dtype=SEG_DTYPE).reshape(-1, k) if np.size(segs) else np.zeros((0, k), SEG_DTYPE)
        n_rows = [int(p.numel()) for p in pos_list]
        for f in range(k):
            if segs.shape[0] and int((segs["off"][:, f] + segs["len"][:, f]).max()) > n_rows[f]:
                raise PgtError(_lib.PGT_EARG, f"sites_align: a segment of file {f} runs beyond its {n_rows[f]} rows")
        most = int(segs["len"].min(axis=1).sum()) if segs.shape[0] else 0
        if cap is None:
            cap = most if idx is None else min(int(t.numel()) for t in idx)
        cap = int(cap)
        dev = torch.device("cuda", self.device)
        if idx is None:
            idx = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(k)]
        if len(idx) != k:
            raise PgtError(_lib.PGT_EARG, "sites_align: one index column per file")
        for f, t in enumerate(idx):
            if t.numel() < cap:
                raise PgtError(_lib.PGT_EARG, f"sites_align: idx[{f}] holds {t.numel()} rows, cap is {cap}")
        wb = self.align_workspace_bytes(k, n_rows[0])
        if work is None:
            work = torch.empty(wb, dtype=torch.uint8, device=dev)
        self._room("sites_align: work", work, wb)
        pp = (C.c_void_p * k)(*[self._dev(t, torch.int32, f"pos_list[{f}]") for f, t in enumerate(pos_list)])
        pi = (C.c_void_p * k)(*[self._dev(t, torch.int32, f"idx[{f}]") for f, t in enumerate(idx)])
        nr = (C.c_uint64 * k)(*n_rows)
        counts = np.zeros(segs.shape[0], dtype=np.uint64)
        n_common = C.c_uint64(0)
        rc = self._lib.pgt_sites_align(self._ctx, pp, nr, k, segs.ctypes.data if segs.size else None, segs.size, pi, cap,
                                       counts.ctypes.data if counts.size else None, C.byref(n_common),
                                       self._dev(work, torch.uint8, "work"), work.numel(), self._stream(stream))
        if rc == _lib.PGT_ECAP:
            e = PgtError(rc, _lib.last_error(self._ctx))
            e.n_common, e.counts = int(n_common.value), counts
            raise e
        self._check(rc)
        n = int(n_common.value)
        return [t[:n] for t in idx], counts, n

    def gather_dev(self, src, idx, out=None, stream=None):
        """out[m] = src[idx[m]] (pgt_gather_dev): src a CUDA tensor of 4- or 8-byte elements, idx an int32 CUDA tensor of
        rows of src.  Returns out (same dtype as src, idx.numel() elements).  Asynchronous on `stream`."""
        import torch
        if not isinstance(src, (torch.Tensor, DeviceColumn)):
            raise PgtError(_lib.PGT_EARG, "gather_dev: src: expected a contiguous CUDA tensor")
        elem = torch.empty(0, dtype=src.dtype).element_size()
        if elem not in (4, 8):
            raise PgtError(_lib.PGT_EARG, f"gather_dev: src: elements of 4 or 8 bytes, not {src.dtype}")
        n = idx.numel()
        if out is None:
            out = torch.empty(n, dtype=src.dtype, device=torch.device("cuda", self.device))
        if out.dtype != src.dtype or out.numel() < n:
            raise PgtError(_lib.PGT_EARG, f"gather_dev: out: {n} elements of {src.dtype} needed")
        self._check(self._lib.pgt_gather_dev(self._ctx, self._dev(out, src.dtype, "out"), self._dev(src, src.dtype, "src"),
                                             self._dev(idx, torch.int32, "idx"), n, elem, self._stream(stream)))
        return out

    def set_max_window(self, sites: int):
        """Performance hint for the *_dev calls: no window is longer than `sites` (0 = unknown)."""
        self._check(self._lib.pgt_set_max_window(self._ctx, int(sites)))
        self._hints = (int(sites), getattr(self, "_hints", (0, 0))[1])
        self._typical = 0  # the library resets it: the explicit longest window stands for the typical one

    def set_window_step(self, sites: int):
        """Performance hint for the *_dev calls: consecutive windows start `sites` apart (0 = unknown);
        small steps select the sliding query (include/pgtwin.h)."""
        self._check(self._lib.pgt_set_window_step(self._ctx, int(sites)))
        self._hints = (getattr(self, "_hints", (0, 0))[0], int(sites))

    def set_typical_window(self, sites: int):
        """Performance hint for tables whose windows vary in length (base-pair windows): the typical length decides
        between the query strategies instead of the longest.  After set_max_window, which resets it (0 = the same)."""
        self._check(self._lib.pgt_set_typical_window(self._ctx, int(sites)))
        self._typical = int(sites)

    def hints(self, max_window: int, window_step: int, typical_window: int = 0):
        """with ctx.hints(max_window, step[, typical]): ... — the hints for the duration of the block, then the previous ones."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            saved = getattr(self, "_hints", (0, 0)) + (getattr(self, "_typical", 0),)
            self.set_max_window(max_window)
            self.set_window_step(window_step)
            self.set_typical_window(typical_window)
            try:
                yield self
            finally:
                self.set_max_window(saved[0])
                self.set_window_step(saved[1])
                self.set_typical_window(saved[2])
        return scope()

    # ---- per-kernel timing ------------------------------------------------------------------
    def set_profiling(self, enabled: bool):
        self._check(self._lib.pgt_set_profiling(self._ctx, int(enabled)))

    def last_kernel_ms(self):
        b, q = C.c_float(0), C.c_float(0)
        self._check(self._lib.pgt_last_kernel_ms(self._ctx, C.byref(b), C.byref(q)))
        return b.value, q.value


def rows_from_device(t, dtype: np.dtype) -> np.ndarray:
    """uint8 CUDA tensor of packed rows -> numpy structured array (synchronises)."""
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype)


def windows_to_device(win: np.ndarray, device):
    import torch
    raw = np.ascontiguousarray(win, dtype=WIN_DTYPE).view(np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


# ---------------------------------------------------------------------------------------------
# the three tools over in-memory columns
# ---------------------------------------------------------------------------------------------
@dataclass
class WindowResult:
    win: np.ndarray   # WIN_DTYPE rows (label_run indexes the chromosome runs)
    rows: np.ndarray  # per-tool row dtype
    total: object = None  # dxy only: DXY_TOTAL_DTYPE scalar


def _own_ctx(ctx):
    return (Context(), True) if ctx is None else (ctx, False)


def fst_window(chr_ids, pos, a, b, W: int = 1, S: int = 1, ctx: Context | None = None) -> WindowResult:
    """fstWindow.cpp:109-155 over columns: rows are (start, end, mid, n, fst)."""
    win = build_windows_sites(run_lengths(chr_ids), W, S)
    ctx, own = _own_ctx(ctx)
    try:
        return WindowResult(win, ctx.fst_reduce(pos, a, b, win))
    finally:
        if own:
            ctx.close()


def het_window(chr_ids, pos, g, W: int = 1, S: int = 1, ctx: Context | None = None) -> WindowResult:
    """hetWindow.cpp:107-153 over columns; genotypes are clipped to int8 (only `>= 0` and `== 1`
    matter, hetWindow.cpp:78-80)."""
    win = build_windows_sites(run_lengths(chr_ids), W, S)
    g8 = np.clip(np.asarray(g), -128, 127).astype(np.int8)
    ctx, own = _own_ctx(ctx)
    try:
        return WindowResult(win, ctx.het_reduce(pos, g8, win))
    finally:
        if own:
            ctx.close()


def _refuse_dxy_window_args(W, S, minind, fixedsite, chr_len):
    """The refusals of dxyWindow's command line, raised before a context is opened (dxy_window and the *_window_pops)."""
    if minind <= 0:
        raise PgtError(_lib.PGT_EARG, "-minind must be at least 1")  # dxyWindow.cpp:105-108
    if W > 0 and S < 1:
        raise PgtError(_lib.PGT_EARG, "Must specify a -stepsize > 0 when -winsize is > 0")  # :128-131
    if not fixedsite and chr_len is None:
        raise PgtError(_lib.PGT_EARG, "Must supply size file unless -fixedsite 1")  # :133-136
    if W == 0 and not fixedsite:
        raise PgtError(_lib.PGT_EDOMAIN, "-winsize 0 needs -fixedsite 1 (the reference crashes here, SURVEY Q10)")


def _dxy_window_table(chr_ids, pos, W, S, fixedsite, chr_len) -> np.ndarray:
    """dxyWindow's table: none (-winsize 0: the genome-wide line alone), site windows (-fixedsite 1) or base-pair slots."""
    rl = run_lengths(chr_ids)
    if W == 0:
        return np.zeros(0, dtype=WIN_DTYPE)
    if fixedsite:
        return build_windows_sites(rl, W, S)
    return build_windows_bp(pos, rl, chr_len, W, S)


def dxy_window(chr_ids, pos, p1, p2, n1, n2, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
               chr_len=None, skip_missing: int = 0, ctx: Context | None = None) -> WindowResult:
    """dxyWindow.cpp:253-436 over two already synchronised populations.  chr_len[r] is the -sizefile
    length of run r (required unless fixedsite).  Rows suppressed by -skip_missing are dropped, as
    dxyWindow.cpp:189 does."""
    _refuse_dxy_window_args(W, S, minind, fixedsite, chr_len)
    win = _dxy_window_table(chr_ids, pos, W, S, fixedsite, chr_len)
    ctx, own = _own_ctx(ctx)
    try:
        rows, tot = ctx.dxy_reduce(pos, p1, p2, n1, n2, minind, win)
    finally:
        if own:
            ctx.close()
    if skip_missing:
        keep = rows["neff"] > 0
        win, rows = win[keep], rows[keep]
    return WindowResult(win, rows, tot)


def _host_col(x, dtype):
    """numpy view of a column given as numpy / list / torch tensor (a CUDA tensor is downloaded; int32 tensors stand for
    u32 columns bit for bit)."""
    if hasattr(x, "detach") and hasattr(x, "cpu"):
        x = x.detach().cpu().numpy()
        if x.dtype == np.int32 and np.dtype(dtype) == np.uint32:
            x = x.view(np.uint32)
    return np.ascontiguousarray(x, dtype=dtype)


def align_sites(chr_ids_list, pos_list, columns_list, ctx: Context | None = None):
    """K files' columns brought onto the sites all K share.  Per file: chr_ids (per-site chromosome ids on the host, equal
    names = equal ids in every file), pos (u32 positions: numpy, or an int32 CUDA tensor) and a list of further columns
    (CUDA tensors or numpy arrays of 4- or 8-byte elements).  The alignment runs on the device (sites_align + gather_dev).
    Returns (chr_ids, pos, aligned_columns_list) as CUDA tensors (chr_ids and pos int32, standing for u32): what
    dxy_window_pops and Context.dxy_pops_reduce_dev take, with freqs = [cols[0] for cols in aligned_columns_list] etc."""
    k = len(pos_list)
    if not 2 <= k <= 8 or len(chr_ids_list) != k or len(columns_list) != k:
        raise PgtError(_lib.PGT_EARG, "align_sites: 2 ... 8 files, each with chromosome ids, positions and a list of columns")
    n_rows = [int(p.numel()) if hasattr(p, "numel") else int(np.size(p)) for p in pos_list]
    for f in range(k):
        nc = int(c.numel()) if hasattr((c := chr_ids_list[f]), "numel") else int(np.size(c))
        if nc != n_rows[f]:
            raise PgtError(_lib.PGT_EARG, f"align_sites: file {f}: {nc} chromosome ids for {n_rows[f]} positions")
        for j, col in enumerate(columns_list[f]):
            m = int(col.numel()) if hasattr(col, "numel") else int(np.size(col))
            if m != n_rows[f]:
                raise PgtError(_lib.PGT_EARG, f"align_sites: file {f}: column {j} has {m} rows, the positions {n_rows[f]}")
            size = col.element_size() if hasattr(col, "element_size") else np.asarray(col).dtype.itemsize
            if size not in (4, 8):
                raise PgtError(_lib.PGT_EARG, f"align_sites: file {f}: column {j}: elements of 4 or 8 bytes, not {size}")
    segs, chr_of = align_segments(chr_ids_list)
    import torch
    ctx, own = _own_ctx(ctx)
    try:
        dev = torch.device("cuda", ctx.device)

        def on_device(x, u32=False):
            if isinstance(x, torch.Tensor):
                return x.to(dev)
            a = np.ascontiguousarray(x, dtype=np.uint32).view(np.int32) if u32 else np.ascontiguousarray(x)
            return torch.from_numpy(a.copy()).to(dev)
        pos_d = [on_device(p, u32=True) for p in pos_list]
        idx, counts, n = ctx.sites_align(pos_d, segs)
        pos = ctx.gather_dev(pos_d[0], idx[0])
        cols = [[ctx.gather_dev(on_device(c), idx[f]) for c in columns_list[f]] for f in range(k)]
        chr_ids = torch.from_numpy(np.repeat(chr_of, counts.astype(np.int64)).view(np.int32).copy()).to(dev)
        torch.cuda.synchronize(dev)
    finally:
        if own:
            ctx.close()
    return chr_ids, pos, cols


def pair_order(n_pops: int):
    """The pairs (i, j), i < j, in the order the all-pairs entry points (fst_af_reduce_dev, dxy_pops_reduce*) lay their
    rows out: (0,1),(0,2),..,(0,n_pops-1),(1,2),.."""
    return [(i, j) for i in range(int(n_pops)) for j in range(i + 1, int(n_pops))]


def trio_order(n_pops: int):
    """The ingroup trios (i, j, k), i < j < k < n_pops - 1, in the order dstat_pops_reduce* lays its rows out (the last
    population is the outgroup): (0,1,2),(0,1,3),..,(0,1,n_pops-2),(0,2,3),.."""
    g = int(n_pops) - 1
    return [(i, j, k) for i in range(g) for j in range(i + 1, g) for k in range(j + 1, g)]


def all_trio_order(n_pops: int):
    """The trios (i, j, k), i < j < k < n_pops, of ALL populations in the order f3_pops_reduce* lays its rows out (there is
    no outgroup): (0,1,2),(0,1,3),..,(0,1,n_pops-1),(0,2,3),.."""
    g = int(n_pops)
    return [(i, j, k) for i in range(g) for j in range(i + 1, g) for k in range(j + 1, g)]


def target_order(i, j, k):
    """The three readings of trio (i, j, k) in the order its row's sums and the block jackknife's items are laid out
    (c = 0, 1, 2), each as (target; source 1, source 2): [(i, j, k), (j, i, k), (k, i, j)]."""
    return [(i, j, k), (j, i, k), (k, i, j)]


def all_quartet_order(n_pops: int):
    """The quartets (i, j, k, l), i < j < k < l < n_pops, of ALL populations in the order f4_pops_reduce* lays its rows out:
    (0,1,2,3),(0,1,2,4),..,(0,1,3,4),.."""
    g = int(n_pops)
    return [(i, j, k, l) for i in range(g) for j in range(i + 1, g) for k in range(j + 1, g) for l in range(k + 1, g)]


def pairing_order(i, j, k, l):
    """The three pairings of quartet (i, j, k, l) in the order its row's sums and the block jackknife's items are laid out
    (c = 0, 1, 2), each as ((a, b), (c, d)) of f4(a, b; c, d): (((i, j), (k, l)), ((i, k), (j, l)), ((i, l), (j, k)))."""
    return ((i, j), (k, l)), ((i, k), (j, l)), ((i, l), (j, k))


def middle_triple_order(n_pops: int):
    """The triples (i, j, k), 1 <= i < j < k <= n_pops - 2, of the MIDDLE populations in the order f4ratio_pops_reduce* lays its
    rows out (population 0 is A, the last one the outgroup): (1,2,3),(1,2,4),..,(1,3,4),.."""
    g = int(n_pops) - 1
    return [(i, j, k) for i in range(1, g) for j in range(i + 1, g) for k in range(j + 1, g)]


def ratio_order(i, j, k):
    """The six admixture proportions of middle triple (i, j, k) in the order f4ratio_alphas and the block jackknife lay them out
    (c = 0 ... 5), each as (B, X, C) of alpha = f4(A,O; X,C) / f4(A,O; B,C), the share of B-related ancestry in X:
    [(i, j, k), (j, i, k), (i, k, j), (k, i, j), (j, k, i), (k, j, i)]."""
    return [(i, j, k), (j, i, k), (i, k, j), (k, i, j), (j, k, i), (k, j, i)]


def f4ratio_alphas(rows) -> np.ndarray:
    """The six admixture proportions of ratio_order from F4RATIO_ROW_DTYPE rows or F4RATIO_TOTAL_DTYPE totals (any shape)
    -> float64 [..., 6]: (numerator, denominator) = (S2, S1), (S1, S2), (-S2, S0), (S0, -S2), (S1, S0), (S0, S1) of the sums
    S0, S1, S2 = g_ij, g_ik, g_jk, each ratio 0 where its denominator is 0.  Nothing is clamped."""
    rows = np.asarray(rows)
    s0, s1, s2 = rows["g_ij"], rows["g_ik"], rows["g_jk"]
    num = np.stack([s2, s1, -s2, s0, s1, s0], axis=-1)
    den = np.stack([s1, s2, s0, -s2, s0, s1], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)


def pbs_item_order(i, j, k):
    """The six items of trio (i, j, k) in the order the block jackknife of PBS lays them out (c = 0 ... 5), each as (statistic,
    focal population): [("pbs", i), ("pbs", j), ("pbs", k), ("pbsn1", i), ("pbsn1", j), ("pbsn1", k)]."""
    return [("pbs", i), ("pbs", j), ("pbs", k), ("pbsn1", i), ("pbsn1", j), ("pbsn1", k)]


def pbsn1_of(rows) -> np.ndarray:
    """PBSn1 (Malaspinas et al. 2016), the branch statistic normalised by the trio's whole tree, of the three focal populations
    from PBS_ROW_DTYPE rows or PBS_TOTAL_DTYPE totals (any shape) -> float64 [..., 3]: from the row's own pbs_i, pbs_j, pbs_k
        s = (pbs_i + pbs_j) + pbs_k        pbsn1_x = pbs_x / (1.0 + s)
    every operation one rounding, in this order.  Nothing is clamped: inf and nan are the IEEE results."""
    rows = np.asarray(rows)
    p = np.stack([rows["pbs_i"], rows["pbs_j"], rows["pbs_k"]], axis=-1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        one_s = 1.0 + ((p[..., 0] + p[..., 1]) + p[..., 2])
        return p / one_s[..., None]


def topology_order(i, j, k):
    """The three topologies of trio (i, j, k) in the order the block jackknife lays its items out (c = 0, 1, 2), each as
    ((P1, P2), P3): [(i, j, k), (i, k, j), (j, k, i)] — D from (abba, baba), (bbaa, baba), (bbaa, abba) of the trio's row."""
    return [(i, j, k), (i, k, j), (j, k, i)]


def _window_pops(st: _PopsStat, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx):
    """What the *_window_pops functions share: dxy_window's refusals, the population count, host columns, the window table and
    one pass of the statistic's numpy form -> (win, rows[tables, n_win], totals[tables])."""
    _refuse_dxy_window_args(W, S, minind, fixedsite, chr_len)
    st.check_count(f"{st.name}_window_pops", freqs, ninds)
    chr_ids, pos = _host_col(chr_ids, None), _host_col(pos, np.uint32)
    freqs, ninds = [_host_col(f, np.float64) for f in freqs], [_host_col(c, np.int32) for c in ninds]
    win = _dxy_window_table(chr_ids, pos, W, S, fixedsite, chr_len)
    ctx, own = _own_ctx(ctx)
    try:
        rows, tot = ctx._pops_reduce(st, pos, freqs, ninds, minind, win)
    finally:
        if own:
            ctx.close()
    return win, rows, tot


def _trio_window_pops_jackknife(st: _PopsStat, jack_dtype, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx, items: int = 3,
                                jack_name: str | None = None, work_bytes=None, work_word: str = "tree"):
    """_window_pops for the rows of a trio statistic (ABBA-BABA, f3) with the rows kept ON THE DEVICE between the reduction and
    the block jackknife (<name>_pops_reduce_dev under the hints the host-buffer form derives from the table: the same rows bit
    for bit, then <name>_jackknife_dev on them) -> (win, rows[n_trios, n_win], totals[n_trios], jack[n_trios, items]).
    jack_name: the jackknife's name where it is not the reduction's (both PBS estimators: "pbs"); work_bytes, work_word: the
    library's size function of a reduction whose workspace holds more than the tree."""
    _refuse_dxy_window_args(W, S, minind, fixedsite, chr_len)
    st.check_count(f"{st.name}_window_pops", freqs, ninds)
    chr_ids, pos = _host_col(chr_ids, None), _host_col(pos, np.uint32)
    freqs, ninds = [_host_col(f, np.float64) for f in freqs], [_host_col(c, np.int32) for c in ninds]
    if any(c.size != pos.size for c in freqs + ninds):
        raise PgtError(_lib.PGT_EARG, f"{st.name}_window_pops: column lengths differ")
    win = _dxy_window_table(chr_ids, pos, W, S, fixedsite, chr_len)
    n_trios = st.tables(len(freqs))
    import torch
    ctx, own = _own_ctx(ctx)
    try:
        dev = torch.device("cuda", ctx.device)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)
        longest, typical, step = table_hints(win)
        with ctx.hints(longest, 0 if step >= 2 ** 63 else step, typical):
            out, tot, _ = ctx._pops_reduce_dev(st, up(pos.view(np.int32)), [up(f) for f in freqs], [up(c) for c in ninds], minind,
                                               windows_to_device(win, dev), None, None, None, None,
                                               getattr(ctx._lib, work_bytes) if work_bytes else None, work_word)
        jack, _ = ctx._jackknife_dev(jack_name or st.name, st.row, jack_dtype, out, win.size, n_trios, None, None, None, items)
        rows = rows_from_device(out, st.row)[: n_trios * win.size].reshape(n_trios, win.size).copy()
        tot = rows_from_device(tot, st.total)[:n_trios].copy()
        jack = rows_from_device(jack, jack_dtype)[: items * n_trios].reshape(n_trios, items).copy()
    finally:
        if own:
            ctx.close()
    return win, rows, tot, jack


def _results_by_pair(n_pops, win, rows, tot, skip_missing, counted: str, keys=None) -> dict:
    """{(i, j): WindowResult} in pair_order (or by `keys`, the tables' own order); -skip_missing drops a pair's rows without
    counted sites (field `counted`)."""
    res = {}
    for p, ij in enumerate(pair_order(n_pops) if keys is None else keys):
        w, r = win, rows[p]
        if skip_missing:
            keep = r[counted] > 0
            w, r = w[keep], r[keep]
        res[ij] = WindowResult(w, r, tot[p])
    return res


def dxy_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                    chr_len=None, skip_missing: int = 0, ctx: Context | None = None) -> dict:
    """dxy_window for ALL pairs of len(freqs) already synchronised populations in one pass: {(i, j): WindowResult}.
    Arguments and errors are those of dxy_window; -skip_missing drops a pair's rows without counted sites from that pair's
    result only.  Columns may be CUDA tensors (align_sites' result): this host-table form downloads them; stay on the device
    with Context.dxy_pops_reduce_dev."""
    win, rows, tot = _window_pops(_DXY_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "neff")


def fst_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                    chr_len=None, skip_missing: int = 0, ctx: Context | None = None, estimator: str = "wc") -> dict:
    """Windowed FST for ALL pairs of len(freqs) already synchronised populations in one pass: {(i, j): WindowResult} with
    fstWindow's rows (n = counted sites of the pair; the skipped ones are (hi - lo) - n) and the genome-wide line as total.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a pair's rows without counted
    sites from that pair's result only.  estimator: "wc" (the Weir–Cockerham components of WCFst(), pgt_fst_pops_reduce)
    or "hudson" (Hudson's ratio of averages, pgt_fst_hudson_pops_reduce: asum = Σ numerator, bsum = Σ dxy)."""
    st = _FST_ESTIMATORS.get(estimator) if isinstance(estimator, str) else None
    if st is None:
        raise PgtError(_lib.PGT_EARG, f'fst_window_pops: estimator must be "wc" or "hudson", not {estimator!r}')
    win, rows, tot = _window_pops(st, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n")


def dstat_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                      chr_len=None, skip_missing: int = 0, ctx: Context | None = None, jackknife: bool = False) -> dict:
    """Windowed ABBA-BABA (Patterson's D) for ALL trios of the first len(freqs) - 1 already synchronised populations against
    the LAST one, the outgroup (4 ... 7 populations), in one pass: {(i, j, k): WindowResult} in trio_order, with rows of
    (start, end, mid, n, d, bbaa, abba, baba) and the genome-wide sums as total.  All columns must report the same allele.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a trio's rows without counted sites
    from that trio's result only.  The per-site definition is pgt_dstat_pops_reduce_dev's (include/pgtwin.h).
    jackknife=True: the result gains the key "jackknife": {(i, j, k): 3 DSTAT_JACK_DTYPE, one per topology_order(i, j, k)} —
    the delete-m_j block jackknife (pgt_dstat_jackknife_dev, on the device rows of the same reduction) over ALL windows of
    the table as blocks, whatever skip_missing is
    (a window without a counted site is no block either way).  The windows must be disjoint: 0 < S < W and W == 0 are
    refused with PGT_EARG before any device use."""
    if jackknife and (W == 0 or 0 < S < W):
        raise PgtError(_lib.PGT_EARG, f"dstat_window_pops: the block jackknife needs disjoint windows as its blocks: "
                                      f"winsize {W} must be positive and stepsize {S} at least the winsize")
    if not jackknife:
        win, rows, tot = _window_pops(_DSTAT_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
        return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=trio_order(len(freqs)))
    win, rows, tot, jack = _trio_window_pops_jackknife(_DSTAT_POPS, DSTAT_JACK_DTYPE, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    res = _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=trio_order(len(freqs)))
    res["jackknife"] = {ijk: jack[t] for t, ijk in enumerate(trio_order(len(freqs)))}
    return res


def fd_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                   chr_len=None, skip_missing: int = 0, ctx: Context | None = None) -> dict:
    """Windowed f_d (Martin et al. 2015) and f_dM (Malinsky et al. 2015) for ALL trios of the first len(freqs) - 1 already
    synchronised populations against the LAST one, the outgroup (4 ... 7 populations), in one pass: {(i, j, k): WindowResult}
    in trio_order, with rows of (start, end, mid, n, fd, fdm, num, fd_den, fdm_den) and the genome-wide sums as total.
    f_d is meant for windows with D >= 0 (P3 -> P2); the row reports it whatever its sign.  f_dM covers both directions.
    Only the topology ((i,j),k) is computed, so the order of the columns chooses it.
    Window arguments and their errors are those of dstat_window_pops; -skip_missing drops a trio's rows without counted sites
    from that trio's result only.  The per-site definition is pgt_fd_pops_reduce_dev's (include/pgtwin.h)."""
    win, rows, tot = _window_pops(_FD_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=trio_order(len(freqs)))


def f3_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                   chr_len=None, skip_missing: int = 0, jackknife: bool = False, ctx: Context | None = None) -> dict:
    """Windowed f3 (Reich et al. 2009; Patterson et al. 2012) for ALL trios of len(freqs) already synchronised populations
    (3 ... 6; no outgroup), every population of a trio as the target, in one pass: {(i, j, k): WindowResult} in
    all_trio_order, with rows of (start, end, mid, n, reserved_, f3_i, f3_j, f3_k) and the genome-wide sums as total.  The
    three values are SUMS over the counted sites, one per target_order(i, j, k): f3 of a window is sum / n.  All columns must
    report the same allele.  A significantly negative f3(target; a, b) shows the target to be admixed between relatives of
    a and b; with an outgroup as the target the value measures the drift a and b share.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a trio's rows without counted sites
    from that trio's result only.  The per-site definition is pgt_f3_pops_reduce_dev's (include/pgtwin.h).
    jackknife=True: the result gains the key "jackknife": {(i, j, k): 3 F3_JACK_DTYPE, one per target_order(i, j, k)} — the
    delete-m_j block jackknife of the mean (pgt_f3_jackknife_dev, on the device rows of the same reduction) over ALL windows
    of the table as blocks, whatever skip_missing is.  The windows must be disjoint: 0 < S < W and W == 0 are refused with
    PGT_EARG before any device use.
    Not computed: f3 normalised by the target's heterozygosity, f4, user-chosen trio lists."""
    if jackknife and (W == 0 or 0 < S < W):
        raise PgtError(_lib.PGT_EARG, f"f3_window_pops: the block jackknife needs disjoint windows as its blocks: "
                                      f"winsize {W} must be positive and stepsize {S} at least the winsize")
    keys = all_trio_order(len(freqs))
    if not jackknife:
        win, rows, tot = _window_pops(_F3_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
        return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    win, rows, tot, jack = _trio_window_pops_jackknife(_F3_POPS, F3_JACK_DTYPE, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    res = _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    res["jackknife"] = {ijk: jack[t] for t, ijk in enumerate(keys)}
    return res


def _pbs_estimator(who: str, estimator) -> _PopsStat:
    st = _PBS_ESTIMATORS.get(estimator) if isinstance(estimator, str) else None
    if st is None:
        raise PgtError(_lib.PGT_EARG, f'{who}: estimator must be "wc" or "hudson", not {estimator!r}')
    return st


def pbs_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                    chr_len=None, skip_missing: int = 0, estimator: str = "wc", ctx: Context | None = None,
                    jackknife: bool = False) -> dict:
    """Windowed population branch statistic (Yi et al. 2010) for ALL trios of len(freqs) already synchronised populations
    (3 ... 6), every population of a trio as the focal one: {(i, j, k): WindowResult} in all_trio_order, with rows of (start,
    end, mid, n, pbs_i, pbs_j, pbs_k, num_ij, num_ik, num_jk, den_ij, den_ik, den_jk) and the genome-wide line as total.  The
    sums are those of the FST estimator ("wc" or "hudson", as fst_window_pops) over the sites where ALL THREE populations have
    minind individuals — not the pairs' own site sets, which is what fst_window_pops reports; fst_xy = num_xy / den_xy.
    Nothing is clamped: a negative FST gives a negative branch, FST = 1 gives inf, inf - inf gives nan.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a trio's rows without counted sites
    from that trio's result only.  The definition is pgt_pbs_pops_reduce_dev's (include/pgtwin.h).
    PBSn1 of rows or totals: pbsn1_of(rows).
    jackknife=True: the result gains the key "jackknife": {(i, j, k): 6 PBS_JACK_DTYPE, one per pbs_item_order(i, j, k)} — the
    delete-m_j block jackknife of PBS and PBSn1 of the genome-wide sums, all six sums losing a block together
    (pgt_pbs_jackknife_dev, on the device rows of the same reduction), over ALL windows of the table as blocks, whatever
    skip_missing is.  The windows must be disjoint: 0 < S < W and W == 0 are refused with PGT_EARG before any device use.
    Not computed: truncation of negative FST, user-chosen trio lists."""
    st = _pbs_estimator("pbs_window_pops", estimator)
    if jackknife and (W == 0 or 0 < S < W):
        raise PgtError(_lib.PGT_EARG, f"pbs_window_pops: the block jackknife needs disjoint windows as its blocks: "
                                      f"winsize {W} must be positive and stepsize {S} at least the winsize")
    keys = all_trio_order(len(freqs))
    if not jackknife:
        win, rows, tot = _window_pops(st, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
        return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    win, rows, tot, jack = _trio_window_pops_jackknife(st, PBS_JACK_DTYPE, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx, items=6,
                                                       jack_name="pbs", work_bytes="pgt_pbs_pops_work_bytes", work_word="work")
    res = _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    res["jackknife"] = {t: jack[n] for n, t in enumerate(keys)}
    return res


def f4_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                   chr_len=None, skip_missing: int = 0, jackknife: bool = False, ctx: Context | None = None) -> dict:
    """Windowed f4 (Reich et al. 2009; Patterson et al. 2012) for ALL quartets of len(freqs) already synchronised populations
    (4 ... 6; no outgroup), every quartet in its three pairings, in one pass: {(i, j, k, l): WindowResult} in
    all_quartet_order, with rows of (start, end, mid, n, reserved_, f4_ij_kl, f4_ik_jl, f4_il_jk) and the genome-wide sums as
    total.  The three values are SUMS over the counted sites, one per pairing_order(i, j, k, l): f4 of a window is sum / n.
    All columns must report the same allele.  f4(a, b; c, d) is 0 in expectation when ((a, b), (c, d)) is the tree: |Z| above
    about 3 rejects that tree.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a quartet's rows without counted sites
    from that quartet's result only.  The per-site definition is pgt_f4_pops_reduce_dev's (include/pgtwin.h).
    jackknife=True: the result gains the key "jackknife": {(i, j, k, l): 3 F4_JACK_DTYPE, one per pairing_order(i, j, k, l)} —
    the delete-m_j block jackknife of the mean (pgt_f4_jackknife_dev, on the device rows of the same reduction) over ALL
    windows of the table as blocks, whatever skip_missing is.  The windows must be disjoint: 0 < S < W and W == 0 are refused
    with PGT_EARG before any device use.
    Not computed: user-chosen quartet lists; f4-ratio admixture proportions come from f4ratio_window_pops."""
    if jackknife and (W == 0 or 0 < S < W):
        raise PgtError(_lib.PGT_EARG, f"f4_window_pops: the block jackknife needs disjoint windows as its blocks: "
                                      f"winsize {W} must be positive and stepsize {S} at least the winsize")
    keys = all_quartet_order(len(freqs))
    if not jackknife:
        win, rows, tot = _window_pops(_F4_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
        return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    win, rows, tot, jack = _trio_window_pops_jackknife(_F4_POPS, F4_JACK_DTYPE, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    res = _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    res["jackknife"] = {q: jack[t] for t, q in enumerate(keys)}
    return res


def f4ratio_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                        chr_len=None, skip_missing: int = 0, jackknife: bool = False, ctx: Context | None = None) -> dict:
    """Windowed f4-ratio (Patterson et al. 2012; ADMIXTOOLS' qpF4ratio) for ALL triples of the middle populations of len(freqs)
    already synchronised populations (5 ... 7): freqs[0] is A, freqs[-1] the outgroup O, and for every triple (i, j, k) of the
    populations between them, in one pass: {(i, j, k): WindowResult} in middle_triple_order, with rows of (start, end, mid, n,
    reserved_, g_ij, g_ik, g_jk) and the genome-wide sums as total.  The three values are SUMS of (p_A - p_O)(p_x - p_y) over
    the sites where ALL FIVE populations have minind individuals; alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C), the share of
    B-related ancestry in X, is a ratio of two of them: f4ratio_alphas(rows) gives the six of ratio_order(i, j, k), 0 where the
    denominator is 0, never clamped to [0, 1].  All columns must report the same allele.
    Window arguments and their errors are those of dxy_window_pops; -skip_missing drops a triple's rows without counted sites
    from that triple's result only.  The per-site definition is pgt_f4ratio_pops_reduce_dev's (include/pgtwin.h).
    jackknife=True: the result gains the key "jackknife": {(i, j, k): 6 F4RATIO_JACK_DTYPE, one per ratio_order(i, j, k)} — the
    delete-m_j block jackknife of the ratio, numerator and denominator losing a block together (pgt_f4ratio_jackknife_dev, on
    the device rows of the same reduction), over ALL windows of the table as blocks, whatever skip_missing is.  The windows must
    be disjoint: 0 < S < W and W == 0 are refused with PGT_EARG before any device use.
    Not computed: user-chosen quintet lists, 8 populations, qpAdm-style multi-source fits."""
    if jackknife and (W == 0 or 0 < S < W):
        raise PgtError(_lib.PGT_EARG, f"f4ratio_window_pops: the block jackknife needs disjoint windows as its blocks: "
                                      f"winsize {W} must be positive and stepsize {S} at least the winsize")
    keys = middle_triple_order(len(freqs))
    if not jackknife:
        win, rows, tot = _window_pops(_F4RATIO_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
        return _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    win, rows, tot, jack = _trio_window_pops_jackknife(_F4RATIO_POPS, F4RATIO_JACK_DTYPE, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx, items=6)
    res = _results_by_pair(len(freqs), win, rows, tot, skip_missing, "n", keys=keys)
    res["jackknife"] = {t: jack[n] for n, t in enumerate(keys)}
    return res


def pi_window_pops(chr_ids, pos, freqs, ninds, W: int = 0, S: int = 0, minind: int = 1, fixedsite: int = 0,
                   chr_len=None, ctx: Context | None = None) -> list:
    """Windowed nucleotide diversity (pi) of EACH of len(freqs) populations (1 ... 8; already synchronised when there are
    several) in one pass: a list of WindowResult, one per population, with dxyWindow's rows (sum = Σ pi over the counted
    sites, neff, nskip) and the genome-wide line as total.  Window arguments and their errors are those of dxy_window_pops.
    The reference has no counterpart; the per-site definition is pgt_pi_pops_reduce_dev's (include/pgtwin.h)."""
    win, rows, tot = _window_pops(_PI_POPS, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, ctx)
    return [WindowResult(win, rows[k], tot[k]) for k in range(len(freqs))]


def ihs_window(chr_ids, pos, score, W: int = 100000, cutoff: float = 2.0, chr_len=None,
               ctx: Context | None = None) -> WindowResult:
    """ihsWindow.cpp:123-221 over columns (defaults of ihsWindow.cpp:225-226): rows are
    (start, end, nsites, nbig, position, value); proportion = nbig / nsites."""
    if cutoff < 0:
        raise PgtError(_lib.PGT_EARG, "|iHS| cutoff must be >= zero")  # ihsWindow.cpp:60-63
    win = build_windows_extreme(pos, run_lengths(chr_ids), chr_len, W)
    ctx, own = _own_ctx(ctx)
    try:
        return WindowResult(win, ctx.extreme_reduce(pos, score, PGT_EXT_IHS, cutoff, win))
    finally:
        if own:
            ctx.close()


def xpehh_window(chr_ids, pos, score, cutoff: float, W: int = 100000, chr_len=None,
                 ctx: Context | None = None) -> WindowResult:
    """xpehhWindow.cpp:126-232 over columns: a negative cutoff looks for the minimum and counts
    scores below it, otherwise the maximum / above (xpehhWindow.cpp:210-216)."""
    win = build_windows_extreme(pos, run_lengths(chr_ids), chr_len, W)
    mode = PGT_EXT_XP_MIN if cutoff < 0 else PGT_EXT_XP_MAX
    ctx, own = _own_ctx(ctx)
    try:
        return WindowResult(win, ctx.extreme_reduce(pos, score, mode, cutoff, win))
    finally:
        if own:
            ctx.close()
