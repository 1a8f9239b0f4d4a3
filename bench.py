#!/usr/bin/env python3
"""bench.py — genomic sites/s of the 2-population FST window scan on MI355X (BASELINE.json metric).

Workload (BASELINE config 4 / north_star's target): ONE synthetic genome of --sites sites (default
10^9) in --chroms chromosomes (default 40), window 50000 sites / step 10000 sites, columns resident
in HBM when the timed region starts.  One step = one pass of the hot path over the whole genome:
build the range tree (the streaming pass over a,b: 16 B/site) + answer every window.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: it builds the columns, warms up (about PREWARM_S seconds of
untimed steps, then --warmup steps), times exactly --steps steps and prints the line; "ms_per_step" is one timed step.
Everything else this script measures or checks — the roofline events, the sanity and reference checks, the CPU
baseline, the 10^8-site configs, the sustained and exchange-overhead legs, telemetry and, for N > 1, rank 0's
single-GPU recomputation of the table — runs only with --full.  --dump-outputs DIR writes the rows of the timed path's
last step (the table a caller of the scan receives) as DIR/<field>.npy, float64, at most 64 MB in all; the inputs are
seeded, so two builds given the same arguments can be compared array for array.

Plain `python bench.py --gpus N` with N > 1 (no WORLD_SIZE in the environment) starts the N ranks itself:
the parent — which never touches the GPU and imports neither torch nor the library — runs the second
command above as a CHILD process on a free port of 127.0.0.1, relays its output and exits with its code.

N > 1 (one process per GPU): the window table is built once (identical on every rank) and cut by
pgt_plan_shards into N contiguous blocks; rank r materialises ONLY its own site range [site_lo,
site_hi) of the genome (counter-based generator keyed on the global site index, halo <= one window)
and reduces its block.  Rows reach rank 0 by an asynchronous double-buffered RCCL gather (--exchange auto, the
default: the transport north_star names, and the only one an unattended run takes) or by peer stores over xGMI into
rank 0's row buffer (no per-step collective; opt-in).  With --exchange both, BOTH transports are timed — the peer
stores after the gather's line has been secured — and, with --full, each assembled table is checked; "value" is the gather's
unless the peer-store run was verified bitwise in this very run AND was faster; both timings are in "extra"
(exchange_gather / exchange_peer).  STRONG scaling: total work is fixed at
--sites; value = --sites x steps / max-over-ranks time.  With --full, after each timed region rank 0 rebuilds the whole
genome (once), runs the single-GPU scan and demands the assembled multi-GPU table to be bitwise equal
("rows_check"); the table's SHA-256 ("rows_sha256") is the same for every N.  --scaling weak instead gives
every rank --sites sites (genome = N x --sites).

`--workload pairs --sites 1e8 --chroms 20` runs BASELINE configs[4] the same way: all 28 pairs of 8 populations
batched in one launch per step over one window table, site ranges sharded over the N GPUs, the 28 x windows
rows of every rank delivered to rank 0 and checked bit for bit against the single-GPU call.

Unattended N > 1 runs (the driver's): every phase — init / columns / gather timed / verify / roofline / peer timed (verify
and roofline with --full) —
is announced on stderr by every rank with its elapsed seconds and runs under its own deadline (PHASE_DEADLINES_S; a
watchdog thread per rank).  A phase that overruns ends the rank with exit code 124 and a line naming the phase, so a
wedged rank reads as "rank 3: phase 'gather timed' exceeded its deadline of 60 s", not as a driver timeout; only the
peer-store transport (opt-in: --exchange both / peer) is DEGRADABLE: once the gather's line is secured, a peer phase
that overruns makes rank 0 print that line with exchange_peer marked unavailable and every rank exit 0.  The collectives
run on RCCL (backend nccl) after a probe all-reduce that is given 60 s on a helper thread; if RCCL cannot be brought up
the ranks agree (over the gloo control group, which always exists) to stage the 4 MB of rows through the CPU instead and
say so at the top of the line ("degraded": true, "ok": false, the metric string names the fallback) and in
config.collective_backend.  Budget of `--gpus 8` on the 10^9-site genome: < 180 s in all — imports ~20 s,
init + probe ~15 s, columns ~5 s, gather timed ~1 s, rank 0's rebuild of the whole 20-GB genome + single-GPU scan ~15 s,
roofline ~1 s; the deadlines (sum 480 s) stay inside the driver's 600 s.

The N=1 run with --full also times BASELINE configs 2, 3 and 5 in their one-GPU form at 10^8 sites
("extra"; --headline-only skips them, e.g. under rocprofv3 --stats) and the reference CPU path on a
bounded sample ("cpu_baseline").  That leg is also the run's LIVE PARITY CHECK: the TSV the reference prints for the
sample (the first 5x10^7 sites = the first two chromosomes, ~5000 windows) is compared with the rows the timed GPU run
produced for those windows — "rows_check": {"against": "reference fstWindow ...", "windows": k, "equal": true}; a mismatch
gives "ok": false and exit code 3.  Round 6: the same check on the genome's LAST chromosomes (a second, untimed reference run beside
the timed one: the last windows and the end-of-file rule), a check of configs[2]'s het rows against the reference hetWindow
("extra.dxy_het_fused_1e8.rows_check"), the per-step cost of the multi-GPU row exchange priced on this one GPU
("extra.exchange_overhead") and the card's identity and telemetry ("extra.telemetry").  Prints ONE JSON line on rank 0 — and nothing
else on stdout (gloo's and RCCL's banners are sent to stderr).
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time


PREWARM_S = 0.5  # about this many seconds of untimed steps before the warm-up steps of every timed region (config.prewarm_steps)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sites", type=float, default=1e9, help="sites of the genome (strong scaling) or per GPU (--scaling weak)")
    ap.add_argument("--chroms", type=int, default=40, help="chromosomes of the genome (per GPU with --scaling weak)")
    ap.add_argument("--winsize", type=int, default=50_000)
    ap.add_argument("--stepsize", type=int, default=10_000)
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong")
    ap.add_argument("--exchange", choices=["auto", "gather", "peer", "both"], default="auto",
                    help="how rows reach rank 0 when N > 1: auto = gather = the asynchronous RCCL gather (the transport "
                         "north_star names); both = time the gather AND, afterwards, peer stores into rank 0's buffer, report "
                         "both, headline = gather unless peer was verified bitwise in this run and faster; peer = peer stores only")
    ap.add_argument("--cpu-sites", type=float, default=5e7,
                    help="sample size of the CPU baseline leg (5e7 sites = 1.6 GB of text, ~10 s of the reference tool)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--prewarm-seconds", type=float, default=PREWARM_S,
                    help="about this many seconds of untimed steps before the warm-up steps of every timed region (0: none, e.g. under "
                         "rocprofv3 --pmc, where every dispatch is serialised)")
    ap.add_argument("--headline-only", action="store_true",
                    help="skip the 10^8-site configs 2/3/5 (so that a rocprofv3 --stats average covers one size only)")
    ap.add_argument("--no-verify", action="store_true", help="N > 1: skip the single-GPU recomputation on rank 0")
    ap.add_argument("--no-exchange-overhead", action="store_true",
                    help="N = 1: skip the leg that prices the multi-GPU row exchange on an RCCL group of one rank (extra.exchange_overhead)")
    ap.add_argument("--exchange-steps", type=int, default=200, help="steps per figure of the exchange_overhead leg")
    ap.add_argument("--workload", choices=["fst", "pairs"], default="fst",
                    help="fst = the headline 2-population scan (default); pairs = BASELINE configs[4]: all --pairs population pairs "
                         "batched over one window table (use --sites 1e8 --chroms 20), sharded by site range like the headline")
    ap.add_argument("--pairs", type=int, default=28, help="population pairs of --workload pairs (8 populations = 28)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: roofline events, sanity and reference checks, CPU baseline, "
                         "the 10^8-site configs, the sustained and exchange-overhead legs, telemetry, and (N > 1) the single-GPU "
                         "recomputation on rank 0.  Without it: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the rows of the timed path's last step as DIR/<field>.npy (float64; at most 64 MB in all, a seeded "
                         "sample of the windows beyond that)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def self_launch(args) -> int:
    """`python bench.py --gpus N` (N > 1) without a launcher: start the N ranks as a child process group.
    Nothing in this process has touched the GPU (no HIP call, torch not even imported), and the ranks are
    CHILDREN (subprocess), never an exec of this process."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode  # stdout / stderr are inherited: rank 0's JSON line passes through


# ---- phases, deadlines, stderr log (stdlib only: usable before torch is imported) -----------------------------
# seconds; a deadline covers ONE entry of a phase.  PGT_BENCH_DEADLINE_SCALE scales them (tests use 0.1 … 0.3).
PHASE_DEADLINES_S = {"init": 120, "columns": 90, "gather timed": 60, "peer timed": 60, "local timed": 120, "verify": 120,
                     "roofline": 30, "extra configs": 600, "sustained": 120, "cpu baseline": 600, "exchange overhead": 120}
T_START = time.perf_counter()


class Phases:
    """`with phases("gather timed"):` — announces the phase on stderr (rank, seconds since start, seconds taken) and arms a
    watchdog for it.  On overrun the watchdog thread (the main thread may sit in a HIP or collective call that never
    returns) writes one line naming rank and phase and ends the process with os._exit: 124, or — when the phase was entered
    `degradable=True` — after rank 0 has printed the line secured so far (`secure()`), 0."""

    def __init__(self, rank=0, world=1, scale=None, stream=None):
        import threading
        self.rank, self.world = rank, world
        self.scale = float(os.environ.get("PGT_BENCH_DEADLINE_SCALE", "1")) if scale is None else scale
        self.stream = stream or sys.stderr
        self.taken = {}            # phase -> seconds (summed over entries)
        self.secured = None        # callable(reason) -> JSON text of the line as far as it is known (rank 0)
        self._lock = threading.Lock()
        self._armed = None         # (name, deadline instant, degradable)
        self._thread = threading.Thread(target=self._watch, daemon=True)
        self._stop = False
        self._thread.start()

    def say(self, msg):
        print(f"[bench r{self.rank}/{self.world} +{time.perf_counter() - T_START:6.1f}s] {msg}", file=self.stream, flush=True)

    def secure(self, make_line):
        self.secured = make_line

    def deadline_of(self, name):
        return PHASE_DEADLINES_S[name] * self.scale

    def _watch(self):
        while not self._stop:
            time.sleep(0.2)
            with self._lock:
                armed = self._armed
            if armed and time.perf_counter() > armed[1]:
                name, _, degradable = armed
                # rank 0 fires 3 s early in a degradable phase: its line must be out before a launcher that sees
                # another rank leave reaps the rest
                self.say(f"phase '{name}' exceeded its deadline of {self.deadline_of(name):.0f} s"
                         + (" — degrading to the result secured before it" if degradable else " — giving up (exit 124)"))
                if degradable:
                    if self.rank == 0 and self.secured is not None:
                        line = self.secured(f"phase '{name}' exceeded its deadline of {self.deadline_of(name):.0f} s")
                        sys.stdout.flush()
                        os.write(stdout_to_stderr.real_fd if stdout_to_stderr.real_fd is not None else 1, (line + "\n").encode())
                    os._exit(0)
                os._exit(124)

    def __call__(self, name, degradable=False):
        return _Phase(self, name, degradable)

    def close(self):
        self._stop = True


class _Phase:
    def __init__(self, ph, name, degradable):
        self.ph, self.name, self.degradable = ph, name, degradable

    def __enter__(self):
        ph = self.ph
        slack = 3.0 if (self.degradable and ph.rank == 0) else 0.0
        self.t0 = time.perf_counter()
        with ph._lock:
            ph._armed = (self.name, self.t0 + max(ph.deadline_of(self.name) - slack, 0.5), self.degradable)
        ph.say(f"{self.name}: start (deadline {ph.deadline_of(self.name):.0f} s)")
        fault_point(ph, self.name)
        return self

    def __exit__(self, et, ev, tb):
        ph = self.ph
        with ph._lock:
            ph._armed = None
        dt = time.perf_counter() - self.t0
        ph.taken[self.name] = ph.taken.get(self.name, 0.0) + dt
        ph.say(f"{self.name}: {'FAILED (' + et.__name__ + ')' if et else 'done'} in {dt:.2f} s")
        return False


class stdout_to_stderr:
    """File descriptor 1 -> 2 for the duration: gloo and RCCL print their banners ("[Gloo] Rank 0 is connected …", "RCCL version : …")
    with C stdio on STDOUT, where this script owes exactly ONE line, the JSON.  libc's buffers are flushed before the descriptor is
    given back, so nothing written meanwhile can surface on stdout later."""

    real_fd = None  # the process' real stdout while a redirection is in force (the watchdog's secured line goes THERE)

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        stdout_to_stderr.real_fd = self.saved
        return self

    def __exit__(self, *exc):
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        stdout_to_stderr.real_fd = None
        os.close(self.saved)
        return False


def fault_point(ph, name):
    """Test hook (tests/test_bench_script.py): PGT_BENCH_FAULT="<rank>:<phase>:<die|hang>" makes that rank die (exit 17) or
    hang at the start of that phase, as a wedged GPU or a lost peer would."""
    spec = os.environ.get("PGT_BENCH_FAULT")
    if not spec:
        return
    r, phase, what = spec.split(":")
    if int(r) == ph.rank and phase == name:
        ph.say(f"fault injected: {what} in phase '{name}'")
        if what == "die":
            os._exit(17)
        while True:
            time.sleep(1)


if __name__ == "__main__":
    _args = parse_args()
    if _args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(_args))

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # this pool's driver only supports dmabuf IPC (RCCL, hipIpc)
# one node: the rendezvous (127.0.0.1), gloo's pairs and RCCL's bootstrap all go over loopback — no dependence on the
# container's hostname resolving or on which interface a library would pick by itself
if os.path.isdir("/sys/class/net/lo"):
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import popgenomicstools_amd as pgt  # noqa: E402
from popgenomicstools_amd._lib import (DXY_ROW_DTYPE, FST_ROW_DTYPE, HET_ROW_DTYPE, PGT_STAT_DXY, PGT_STAT_FST,  # noqa: E402
                                       PGT_STAT_HET, WIN_DTYPE, PgtError)
from popgenomicstools_amd.distributed import RowExchange  # noqa: E402
from popgenomicstools_amd.window_scan import windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402
from gpu_telemetry import Telemetry, pci_bus_id_of  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy ceiling)
BYTES_PER_SITE = 16.0  # algorithmic: a,b f64 read once by the tree-build kernel
SEED = 12345


DUMP_LIMIT_BYTES = 60 << 20  # --dump-outputs: the arrays' payload stays below 64 MB with room for the .npy headers


def dump_outputs(out_dir, table, n_tables, n_windows):
    """--dump-outputs: the row table of the timed path's last step, one float64 array per field of FST_ROW_DTYPE
    (DIR/<field>.npy, shape (windows,), or (pairs, windows) with --workload pairs; the u32 fields are exact in float64).
    A table above DUMP_LIMIT_BYTES is cut to a fixed sample of its windows (seeded, sorted, the same windows in every
    table), whose indices go to DIR/window_index.npy."""
    rows = np.frombuffer(table.tobytes(), dtype=FST_ROW_DTYPE).reshape(n_tables, n_windows)
    fields = FST_ROW_DTYPE.names
    idx = None
    if n_tables * n_windows * len(fields) * 8 > DUMP_LIMIT_BYTES:
        keep = DUMP_LIMIT_BYTES // (n_tables * len(fields) * 8 + 8)
        idx = np.sort(np.random.default_rng(SEED).choice(n_windows, size=keep, replace=False))
        rows = rows[:, idx]
    os.makedirs(out_dir, exist_ok=True)
    for f in fields:
        col = rows[f].astype(np.float64)
        np.save(os.path.join(out_dir, f + ".npy"), col if n_tables > 1 else col[0])
    if idx is not None:
        np.save(os.path.join(out_dir, "window_index.npy"), idx.astype(np.float64))


def fmt_g6(x):
    """`%g` of C / the default ostream precision the reference prints with (fstWindow.cpp:88)."""
    return "%g" % x


def checker_tools():
    """oracle/ (test infrastructure): the text writers, the compiled reference binaries under oracle/_ref and the CPU port.
    bench.py uses them in exactly three places, all outside every timed region: cpu_baseline (the reported CPU number + the live
    parity check of the headline rows), het_rows_check (configs[2]) and pair_rows_check (configs[4]).  Never on the measured path."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_bind
    return oracle_bind


def check_rows_against_tsv(tsv_path, table, win, n_sample, against, row_dtype=None, value="fst", count="n", first_site=0):
    """The LIVE parity check of a timed run (fstWindow.cpp:69-107,150-152; hetWindow.cpp:66-105,148-150): the reference's TSV
    for the first n_sample sites against the rows the GPU produced for the whole genome in the timed run.  Comparable are
    the windows that end inside the sample (the streaming machine emits them before it can know what follows); what the
    reference prints after them belongs to the sample's truncated last chromosome.  Coordinates, midpoint, count and label
    exact; the statistic as printed (`%g`), or — on a rounding boundary of the six printed digits — printed from a value
    within 1e-9 relative.  row_dtype / value / count: FST rows (`fst`, `n`) by default; het rows are (`h`, `nonmissing`)."""
    rows = np.frombuffer(table.tobytes(), dtype=row_dtype or FST_ROW_DTYPE)[:win.size]  # pair 0 = the first table
    with open(tsv_path) as fh:
        ref_lines = fh.read().splitlines()
    if first_site:
        # a TAIL sample (sites [first_site, n) with first_site a chromosome start): a machine started there emits exactly the
        # full run's windows that begin at or behind first_site (those in front of it carry sites of the previous chromosome,
        # SURVEY Q1), up to and including the end-of-file rule (Q2) — every reference row must have its window
        at = int(np.count_nonzero(win["lo"] < first_site))
        assert np.all(win["lo"][at:] >= first_site), "windows beginning inside the tail sample are a suffix of the table"
        k = int(win.size - at)
        res = {"against": against, "windows": k, "reference_rows": len(ref_lines), "equal": False}
        if len(ref_lines) != k:
            res["mismatch"] = f"the reference printed {len(ref_lines)} rows for the tail sample, the GPU table has {k} windows beginning inside it"
            return res
    else:
        at = 0
        k = int(np.count_nonzero(win["hi"] <= n_sample))
        assert np.all(win["hi"][:k] <= n_sample), "windows ending inside the sample are a prefix of the table"
        res = {"against": against, "windows": k, "reference_rows": len(ref_lines), "equal": False}
        if len(ref_lines) < k:
            res["mismatch"] = f"the reference printed {len(ref_lines)} rows, the GPU table has {k} windows ending inside the sample"
            return res
    rounding_boundary = 0
    for i in range(k):
        r = rows[at + i]
        want = ["chr%d" % (int(win["label_run"][at + i]) + 1), str(int(r["start"])), str(int(r["end"])), str(int(r["mid"])), None, str(int(r[count]))]
        got = ref_lines[i].split("\t")
        f = float(r[value])
        ok = len(got) == 6 and all(w is None or w == g for w, g in zip(want, got))
        if ok and got[4] != fmt_g6(f):
            if got[4] in (fmt_g6(f * (1 + 1e-9)), fmt_g6(f * (1 - 1e-9))) or abs(float(got[4]) - f) <= 1e-9 * abs(f) + 1e-12:
                rounding_boundary += 1
            else:
                ok = False
        if not ok:
            want[4] = fmt_g6(f)
            res["mismatch"] = f"row {i}: reference {ref_lines[i]!r}, GPU {chr(9).join(want)!r}"
            return res
    res["equal"] = True
    res[value + "_on_a_rounding_boundary"] = rounding_boundary
    res["tsv_sha256"] = hashlib.sha256("\n".join(ref_lines[:k]).encode()).hexdigest()
    return res


def pair_rows_check(g8, pos, a, b, pair_table, win_h, W, S, pair, n_sample=20_000_000):
    """configs[4]'s live reference check (one-GPU form): the UNMODIFIED reference fstWindow on the first n_sample sites of ONE of the 28
    batched pairs (its `a`, `b` columns as text, ~4 s of the CPU tool, outside every timed region) against that pair's table of the
    batched call — that `grid.y` = pair p really reduced pair p's columns into table p (fstWindow.cpp:69-107)."""
    oracle_bind = checker_tools()
    ref = oracle_bind.ref_binary("fstWindow")
    orc = oracle_bind.load()
    tmpdir = tempfile.mkdtemp(prefix="pgt_bench_pair_")
    path, tsv = os.path.join(tmpdir, "sample.fst.txt"), os.path.join(tmpdir, "sample.fst.tsv")
    try:
        orc.write_fst_text(path, g8.chr_ids_np(0, n_sample), pos[:n_sample].cpu().numpy().view(np.uint32), a[:n_sample].cpu().numpy(),
                           b[:n_sample].cpu().numpy())
        t0 = time.perf_counter()
        if ref:
            with open(tsv, "w") as out_fh:
                subprocess.run([ref, path, str(W), str(S)], stdout=out_fh, check=True, timeout=300)
        else:
            assert orc.fst_text(path, W, S, tsv) == 0
        dt = time.perf_counter() - t0
        res = check_rows_against_tsv(tsv, pair_table, win_h, n_sample,
                                     "reference fstWindow (oracle/_ref/fstWindow, the unmodified reference source compiled)" if ref
                                     else "oracle port (oracle/liboracle.so; the reference binary did not travel)")
        res["sample"] = f"first {n_sample} sites of pair {pair} of 28 as text, {dt:.2f} s of the CPU tool"
        return res
    finally:
        for f_ in (path, tsv):
            if os.path.exists(f_):
                os.unlink(f_)
        os.rmdir(tmpdir)


def het_rows_check(g8, pos, g1, het_table, win_h, W, S, n_sample=20_000_000):
    """configs[2]'s live reference check: the UNMODIFIED reference hetWindow (oracle/_ref/hetWindow;
    hetWindow.cpp:66-105,148-150) on the first n_sample sites of the fused run's g1 column as text (~3 s, outside every timed
    region) against the het rows the fused dxy + het x2 kernel produced for those windows: coordinates, midpoint and the
    non-missing count exact, h as printed.  There is no dxy leg: no reference dxyWindow binary exists in this image."""
    oracle_bind = checker_tools()
    ref = oracle_bind.ref_binary("hetWindow")
    orc = oracle_bind.load()
    tmpdir = tempfile.mkdtemp(prefix="pgt_bench_het_")
    path, tsv = os.path.join(tmpdir, "sample.het.txt"), os.path.join(tmpdir, "sample.het.tsv")
    try:
        orc.write_het_text(path, g8.chr_ids_np(0, n_sample), pos[:n_sample].cpu().numpy().view(np.uint32), g1[:n_sample].cpu().numpy())
        t0 = time.perf_counter()
        if ref:
            with open(tsv, "w") as out_fh:
                subprocess.run([ref, path, str(W), str(S)], stdout=out_fh, check=True, timeout=300)
        else:
            assert orc.het_text(path, W, S, tsv) == 0
        dt = time.perf_counter() - t0
        res = check_rows_against_tsv(tsv, het_table, win_h, n_sample,
                                     "reference hetWindow (oracle/_ref/hetWindow, the unmodified reference source compiled)" if ref
                                     else "oracle port (oracle/liboracle.so; the reference binary did not travel)",
                                     row_dtype=HET_ROW_DTYPE, value="h", count="nonmissing")
        res["sample"] = f"first {n_sample} sites of g1 as text, {dt:.2f} s of the CPU tool"
        return res
    finally:
        for f_ in (path, tsv):
            if os.path.exists(f_):
                os.unlink(f_)
        os.rmdir(tmpdir)


def cpu_baseline(pos, a, b, genome, W, S, n_sample, ctx=None, extra=None, beside=None, table=None, win=None):
    """The reference CPU path on this box's host cores, on a bounded sample of the same workload:
    the first n_sample sites written as the tool's text input, then the UNMODIFIED reference binary
    (oracle/_ref/fstWindow, kind "reference") — or, if that binary did not travel, our restatement
    (oracle/liboracle.so, kind "port") — timed end to end, single-threaded like the reference.  Its TSV goes to a file
    (a few thousand rows) and is compared with the rows of the timed GPU run: -> (cpu_baseline, rows_check).
    beside: callable(done) run on the calling thread WHILE the CPU run goes on a worker thread (its clock is taken there):
    the sustained leg, which keeps the GPU busy for those ~12 s (one of this box's 256 cores launches kernels meanwhile)."""
    oracle_bind = checker_tools()
    orc = oracle_bind.load()
    n_sample = int(min(n_sample, a.numel()))
    hp = pos[:n_sample].cpu().numpy().view(np.uint32)
    ha, hb = a[:n_sample].cpu().numpy(), b[:n_sample].cpu().numpy()
    chr_ids = genome.chr_ids_np(0, n_sample)
    tmpdir = tempfile.mkdtemp(prefix="pgt_bench_")
    path = os.path.join(tmpdir, "sample.fst.txt")
    tsv = os.path.join(tmpdir, "sample.windows.tsv")
    orc.write_fst_text(path, chr_ids, hp, ha, hb)
    ref = oracle_bind.ref_binary("fstWindow")
    kind = "reference" if ref else "port"
    timing = {}
    # A second sample, NOT timed: the genome's last chromosomes (about n_sample sites), run beside the first on another core — its
    # TSV covers what the head sample cannot: the last windows of the genome and the end-of-file rule (fstWindow.cpp:150-152)
    n_all = int(a.numel())
    starts = genome.chr_start[genome.chr_start >= max(n_all - n_sample, n_sample)]
    tail_from = int(starts[0]) if (table is not None and starts.size and int(starts[0]) < n_all) else 0
    path_t, tsv_t = os.path.join(tmpdir, "tail.fst.txt"), os.path.join(tmpdir, "tail.windows.tsv")
    if tail_from:
        orc.write_fst_text(path_t, genome.chr_ids_np(tail_from, n_all), pos[tail_from:].cpu().numpy().view(np.uint32),
                           a[tail_from:].cpu().numpy(), b[tail_from:].cpu().numpy())

    def tail_run():
        try:
            if ref:
                with open(tsv_t, "w") as out_fh:
                    subprocess.run([ref, path_t, str(W), str(S)], stdout=out_fh, check=True)
            else:
                assert orc.fst_text(path_t, W, S, tsv_t) == 0
        except BaseException as e:  # noqa: BLE001
            timing["tail_error"] = e

    def cpu_run():
        t0 = time.perf_counter()
        try:
            if ref:
                with open(tsv, "w") as out_fh:
                    subprocess.run([ref, path, str(W), str(S)], stdout=out_fh, check=True)
            else:
                assert orc.fst_text(path, W, S, tsv) == 0  # a ctypes call: the GIL is released while it runs
            timing["dt"] = time.perf_counter() - t0
        except BaseException as e:  # noqa: BLE001 — reported on the calling thread
            timing["error"] = e

    import threading
    th = threading.Thread(target=cpu_run)
    th_tail = threading.Thread(target=tail_run) if tail_from else None
    th.start()
    if th_tail:
        th_tail.start()
    if beside is not None:
        beside(lambda: not th.is_alive())
    th.join()
    if th_tail:
        th_tail.join()
    if "error" in timing:
        raise timing["error"]
    if "tail_error" in timing:
        raise timing["tail_error"]
    dt = timing["dt"]
    if ctx is not None and extra is not None:
        # the same text through the device-side ingest (pgt_ingest_text): the parsed columns must equal the resident ones
        from popgenomicstools_amd._lib import PGT_TOK_CHR, PGT_TOK_F64, PGT_TOK_U32
        text = open(path, "rb").read()
        t1 = time.perf_counter()
        ing = ctx.ingest_text(text, [PGT_TOK_CHR, PGT_TOK_U32, PGT_TOK_F64, PGT_TOK_F64])
        t_ing = time.perf_counter() - t1
        assert ing.rows == n_sample and ing.bad_line == -1, ("ingest rows", ing.rows, n_sample, ing.bad_line)
        assert ing.run_len.tolist() == np.bincount(chr_ids).tolist(), ("ingest runs", ing.run_len.tolist()[:4])
        for tok, ref_col in ((1, hp), (2, ha), (3, hb)):  # == (the text cannot tell -0.0 written as 0.000000 apart)
            got = ing.column_np(tok)
            ne = np.flatnonzero(got != ref_col)
            assert ne.size == 0, ("ingest column", tok, int(ne.size), int(ne[0]), got[ne[0]], ref_col[ne[0]])
        extra["ingest_text"] = {"config": f"pgt_ingest_text on the CPU-baseline sample: {n_sample} lines, {len(text)} bytes of text -> pos, a, b "
                                          "columns on the GPU + chromosome runs (upload included)",
                                "seconds": t_ing, "lines_per_s": n_sample / t_ing, "text_GB_per_s": len(text) / t_ing / 1e9,
                                "columns_equal_resident": True}
        ing.free()
        del text
    rows_check = None
    if table is not None:
        rows_check = check_rows_against_tsv(tsv, table, win, n_sample,
                                            "reference fstWindow (oracle/_ref/fstWindow, the unmodified reference source compiled)" if ref
                                            else "oracle port (oracle/liboracle.so; the reference binary did not travel)")
        if tail_from:
            tail = check_rows_against_tsv(tsv_t, table, win, n_all, rows_check["against"], first_site=tail_from)
            rows_check["tail"] = {"sites": f"[{tail_from}, {n_all}): the last {n_all - tail_from} sites (the last chromosomes), the reference run beside "
                                           "the timed one on another core", **{k_: v_ for k_, v_ in tail.items() if k_ != "against"}}
            rows_check["windows"] += tail["windows"]
            rows_check["reference_rows"] += tail["reference_rows"]
            if not tail["equal"]:
                rows_check["equal"] = False
                rows_check["mismatch"] = "tail sample: " + tail.get("mismatch", "?")
    for f_ in (path, tsv, path_t, tsv_t):
        if os.path.exists(f_):
            os.unlink(f_)
    os.rmdir(tmpdir)
    return {"value": n_sample / dt, "unit": "sites/s", "cores": 1, "kind": kind,
            "sample": f"first {n_sample} sites of the workload as text ({'oracle/_ref/fstWindow' if ref else 'oracle port'} "
                      f"{W} {S}, parse included, stdout to a file, {dt:.2f} s); host has {os.cpu_count()} logical cores, "
                      f"the reference is single-threaded",
            "beside": (("the sustained GPU leg ran on another host thread meanwhile (one core launching kernels)" if beside is not None
                        else "nothing") + ("; a second, untimed reference run (the tail sample of rows_check) on another core" if tail_from else ""))}, rows_check


def timed_config(ctx, call, alg_bytes, reps=15):
    """One BASELINE config in its one-GPU form: median whole-step time from events on the launch stream
    (= torch's current stream) and the build kernel's own time from the library's HIP events."""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    step_ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
    ctx.set_profiling(True)
    bm = []
    for _ in range(reps):
        call()
        bm.append(ctx.last_kernel_ms()[0])
    ctx.set_profiling(False)
    build_ms = float(np.median(bm))
    return {"ms_per_step": step_ms, "build_kernel_ms": build_ms, "algorithmic_bytes": alg_bytes,
            "roofline_frac": alg_bytes / (build_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}


def sustained_leg(step, alg_bytes_per_step, sites, seconds=2.5, until=None, max_seconds=60.0, chunk_seconds=0.25):
    """>= `seconds` of back-to-back headline steps — and, with `until`, on until that callable says stop (the CPU baseline runs
    beside this leg: ~12 s) — WALL-timed between two device synchronisations, so that an outside sampler (rocm-smi, the driver's)
    sees the GPU busy and a clock droop under sustained load would show: the rate of every quarter second is reported beside the
    whole (HIP events between the chunks)."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 10
    per_chunk = max(1, int(np.ceil(chunk_seconds / per)))
    marks = [torch.cuda.Event(enable_timing=True)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks[0].record()
    while True:
        for _ in range(per_chunk):
            step()
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        marks[-1].synchronize()  # at most one chunk is queued ahead: the loop ends within a chunk of `until`
        el = time.perf_counter() - t0
        if el >= max_seconds or (el >= seconds and (until is None or until())):
            break
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    chunks = len(marks) - 1
    steps = per_chunk * chunks
    chunk_gbs = [alg_bytes_per_step * per_chunk / (marks[c].elapsed_time(marks[c + 1]) * 1e-3) / 1e9 for c in range(chunks)]
    return {"config": f"{steps} back-to-back steps of the headline workload, wall-clocked between two device synchronisations"
                      + (" — running beside the CPU baseline, for as long as that took" if until is not None else ""),
            "steps": steps, "wall_seconds": wall, "ms_per_step": wall / steps * 1e3, "sites_per_s": sites * steps / wall,
            "GB_per_s": alg_bytes_per_step * steps / wall / 1e9, "frac_of_hbm_peak": alg_bytes_per_step * steps / wall / 1e9 / HBM_PEAK_GBS,
            "chunks": chunks, "steps_per_chunk": per_chunk,
            "chunk_GB_per_s_min_median_max": [round(float(np.min(chunk_gbs)), 1), round(float(np.median(chunk_gbs)), 1), round(float(np.max(chunk_gbs)), 1)],
            "chunk_GB_per_s_first_10": [round(x, 1) for x in chunk_gbs[:10]], "chunk_GB_per_s_last_10": [round(x, 1) for x in chunk_gbs[-10:]],
            "first_vs_last_chunk": chunk_gbs[-1] / chunk_gbs[0]}


def extra_configs(ctx, dev, W, S, tree_pool, check_het=True):
    """BASELINE configs 2, 3, 5 (one-GPU forms) at 10^8 sites in 20 chromosomes, same generator."""
    n8 = 100_000_000
    g8 = SynthGenome(SEED, n8, 20)
    win_h = pgt.build_windows_sites(g8.run_len, W, S)
    win = windows_to_device(win_h, dev)
    nw = win_h.size
    ctx.set_max_window(W)
    out = {}
    pos, a, b = g8.fst_columns_t(0, n8, dev)
    rows = torch.empty(28 * nw * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    r = timed_config(ctx, lambda: ctx.fst_reduce_dev(pos, a, b, win, out=rows, tree=tree_pool), 16.0 * n8)
    r["sites_per_s"] = n8 / (r["ms_per_step"] * 1e-3)
    out["fst_1e8"] = dict(r, config="BASELINE configs[1]: fstWindow 2 pops x 1e8 sites, 1 GPU", kernel="fst_build_kernel")
    # config 3: dxyWindow + hetWindow of two genotype columns, one shared position column and window table
    p1, p2, n1, n2 = g8.dxy_columns_t(0, n8, dev)
    g1, g2 = g8.genotype_t(0, 0, n8, dev), g8.genotype_t(1, 0, n8, dev)
    r = timed_config(ctx, lambda: ctx.dxy_het_reduce_dev(pos, p1, p2, n1, n2, g1, g2, 5, win, tree=tree_pool), 26.0 * n8)
    r["sites_per_s"] = n8 / (r["ms_per_step"] * 1e-3)
    out["dxy_het_fused_1e8"] = dict(r, config="BASELINE configs[2]: dxyWindow + hetWindow x2, shared SoA, 1e8 sites, 1 GPU",
                                    kernel="dxy_het_build_kernel")
    if check_het:
        fused = ctx.dxy_het_reduce_dev(pos, p1, p2, n1, n2, g1, g2, 5, win, tree=tree_pool)
        torch.cuda.synchronize()
        out["dxy_het_fused_1e8"]["rows_check"] = het_rows_check(g8, pos, g1, fused[2].cpu().numpy(), win_h, W, S)
        del fused
    del p1, p2, n1, n2, g1, g2
    # the same 28 pairs from 8 allele-frequency columns: 64 B/site instead of 448
    fr = [g8.freq_t(k, 0, n8, dev) for k in range(8)]
    nsamp = [10.0 + k for k in range(8)]
    af_tree = torch.empty(int(pgt._lib.load().pgt_af_tree_bytes(8, n8)), dtype=torch.uint8, device=dev)
    r = timed_config(ctx, lambda: ctx.fst_af_reduce_dev(pos, fr, nsamp, win, out=rows, tree=af_tree), 64.0 * n8, reps=8)
    r["sites_per_s"] = n8 / (r["ms_per_step"] * 1e-3)
    out["af8_pairs28_1e8"] = dict(r, config="SURVEY 8(f2): 28 pairs from 8 allele-frequency columns x 1e8 sites (WCFst on device)",
                                  kernel="af_build_kernel<8>")
    del fr, af_tree
    # config 5, one-GPU form: 28 population pairs batched over one table (grid.y = pair)
    al, bl = [a], [b]
    for p in range(1, 28):
        pa, pb = g8.pair_columns_t(p, 0, n8, dev)
        al.append(pa)
        bl.append(pb)
    r = timed_config(ctx, lambda: ctx.fst_reduce_pairs_dev(pos, al, bl, win, out=rows, tree=tree_pool), 448.0 * n8, reps=6)
    r["sites_per_s"] = n8 / (r["ms_per_step"] * 1e-3)
    out["pairs28_1e8"] = dict(r, config="BASELINE configs[4], one-GPU form: fstWindow 28 pop-pairs x 1e8 sites batched",
                              kernel="fst_build_kernel (grid.y = 28)")
    if check_het:  # (the same switch: --no-cpu runs skip every leg that needs the CPU tools)
        torch.cuda.synchronize()
        p_ = 17
        tbl = rows[p_ * nw * FST_ROW_DTYPE.itemsize: (p_ + 1) * nw * FST_ROW_DTYPE.itemsize].cpu().numpy()
        out["pairs28_1e8"]["rows_check"] = pair_rows_check(g8, pos, al[p_], bl[p_], tbl, win_h, W, S, p_)
    del al, bl
    # ihsWindow-style extreme-score scan: one f64 score column, 100 kb windows
    from popgenomicstools_amd._lib import EXT_ROW_DTYPE, PGT_EXT_IHS
    ewin_h = pgt.build_windows_extreme(pos.cpu().numpy().view(np.uint32), g8.run_len, None, 100_000)
    ewin = windows_to_device(ewin_h, dev)
    erows = torch.empty(ewin_h.size * EXT_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    score = a * 40.0 - 2.0
    ctx.set_max_window(int((ewin_h["hi"] - ewin_h["lo"]).max()))
    r = timed_config(ctx, lambda: ctx.extreme_reduce_dev(pos, score, PGT_EXT_IHS, 2.0, ewin, out=erows, tree=tree_pool), 8.0 * n8)
    r["sites_per_s"] = n8 / (r["ms_per_step"] * 1e-3)
    out["ihs_extreme_1e8"] = dict(r, config="SURVEY 8(f3): ihsWindow-style extreme-score scan, 1e8 sites, 100 kb windows",
                                  kernel="ext_build_kernel")
    del score
    # S << W (fstWindow W=50000, S=1 and S=100) on 10^7 sites: the query strategies against one wave per window
    n7 = 10_000_000
    q = {}
    for S_ in (1, 100):
        win1_h = pgt.build_windows_sites(np.array([n7], dtype=np.uint64), W, S_)
        win1 = windows_to_device(win1_h, dev)
        rows1 = torch.empty(win1_h.size * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        # (name, step hint, longest-window hint): an unknown longest window (0) rules the group query out -> the sliding one
        for name, hint, mw in (("per_window", 0, W), ("sliding", S_, 0), ("group", S_, W)):
            if name == "sliding" and S_ > 32:
                continue
            ctx.set_max_window(mw)
            ctx.set_window_step(hint)
            ctx.set_profiling(True)
            t = []
            for _ in range(4):
                ctx.fst_reduce_dev(pos[:n7], a[:n7], b[:n7], win1, out=rows1, tree=tree_pool)
                t.append(ctx.last_kernel_ms()[1])
            ctx.set_profiling(False)
            q[f"S{S_}_{name}"] = float(np.median(t[1:]))
        q[f"S{S_}_windows"] = int(win1_h.size)
        del win1, rows1
    ctx.set_window_step(0)
    ctx.set_max_window(W)
    out["fst_1e7_small_step_query"] = {"config": "fstWindow 1e7 sites, W=50000, S=1 (9.95e6 windows) and S=100 (99501 windows): query kernel only, ms; "
                                                 "the product takes the group query for both (pgt_set_window_step <= 1024, windows >= 16384 sites)",
                                       **q}
    return out


def exchange_overhead(ctx, dev, dev_index, headline_cols, win, tree, W, S, ph, steps=200):
    """What the multi-GPU row exchange costs PER STEP, measured on this one GPU: the step of the
    8-GPU run — build + query of ONE shard (1/8 of the window table, pgt_plan_shards) — timed back to back with the rows
    left where the kernel wrote them ("local") and with the product's RowExchange(mode="gather") running exactly as it
    does between GPUs: torch.distributed.gather on an RCCL group (here: of one rank — gather to itself), asynchronous,
    two send buffers and two receive sets, the event waits of begin().  What is NOT in it: the wire (40 B x 12 500 rows
    = 0.5 MB per step and rank over xGMI) and waiting for slower ranks.  Three workloads: the headline's 8-GPU shard
    (1.25e8 sites), the whole 10^9-site genome (the N = 1 step with a 4-MB gather), and the 8-GPU shard of BASELINE
    configs[4] (28 pairs x 1.25e7 sites, 28 x the rows).  local and gather legs alternate (3 rounds), medians reported;
    the tables of both modes must be equal bit for bit."""
    from datetime import timedelta
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    t0 = time.perf_counter()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, timeout=timedelta(seconds=60))
    group = dist.new_group(backend="nccl", timeout=timedelta(minutes=5))  # nccl == RCCL on ROCm
    probe = torch.ones(1, dtype=torch.float32, device=dev)
    dist.all_reduce(probe, group=group)
    torch.cuda.synchronize()
    assert float(probe.item()) == 1.0
    bring_up = time.perf_counter() - t0
    K = max(20, int(steps))

    def one(scan_into, counts, tables, to_self):
        ex = RowExchange(ctx, counts, FST_ROW_DTYPE.itemsize, dev, dst=0, group=group, mode="gather", tables=tables,
                         coll_device=dev, gather_to_self=to_self)
        assert ex.mode == ("gather" if to_self else "local")

        def step():
            out = ex.begin()
            scan_into(out)
            ex.end()

        for _ in range(20):
            step()
        ex.flush()
        t_end = 0.0
        t1 = time.perf_counter()
        for _ in range(K):
            out = ex.begin()
            scan_into(out)
            te = time.perf_counter()
            ex.end()
            t_end += time.perf_counter() - te
        t_host = time.perf_counter() - t1  # the host has enqueued everything: how far it runs ahead of the GPU
        ex.flush()
        dt = time.perf_counter() - t1
        table = ex.finish()
        ex.close()
        return dt / K * 1e3, t_host / K * 1e3, t_end / K * 1e3, hashlib.sha256(table.tobytes()).hexdigest()

    side = torch.cuda.Stream(device=dev)

    def one_overlapped(scan_into, counts):
        """The SHAPE of the multi-GPU gather on this rank's launch stream, with a plain copy standing in for the transfer: per
        step one event recorded behind the query, the rows moved by ANOTHER stream that waits for that event (RCCL's stream
        does exactly this), two send buffers, and a stream-level wait only if the copy issued two steps ago has not finished.
        (torch's one-rank RCCL gather is not this shape: it runs its copy IN the launch stream — profiles/r06/exchange_trace_summary.md.)"""
        nbytes = max(int(counts[0]) * FST_ROW_DTYPE.itemsize, 1)
        bufs = [torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        recv = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        pending = [None, None]
        k = 0

        def step():
            nonlocal k
            if pending[k] is not None and not pending[k].query():
                torch.cuda.current_stream().wait_event(pending[k])
            scan_into(bufs[k])
            ev = torch.cuda.Event()
            ev.record()
            side.wait_event(ev)
            with torch.cuda.stream(side):
                recv[k].copy_(bufs[k], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
            pending[k] = done
            k ^= 1

        for _ in range(20):
            step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(K):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        return dt / K * 1e3, hashlib.sha256(recv[k ^ 1].cpu().numpy().tobytes()).hexdigest()

    def workload(name, scan_into, counts, tables, what):
        loc, gat, ovl, host_l, host_g, end_g, sha, sha_o = [], [], [], [], [], [], set(), set()
        for _ in range(3):
            ms, h, _e, d = one(scan_into, counts, tables, False)
            loc.append(ms)
            host_l.append(h)
            sha.add(d)
            ms, h, e, d = one(scan_into, counts, tables, True)
            gat.append(ms)
            host_g.append(h)
            end_g.append(e)
            sha.add(d)
            ms, d = one_overlapped(scan_into, counts)
            ovl.append(ms)
            sha_o.add(d)
        l_, g_, o_ = float(np.median(loc)), float(np.median(gat)), float(np.median(ovl))
        return {"config": what, "rows_per_step": int(counts[0]), "row_bytes_per_step": int(counts[0]) * FST_ROW_DTYPE.itemsize,
                "steps_per_figure": K, "local_ms_per_step": l_, "gather_ms_per_step": g_,
                "overhead_ms_per_step": g_ - l_, "overhead_frac_of_step": (g_ - l_) / l_,
                "overlapped_copy_ms_per_step": o_, "overlapped_copy_overhead_ms_per_step": o_ - l_,
                "overlapped_copy_overhead_frac_of_step": (o_ - l_) / l_,
                "local_ms_all": [round(x, 5) for x in loc], "gather_ms_all": [round(x, 5) for x in gat], "overlapped_copy_ms_all": [round(x, 5) for x in ovl],
                "host_enqueue_ms_per_step": {"local": float(np.median(host_l)), "gather": float(np.median(host_g)),
                                             "of_which_gather_call": float(np.median(end_g))},
                "tables_equal_bitwise": len(sha) == 1 and (tables > 1 or sha_o <= sha)}

    out = {"collective": "torch.distributed.gather on an RCCL (nccl) group of ONE rank, async_op, double-buffered (RowExchange mode 'gather', "
                         "gather_to_self) vs rows left in place ('local'); alternating legs, medians of 3.  NOTE: torch serves a one-rank gather "
                         "with a device-to-device copy enqueued IN the launch stream (kernel trace: the copy sits between query k and build k+1), "
                         "so 'gather' is the cost of handing the rows over with NOTHING overlapped — an upper bound; 'overlapped_copy' has the "
                         "shape the multi-GPU run has on every rank (an event behind the query, the rows moved by another stream)",
           "rccl_bring_up_seconds": round(bring_up, 2)}
    pos, a, b = headline_cols
    n_total = int(a.numel())
    # (a) the 8-GPU shard of the headline genome (rank 0's: sites [0, site_hi))
    sh8 = pgt.plan_shards(win, 8)[0]
    lo, hi = int(sh8["site_lo"]), int(sh8["site_hi"])
    assert lo == 0
    loc_w = np.array(win[int(sh8["win_begin"]): int(sh8["win_end"])], dtype=WIN_DTYPE, copy=True)
    wd8 = windows_to_device(loc_w, dev)
    p8, a8, b8 = pos[lo:hi], a[lo:hi], b[lo:hi]
    out["fst_shard_of_8"] = workload("fst", lambda o: ctx.fst_reduce_dev(p8, a8, b8, wd8, out=o, tree=tree), [loc_w.size], 1,
                                     f"rank 0's shard of the {n_total:.0e}-site headline genome cut 8 ways: {hi - lo} sites resident, "
                                     f"{loc_w.size} windows per step")
    # (b) the whole genome: the N = 1 step with its 4-MB table gathered every step
    wd1 = windows_to_device(win, dev)
    out["fst_whole_genome"] = workload("fst", lambda o: ctx.fst_reduce_dev(pos, a, b, wd1, out=o, tree=tree), [win.size], 1,
                                       f"the whole {n_total:.0e}-site genome, {win.size} windows per step")
    del wd8, wd1
    # (c) BASELINE configs[4] cut 8 ways: 28 pairs x 1.25e7 sites, 28 tables of rows per step
    n8 = min(100_000_000, n_total)  # (a smaller genome only in the tests' small runs)
    g8 = SynthGenome(SEED, n8, 20)
    win8 = pgt.build_windows_sites(g8.run_len, W, S)
    shp = pgt.plan_shards(win8, 8)[0]
    lo, hi = int(shp["site_lo"]), int(shp["site_hi"])
    loc_p = np.array(win8[int(shp["win_begin"]): int(shp["win_end"])], dtype=WIN_DTYPE, copy=True)
    wdp = windows_to_device(loc_p, dev)
    pp = g8.pos_t(lo, hi, dev)
    cols = [g8.pair_columns_t(k, lo, hi, dev) for k in range(28)]
    al, bl = [c[0] for c in cols], [c[1] for c in cols]
    out["pairs28_shard_of_8"] = workload("pairs", lambda o: ctx.fst_reduce_pairs_dev(pp, al, bl, wdp, out=o, tree=tree), [28 * loc_p.size], 28,
                                         f"rank 0's shard of BASELINE configs[4] (28 pairs x {n8:.0e} sites) cut 8 ways: {hi - lo} sites resident, "
                                         f"{loc_p.size} windows x 28 tables per step")
    del cols, al, bl, pp, wdp
    dist.destroy_process_group()
    return out


def kernel_source_sha256():
    """SHA-256 over the sources the build kernels are compiled from (what profiles/pmc_headline.json is keyed on)."""
    h = hashlib.sha256()
    for f in ("pgt_kernels.hip", "pgt_device.h"):
        with open(os.path.join(ROOT, "popgenomicstools_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def pmc_traffic(n, n_tables):
    """-> (HBM bytes per launch of the build kernel from the committed PMC passes, or None; where the figure comes from).
    profiles/pmc_headline.json is written by tools/collect_profiles.sh from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over
    the 10^9-site headline workload, together with the hash of the kernel sources it was measured on: a tree whose kernels
    have changed since reports null instead of a stale constant."""
    path = os.path.join(ROOT, "profiles", "pmc_headline.json")
    if not (n == 1_000_000_000 and n_tables == 1):
        return None, "null: the committed PMC passes cover the 10^9-site, one-pair headline workload only"
    try:
        with open(path) as fh:
            rec = json.load(fh)
    except (OSError, ValueError) as e:
        return None, f"null: {path} unreadable ({e})"
    if rec.get("kernel_source_sha256") != kernel_source_sha256():
        print("bench.py: WARNING: profiles/pmc_headline.json was measured on other kernel sources (hash differs): "
              "roofline.traffic = null; rerun tools/collect_profiles.sh", file=sys.stderr, flush=True)
        return None, "null: profiles/pmc_headline.json was measured on other kernel sources (SHA-256 of csrc/pgt_kernels.hip + pgt_device.h differs)"
    return float(rec["traffic_bytes_per_launch"]), (
        f"profiles/pmc_headline.json ({rec.get('collected', '?')}): rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes over "
        f"`{rec.get('command', '?')}`, {rec.get('dispatches', '?')} dispatches each: 2 x {rec.get('fetch_kib')} KiB (gfx950: FETCH_SIZE "
        f"reports half the bytes of a wide coalesced read, MI355X_MICROARCH.md 'HBM / rocprofv3') + {rec.get('write_kib')} KiB written; "
        "measured on kernel sources with the same SHA-256 as this tree's, not by this run")


def bring_up_collectives(world, rank, dev, ph):
    """-> (group for the data-path collectives, device their tensors live on, description).
    The default group is gloo over 127.0.0.1 (the control plane: agreement and verdict flags; it comes up wherever TCP does).
    RCCL (backend nccl) is a second group (created on the main thread, lazily), probed with one all-reduce on a helper thread
    that gets 60 s (at most half of the init deadline): if the probe fails or does not return on ANY rank, all ranks agree over
    gloo to stage the rows through the CPU instead — a DEGRADED run: "degraded": true at the top of the line, the metric
    string says so, "ok" is false (the number is not the RCCL result the run was asked for); exit code 0 so that the line is kept."""
    import threading
    from datetime import timedelta
    dist.init_process_group("gloo", timeout=timedelta(seconds=max(30.0, ph.deadline_of("init"))))
    want = os.environ.get("PGT_BENCH_BACKEND", "nccl")  # rehearsal knob: gloo = skip RCCL altogether
    if want != "nccl":
        return None, torch.device("cpu"), f"{want} (REHEARSAL: PGT_BENCH_BACKEND)"
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")  # an abandoned probe must not abort the process later
    box = {}
    # The GROUP is created here, on the main thread: new_group coordinates through the default (gloo) group and its store,
    # and that group must never be used from two threads at once (the fallback agreement below uses it too).  Only the probe
    # collective itself — the call that can hang when RCCL cannot reach a peer — runs on the helper thread.
    try:
        torch.cuda.set_device(dev)
        # no device_id: the communicator is then created lazily by the first collective — on the helper thread, where a hang
        # costs the probe its time share and nothing else (with device_id new_group itself would connect, here)
        box["group"] = dist.new_group(backend="nccl", timeout=timedelta(minutes=30))  # nccl == RCCL on ROCm
    except Exception as e:  # noqa: BLE001 — any failure means "no RCCL", the reason is reported
        box["error"] = f"{type(e).__name__}: {e}"

    def probe():
        try:
            fault_point(ph, "rccl probe")
            torch.cuda.set_device(dev)  # the current device is per thread
            t = torch.ones(1, dtype=torch.float32, device=dev)
            dist.all_reduce(t, group=box["group"])
            box["sum"] = float(t.item())
        except Exception as e:  # noqa: BLE001
            box["error"] = f"{type(e).__name__}: {e}"

    th = None
    if "group" in box:
        th = threading.Thread(target=probe, daemon=True)
        th.start()
        # half of the init deadline at most (the gloo bring-up above and the agreement below share it): a probe that never
        # returns must leave the fallback room to happen before the watchdog's exit 124
        th.join(min(60.0, 0.5 * ph.deadline_of("init")))  # a first RCCL bring-up on an eight-GPU node can take tens of seconds
    ok = 1 if (box.get("sum") == float(world)) else 0
    why = box.get("error") or ("probe all-reduce did not return in time" if th is not None and th.is_alive() else f"probe all-reduce gave {box.get('sum')}")
    flag = torch.tensor([ok], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)  # gloo; the helper thread, if still alive, sits inside RCCL, not in this group
    if int(flag.item()) == 1:
        return box["group"], dev, "nccl (RCCL)"
    ph.say("RCCL unusable on some rank" + (f" (here: {why})" if not ok else "") + " — rows will be staged through the CPU over gloo")
    return None, torch.device("cpu"), "gloo, rows staged through the CPU (FALLBACK: RCCL could not be brought up" + (f": {why}" if not ok else " on another rank") + ")"


def main():
    args = parse_args()
    pairs_mode = args.workload == "pairs"
    n_tables = args.pairs if pairs_mode else 1

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    ph = Phases(rank, world)
    ph.say(f"imports done; pid {os.getpid()}")
    # Rehearsal knobs for a one-GPU box (never set by the driver): PGT_BENCH_BACKEND=gloo skips RCCL (rows staged through
    # the CPU), PGT_BENCH_SHARE_GPU=1 puts every rank on GPU 0.  The measured configuration is always the default: one
    # GPU per rank, collectives on RCCL over xGMI.
    dev_index = 0 if os.environ.get("PGT_BENCH_SHARE_GPU") == "1" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    tel = Telemetry(pci_bus_id_of(dev_index)) if rank == 0 and args.full else None  # sysfs / amdsmi only: no HIP call, no process started
    telemetry = {"reader": tel.describe(), "at_start": tel.snapshot()} if tel else {}
    group, coll_dev, backend_desc = None, dev, "none (single GPU)"
    if world > 1:
        with ph("init"), stdout_to_stderr():
            group, coll_dev, backend_desc = bring_up_collectives(world, rank, dev, ph)
        ph.say("collectives: " + backend_desc)

    W, S = args.winsize, args.stepsize
    mult = world if args.scaling == "weak" else 1
    n_total = int(args.sites) * mult
    with ph("columns"):
        genome = SynthGenome(SEED, n_total, args.chroms * mult)
        win = pgt.build_windows_sites(genome.run_len, W, S)  # host, O(#windows), identical on every rank
        shards = pgt.plan_shards(win, world)
        sh = shards[rank]
        site_lo, site_hi = int(sh["site_lo"]), int(sh["site_hi"])
        local = np.array(win[int(sh["win_begin"]): int(sh["win_end"])], dtype=WIN_DTYPE, copy=True)
        local["lo"] -= site_lo
        local["hi"] -= site_lo
        n = site_hi - site_lo  # sites resident on this GPU (own block + halo)

        def load_columns(lo_, hi_):
            """-> (pos, [a per pair], [b per pair]) of sites [lo_, hi_) on this GPU"""
            if not pairs_mode:
                p_, a_, b_ = genome.fst_columns_t(lo_, hi_, dev)
                return p_, [a_], [b_]
            cols = [genome.pair_columns_t(k, lo_, hi_, dev) for k in range(n_tables)]
            return genome.pos_t(lo_, hi_, dev), [c[0] for c in cols], [c[1] for c in cols]

        mycols = load_columns(site_lo, site_hi)
        pos, a, b = mycols[0], mycols[1][0], mycols[2][0]
        win_d = windows_to_device(local, dev)
        ctx = pgt.Context(dev_index)
        ctx.set_max_window(int((win["hi"] - win["lo"]).max()))  # = W: tree levels above 8192 sites are not needed
        want_extra = args.full and world == 1 and not args.headline_only and not pairs_mode
        tree_bytes = max(ctx.tree_bytes(PGT_STAT_FST, n), 28 * ctx.tree_bytes(PGT_STAT_FST, 100_000_000),
                         ctx.tree_bytes(PGT_STAT_DXY, 100_000_000) + 2 * ctx.tree_bytes(PGT_STAT_HET, 100_000_000)) \
            if want_extra else n_tables * ctx.tree_bytes(PGT_STAT_FST, n)
        tree = torch.empty(tree_bytes, dtype=torch.uint8, device=dev)
        counts = (shards["win_end"] - shards["win_begin"]).astype(np.int64) * n_tables  # rows per rank and step
        ctx.set_window_step(S)  # the query strategy follows (W, S) of the whole table, not a rank's slice of it
        torch.cuda.synchronize()
    ph.say(f"{n} sites resident ({n * 20 * n_tables / 1e9:.2f} GB of columns), {int(counts[rank])} rows per step")

    def scan(cols, wtab, out, tree_):
        if pairs_mode:
            return ctx.fst_reduce_pairs_dev(cols[0], cols[1], cols[2], wtab, out=out, tree=tree_)
        return ctx.fst_reduce_dev(cols[0], cols[1][0], cols[2][0], wtab, out=out, tree=tree_)

    # about PREWARM_S seconds of steps, from the largest shard's size (identical on every rank)
    max_resident = max(int(s_["site_hi"] - s_["site_lo"]) for s_ in shards)
    prewarm_steps = int(min(500, max(20, args.prewarm_seconds / (max_resident * BYTES_PER_SITE * n_tables / 6.5e12 + 30e-6)))) \
        if args.prewarm_seconds > 0 else 0

    def timed_region(ex):
        def step():
            out = ex.begin()
            scan(mycols, win_d, out, tree)
            ex.end()

        def fence():
            ex.flush()
            if world > 1:
                if coll_dev.type == "cuda":  # RCCL: name this rank's device (the group was created without a bound one)
                    dist.barrier(group=group, device_ids=[dev_index])
                else:
                    dist.barrier(group=group)
            torch.cuda.synchronize()

        # bring the GPU to its steady state first: after the set-up phase (host-side table building, allocation) the first legs of a
        # process have read up to 3.5 % slower than the same steps two seconds later (profiles/r04/README.md); about PREWARM_S
        # seconds of untimed steps, then the W warm-up steps the caller asked for, then exactly K timed steps
        for k in range(prewarm_steps):  # the same count on every rank: every step issues its collective
            step()
            if k % 10 == 9:
                ex.flush()
        for _ in range(args.warmup):
            step()
        fence()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt_ = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt_], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            dt_ = float(t.item())
        return dt_

    # --- N > 1: every assembled table must be the single-GPU table, bit for bit -----------------
    single = {}

    def single_gpu_table():
        """rank 0: the whole genome on this one GPU through the same entry point (outside any timed region)."""
        if "t" not in single:
            fcols = load_columns(0, n_total)
            ftree = torch.empty(n_tables * ctx.tree_bytes(PGT_STAT_FST, n_total), dtype=torch.uint8, device=dev)
            fout = torch.empty(n_tables * win.size * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            scan(fcols, windows_to_device(win, dev), fout, ftree)
            single["t"] = fout.cpu().numpy().tobytes()
            del fcols, ftree, fout
            torch.cuda.empty_cache()
        return single["t"]

    can_verify = args.full and world > 1 and not args.no_verify and (args.scaling == "strong" or n_total <= 2_000_000_000)

    def run_transport(mode, degradable=False):
        """One row transport: timed region + the table of its last step + the bitwise check.  Collective."""
        with ph(f"{mode} timed", degradable=degradable):
            try:
                ex = RowExchange(ctx, counts, FST_ROW_DTYPE.itemsize, dev, dst=0, mode=mode, coll_device=coll_dev, tables=n_tables,
                                 group=group)
            except PgtError as e:  # peer: the buffer cannot be mapped by every rank (decided collectively)
                return {"mode": mode, "available": False, "why": str(e)}
            if tel and world == 1 and "timed_region" not in telemetry:  # a sampler thread beside the headline's timed region (prewarm included)
                telemetry["before_timed"] = tel.snapshot()
                with tel.sampling(period_s=0.05) as smp:
                    dt_ = timed_region(ex)
                telemetry["timed_region"] = smp.summary()
                telemetry["after_timed"] = tel.snapshot(light=True)
            elif tel and "before_timed" not in telemetry:  # N > 1: a reading before and after, no thread beside rank 0's launch loop
                telemetry["before_timed"] = tel.snapshot()
                dt_ = timed_region(ex)
                telemetry["after_timed"] = tel.snapshot()
            else:
                dt_ = timed_region(ex)
            table_ = ex.finish()  # rank 0: the assembled table of the last step (uint8 numpy)
        res = {"mode": ex.mode, "available": True, "dt": dt_, "table": table_, "verified": None}
        if world > 1 and args.full:
            with ph("verify", degradable=degradable):
                verdict = torch.zeros(1, dtype=torch.int32)
                if rank == 0 and can_verify:
                    verdict[0] = 0 if single_gpu_table() == table_.tobytes() else 1
                dist.broadcast(verdict, src=0)  # gloo control group
                res["verified"] = (int(verdict.item()) == 0) if can_verify else None
                ex.close()
        else:
            ex.close()
        return res

    def roofline_events():
        """The dominant kernel's average launch duration, by HIP events on the launch stream -> (build ms, query ms, detail).
        K back-to-back launches of the BUILD ALONE (the same entry point with an empty window table: nothing but the build kernel
        is launched) between two events, then K whole steps between two events: no event sits between two kernels, so the
        figures are those of the timed region's own launches (an event record between kernels costs each of them ~1 %: with
        the library's per-call profiling events build + query used to exceed the step they were part of).  query = step - build.
        The per-call profiling events are still taken and reported in `detail` for comparison."""
        with ph("roofline"):
            scratch = torch.empty(max(int(counts[rank]) * FST_ROW_DTYPE.itemsize, 1), dtype=torch.uint8, device=dev)
            no_win = win_d[:0]
            K = max(5, min(args.steps, 20))

            def avg_ms(fn):
                for _ in range(2):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / K

            build_only = avg_ms(lambda: scan(mycols, no_win, scratch, tree))
            whole_step = avg_ms(lambda: scan(mycols, win_d, scratch, tree))
            ctx.set_profiling(True)
            build_ms, query_ms = [], []
            for _ in range(K):
                scan(mycols, win_d, scratch, tree)
                bm, qm = ctx.last_kernel_ms()
                build_ms.append(bm)
                query_ms.append(qm)
            ctx.set_profiling(False)
        detail = {"launches_per_figure": K, "build_only_ms": build_only, "whole_step_ms": whole_step,
                  "per_call_profiling_events": {"build_ms": float(np.mean(build_ms)), "query_ms": float(np.mean(query_ms)),
                                                "note": "an event between the build and the query launch of every call: inflates both"}}
        return build_only, max(whole_step - build_only, 0.0), detail

    def assemble(runs, build_avg, query_avg, extra, cpu, note=None, ref_check=None):
        """rank 0: the JSON line from the transports that have run so far."""
        usable = [r for r in runs if r["available"]]
        good = [r for r in usable if r["verified"] is not False]
        # headline: the gather, unless peer stores were verified in this run and were faster; an unverifiable run
        # (--no-verify, genome too large to rebuild) never promotes peer stores
        head = good[0]
        for r in good[1:]:
            if r["mode"] == "peer" and r["verified"] and r["dt"] < head["dt"]:
                head = r
        dt, table, head_mode = head["dt"], head["table"], head["mode"]
        rows_check = ref_check  # N = 1: the reference's own TSV for the CPU-baseline sample against this run's rows (or None: --no-cpu)
        if world > 1:
            rows_check = ("bitwise equal to the single-GPU scan of the whole genome" if can_verify else
                          "skipped (checked with --full)" if not args.full else
                          ("skipped (--no-verify)" if args.no_verify else "skipped (weak-scaling genome too large to rebuild on one GPU)"))
        sha = hashlib.sha256(table.tobytes()).hexdigest()
        rows = np.frombuffer(table.tobytes(), dtype=FST_ROW_DTYPE)
        assert rows.size == n_tables * win.size  # table-major: pair 0's rows come first
        extra = dict(extra)
        for r in runs:
            key = "exchange_" + r["mode"]
            if not r["available"]:
                extra[key] = {"available": False, "why": r["why"]}
            elif world > 1:
                extra[key] = {"ms_per_step": r["dt"] / args.steps * 1e3, "sites_per_s": float(n_total) * args.steps / r["dt"],
                              "rows_check": ("bitwise equal" if r["verified"] else "DIFFERS") if r["verified"] is not None else "not verified",
                              "headline": r is head}
        if note:
            extra["note"] = note
        extra["phase_seconds"] = {k: round(v, 3) for k, v in ph.taken.items()}
        extra["seconds_since_start"] = round(time.perf_counter() - T_START, 2)
        roofline = None  # a plain run takes no roofline events (--full)
        if build_avg is not None:
            achieved = BYTES_PER_SITE * n_tables * n / (build_avg * 1e-3) / 1e9  # GB/s
            traffic, traffic_source = pmc_traffic(n, n_tables)
            roofline = {"bound": "hbm", "kernel": "fst_build_kernel", "achieved": achieved, "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                        "traffic_unit": "HBM bytes per launch of the build kernel (read + written)",
                        "traffic_source": traffic_source,
                        "kernel_ms": build_avg, "query_kernel_ms": query_avg, "measured": roof_detail,
                        "algorithmic_bytes_per_launch": BYTES_PER_SITE * n_tables * n, "sites_per_launch": n}
        per_gpu = [int(s_["site_hi"] - s_["site_lo"]) for s_ in shards]
        degraded = world > 1 and "FALLBACK" in backend_desc  # RCCL could not be brought up: rows went through the CPU over gloo
        line = {
            "metric": ("genomic sites/sec for 2-pop FST window scan" if not pairs_mode else
                       f"genomic sites/sec for the all-pairs FST window scan ({n_tables} population pairs per site)")
                      + (" — DEGRADED: rows staged through the CPU over gloo, RCCL unavailable" if degraded else ""),
            "value": float(n_total) * args.steps / dt,
            "unit": "sites/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            # every transport that ran delivered the single-GPU table (or was not verifiable by request)
            "ok": (all(r["verified"] is not False for r in usable) and (ref_check is None or bool(ref_check["equal"])) and not degraded
                   and bool(extra.get("dxy_het_fused_1e8", {}).get("rows_check", {"equal": True})["equal"])
                   and bool(extra.get("pairs28_1e8", {}).get("rows_check", {"equal": True})["equal"])),
            "degraded": degraded,
            "config": {"workload": (f"fstWindow 2 pops x {n_total:.0e} sites total" if not pairs_mode else
                                    f"fstWindow all {n_tables} pairs of 8 populations x {n_total:.0e} sites total, one batched call per step,")
                                   + f" in {genome.run_len.size} chromosomes"
                                   + (f" sharded x{world} by window blocks (pgt_plan_shards)" if world > 1 else "")
                                   + f", window {W} sites / step {S} sites, {win.size} windows, columns resident in HBM"
                                   + (f", rows to rank 0 by {'peer stores over xGMI' if head_mode == 'peer' else 'async gather'}"
                                      if world > 1 else ""),
                       "baseline_config": ("BASELINE configs[3] (10^9-site fstWindow scan sharded over the GPUs; at N=1 the same genome "
                                           "on one GPU: the size north_star's roofline target is quoted on); configs[1], [2], [4] in `extra`"
                                           if not pairs_mode else
                                           "BASELINE configs[4]: fstWindow all-pairs of 8 populations x 10^8 sites, pairs batched in one launch, "
                                           "site ranges sharded over the GPUs"),
                       "sites_total": n_total, "sites_resident_per_gpu": per_gpu, "winsize": W, "stepsize": S,
                       "windows": int(win.size), "seed": SEED, "row_exchange": head_mode, "collective_backend": backend_desc,
                       "prewarm_steps": prewarm_steps,
                       "parallelism": f"site-range shards x{world}" if world > 1 else "single GPU"},
            "rows_sha256": sha,
            "rows_check": rows_check,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "extra": extra,
        }
        return json.dumps(line)

    def sanity(table):
        """rank 0: a sample of its windows against float64 sums taken by torch (an independent path)."""
        rows = np.frombuffer(table.tobytes(), dtype=FST_ROW_DTYPE)
        mine = np.arange(int(sh["win_begin"]), int(sh["win_end"]))
        for i in mine[np.linspace(0, mine.size - 1, 7).astype(int)]:
            lo, hi = int(win["lo"][i]) - site_lo, int(win["hi"][i]) - site_lo
            ref = float(a[lo:hi].sum()) / float(b[lo:hi].sum())  # pair 0 = the first table
            assert abs(rows["fst"][i] - ref) <= 1e-9 * abs(ref) + 1e-12, (i, rows["fst"][i], ref)
            assert rows["n"][i] == hi - lo and rows["start"][i] == (int(pos[lo]) & 0xFFFFFFFF)

    if world == 1:
        modes = ["local"]
    else:
        modes = {"auto": ["gather"], "gather": ["gather"], "peer": ["peer"], "both": ["gather", "peer"]}[args.exchange]
    runs = [run_transport(modes[0])]
    if not runs[0]["available"]:
        raise SystemExit("bench.py: --exchange peer, but the row buffer cannot be mapped by every rank: " + runs[0]["why"])
    if runs[0]["verified"] is False:
        if rank == 0:
            print(f"bench.py: the table assembled by '{runs[0]['mode']}' differs from the single-GPU table of the same genome",
                  file=sys.stderr, flush=True)
        raise SystemExit(3)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, runs[0]["table"], n_tables, int(win.size))
    build_avg, query_avg, roof_detail = None, None, None
    if args.full:
        if rank == 0:
            sanity(runs[0]["table"])
        build_avg, query_avg, roof_detail = roofline_events()
    if len(modes) > 1:
        # the gather's line is secured: whatever the opt-in second transport does (a mapping that never returns, stores
        # that never land) can no longer cost the run its result
        if rank == 0:
            ph.secure(lambda why: assemble(runs + [{"mode": modes[1], "available": False, "why": why}], build_avg, query_avg, {}, None,
                                           note="second transport abandoned: " + why))
        runs.append(run_transport(modes[1], degradable=True))
        if runs[1]["available"] and runs[1]["verified"] is False and rank == 0:
            print(f"bench.py: the table assembled by '{runs[1]['mode']}' DIFFERS from the single-GPU table of the same genome "
                  "(\"ok\": false in the line)", file=sys.stderr, flush=True)

    extra, cpu, ref_check = {}, None, None
    if rank == 0 and world == 1 and not pairs_mode and args.full:
        if not args.headline_only:
            with ph("extra configs"):
                extra = extra_configs(ctx, dev, W, S, tree, check_het=not args.no_cpu)
                ctx.set_max_window(int((win["hi"] - win["lo"]).max()))
                ctx.set_window_step(S)
        sust_out = torch.empty(max(int(counts[rank]) * FST_ROW_DTYPE.itemsize, 1), dtype=torch.uint8, device=dev)

        def sustained(until=None):
            with tel.sampling(period_s=0.1) as smp:
                extra["sustained"] = sustained_leg(lambda: scan(mycols, win_d, sust_out, tree), BYTES_PER_SITE * n, n, until=until)
            telemetry["sustained"] = smp.summary()

        if args.no_cpu and not args.headline_only:
            with ph("sustained"):
                sustained()
        if not args.no_cpu:
            with ph("cpu baseline"):  # with the sustained leg beside it (not in --headline-only runs: rocprofv3 traces every dispatch)
                cpu, ref_check = cpu_baseline(pos, a, b, genome, W, S, args.cpu_sites, ctx, extra, beside=None if args.headline_only else sustained,
                                              table=runs[0]["table"], win=win)
        del sust_out
        if not args.headline_only and not args.no_exchange_overhead:
            # LAST, and degradable: everything else is in hand — should RCCL wedge on this box, the watchdog prints the line
            # without this leg (exit 0) instead of losing the run
            ph.secure(lambda why: assemble(runs, build_avg, query_avg, dict(extra, exchange_overhead={"available": False, "why": why},
                                                                             telemetry=telemetry), cpu, ref_check=ref_check))
            with ph("exchange overhead", degradable=True), stdout_to_stderr():
                try:
                    extra["exchange_overhead"] = exchange_overhead(ctx, dev, dev_index, (pos, a, b), win, tree, W, S, ph, steps=args.exchange_steps)
                except Exception as e:  # noqa: BLE001 — RCCL absent / refused: reported, the headline stands
                    extra["exchange_overhead"] = {"available": False, "why": f"{type(e).__name__}: {e}"}
    if tel:
        telemetry["at_end"] = tel.snapshot()
        extra = dict(extra, telemetry=telemetry)

    if rank == 0:
        print(assemble(runs, build_avg, query_avg, extra, cpu, ref_check=ref_check), flush=True)
    ph.say("line printed" if rank == 0 else "done")
    all_ok = all(r["verified"] is not False for r in runs if r["available"])
    ctx.close()
    ph.close()
    if ref_check is not None and not ref_check["equal"]:  # N = 1: the timed run's rows differ from the reference's TSV
        print("bench.py: rows of the timed run DIFFER from the reference's TSV on the CPU-baseline sample: " + ref_check.get("mismatch", "?"),
              file=sys.stderr, flush=True)
        sys.exit(3)
    het_check = extra.get("dxy_het_fused_1e8", {}).get("rows_check") if isinstance(extra, dict) else None
    if het_check is not None and not het_check["equal"]:  # configs[2]: the fused kernel's het rows differ from the reference's TSV
        print("bench.py: het rows of the fused dxy + het run DIFFER from the reference hetWindow's TSV: " + het_check.get("mismatch", "?"),
              file=sys.stderr, flush=True)
        sys.exit(3)
    pair_check = extra.get("pairs28_1e8", {}).get("rows_check") if isinstance(extra, dict) else None
    if pair_check is not None and not pair_check["equal"]:  # configs[4]: a pair's table of the batched call differs from the reference's TSV
        print("bench.py: rows of pair 17 of the batched 28-pair run DIFFER from the reference fstWindow's TSV: " + pair_check.get("mismatch", "?"),
              file=sys.stderr, flush=True)
        sys.exit(3)
    if world > 1:
        dist.barrier()
        sys.stdout.flush()
        sys.stderr.flush()
        # os._exit: no destructor of an abandoned RCCL probe (or of a half-built communicator) gets to hang the exit;
        # 3 = an explicitly requested transport delivered a table that differs ("ok": false in the line above)
        os._exit(0 if all_ok else 3)


if __name__ == "__main__":
    main()
