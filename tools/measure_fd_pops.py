#!/usr/bin/env python3
"""f_d / f_dM of all ingroup trios of K populations (fd_pops_reduce_dev) on one MI355X, beside the ABBA-BABA call of the same K
on the same columns and window table (dstat_pops_reduce_dev): the two ALTERNATE in one process on one card.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {4, 5, 6, 7} (argv[2], comma separated, overrides); the
last of the K populations is the outgroup.  Before anything is timed the coordinates and counts of the two calls' rows must
be equal, every row's num within 1e-9 (abba + baba) + 1e-12 of the D row's abba - baba, fdm_den >= 0 and |fdm| <= 1 + 1e-9; a
mismatch exits non-zero.
Timing: after a warm-up of both calls (discarded), the two legs alternate, 3 repetitions each; a repetition is as many
back-to-back steps as fill at least one second (the count is fixed after the warm-up and printed), timed by events on the
launch stream; build and query by the library's events, 7 alternating readings each; medians.  The build's share of the 8 TB/s
HBM peak is taken on the 12 K bytes per site the columns hold.  One JSON line per K on stdout."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popgenomicstools_amd as pgt  # noqa: E402
from popgenomicstools_amd._lib import DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, FD_ROW_DTYPE, FD_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import rows_from_device, trio_order, windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402

HBM_PEAK = 8e12  # bytes/s


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def one_k(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    """the f_d call and the ABBA-BABA call alternately on the same columns -> one JSON line; False when their rows disagree"""
    trios = trio_order(k)
    shape = {"fd": (FD_ROW_DTYPE, FD_TOTAL_DTYPE, ctx.fd_pops_reduce_dev, ctx.fd_pops_tree_bytes(k, n)),
             "dstat": (DSTAT_ROW_DTYPE, DSTAT_TOTAL_DTYPE, ctx.dstat_pops_reduce_dev, ctx.dstat_pops_tree_bytes(k, n))}
    out = {e: torch.empty(len(trios) * n_win * s[0].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tot = {e: torch.empty(len(trios) * s[1].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tree = {e: torch.empty(s[3], dtype=torch.uint8, device=dev) for e, s in shape.items()}
    leg = {e: (lambda e=e: shape[e][2](pos, f, c, minind, win, out=out[e], tot=tot[e], tree=tree[e])) for e in shape}
    for e in shape:
        leg[e]()
    torch.cuda.synchronize()
    rf = rows_from_device(out["fd"], FD_ROW_DTYPE).reshape(len(trios), n_win)
    rd = rows_from_device(out["dstat"], DSTAT_ROW_DTYPE).reshape(len(trios), n_win)
    ok = all(np.array_equal(rf[fld], rd[fld]) for fld in ("start", "end", "mid", "n"))
    ok = ok and bool(np.all(np.abs(rf["num"] - (rd["abba"] - rd["baba"])) <= 1e-9 * (rd["abba"] + rd["baba"]) + 1e-12))
    ok = ok and bool(np.all(rf["fdm_den"] >= 0) and np.all(np.abs(rf["fdm"]) <= 1 + 1e-9) and np.all(np.isfinite(rf["fd"])))
    if not ok:
        print(json.dumps({"k": k, "rows_check": "FAILED: the rows of the two calls disagree"}), flush=True)
        return False
    for _ in range(3):  # warm-up, discarded
        for e in shape:
            leg[e]()
    torch.cuda.synchronize()
    steps = {e: max(1, int(np.ceil(1000.0 / event_ms(leg[e], 3)))) for e in shape}
    step_ms = {e: [] for e in shape}
    for _ in range(3):  # alternating
        for e in shape:
            step_ms[e].append(event_ms(leg[e], steps[e]))
    ctx.set_profiling(True)
    bq = {e: [] for e in shape}
    for _ in range(7):  # alternating
        for e in shape:
            leg[e]()
            bq[e].append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    res = {"k": k, "n_sites": n, "n_trios": len(trios), "n_win": int(n_win), "W": W, "S": S, "minind": minind,
           "rows_check": "ok", "steps_per_repetition": steps, "card": card}
    for e in shape:
        build = float(np.median([x[0] for x in bq[e]]))
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": build,
                  "query_ms": float(np.median([x[1] for x in bq[e]])),
                  "build_fraction_of_hbm_peak": 12.0 * k * n / (build * 1e-3) / HBM_PEAK}
    res["fd_build_over_dstat_build"] = res["fd"]["build_ms"] / res["dstat"]["build_ms"]
    res["fd_query_over_dstat_query"] = res["fd"]["query_ms"] / res["dstat"]["query_ms"]
    res["fd_step_over_dstat_step"] = res["fd"]["step_ms"] / res["dstat"]["step_ms"]
    print(json.dumps(res), flush=True)
    return True


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 5, 6, 7]
    dev = torch.device("cuda", 0)
    W, S, minind = 50_000, 10_000, 5
    ctx = pgt.Context(0)
    props = torch.cuda.get_device_properties(0)
    card = {"name": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
            "hip": torch.version.hip}
    genomes = [SynthGenome(12345 + q, n, 20) for q in range((max(ks) + 1) // 2)]
    pos = genomes[0].pos_t(0, n, dev)
    freqs, ninds = [], []
    for g in genomes:
        p1, p2, n1, n2 = g.dxy_columns_t(0, n, dev)
        freqs += [p1, p2]
        ninds += [n1, n2]
    win_h = pgt.build_windows_sites(genomes[0].run_len, W, S)
    win = windows_to_device(win_h, dev)
    ctx.set_max_window(W)
    rc = 0
    for k in ks:
        if not one_k(ctx, k, n, pos, freqs[:k], ninds[:k], minind, win, win_h.size, dev, card, W, S):
            rc = 1
            break
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
