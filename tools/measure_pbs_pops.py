#!/usr/bin/env python3
"""The population branch statistic of all trios of K populations (pbs_pops_reduce_dev, both estimators) on one MI355X, beside
Hudson's FST of all pairs (fst_hudson_pops_reduce_dev) and f3 of all trios (f3_pops_reduce_dev) of the same K on the same columns
and window table: the four ALTERNATE in one process on one card.  A PBS call is two passes of the walk f3 makes once (three
sums per trio each) and a finishing kernel, so its step is read against two f3 steps.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {3, 4, 5, 6} (argv[2], comma separated, overrides).  Before
anything is timed the coordinates of all calls' rows must be equal, a trio's count must equal f3's and not exceed the count of
any of its pairs, and where it equals the count of the pair (i, j) the Hudson rows' num_ij and den_ij must lie within
2 (1e-9 * 4 bsum + 1e-12) of that pair's asum and bsum (a site's dxy bounds every term of its numerator from above); a mismatch
exits non-zero.
Timing: after a warm-up of all calls (discarded), the legs alternate, 3 repetitions each; a repetition is as many back-to-back
steps as fill at least one second (the count is fixed after the warm-up and printed), timed by events on the launch stream;
build and query by the library's events, 7 alternating readings each; medians.  For a PBS call the library's "build" is the
first pass and the second pass's build, its "query" the second query and the finish.  One JSON line per K on stdout."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popgenomicstools_amd as pgt  # noqa: E402
from popgenomicstools_amd._lib import F3_ROW_DTYPE, F3_TOTAL_DTYPE, FST_ROW_DTYPE, FST_TOTAL_DTYPE, PBS_ROW_DTYPE, PBS_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import all_trio_order, pair_order, rows_from_device, windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rows_agree(k, rp, rf, rh):
    """the checks of the docstring: rp the Hudson PBS rows, rf the f3 rows, rh the rows of Hudson's FST of all pairs"""
    pairs = pair_order(k)
    for t, (i, j, kk) in enumerate(all_trio_order(k)):
        if not all(np.array_equal(rp[t][fld], rf[t][fld]) for fld in ("start", "end", "mid", "n")):
            return False
        for a, b in ((i, j), (i, kk), (j, kk)):
            p = rh[pairs.index((a, b))]
            if not all(np.array_equal(rp[t][fld], p[fld]) for fld in ("start", "end", "mid")) or np.any(rp[t]["n"] > p["n"]):
                return False
        p = rh[pairs.index((i, j))]
        same = rp[t]["n"] == p["n"]
        bound = 2 * (1e-9 * 4.0 * p["bsum"][same] + 1e-12)
        if np.any(np.abs(rp[t]["num_ij"] - p["asum"])[same] > bound) or np.any(np.abs(rp[t]["den_ij"] - p["bsum"])[same] > bound):
            return False
    return True


def one_k(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    T, P = len(all_trio_order(k)), len(pair_order(k))
    wb = ctx.pbs_pops_work_bytes(k, n, n_win)
    shape = {  # leg -> (row dtype, total dtype, tables, workspace bytes, call)
        "pbs_wc": (PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, T, wb, lambda o, t, w: ctx.pbs_pops_reduce_dev(pos, f, c, minind, win, estimator="wc", out=o, tot=t, work=w)),
        "pbs_hudson": (PBS_ROW_DTYPE, PBS_TOTAL_DTYPE, T, wb, lambda o, t, w: ctx.pbs_pops_reduce_dev(pos, f, c, minind, win, estimator="hudson", out=o, tot=t, work=w)),
        "fst_hudson": (FST_ROW_DTYPE, FST_TOTAL_DTYPE, P, ctx.fst_hudson_pops_tree_bytes(k, n), lambda o, t, w: ctx.fst_hudson_pops_reduce_dev(pos, f, c, minind, win, out=o, tot=t, tree=w)),
        "f3": (F3_ROW_DTYPE, F3_TOTAL_DTYPE, T, ctx.f3_pops_tree_bytes(k, n), lambda o, t, w: ctx.f3_pops_reduce_dev(pos, f, c, minind, win, out=o, tot=t, tree=w)),
    }
    out = {e: torch.empty(s[2] * n_win * s[0].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tot = {e: torch.empty(s[2] * s[1].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    work = {e: torch.empty(s[3], dtype=torch.uint8, device=dev) for e, s in shape.items()}
    leg = {e: (lambda e=e: shape[e][4](out[e], tot[e], work[e])) for e in shape}
    for e in shape:
        leg[e]()
    torch.cuda.synchronize()
    rows = {e: rows_from_device(out[e], s[0]).reshape(s[2], n_win) for e, s in shape.items()}
    if not rows_agree(k, rows["pbs_hudson"], rows["f3"], rows["fst_hudson"]) or not np.array_equal(rows["pbs_wc"]["n"], rows["pbs_hudson"]["n"]):
        print(json.dumps({"k": k, "rows_check": "FAILED: the rows of the calls disagree"}), flush=True)
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
    res = {"k": k, "n_sites": n, "n_trios": T, "n_pairs": P, "n_win": int(n_win), "W": W, "S": S, "minind": minind,
           "rows_check": "ok", "steps_per_repetition": steps, "card": card}
    for e in shape:
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": float(np.median([x[0] for x in bq[e]])),
                  "query_ms": float(np.median([x[1] for x in bq[e]]))}
    for e in ("pbs_wc", "pbs_hudson"):
        res[f"{e}_step_over_two_f3_steps"] = res[e]["step_ms"] / (2 * res["f3"]["step_ms"])
        res[f"{e}_step_over_hudson_fst_step"] = res[e]["step_ms"] / res["fst_hudson"]["step_ms"]
    print(json.dumps(res), flush=True)
    return True


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [3, 4, 5, 6]
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
