#!/usr/bin/env python3
"""FST of all pairs of K populations from their MAF columns on one MI355X: K(K-1)/2 two-population calls of fst_pops_reduce_dev
(leg a: one call per pair, 24 B/site/pair) against ONE K-population call (leg b: 12 B/site/population), in one process on one card.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {2, 4, 8}.  Before anything is timed, leg (b)'s rows are
compared with leg (a)'s (coordinates and counts exactly, sums within 1e-9 |y| + 1e-12); a mismatch exits non-zero.  Timing:
after a warm-up of every shape, the two legs ALTERNATE, 3 repetitions each; a repetition is as many back-to-back steps as
fill at least one second (the count is fixed after the warm-up and printed), timed by events on the launch stream; medians.
The build kernel's own time comes from the library's events (last_kernel_ms).  One JSON line per K on stdout.

--estimators (anywhere on the command line) runs another leg instead: the two estimators of the K-population call, Weir-Cockerham
(fst_pops_reduce_dev) and Hudson (fst_hudson_pops_reduce_dev), ALTERNATELY on the same columns, table and buffers in one
process; counts and coordinates of the two must be equal before anything is timed; whole steps by events as above, build and
query by the library's events, 7 alternating readings each after the warm-up; medians.  One JSON line per K."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popgenomicstools_amd as pgt  # noqa: E402
from popgenomicstools_amd._lib import FST_ROW_DTYPE, FST_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import pair_order, rows_from_device, windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402

REL, ABS = 1e-9, 1e-12
HBM_PEAK = 8e12  # bytes/s


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def estimator_leg(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    """WC and Hudson K-population calls alternately on the same columns -> one JSON line; False when their counts differ"""
    n_pairs = len(pair_order(k))
    calls = {"wc": ctx.fst_pops_reduce_dev, "hudson": ctx.fst_hudson_pops_reduce_dev}
    out = {e: torch.empty(n_pairs * n_win * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev) for e in calls}
    tot = {e: torch.empty(FST_TOTAL_DTYPE.itemsize * n_pairs, dtype=torch.uint8, device=dev) for e in calls}
    tree = torch.empty(ctx.fst_pops_tree_bytes(k, n), dtype=torch.uint8, device=dev)  # one buffer, the two in turn
    leg = {e: (lambda e=e: calls[e](pos, f, c, minind, win, out=out[e], tot=tot[e], tree=tree)) for e in calls}
    for e in calls:
        leg[e]()
    torch.cuda.synchronize()
    rw, rh = rows_from_device(out["wc"], FST_ROW_DTYPE), rows_from_device(out["hudson"], FST_ROW_DTYPE)
    if not all(np.array_equal(rw[fld], rh[fld]) for fld in ("start", "end", "mid", "n")):
        print(json.dumps({"k": k, "rows_check": "FAILED: counts or coordinates of the two estimators differ"}), flush=True)
        return False
    for _ in range(3):  # warm-up, discarded
        for e in calls:
            leg[e]()
    torch.cuda.synchronize()
    steps = {e: max(1, int(np.ceil(1000.0 / event_ms(leg[e], 3)))) for e in calls}
    step_ms = {e: [] for e in calls}
    for _ in range(3):  # alternating
        for e in calls:
            step_ms[e].append(event_ms(leg[e], steps[e]))
    ctx.set_profiling(True)
    bq = {e: [] for e in calls}
    for _ in range(7):  # alternating
        for e in calls:
            leg[e]()
            bq[e].append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    res = {"k": k, "n_sites": n, "n_pairs": n_pairs, "n_win": int(n_win), "W": W, "S": S, "minind": minind, "rows_check": "ok",
           "steps_per_repetition": steps, "card": card}
    for e in calls:
        build = float(np.median([x[0] for x in bq[e]]))
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": build,
                  "query_ms": float(np.median([x[1] for x in bq[e]])),
                  "build_fraction_of_hbm_peak": 12.0 * k * n / (build * 1e-3) / HBM_PEAK}
    res["hudson_build_over_wc_build"] = res["hudson"]["build_ms"] / res["wc"]["build_ms"]
    res["hudson_step_over_wc_step"] = res["hudson"]["step_ms"] / res["wc"]["step_ms"]
    print(json.dumps(res), flush=True)
    return True


def main():
    estimators = "--estimators" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--estimators"]
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [2, 4, 8]
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
    n_win = win_h.size
    ctx.set_max_window(W)
    pair_tree = torch.empty(ctx.fst_pops_tree_bytes(2, n), dtype=torch.uint8, device=dev)
    rc = 0
    for k in ks:
        pairs = pair_order(k)
        f, c = freqs[:k], ninds[:k]
        if estimators:
            if not estimator_leg(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
                rc = 1
                break
            continue
        out_a = torch.empty(len(pairs) * n_win * FST_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        out_b = torch.empty_like(out_a)
        tot_a = torch.empty(FST_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        tot_b = torch.empty(FST_TOTAL_DTYPE.itemsize * len(pairs), dtype=torch.uint8, device=dev)
        tree_b = torch.empty(ctx.fst_pops_tree_bytes(k, n), dtype=torch.uint8, device=dev)
        row_b = n_win * FST_ROW_DTYPE.itemsize

        def leg_a():
            for p, (i, j) in enumerate(pairs):
                ctx.fst_pops_reduce_dev(pos, [f[i], f[j]], [c[i], c[j]], minind, win, out=out_a[p * row_b:(p + 1) * row_b], tot=tot_a, tree=pair_tree)

        def leg_b():
            ctx.fst_pops_reduce_dev(pos, f, c, minind, win, out=out_b, tot=tot_b, tree=tree_b)

        # rows check before anything is timed
        leg_a()
        leg_b()
        torch.cuda.synchronize()
        ra, rb = rows_from_device(out_a, FST_ROW_DTYPE), rows_from_device(out_b, FST_ROW_DTYPE)
        exact = all(np.array_equal(ra[fld], rb[fld]) for fld in ("start", "end", "mid", "n"))
        within, max_rel = True, 0.0
        for fld in ("asum", "bsum", "fst"):
            diff = np.abs(rb[fld] - ra[fld])
            within = within and bool(np.all(diff <= REL * np.abs(ra[fld]) + ABS))
            max_rel = max(max_rel, float(np.max(diff / np.maximum(np.abs(ra[fld]), 1e-300))) if ra.size else 0.0)
        if not (exact and within):
            print(json.dumps({"k": k, "rows_check": "FAILED", "counts_and_coordinates_equal": exact, "sums_within_bound": within,
                              "max_rel_diff": max_rel}), flush=True)
            rc = 1
            break
        # warm-up of both shapes, then the step counts that fill a second
        for _ in range(3):
            leg_a()
            leg_b()
        torch.cuda.synchronize()
        steps_a = max(1, int(np.ceil(1000.0 / event_ms(leg_a, 3))))
        steps_b = max(1, int(np.ceil(1000.0 / event_ms(leg_b, 3))))
        ta, tb = [], []
        for _ in range(3):  # alternating
            ta.append(event_ms(leg_a, steps_a))
            tb.append(event_ms(leg_b, steps_b))
        ctx.set_profiling(True)
        bq = []
        for _ in range(7):
            leg_b()
            bq.append(ctx.last_kernel_ms())
        ctx.set_profiling(False)
        build_ms = float(np.median([x[0] for x in bq]))
        query_ms = float(np.median([x[1] for x in bq]))
        a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({
            "k": k, "n_sites": n, "n_pairs": len(pairs), "n_win": int(n_win), "W": W, "S": S, "minind": minind,
            "rows_check": "ok", "max_rel_diff_vs_pair_path": max_rel,
            "steps_per_repetition": {"pair_path": steps_a, "pops": steps_b},
            "pair_path_ms_per_step": a_ms, "pops_ms_per_step": b_ms, "pair_path_over_pops": a_ms / b_ms,
            "repetitions_ms": {"pair_path": ta, "pops": tb},
            "pops_build_ms": build_ms, "pops_query_ms": query_ms,
            "pops_build_fraction_of_hbm_peak": 12.0 * k * n / (build_ms * 1e-3) / HBM_PEAK,
            "card": card}), flush=True)
        del out_a, out_b, tree_b
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
