#!/usr/bin/env python3
"""f3 of all trios of K populations (f3_pops_reduce_dev) on one MI355X, beside Hudson's FST of all pairs of the same K on the
same columns and window table (fst_hudson_pops_reduce_dev — the same count transport, the same 12 B/site/population and the
same per-population term h): the two ALTERNATE in one process on one card.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {3, 4, 5, 6} (argv[2], comma separated, overrides).  Before
anything is timed the coordinates of the two calls' rows must be equal, a trio's count must not exceed the count of any of its
pairs (a site counted for the trio is counted for the pair), and where they are equal for the pair (i, j) of trio (i, j, k) the
row's f3_i + f3_j must lie within 1e-9 * 4 bsum + 1e-12 of Hudson's asum (bsum is Σ dxy of the pair, and a site's dxy is at
least |p_i - p_j| and at least p (1 - p) of either population, so 4 bsum bounds the Σ(|product| + |h|) of the two f3 sums
from above); a mismatch exits non-zero.
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
from popgenomicstools_amd._lib import F3_ROW_DTYPE, F3_TOTAL_DTYPE, FST_ROW_DTYPE, FST_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import all_trio_order, pair_order, rows_from_device, windows_to_device  # noqa: E402
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


def rows_agree(k, rf, rh):
    """the checks of the docstring on the rows of the two calls"""
    pairs = pair_order(k)
    for t, (i, j, kk) in enumerate(all_trio_order(k)):
        for a, b in ((i, j), (i, kk), (j, kk)):
            p = rh[pairs.index((a, b))]
            if not all(np.array_equal(rf[t][fld], p[fld]) for fld in ("start", "end", "mid")) or np.any(rf[t]["n"] > p["n"]):
                return False
        p = rh[pairs.index((i, j))]
        same = rf[t]["n"] == p["n"]
        gap = np.abs(rf[t]["f3_i"] + rf[t]["f3_j"] - p["asum"])
        if np.any(gap[same] > 1e-9 * 4.0 * p["bsum"][same] + 1e-12):
            return False
        if not all(np.all(np.isfinite(rf[t][fld])) for fld in ("f3_i", "f3_j", "f3_k")) or rf[t]["reserved_"].view(np.uint64).any():
            return False
    return True


def one_k(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    """the f3 call and Hudson's FST call alternately on the same columns -> one JSON line; False when their rows disagree"""
    tables = {"f3": len(all_trio_order(k)), "fst_hudson": len(pair_order(k))}
    shape = {"f3": (F3_ROW_DTYPE, F3_TOTAL_DTYPE, ctx.f3_pops_reduce_dev, ctx.f3_pops_tree_bytes(k, n)),
             "fst_hudson": (FST_ROW_DTYPE, FST_TOTAL_DTYPE, ctx.fst_hudson_pops_reduce_dev, ctx.fst_hudson_pops_tree_bytes(k, n))}
    out = {e: torch.empty(tables[e] * n_win * s[0].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tot = {e: torch.empty(tables[e] * s[1].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tree = {e: torch.empty(s[3], dtype=torch.uint8, device=dev) for e, s in shape.items()}
    leg = {e: (lambda e=e: shape[e][2](pos, f, c, minind, win, out=out[e], tot=tot[e], tree=tree[e])) for e in shape}
    for e in shape:
        leg[e]()
    torch.cuda.synchronize()
    rf = rows_from_device(out["f3"], F3_ROW_DTYPE).reshape(tables["f3"], n_win)
    rh = rows_from_device(out["fst_hudson"], FST_ROW_DTYPE).reshape(tables["fst_hudson"], n_win)
    if not rows_agree(k, rf, rh):
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
    res = {"k": k, "n_sites": n, "n_trios": tables["f3"], "n_pairs": tables["fst_hudson"], "n_win": int(n_win), "W": W, "S": S,
           "minind": minind, "rows_check": "ok", "steps_per_repetition": steps, "card": card}
    for e in shape:
        build = float(np.median([x[0] for x in bq[e]]))
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": build,
                  "query_ms": float(np.median([x[1] for x in bq[e]])),
                  "build_fraction_of_hbm_peak": 12.0 * k * n / (build * 1e-3) / HBM_PEAK}
    res["f3_build_over_hudson_build"] = res["f3"]["build_ms"] / res["fst_hudson"]["build_ms"]
    res["f3_query_over_hudson_query"] = res["f3"]["query_ms"] / res["fst_hudson"]["query_ms"]
    res["f3_step_over_hudson_step"] = res["f3"]["step_ms"] / res["fst_hudson"]["step_ms"]
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
