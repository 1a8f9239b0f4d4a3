#!/usr/bin/env python3
"""f4 of all quartets of K populations (f4_pops_reduce_dev) on one MI355X, beside f3 of all trios of the same K on the same
columns and window table (f3_pops_reduce_dev — the same walk, the same 12 B/site/population, three sums per item; f3 carries
C(K, 3) items, the counts as values and a division per population, f4 C(K, 4) items and the counts as bits): the two ALTERNATE
in one process on one card.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {4, 5, 6} (argv[2], comma separated, overrides).  Before
anything is timed the coordinates of the two calls' rows must be equal, a quartet's count must not exceed the count of any of
its trios (a site counted for the quartet is counted for the trio), every sum must be finite, reserved_ must be +0.0, and a row's
three sums must cancel, |s0 - s1 + s2| <= 3 (1e-9 n + 1e-12) with n the row's counted sites (every product is at most 1 in
magnitude, so n bounds the Σ|product| of each sum from above); a mismatch exits non-zero.
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
from popgenomicstools_amd._lib import F3_ROW_DTYPE, F3_TOTAL_DTYPE, F4_ROW_DTYPE, F4_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import all_quartet_order, all_trio_order, rows_from_device, windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402

HBM_PEAK = 8e12  # bytes/s
SUMS = ("f4_ij_kl", "f4_ik_jl", "f4_il_jk")


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rows_agree(k, r4, r3):
    """the checks of the docstring on the rows of the two calls"""
    trios = all_trio_order(k)
    for t, q in enumerate(all_quartet_order(k)):
        for a in range(4):
            p = r3[trios.index(tuple(x for i, x in enumerate(q) if i != a))]
            if not all(np.array_equal(r4[t][fld], p[fld]) for fld in ("start", "end", "mid")) or np.any(r4[t]["n"] > p["n"]):
                return False
        if not all(np.all(np.isfinite(r4[t][fld])) for fld in SUMS) or r4[t]["reserved_"].view(np.uint64).any():
            return False
        gap = np.abs(r4[t][SUMS[0]] - r4[t][SUMS[1]] + r4[t][SUMS[2]])
        if np.any(gap > 3.0 * (1e-9 * r4[t]["n"] + 1e-12)):
            return False
    return True


def one_k(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    """the f4 call and the f3 call alternately on the same columns -> one JSON line; False when their rows disagree"""
    tables = {"f4": len(all_quartet_order(k)), "f3": len(all_trio_order(k))}
    shape = {"f4": (F4_ROW_DTYPE, F4_TOTAL_DTYPE, ctx.f4_pops_reduce_dev, ctx.f4_pops_tree_bytes(k, n)),
             "f3": (F3_ROW_DTYPE, F3_TOTAL_DTYPE, ctx.f3_pops_reduce_dev, ctx.f3_pops_tree_bytes(k, n))}
    out = {e: torch.empty(tables[e] * n_win * s[0].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tot = {e: torch.empty(tables[e] * s[1].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tree = {e: torch.empty(s[3], dtype=torch.uint8, device=dev) for e, s in shape.items()}
    leg = {e: (lambda e=e: shape[e][2](pos, f, c, minind, win, out=out[e], tot=tot[e], tree=tree[e])) for e in shape}
    for e in shape:
        leg[e]()
    torch.cuda.synchronize()
    r4 = rows_from_device(out["f4"], F4_ROW_DTYPE).reshape(tables["f4"], n_win)
    r3 = rows_from_device(out["f3"], F3_ROW_DTYPE).reshape(tables["f3"], n_win)
    if not rows_agree(k, r4, r3):
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
    res = {"k": k, "n_sites": n, "n_quartets": tables["f4"], "n_trios": tables["f3"], "n_win": int(n_win), "W": W, "S": S,
           "minind": minind, "rows_check": "ok", "steps_per_repetition": steps, "card": card}
    for e in shape:
        build = float(np.median([x[0] for x in bq[e]]))
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": build,
                  "query_ms": float(np.median([x[1] for x in bq[e]])),
                  "build_fraction_of_hbm_peak": 12.0 * k * n / (build * 1e-3) / HBM_PEAK}
    res["f4_build_over_f3_build"] = res["f4"]["build_ms"] / res["f3"]["build_ms"]
    res["f4_query_over_f3_query"] = res["f4"]["query_ms"] / res["f3"]["query_ms"]
    res["f4_step_over_f3_step"] = res["f4"]["step_ms"] / res["f3"]["step_ms"]
    print(json.dumps(res), flush=True)
    return True


def main(one_k=one_k, default_ks=(4, 5, 6)):
    """one_k, default_ks: the legs of a K and the K to run (tools/measure_f4ratio_pops.py passes its own)"""
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else list(default_ks)
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
