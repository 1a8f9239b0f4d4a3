#!/usr/bin/env python3
"""The f4-ratio sums of all middle triples of K populations (f4ratio_pops_reduce_dev) on one MI355X, beside f4 of all quartets
of the same K on the same columns and window table (f4_pops_reduce_dev: the same walk and 12 B/site/population, three sums per
item, the counts as bits): the two ALTERNATE in one process on one card.  f4 stops at K = 6: at K = 7 the f4-ratio runs alone.

Columns, window table, arguments (sites, then K comma separated; here K in {5, 6, 7}), timing method and output are those of
tools/measure_f4_pops.py, whose main() this tool calls with its own two legs.  Before anything is timed the coordinates of the
two calls' rows must be equal, a triple's count must not exceed that of the f4 call's quartet (A, i, j, O), every sum must be
finite, reserved_ +0.0, and a row's three sums must cancel, |s0 - s1 + s2| <= 3 (1e-9 n + 1e-12); a mismatch exits non-zero."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from popgenomicstools_amd._lib import F4_ROW_DTYPE, F4_TOTAL_DTYPE, F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE  # noqa: E402
from popgenomicstools_amd.window_scan import all_quartet_order, middle_triple_order, rows_from_device, windows_to_device  # noqa: E402
import measure_f4_pops as base  # noqa: E402  (the columns, the table, event_ms and main(), which takes this tool's legs)
from measure_f4_pops import HBM_PEAK, event_ms  # noqa: E402

SUMS = ("g_ij", "g_ik", "g_jk")


def rows_agree(k, rr, r4):
    """the checks of the docstring on the rows of the two calls (r4: None at K = 7)"""
    quartets = all_quartet_order(k) if r4 is not None else []
    for t, (i, j, kk) in enumerate(middle_triple_order(k)):
        if r4 is not None:
            p = r4[quartets.index((0, i, j, k - 1))]
            if not all(np.array_equal(rr[t][fld], p[fld]) for fld in ("start", "end", "mid")) or np.any(rr[t]["n"] > p["n"]):
                return False
        if not all(np.all(np.isfinite(rr[t][fld])) for fld in SUMS) or rr[t]["reserved_"].view(np.uint64).any():
            return False
        gap = np.abs(rr[t][SUMS[0]] - rr[t][SUMS[1]] + rr[t][SUMS[2]])
        if np.any(gap > 3.0 * (1e-9 * rr[t]["n"] + 1e-12)) or not np.any(rr[t]["n"] > 0):
            return False
    return True


def one_k(ctx, k, n, pos, f, c, minind, win, n_win, dev, card, W, S):
    """the f4-ratio call and the f4 call alternately on the same columns -> one JSON line; False when their rows disagree"""
    tables = {"f4ratio": len(middle_triple_order(k))}
    shape = {"f4ratio": (F4RATIO_ROW_DTYPE, F4RATIO_TOTAL_DTYPE, ctx.f4ratio_pops_reduce_dev, ctx.f4ratio_pops_tree_bytes(k, n))}
    if k <= 6:
        tables["f4"] = len(all_quartet_order(k))
        shape["f4"] = (F4_ROW_DTYPE, F4_TOTAL_DTYPE, ctx.f4_pops_reduce_dev, ctx.f4_pops_tree_bytes(k, n))
    out = {e: torch.empty(tables[e] * n_win * s[0].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tot = {e: torch.empty(tables[e] * s[1].itemsize, dtype=torch.uint8, device=dev) for e, s in shape.items()}
    tree = {e: torch.empty(s[3], dtype=torch.uint8, device=dev) for e, s in shape.items()}
    leg = {e: (lambda e=e: shape[e][2](pos, f, c, minind, win, out=out[e], tot=tot[e], tree=tree[e])) for e in shape}
    for e in shape:
        leg[e]()
    torch.cuda.synchronize()
    rr = rows_from_device(out["f4ratio"], F4RATIO_ROW_DTYPE).reshape(tables["f4ratio"], n_win)
    r4 = rows_from_device(out["f4"], F4_ROW_DTYPE).reshape(tables["f4"], n_win) if "f4" in shape else None
    if not rows_agree(k, rr, r4):
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
    res = {"k": k, "n_sites": n, "n_triples": tables["f4ratio"], "n_quartets": tables.get("f4"), "n_win": int(n_win), "W": W, "S": S,
           "minind": minind, "rows_check": "ok", "steps_per_repetition": steps, "card": card}
    for e in shape:
        build = float(np.median([x[0] for x in bq[e]]))
        res[e] = {"step_ms": float(np.median(step_ms[e])), "repetitions_ms": step_ms[e], "build_ms": build,
                  "query_ms": float(np.median([x[1] for x in bq[e]])),
                  "build_fraction_of_hbm_peak": 12.0 * k * n / (build * 1e-3) / HBM_PEAK}
    if "f4" in shape:
        res["f4ratio_build_over_f4_build"] = res["f4ratio"]["build_ms"] / res["f4"]["build_ms"]
        res["f4ratio_query_over_f4_query"] = res["f4ratio"]["query_ms"] / res["f4"]["query_ms"]
        res["f4ratio_step_over_f4_step"] = res["f4ratio"]["step_ms"] / res["f4"]["step_ms"]
    print(json.dumps(res), flush=True)
    return True


if __name__ == "__main__":
    base.main(one_k=one_k, default_ks=(5, 6, 7))
