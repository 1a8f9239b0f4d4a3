#!/usr/bin/env python3
"""Nucleotide diversity per population (pi_pops_reduce_dev) on one MI355X, in one process on one card.

10^8 sites (argv[1] overrides), 20 chromosomes, W = 50 000, S = 10 000, minind 5, columns from synth_genome.py (populations
2q, 2q+1 are the two populations of SynthGenome(12345 + q)), K in {1, 4, 8} (argv[2] overrides).

Part 1, the build.  Before anything is timed, the rows of every K are compared with float64 torch arithmetic on the card
(per-site values in the order of the definition, window sums as differences of a float64 prefix sum; counts exactly, sums
within 1e-9 |y| + 1e-12); a mismatch exits non-zero.  Then the legs ALTERNATE — the pi call of each K and, as the
yardstick, pgt_dxy_reduce_dev on the first two populations (24 B/site) — 2 warm-up rounds discarded, 9 measured rounds;
per leg the build kernel's time from the library's events (last_kernel_ms), median over the rounds, and its share of the
8 TB/s HBM peak on 12 K B/site (24 B/site for dxy).  The call's whole time (build + query) is the events' sum.

Part 2, the S = 1 query at ~10^8 windows, K = 1: the table W = 50 000, S = 1 answered by the group query (the strategy
the table's own hints select) and by the plain one-wave-per-window range query (step hint 0), alternating, 1 warm-up round
discarded, 7 measured; the query kernel's time from the same events, medians; rows compared between the two.

One JSON line per result on stdout."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popgenomicstools_amd as pgt  # noqa: E402
from popgenomicstools_amd._lib import DXY_ROW_DTYPE, DXY_TOTAL_DTYPE, PGT_STAT_DXY  # noqa: E402
from popgenomicstools_amd.window_scan import rows_from_device, table_hints, windows_to_device  # noqa: E402
from synth_genome import SynthGenome  # noqa: E402

REL, ABS = 1e-9, 1e-12
HBM_PEAK = 8e12  # bytes/s
WARMUP, ROUNDS = 2, 9


def torch_rows(f, c, minind, lo, hi):
    """-> (sum, neff) per window from float64 arithmetic on the card, per-site values in the definition's order"""
    dn = c.to(torch.float64)
    two_n = 2.0 * dn
    v = ((2.0 * f) * (1.0 - f)) * (two_n / (two_n - 1.0))
    ok = c >= minind
    ps = torch.cat([torch.zeros(1, dtype=torch.float64, device=f.device), torch.cumsum(torch.where(ok, v, torch.zeros_like(v)), 0)])
    pn = torch.cat([torch.zeros(1, dtype=torch.int64, device=f.device), torch.cumsum(ok.to(torch.int64), 0)])
    return (ps[hi] - ps[lo]).cpu().numpy(), (pn[hi] - pn[lo]).cpu().numpy()


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 4, 8]
    dev = torch.device("cuda", 0)
    W, S, minind = 50_000, 10_000, 5
    ctx = pgt.Context(0)
    props = torch.cuda.get_device_properties(0)
    card = {"name": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
            "hip": torch.version.hip}
    genomes = [SynthGenome(12345 + q, n, 20) for q in range((max(ks + [2]) + 1) // 2)]
    pos = genomes[0].pos_t(0, n, dev)
    freqs, ninds = [], []
    for g in genomes:
        p1, p2, n1, n2 = g.dxy_columns_t(0, n, dev)
        freqs += [p1, p2]
        ninds += [n1, n2]
    win_h = pgt.build_windows_sites(genomes[0].run_len, W, S)
    win = windows_to_device(win_h, dev)
    n_win = win_h.size
    lo = torch.from_numpy(win_h["lo"].astype(np.int64)).to(dev)
    hi = torch.from_numpy(win_h["hi"].astype(np.int64)).to(dev)
    ctx.set_max_window(W)
    ctx.set_window_step(S)

    # ---- part 1: the build ---------------------------------------------------------------------------------------------
    bufs = {}
    for k in ks:
        bufs[k] = (torch.empty(k * n_win * DXY_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                   torch.empty(k * DXY_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                   torch.empty(ctx.pi_pops_tree_bytes(k, n), dtype=torch.uint8, device=dev))
    dxy_out = torch.empty(n_win * DXY_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    dxy_tot = torch.empty(DXY_TOTAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    dxy_tree = torch.empty(ctx.tree_bytes(PGT_STAT_DXY, n), dtype=torch.uint8, device=dev)

    def pi_leg(k):
        out, tot, tree = bufs[k]
        ctx.pi_pops_reduce_dev(pos, freqs[:k], ninds[:k], minind, win, out=out, tot=tot, tree=tree)

    def dxy_leg():
        ctx.dxy_reduce_dev(pos, freqs[0], freqs[1], ninds[0], ninds[1], minind, win, out=dxy_out, tot=dxy_tot, tree=dxy_tree)

    for k in ks:  # rows check before anything is timed
        pi_leg(k)
        torch.cuda.synchronize()
        rows = rows_from_device(bufs[k][0], DXY_ROW_DTYPE).reshape(k, n_win)
        tots = rows_from_device(bufs[k][1], DXY_TOTAL_DTYPE)
        max_rel = 0.0
        for p in range(k):
            want, neff = torch_rows(freqs[p], ninds[p], minind, lo, hi)
            diff = np.abs(rows[p]["sum"] - want)
            ok = (np.array_equal(rows[p]["neff"], neff.astype(np.uint32)) and bool(np.all(diff <= REL * np.abs(want) + ABS))
                  and int(tots[p]["neff"]) + int(tots[p]["nskip"]) == n)
            max_rel = max(max_rel, float(np.max(diff / np.maximum(np.abs(want), 1e-300))))
            if not ok:
                print(json.dumps({"k": k, "population": p, "rows_check": "FAILED", "max_rel_diff": max_rel}), flush=True)
                ctx.close()
                sys.exit(1)
        print(json.dumps({"k": k, "rows_check": "ok", "max_rel_diff_vs_torch_f64": max_rel}), flush=True)

    ctx.set_profiling(True)
    legs = [("pi", k) for k in ks] + [("dxy", 2)]
    times = {leg: [] for leg in legs}
    for r in range(WARMUP + ROUNDS):  # alternating legs; the warm-up rounds are discarded
        for leg in legs:
            pi_leg(leg[1]) if leg[0] == "pi" else dxy_leg()
            bq = ctx.last_kernel_ms()  # synchronises on the call's events
            if r >= WARMUP:
                times[leg].append(bq)
    for leg in legs:
        b = [x[0] for x in times[leg]]
        q = [x[1] for x in times[leg]]
        bytes_per_site = 12.0 * leg[1] if leg[0] == "pi" else 24.0
        bm = float(np.median(b))
        print(json.dumps({
            "part": "build", "leg": f"{leg[0]} K={leg[1]}" if leg[0] == "pi" else "dxy (pgt_dxy_reduce_dev, the yardstick)",
            "n_sites": n, "n_win": int(n_win), "W": W, "S": S, "minind": minind, "bytes_per_site": bytes_per_site,
            "rounds": ROUNDS, "warmup_rounds_discarded": WARMUP,
            "build_ms_median": bm, "build_ms_min": float(np.min(b)), "build_ms_max": float(np.max(b)),
            "build_fraction_of_hbm_peak": bytes_per_site * n / (bm * 1e-3) / HBM_PEAK,
            "query_ms_median": float(np.median(q)), "card": card}), flush=True)
    for k in ks:
        del bufs[k]
    del dxy_out, dxy_tree

    # ---- part 2: S = 1, group query against the plain range query ---------------------------------------------------------
    win1_h = pgt.build_windows_sites(genomes[0].run_len, W, 1)
    m, typical, step = table_hints(win1_h)
    win1 = windows_to_device(win1_h, dev)
    nw = win1_h.size
    del win1_h
    outs = [torch.empty(nw * DXY_ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(2)]
    tree = torch.empty(ctx.pi_pops_tree_bytes(1, n), dtype=torch.uint8, device=dev)
    strategies = [("group query (the table's hints)", (m, step, typical)), ("one wave per window (step hint 0)", (m, 0, typical))]
    q = {name: [] for name, _ in strategies}
    for r in range(1 + 7):
        for i, (name, h) in enumerate(strategies):
            with ctx.hints(*h):
                ctx.pi_pops_reduce_dev(pos, freqs[:1], ninds[:1], minind, win1, out=outs[i], tot=False, tree=tree)
                bq = ctx.last_kernel_ms()
            if r >= 1:
                q[name].append(bq[1])
    r0, r1 = outs[0].view(torch.float64).view(-1, 3), outs[1].view(torch.float64).view(-1, 3)
    ints_equal = bool(torch.equal(outs[0].view(torch.int32).view(-1, 6)[:, :4], outs[1].view(torch.int32).view(-1, 6)[:, :4]))
    d = ((r0[:, 2] - r1[:, 2]).abs() / r1[:, 2].abs().clamp_min(1e-300)).max().item()
    for name, _ in strategies:
        print(json.dumps({"part": "query S=1", "strategy": name, "n_sites": n, "n_win": int(nw), "W": W, "K": 1,
                          "query_ms_median": float(np.median(q[name])), "query_ms_min": float(np.min(q[name])),
                          "query_ms_max": float(np.max(q[name])), "rounds": 7, "warmup_rounds_discarded": 1}), flush=True)
    print(json.dumps({"part": "query S=1", "coordinates_and_counts_equal": ints_equal, "max_rel_diff_of_sums_between_strategies": d}), flush=True)
    ctx.close()
    sys.exit(0 if ints_equal and d <= 1e-9 else 1)


if __name__ == "__main__":
    main()
