#!/usr/bin/env python3
"""pgt_sites_align + the gathers behind it on one MI355X, beside two yardsticks.

Part 1: K in {2, 4, 8} files of about 10^8 rows (argv[1] overrides), 20 chromosomes; every file keeps a random share q of one
universe of sites, q chosen so that about 90 % of file 0's rows are common to all K.  Before anything is timed the index
columns are checked (every file holds the same position at idx[k][m]; n_common = the sites no file dropped).  Two legs
ALTERNATE, 3 repetitions each: (a) sites_align (synchronous: wall clock around the call), (b) the 2K + 1 gathers (aligned
position column, frequency f64 and count i32 of every file; events on the stream).  Yardstick: the bytes that must move — 4 B
per row and file read, 4 B per common site and file written, the gathered columns read and written (and their index columns
read) — at the 8 TB/s peak.
Part 2 (K = 2): the "sync + table" phase of bin/dxyWindow under PGT_HOST_TIMING=1 on two nested MAF files of 2*10^7 lines
(argv[2] overrides; the host merge this replaces: dxyWindow_main.cpp keeps it), alternating with sites_align + gathers on
the same site lists.  One JSON line per measurement on stdout."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import popgenomicstools_amd as pgt  # noqa: E402

HBM_PEAK = 8e12
N_CHR = 20


def make_files(n_rows, k, share_common, dev, gen):
    """-> per file (pos int32 tensor, run lengths), the number of common sites"""
    q = share_common ** (1.0 / max(k - 1, 1))
    per_chr = int(n_rows / q) // N_CHR
    uni = torch.cat([torch.cumsum(torch.randint(1, 60, (per_chr,), device=dev, generator=gen, dtype=torch.int32), 0, dtype=torch.int32)
                     for _ in range(N_CHR)])
    files, every = [], torch.ones(uni.numel(), dtype=torch.bool, device=dev)
    for _ in range(k):
        keep = torch.rand(uni.numel(), device=dev, generator=gen) < q
        every &= keep
        files.append((uni[keep].contiguous(), keep.view(N_CHR, per_chr).sum(1).cpu().numpy().astype(np.uint64)))
    return files, int(every.sum())


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(ctx, files, n_common, dev, card, label):
    k = len(files)
    pos = [f[0] for f in files]
    segs, _ = pgt.align_segments_runs([np.arange(N_CHR)] * k, [f[1] for f in files])
    freq = [torch.rand(p.numel(), dtype=torch.float64, device=dev) for p in pos]
    nind = [torch.randint(0, 20, (p.numel(),), dtype=torch.int32, device=dev) for p in pos]
    cap = int(min(p.numel() for p in pos))
    idx = [torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(k)]
    work = torch.empty(ctx.align_workspace_bytes(k, pos[0].numel()), dtype=torch.uint8, device=dev)
    got = {}

    def leg_align():
        got["idx"], got["counts"], got["n"] = ctx.sites_align(pos, segs, cap=cap, idx=idx, work=work)
    leg_align()
    n = got["n"]
    ok = n == n_common and all(torch.equal(pos[0][got["idx"][0].long()], pos[j][got["idx"][j].long()]) for j in range(1, k))
    ok = ok and all(bool((got["idx"][j][1:] > got["idx"][j][:-1]).all()) for j in range(k))
    if not ok:
        print(json.dumps({"what": label, "k": k, "check": "FAILED", "n_common": n, "expected": n_common}), flush=True)
        return False
    out_pos = torch.empty(n, dtype=torch.int32, device=dev)
    out_f = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(k)]
    out_c = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(k)]

    def leg_gather():
        ctx.gather_dev(pos[0], got["idx"][0], out=out_pos)
        for j in range(k):
            ctx.gather_dev(freq[j], got["idx"][j], out=out_f[j])
            ctx.gather_dev(nind[j], got["idx"][j], out=out_c[j])
    for _ in range(2):  # warm-up
        leg_align()
        leg_gather()
    ta, tg = [], []
    for _ in range(3):  # alternating
        ta.append(min(wall_ms(leg_align) for _ in range(3)))
        tg.append(min(event_ms(leg_gather) for _ in range(3)))
    rows = sum(p.numel() for p in pos)
    bytes_align = 4 * rows + 4 * k * n
    bytes_gather = n * (4 + 4 + 4) + k * n * (8 + 8 + 4 + 4 + 4 + 4)  # element read + written, index read, per gathered column
    a_ms, g_ms = float(np.median(ta)), float(np.median(tg))
    print(json.dumps({
        "what": label, "k": k, "rows_per_file": [int(p.numel()) for p in pos], "n_common": n, "check": "ok",
        "align_ms": a_ms, "gather_ms": g_ms, "align_plus_gather_ms": a_ms + g_ms, "repetitions_ms": {"align": ta, "gather": tg},
        "bytes_align": bytes_align, "bytes_gather": bytes_gather,
        "floor_ms_at_8TBps": {"align": bytes_align / HBM_PEAK * 1e3, "gather": bytes_gather / HBM_PEAK * 1e3},
        "fraction_of_hbm_peak": {"align": bytes_align / (a_ms * 1e-3) / HBM_PEAK, "gather": bytes_gather / (g_ms * 1e-3) / HBM_PEAK},
        "card": card}), flush=True)
    return a_ms + g_ms


def write_maf(path, chr_of, pos, rng):
    """fixed-width lines `cNN pos A C A 0.ffffff nn`, formatted with array arithmetic (2*10^7 lines in seconds)"""
    n = pos.size
    fr = rng.integers(0, 1000000, n)
    ni = rng.integers(0, 20, n)
    line = np.frombuffer(b"c00\t000000000\tA\tC\tA\t0.000000\t00\n", dtype=np.uint8)
    buf = np.tile(line, (n, 1))

    def digits(col0, width, v):
        v = v.astype(np.int64)
        for d in range(width):
            buf[:, col0 + width - 1 - d] = 48 + v % 10
            v //= 10
    digits(1, 2, chr_of)
    digits(4, 9, pos)
    digits(22, 6, fr)
    digits(29, 2, ni)
    with open(path, "wb") as fh:
        fh.write(b"chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\n")
        fh.write(buf.tobytes())


def host_merge_yardstick(ctx, n_lines, dev, gen, card):
    files, n_common = make_files(n_lines, 2, 0.9, dev, gen)
    # nested: file 1 lists everything file 0 lists and more
    uni = torch.unique(torch.cat([files[0][0].long() + (torch.repeat_interleave(torch.arange(N_CHR, device=dev), torch.from_numpy(files[0][1].astype(np.int64)).to(dev)) << 32),
                                  files[1][0].long() + (torch.repeat_interleave(torch.arange(N_CHR, device=dev), torch.from_numpy(files[1][1].astype(np.int64)).to(dev)) << 32)]))
    big_pos, big_chr = (uni & 0xFFFFFFFF).int(), (uni >> 32)
    big_len = torch.bincount(big_chr, minlength=N_CHR).cpu().numpy().astype(np.uint64)
    nested = [files[0], (big_pos.contiguous(), big_len)]
    rng = np.random.default_rng(5)
    tool = os.path.join(ROOT, "popgenomicstools_amd", "bin", "dxyWindow")
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for j, (p, rl) in enumerate(nested):
            paths.append(os.path.join(d, f"p{j}.mafs"))
            write_maf(paths[-1], np.repeat(np.arange(N_CHR), rl.astype(np.int64)), p.cpu().numpy(), rng)
        cmd = [tool, "-fixedsite", "1", "-winsize", "50000", "-stepsize", "10000"] + paths
        host, ours = [], []
        for _ in range(3):  # alternating
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PGT_HOST_TIMING="1"))
            m = re.search(r"\[pgt-host\] sync \+ table\s+([0-9.]+) ms", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps({"what": "dxyWindow sync + table", "error": r.stderr[-400:]}), flush=True)
                return
            host.append(float(m.group(1)))
            ours.append(measure(ctx, nested, int(nested[0][0].numel()), dev, card, "K = 2 on the nested lists of the dxyWindow run"))
        print(json.dumps({"what": "dxyWindow (parent commit's host merge) sync + table phase", "lines": [int(x[0].numel()) for x in nested],
                          "command": " ".join(["PGT_HOST_TIMING=1", "bin/dxyWindow"] + cmd[1:-2] + ["p0.mafs", "p1.mafs"]),
                          "sync_plus_table_ms": host, "median_ms": float(np.median(host)),
                          "sites_align_plus_gathers_ms": ours, "card": card}), flush=True)


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    n_lines = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20_000_000
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240817)
    props = torch.cuda.get_device_properties(0)
    card = {"name": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count, "hip": torch.version.hip}
    ctx = pgt.Context(0)
    rc = 0
    for k in (2, 4, 8):
        files, n_common = make_files(n, k, 0.9, dev, gen)
        if measure(ctx, files, n_common, dev, card, "random lists, about 90 % of file 0 common") is False:
            rc = 1
            break
        del files
        torch.cuda.empty_cache()
    if rc == 0 and n_lines > 0:
        host_merge_yardstick(ctx, n_lines, dev, gen, card)
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
