"""GPU: `bin/pbsWindowPops` — PBS windows of all trios from K MAF files, every population of a trio as the focal one.  Every
PREFIX.pop<i>_pop<j>_pop<k>.pbs and PREFIX.global is held to what the NumPy model of the definition (tests/pbs_pops_model.py)
gives for the sites all files list, formatted by the tool's rules: labels and integers byte for byte, the float columns
numerically at %g precision — half a unit of the sixth digit — plus what the contract's bound on the six sums (1e-9 A + 1e-12
each) allows the printed value to move: for FST = num / den that is (dnum + |FST| dden) / |den|, for T = -log(1 - FST) that
divided by |1 - FST|, for a PBS half the sum of its three branches' — first-order propagation, doubled.  stdout stays empty;
each refusal has its exit code and message."""
import math
import os

import numpy as np
import pytest

import helpers
import pbs_pops_model
from pbs_pops_model import PAIRS, PBS, all_trio_order
from test_cli_dstat_pops import MODES
from test_cli_fst_pops import common_columns, options
from test_cli_pops import random_rows, run, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu
ESTIMATORS = ("wc", "hudson")


@pytest.fixture(scope="module")
def tools():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "pbsWindowPops"), os.path.join(BIN, "fstWindowPops")


def table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len):
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import run_lengths
    rl = run_lengths(chr_ids)
    if W == 0:
        return np.zeros(0, dtype=WIN_DTYPE)
    return pgt.build_windows_sites(rl, W, S) if fixedsite else pgt.build_windows_bp(pos, rl, chr_len, W, S)


def printed_values(r, a):
    """r: a model row or total; a: {sum: its A} -> [(value, slack)] of pbs_i pbs_j pbs_k fst_ij fst_ik fst_jk"""
    fst, t_slack = [], []
    for p in PAIRS:
        num, den = float(r[f"num_{p}"]), float(r[f"den_{p}"])
        x = pbs_pops_model.fst_of(num, den)
        dn, dd = 1e-9 * a[f"num_{p}"] + 1e-12, 1e-9 * a[f"den_{p}"] + 1e-12
        s = 2 * (dn + abs(x) * dd) / abs(den) if den != 0 else 0.0
        fst.append((x, s))
        t_slack.append(s / abs(1 - x) if x != 1 else math.inf)
    order = {"pbs_i": (0, 1, 2), "pbs_j": (0, 2, 1), "pbs_k": (1, 2, 0)}
    return [(float(r[f]), 0.5 * sum(t_slack[c] for c in order[f])) for f in PBS] + fst


def expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing, est):
    """-> ({(i, j, k): rows of PREFIX.pop<i>_pop<j>_pop<k>.pbs or None}, rows of PREFIX.global)"""
    rows, tot, A, A_tot = pbs_pops_model.model(pos, freqs, ninds, minind, win, est)
    files, glob = {}, []
    for t, (i, j, k) in enumerate(all_trio_order(len(freqs))):
        lines = []
        for w, (wd, r) in enumerate(zip(win, rows[t])):
            n = int(r["n"])
            if skip_missing and n == 0:
                continue
            lines.append([names[int(wd["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))]
                         + printed_values(r, {s: A[s][t][w] for s in A}) + [str(n), str(int(wd["hi"]) - int(wd["lo"]) - n)])
        files[(i + 1, j + 1, k + 1)] = lines if W > 0 else None
        glob.append([str(i + 1), str(j + 1), str(k + 1)] + printed_values(tot[t], {s: A_tot[s][t] for s in A_tot})
                    + [str(int(tot[t]["neff"])), str(int(tot[t]["nskip"]))])
    return files, glob


def close_value(text, want):
    y, slack = want
    if not math.isfinite(y):  # inf and nan are printed as printf prints them; a NaN has no sign
        return text == ("nan" if y != y else ("inf" if y > 0 else "-inf"))
    assert text == "%g" % float(text), text
    return abs(float(text) - y) <= 5.1e-6 * abs(y) + slack + helpers.ABS


def check_outputs(prefix, files, glob, what):
    for (i, j, k), want in files.items():
        path = f"{prefix}.pop{i}_pop{j}_pop{k}.pbs"
        if want is None:
            assert not os.path.exists(path), what
            continue
        got = helpers.parse_tsv(open(path).read())
        assert len(got) == len(want), (what, (i, j, k), len(got), len(want))
        for g, w in zip(got, want):
            assert len(g) == 12 and g[:4] == w[:4] and g[10:] == w[10:], (what, (i, j, k), g, w)
            assert all(close_value(g[c], w[c]) for c in range(4, 10)), (what, (i, j, k), g, w)
    got = helpers.parse_tsv(open(prefix + ".global").read())
    assert len(got) == len(glob) == len(files)
    for g, w in zip(got, glob):
        assert len(g) == 11 and g[:3] == w[:3] and g[9:] == w[9:], (what, g, w)
        assert all(close_value(g[c], w[c]) for c in range(3, 9)), (what, g, w)


def listed(prefix):
    base = os.path.basename(prefix)
    return sorted(f for f in os.listdir(os.path.dirname(prefix)) if f.startswith(base + "."))


@pytest.mark.parametrize("k", [3, 5])
def test_files_equal_the_model_on_the_common_sites(pgt, tools, tmp_path, k):
    tool = tools[0]
    rng = np.random.default_rng(770 + k)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 320)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    tables = [random_rows(rng, chroms, uni, keep) for keep in (0.95, 0.9, 0.92, 0.97, 0.94)[:k]]
    tables[1] = [r for r in tables[1] if r[0] != "chrB" or r[1] > 2000]  # half a chromosome is missing from one file
    for t in tables:  # nInd up to 20, as the project generates it
        t[:] = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in t]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == chroms and pos.size > 150
    assert len({len(t) for t in tables}) == k and all(len(t) > pos.size for t in tables)  # differing site lists: the alignment matters
    paths = []
    for n, t in enumerate(tables):
        gz = n == 1  # one file is compressed
        paths.append(str(tmp_path / (f"p{n}.mafs" + (".gz" if gz else ""))))
        write_maf(paths[-1], t, gz=gz)
    chr_len = np.array([int(uni[c].max()) + 137 for c in names], dtype=np.uint32)
    jobs, tags = [], []

    def add(tag, mode, extra, ingest="1"):
        os.makedirs(tmp_path / tag)
        jobs.append(([tool] + options(*mode, str(sizes)) + extra + ["-out", str(tmp_path / tag / "o")] + paths, {"PGT_GPU_INGEST": ingest}))
        tags.append(tag)

    for mi, m in enumerate(MODES):
        add(f"m{mi}_hudson", m, ["-estimator", "hudson"])
        add(f"m{mi}_wc", m, ["-estimator", "wc"] if mi % 2 else [])  # wc is the default
    add("m1_host", MODES[1], [], ingest="0")
    for j, r in zip(jobs, run_all(jobs, workers=4)):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)
    trios = [(i + 1, j + 1, kk + 1) for i, j, kk in all_trio_order(k)]
    dropped = False
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        win = table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len)
        want_names = sorted(([f"o.pop{i}_pop{j}_pop{kk}.pbs" for i, j, kk in trios] if W else []) + ["o.global"])
        for est in ESTIMATORS:
            files, glob = expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing, est)
            if skip_missing and W:
                every, _ = expected_files(names, pos, freqs, ninds, win, W, minind, 0, est)
                dropped = dropped or any(len(files[t]) < len(every[t]) for t in files)
            prefix = str(tmp_path / f"m{mi}_{est}" / "o")
            assert listed(prefix) == want_names, (MODES[mi], est, listed(prefix))
            check_outputs(prefix, files, glob, (k, est, MODES[mi]))
        if mi == 1:  # the files parsed on the host give the same bytes
            host, prefix = str(tmp_path / "m1_host" / "o"), str(tmp_path / "m1_wc" / "o")
            assert listed(host) == want_names
            for name in want_names:
                assert open(os.path.join(os.path.dirname(host), name), "rb").read() == open(os.path.join(os.path.dirname(prefix), name), "rb").read(), name
    assert dropped, "-skip_missing 1 must have had a row to drop"


@pytest.mark.parametrize("est", ESTIMATORS)
def test_fst_columns_equal_fstWindowPops_where_the_site_sets_are_the_same(pgt, tools, tmp_path, est):
    """Identical site lists and nInd >= minind everywhere: a trio's site set is each pair's own, and fst_ij / fst_ik / fst_jk are
    the .fst columns of fstWindowPops on the same files: both are %g of sums within the contract's bound."""
    tool, fst_tool = tools
    rng = np.random.default_rng(790)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 260)) for c in chroms}
    tables = [[(c, p, fr, int(rng.integers(5, 21))) for c, p, fr, _ in random_rows(rng, chroms, uni, 1.1)] for _ in range(3)]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert all(len(t) == pos.size for t in tables)
    paths = [str(tmp_path / f"p{n}.mafs") for n in range(3)]
    for p, t in zip(paths, tables):
        write_maf(p, t)
    opts = ["-fixedsite", "1", "-winsize", "40", "-stepsize", "15", "-minind", "5", "-estimator", est]
    for tl, tag in ((tool, "pbs"), (fst_tool, "fst")):
        r = run([tl] + opts + ["-out", str(tmp_path / tag)] + paths, {})
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (tag, r.stderr)
    pbs = helpers.parse_tsv(open(str(tmp_path / "pbs") + ".pop1_pop2_pop3.pbs").read())
    win = table_for(pgt, chr_ids, pos, 40, 15, 1, None)
    want = expected_files(names, pos, freqs, ninds, win, 40, 5, 0, est)[0][(1, 2, 3)]
    assert len(pbs) == len(want) > 10
    for col, (i, j) in zip((7, 8, 9), ((1, 2), (1, 3), (2, 3))):
        fst = helpers.parse_tsv(open(str(tmp_path / "fst") + f".pop{i}_pop{j}.fst").read())
        assert len(fst) == len(pbs)
        for a, b, w in zip(pbs, fst, want):
            assert a[:4] == b[:4] and a[10:] == b[5:], (a, b)  # the same windows and the same counts
            y, slack = w[col]
            assert abs(float(a[col]) - float(b[4])) <= 2 * (5.1e-6 * abs(y) + slack) + helpers.ABS, (i, j, a, b)


def test_refusals_exit_codes_and_messages(tools, tmp_path):
    tool = tools[0]
    row = "chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\n"
    m = [str(tmp_path / f"p{k}.mafs") for k in range(7)]
    for n, p in enumerate(m):
        open(p, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.{(3 * s + n) % 10}00000\t5\n" for s in range(1, 9)))
    other = str(tmp_path / "other.mafs")
    open(other, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.500000\t5\n" for s in range(100, 104)))
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    cases = [
        (head + m[:2], "pbsWindowPops: between 3 and 6 MAF files are needed (2 given)"),
        (head + m[:7], "pbsWindowPops: between 3 and 6 MAF files are needed (7 given)"),
        (["-estimator", "nei"] + head + m[:3], "-estimator must be wc or hudson (given: nei)"),
        (["-winsize", "4", "-stepsize", "4", "-out", out] + m[:3], "Must supply size file unless -fixedsite 1"),
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "4"] + m[:3], "Must supply -out PREFIX"),
        (head + m[:2] + [str(tmp_path / "missing.mafs")], "Unable to open Pop3 MAF file"),
        (head + m[:2] + [other], "pbsWindowPops: the MAF files share no site"),
    ]
    for args, msg in cases:
        r = run([tool] + args, {})
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr, (args, r.returncode, r.stderr)
        assert [f for f in os.listdir(tmp_path) if f.startswith("o.")] == [], args
    r = run([tool, "-estimator", "hudson"] + head + m[:3], {})  # the same files and options, unharmed, run
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("o.")) == ["o.global", "o.pop1_pop2_pop3.pbs"]
    rows = helpers.parse_tsv(open(out + ".pop1_pop2_pop3.pbs").read())
    assert [r[1:4] + r[10:] for r in rows] == [["1", "4", "2", "4", "0"], ["5", "8", "6", "4", "0"]]
