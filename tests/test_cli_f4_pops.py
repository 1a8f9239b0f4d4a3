"""GPU: `bin/f4WindowPops` — f4 windows of all quartets from K MAF files, every quartet in its three pairings.  Every
PREFIX.pop<i>_pop<j>_pop<k>_pop<l>.f4, PREFIX.global and PREFIX.jackknife is held to what the NumPy models of the definitions
(tests/f4_pops_model.py, tests/f3_jack_model.py for the jackknife of a mean) and the Python mirror f4_window_pops give for the
sites all files list, formatted by the tool's rules: labels and integers byte for byte, the float columns numerically at %g
precision — half a unit of the sixth digit, plus the contract's bound on the window's sum (1e-9 A + 1e-12) divided by the number
of sites, since a printed value is a mean.  The row files are the same with and without -jackknife 1; stdout stays empty; each
refusal has its exit code and message."""
import os

import numpy as np
import pytest

import f3_jack_model
import f4_pops_model
import helpers
import pops_cli_cases
from f4_pops_model import SUMS, all_quartet_order
from test_cli_dstat_pops import MODES
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pops import random_rows, run, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "f4WindowPops")


def table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len):
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import run_lengths
    rl = run_lengths(chr_ids)
    if W == 0:
        return np.zeros(0, dtype=WIN_DTYPE)
    return pgt.build_windows_sites(rl, W, S) if fixedsite else pgt.build_windows_bp(pos, rl, chr_len, W, S)


def expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing):
    """-> ({(i, j, k, l): rows of PREFIX.pop<i>_pop<j>_pop<k>_pop<l>.f4 or None}, rows of PREFIX.global, the model's rows): a
    float column is (mean, the bound on it that comes from the sum's)"""
    rows, tot, A, A_tot = f4_pops_model.model(pos, freqs, ninds, minind, win)
    files, glob = {}, []
    for t, q in enumerate(all_quartet_order(len(freqs))):
        lines = []
        for w, (wd, r) in enumerate(zip(win, rows[t])):
            if skip_missing and int(r["n"]) == 0:
                continue
            n = int(r["n"])
            vals = [(float(f4_pops_model.mean(r[f], n)), (1e-9 * A[f][t][w] + 1e-12) / max(n, 1)) for f in SUMS]
            lines.append([names[int(wd["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))] + vals
                         + [str(n), str(int(wd["hi"]) - int(wd["lo"]) - n)])
        files[tuple(x + 1 for x in q)] = lines if W > 0 else None
        n = int(tot[t]["neff"])
        glob.append([str(x + 1) for x in q] + [(float(f4_pops_model.mean(tot[t][f], n)), (1e-9 * A_tot[f][t] + 1e-12) / max(n, 1)) for f in SUMS]
                    + [str(n), str(int(tot[t]["nskip"]))])
    return files, glob, rows


def close_mean(text, want):
    y, slack = want
    assert text == "%g" % float(text), text
    return abs(float(text) - y) <= 5.1e-6 * abs(y) + slack + helpers.ABS


def file_of(prefix, q):
    return f"{prefix}." + "_".join(f"pop{x}" for x in q) + ".f4"


def check_outputs(prefix, files, glob, what):
    for q, want in files.items():
        path = file_of(prefix, q)
        if want is None:
            assert not os.path.exists(path), what
            continue
        got = helpers.parse_tsv(open(path).read())
        assert len(got) == len(want), (what, q, len(got), len(want))
        for g, w in zip(got, want):
            assert len(g) == 9 and g[:4] == w[:4] and g[7:] == w[7:], (what, q, g, w)
            assert all(close_mean(g[c], w[c]) for c in (4, 5, 6)), (what, q, g, w)
    got = helpers.parse_tsv(open(prefix + ".global").read())
    assert len(got) == len(glob) == len(files)
    for g, w in zip(got, glob):
        assert len(g) == 9 and g[:4] == w[:4] and g[7:] == w[7:], (what, g, w)
        assert all(close_mean(g[c], w[c]) for c in (4, 5, 6)), (what, g, w)


def check_against_the_python_mirror(pgt, prefix, chr_ids, pos, freqs, ninds, W, S, fixedsite, skip_missing, minind, chr_len, what):
    """the same run through f4_window_pops: as many rows per quartet, coordinates and counts byte for byte, the means at print precision"""
    res = pgt.f4_window_pops(chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len=None if fixedsite else chr_len, skip_missing=skip_missing)
    assert list(res) == all_quartet_order(len(freqs))
    glob = helpers.parse_tsv(open(prefix + ".global").read())
    for t, q in enumerate(res):
        tot = res[q].total
        assert glob[t][:4] == [str(x + 1) for x in q] and glob[t][7:] == [str(int(tot["neff"])), str(int(tot["nskip"]))], (what, q)
        for c, f in zip((4, 5, 6), SUMS):
            assert close_g6(glob[t][c], float(f4_pops_model.mean(tot[f], tot["neff"]))), (what, q, f)
        if W == 0:
            continue
        got = helpers.parse_tsv(open(file_of(prefix, tuple(x + 1 for x in q))).read())
        rows = res[q].rows
        assert len(got) == rows.size, (what, q)
        for g, r in zip(got, rows):
            assert g[1:4] == [str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))] and g[7] == str(int(r["n"])), (what, q, g, r)
            for c, f in zip((4, 5, 6), SUMS):
                assert close_g6(g[c], float(f4_pops_model.mean(r[f], r["n"]))), (what, q, f, g, r)


def listed(prefix):
    base = os.path.basename(prefix)
    return sorted(f for f in os.listdir(os.path.dirname(prefix)) if f.startswith(base + "."))


@pytest.mark.parametrize("k", [4, 5])
def test_files_equal_the_models_on_the_common_sites(pgt, tool, tmp_path, k):
    rng = np.random.default_rng(670 + k)
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

    JACK_MODES = (2, 4)  # (7, 7) site windows with -skip_missing 1 and (300, 300) base-pair windows: both disjoint
    assert MODES[3][0] == 0 and {m[2] for m in MODES} == {0, 1} and {m[3] for m in MODES} == {0, 1}  # -winsize 0, both window modes, -skip_missing
    for mi, m in enumerate(MODES):
        add(f"m{mi}", m, [])
        if mi in JACK_MODES:
            add(f"m{mi}_jack", m, ["-jackknife", "1"])
    add("m1_host", MODES[1], [], ingest="0")
    add("m4_jack0", MODES[4], ["-jackknife", "0"])
    for j, r in zip(jobs, run_all(jobs, workers=4)):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)
    quartets = [tuple(x + 1 for x in q) for q in all_quartet_order(k)]
    dropped = False
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        win = table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len)
        files, glob, rows = expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing)
        if skip_missing and W:
            every, _, _ = expected_files(names, pos, freqs, ninds, win, W, minind, 0)
            dropped = dropped or any(len(files[t]) < len(every[t]) for t in files)
        prefix = str(tmp_path / f"m{mi}" / "o")
        want_names = sorted(([os.path.basename(file_of("o", q)) for q in quartets] if W else []) + ["o.global"])
        assert listed(prefix) == want_names, (MODES[mi], listed(prefix))
        check_outputs(prefix, files, glob, (k, MODES[mi]))
        check_against_the_python_mirror(pgt, prefix, chr_ids, pos, freqs, ninds, W, S, fixedsite, skip_missing, minind, chr_len, (k, MODES[mi]))
        if mi == 1:  # the files parsed on the host give the same bytes
            host = str(tmp_path / "m1_host" / "o")
            assert listed(host) == want_names
            for name in want_names:
                assert open(os.path.join(os.path.dirname(host), name), "rb").read() == open(os.path.join(os.path.dirname(prefix), name), "rb").read(), name
        if mi not in JACK_MODES:
            continue
        jack = str(tmp_path / f"m{mi}_jack" / "o")
        assert listed(jack) == sorted(want_names + ["o.jackknife"])
        for name in want_names:  # the row files are the same with and without -jackknife 1
            assert open(os.path.join(os.path.dirname(jack), name), "rb").read() == open(os.path.join(os.path.dirname(prefix), name), "rb").read(), (mi, name)
        got = helpers.parse_tsv(open(jack + ".jackknife").read())
        assert len(got) == 3 * len(quartets)
        line = 0
        for t, q in enumerate(all_quartet_order(k)):  # ALL windows are blocks, whatever -skip_missing is
            want3 = f3_jack_model.jack_rows(rows[t].view(f3_jack_model.F3_ROW_DTYPE), f3_jack_model.jack_float)
            assert want3[0]["n_blocks"] >= 8
            for ((a, b), (c, d)), want in zip(pgt.pairing_order(*q), want3):
                g = got[line]
                line += 1
                assert len(g) == 10 and g[:4] == [str(p + 1) for p in (a, b, c, d)], (q, g)
                assert g[8] == str(want["n_blocks"]) and g[9] == str(want["n_sites"]), (q, g, want)
                for col, key in ((4, "f3"), (5, "f3_jack"), (6, "se"), (7, "z")):
                    if want[key] != want[key]:
                        assert g[col] == "nan", (q, key, g)
                    else:
                        assert g[col] == "%g" % float(g[col]) and close_g6(g[col], want[key]), (q, key, g, want)
                assert float(g[6]) > 0
    assert dropped, "-skip_missing 1 must have had a row to drop"
    plain, zero = str(tmp_path / "m4" / "o"), str(tmp_path / "m4_jack0" / "o")  # -jackknife 0 is the run without the option
    assert listed(zero) == listed(plain)
    for name in listed(plain):
        assert open(os.path.join(os.path.dirname(zero), name), "rb").read() == open(os.path.join(os.path.dirname(plain), name), "rb").read(), name


def test_refusals_exit_codes_and_messages(tool, tmp_path):
    row = "chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\n"
    m = [str(tmp_path / f"p{k}.mafs") for k in range(7)]
    for n, p in enumerate(m):
        open(p, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.{(3 * s + n * n) % 10}00000\t5\n" for s in range(1, 9)))
    other = str(tmp_path / "other.mafs")
    open(other, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.500000\t5\n" for s in range(100, 104)))
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    f3 = os.path.join(BIN, "f3WindowPops")
    overlap = ["-jackknife", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-out", out]
    cases = [
        (head + m[:3], "f4WindowPops: between 4 and 6 MAF files are needed (3 given)"),
        (head + m[:7], "f4WindowPops: between 4 and 6 MAF files are needed (7 given)"),
        (head + pops_cli_cases.mafs(3), "f4WindowPops: between 4 and 6 MAF files are needed (3 given)"),
        (overlap + m[:4], "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0", "-out", out] + m[:4], "-jackknife 1 needs windows as its blocks"),
        (["-jackknife", "3"] + head + m[:4], "-jackknife must be 0 or 1 (given: 3)"),
        (["-winsize", "4", "-stepsize", "4", "-out", out] + m[:4], "Must supply size file unless -fixedsite 1"),
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "4"] + m[:4], "Must supply -out PREFIX"),
        (head + m[:3] + [str(tmp_path / "missing.mafs")], "Unable to open Pop4 MAF file"),
        (head + m[:3] + [other], "f4WindowPops: the MAF files share no site"),
    ]
    for args, msg in cases:
        r = run([tool] + args, {})
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr, (args, r.returncode, r.stderr)
        assert [f for f in os.listdir(tmp_path) if f.startswith("o.")] == [], args
    # -jackknife 1 with -stepsize below -winsize: exit 255 and f3WindowPops' own words
    r4, r3 = run([tool] + overlap + m[:4], {}), run([f3] + overlap + m[:4], {})
    assert r4.returncode == r3.returncode == 255 and r4.stderr == r3.stderr != "" and r4.stdout == r3.stdout == ""
    r = run([tool, "-jackknife", "1"] + head + m[:4], {})  # the same files and options, unharmed, run
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("o.")) == ["o.global", "o.jackknife", "o.pop1_pop2_pop3_pop4.f4"]
    rows = helpers.parse_tsv(open(out + ".pop1_pop2_pop3_pop4.f4").read())
    assert [r[1:4] + r[7:] for r in rows] == [["1", "4", "2", "4", "0"], ["5", "8", "6", "4", "0"]]
    jack = helpers.parse_tsv(open(out + ".jackknife").read())
    assert [g[:4] for g in jack] == [["1", "2", "3", "4"], ["1", "3", "2", "4"], ["1", "4", "2", "3"]] and all(len(g) == 10 and g[8:] == ["2", "8"] for g in jack)
