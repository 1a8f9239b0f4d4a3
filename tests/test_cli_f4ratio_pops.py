"""GPU: `bin/f4ratioWindowPops` — f4-ratio admixture proportions of all middle triples from K MAF files, the first being A and the
last the outgroup.  Every PREFIX.pop<i>_pop<j>_pop<k>.f4ratio, PREFIX.global and PREFIX.jackknife is held to what the NumPy models
of the definitions (tests/f4ratio_pops_model.py, tests/f4ratio_jack_model.py) and the Python mirror f4ratio_window_pops give
for the sites all files list, formatted by the tool's rules: labels and integers byte for byte, the ratio columns numerically.

The bound on a printed ratio alpha = N / D is derived from the contract's bound on the two sums, dN = 1e-9 A_N + 1e-12 and
dD = 1e-9 A_D + 1e-12 (A the window's Σ|product| of the sum): |N'/D' - N/D| <= (dN + |alpha| dD) / (|D| - dD), plus half a
unit of the sixth digit of %g; a ratio whose |D| does not exceed dD is not compared (the sums' contract says nothing about it),
and the test asserts that this leaves nearly all of them, the genome-wide ones among them.  The frequencies come from the
admixture tree of tests/f4ratio_pops_model.py, so the genome-wide denominators are well away from zero.
The row files are the same with and without -jackknife 1; stdout stays empty; each refusal has its exit code and message."""
import os

import numpy as np
import pytest

import f4ratio_jack_model
import f4ratio_pops_model as model
import helpers
import pops_cli_cases
from f4ratio_pops_model import RATIOS, SUMS, middle_triple_order
from test_cli_dstat_pops import MODES
from test_cli_f4_pops import listed, table_for
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pops import run, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "f4ratioWindowPops")


def ratios_with_bounds(s, a):
    """s, a: the three sums and their Σ|product| -> six (alpha, slack or None): slack from the sums' contract, None where the
    denominator is within its own bound of zero"""
    out = []
    for (sn, n), (sd, d) in RATIOS:
        N, D = sn * float(s[n]), sd * float(s[d])
        dN, dD = 1e-9 * float(a[n]) + 1e-12, 1e-9 * float(a[d]) + 1e-12
        alpha = float(model.q(N, D))
        if float(a[n]) == 0.0 and float(a[d]) == 0.0:  # no counted site, or only zero terms: both sums are exactly 0 on either side
            out.append((0.0, 0.0))
            continue
        out.append((alpha, (dN + abs(alpha) * dD) / (abs(D) - dD) if abs(D) > dD else None))
    return out


def expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing):
    """-> ({(i, j, k): rows of PREFIX.pop<i>_pop<j>_pop<k>.f4ratio or None}, rows of PREFIX.global, the model's rows), i, j, k
    the files' numbers on the command line"""
    rows, tot, A, A_tot = model.model(pos, freqs, ninds, minind, win)
    files, glob = {}, []
    for t, q in enumerate(middle_triple_order(len(freqs))):
        lines = []
        for w, (wd, r) in enumerate(zip(win, rows[t])):
            if skip_missing and int(r["n"]) == 0:
                continue
            n = int(r["n"])
            vals = ratios_with_bounds([r[f] for f in SUMS], [A[f][t][w] for f in SUMS])
            lines.append([names[int(wd["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))] + vals
                         + [str(n), str(int(wd["hi"]) - int(wd["lo"]) - n)])
        files[tuple(x + 1 for x in q)] = lines if W > 0 else None
        glob.append([str(x + 1) for x in q] + ratios_with_bounds([tot[t][f] for f in SUMS], [A_tot[f][t] for f in SUMS])
                    + [str(int(tot[t]["neff"])), str(int(tot[t]["nskip"]))])
    return files, glob, rows


def close_ratio(text, want, seen):
    y, slack = want
    assert text == "%g" % float(text), text
    seen[slack is not None] += 1
    return slack is None or abs(float(text) - y) <= 5.1e-6 * abs(y) + slack + helpers.ABS


def file_of(prefix, q):
    return f"{prefix}." + "_".join(f"pop{x}" for x in q) + ".f4ratio"


def check_outputs(prefix, files, glob, what):
    seen = {True: 0, False: 0}
    for q, want in files.items():
        path = file_of(prefix, q)
        if want is None:
            assert not os.path.exists(path), what
            continue
        got = helpers.parse_tsv(open(path).read())
        assert len(got) == len(want), (what, q, len(got), len(want))
        for g, w in zip(got, want):
            assert len(g) == 12 and g[:4] == w[:4] and g[10:] == w[10:], (what, q, g, w)
            assert all(close_ratio(g[c], w[c], seen) for c in range(4, 10)), (what, q, g, w)
            if w[10] == "0":
                assert g[4:10] == ["0"] * 6, (what, q, g)  # no analyzed site: every ratio is 0 by the convention
    got = helpers.parse_tsv(open(prefix + ".global").read())
    assert len(got) == len(glob) == len(files)
    for g, w in zip(got, glob):
        assert len(g) == 11 and g[:3] == w[:3] and g[9:] == w[9:], (what, g, w)
        assert all(w[c][1] is not None and close_ratio(g[c], w[c], seen) for c in range(3, 9)), (what, g, w)
    assert seen[True] > 20 * seen[False], (what, seen)  # nearly every printed ratio was compared


def check_against_the_python_mirror(pgt, prefix, chr_ids, pos, freqs, ninds, W, S, fixedsite, skip_missing, minind, chr_len, what):
    """the same run through f4ratio_window_pops: as many rows per triple, coordinates and counts byte for byte, the ratios (one
    division of the same sums) at print precision"""
    res = pgt.f4ratio_window_pops(chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len=None if fixedsite else chr_len, skip_missing=skip_missing)
    assert list(res) == middle_triple_order(len(freqs))
    glob = helpers.parse_tsv(open(prefix + ".global").read())
    for t, q in enumerate(res):
        tot = res[q].total
        assert glob[t][:3] == [str(x + 1) for x in q] and glob[t][9:] == [str(int(tot["neff"])), str(int(tot["nskip"]))], (what, q)
        for c, a in enumerate(pgt.f4ratio_alphas(tot)):
            assert close_g6(glob[t][3 + c], float(a)), (what, q, c)
        if W == 0:
            continue
        got = helpers.parse_tsv(open(file_of(prefix, tuple(x + 1 for x in q))).read())
        rows = res[q].rows
        assert len(got) == rows.size, (what, q)
        for g, r, al in zip(got, rows, pgt.f4ratio_alphas(rows)):
            assert g[1:4] == [str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))] and g[10] == str(int(r["n"])), (what, q, g, r)
            for c in range(6):
                assert close_g6(g[4 + c], float(al[c])), (what, q, c, g, r)


@pytest.mark.parametrize("k", [5, 6])
def test_files_equal_the_models_on_the_common_sites(pgt, tool, tmp_path, k):
    rng = np.random.default_rng(970 + k)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 420)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    keeps = (0.95, 0.9, 0.92, 0.97, 0.94, 0.96)[:k]
    tables = [[] for _ in range(k)]
    for c in chroms:  # the admixture tree at every position of the universe; each file lists its own subset of them
        f, _ = model.admixture_inputs(rng, uni[c].size, k)
        for p in range(k):
            here = rng.random(uni[c].size) < keeps[p]
            tables[p] += [(c, int(s), float(np.round(x, 6)), int(rng.integers(3, 21))) for s, x in zip(uni[c][here], f[p][here])]
    tables[1] = [r for r in tables[1] if r[0] != "chrB" or r[1] > 2000]  # half a chromosome is missing from one file
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == chroms and pos.size > 200
    assert len({len(t) for t in tables}) > 2 and all(len(t) > pos.size for t in tables)  # differing site lists: the alignment matters
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
    triples = [tuple(x + 1 for x in q) for q in middle_triple_order(k)]
    assert triples[0] == (2, 3, 4)  # the file numbers of the command line: file 1 is A
    dropped = False
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        win = table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len)
        files, glob, rows = expected_files(names, pos, freqs, ninds, win, W, minind, skip_missing)
        if skip_missing and W:
            every, _, _ = expected_files(names, pos, freqs, ninds, win, W, minind, 0)
            dropped = dropped or any(len(files[t]) < len(every[t]) for t in files)
        prefix = str(tmp_path / f"m{mi}" / "o")
        want_names = sorted(([os.path.basename(file_of("o", q)) for q in triples] if W else []) + ["o.global"])
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
        assert len(got) == 6 * len(triples)
        line = 0
        for t, q in enumerate(middle_triple_order(k)):  # ALL windows are blocks, whatever -skip_missing is
            want6 = f4ratio_jack_model.jack_rows(rows[t], f4ratio_jack_model.jack_float)
            assert want6[0]["n_blocks"] >= 8
            for (B, X, C), want in zip(pgt.ratio_order(*q), want6):
                g = got[line]
                line += 1
                assert len(g) == 9 and g[:3] == [str(p + 1) for p in (B, X, C)], (q, g)
                assert g[7] == str(want["n_blocks"]) and g[8] == str(want["n_sites"]), (q, g, want)
                for col, key in ((3, "alpha"), (4, "alpha_jack"), (5, "se"), (6, "z")):
                    if want[key] != want[key]:
                        assert g[col] == "nan", (q, key, g)
                    else:
                        assert g[col] == "%g" % float(g[col]) and close_g6(g[col], want[key]), (q, key, g, want)
                assert float(g[5]) > 0
    assert dropped, "-skip_missing 1 must have had a row to drop"
    plain, zero = str(tmp_path / "m4" / "o"), str(tmp_path / "m4_jack0" / "o")  # -jackknife 0 is the run without the option
    assert listed(zero) == listed(plain)
    for name in listed(plain):
        assert open(os.path.join(os.path.dirname(zero), name), "rb").read() == open(os.path.join(os.path.dirname(plain), name), "rb").read(), name


def test_refusals_exit_codes_and_messages(tool, tmp_path):
    row = "chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd\n"
    m = [str(tmp_path / f"p{k}.mafs") for k in range(8)]
    for n, p in enumerate(m):
        open(p, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.{(3 * s + n * n) % 10}00000\t5\n" for s in range(1, 9)))
    other = str(tmp_path / "other.mafs")
    open(other, "w").write(row + "".join(f"c1\t{s}\tA\tC\tA\t0.500000\t5\n" for s in range(100, 104)))
    out = str(tmp_path / "o")
    head = ["-fixedsite", "1", "-winsize", "4", "-stepsize", "4", "-out", out]
    f4 = os.path.join(BIN, "f4WindowPops")
    overlap = ["-jackknife", "1", "-fixedsite", "1", "-winsize", "4", "-stepsize", "2", "-out", out]
    cases = [
        (head + m[:4], "f4ratioWindowPops: between 5 and 7 MAF files are needed (4 given)"),
        (head + m[:8], "f4ratioWindowPops: between 5 and 7 MAF files are needed (8 given)"),
        (head + pops_cli_cases.mafs(4), "f4ratioWindowPops: between 5 and 7 MAF files are needed (4 given)"),
        (overlap + m[:5], "-jackknife 1 needs windows that do not overlap: -stepsize (2) must not be below -winsize (4)"),
        (["-jackknife", "1", "-fixedsite", "1", "-winsize", "0", "-out", out] + m[:5], "-jackknife 1 needs windows as its blocks"),
        (["-jackknife", "2"] + head + m[:5], "-jackknife must be 0 or 1 (given: 2)"),
        (["-winsize", "4", "-stepsize", "4", "-out", out] + m[:5], "Must supply size file unless -fixedsite 1"),
        (["-fixedsite", "1", "-winsize", "4", "-stepsize", "4"] + m[:5], "Must supply -out PREFIX"),
        (head + m[:4] + [str(tmp_path / "missing.mafs")], "Unable to open Pop5 MAF file"),
        (head + m[:4] + [other], "f4ratioWindowPops: the MAF files share no site"),
    ]
    for args, msg in cases:
        r = run([tool] + args, {})
        assert r.returncode == 255 and r.stdout == "" and msg in r.stderr, (args, r.returncode, r.stderr)
        assert [f for f in os.listdir(tmp_path) if f.startswith("o.")] == [], args
    # -jackknife 1 with -stepsize below -winsize: exit 255 and f4WindowPops' own words
    r5, r4 = run([tool] + overlap + m[:5], {}), run([f4] + overlap + m[:5], {})
    assert r5.returncode == r4.returncode == 255 and r5.stderr == r4.stderr != "" and r5.stdout == r4.stdout == ""
    r = run([tool, "-jackknife", "1"] + head + m[:5], {})  # the same files and options, unharmed, run
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("o.")) == ["o.global", "o.jackknife", "o.pop2_pop3_pop4.f4ratio"]
    rows = helpers.parse_tsv(open(out + ".pop2_pop3_pop4.f4ratio").read())
    assert [len(r) for r in rows] == [12, 12] and [r[1:4] + r[10:] for r in rows] == [["1", "4", "2", "4", "0"], ["5", "8", "6", "4", "0"]]
    glob = helpers.parse_tsv(open(out + ".global").read())
    assert len(glob) == 1 and glob[0][:3] == ["2", "3", "4"] and glob[0][9:] == ["8", "0"]
    jack = helpers.parse_tsv(open(out + ".jackknife").read())
    assert [g[:3] for g in jack] == [["2", "3", "4"], ["3", "2", "4"], ["2", "4", "3"], ["4", "2", "3"], ["3", "4", "2"], ["4", "3", "2"]]
    assert all(len(g) == 9 and g[7:] == ["2", "8"] for g in jack)
