"""GPU: bin/piWindowPops — windowed nucleotide diversity of each of K populations from K MAF files.  Every per-population
file and PREFIX.global is held to what the NumPy model of the spec (tests/pi_pops_model.py) prints for the sites all files
list (one file: all its sites): labels and integers byte for byte, the pi column numerically as the other command-line tests
do."""
import os

import numpy as np
import pytest

import helpers
import pi_pops_model
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pops import random_rows, run, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hosts():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return {t: os.path.join(BIN, t) for t in ("piWindowPops", "dxyWindowPops", "fstWindowPops")}


def expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing):
    """-> ([rows of PREFIX.pop<i>.pi or None per population], lines of PREFIX.global)"""
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import run_lengths
    rl = run_lengths(chr_ids)
    if W == 0:
        win = np.zeros(0, dtype=WIN_DTYPE)
    elif fixedsite:
        win = pgt.build_windows_sites(rl, W, S)
    else:
        win = pgt.build_windows_bp(pos, rl, chr_len, W, S)
    rows, tot = pi_pops_model.model(pos, freqs, ninds, minind, win)
    files, glob = [], []
    for p in range(len(freqs)):
        lines = []
        for w, r in zip(win, rows[p]):
            if skip_missing and int(r["neff"]) == 0:
                continue
            lines.append([names[int(w["label_run"])], str(int(r["start"])), str(int(r["end"])), float(r["sum"]), str(int(r["neff"])), str(int(r["nskip"]))])
        files.append(lines if W > 0 else None)
        glob.append([str(p + 1), float(tot[p]["sum"]), str(int(tot[p]["neff"])), str(int(tot[p]["nskip"]))])
    return files, glob


def check_outputs(prefix, files, glob, what):
    for p, want in enumerate(files):
        path = f"{prefix}.pop{p + 1}.pi"
        if want is None:
            assert not os.path.exists(path), what
            continue
        got = helpers.parse_tsv(open(path).read())
        assert len(got) == len(want), (what, p, len(got), len(want))
        for g, w in zip(got, want):  # chr start end pi_sum neff nskip
            assert g[:3] == w[:3] and g[4:] == w[4:] and close_g6(g[3], w[3]), (what, p, g, w)
    got = helpers.parse_tsv(open(prefix + ".global").read())
    assert len(got) == len(glob)
    for g, w in zip(got, glob):  # i pi_sum neff nskip
        assert g[0] == w[0] and g[2:] == w[2:] and close_g6(g[1], w[1]), (what, g, w)


MODES = [  # (winsize, stepsize, fixedsite, skip_missing, minind)
    (500, 200, 0, 0, 5),   # bp windows with a sizefile
    (40, 15, 1, 0, 5),
    (1, 1, 1, 1, 5),       # the per-site output, rows without a counted site dropped
    (0, 0, 1, 0, 5),       # PREFIX.global alone
    (300, 300, 0, 1, 1),
]


@pytest.mark.parametrize("k", [1, 3])
def test_files_equal_the_model_on_the_common_sites(pgt, hosts, tmp_path, k):
    rng = np.random.default_rng(90 + k)
    chroms = ["chrA", "chrB", "chrC"]
    uni = {c: np.unique(rng.integers(1, 4000, 300)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    tables = [random_rows(rng, chroms, uni, keep) for keep in (0.9, 0.8, 0.85)[:k]]
    if k > 1:
        tables[1] = [r for r in tables[1] if r[0] != "chrB"]  # one chromosome is missing from one file
    for t in tables:  # nInd up to 20, as the project generates it
        t[:] = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in t]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == (["chrA", "chrC"] if k > 1 else chroms) and pos.size > 100
    assert len({len(t) for t in tables}) == k  # differing, non-nested lists
    paths = []
    for n, t in enumerate(tables):
        paths.append(str(tmp_path / (f"p{n}.mafs" + (".gz" if n == 1 else ""))))
        write_maf(paths[-1], t, gz=(n == 1))
    chr_len = np.array([int(uni[c].max()) + 137 for c in names], dtype=np.uint32)
    jobs = []
    for mi, m in enumerate(MODES):
        for ingest in "01":
            jobs.append(([hosts["piWindowPops"]] + options(*m, str(sizes)) + ["-out", str(tmp_path / f"o{mi}_{ingest}")] + paths, {"PGT_GPU_INGEST": ingest}))
    res = run_all(jobs)
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        files, glob = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing)
        if W == 1:
            assert any(len(f) < pos.size for f in files), "-skip_missing drops rows here"
        for g, ingest in enumerate("01"):
            r = res[2 * mi + g]
            what = (k, MODES[mi], ingest)
            assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (what, r.returncode, r.stderr)
            check_outputs(str(tmp_path / f"o{mi}_{ingest}"), files, glob, what)
        for p in range(1, k + 1):  # the two ingest paths give the same bytes
            a, b = (str(tmp_path / f"o{mi}_{g}.pop{p}.pi") for g in "01")
            if W:
                assert open(a, "rb").read() == open(b, "rb").read(), (MODES[mi], p)
        assert open(str(tmp_path / f"o{mi}_0.global"), "rb").read() == open(str(tmp_path / f"o{mi}_1.global"), "rb").read()


def test_one_file_equals_the_same_file_given_twice(hosts, tmp_path):
    rng = np.random.default_rng(95)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 300)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    table = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in random_rows(rng, chroms, uni, 0.9)]
    path = str(tmp_path / "p.mafs")
    write_maf(path, table)
    jobs = []
    for mi, m in enumerate(MODES):
        jobs.append(([hosts["piWindowPops"]] + options(*m, str(sizes)) + ["-out", str(tmp_path / f"one{mi}"), path], None))
        jobs.append(([hosts["piWindowPops"]] + options(*m, str(sizes)) + ["-out", str(tmp_path / f"two{mi}"), path, path], None))
    for r in run_all(jobs):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (r.returncode, r.stderr)
    for mi, m in enumerate(MODES):
        one_g = open(str(tmp_path / f"one{mi}.global")).read().splitlines()
        two_g = open(str(tmp_path / f"two{mi}.global")).read().splitlines()
        assert len(one_g) == 1 and len(two_g) == 2
        assert one_g[0].split("\t")[1:] == two_g[0].split("\t")[1:] == two_g[1].split("\t")[1:]
        if m[0]:
            one = open(str(tmp_path / f"one{mi}.pop1.pi"), "rb").read()
            assert len(one) > 0
            for p in (1, 2):
                assert open(str(tmp_path / f"two{mi}.pop{p}.pi"), "rb").read() == one, (m, p)


def test_refusals(hosts, tmp_path):
    tool = hosts["piWindowPops"]
    m = [str(tmp_path / f"p{k}.mafs") for k in range(9)]
    for p in m:
        write_maf(p, [("c1", 1, 0.5, 5)])
    base = [tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", str(tmp_path / "o")]
    cases = [
        ([tool, "-minind", "0", "-out", "o"] + m[:1], "-minind must be at least 1"),
        (base, "piWindowPops: between 1 and 8 MAF files are needed (0 given)"),
        (base + m, "piWindowPops: between 1 and 8 MAF files are needed (9 given)"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1"] + m[:1], "Must supply -out PREFIX"),
        ([tool, "-winsize", "2", "-stepsize", "1", "-out", "o"] + m[:1], "Must supply size file unless -fixedsite 1"),
        ([tool, "-bogus", "1", "-out", "o"] + m[:1], "Unknown command: -bogus"),
    ]
    for cmd, text in cases:
        r = run(cmd)
        assert r.returncode == 255 and text in r.stderr and r.stdout == "", (cmd, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "o.global"))
    # the shared parser's default is unchanged: the all-pairs tools still refuse ONE file with their own message
    for name in ("dxyWindowPops", "fstWindowPops"):
        r = run([hosts[name]] + base[1:] + m[:1])
        assert r.returncode == 255 and f"{name}: between 2 and 8 MAF files are needed (1 given)" in r.stderr and r.stdout == ""
