"""GPU: bin/fstWindowPops -estimator hudson — Hudson's FST of all pairs from K MAF files.  Every per-pair file and
PREFIX.global is held to what the NumPy model of the definition (tests/fst_hudson_model.py) prints for the sites all files
list: labels and integers byte for byte, the FST column numerically as the other command-line tests do; the counts also to
bin/dxyWindowPops; and -estimator wc to the output without the option, byte for byte."""
import os

import numpy as np
import pytest

import fst_hudson_model
import helpers
from test_cli_fst_pops import MODES, check_outputs, common_columns, options
from test_cli_pops import random_rows, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hosts():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return {t: os.path.join(BIN, t) for t in ("dxyWindowPops", "fstWindowPops")}


def expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing):
    """-> ({(i, j): rows of PREFIX.pop<i>_pop<j>.fst or None}, rows of PREFIX.global), from the Hudson model"""
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import pair_order, run_lengths
    rl = run_lengths(chr_ids)
    if W == 0:
        win = np.zeros(0, dtype=WIN_DTYPE)
    elif fixedsite:
        win = pgt.build_windows_sites(rl, W, S)
    else:
        win = pgt.build_windows_bp(pos, rl, chr_len, W, S)
    rows, tot = fst_hudson_model.model(pos, freqs, ninds, minind, win)
    files, glob = {}, []
    for p, (i, j) in enumerate(pair_order(len(freqs))):
        lines = []
        for w, r in zip(win, rows[p]):
            if skip_missing and int(r["n"]) == 0:
                continue
            nskip = int(w["hi"]) - int(w["lo"]) - int(r["n"])
            lines.append([names[int(w["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"])), float(r["fst"]), str(int(r["n"])), str(nskip)])
        files[(i + 1, j + 1)] = lines if W > 0 else None
        glob.append([str(i + 1), str(j + 1), fst_hudson_model.fst_of(float(tot[p]["asum"]), float(tot[p]["bsum"])), str(int(tot[p]["neff"])), str(int(tot[p]["nskip"]))])
    return files, glob


HUDSON_MODES = [MODES[0], MODES[1], MODES[3]]  # bp windows, site windows, the global-only form


@pytest.mark.parametrize("k", [2, 3])
def test_files_equal_the_model_and_wc_is_the_default(pgt, hosts, tmp_path, k):
    rng = np.random.default_rng(170 + k)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 300)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    tables = [random_rows(rng, chroms, uni, keep) for keep in (0.9, 0.8, 0.85)[:k]]
    tables[1] = [r for r in tables[1] if r[0] != "chrB"]  # one chromosome is missing from one file
    for t in tables:  # nInd up to 20, as the project generates it
        t[:] = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in t]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == ["chrA"] and pos.size > 100
    assert len({len(t) for t in tables}) == k  # differing site lists
    paths = []
    for n, t in enumerate(tables):
        paths.append(str(tmp_path / (f"p{n}.mafs" + (".gz" if n == 1 else ""))))
        write_maf(paths[-1], t, gz=(n == 1))
    chr_len = np.array([int(uni[c].max()) + 137 for c in names], dtype=np.uint32)
    fst, dxy = hosts["fstWindowPops"], hosts["dxyWindowPops"]
    jobs = []
    for mi, m in enumerate(HUDSON_MODES):
        for ingest in "01":
            jobs.append(([fst, "-estimator", "hudson"] + options(*m, str(sizes)) + ["-out", str(tmp_path / f"h{mi}_{ingest}")] + paths, {"PGT_GPU_INGEST": ingest}))
    for mi in (0, 1):
        o = options(*HUDSON_MODES[mi], str(sizes))
        jobs.append(([fst] + o + ["-estimator", "wc", "-out", str(tmp_path / f"w{mi}")] + paths, None))
        jobs.append(([fst] + o + ["-out", str(tmp_path / f"n{mi}")] + paths, None))
        jobs.append(([dxy] + o + ["-out", str(tmp_path / f"d{mi}")] + paths, None))
    res = run_all(jobs, workers=6)
    for j, r in zip(jobs, res):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)
    pairs = [(i, j) for i in range(1, k + 1) for j in range(i + 1, k + 1)]
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(HUDSON_MODES):
        files, glob = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing)
        for ingest in "01":
            check_outputs(str(tmp_path / f"h{mi}_{ingest}"), k, files, glob, (k, HUDSON_MODES[mi], ingest))
    for mi in (0, 1):
        for i, j in pairs:
            # -estimator wc is the output without the option, byte for byte — and not Hudson's
            w = open(str(tmp_path / f"w{mi}.pop{i}_pop{j}.fst"), "rb").read()
            assert w == open(str(tmp_path / f"n{mi}.pop{i}_pop{j}.fst"), "rb").read() and len(w) > 0
            h = open(str(tmp_path / f"h{mi}_0.pop{i}_pop{j}.fst"), "rb").read()
            assert h != w
            # the same windows and the same predicate as dxyWindowPops: columns 6 and 7 (dxy: chr start end dxy neff nskip)
            d = helpers.parse_tsv(open(str(tmp_path / f"d{mi}.pop{i}_pop{j}.dxy")).read())
            f = helpers.parse_tsv(h.decode())
            assert len(d) == len(f) > 0
            for x, y in zip(d, f):
                assert x[:3] == y[:3] and x[4:] == y[5:], (x, y)
        assert open(str(tmp_path / f"w{mi}.global"), "rb").read() == open(str(tmp_path / f"n{mi}.global"), "rb").read()
