"""GPU: bin/dstatWindowPops — ABBA-BABA windows of all ingroup trios from K MAF files, the last being the outgroup.  Every
per-trio file and PREFIX.global is held to what the NumPy model of the definition (tests/dstat_pops_model.py) gives for the
sites all files list: labels and integers byte for byte, the float columns numerically at %g precision, as the other
command-line tests of the K-file front end compare."""
import os

import numpy as np
import pytest

import dstat_pops_model
import helpers
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pops import random_rows, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu

MODES = [  # (winsize, stepsize, fixedsite, skip_missing, minind)
    (500, 200, 0, 0, 5),   # base-pair windows
    (40, 15, 1, 0, 5),     # site windows
    (7, 7, 1, 1, 5),       # short site windows: some hold no counted site and are dropped
    (0, 0, 1, 0, 5),       # the global-only form
    (300, 300, 0, 1, 1),
]


@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "dstatWindowPops")


def expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing):
    """-> ({(i, j, k): rows of PREFIX.pop<i>_pop<j>_pop<k>.dstat or None}, rows of PREFIX.global), from the model"""
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import run_lengths, trio_order
    rl = run_lengths(chr_ids)
    if W == 0:
        win = np.zeros(0, dtype=WIN_DTYPE)
    elif fixedsite:
        win = pgt.build_windows_sites(rl, W, S)
    else:
        win = pgt.build_windows_bp(pos, rl, chr_len, W, S)
    rows, tot = dstat_pops_model.model(pos, freqs, ninds, minind, win)
    files, glob = {}, []
    for t, (i, j, k) in enumerate(trio_order(len(freqs))):
        lines = []
        for w, r in zip(win, rows[t]):
            if skip_missing and int(r["n"]) == 0:
                continue
            nskip = int(w["hi"]) - int(w["lo"]) - int(r["n"])
            lines.append([names[int(w["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"])),
                          float(r["d"]), float(r["bbaa"]), float(r["abba"]), float(r["baba"]), str(int(r["n"])), str(nskip)])
        files[(i + 1, j + 1, k + 1)] = lines if W > 0 else None
        d = float(dstat_pops_model.d_of(tot[t]["abba"], tot[t]["baba"]))
        glob.append([str(i + 1), str(j + 1), str(k + 1), d, float(tot[t]["bbaa"]), float(tot[t]["abba"]), float(tot[t]["baba"]),
                     str(int(tot[t]["neff"])), str(int(tot[t]["nskip"]))])
    return files, glob


def check_outputs(prefix, files, glob, what):
    listed = sorted(f for f in os.listdir(os.path.dirname(prefix)) if f.startswith(os.path.basename(prefix) + "."))
    base = os.path.basename(prefix)
    want_names = sorted([f"{base}.pop{i}_pop{j}_pop{k}.dstat" for (i, j, k), w in files.items() if w is not None] + [base + ".global"])
    assert listed == want_names, (what, listed)
    for (i, j, k), want in files.items():
        if want is None:
            continue
        got = helpers.parse_tsv(open(f"{prefix}.pop{i}_pop{j}_pop{k}.dstat").read())
        assert len(got) == len(want), (what, (i, j, k), len(got), len(want))
        for g, w in zip(got, want):
            assert len(g) == 10 and g[:4] == w[:4] and g[8:] == w[8:], (what, (i, j, k), g, w)
            assert all(close_g6(g[c], w[c]) for c in (4, 5, 6, 7)), (what, (i, j, k), g, w)
    got = helpers.parse_tsv(open(prefix + ".global").read())
    assert len(got) == len(glob) == len(files)
    for g, w in zip(got, glob):
        assert len(g) == 9 and g[:3] == w[:3] and g[7:] == w[7:], (what, g, w)
        assert all(close_g6(g[c], w[c]) for c in (3, 4, 5, 6)), (what, g, w)


@pytest.mark.parametrize("k", [4, 5])
def test_files_equal_the_model_on_the_common_sites(pgt, tool, tmp_path, k):
    rng = np.random.default_rng(270 + k)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 4000, 320)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    tables = [random_rows(rng, chroms, uni, keep) for keep in (0.95, 0.9, 0.92, 0.97, 0.93)[:k]]
    tables[1] = [r for r in tables[1] if r[0] != "chrB" or r[1] > 2000]  # half a chromosome is missing from one file
    for t in tables:  # nInd up to 20, as the project generates it
        t[:] = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in t]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == chroms and pos.size > 150
    assert len({len(t) for t in tables}) == k and all(len(t) > pos.size for t in tables)  # differing site lists: the alignment matters
    paths = []
    for n, t in enumerate(tables):
        gz = n in (1, k - 1)  # the outgroup and one ingroup file are compressed
        paths.append(str(tmp_path / (f"p{n}.mafs" + (".gz" if gz else ""))))
        write_maf(paths[-1], t, gz=gz)
    chr_len = np.array([int(uni[c].max()) + 137 for c in names], dtype=np.uint32)
    jobs = []
    for mi, m in enumerate(MODES):
        for ingest in ("01" if mi < 2 else "1"):
            jobs.append(([tool] + options(*m, str(sizes)) + ["-out", str(tmp_path / f"m{mi}_{ingest}" / "o")] + paths, {"PGT_GPU_INGEST": ingest}))
            os.makedirs(tmp_path / f"m{mi}_{ingest}")
    res = run_all(jobs, workers=4)
    for j, r in zip(jobs, res):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)
    dropped = False
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        files, glob = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing)
        assert len(files) == (k - 1) * (k - 2) * (k - 3) // 6
        if skip_missing and W:
            all_rows, _ = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, 0)
            dropped = dropped or any(len(files[t]) < len(all_rows[t]) for t in files)
        for ingest in ("01" if mi < 2 else "1"):
            check_outputs(str(tmp_path / f"m{mi}_{ingest}" / "o"), files, glob, (k, MODES[mi], ingest))
    assert dropped, "-skip_missing 1 must have had a row to drop"
