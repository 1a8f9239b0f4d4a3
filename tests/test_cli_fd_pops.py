"""GPU: `bin/dstatWindowPops -fd 1` — f_d and f_dM windows of all ingroup trios from K MAF files, the last being the outgroup.
Every PREFIX.pop<i>_pop<j>_pop<k>.fd and PREFIX.fd.global is held to what the NumPy model of the definition
(tests/fd_pops_model.py) gives for the sites all files list: labels and integers byte for byte, the float columns numerically
at %g precision, as tests/test_cli_dstat_pops.py compares.  Everything the tool writes without the option it writes with it,
byte for byte, and without the option it writes no file more than before."""
import os

import numpy as np
import pytest

import fd_pops_model
import helpers
from test_cli_dstat_pops import MODES
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pops import random_rows, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "dstatWindowPops")


def expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing):
    """-> ({(i, j, k): rows of PREFIX.pop<i>_pop<j>_pop<k>.fd or None}, rows of PREFIX.fd.global), from the model"""
    from popgenomicstools_amd._lib import WIN_DTYPE
    from popgenomicstools_amd.window_scan import run_lengths, trio_order
    rl = run_lengths(chr_ids)
    if W == 0:
        win = np.zeros(0, dtype=WIN_DTYPE)
    elif fixedsite:
        win = pgt.build_windows_sites(rl, W, S)
    else:
        win = pgt.build_windows_bp(pos, rl, chr_len, W, S)
    rows, tot, _, _ = fd_pops_model.model(pos, freqs, ninds, minind, win)
    files, glob = {}, []
    for t, (i, j, k) in enumerate(trio_order(len(freqs))):
        lines = []
        for w, r in zip(win, rows[t]):
            if skip_missing and int(r["n"]) == 0:
                continue
            nskip = int(w["hi"]) - int(w["lo"]) - int(r["n"])
            lines.append([names[int(w["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"])),
                          float(r["fd"]), float(r["fdm"]), float(r["num"]), float(r["fd_den"]), float(r["fdm_den"]), str(int(r["n"])), str(nskip)])
        files[(i + 1, j + 1, k + 1)] = lines if W > 0 else None
        glob.append([str(i + 1), str(j + 1), str(k + 1), float(fd_pops_model.ratio(tot[t]["num"], tot[t]["fd_den"])),
                     float(fd_pops_model.ratio(tot[t]["num"], tot[t]["fdm_den"])), float(tot[t]["num"]), float(tot[t]["fd_den"]),
                     float(tot[t]["fdm_den"]), str(int(tot[t]["neff"])), str(int(tot[t]["nskip"]))])
    return files, glob


def listed(prefix):
    base = os.path.basename(prefix)
    return sorted(f for f in os.listdir(os.path.dirname(prefix)) if f.startswith(base + "."))


def names_without_fd(prefix, trios, W, jackknife=False):
    base = os.path.basename(prefix)
    return sorted(([f"{base}.pop{i}_pop{j}_pop{k}.dstat" for i, j, k in trios] if W else []) + [base + ".global"] + ([base + ".jackknife"] if jackknife else []))


def check_fd_outputs(prefix, files, glob, what):
    for (i, j, k), want in files.items():
        path = f"{prefix}.pop{i}_pop{j}_pop{k}.fd"
        if want is None:
            assert not os.path.exists(path), what
            continue
        got = helpers.parse_tsv(open(path).read())
        assert len(got) == len(want), (what, (i, j, k), len(got), len(want))
        for g, w in zip(got, want):
            assert len(g) == 11 and g[:4] == w[:4] and g[9:] == w[9:], (what, (i, j, k), g, w)
            assert all(close_g6(g[c], w[c]) for c in (4, 5, 6, 7, 8)), (what, (i, j, k), g, w)
    got = helpers.parse_tsv(open(prefix + ".fd.global").read())
    assert len(got) == len(glob) == len(files)
    for g, w in zip(got, glob):
        assert len(g) == 10 and g[:3] == w[:3] and g[8:] == w[8:], (what, g, w)
        assert all(close_g6(g[c], w[c]) for c in (3, 4, 5, 6, 7)), (what, g, w)


@pytest.mark.parametrize("k", [4, 5])
def test_fd_files_equal_the_model_and_the_other_files_do_not_move(pgt, tool, tmp_path, k):
    rng = np.random.default_rng(370 + k)
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
    jobs, tags = [], []

    def add(tag, mode, extra, ingest):
        os.makedirs(tmp_path / tag)
        jobs.append(([tool] + options(*mode, str(sizes)) + extra + ["-out", str(tmp_path / tag / "o")] + paths, {"PGT_GPU_INGEST": ingest}))
        tags.append(tag)

    for mi, m in enumerate(MODES):
        add(f"m{mi}_plain", m, [], "1")
        for ingest in ("01" if mi < 2 else "1"):
            add(f"m{mi}_fd_{ingest}", m, ["-fd", "1"], ingest)
    add("m4_fd0", MODES[4], ["-fd", "0"], "1")
    add("m4_jack", MODES[4], ["-jackknife", "1"], "1")      # (300, 300): disjoint windows
    add("m4_fd_jack", MODES[4], ["-jackknife", "1", "-fd", "1"], "1")
    res = run_all(jobs, workers=4)
    for j, r in zip(jobs, res):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)
    from popgenomicstools_amd.window_scan import trio_order
    trios = [(i + 1, j + 1, kk + 1) for i, j, kk in trio_order(k)]
    dropped = False
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        files, glob = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, skip_missing)
        assert len(files) == len(trios)
        if skip_missing and W:
            all_rows, _ = expected_files(pgt, names, chr_ids, pos, freqs, ninds, W, S, minind, fixedsite, chr_len, 0)
            dropped = dropped or any(len(files[t]) < len(all_rows[t]) for t in files)
        plain = str(tmp_path / f"m{mi}_plain" / "o")
        without = names_without_fd(plain, trios, W)
        assert listed(plain) == without, (MODES[mi], "without -fd the files written are exactly those of before")
        for ingest in ("01" if mi < 2 else "1"):
            prefix = str(tmp_path / f"m{mi}_fd_{ingest}" / "o")
            what = (k, MODES[mi], ingest)
            want_names = sorted(without + ([f"o.pop{i}_pop{j}_pop{kk}.fd" for i, j, kk in trios] if W else []) + ["o.fd.global"])
            assert listed(prefix) == want_names, (what, listed(prefix))
            check_fd_outputs(prefix, files, glob, what)
            for name in without:  # the .dstat files and PREFIX.global: byte-identical to the run without -fd
                assert open(os.path.join(os.path.dirname(prefix), name), "rb").read() == open(os.path.join(os.path.dirname(plain), name), "rb").read(), (what, name)
    assert dropped, "-skip_missing 1 must have had a row to drop"
    # -fd 0 is the run without the option; -fd 1 and -jackknife 1 together do not interact
    W = MODES[4][0]
    plain, fd0 = str(tmp_path / "m4_plain" / "o"), str(tmp_path / "m4_fd0" / "o")
    assert listed(fd0) == listed(plain)
    jack, both, fd = str(tmp_path / "m4_jack" / "o"), str(tmp_path / "m4_fd_jack" / "o"), str(tmp_path / "m4_fd_1" / "o")
    assert listed(jack) == names_without_fd(jack, trios, W, jackknife=True)
    assert listed(both) == sorted(listed(jack) + [f"o.pop{i}_pop{j}_pop{kk}.fd" for i, j, kk in trios] + ["o.fd.global"])
    for name in listed(both):
        src = jack if name in listed(jack) else fd
        assert open(os.path.join(os.path.dirname(both), name), "rb").read() == open(os.path.join(os.path.dirname(src), name), "rb").read(), name
    assert os.path.getsize(both + ".jackknife") > 0
