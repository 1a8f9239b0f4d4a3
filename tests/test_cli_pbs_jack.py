"""GPU: `bin/pbsWindowPops -blockjack 1 -pbsn1 1` — PREFIX.jackknife against the float model of the definition
(tests/pbs_jack_model.py: jack_float) applied to the rows the NumPy model of the reduction (tests/pbs_pops_model.py) gives for the
sites all files list; PREFIX.pop<i>_pop<j>_pop<k>.pbsn1 and PREFIX.pbsn1.global against pbsn1_of on those rows; every .pbs file
and PREFIX.global byte for byte what a run without the options writes; and the list of files exactly the expected one.  K = 3 and
K = 4, both FST estimators, site windows and base-pair windows.  Printed values are compared at %g precision (close_g6 of the
other command-line tests); a PBSn1 may move, beside that, by what the contract's bound on the six sums lets the three PBS move
(the slack of tests/test_cli_pbs_pops.py: printed_values), propagated through pbs_x / (1 + s) to first order."""
import os

import numpy as np
import pytest

import helpers
import pbs_jack_model as model
import pbs_pops_model
from pbs_pops_model import all_trio_order
from test_cli_fst_pops import close_g6, common_columns, options
from test_cli_pbs_pops import close_value, listed, printed_values, table_for
from test_cli_pops import random_rows, run_all, write_maf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")
pytestmark = pytest.mark.gpu
MODES = [  # (winsize, stepsize, fixedsite, skip_missing, minind): disjoint windows, as the blocks must be
    (50, 50, 1, 0, 5),     # site windows
    (400, 400, 0, 0, 5),   # base-pair windows
]
ESTIMATORS = ("wc", "hudson")


@pytest.fixture(scope="module")
def tool():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return os.path.join(BIN, "pbsWindowPops")


def pbsn1_values(pgt, r, a):
    """-> [(value, slack)] of pbsn1_i, pbsn1_j, pbsn1_k of a model row or total"""
    pbs = printed_values(r, a)[:3]
    one_s = 1.0 + ((pbs[0][0] + pbs[1][0]) + pbs[2][0])
    n1 = pgt.pbsn1_of(r)
    total = sum(s for _, s in pbs)
    out = []
    for c in range(3):
        y = float(n1[c])
        slack = 2 * (pbs[c][1] + abs(y) * total) / abs(one_s) if np.isfinite(y) and one_s != 0 else 0.0
        out.append((y, slack))
    return out


@pytest.mark.parametrize("k", [3, 4])
def test_jackknife_and_pbsn1_files_and_untouched_other_files(pgt, tool, tmp_path, k):
    rng = np.random.default_rng(2016 + k)
    chroms = ["chrA", "chrB"]
    uni = {c: np.unique(rng.integers(1, 12000, 700)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    tables = [random_rows(rng, chroms, uni, keep) for keep in (0.95, 0.9, 0.92, 0.97)[:k]]
    for t in tables:  # nInd up to 20, as the project generates it
        t[:] = [(c, p, fr, int(rng.integers(0, 21))) for c, p, fr, _ in t]
    names, chr_ids, pos, freqs, ninds = common_columns(tables)
    assert names == chroms and pos.size > 700
    paths = []
    for n, t in enumerate(tables):
        paths.append(str(tmp_path / (f"p{n}.mafs" + (".gz" if n == 1 else ""))))
        write_maf(paths[-1], t, gz=(n == 1))
    chr_len = np.array([int(uni[c].max()) + 137 for c in names], dtype=np.uint32)
    jobs, tags = [], []
    for mi, m in enumerate(MODES):
        for est in ESTIMATORS:
            for tag, extra in (("with", ["-blockjack", "1", "-pbsn1", "1"]), ("without", [])):
                d = tmp_path / f"m{mi}_{est}_{tag}"
                os.makedirs(d)
                jobs.append(([tool] + options(*m, str(sizes)) + ["-estimator", est] + extra + ["-out", str(d / "o")] + paths, {}))
                tags.append((mi, est, tag))
    # options given as 0 are options not given; PBSn1 without windows writes its genome-wide file alone
    os.makedirs(tmp_path / "zero")
    jobs.append(([tool] + options(*MODES[0], str(sizes)) + ["-blockjack", "0", "-pbsn1", "0", "-out", str(tmp_path / "zero" / "o")] + paths, {}))
    os.makedirs(tmp_path / "global")
    jobs.append(([tool, "-fixedsite", "1", "-winsize", "0", "-minind", "5", "-pbsn1", "1", "-out", str(tmp_path / "global" / "o")] + paths, {}))
    for j, r in zip(jobs, run_all(jobs, workers=5)):
        assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (j[0], r.returncode, r.stderr)

    trios = all_trio_order(k)
    stems = [f"o.pop{i + 1}_pop{j + 1}_pop{kk + 1}" for i, j, kk in trios]
    plain = sorted([s + ".pbs" for s in stems] + ["o.global"])
    assert listed(str(tmp_path / "zero" / "o")) == plain and listed(str(tmp_path / "global" / "o")) == ["o.global", "o.pbsn1.global"]
    for name in plain:
        assert open(tmp_path / "zero" / name, "rb").read() == open(tmp_path / "m0_wc_without" / name, "rb").read(), name
    for mi, (W, S, fixedsite, skip_missing, minind) in enumerate(MODES):
        win = table_for(pgt, chr_ids, pos, W, S, fixedsite, chr_len)
        for est in ESTIMATORS:
            what = (k, est, MODES[mi])
            with_, without = tmp_path / f"m{mi}_{est}_with", tmp_path / f"m{mi}_{est}_without"
            assert listed(str(without / "o")) == plain, what
            assert listed(str(with_ / "o")) == sorted(plain + [s + ".pbsn1" for s in stems] + ["o.jackknife", "o.pbsn1.global"]), what
            for name in plain:
                assert open(with_ / name, "rb").read() == open(without / name, "rb").read(), (what, name)
            rows, tot, A, A_tot = pbs_pops_model.model(pos, freqs, ninds, minind, win, est)
            # ---- PREFIX.jackknife
            got = helpers.parse_tsv(open(with_ / "o.jackknife").read())
            assert len(got) == 6 * len(trios), what
            line = 0
            for t, ijk in enumerate(trios):
                assert int((rows[t]["n"] > 0).sum()) >= 12, what
                focal_lines = [(ijk[0], ijk[1], ijk[2]), (ijk[1], ijk[0], ijk[2]), (ijk[2], ijk[0], ijk[1])]
                for c, want in enumerate(model.jack_rows(rows[t], model.jack_float)):
                    g = got[line]
                    line += 1
                    assert len(g) == 10 and g[0] == ("pbs" if c < 3 else "pbsn1") and g[1:4] == [str(p + 1) for p in focal_lines[c % 3]], (what, ijk, g)
                    assert g[8] == str(want["n_blocks"]) and g[9] == str(want["n_sites"]), (what, ijk, g, want)
                    for col, key in ((4, "stat"), (5, "stat_jack"), (6, "se"), (7, "z")):
                        assert np.isfinite(want[key]), (what, ijk, c, key, want)
                        assert g[col] == "%g" % float(g[col]) and close_g6(g[col], want[key]), (what, ijk, c, key, g, want)
                    assert float(g[6]) > 0
            # ---- the PBSn1 files
            for t, (stem, ijk) in enumerate(zip(stems, trios)):
                got = helpers.parse_tsv(open(with_ / (stem + ".pbsn1")).read())
                assert len(got) == win.size, (what, ijk)
                for w, (g, wd, r) in enumerate(zip(got, win, rows[t])):
                    n = int(r["n"])
                    lead = [names[int(wd["label_run"])], str(int(r["start"])), str(int(r["end"])), str(int(r["mid"]))]
                    assert len(g) == 9 and g[:4] == lead and g[7:] == [str(n), str(int(wd["hi"]) - int(wd["lo"]) - n)], (what, ijk, g)
                    want = pbsn1_values(pgt, r, {s: A[s][t][w] for s in A})
                    assert all(close_value(g[4 + c], want[c]) for c in range(3)), (what, ijk, g, want)
            got = helpers.parse_tsv(open(with_ / "o.pbsn1.global").read())
            assert len(got) == len(trios)
            for t, (g, ijk) in enumerate(zip(got, trios)):
                assert len(g) == 8 and g[:3] == [str(p + 1) for p in ijk] and g[6:] == [str(int(tot[t]["neff"])), str(int(tot[t]["nskip"]))], (what, g)
                want = pbsn1_values(pgt, tot[t], {s: A_tot[s][t] for s in A_tot})
                assert all(close_value(g[3 + c], want[c]) for c in range(3)), (what, g, want)
            if mi == 0 and est == "wc":  # the genome-wide file does not depend on the windows
                assert open(tmp_path / "global" / "o.pbsn1.global", "rb").read() == open(with_ / "o.pbsn1.global", "rb").read()
