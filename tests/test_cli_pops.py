"""bin/dxyWindowPops: dxy of all pairs from K MAF files.  Command-line behaviour and the refusals that come before any GPU
use are checked on CPU; the output is held to the shipped bin/dxyWindow on the same (or, for K > 2, the commonly
filtered) files — labels, coordinates, neff and nskip byte for byte, the dxy column within helpers.REL / helpers.ABS."""
import gzip
import itertools
import os
import subprocess

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popgenomicstools_amd", "bin")


@pytest.fixture(scope="module")
def hosts():
    from popgenomicstools_amd import build
    build.build_lib()
    build.build_hosts()
    return {t: os.path.join(BIN, t) for t in ("dxyWindow", "dxyWindowPops")}


def run(cmd, env=None):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


def run_all(jobs, workers=3):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda j: run(*j), jobs))


HEADER = "chromo\tposition\tmajor\tminor\tref\tknownEM\tnInd"


def write_maf(path, rows, gz=False):
    """rows: (chromosome, position, frequency, nInd)"""
    text = HEADER + "\n" + "".join(f"{c}\t{p}\tA\tC\tA\t{fr:.6f}\t{n}\n" for c, p, fr, n in rows)
    if gz:
        with gzip.open(path, "wt") as fh:
            fh.write(text)
    else:
        open(path, "w").write(text)


def random_rows(rng, chromosomes, universe, keep):
    rows = []
    for c in chromosomes:
        for p in universe[c][rng.random(universe[c].size) < keep]:
            rows.append((c, int(p), float(rng.integers(0, 1000001)) / 1e6, int(rng.integers(0, 12))))
    return rows


def compare_tsv(got_text, want_text, what):
    """chr start end dxy neff nskip: everything byte for byte but the dxy column, which is compared numerically with the
    project's standing bound (both sides are %g of sums that agree to the last bits: the printed digits differ only where a
    sum sits on a rounding boundary of the sixth digit)."""
    got, want = helpers.parse_tsv(got_text), helpers.parse_tsv(want_text)
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert g[:3] == w[:3] and g[4:] == w[4:], (what, g, w)
        x, y = float(g[3]), float(w[3])
        assert abs(x - y) <= helpers.REL * abs(y) + helpers.ABS, (what, g, w)


def compare_global(global_line, dxy_total_line, pair, what):
    g, w = global_line.split("\t"), dxy_total_line.strip().split("\t")
    assert g[:2] == [str(pair[0]), str(pair[1])] and g[3:] == w[1:], (what, g, w)
    x, y = float(g[2]), float(w[0])
    assert abs(x - y) <= helpers.REL * abs(y) + helpers.ABS, (what, g, w)


# ---- CPU: the command line ----------------------------------------------------------------------------------------------
def test_help_and_argument_refusals(hosts, tmp_path):
    tool = hosts["dxyWindowPops"]
    r = run([tool])
    assert r.returncode == 0 and "-out" in r.stdout and "-skip_missing" in r.stdout and "PGT_MAX_RESIDENT_SITES" in r.stdout
    assert "PGT_DXY_SYNC" in r.stdout and "One GPU" in r.stdout
    m = [str(tmp_path / f"p{k}.mafs") for k in range(9)]
    for p in m:
        write_maf(p, [("c1", 1, 0.5, 5)])
    base = [tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", str(tmp_path / "o")]
    cases = [
        (base + m[:1], "between 2 and 8 MAF files are needed (1 given)"),
        (base, "between 2 and 8 MAF files are needed (0 given)"),
        (base + m, "between 2 and 8 MAF files are needed (9 given)"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1"] + m[:2], "Must supply -out PREFIX"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "3", "-out", "o"] + m[:2], "-stepsize must not exceed -winsize"),
        ([tool, "-winsize", "0", "-sizefile", "s", "-out", "o"] + m[:2], "-winsize 0 (global dxy) requires -fixedsite 1"),
        ([tool, "-fixedsite", "1", "-winsize", "2", "-out", "o"] + m[:2], "Must specify a -stepsize > 0 when -winsize is > 0"),
        ([tool, "-winsize", "2", "-stepsize", "1", "-out", "o"] + m[:2], "Must supply size file unless -fixedsite 1"),
        ([tool, "-minind", "0", "-out", "o"] + m[:2], "-minind must be at least 1"),
        ([tool, "-bogus", "1", "-out", "o"] + m[:2], "Unknown command: -bogus"),
        (base + [m[0], str(tmp_path / "absent.mafs")], "Unable to open Pop2 MAF file"),
    ]
    for cmd, text in cases:
        r = run(cmd)
        assert r.returncode == 255 and text in r.stderr and r.stdout == "", (cmd, r.returncode, r.stderr)
    # the same words and exit codes as the two-population host, where the option exists there
    two = hosts["dxyWindow"]
    for opts in (["-fixedsite", "1", "-winsize", "2", "-stepsize", "3"], ["-winsize", "0", "-sizefile", "s"], ["-minind", "0"]):
        a, b = run([two] + opts + m[:2]), run([tool] + opts + ["-out", "o"] + m[:2])
        assert a.returncode == b.returncode == 255 and a.stderr == b.stderr


def test_refusals_after_the_parse(hosts, tmp_path):
    """Decided from the parsed run tables on the host, before the device is needed: differing first chromosomes, a
    chromosome in two blocks, inconsistent order, no common chromosome, a bad line, PGT_MAX_RESIDENT_SITES."""
    tool = hosts["dxyWindowPops"]
    base = [tool, "-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", str(tmp_path / "o")]

    def files(*tables):
        paths = []
        for k, rows in enumerate(tables):
            paths.append(str(tmp_path / f"f{k}.mafs"))
            write_maf(paths[-1], rows)
        return paths
    site = lambda c, p: (c, p, 0.25, 5)  # noqa: E731
    env = {"PGT_GPU_INGEST": "0"}
    r = run(base + files([site("cA", 1)], [site("cB", 1)]), env)
    assert r.returncode == 255 and "Chromosomes in MAF files differ" in r.stderr
    r = run(base + files([site("cA", 1), site("cB", 1), site("cC", 2)], [site("cA", 1), site("cC", 1), site("cB", 2)]), env)
    assert r.returncode == 255 and "chromosome cC" in r.stderr and "same order" in r.stderr, r.stderr
    r = run(base + files([site("cA", 1), site("cB", 1), site("cA", 2)], [site("cA", 1), site("cB", 1)], [site("cA", 1)]), env)
    assert r.returncode == 255 and "chromosome cA" in r.stderr and "two separate blocks" in r.stderr, r.stderr
    paths = files([site("cA", 1), site("cA", 2)], [site("cA", 1)])
    open(paths[1], "a").write("cA\t7\tA\tC\tA\t1.5\t3\n")
    r = run(base + paths, env)
    assert r.returncode == 255 and "cannot parse MAF line" in r.stderr and "line 3 of " + paths[1] in r.stderr
    paths = files([site("cA", p) for p in range(1, 11)], [site("cA", p) for p in range(1, 8)])
    r = run(base + paths, dict(env, PGT_MAX_RESIDENT_SITES="9"))
    assert r.returncode == 255 and "PGT_MAX_RESIDENT_SITES=9" in r.stderr and "no passes mode" in r.stderr and paths[0] in r.stderr
    assert not os.path.exists(str(tmp_path / "o.global"))  # refused, not truncated: nothing was written
    r = run(base + files([site("cA", 1)], [("cA", 1, 0.5, 5)][:0]), env)
    assert r.returncode == 255 and "holds no sites" in r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def read_outputs(prefix, k):
    out = {}
    for i, j in itertools.combinations(range(1, k + 1), 2):
        p = f"{prefix}.pop{i}_pop{j}.dxy"
        out[(i, j)] = open(p).read() if os.path.exists(p) else None
    return out, open(prefix + ".global").read().splitlines()


MODES = [  # (options, needs the size file)
    (["-winsize", "500", "-stepsize", "200"], True),
    (["-fixedsite", "1", "-winsize", "40", "-stepsize", "15"], False),
    (["-fixedsite", "1", "-winsize", "1", "-stepsize", "1"], False),
    (["-fixedsite", "1", "-winsize", "0"], False),
    (["-winsize", "300", "-stepsize", "300", "-skip_missing", "1"], True),
    (["-fixedsite", "1", "-winsize", "25", "-stepsize", "25", "-minind", "5"], False),
]


@pytest.mark.gpu
def test_two_files_equal_dxywindow(hosts, tmp_path):
    """K = 2 against the shipped bin/dxyWindow on the same files and options: every mode on identical, nested and
    non-nested lists, plain and gzip input, with the device parser and with the host parser."""
    rng = np.random.default_rng(77)
    chroms = ["chrA", "chrB", "chrC"]
    uni = {c: np.unique(rng.integers(1, 6000, 900)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 137}\n" for c in chroms))
    full = random_rows(rng, chroms, uni, 1.0)
    other = [(c, p, float(rng.integers(0, 1000001)) / 1e6, int(rng.integers(0, 12))) for c, p, _, _ in full]
    inputs = {
        "identical": (full, other),
        "nested": (full, [r for r in other if rng.random() < 0.7]),
        "nested the other way": ([r for r in full if rng.random() < 0.7], other),
        "non-nested": ([r for r in full if rng.random() < 0.8], [r for r in other if rng.random() < 0.8 or r[0] == "chrC"][3:]),
    }
    jobs, meta = [], []
    for n, ((kind, (rows1, rows2)), gz) in enumerate(itertools.product(inputs.items(), (False, True))):
        d = tmp_path / f"in{n}"
        d.mkdir()
        m1, m2 = str(d / ("p1.mafs.gz" if gz else "p1.mafs")), str(d / "p2.mafs")
        write_maf(m1, rows1, gz)
        write_maf(m2, rows2)
        # every mode on every kind of list; the compression and the parser alternate so that each meets every mode
        for mi, (opts, need_sizes) in enumerate(MODES):
            if (mi + n) % 2 and kind != "non-nested":
                continue
            o = opts + (["-sizefile", str(sizes)] if need_sizes else [])
            jobs.append(([hosts["dxyWindow"]] + o + [m1, m2], None))
            for ingest in ("0", "1"):
                prefix = str(d / f"out{mi}_{ingest}")
                jobs.append(([hosts["dxyWindowPops"]] + o + ["-out", prefix, m1, m2], {"PGT_GPU_INGEST": ingest}))
            meta.append((kind, gz, opts, str(d), mi))
    res = run_all(jobs)
    assert len(meta) >= 30
    for n, (kind, gz, opts, d, mi) in enumerate(meta):
        ref, pops = res[3 * n], res[3 * n + 1: 3 * n + 3]
        what = (kind, gz, opts)
        assert ref.returncode == 0, (what, ref.stderr)
        for ingest, r in zip("01", pops):
            assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (what, ingest, r.returncode, r.stderr)
            files, glob = read_outputs(os.path.join(d, f"out{mi}_{ingest}"), 2)
            global_only = "0" == opts[opts.index("-winsize") + 1]
            assert len(glob) == 1
            if global_only:
                assert files[(1, 2)] is None
                compare_global(glob[0], ref.stdout, (1, 2), what)
            else:
                compare_tsv(files[(1, 2)], ref.stdout, what)
                compare_global(glob[0], ref.stderr, (1, 2), what)
    # the device parser and the host parser give the same bytes
    for n, (kind, gz, opts, d, mi) in enumerate(meta):
        a, b = read_outputs(os.path.join(d, f"out{mi}_0"), 2), read_outputs(os.path.join(d, f"out{mi}_1"), 2)
        assert a == b, (kind, gz, opts)


@pytest.mark.gpu
def test_known_answers_through_the_new_tool(hosts, tmp_path):
    """The two-population rows of tests/golden/dxy_kat.json (recorded from the reference) come out of dxyWindowPops."""
    k = helpers.load_golden("dxy_kat.json")
    m1, m2, sz = str(tmp_path / "p1.mafs.gz"), str(tmp_path / "p2.mafs"), tmp_path / "sizes.txt"
    write_maf(m1, k["pop1"], gz=True)
    write_maf(m2, k["pop2"])
    assert k["header"] == HEADER
    sz.write_text("".join(f"{c}\t{n}\n" for c, n in k["sizes"]))
    for n, c in enumerate(k["cases"]):
        prefix = str(tmp_path / f"kat{n}")
        cmd = [hosts["dxyWindowPops"], "-winsize", str(c["winsize"]), "-stepsize", str(c["stepsize"]), "-minind", str(k["minind"]),
               "-fixedsite", str(c["fixedsite"]), "-skip_missing", str(c["skip_missing"]), "-out", prefix]
        if not c["fixedsite"]:
            cmd += ["-sizefile", str(sz)]
        r = run(cmd + [m1, m2])
        assert r.returncode == 0 and r.stdout == "", r.stderr
        files, glob = read_outputs(prefix, 2)
        if c["winsize"] == 0:
            assert files[(1, 2)] is None
            compare_global(glob[0], c["stdout"], (1, 2), n)
        else:
            compare_tsv(files[(1, 2)], c["stdout"], n)
            compare_global(glob[0], c["stderr"], (1, 2), n)


@pytest.mark.gpu
def test_four_files_with_differing_lists(hosts, tmp_path):
    """K = 4: each of the 6 pair files equals bin/dxyWindow on that pair's two files filtered to the sites all four list."""
    rng = np.random.default_rng(99)
    chroms = ["s1", "s2", "s3", "s4"]
    uni = {c: np.unique(rng.integers(1, 9000, 1500)) for c in chroms}
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join(f"{c}\t{int(uni[c].max()) + 55}\n" for c in chroms))
    tables = [random_rows(rng, [c for c in chroms if not (c == "s3" and k == 2)], uni, keep) for k, keep in enumerate((0.9, 0.8, 0.95, 0.85))]
    tables[1] = [r for r in tables[1] if r[0] != "s4"] + [("s9", 5, 0.5, 5)] + [r for r in tables[1] if r[0] == "s4"]  # a chromosome of its own in between
    common = set.intersection(*[{(c, p) for c, p, _, _ in t} for t in tables])
    assert len(common) > 500 and not any(c == "s3" for c, _ in common)
    raw, filt = [], []
    for k, t in enumerate(tables):
        raw.append(str(tmp_path / (f"raw{k}.mafs" + (".gz" if k == 1 else ""))))
        write_maf(raw[-1], t, gz=(k == 1))
        filt.append(str(tmp_path / f"common{k}.mafs"))
        write_maf(filt[-1], [r for r in t if (r[0], r[1]) in common])
    pairs = list(itertools.combinations(range(4), 2))
    for mi, (opts, need_sizes) in enumerate((MODES[0], MODES[1], MODES[3], MODES[5])):
        o = opts + (["-sizefile", str(sizes)] if need_sizes else [])
        jobs = [([hosts["dxyWindowPops"]] + o + ["-out", str(tmp_path / f"q{mi}_{g}")] + raw, {"PGT_GPU_INGEST": g}) for g in "01"]
        jobs += [([hosts["dxyWindow"]] + o + [filt[i], filt[j]], None) for i, j in pairs]
        res = run_all(jobs)
        for r in res:
            assert r.returncode == 0, (opts, r.stderr)
        for g in "01":
            files, glob = read_outputs(str(tmp_path / f"q{mi}_{g}"), 4)
            assert len(glob) == 6
            for n, (i, j) in enumerate(pairs):
                ref = res[2 + n]
                what = (opts, g, i, j)
                if opts[opts.index("-winsize") + 1] == "0":
                    assert files[(i + 1, j + 1)] is None
                    compare_global(glob[n], ref.stdout, (i + 1, j + 1), what)
                else:
                    compare_tsv(files[(i + 1, j + 1)], ref.stdout, what)
                    compare_global(glob[n], ref.stderr, (i + 1, j + 1), what)


@pytest.mark.gpu
def test_no_common_site_and_timing(hosts, tmp_path):
    a, b = str(tmp_path / "a.mafs"), str(tmp_path / "b.mafs")
    write_maf(a, [("cA", p, 0.5, 5) for p in range(1, 40, 2)])
    write_maf(b, [("cA", p, 0.5, 5) for p in range(2, 40, 2)])
    base = [hosts["dxyWindowPops"], "-fixedsite", "1", "-winsize", "2", "-stepsize", "1", "-out", str(tmp_path / "o")]
    for ingest in "01":
        r = run(base + [a, b], {"PGT_GPU_INGEST": ingest})
        assert r.returncode == 255 and r.stdout == "" and "dxyWindowPops: the MAF files share no site" in r.stderr
    write_maf(b, [("cA", p, 0.25, 5) for p in range(1, 40)])
    r = run(base + [a, b], {"PGT_HOST_TIMING": "1", "PGT_DEVICES": "0,0"})  # several entries: the first is used
    assert r.returncode == 0 and r.stdout == "" and "[pgt-host] align" in r.stderr and "[pgt-host] total" in r.stderr
    assert len(open(str(tmp_path / "o.pop1_pop2.dxy")).read().splitlines()) == 19
    r = run(base + [a, b], {"PGT_MAX_RESIDENT_SITES": "30", "PGT_GPU_INGEST": "1"})
    assert r.returncode == 255 and "PGT_MAX_RESIDENT_SITES=30" in r.stderr and b in r.stderr
