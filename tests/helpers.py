"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# float columns are compared numerically: |x - y| <= REL * |y| + ABS (north_star: 1e-9 relative;
# the absolute floor covers ratios of sums that cancel to ~0, SURVEY.md §7 hard parts)
REL, ABS = 1e-9, 1e-12


def load_golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def parse_table(text, kind):
    """fst / het text -> (names per run, chr run ids, pos, cols...) exactly as the tools tokenise it."""
    names, chr_ids, pos, c1, c2 = [], [], [], [], []
    for line in text.splitlines():
        if not line.strip():
            break
        tok = line.split()
        if not names or names[-1] != tok[0]:
            names.append(tok[0])
        chr_ids.append(len(names) - 1)
        pos.append(int(tok[1]))
        if kind == "fst":
            c1.append(float(tok[2]))
            c2.append(float(tok[3]))
        else:
            c1.append(int(tok[2]))
    chr_ids = np.array(chr_ids, dtype=np.uint32)
    pos = np.array(pos, dtype=np.uint64).astype(np.uint32)
    if kind == "fst":
        return names, chr_ids, pos, np.array(c1, dtype=np.float64), np.array(c2, dtype=np.float64)
    return names, chr_ids, pos, np.array(c1, dtype=np.int32)


def parse_tsv(stdout):
    return [ln.split("\t") for ln in stdout.splitlines() if ln]


def close(x, y):
    return abs(x - y) <= REL * abs(y) + ABS


def fmt_g(x):
    """std::cout << double with default precision == printf('%g')."""
    s = "%g" % x
    return s


def assert_rows_match_tsv(names, win, rows, stat_field, count_field, tsv_rows, with_mid=True):
    """Integers, coordinates and labels byte-exact against the reference TSV; the float column
    numerically (the TSV carries 6 significant digits, so the tolerance is half a unit of the
    6th digit on top of REL)."""
    assert len(rows) == len(tsv_rows), (len(rows), len(tsv_rows))
    for w, r, t in zip(win, rows, tsv_rows):
        assert names[int(w["label_run"])] == t[0]
        assert str(int(r["start"])) == t[1] and str(int(r["end"])) == t[2]
        k = 3
        if with_mid:
            assert str(int(r["mid"])) == t[3]
            k = 4
        ref = float(t[k])
        got = float(r[stat_field])
        assert abs(got - ref) <= 5.1e-6 * abs(ref) + 1e-12, (got, ref)
        assert str(int(r[count_field])) == t[k + 1]


def extreme_case_args(case, tmp_path):
    """Materialise a ref_extreme.json case: returns (in_path, W, cutoff, chrlen_path or None)."""
    paths = {}
    for name, text in case["files"].items():
        p = tmp_path / name
        p.write_text(text)
        paths[name] = str(p)
    a = case["args"]
    W = int(a[a.index("-winsize") + 1])
    chrlen = paths[a[a.index("-chrlen") + 1][1:]] if "-chrlen" in a else None
    cutoff = float(a[a.index("-cutoff") + 1]) if case["tool"] == "ihsWindow" else float(a[1])
    return paths["in.norm"], W, cutoff, chrlen


def write_bgzf(path, data: bytes, block=0xff00, level=6):
    """`data` as a bgzf file (what ANGSD writes its .mafs.gz with): independent gzip members of at most 64 KiB,
    each with the "BC" extra field giving its size, then the empty end-of-file member."""
    import struct
    import zlib
    out = bytearray()
    chunks = [data[o: o + block] for o in range(0, len(data), block)] + [b""]
    for c in chunks:
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        d = z.compress(c) + z.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(d) + 8 - 1)
        out += d + struct.pack("<II", zlib.crc32(c) & 0xFFFFFFFF, len(c))
    with open(path, "wb") as fh:
        fh.write(bytes(out))


def dxy_ref_cases(tmp_path, plain_text=False):
    """The reference-made dxyWindow fixtures (tests/golden/ref_dxy.json: written by make_golden.py only on an image
    with the real Boost.Iostreams, where oracle/Makefile builds the unmodified dxyWindow.cpp).  None when absent —
    the dxy oracle is then "parity unpinned".  Yields (case, argv tail with real paths, options dict); with
    plain_text the gzip members are inflated first (the oracle's text front end reads plain text only)."""
    import base64
    import gzip
    path = os.path.join(GOLDEN, "ref_dxy.json")
    if not os.path.exists(path):
        return None
    out = []
    for k, c in enumerate(json.load(open(path))["cases"]):
        d = tmp_path / f"dxyref{k}"
        d.mkdir()
        names = {}
        for name, b64 in c["files"].items():
            raw = base64.b64decode(b64)
            if plain_text and name.endswith(".gz"):
                raw, new = gzip.decompress(raw), name[:-3]
            else:
                new = name
            (d / new).write_bytes(raw)
            names["@" + name] = str(d / new)
        argv = [names.get(a, a) for a in c["args"]]
        opt = {"winsize": 0, "stepsize": 0, "minind": 1, "fixedsite": 0, "skip_missing": 0, "sizefile": None}
        for i in range(0, len(argv) - 2, 2):
            key = argv[i].lstrip("-")
            opt[key] = argv[i + 1] if key == "sizefile" else int(argv[i + 1])
        opt["maf1"], opt["maf2"] = argv[-2], argv[-1]
        out.append((c, argv, opt))
    return out


def small_step_cases():
    """tests/golden/ref_small_step.json: reference-made runs with S << W whose inputs are regenerated from a seed
    (tests/golden/make_golden.py: small_step_input).  Yields (case, columns dict, fst text, het text) per distinct input."""
    import sys
    sys.path.insert(0, GOLDEN)
    import make_golden
    cases = load_golden("ref_small_step.json")["cases"]
    seen = {}
    for c in cases:
        key = (c["seed"], c["n"], c["n_chr"])
        if key not in seen:
            chr_ids, pos, a, b, g, fst, het = make_golden.small_step_input(*key)
            seen[key] = {"chr_ids": chr_ids, "pos": pos, "a": a, "b": b, "g": g, "fst": fst, "het": het}
        yield c, seen[key]


def write_hand_walked_case(case, header, tmp_path):
    """Materialise one case of tests/golden/dxy_hand_walked.json -> (maf1 path, maf2 path, size file path or None)."""
    d = tmp_path / case["name"]
    d.mkdir(exist_ok=True)
    paths = []
    for key in ("pop1", "pop2"):
        p = d / (key + ".mafs")
        with open(p, "w") as f:
            f.write(header + "\n")
            for c, pos, fr, n in case[key]:
                f.write(f"{c}\t{pos}\tA\tC\tA\t{fr:.6f}\t{n}\n")
        paths.append(str(p))
    sz = None
    if case["sizes"]:
        sz = d / "sizes.txt"
        sz.write_text("".join(f"{c}\t{n}\n" for c, n in case["sizes"]))
        sz = str(sz)
    return paths[0], paths[1], sz


def hand_walked_product_expectation(case, run):
    """What the GPU host / C-ABI must give for a run of a hand-walked case: the reference's output, or — for the
    documented deliberate divergences — the output of the machine on the sites both files list."""
    if case["product"] == "same":
        return run["stdout"], run["stderr"]
    if case["product"].get("rc", 0) != 0:  # the product refuses this input (exit status, a phrase of the message); nothing on stdout
        return None, case["product"]["stderr_contains"]
    return case["product"]["stdout"], case["product"]["stderr"]


# ---- workspace contract (tests/test_workspace_contract.py) ---------------------------------------------------------------
GUARD = 4096


class GuardedBuffers:
    """The buffers one call receives (tree, out, tot, ...), carved from ONE allocation: every buffer starts 256-byte aligned
    and lies between guards of at least 4 KiB, which (with the slack up to the next 256 bytes) hold a seeded byte pattern.
    check() synchronises and asserts that no guard byte changed."""

    def __init__(self, sizes, seed, device):
        import torch
        self.spans, off = [], GUARD
        for s in sizes:
            self.spans.append((off, off + int(s)))
            off += (int(s) + 255) // 256 * 256 + GUARD
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        self.pattern = torch.randint(0, 256, (off,), dtype=torch.uint8, device=device, generator=gen)
        self.arena = self.pattern.clone()
        assert self.arena.data_ptr() % 256 == 0
        self.bufs = [self.arena[a:b] for a, b in self.spans]

    def check(self, what=""):
        import torch
        torch.cuda.synchronize()
        prev = 0
        for a, b in self.spans + [(self.arena.numel(), self.arena.numel())]:
            if not torch.equal(self.arena[prev:a], self.pattern[prev:a]):
                bad = torch.nonzero(self.arena[prev:a] != self.pattern[prev:a])[:4].flatten().tolist()
                raise AssertionError(f"{what}: guard bytes [{prev}, {a}) changed at offsets {[prev + x for x in bad]} "
                                     f"(buffers at {self.spans})")
            prev = b


def padded_column(x, fill, device, pad_bytes=GUARD):
    """x (numpy) as a 16-byte-aligned view into a larger device tensor whose pad_bytes before and after hold `fill`: a kernel
    that reads outside [0, n) picks up the fill value."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    k = pad_bytes // t.element_size()
    full = torch.full((t.numel() + 2 * k,), fill, dtype=t.dtype, device=device)
    full[k:k + t.numel()].copy_(t)
    view = full[k:k + t.numel()]
    assert view.data_ptr() % 16 == 0
    return view


EXT_POISON_NODE = np.array([(1e300, 0xFFFFFFFF, 0x40000000)], dtype=[("key", "<f8"), ("idx", "<u4"), ("count", "<u4")])


def poison_tree(tree, kind, other=None, ext=False):
    """Fill a tree workspace before a call.  kind 0: every byte 0xFF (a stale f64 is NaN, a stale count 0xFFFFFFFF) — for the
    extreme-score tree, whose query dereferences pos[node.idx], nodes {key +1e300, idx 0xFFFFFFFF (the index the query
    guards), count 2^30} instead, so that any stale node read wins the maximum and shows in the row; kind 1: `other`, the
    fully built tree of a different dataset of the same size (finite, indices below n); kind 2: zeros."""
    import torch
    if kind == 0:
        if ext:
            node = torch.from_numpy(EXT_POISON_NODE.view(np.uint8).copy()).to(tree.device)
            tree.view(-1, 16).copy_(node.expand(tree.numel() // 16, 16))
        else:
            tree.fill_(0xFF)
    elif kind == 1:
        tree.copy_(other[:tree.numel()])
    else:
        tree.zero_()


def rows_equal(got, want, what):
    """Structured rows equal bit for bit, the pad_ fields excepted; the message names the first differing row and field."""
    got, want = got.copy(), want.copy()
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, want.dtype, got.size, want.size)
    if "pad_" in got.dtype.names:
        got["pad_"] = 0
        want["pad_"] = 0
    if got.tobytes() == want.tobytes():
        return
    g8 = got.view(np.uint8).reshape(got.size, -1)
    w8 = want.view(np.uint8).reshape(want.size, -1)
    i = int(np.flatnonzero((g8 != w8).any(axis=1))[0])
    fields = [f for f in got.dtype.names if got[f][i].tobytes() != want[f][i].tobytes()]
    raise AssertionError(f"{what}: {int((g8 != w8).any(axis=1).sum())} of {got.size} rows differ; first row {i}, fields {fields}: "
                         f"got {got[i]}, want {want[i]}")
