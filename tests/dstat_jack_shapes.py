"""The launch arithmetic of the block jackknife (jack_plan / jack_work of csrc/pgt_internal.h) restated in Python, the table
sizes at which its kernels take another path, and the synthetic row tables the jackknife tests share
(tests/test_dstat_jack_cpu.py holds the constants to the literal definitions in csrc/ and to pgt_dstat_jackknife_work_bytes).

A trio's rows are cut into chunks of CHUNK consecutive blocks (one row per lane); the trio gets n_partials waves, wave p walks
the chunks [p * chunks_per_wave, (p + 1) * chunks_per_wave) and leaves one partial per phase; partials are re-added by one
wave, lane l taking partials l, l + 64, .. — so more than 64 partials is where a lane re-adds a second one."""
import functools

import numpy as np

from popgenomicstools_amd._lib import DSTAT_ROW_DTYPE

CHUNK = 64            # kJackChunk
MAX_PARTIALS = 1024   # kJackMaxPartials
MAX_TRIOS = 20        # kJackMaxTrios
WORDS_PER_PARTIAL = 5 + 3 + 3  # kJackTotalWords + 2 * kJackTopologies, 8 bytes each


def plan(n_win):
    """-> (chunks, chunks_per_wave, n_partials) of jack_plan(n_win)"""
    chunks = -(-n_win // CHUNK)
    if chunks == 0:
        return 0, 0, 0
    per_wave = -(-chunks // MAX_PARTIALS)
    return chunks, per_wave, -(-chunks // per_wave)


def work_bytes(n_trios, n_win):
    if not 1 <= n_trios <= MAX_TRIOS:
        return 0
    cap = min(plan(n_win)[0], MAX_PARTIALS)  # the bound of n_partials, monotone in n_win (n_partials itself drops at 1025 chunks)
    return max(256, -(-(n_trios * cap * 8 * WORDS_PER_PARTIAL) // 256) * 256)


N_WIN_SECOND_CHUNK = CHUNK * MAX_PARTIALS + 1  # 65 537: the smallest table at which some wave takes a second chunk
N_WIN_PARTIALS_ABOVE_64 = CHUNK * 64 + 1       # 4 097: the smallest at which an item has more than 64 partials
assert plan(N_WIN_SECOND_CHUNK - 1)[1] == 1 and plan(N_WIN_SECOND_CHUNK)[1] == 2
assert plan(N_WIN_PARTIALS_ABOVE_64 - 1)[2] == 64 and plan(N_WIN_PARTIALS_ABOVE_64)[2] == 65

SMALL_N_WIN = (0, 1, 2, 3, 63, 64, 65, 127, 129, 4096)
LARGE_N_WIN = (N_WIN_PARTIALS_ABOVE_64, N_WIN_SECOND_CHUNK)
EXACT_UP_TO = 4096  # blocks up to which the tests compare with the exact-rational model


@functools.lru_cache(maxsize=None)
def synth_rows(n_win, n_trios=MAX_TRIOS, seed=0):
    """[n_trios, n_win] DSTAT_ROW_DTYPE: per trio independent bbaa / abba / baba in (0, 50) — multiples of 2^-10, so that the
    exact model's integers stay short — and n in 1 ... 512; about one block in seven has n = 0 and NaN sums (a block that
    is not used must never reach a sum).  The coordinates and d are filled but mean nothing to the jackknife.  A table of
    fewer trios of the same n_win and seed is a prefix of this one.  Read-only."""
    rows = np.zeros((n_trios, n_win), dtype=DSTAT_ROW_DTYPE)
    for t in range(n_trios):
        rng = np.random.default_rng([seed, n_win, t])
        for f in ("bbaa", "abba", "baba"):
            rows[f][t] = rng.integers(1, 50 * 1024, n_win) / 1024.0
        rows["n"][t] = rng.integers(1, 513, n_win)
        empty = rng.random(n_win) < 1 / 7
        rows["n"][t][empty] = 0
        for f in ("bbaa", "abba", "baba"):
            rows[f][t][empty] = np.nan
        rows["start"][t] = np.arange(n_win) * 100 + 1
        rows["end"][t] = rows["start"][t] + 99
        rows["mid"][t] = rows["start"][t] + 49
        den = rows["abba"][t] + rows["baba"][t]
        rows["d"][t] = np.where(empty, 0.0, (rows["abba"][t] - rows["baba"][t]) / np.where(empty, 1.0, den))
    rows.setflags(write=False)
    return rows


GOLDEN_N_WIN = 4096  # the one shape whose exact evaluation takes a minute: recorded by tests/golden/make_dstat_jack_exact.py


@functools.lru_cache(maxsize=None)
def exact_reference(n_win):
    """[MAX_TRIOS][3] dicts (d, d_jack, se, z, n_sites, n_blocks) of synth_rows(n_win) from the exact-rational model: evaluated
    here for the small tables, read from tests/golden/dstat_jack_exact.json (the same evaluation, recorded) for 4 096 blocks."""
    import json
    import os

    import dstat_jack_model
    assert n_win <= EXACT_UP_TO
    if n_win == GOLDEN_N_WIN:
        rec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dstat_jack_exact.json")))
        assert rec["n_win"] == n_win and rec["n_trios"] == MAX_TRIOS and rec["seed"] == 0
        return [[{k: (float.fromhex(v) if isinstance(v, str) else v) for k, v in item.items()} for item in trio] for trio in rec["items"]]
    rows = synth_rows(n_win)
    out = []
    for t in range(MAX_TRIOS):
        out.append([{k: v for k, v in item.items() if k != "var"} for item in dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_exact)])
    return out


@functools.lru_cache(maxsize=None)
def float_reference(n_win, n_trios=MAX_TRIOS):
    import dstat_jack_model
    rows = synth_rows(n_win, n_trios)
    return [dstat_jack_model.jack_rows(rows[t], dstat_jack_model.jack_float) for t in range(n_trios)]


# Hand-checkable tables of one item: blocks (x, y, m) and what the definition gives, every value exact in f64 (the CPU test
# holds both models to them, the GPU test the kernels, bit for bit).
NAN = float("nan")
HAND_CASES = [
    ("two blocks", [(3, 1, 1), (1, 3, 1)], dict(d=0.0, d_jack=0.0, se=0.5, z=0.0, n_blocks=2, n_sites=2)),
    ("64 identical blocks", [(3, 1, 8)] * 64, dict(d=0.5, d_jack=0.5, se=0.0, z=NAN, n_blocks=64, n_sites=512)),
    ("one block", [(3, 1, 5)], dict(d=0.5, d_jack=0.5, se=NAN, z=NAN, n_blocks=1, n_sites=5)),
    ("an unused block between two used ones", [(3, 1, 1), (NAN, NAN, 0), (1, 3, 1)],
     dict(d=0.0, d_jack=0.0, se=0.5, z=0.0, n_blocks=2, n_sites=2)),
    # leaving the second block out leaves x + y = 0: theta_-2 = 0 by the ratio's convention; theta_J = 2 * 0.5 - (0.25 + 0) = 0.75,
    # tau = (0.5, 1), sigma^2 = (0.0625 + 0.0625) / 2
    ("a block with x + y = 0", [(0, 0, 1), (3, 1, 1)], dict(d=0.5, d_jack=0.75, se=0.25, z=3.0, n_blocks=2, n_sites=2)),
    ("no block", [], dict(d=0.0, d_jack=0.0, se=NAN, z=NAN, n_blocks=0, n_sites=0)),
]


def same_item(got, want):
    """equal value for value (NaN equals NaN, -0.0 equals 0.0); got / want: mappings with the six result fields"""
    for k in ("d", "d_jack", "se", "z"):
        a, b = float(got[k]), float(want[k])
        if not (a == b or (a != a and b != b)):
            return False
    return int(got["n_blocks"]) == int(want["n_blocks"]) and int(got["n_sites"]) == int(want["n_sites"])
