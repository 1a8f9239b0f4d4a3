// pgt_internal.h — shared between the HIP kernels, the C-ABI and the host window builders.
// Not part of the public interface (that is include/pgtwin.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "pgtwin.h"

namespace pgt {

constexpr int kWave = 64;        // gfx950 wavefront
constexpr int kRadix = 64;       // children per tree node above the leaf level = one lane each
constexpr int kLeafF64 = 128;    // sites per level-1 node for f64 columns: one 16-B load per lane
constexpr int kLeafI8 = 1024;    // sites per level-1 node for the int8 genotype column: 16 B per lane
constexpr int kLeafExt = 256;    // sites per level-1 node for the single-column extreme-score scan: 2 x 16 B per lane
constexpr int kMaxLevels = 8;

// Node sizes in bytes (all levels of one tree use the same node type).
constexpr size_t kNodeFst = 16;  // {double Σa, double Σb}
constexpr size_t kNodeHet = 8;   // {u32 nonmissing, u32 nhet}
constexpr size_t kNodeDxy = 16;  // {double Σd, u32 neff, u32 nskip}

struct TreeLayout {
    int n_levels = 0;                   // levels 1..n_levels exist
    uint64_t count[kMaxLevels] = {};    // nodes stored per level (level 1 padded to 64 * count[1])
    size_t offset[kMaxLevels] = {};     // byte offset of each level in the workspace
    size_t partials = 0;                // dxy only: byte offset of the build waves' partial sums (the genome-wide line)
    size_t bytes = 0;
};
// The build kernels of the f64 trees run on at most this many waves (512 workgroups of 4: what is resident at once, see
// build_grid in pgt_kernels.hip); the dxy build leaves one partial sum per wave behind the tree.
constexpr uint32_t kMaxBuildWaves = 2048;

inline int leaf_sites(int stat) { return stat == PGT_STAT_HET ? kLeafI8 : (stat == PGT_STAT_EXT ? kLeafExt : kLeafF64); }
inline size_t node_bytes(int stat) { return stat == PGT_STAT_HET ? kNodeHet : 16; }

// Level 1 and 2 come out of the streaming build kernel; higher levels are added while a level
// still has more than 64 nodes (so the top level is always reducible by one wave-wide load).
inline TreeLayout tree_layout_for(uint64_t leaf, size_t nb, uint64_t n_sites) {
    TreeLayout t;
    uint64_t n_l2 = (n_sites + leaf * kRadix - 1) / (leaf * kRadix);
    if (n_l2 == 0) n_l2 = 1;
    uint64_t c = n_l2 * kRadix;
    size_t off = 0;
    int k = 0;
    auto push = [&](uint64_t cnt) {
        t.count[k] = cnt;
        t.offset[k] = off;
        off += ((cnt * nb + 255) / 256) * 256;
        ++k;
    };
    push(c);       // level 1
    push(n_l2);    // level 2
    c = n_l2;
    while (c > (uint64_t)kRadix && k < kMaxLevels) {
        c = (c + kRadix - 1) / kRadix;
        push(c);
    }
    t.n_levels = k;
    t.bytes = off;
    return t;
}
inline TreeLayout tree_layout(int stat, uint64_t n_sites) {
    TreeLayout t = tree_layout_for((uint64_t)leaf_sites(stat), node_bytes(stat), n_sites);
    if (stat == PGT_STAT_DXY) {  // + one node per build wave: the genome-wide line is their sum (no upper levels needed for it)
        t.partials = t.bytes;
        t.bytes += (size_t)kMaxBuildWaves * kNodeDxy;
    }
    return t;
}

// Levels worth building when no window is longer than max_window sites (0 = unknown: all).
// Level k (k >= 2) has nodes of leaf*64^(k-1) sites; a window can only contain such a node if it
// is at least that long.  The levels the build kernel writes itself always exist: `built` = 2 for the f64
// trees (levels 1 and 2 leave the streaming kernel together), 1 for the int8 tree, whose level 2 (65536 sites)
// is a tree_up launch of its own — skipped for windows shorter than that (round 5: W = 50000).
inline int useful_levels_for(const TreeLayout &t, uint64_t leaf, uint64_t max_window, int built = 2) {
    if (max_window == 0) return t.n_levels;
    int k = built;
    uint64_t node = leaf * kRadix;  // level-2 node
    for (int j = 2; j <= built; ++j) node *= kRadix;  // the first level above the built ones
    while (k < t.n_levels && node <= max_window) {
        ++k;
        node *= kRadix;
    }
    return k;
}
inline int useful_levels(const TreeLayout &t, int stat, uint64_t max_window) {
    return useful_levels_for(t, (uint64_t)leaf_sites(stat), max_window, stat == PGT_STAT_HET ? 1 : 2);
}

// ---- allele-frequency front end (pgt_af_kernels.hip): nodes of V scalar sums, node-major ------
// A node is V consecutive doubles (V = NP + NP(NP-1)/2), the nodes of a level are contiguous: the 16
// level-1 nodes (512 sites each) a build wave finishes together are ONE contiguous block of 128*V bytes (4.5 KiB
// at 8 populations), and a query lane reads a node as one contiguous run.  Levels 2 and up are those of the
// f64 layout (8192 sites, x64 per level).
constexpr int kAfMaxPops = 8;
constexpr int kAfLeafPieces = 4;  // 128-site pieces per level-1 node of the AF tree (pgt_af_kernels.hip: kAfPieces)
struct AfTree {
    char *base;
    size_t off[kMaxLevels];  // byte offset of level slot k
    int n_levels;
    int n_vals;              // V: doubles per node
};
// the AF tree's level 1 holds 64 / kAfLeafPieces nodes per level-2 node (pgt_af_kernels.hip), a fraction of the f64 layout's count
inline size_t af_level_bytes(const TreeLayout &t, int k, int n_vals) {
    const uint64_t nodes = k == 0 ? t.count[0] / kAfLeafPieces : t.count[k];
    return ((nodes * (size_t)n_vals * 8 + 255) / 256) * 256;
}
inline size_t af_tree_bytes(const TreeLayout &t, int n_vals) {
    size_t b = 0;
    for (int k = 0; k < t.n_levels; ++k) b += af_level_bytes(t, k, n_vals);
    return b;
}
inline AfTree af_tree_view(const TreeLayout &t, int n_vals, void *tree, int levels) {
    AfTree v{};
    v.base = static_cast<char *>(tree);
    v.n_levels = levels;
    v.n_vals = n_vals;
    size_t off = 0;
    for (int k = 0; k < t.n_levels; ++k) {
        v.off[k] = off;
        off += af_level_bytes(t, k, n_vals);
    }
    return v;
}

// ---- the (freq, nInd) front ends: dxy and FST of all population pairs, pi per population ------
constexpr int kPopsMaxPops = 8;     // populations per call of pgt_{dxy,fst,pi}_pops_reduce*: sizes their pointer arrays
constexpr int kPopsLeafPieces = 4;  // 128-site pieces per level-1 node of the all-pairs trees below

// ---- the trees of the all-pairs / all-trios front ends (pgt_pops_walk.h): nodes of S sums and a count per item, node-major ------
// An item is a pair (dxy: P = NP(NP-1)/2 of {Σd}; FST: {Σa, Σ(a+b)}) or an ingroup trio (ABBA-BABA: T = C(NP-1, 3) of {Σbbaa,
// Σabba, Σbaba}).  A level holds two arrays: S * items doubles per node (sum 0 of item 0 .. items-1, then sum 1, ..) and
// items u32 per node (their neff); nskip is not stored (every site of a range is a data site: nskip = sites - neff).
// Level 1: 512-site nodes, 16 per level-2 node; levels 2 and up are those of the f64 layout (8192 sites, x64 per level).
// Behind the levels one such node per build wave: the genome-wide lines are their sums in wave order (as
// TreeLayout::partials for the two-population tree).
struct PopsTree {
    char *base;
    size_t sum_off[kMaxLevels];  // byte offset of level slot k: S * items doubles per node
    size_t cnt_off[kMaxLevels];  // ... items u32 per node
    size_t part_sum, part_cnt;   // [build wave][S * items] doubles / [build wave][items] u32
    size_t bytes;
    int n_levels;
    int n_items;
    uint32_t n_partials;         // build waves that left a partial (0: no sites)
};

// Its layout: per level and behind the levels an array of sums_per_item doubles per item and node (1: Σd; 2: Σa and Σ(a+b);
// 3: the three patterns) and an array of one u32 per item and node, each padded to 256 bytes.
inline PopsTree pops_tree_view(const TreeLayout &t, int n_items, int sums_per_item, void *tree, int levels) {
    PopsTree v{};
    v.base = static_cast<char *>(tree);
    v.n_levels = levels;
    v.n_items = n_items;
    const size_t sum_bytes = (size_t)8 * sums_per_item;
    auto pad = [](size_t b) { return ((b + 255) / 256) * 256; };
    size_t off = 0;
    for (int k = 0; k < t.n_levels; ++k) {
        const uint64_t nodes = k == 0 ? t.count[0] / kPopsLeafPieces : t.count[k];
        v.sum_off[k] = off;
        off += pad(nodes * (size_t)n_items * sum_bytes);
        v.cnt_off[k] = off;
        off += pad(nodes * (size_t)n_items * 4);
    }
    v.part_sum = off;
    off += pad((size_t)kMaxBuildWaves * n_items * sum_bytes);
    v.part_cnt = off;
    off += pad((size_t)kMaxBuildWaves * n_items * 4);
    v.bytes = off;
    return v;
}

// ---- delete-m_j block jackknife of a ratio of two block sums (pgt_dstat_jack_kernels.hip) -----------------------------------
// The rows of one trio are cut into chunks of kJackChunk consecutive blocks (one row per lane); a trio gets n_partials waves,
// wave p takes the chunks [p * chunks_per_wave, (p + 1) * chunks_per_wave) and leaves one partial per phase.  The plan is a
// function of n_win alone: the order of every addition is, and so are an item's bits whatever else the call holds.
constexpr uint32_t kJackChunk = 64;          // blocks a wave reads at once: 64 rows of 48 bytes, 3 KiB contiguous
constexpr uint32_t kJackMaxPartials = 1024;  // waves, and partials of each phase, per trio at most
constexpr uint32_t kJackMaxTrios = 20;       // C(6, 3): what pgt_dstat_pops_reduce_dev can write
constexpr int kJackTotalWords = 5;           // phase 1 per wave: Σbbaa, Σabba, Σbaba (f64), Σn (u64), used blocks (u64)
constexpr int kJackTopologies = 3;           // phases 2 and 3 per wave: one f64 per topology
constexpr int kJackRatioItems = 6;           // ... and per admixture proportion of a middle triple (pgt_f4ratio_jackknife_dev)
constexpr int kJackPbsItems = 6;             // ... and per PBS / PBSn1 of a trio's three focal populations (pgt_pbs_jackknife_dev)
constexpr int kJackSums = 3;                 // sums of a 48-byte row; a pgt_pbs_row has kJackPbsSums
constexpr int kJackPbsSums = 6;
constexpr int jack_total_words(int sums) { return sums + 2; }  // phase 1 per wave: the sums (f64), Σn (u64), used blocks (u64)
static_assert(jack_total_words(kJackSums) == kJackTotalWords, "the three-sum rows keep their five words");
struct JackPlan {
    uint64_t chunks = 0;           // ceil(n_win / kJackChunk)
    uint64_t chunks_per_wave = 0;  // ceil(chunks / kJackMaxPartials)
    uint32_t n_partials = 0;       // ceil(chunks / chunks_per_wave) <= kJackMaxPartials; 0 without a block
};
inline JackPlan jack_plan(uint64_t n_win) {
    JackPlan p;
    p.chunks = n_win / kJackChunk + (n_win % kJackChunk ? 1 : 0);
    if (p.chunks == 0) return p;
    p.chunks_per_wave = (p.chunks + kJackMaxPartials - 1) / kJackMaxPartials;
    p.n_partials = (uint32_t)((p.chunks + p.chunks_per_wave - 1) / p.chunks_per_wave);
    return p;
}
// The workspace, in 8-byte words: [trio][word k < 5][partial] of phase 1 (jack_total_words(sums): 8 for the six sums of a
// pgt_pbs_row), then [trio][topology][partial] of phase 2 and the same of phase 3.  Its SIZE is that of min(chunks, kJackMaxPartials) partials — what n_partials never exceeds, and monotone in n_win
// where n_partials itself is not (1025 chunks make 513 waves of two) — and 256 bytes at least (a call without blocks reads and
// writes none of it).
struct JackWork {
    size_t totals = 0, drop = 0, var = 0;  // byte offsets of the three phases' partials
    size_t bytes = 0;
};
// items: the estimator's items per table (kJackTopologies; the ratio of pgt_f4ratio_jackknife_dev: kJackRatioItems; PBS:
// kJackPbsItems); sums: the sums of a row (kJackSums; a pgt_pbs_row: kJackPbsSums — 8 + 6 + 6 = 20 words per partial)
inline JackWork jack_work(uint32_t n_trios, uint64_t n_win, int items = kJackTopologies, int sums = kJackSums) {
    JackWork w;
    const size_t per = (size_t)n_trios * jack_plan(n_win).n_partials * 8;
    w.totals = 0;
    w.drop = w.totals + per * jack_total_words(sums);
    w.var = w.drop + per * items;
    const JackPlan p = jack_plan(n_win);
    const size_t cap = (size_t)(p.chunks < kJackMaxPartials ? p.chunks : kJackMaxPartials);
    w.bytes = (((size_t)n_trios * cap * 8 * (jack_total_words(sums) + 2 * items) + 255) / 256) * 256;
    if (w.bytes == 0) w.bytes = 256;
    return w;
}
// 1 <= n_trios <= kJackMaxTrios and every pointer checked by the caller; ev_*: hipEvent_t as void* or NULL
int launch_dstat_jackknife(const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios, pgt_dstat_jack *out, void *work,
                           void *stream, void *ev_query0, void *ev_query1, std::string *err);
// the same phases with the mean estimator (F3Mean) over the rows of pgt_f3_pops_reduce_dev; plan and workspace as above
int launch_f3_jackknife(const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios, pgt_f3_jack *out, void *work,
                        void *stream, void *ev_query0, void *ev_query1, std::string *err);
// the mean estimator again, over the rows of pgt_f4_pops_reduce_dev: 1 <= n_quartets <= kJackMaxQuartets
constexpr uint32_t kJackMaxQuartets = 15;    // C(6, 4): what pgt_f4_pops_reduce_dev can write
int launch_f4_jackknife(const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets, pgt_f4_jack *out, void *work,
                        void *stream, void *ev_query0, void *ev_query1, std::string *err);
// the signed ratio of two block sums (Ratio), six items per table, over the rows of pgt_f4ratio_pops_reduce_dev:
// 1 <= n_triples <= kJackMaxTriples; the workspace is jack_work(n_triples, n_win, kJackRatioItems)
constexpr uint32_t kJackMaxTriples = 10;     // C(5, 3): what pgt_f4ratio_pops_reduce_dev can write
int launch_f4ratio_jackknife(const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples, pgt_f4ratio_jack *out, void *work,
                             void *stream, void *ev_query0, void *ev_query1, std::string *err);
// PBS and PBSn1 of a trio's three focal populations (Pbs), six items per table from the SIX sums of the 88-byte rows of
// pgt_pbs_pops_reduce_dev: 1 <= n_trios <= kJackMaxTrios; the workspace is jack_work(n_trios, n_win, kJackPbsItems, kJackPbsSums)
int launch_pbs_jackknife(const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios, pgt_pbs_jack *out, void *work,
                         void *stream, void *ev_query0, void *ev_query1, std::string *err);

// Speed-only hints of a context (pgt_set_max_window, pgt_set_window_step); 0 = unknown.
struct Hints {
    uint64_t max_window = 0;   // longest window in sites: tree levels with larger nodes are not built
    uint64_t window_step = 0;  // typical distance between consecutive window starts: selects the query strategy
    uint64_t typical_window = 0;  // typical window length where the library saw the table itself (host tables); 0: max_window stands for it
    uint32_t fst_build_blocks = 0;  // PGT_FST_BUILD_BLOCKS, read once by pgt_open: the fst build's workgroup cap instead of kFstBuildBlocks
                                    // (0: unset).  A testing knob: with 1, four waves walk the whole column, so a short column reaches any
                                    // number of tiles per wave (the deep stage of pgt_kernels.hip); rows and nodes do not depend on it
};
// ---- query strategies, chosen from the hints alone (the same on every rank when the hints are) ----------------
// step == 0 (unknown) or large: one wave per window.  0 < step <= kGroupMaxStep and windows of at least two level-2
// tiles (max-window hint): the GROUP query (64 consecutive windows per wave share tile scans, level-1 node scans and the
// interior) — it beats the sliding query at every step it applies to (10^8 sites, W = 50000: S = 1 2.85 against 4.10 ms,
// S = 8 0.65 against 1.80, S = 32 0.60 against 1.55; profiles/r03/measure_query_1e8_strategies.md).  Shorter windows
// with step <= kSlideMaxStep: the sliding query (per-site scans of 128-site tiles; it needs only 256-site windows).
constexpr uint64_t kSlideMaxStep = 32;
constexpr uint64_t kGroupMaxStep = 1024;  // above, a group's starts span too many level-2 tiles and there are too few groups to fill the chip (10^8 sites: a tie at 2048)
// Windows per wave of the sliding query for a given step (0 or 1 = not the sliding query).
inline uint32_t slide_group(uint64_t step) {
    if (step == 0 || step > kSlideMaxStep) return 1;
    const uint64_t g = 128 / step + 1;
    return (uint32_t)(g > 64 ? 64 : g);
}
// leaf = sites per level-1 node of the statistic's tree (its level-2 tiles are 64 leaves)
inline bool group_query(const Hints &h, uint64_t leaf) {
    const uint64_t typical = h.typical_window ? h.typical_window : h.max_window;
    return h.window_step > 0 && h.window_step <= kGroupMaxStep && typical >= 2 * leaf * kRadix;
}
// the group query's ragged ends: shared 128-site tile scans up to this step, per window above (see query_group_body)
inline int group_edge_scans(const Hints &h) { return h.window_step <= 64 ? 1 : 0; }
// Windows per wave of the group query: 64 when that still gives the chip ~8000 waves, else fewer (rows do not depend on it)
inline uint32_t group_size(uint64_t n_win) {
    return n_win >= 64ull * 8192 ? 64u : (n_win >= 32ull * 8192 ? 32u : 16u);
}

// What every launcher below ends in: where it runs, what it records, where its message goes, what it may assume
struct LaunchEnv {
    void *stream;                             // hipStream_t as void*
    void *ev_build0, *ev_build1, *ev_query1;  // hipEvent_t as void* or NULL: recorded before the build, behind it, behind the query
    std::string *err;
    const Hints &hints;
};

// ---- launchers implemented in pgt_kernels.hip ----------
int launch_fst(const uint32_t *pos, const double *const *a, const double *const *b, uint32_t n_pairs,
               uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, void *tree, const LaunchEnv &e);
int launch_het(const uint32_t *pos, const int8_t *g, uint64_t n, const pgt_win *win, uint64_t n_win,
               pgt_het_row *out, void *tree, const LaunchEnv &e);
int launch_dxy(const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
               const int32_t *n2, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
               pgt_dxy_row *out, pgt_dxy_total *tot, void *tree, const LaunchEnv &e);

int launch_dxy_het(const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
                   const int32_t *n2, const int8_t *g1, const int8_t *g2, uint64_t n, int minind,
                   const pgt_win *win, uint64_t n_win, pgt_dxy_row *dxy_out, pgt_dxy_total *tot,
                   pgt_het_row *het_out1, pgt_het_row *het_out2, void *tree, const LaunchEnv &e);

int launch_ext(const uint32_t *pos, const double *score, uint64_t n, int mode, double cutoff, const pgt_win *win,
               uint64_t n_win, pgt_ext_row *out, void *tree, const LaunchEnv &e);
int launch_fst_af(const uint32_t *pos, const double *const *freq, const double *nsamp, uint32_t n_pops,
                  uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, void *tree, const LaunchEnv &e);

// pgt_dxy_pops_kernels.hip: tot = n_pairs device totals or NULL; 2 <= n_pops <= 8 (checked by the caller)
int launch_dxy_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                    uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot,
                    void *tree, const LaunchEnv &e);

// pgt_fst_pops_kernels.hip: tot = n_pairs device totals or NULL; 2 <= n_pops <= 8 and minind >= 1 (checked by the caller).
// The estimator selects the per-site function the kernels are instantiated with (pgt_fst_pops_reduce_dev: WeirCockerham,
// pgt_fst_hudson_pops_reduce_dev: Hudson); tree layout, grids and the order of all additions are the same for both.
enum class FstPopsEstimator { WeirCockerham, Hudson };
int launch_fst_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                    uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot,
                    void *tree, const LaunchEnv &e, FstPopsEstimator estimator);

// pgt_dstat_pops_kernels.hip: tot = C(n_pops - 1, 3) device totals or NULL; 4 <= n_pops <= 7 (the last population is the
// outgroup) and minind >= 1 (checked by the caller); out = one table of n_win rows per trio, in lexicographic trio order
int launch_dstat_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                      uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, pgt_dstat_total *tot,
                      void *tree, const LaunchEnv &e);

// pgt_fd_pops_kernels.hip: f_d / f_dM of the same trios; arguments, limits and tree size as launch_dstat_pops
int launch_fd_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                   uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_fd_row *out, pgt_fd_total *tot,
                   void *tree, const LaunchEnv &e);

// pgt_f3_pops_kernels.hip: f3 of ALL trios of the populations (no outgroup), each population of a trio as the target;
// tot = C(n_pops, 3) device totals or NULL; 3 <= n_pops <= 6 and minind >= 1 (checked by the caller); out = one table of n_win
// rows per trio, in lexicographic trio order; the tree has launch_dstat_pops' layout at n_pops + 1
int launch_f3_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                   uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f3_row *out, pgt_f3_total *tot,
                   void *tree, const LaunchEnv &e);

// pgt_f4_pops_kernels.hip: f4 of ALL quartets of the populations (no outgroup), each quartet in its three pairings;
// tot = C(n_pops, 4) device totals or NULL; 4 <= n_pops <= 6 and minind >= 1 (checked by the caller); out = one table of n_win
// rows per quartet, in lexicographic quartet order; a node is 3 C(n_pops, 4) doubles and C(n_pops, 4) u32
int launch_f4_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                   uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4_row *out, pgt_f4_total *tot,
                   void *tree, const LaunchEnv &e);

// pgt_f4ratio_pops_kernels.hip: the f4-ratio sums of ALL triples of the middle populations 1 .. n_pops - 2, between population 0
// (A) and the last one (the outgroup); tot = C(n_pops - 2, 3) device totals or NULL; 5 <= n_pops <= 7 and minind >= 1 (checked
// by the caller); out = one table of n_win rows per triple, in lexicographic order; a node is 3 T doubles and T u32
int launch_f4ratio_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                        uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out, pgt_f4ratio_total *tot,
                        void *tree, const LaunchEnv &e);

// pgt_pbs_pops_kernels.hip: the population branch statistic of ALL trios, every population of a trio as the focal one, in two
// passes of the walk (three numerators, then three denominators per trio) and a finishing kernel.  A pass writes scratch rows
// and scratch totals; the workspace holds the tree of one pass (pgt_f3_pops_reduce_dev's: 3 T doubles and T u32 per node,
// reused by the second pass), then the scratch rows of the two passes (T * n_win each), then their scratch totals (T each),
// every part padded to 256 bytes.
struct PbsPassRow {  // 40 bytes
    uint32_t start, end, mid, n;
    double s[3];  // the pass's sums of the pairs (i,j), (i,k), (j,k)
};
struct PbsPassTotal {  // 40 bytes
    double s[3];
    uint64_t neff, nskip;
};
struct PbsWork {
    uint32_t n_trios = 0;
    size_t tree_bytes = 0;       // the tree at offset 0
    size_t rows[2] = {0, 0};     // byte offsets of the passes' scratch rows ...
    size_t tot[2] = {0, 0};      // ... and scratch totals
    size_t bytes = 0;
};
// 3 <= n_pops <= 6 (checked by the caller)
inline PbsWork pbs_work(uint32_t n_pops, uint64_t n_sites, uint64_t n_win) {
    PbsWork w;
    auto pad = [](size_t b) { return ((b + 255) / 256) * 256; };
    w.n_trios = n_pops * (n_pops - 1) * (n_pops - 2) / 6;
    w.tree_bytes = pops_tree_view(tree_layout(PGT_STAT_FST, n_sites), (int)w.n_trios, 3, nullptr, 0).bytes;
    const size_t row_bytes = pad((size_t)w.n_trios * n_win * sizeof(PbsPassRow)), tot_bytes = pad((size_t)w.n_trios * sizeof(PbsPassTotal));
    w.rows[0] = pad(w.tree_bytes);
    w.rows[1] = w.rows[0] + row_bytes;
    w.tot[0] = w.rows[1] + row_bytes;
    w.tot[1] = w.tot[0] + tot_bytes;
    w.bytes = w.tot[1] + tot_bytes;
    return w;
}
// tot = C(n_pops, 3) device totals or NULL; 3 <= n_pops <= 6, minind >= 1, and n_win > 0 or tot (checked by the caller);
// out = one table of n_win rows per trio, in lexicographic trio order; work = pbs_work(..).bytes; the estimator names the
// per-site values of a pair (pgt_fst_site.h), as in launch_fst_pops
int launch_pbs_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                    uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot,
                    void *work, const LaunchEnv &e, FstPopsEstimator estimator);

// pgt_kernels.hip: pi per population, 1 <= n_pops <= 8 and minind >= 1 (checked by the caller); out = n_pops tables of
// n_win rows, tot = n_pops device totals or NULL; tree = n_pops trees of tree_layout(PGT_STAT_DXY, n).bytes each
int launch_pi_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops,
                   uint64_t n, int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot,
                   void *tree, const LaunchEnv &e);

// pgt_align_kernels.hip: the sites common to K position columns (pgt_sites_align) and the gather behind it.
// The workspace, every part 256-byte aligned: the plan (segments as u32 pairs, first tile per chromosome), the first output
// row per chromosome, per tile of 1024 pivot rows its count and first output row, and per file k >= 1 the row found for
// every pivot row.  A call handles at most kAlignMaxChr matched chromosomes (the plan's share of the workspace is fixed:
// pgt_align_workspace_bytes knows only the files and the pivot's rows).
constexpr int kAlignMaxFiles = 8;
constexpr uint32_t kAlignMaxChr = 4096;
struct AlignLayout {
    size_t seg, tile_first, chr_first, tile_count, tile_row;
    size_t prov[kAlignMaxFiles];
    uint64_t max_tiles;
    size_t bytes;
};
AlignLayout align_layout(uint32_t n_files, uint64_t n_rows_file0);
// synchronous; arguments checked by the caller (pgt_api.cpp); seg: n_chr * n_files entries, chromosome-major
int launch_sites_align(const uint32_t *const *pos, const uint64_t *n_rows, uint32_t n_files, const pgt_seg *seg, size_t n_chr,
                       uint32_t *const *idx, uint64_t cap, uint64_t *seg_count, uint64_t *n_common, void *work, void *stream,
                       std::string *err);
int launch_gather(void *dst, const void *src, const uint32_t *idx, uint64_t n, uint32_t elem_bytes, void *stream, std::string *err);

// pgt_windows.cpp: the site-window rules per chromosome run in closed form (see there); plain data, also read by
// the kernel that writes a window table on the device (pgt_kernels.hip: launch_windows_from_plan)
struct RunPlan {
    uint64_t out0 = 0;  // index of the run's first window in the table
    uint64_t K = 0;     // full windows [hi0 + k*S - W, hi0 + k*S), k < K
    uint64_t hi0 = 0;
    uint64_t tail_lo = 0, tail_hi = 0;  // one more window [tail_lo, tail_hi) at the end of the run ...
    uint32_t tail = 0, pad_ = 0;        // ... if tail != 0
};
// -> PGT_OK and the plan of (run_len, W, S) in site mode + the number of windows; argument errors as pgt_build_windows_sites
int plan_site_windows(const uint64_t *run_len, size_t n_runs, uint32_t W, uint32_t S, std::vector<RunPlan> &plan, uint64_t *count);
int launch_windows_from_plan(const RunPlan *d_plan, uint64_t n_runs, uint64_t n_win, uint32_t W, uint32_t S, pgt_win *d_out,
                             void *stream, std::string *err);

// pgt_kernels.hip: words[i] = splitmix64(seed + i) by plain global stores (pgt_rowbuf_fill: mapping self-test)
int launch_fill_pattern(uint64_t *words, uint64_t n_words, uint64_t seed, void *stream, std::string *err);

// pgt_ingest.hip: text -> device columns + chromosome runs (synchronous, default stream of `device`)
int ingest_text(int device, const char *text, size_t len, const uint8_t *tokens, int n_tokens, uint64_t front, pgt_ingest **out, std::string *err);
size_t ingest_column_bytes(const pgt_ingest *ing, int token);  // rows * element size of the token's column (0: no column)

int init_kernels(std::string *err);     // pgt_kernels.hip: one-time kernel attributes (called by pgt_open)
int init_af_kernels(std::string *err);  // pgt_af_kernels.hip
int init_dxy_pops_kernels(std::string *err);  // pgt_dxy_pops_kernels.hip
int init_fst_pops_kernels(std::string *err);  // pgt_fst_pops_kernels.hip
int init_dstat_pops_kernels(std::string *err);  // pgt_dstat_pops_kernels.hip
int init_fd_pops_kernels(std::string *err);     // pgt_fd_pops_kernels.hip
int init_f3_pops_kernels(std::string *err);     // pgt_f3_pops_kernels.hip
int init_pbs_pops_kernels(std::string *err);    // pgt_pbs_pops_kernels.hip
int init_f4_pops_kernels(std::string *err);     // pgt_f4_pops_kernels.hip
int init_f4ratio_pops_kernels(std::string *err);  // pgt_f4ratio_pops_kernels.hip

// thread-local message for the ctx-less entry points
void set_global_error(const std::string &msg);
const std::string &global_error();

}  // namespace pgt
