// pgt_dstat_jack_kernels.hip — the weighted (delete-m_j) block jackknife of Busing, Meijer & van der Leeden (1999) for a RATIO OF
// TWO BLOCK SUMS with block weights, fed here with the window rows of pgt_dstat_pops_reduce_dev: standard error and Z of
// Patterson's D for every trio and each of its three topologies.
//
// Spec (include/pgtwin.h, pgt_dstat_jackknife_dev).  rows[t * n_win + w] is trio t's row of window w; every window is a block,
// used iff its n > 0, with weight m_j = n.  Item u = 3 t + c takes (x, y) = (abba, baba) / (bbaa, baba) / (bbaa, abba) for
// c = 0 / 1 / 2.  Over the used blocks g = their number, n = Σ m_j, X = Σ x_j, Y = Σ y_j, and with
// ratio(a, b) = (a + b) != 0 ? (a - b) / (a + b) : 0:
//     theta    = ratio(X, Y)                         theta_-j = ratio(X - x_j, Y - y_j)               h_j = n / m_j
//     theta_J  = g theta - Σ_j (1 - m_j / n) theta_-j
//     tau_j    = theta + (h_j - 1) (theta - theta_-j)
//     sigma^2  = (1 / g) Σ_j (tau_j - theta_J)^2 / (h_j - 1)
// Every operation is one __d*_rn intrinsic (nothing is contracted); a block that is not used is selected away, never added.
//
// A second ESTIMATOR runs through the same phases (pgt_f3_jackknife_dev, over the rows of pgt_f3_pops_reduce_dev): a MEAN
// instead of a ratio of two sums — item u = 3 t + c takes x_j = sum c of the row (the target i / j / k of the trio), and with
// mean(a, b) = b != 0 ? a / b : 0:     theta = mean(X, n)     theta_-j = mean(X - x_j, n - m_j)     (n, m_j as f64)
// h_j, theta_J, tau_j and sigma^2 as above.  The estimator (struct D, struct Mean below: F3Mean, and F4Mean over the rows of
// pgt_f4_pops_reduce_dev) is a template parameter of the phases that look at an estimate; the totals, the plan, the chunking,
// readd(), the workspace layout and the order of every addition are common, and the row types of these three are 48 bytes with n and the three
// sums at the same offsets.  A third estimator, the signed RATIO of two of a row's sums (struct Ratio: the f4-ratio's admixture
// proportions, pgt_f4ratio_jackknife_dev), has SIX items per row where the others have three: the item count is a constant of
// the estimator (kItems) that sizes the per-lane arrays and the partials of phases 2 and 3.  A fourth, the population branch
// statistic (struct Pbs: PBS and PBSn1 of the three focal populations, pgt_pbs_jackknife_dev), reads rows of another type: 88
// bytes with SIX sums.  The number of sums and the loads of a row are constants of the estimator's ROWS (Rows48, RowsPbs:
// kSums sizes the totals and phase 1's partials), and Pbs states all its items of a set of sums at once (kJoint: three logs).
//
// Three dependent reductions over the rows and one closing kernel, all on the plan of jack_plan(n_win) (pgt_internal.h):
//   phase 1  jack_totals_kernel   per wave Σbbaa, Σabba, Σbaba, Σn, g of its chunks                 -> 5 words per wave (Pbs: six sums, 8)
//   phase 2  jack_drop_kernel     re-adds phase 1's partials of its trio (theta), then per topology
//                                 Σ (1 - m_j / n) theta_-j over its chunks                          -> 3 doubles per wave (Ratio, Pbs: 6)
//   phase 3  jack_var_kernel      re-adds phases 1 and 2 (theta_J), then per topology
//                                 Σ (tau_j - theta_J)^2 / (h_j - 1) over its chunks                 -> 3 doubles per wave (Ratio, Pbs: 6)
//   close    jack_close_kernel    one wave per item: re-adds all three, writes pgt_dstat_jack
// The grid is (ceil(n_partials / 4), n_trios) workgroups of 4 waves: blockIdx.y is the trio, wave p of it walks the chunks
// [p * chunks_per_wave, (p + 1) * chunks_per_wave) — 64 consecutive rows (48 bytes; Pbs: 88) each, one row per lane, all items
// from that one read.  A lane adds its rows in chunk order, the wave closes with the fixed butterfly of wave_sum, and partials
// are re-added by readd(): lane l adds partials l, l + 64, .. in turn, then the same butterfly.  No atomics; every order is a
// function of n_win alone, and a wave touches its own trio's rows and partials only: an item's bits do not depend on n_trios
// or on the other trios.  Phases 2 and 3 are not merged by expanding the square (that subtracts two large, nearly equal sums).
// With at most 1024 partials per item the re-adding is 16 loads per lane from L2: no finishing launch between the phases.
// Every partial a later phase reads was written by the phase before it in the same call (all n_partials waves of a trio
// store theirs, a wave without a used block stores zeros).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "pgt_device.h"
#include "pgt_internal.h"
#include "pgt_pops_common.h"

namespace pgt {
namespace {

using namespace dev;

struct JackArgs {
    const char *rows;          // n_trios x n_win rows of the estimator's type, trio-major
    uint64_t n_win;
    uint64_t chunks;           // jack_plan(n_win)
    uint64_t chunks_per_wave;
    uint32_t n_partials;
    uint32_t n_trios;
    uint64_t *totals;          // [trio][kSums + 2][n_partials]: the sums (Σbbaa, Σabba, Σbaba; Pbs: six) as f64 bits, Σn, g
    double *drop;              // [trio][Est::kItems][n_partials]: 3, or the 6 of Ratio
    double *var;               // [trio][Est::kItems][n_partials]
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m, kWave);
    return v;
}

__device__ __forceinline__ double ratio(double a, double b) {
    const double den = __dadd_rn(a, b);
    return den != 0.0 ? __ddiv_rn(__dsub_rn(a, b), den) : 0.0;
}

// (x, y) of topology c from a row's, or the totals', three sums {bbaa, abba, baba}
__device__ __forceinline__ double topo_x(int c, double bbaa, double abba) { return c == 0 ? abba : bbaa; }
__device__ __forceinline__ double topo_y(int c, double abba, double baba) { return c == 2 ? abba : baba; }

// ---- the rows: how many sums a row carries, and how a lane loads the weight n and the sums x[kSums] of its row -------------------
// the 48-byte rows (pgt_dstat_row and the types with n and the three sums at its offsets): three plain 16-byte vector loads;
// start / end / mid / d are not looked at
struct Rows48 {
    static constexpr int kSums = 3;
    static constexpr size_t kBytes = sizeof(pgt_dstat_row);
    static __device__ __forceinline__ void load(const char *r, uint32_t &m, double *x) {
        const uint4 head = *reinterpret_cast<const uint4 *>(r);           // start, end, mid, n
        const double2 v0 = *reinterpret_cast<const double2 *>(r + 16);    // d, bbaa
        const double2 v1 = *reinterpret_cast<const double2 *>(r + 32);    // abba, baba
        m = head.w;
        x[0] = v0.y;
        x[1] = v1.x;
        x[2] = v1.y;
    }
};
// pgt_pbs_row: 88 bytes, so a row at an odd index is 8-byte aligned only: n and the six sums by plain 4- and 8-byte loads per
// lane (no LDS stage and so no barrier: a padding wave returns at once; profiles/r20/pbs_jack.md).  The coordinates and the
// three pbs are not looked at.
struct RowsPbs {
    static constexpr int kSums = 6;
    static constexpr size_t kBytes = sizeof(pgt_pbs_row);
    static __device__ __forceinline__ void load(const char *r, uint32_t &m, double *x) {
        m = *reinterpret_cast<const uint32_t *>(r + offsetof(pgt_pbs_row, n));
        const double *sums = reinterpret_cast<const double *>(r + offsetof(pgt_pbs_row, num_ij));  // num_ij, num_ik, num_jk, den_ij, den_ik, den_jk
#pragma unroll
        for (int k = 0; k < kSums; ++k) x[k] = sums[k];
    }
};
static_assert(sizeof(pgt_pbs_row) == 88 && offsetof(pgt_pbs_row, n) == 12 && offsetof(pgt_pbs_row, num_ij) == 40 && offsetof(pgt_pbs_row, den_jk) == 80 &&
              sizeof(pgt_pbs_jack) == sizeof(pgt_f4_jack), "the row layout RowsPbs::load assumes; results in the layout of pgt_f4_jack");

// ---- the estimators: what theta is of the sums and a weight; everything else in this file is common to them ---------------------
// theta(c, s, n): item c's estimate from the sums s[kSums] and the weight n of the used blocks; theta_drop(c, s, n, x, m):
// the same with one block (its sums x, its weight m as f64) taken out.  An estimator whose items share their costly part
// (kJoint) states all(s, n, th) instead: every item of one set of sums.
struct D {  // Patterson's D of topology c: ratio(x, y) of two of the three sums (the head of this file)
    using Row = pgt_dstat_row;
    using Out = pgt_dstat_jack;
    using Rows = Rows48;
    static constexpr int kItems = kJackTopologies;
    static constexpr bool kDropFromSums = false, kJoint = false;
    static __device__ __forceinline__ double theta(int c, const double *s, double) { return ratio(topo_x(c, s[0], s[1]), topo_y(c, s[1], s[2])); }
    static __device__ __forceinline__ double theta_drop(int c, const double *s, double, const double *x /* bbaa, abba, baba */, double) {
        return ratio(__dsub_rn(topo_x(c, s[0], s[1]), topo_x(c, x[0], x[1])), __dsub_rn(topo_y(c, s[1], s[2]), topo_y(c, x[1], x[2])));
    }
    static __device__ __forceinline__ void set(Out &r, double th, double th_j, double se, double z) { r.d = th; r.d_jack = th_j; r.se = se; r.z = z; }
};
// f3 with target c of the trio (pgt_f3_jackknife_dev): a MEAN, x_j = sum c of the row, with mean(a, b) = b != 0 ? a / b : 0
//     theta = mean(X, n)                              theta_-j = mean(X - x_j, n - m_j)        (n, m_j as f64)
__device__ __forceinline__ double mean(double a, double b) { return b != 0.0 ? __ddiv_rn(a, b) : 0.0; }
// One body for the two row and result types that carry a mean (the rows of pgt_f3_pops_reduce_dev and of pgt_f4_pops_reduce_dev:
// n and the three sums at the same offsets; the results differ in the names of their first two fields alone).
__device__ __forceinline__ void set_estimates(pgt_f3_jack &r, double th, double th_j) { r.f3 = th; r.f3_jack = th_j; }
__device__ __forceinline__ void set_estimates(pgt_f4_jack &r, double th, double th_j) { r.f4 = th; r.f4_jack = th_j; }
template <class RowT, class OutT>
struct Mean {
    using Row = RowT;
    using Out = OutT;
    using Rows = Rows48;
    static constexpr int kItems = kJackTopologies;
    static constexpr bool kDropFromSums = false, kJoint = false;
    static __device__ __forceinline__ double pick(int c, double x0, double x1, double x2) { return c == 0 ? x0 : (c == 1 ? x1 : x2); }
    static __device__ __forceinline__ double theta(int c, const double *s, double n) { return mean(pick(c, s[0], s[1], s[2]), n); }
    static __device__ __forceinline__ double theta_drop(int c, const double *s, double n, const double *x, double m) {
        return mean(__dsub_rn(pick(c, s[0], s[1], s[2]), pick(c, x[0], x[1], x[2])), __dsub_rn(n, m));
    }
    static __device__ __forceinline__ void set(Out &r, double th, double th_j, double se, double z) { set_estimates(r, th, th_j); r.se = se; r.z = z; }
};
using F3Mean = Mean<pgt_f3_row, pgt_f3_jack>;  // item c: f3 with target c of the trio
using F4Mean = Mean<pgt_f4_row, pgt_f4_jack>;  // item c: f4 of pairing c of the quartet, (ij;kl) / (ik;jl) / (il;jk)
// The f4-ratio (pgt_f4ratio_jackknife_dev): the SIGNED RATIO OF TWO BLOCK SUMS, numerator and denominator losing a block together.
// A row's sums are S0, S1, S2 = Σ e d_ij, Σ e d_ik, Σ e d_jk of middle triple (i, j, k); item c is alpha(B, X, C) =
// f4(A,O; X,C) / f4(A,O; B,C), SIX per row:    c  (B,X,C)   N_c   D_c          c  (B,X,C)   N_c   D_c
//                                              0  (i,j,k)   +S2   +S1          3  (k,i,j)   +S0   -S2
//                                              1  (j,i,k)   +S1   +S2          4  (j,k,i)   +S1   +S0
//                                              2  (i,k,j)   -S2   +S0          5  (k,j,i)   +S0   +S1
//     theta = q(N_c, D_c)                             theta_-j = q(N_c - n_cj, D_c - d_cj)     q = mean above; the weight decides "used" alone
// N_c and D_c are single sums under a sign, and negation is exact: taking block j out of the three sums first and reading the
// item off the rest is the same value, so this estimator states theta alone (kDropFromSums; theta_without below).
struct Ratio {
    using Row = pgt_f4ratio_row;
    using Out = pgt_f4ratio_jack;
    using Rows = Rows48;
    static constexpr int kItems = kJackRatioItems;
    static constexpr bool kDropFromSums = true, kJoint = false;
    static __device__ __forceinline__ double num(int c, double s0, double s1, double s2) {
        return c == 0 ? s2 : (c == 1 || c == 4 ? s1 : (c == 2 ? -s2 : s0));
    }
    static __device__ __forceinline__ double den(int c, double s0, double s1, double s2) {
        return c == 0 || c == 5 ? s1 : (c == 1 ? s2 : (c == 3 ? -s2 : s0));
    }
    static __device__ __forceinline__ double theta(int c, const double *s, double) { return mean(num(c, s[0], s[1], s[2]), den(c, s[0], s[1], s[2])); }
    static __device__ __forceinline__ void set(Out &r, double th, double th_j, double se, double z) { r.alpha = th; r.alpha_jack = th_j; r.se = se; r.z = z; }
};
// The population branch statistic (pgt_pbs_jackknife_dev) over the rows of pgt_pbs_pops_reduce_dev: a NON-LINEAR function of SIX
// block sums S = (num_ij, num_ik, num_jk, den_ij, den_ik, den_jk).  E(S): the row arithmetic of pgt_pbs_row (pbs_of,
// pgt_pops_common.h: fst_xy = den_xy != 0 ? num_xy / den_xy : 0, T_xy = -log(1 - fst_xy), three logs) gives pbs_i, pbs_j, pbs_k,
// items 0 ... 2; items 3 ... 5 are PBSn1 (Malaspinas et al. 2016) of the same focal populations,
//     s = (pbs_i + pbs_j) + pbs_k        pbsn1_x = pbs_x / (1.0 + s)
// Nothing is clamped.  theta = E(Σ S), theta_-j = E(Σ S - s_j), each of the six sums losing the block with one rounding
// (kDropFromSums); E is evaluated once per block for all six items (kJoint).  The weight decides "used" alone.
struct Pbs {
    using Row = pgt_pbs_row;
    using Out = pgt_pbs_jack;
    using Rows = RowsPbs;
    static constexpr int kItems = kJackPbsItems;
    static constexpr bool kDropFromSums = true, kJoint = true;
    static __device__ __forceinline__ void all(const double *s, double, double *th) {
        pbs_of(s, s + 3, th[0], th[1], th[2]);
        const double one_s = __dadd_rn(1.0, __dadd_rn(__dadd_rn(th[0], th[1]), th[2]));
#pragma unroll
        for (int k = 0; k < 3; ++k) th[3 + k] = __ddiv_rn(th[k], one_s);
    }
    static __device__ __forceinline__ void set(Out &r, double th, double th_j, double se, double z) { r.stat = th; r.stat_jack = th_j; r.se = se; r.z = z; }
};

// Σ of n_partials doubles in index order per lane (l, l + 64, ..), then the butterfly: the same bits in every lane of every wave
__device__ __forceinline__ double readd(const double *p, uint32_t n_partials, int lane) {
    double a = 0.0;
    for (uint32_t i = (uint32_t)lane; i < n_partials; i += kWave) a = __dadd_rn(a, p[i]);
    return dev::wave_sum(a);
}
__device__ __forceinline__ uint64_t readd(const uint64_t *p, uint32_t n_partials, int lane) {
    uint64_t a = 0;
    for (uint32_t i = (uint32_t)lane; i < n_partials; i += kWave) a += p[i];
    return wave_sum(a);
}

template <int NS>
struct Totals {
    double s[NS];  // the sums over the used blocks (Σbbaa, Σabba, Σbaba; the six of a pgt_pbs_row)
    double n;      // Σ m_j as f64 (exact below 2^53 sites)
    uint64_t n_sites;
    uint32_t g;
};
template <int NS>
__device__ __forceinline__ Totals<NS> read_totals(const JackArgs &a, uint32_t trio, int lane) {
    const uint64_t *base = a.totals + (uint64_t)trio * jack_total_words(NS) * a.n_partials;
    Totals<NS> t;
#pragma unroll
    for (int k = 0; k < NS; ++k) t.s[k] = readd(reinterpret_cast<const double *>(base + (uint64_t)k * a.n_partials), a.n_partials, lane);
    t.n_sites = readd(base + (uint64_t)NS * a.n_partials, a.n_partials, lane);
    t.g = (uint32_t)readd(base + (uint64_t)(NS + 1) * a.n_partials, a.n_partials, lane);
    t.n = (double)t.n_sites;
    return t;
}

// the wave's rows, one per lane and chunk, in chunk order: f(used, m_j, x[kSums]); a lane beyond the table sees an unused block
// of zeros.  Rows::load reads a row.
template <class Rows, class F>
__device__ __forceinline__ void for_rows(const JackArgs &a, uint32_t trio, uint32_t p, int lane, F f) {
    const char *rows_t = a.rows + (uint64_t)trio * a.n_win * Rows::kBytes;
    const uint64_t c0 = (uint64_t)p * a.chunks_per_wave;
    const uint64_t c1 = c0 + a.chunks_per_wave < a.chunks ? c0 + a.chunks_per_wave : a.chunks;
#pragma unroll 2
    for (uint64_t c = c0; c < c1; ++c) {
        const uint64_t j = c * kJackChunk + (uint64_t)lane;
        uint32_t m = 0;
        double x[Rows::kSums];
#pragma unroll
        for (int k = 0; k < Rows::kSums; ++k) x[k] = 0.0;
        if (j < a.n_win) Rows::load(rows_t + j * Rows::kBytes, m, x);
        f(m > 0, m, x);
    }
}
static_assert(sizeof(pgt_dstat_row) == 48 && sizeof(pgt_dstat_jack) == 48, "the row layout Rows48::load assumes");
// the rows of pgt_f3_pops_reduce_dev go through the same loads: n and the three sums sit where pgt_dstat_row has them
static_assert(sizeof(pgt_f3_row) == sizeof(pgt_dstat_row) && sizeof(pgt_f3_jack) == sizeof(pgt_dstat_jack), "one row loader, one result layout");
static_assert(offsetof(pgt_f3_row, n) == offsetof(pgt_dstat_row, n) && offsetof(pgt_f3_row, f3_i) == offsetof(pgt_dstat_row, bbaa) &&
              offsetof(pgt_f3_row, f3_j) == offsetof(pgt_dstat_row, abba) && offsetof(pgt_f3_row, f3_k) == offsetof(pgt_dstat_row, baba),
              "the three sums of an f3 row at the offsets of bbaa / abba / baba");
// ... and so do the rows of pgt_f4_pops_reduce_dev
static_assert(sizeof(pgt_f4_row) == sizeof(pgt_f3_row) && sizeof(pgt_f4_jack) == sizeof(pgt_f3_jack), "one row loader, one result layout");
static_assert(offsetof(pgt_f4_row, n) == offsetof(pgt_f3_row, n) && offsetof(pgt_f4_row, f4_ij_kl) == offsetof(pgt_f3_row, f3_i) &&
              offsetof(pgt_f4_row, f4_ik_jl) == offsetof(pgt_f3_row, f3_j) && offsetof(pgt_f4_row, f4_il_jk) == offsetof(pgt_f3_row, f3_k),
              "the three sums of an f4 row at the offsets of f3_i / f3_j / f3_k");
static_assert(offsetof(pgt_f4_jack, f4) == offsetof(pgt_f3_jack, f3) && offsetof(pgt_f4_jack, f4_jack) == offsetof(pgt_f3_jack, f3_jack) &&
              offsetof(pgt_f4_jack, se) == offsetof(pgt_f3_jack, se) && offsetof(pgt_f4_jack, n_blocks) == offsetof(pgt_f3_jack, n_blocks),
              "pgt_f4_jack in pgt_f3_jack's layout");
// ... and the rows of pgt_f4ratio_pops_reduce_dev; its results have the layout of pgt_f4_jack
static_assert(sizeof(pgt_f4ratio_row) == sizeof(pgt_f4_row) && sizeof(pgt_f4ratio_jack) == sizeof(pgt_f4_jack), "one row loader, one result layout");
static_assert(offsetof(pgt_f4ratio_row, n) == offsetof(pgt_f4_row, n) && offsetof(pgt_f4ratio_row, g_ij) == offsetof(pgt_f4_row, f4_ij_kl) &&
              offsetof(pgt_f4ratio_row, g_ik) == offsetof(pgt_f4_row, f4_ik_jl) && offsetof(pgt_f4ratio_row, g_jk) == offsetof(pgt_f4_row, f4_il_jk),
              "the three sums of an f4-ratio row at the offsets of f4_ij_kl / f4_ik_jl / f4_il_jk");
static_assert(offsetof(pgt_f4ratio_jack, alpha) == offsetof(pgt_f4_jack, f4) && offsetof(pgt_f4ratio_jack, alpha_jack) == offsetof(pgt_f4_jack, f4_jack) &&
              offsetof(pgt_f4ratio_jack, se) == offsetof(pgt_f4_jack, se) && offsetof(pgt_f4ratio_jack, n_blocks) == offsetof(pgt_f4_jack, n_blocks),
              "pgt_f4ratio_jack in pgt_f4_jack's layout");

// wave p of trio blockIdx.y; -1: a wave that pads the last workgroup (it returns: no barrier is ever used)
__device__ __forceinline__ int64_t my_partial(const JackArgs &a) {
    const uint32_t p = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return p < a.n_partials ? (int64_t)p : -1;
}

template <class Est>
using TotalsOf = Totals<Est::Rows::kSums>;

// every item's theta of one set of sums: the estimator's joint statement (kJoint), or item after item
template <class Est>
__device__ __forceinline__ void thetas(const double *s, double n, double *th) {
    if constexpr (Est::kJoint) {
        Est::all(s, n, th);
    } else {
#pragma unroll
        for (int c = 0; c < Est::kItems; ++c) th[c] = Est::theta(c, s, n);
    }
}
// theta of item c alone (c need not be a constant: the items are selected, never indexed)
template <class Est>
__device__ __forceinline__ double theta_of(int c, const TotalsOf<Est> &t) {
    if constexpr (Est::kJoint) {
        double th[Est::kItems];
        Est::all(t.s, t.n, th);
        double v = th[0];
#pragma unroll
        for (int k = 1; k < Est::kItems; ++k) v = c == k ? th[k] : v;
        return v;
    } else {
        return Est::theta(c, t.s, t.n);
    }
}
// theta_-j of every item: the estimator's own statement of it, or (kDropFromSums) its thetas of the sums and the weight less block j's
template <class Est>
__device__ __forceinline__ void thetas_without(const TotalsOf<Est> &t, const double *x, double m, double *th) {
    if constexpr (Est::kDropFromSums) {
        constexpr int NS = Est::Rows::kSums;
        double rest[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) rest[k] = __dsub_rn(t.s[k], x[k]);
        thetas<Est>(rest, __dsub_rn(t.n, m), th);
    } else {
#pragma unroll
        for (int c = 0; c < Est::kItems; ++c) th[c] = Est::theta_drop(c, t.s, t.n, x, m);
    }
}

// ---- phase 1: the totals -----------------------------------------------------------------------------------------------------
// a function of the rows alone (their sum count and loads): one instance for the 48-byte rows, one for pgt_pbs_row
template <class Rows>
__global__ __launch_bounds__(256) void jack_totals_kernel(JackArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t trio = blockIdx.y;
    const int64_t pp = my_partial(a);
    if (pp < 0) return;
    const uint32_t p = (uint32_t)pp;
    constexpr int NS = Rows::kSums;
    double s[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    uint64_t n = 0, g = 0;
    for_rows<Rows>(a, trio, p, lane, [&](bool used, uint32_t m, const double *x) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = __dadd_rn(s[k], used ? x[k] : 0.0);
        n += m;  // an unused block has m == 0
        g += used ? 1u : 0u;
    });
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = dev::wave_sum(s[k]);
    n = wave_sum(n);
    g = wave_sum(g);
    if (lane == 0) {
        uint64_t *base = a.totals + (uint64_t)trio * jack_total_words(NS) * a.n_partials + p;
#pragma unroll
        for (int k = 0; k < NS; ++k) reinterpret_cast<double *>(base)[(uint64_t)k * a.n_partials] = s[k];
        base[(uint64_t)NS * a.n_partials] = n;
        base[(uint64_t)(NS + 1) * a.n_partials] = g;
    }
}

// ---- phase 2: Σ (1 - m_j / n) theta_-j ---------------------------------------------------------------------------------------
template <class Est>
__global__ __launch_bounds__(256) void jack_drop_kernel(JackArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t trio = blockIdx.y;
    const int64_t pp = my_partial(a);
    if (pp < 0) return;
    const uint32_t p = (uint32_t)pp;
    const TotalsOf<Est> t = read_totals<Est::Rows::kSums>(a, trio, lane);
    constexpr int kItems = Est::kItems;
    double acc[kItems];
#pragma unroll
    for (int c = 0; c < kItems; ++c) acc[c] = 0.0;
    for_rows<typename Est::Rows>(a, trio, p, lane, [&](bool used, uint32_t m, const double *x) {
        const double w = __dsub_rn(1.0, __ddiv_rn((double)m, t.n));
        double th[kItems];
        thetas_without<Est>(t, x, (double)m, th);
#pragma unroll
        for (int c = 0; c < kItems; ++c) acc[c] = __dadd_rn(acc[c], used ? __dmul_rn(w, th[c]) : 0.0);
    });
#pragma unroll
    for (int c = 0; c < kItems; ++c) {
        const double v = dev::wave_sum(acc[c]);
        if (lane == 0) a.drop[((uint64_t)trio * kItems + c) * a.n_partials + p] = v;
    }
}

// theta_J of item c from its theta and the re-added partials of phase 2 (the same bits wherever it is called)
template <class Est>
__device__ __forceinline__ double jack_estimate(const JackArgs &a, const TotalsOf<Est> &t, uint32_t trio, int c, int lane, double theta) {
    const double drop = readd(a.drop + ((uint64_t)trio * Est::kItems + c) * a.n_partials, a.n_partials, lane);
    return __dsub_rn(__dmul_rn((double)t.g, theta), drop);
}

// ---- phase 3: Σ (tau_j - theta_J)^2 / (h_j - 1) -----------------------------------------------------------------------------
template <class Est>
__global__ __launch_bounds__(256) void jack_var_kernel(JackArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t trio = blockIdx.y;
    const int64_t pp = my_partial(a);
    if (pp < 0) return;
    const uint32_t p = (uint32_t)pp;
    const TotalsOf<Est> t = read_totals<Est::Rows::kSums>(a, trio, lane);
    constexpr int kItems = Est::kItems;
    double theta[kItems], theta_j[kItems], acc[kItems];
    thetas<Est>(t.s, t.n, theta);  // every item of the totals from ONE evaluation of the estimator
#pragma unroll
    for (int c = 0; c < kItems; ++c) {
        theta_j[c] = jack_estimate<Est>(a, t, trio, c, lane, theta[c]);
        acc[c] = 0.0;
    }
    for_rows<typename Est::Rows>(a, trio, p, lane, [&](bool used, uint32_t m, const double *x) {
        const double hm1 = __dsub_rn(__ddiv_rn(t.n, (double)m), 1.0);  // an unused block: inf, selected away below
        double th[kItems];
        thetas_without<Est>(t, x, (double)m, th);
#pragma unroll
        for (int c = 0; c < kItems; ++c) {
            const double tau = __dadd_rn(theta[c], __dmul_rn(hm1, __dsub_rn(theta[c], th[c])));
            const double dv = __dsub_rn(tau, theta_j[c]);
            acc[c] = __dadd_rn(acc[c], used ? __ddiv_rn(__dmul_rn(dv, dv), hm1) : 0.0);
        }
    });
#pragma unroll
    for (int c = 0; c < kItems; ++c) {
        const double v = dev::wave_sum(acc[c]);
        if (lane == 0) a.var[((uint64_t)trio * kItems + c) * a.n_partials + p] = v;
    }
}

// ---- close: one wave per item ------------------------------------------------------------------------------------------------
template <class Est>
__global__ __launch_bounds__(256) void jack_close_kernel(JackArgs a, typename Est::Out *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t u = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (u >= a.n_trios * Est::kItems) return;
    const uint32_t trio = u / Est::kItems;
    const int c = (int)(u % Est::kItems);
    const TotalsOf<Est> t = read_totals<Est::Rows::kSums>(a, trio, lane);  // without a partial (n_win == 0): zeros
    const double theta = theta_of<Est>(c, t);
    const double theta_j = jack_estimate<Est>(a, t, trio, c, lane, theta);
    const double vs = readd(a.var + ((uint64_t)trio * Est::kItems + c) * a.n_partials, a.n_partials, lane);
    typename Est::Out r;
    r.n_sites = t.n_sites;
    r.n_blocks = t.g;
    r.pad_ = 0;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (t.g >= 2) {
        const double se = __dsqrt_rn(__ddiv_rn(vs, (double)t.g));
        Est::set(r, theta, theta_j, se, se > 0.0 ? __ddiv_rn(theta_j, se) : nan);
    } else {
        Est::set(r, theta, theta, nan, nan);
    }
    if (lane == 0) out[u] = r;
}

template <class Est>
int launch_jackknife(const typename Est::Row *rows, uint64_t n_win, uint32_t n_trios, typename Est::Out *out, void *work,
                     void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const JackPlan plan = jack_plan(n_win);
    const JackWork w = jack_work(n_trios, n_win, Est::kItems, Est::Rows::kSums);
    JackArgs a{};
    a.rows = reinterpret_cast<const char *>(rows);
    a.n_win = n_win;
    a.chunks = plan.chunks;
    a.chunks_per_wave = plan.chunks_per_wave;
    a.n_partials = plan.n_partials;
    a.n_trios = n_trios;
    a.totals = reinterpret_cast<uint64_t *>(static_cast<char *>(work) + w.totals);
    a.drop = reinterpret_cast<double *>(static_cast<char *>(work) + w.drop);
    a.var = reinterpret_cast<double *>(static_cast<char *>(work) + w.var);
    if (int rc = record_event(ev_query0, s, err)) return rc;
    if (plan.n_partials > 0) {
        const dim3 grid((plan.n_partials + 3) / 4, n_trios);
        hipLaunchKernelGGL(jack_totals_kernel<typename Est::Rows>, grid, dim3(256), 0, s, a);
        if (int rc = hip_fail(hipGetLastError(), "jack_totals_kernel", err)) return rc;
        hipLaunchKernelGGL(jack_drop_kernel<Est>, grid, dim3(256), 0, s, a);
        if (int rc = hip_fail(hipGetLastError(), "jack_drop_kernel", err)) return rc;
        hipLaunchKernelGGL(jack_var_kernel<Est>, grid, dim3(256), 0, s, a);
        if (int rc = hip_fail(hipGetLastError(), "jack_var_kernel", err)) return rc;
    }
    hipLaunchKernelGGL(jack_close_kernel<Est>, dim3((n_trios * Est::kItems + 3) / 4), dim3(256), 0, s, a, out);
    if (int rc = hip_fail(hipGetLastError(), "jack_close_kernel", err)) return rc;
    return record_event(ev_query1, s, err);
}

}  // namespace

int launch_dstat_jackknife(const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios, pgt_dstat_jack *out, void *work,
                           void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    return launch_jackknife<D>(rows, n_win, n_trios, out, work, stream, ev_query0, ev_query1, err);
}

// the rows of pgt_f3_pops_reduce_dev: item u = 3 t + c is f3 with population c (i / j / k) of trio t as the target
int launch_f3_jackknife(const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios, pgt_f3_jack *out, void *work,
                        void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    return launch_jackknife<F3Mean>(rows, n_win, n_trios, out, work, stream, ev_query0, ev_query1, err);
}

// the rows of pgt_f4_pops_reduce_dev: item u = 3 q + c is f4 of pairing c, (ij;kl) / (ik;jl) / (il;jk), of quartet q
int launch_f4_jackknife(const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets, pgt_f4_jack *out, void *work,
                        void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    return launch_jackknife<F4Mean>(rows, n_win, n_quartets, out, work, stream, ev_query0, ev_query1, err);
}

// the rows of pgt_f4ratio_pops_reduce_dev: item u = 6 t + c is admixture proportion c of middle triple t (Ratio)
int launch_f4ratio_jackknife(const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples, pgt_f4ratio_jack *out, void *work,
                             void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    return launch_jackknife<Ratio>(rows, n_win, n_triples, out, work, stream, ev_query0, ev_query1, err);
}

// the rows of pgt_pbs_pops_reduce_dev (either FST estimator): item u = 6 t + c is PBS (c < 3) or PBSn1 (c >= 3) of trio t with
// population c % 3 (i / j / k) as the focal one (Pbs)
int launch_pbs_jackknife(const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios, pgt_pbs_jack *out, void *work,
                         void *stream, void *ev_query0, void *ev_query1, std::string *err) {
    return launch_jackknife<Pbs>(rows, n_win, n_trios, out, work, stream, ev_query0, ev_query1, err);
}

}  // namespace pgt
