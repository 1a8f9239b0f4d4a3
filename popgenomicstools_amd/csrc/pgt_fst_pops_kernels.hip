// pgt_fst_pops_kernels.hip — fstWindow's window statistic Σa / Σ(a+b) for ALL pairs i < j of up to 8 populations in ONE pass
// over the populations' own MAF columns (allele frequency f64 + individual count i32: 12 B/site/population), with the
// PER-SITE sample sizes a MAF file carries and dxyWindow's -minind predicate.
//
// Spec, per pair (i, j) and site s: the site counts iff nInd_i >= minind && nInd_j >= minind (dxyWindow.cpp:381, as
// pgt_dxy_pops_kernels.hip applies it; minind >= 1), and then contributes the two columns WCFst() returns
// (betaAFOutlier.R:405-417) evaluated with n1 = nInd_i, n2 = nInd_j (the site's diploid sample sizes), f1, f2 the frequencies:
//     npool = n1+n2;  alpha_k = 2 f_k (1-f_k);  b = (n1 alpha1 + n2 alpha2)/(npool-1)
//     a = (4 n1 (f1-fpool)^2 + 4 n2 (f2-fpool)^2 - b)/(4 n1 n2/npool) = (f1-f2)^2 - b npool/(4 n1 n2)
// (the identity of pgt_af_kernels.hip:12-15, which holds per site).  A window's row is Σa, Σ(a+b) and the number of counted
// sites; fst = Σa / Σ(a+b) (fstWindow.cpp:85).  The factorisation of pgt_af_kernels.hip (A_k, D_ij) rests on constant sample
// sizes and does not hold here: every pair keeps its own {Σa, Σ(a+b), neff}.
//
// The divisions: both divisors depend on (n1, n2) alone.  With q = 1/((npool-1) 4 n1 n2) — ONE reciprocal per pair and site,
// v_rcp_f64 refined by two Newton steps (relative error of q about 2^-52; the hardware estimate carries about 2^-23) —
//     b = (n1 alpha1 + n2 alpha2) q (4 n1 n2),      b npool/(4 n1 n2) = (n1 alpha1 + n2 alpha2) q npool.
// The per-population terms (n_k as a double, 4 n_k, n_k alpha_k) are computed once per site.  A site that is not counted may
// have n1 n2 = 0 (q infinite, a NaN): its values are never added (a select, not a product with 0).
//
// A second estimator, Hudson's ratio of averages (struct Hudson below; pgt_fst_hudson_pops_reduce_dev), runs through the same
// kernels: the estimator is a template parameter that names the per-site function, and nothing else knows about it.
//
// Tree, build walk, reduce-scatter, LDS-staged node block, per-wave partials and the one-wave-per-window query: those of
// pgt_dxy_pops_kernels.hip, with two sums per pair.  The counts are needed as VALUES here, not only for the predicate: they
// are read by 16-byte loads in the four-sites-per-lane layout (lane L: sites 4L .. 4L+3 of a pair of 128-site pieces) and the
// lane that owns sites 2l, 2l+1 of piece h in the frequency layout fetches them from lane 32h + (l >> 1) (four ds_bpermute
// per population and piece).  Per population "at least minind individuals" is a lane mask, a pair's predicate the AND of
// two of them, its neff the popcount of that AND.
//
// Rows of a pair are functions of the pair's own four columns and the window alone: every pair's arithmetic reads only its
// two populations' registers, and the order of all additions is fixed by the site index and the window.
// pgt_set_window_step is ignored by this entry point: every table is answered by the one-wave-per-window query.
#include <hip/hip_runtime.h>

#include "pgt_device.h"
#include "pgt_internal.h"
#include "pgt_pops_common.h"

namespace pgt {
namespace {

using namespace dev;

constexpr int kPieces = kPopsLeafPieces;   // 128-site pieces per level-1 node
constexpr int kLeaf = kPieces * kLeafF64;     // sites per level-1 node
constexpr int kRadix1 = kRadix / kPieces;     // level-1 nodes per level-2 node
static_assert(kPieces == 4, "the build walks a leaf as two pairs of pieces");

template <int NP>
struct Shape {
    static constexpr int kPairs = pair_count(NP);  // lexicographic (i < j): (0,1),(0,2),..,(0,NP-1),(1,2),..
    static constexpr int kSums = 2 * kPairs;       // Σa of every pair, then Σ(a+b) of every pair
};

struct PopCols {
    const double *f[kPopsMaxPops];
    const int32_t *c[kPopsMaxPops];
};

// 1/d for d >= 1 (finite): the hardware estimate and two Newton steps
__device__ __forceinline__ double recip(double d) {
    double x = __builtin_amdgcn_rcp(d);
    x = fma(x, fma(-d, x, 1.0), x);
    x = fma(x, fma(-d, x, 1.0), x);
    return x;
}

// ---- per-site contribution ---------------------------------------------------------------------------------------------
// One site of this lane into the lane's 2 P running sums and the wave's P counters.  f[k], c[k]: population k's frequency and
// individual count at the site (a site outside the range carries a count of 0: never counted, minind >= 1).
// MUST be called by all 64 lanes together (the counters are popcounts of ballots).
// The estimator is a compile-time tag with a static per-site function: the walk, the stage, the tree and the query below are
// written once and know only that a pair keeps two sums (acc[v], acc[P + v]) and a count (cnt[v]).
struct WeirCockerham {  // the spec at the top of this file: acc[v] += a, acc[P + v] += a + b
    template <int NP>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *f, const int *c, int minind) {
        constexpr int P = Shape<NP>::kPairs;
        double nd[NP], n4[NP], na[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            nd[k] = (double)c[k];
            ok[k] = c[k] >= minind;
            n4[k] = 4.0 * nd[k];
            na[k] = nd[k] * ((2.0 * f[k]) * (1.0 - f[k]));  // n_k alpha_k, betaAFOutlier.R:408-410
        }
        int v = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool counted = ok[i] && ok[j];
                const double npool = nd[i] + nd[j];
                const double p4 = n4[i] * nd[j];                // 4 n1 n2
                const double q = recip((npool - 1.0) * p4);
                const double t = (na[i] + na[j]) * q;
                const double b = t * p4;
                const double d = f[i] - f[j];
                const double a = d * d - t * npool;
                const double ab = a + b;
                acc[v] = acc[v] + (counted ? a : 0.0);
                acc[P + v] = acc[P + v] + (counted ? ab : 0.0);
                cnt[v] += (uint32_t)__popcll(__ballot(counted));
                ++v;
            }
    }
};

// Hudson's estimator as a ratio of averages (Hudson, Slatkin & Maddison 1992; Bhatia et al. 2013, eq. 10), the definition of
// pgt_fst_hudson_pops_reduce_dev in include/pgtwin.h: acc[v] += (p1 - p2)^2 - h_1 - h_2 with h_k = p_k (1 - p_k) / (2 n_k - 1),
// acc[P + v] += p1 (1 - p2) + p2 (1 - p1) — dxy_site_pred's roundings (pgt_kernels.hip), so a pair's denominator IS its dxy.
// Every operation is rounded on its own.  The only division is per population and site (pi_site's divisor 2 n - 1: odd, never
// 0), not per pair; an uncounted site (n_k <= 0: a negative divisor; any frequency) is selected away, never multiplied.
struct Hudson {
    template <int NP>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *f, const int *c, int minind) {
        constexpr int P = Shape<NP>::kPairs;
        double om[NP], h[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            ok[k] = c[k] >= minind;
            om[k] = __dsub_rn(1.0, f[k]);
            const double m = __dsub_rn(__dmul_rn(2.0, (double)c[k]), 1.0);  // haploid sample size minus one
            h[k] = __ddiv_rn(__dmul_rn(f[k], om[k]), m);
        }
        int v = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool counted = ok[i] && ok[j];
                const double d = __dsub_rn(f[i], f[j]);
                const double num = __dsub_rn(__dsub_rn(__dmul_rn(d, d), h[i]), h[j]);
                const double den = __dadd_rn(__dmul_rn(f[i], om[j]), __dmul_rn(f[j], om[i]));
                acc[v] = acc[v] + (counted ? num : 0.0);
                acc[P + v] = acc[P + v] + (counted ? den : 0.0);
                cnt[v] += (uint32_t)__popcll(__ballot(counted));
                ++v;
            }
    }
};

template <int NP, class Est>
__device__ __forceinline__ void fst_pops_site(double *acc, uint32_t *cnt, const double *f, const int *c, int minind) {
    Est::template site<NP>(acc, cnt, f, c, minind);
}

// A pair of 128-site pieces in registers: the counts of the pair's 256 sites (lane L: sites 4L .. 4L+3 of the pair) and
// the frequencies of its two pieces (lane l: sites 2l, 2l+1 of piece h).
template <int NP>
struct PieceSet {
    int4 k[NP];
    double2 f[2][NP];
};
// The lane's four sites of a pair of pieces, in site order, into the running sums.
template <int NP, class Est>
__device__ __forceinline__ void fst_pops_accumulate(double *acc, uint32_t *cnt, const PieceSet<NP> &s, int minind, int lane) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // this lane's sites 2l, 2l+1 of piece h = pair sites 128h + 2l + q: count lane 32h + (l >> 1), component 2(l & 1) + q
        const int src = 32 * h + (lane >> 1);
        const bool odd = (lane & 1) != 0;
        double px[NP], py[NP];
        int cx[NP], cy[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int x = __shfl(s.k[k].x, src, kWave), y = __shfl(s.k[k].y, src, kWave);
            const int z = __shfl(s.k[k].z, src, kWave), w = __shfl(s.k[k].w, src, kWave);
            cx[k] = odd ? z : x;
            cy[k] = odd ? w : y;
            px[k] = s.f[h][k].x;
            py[k] = s.f[h][k].y;
        }
        fst_pops_site<NP, Est>(acc, cnt, px, cx, minind);
        fst_pops_site<NP, Est>(acc, cnt, py, cy, minind);
    }
}

template <int NP>
__device__ __forceinline__ double *sum_node(const FstPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<double *>(tv.base + tv.sum_off[slot]) + i * Shape<NP>::kSums;
}
template <int NP>
__device__ __forceinline__ uint32_t *cnt_node(const FstPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[slot]) + i * Shape<NP>::kPairs;
}

// ---- BUILD: one wave per level-2 tile (64 pieces of 128 sites = 16 leaf nodes of 512 sites) -----------------------------
// The walk of dxy_pops_build_body: a PAIR of pieces is the unit (a 16-byte count load spans two pieces), two register sets
// swap roles, a full tile is walked from a piece of the wave's own, the tile's level-1 nodes are staged in LDS and leave as
// contiguous blocks of nt stores.  A leaf's sums do not depend on the wave or on where its walk started: a lane adds its 8
// sites of the leaf in site order, the reduce-scatter is a fixed tree, and the level-2 node adds the 16 leaf nodes in leaf order.
template <int NP, class Est>
__device__ __forceinline__ void fst_pops_build_body(const PopCols &cols, int minind, uint64_t n, uint64_t n_l2, const FstPopsTree &tv) {
    constexpr int P = Shape<NP>::kPairs;
    constexpr int V = Shape<NP>::kSums;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int my = rs_my_index<V>(lane);
    const uint32_t lane_bytes = (uint32_t)lane * 16u;
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    // the wave's LDS stage: 16 nodes x 2 P doubles, then 16 nodes x P u32 (private to the wave: no barrier)
    extern __shared__ __attribute__((aligned(16))) char fst_pops_stage[];
    char *stage = fst_pops_stage + (size_t)(threadIdx.x >> 6) * (kRadix1 * P * 20);
    double *stage_s = reinterpret_cast<double *>(stage);
    uint32_t *stage_c = reinterpret_cast<uint32_t *>(stage + kRadix1 * V * 8);

    double tot_s = 0.0;   // lane `my`: Σ of the level-2 nodes this wave wrote, in tile order (the genome-wide line's partial)
    uint32_t tot_c = 0;   // lane p < P: their neff

    for (uint64_t t = wave0; t < n_l2; t += n_waves) {
        const uint64_t base = t * kTile2;
        const bool full = base + kTile2 <= n;
        // a multiple of the leaf's pieces below 64 (see tile_rotation in pgt_kernels.hip); the partial last tile is walked from its start
        const int rot = full ? (int)(((wave0 * 0x9E3779B1ull) >> 13) & (uint64_t)(kRadix - kPieces)) : 0;
        double acc[V];
        uint32_t cnt[P];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < P; ++v) cnt[v] = 0u;
        auto finish_leaf = [&](int node) {  // the leaf's 2 P sums and P counts into the stage; the running sums start again
            rs_steps<V, 0>(acc, lane);
            if (my >= 0) stage_s[node * V + my] = acc[0];
            uint32_t cv = 0;
#pragma unroll
            for (int v = 0; v < P; ++v) cv = lane == v ? cnt[v] : cv;
            if (lane < P) stage_c[node * P + lane] = cv;
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
            for (int v = 0; v < P; ++v) cnt[v] = 0u;
        };
        if (full) {
            auto load_full = [&](PieceSet<NP> &d, int j) {  // pieces j, j+1 (j even) of a FULL tile: 16-byte nt loads only
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    d.k[k] = load16_nt(reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(cols.c[k] + base + (uint64_t)j * kLeafF64) + lane_bytes));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < NP; ++k)
                        d.f[h][k] = load16<true>(reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(cols.f[k] + base + (uint64_t)(j + h) * kLeafF64) + lane_bytes));
            };
            PieceSet<NP> a, b;
            load_full(a, rot);
#pragma unroll 1
            for (int i = 0; i < kRadix; i += kPieces) {  // one leaf per turn
                const int j = (i + rot) & (kRadix - 1);  // rot is a multiple of the leaf's pieces: they stay together
                load_full(b, j + 2);
                fst_pops_accumulate<NP, Est>(acc, cnt, a, minind, lane);
                if (i + kPieces < kRadix) load_full(a, (j + kPieces) & (kRadix - 1));
                fst_pops_accumulate<NP, Est>(acc, cnt, b, minind, lane);
                finish_leaf(j / kPieces);
            }
        } else {  // the last, partial tile (one wave, once): guarded loads; a site beyond n has a count of 0 and is never counted
#pragma unroll 1
            for (int q = 0; q < kRadix1; ++q) {
#pragma unroll 1
                for (int g = 0; g < 2; ++g) {
                    const int j = q * kPieces + 2 * g;
                    PieceSet<NP> s;
                    const uint64_t c0 = base + (uint64_t)j * kLeafF64 + 4 * (uint64_t)lane;
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        s.k[k].x = c0 < n ? cols.c[k][c0] : 0;
                        s.k[k].y = c0 + 1 < n ? cols.c[k][c0 + 1] : 0;
                        s.k[k].z = c0 + 2 < n ? cols.c[k][c0 + 2] : 0;
                        s.k[k].w = c0 + 3 < n ? cols.c[k][c0 + 3] : 0;
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint64_t f0 = base + (uint64_t)(j + h) * kLeafF64 + 2 * (uint64_t)lane;
#pragma unroll
                        for (int k = 0; k < NP; ++k) {
                            s.f[h][k].x = f0 < n ? cols.f[k][f0] : 0.0;
                            s.f[h][k].y = f0 + 1 < n ? cols.f[k][f0 + 1] : 0.0;
                        }
                    }
                    fst_pops_accumulate<NP, Est>(acc, cnt, s, minind, lane);
                }
                finish_leaf(q);
            }
        }
        // the level-2 node = the tile's leaf nodes added in LEAF order, whatever order they were produced in
        if (my >= 0) {
            double l2 = 0.0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) l2 += stage_s[q * V + my];
            sum_node<NP>(tv, 1, t)[my] = l2;
            tot_s += l2;
        }
        if (lane < P) {
            uint32_t c2 = 0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) c2 += stage_c[q * P + lane];
            cnt_node<NP>(tv, 1, t)[lane] = c2;
            tot_c += c2;
        }
        // the tile's 16 level-1 nodes: one contiguous block of 256 P bytes of sums and one of 64 P bytes of counts
        flush_stage<V * kRadix1>(sum_node<NP>(tv, 0, t * kRadix1), stage_s, lane);
        {
            uint4 *cdst = reinterpret_cast<uint4 *>(cnt_node<NP>(tv, 0, t * kRadix1));
            const uint4 *csrc = reinterpret_cast<const uint4 *>(stage_c);
            constexpr int kCVec = P * kRadix1 / 4;
#pragma unroll 2
            for (int e = lane; e < kCVec; e += kWave) {
                const uint4 w = csrc[e];
                __builtin_nontemporal_store(w.x, &cdst[e].x);
                __builtin_nontemporal_store(w.y, &cdst[e].y);
                __builtin_nontemporal_store(w.z, &cdst[e].z);
                __builtin_nontemporal_store(w.w, &cdst[e].w);
            }
        }
    }
    // one partial {Σa, Σ(a+b), neff} per pair and build wave: the genome-wide lines are their sums in wave order (fixed by the
    // static grid, a function of n alone); a wave without a tile leaves the identity
    if (my >= 0) reinterpret_cast<double *>(tv.base + tv.part_sum)[wave0 * V + my] = tot_s;
    if (lane < P) reinterpret_cast<uint32_t *>(tv.base + tv.part_cnt)[wave0 * P + lane] = tot_c;
}

// Two occupancies of the one body (as dxy_pops_build_kernel / _w1): two waves per SIMD with 256 registers each, or one with
// the whole file.
template <int NP, class Est>
__global__ __launch_bounds__(256, 2) void fst_pops_build_kernel(PopCols cols, int minind, uint64_t n, uint64_t n_l2, FstPopsTree tv) {
    fst_pops_build_body<NP, Est>(cols, minind, n, n_l2, tv);
}
template <int NP, class Est>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void fst_pops_build_kernel_w1(PopCols cols, int minind, uint64_t n, uint64_t n_l2, FstPopsTree tv) {
    fst_pops_build_body<NP, Est>(cols, minind, n, n_l2, tv);
}
constexpr int kOneWaveFrom = 5;  // populations from which the build takes one wave per SIMD (two register sets of 12 NP and 3 P running values)

// ---- upper levels: parent = Σ of 64 children, per sum (blockIdx.y < 2 P; the first P also carry the pair's count) --------
__global__ __launch_bounds__(256) void fst_pops_up_kernel(FstPopsTree tv, int child_slot, uint64_t n_child, uint64_t n_parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int v = blockIdx.y, P = tv.n_pairs, V = 2 * P;
    const double *cs = reinterpret_cast<const double *>(tv.base + tv.sum_off[child_slot]);
    const uint32_t *cc = reinterpret_cast<const uint32_t *>(tv.base + tv.cnt_off[child_slot]);
    double *ps = reinterpret_cast<double *>(tv.base + tv.sum_off[child_slot + 1]);
    uint32_t *pc = reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[child_slot + 1]);
    for (uint64_t p = wave0; p < n_parent; p += n_waves) {
        const uint64_t i = p * kRadix + lane;
        double x = i < n_child ? cs[i * V + v] : 0.0;
        x = wave_sum(x);
        if (lane == 0) ps[p * V + v] = x;
        if (v < P) {
            uint32_t c = i < n_child ? cc[i * P + v] : 0u;
            c = wave_sum(c);
            if (lane == 0) pc[p * P + v] = c;
        }
    }
}

// ---- QUERY: one wave per window, all pairs at once; one more item for the genome-wide lines ------------------------------
// dxy_pops_query_kernel with two sums per pair: a lane takes the QUAD of sites 4L .. 4L+3 of a 256-site stride that starts at
// a multiple of 4 (one 16-byte load per count column, two per frequency column); sites of the quad outside [from, to) get a
// count of 0; the column's last quad, when n is not a multiple of 4, is read site by site.  A lane adds its items in an order
// that depends on the window alone: left sites, right sites, then per level the left and right ragged nodes.
template <int NP, class Est>
__global__ __launch_bounds__(256, (NP >= 5 ? 1 : 2)) void fst_pops_query_kernel(PopCols cols, int minind, const uint32_t *__restrict__ pos, FstPopsTree tv,
                                                             const pgt_win *__restrict__ win, uint64_t n_win,
                                                             pgt_fst_row *__restrict__ out, pgt_fst_total *__restrict__ tot, uint64_t n_sites) {
    constexpr int P = Shape<NP>::kPairs;
    constexpr int V = Shape<NP>::kSums;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_items = n_win + (tot ? 1 : 0);

    for (uint64_t w = wave0; w < n_items; w += n_waves) {
        double acc[V];      // per lane
        uint32_t ncnt[P];   // per lane: neff of the nodes this lane read
        uint32_t scnt[P];   // wave-uniform: neff of the ragged sites
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < P; ++v) { ncnt[v] = 0u; scnt[v] = 0u; }
        if (w == n_win) {  // the genome-wide lines: the build waves' partials, lane l adds partials l, l + 64, .. in turn
            const double *ps = reinterpret_cast<const double *>(tv.base + tv.part_sum);
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(tv.base + tv.part_cnt);
            for (uint32_t i = (uint32_t)lane; i < tv.n_partials; i += kWave) {
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += ps[(uint64_t)i * V + v];
#pragma unroll
                for (int v = 0; v < P; ++v) ncnt[v] += pc[(uint64_t)i * P + v];
            }
            double sa = 0.0, sb = 0.0;
            uint32_t c = 0;
#pragma unroll
            for (int v = 0; v < P; ++v) {
                const double av = wave_sum(acc[v]);
                const double bv = wave_sum(acc[P + v]);
                const uint32_t cv = wave_sum(ncnt[v]);
                if (v == lane) { sa = av; sb = bv; c = cv; }
            }
            if (lane < P) {
                pgt_fst_total r;
                r.asum = sa + 0.0;
                r.bsum = sb + 0.0;
                r.neff = c;
                r.nskip = n_sites - c;
                tot[lane] = r;
            }
            continue;
        }
        const pgt_win wd = win[w];
        const uint64_t hi = wd.hi < n_sites ? wd.hi : n_sites;  // clamped: a corrupt table can never fault the GPU
        const uint64_t lo = wd.lo < hi ? wd.lo : hi;
        uint32_t start = wd.start, end = wd.end;
        if (!(wd.flags & PGT_WIN_COORDS)) {
            start = hi > lo ? pos[lo] : 0u;
            end = hi > lo ? pos[hi - 1] : 0u;
        }
        auto sum_sites = [&](uint64_t from, uint64_t to) {  // wave-uniform arguments; to <= n_sites
            for (uint64_t at = from & ~(uint64_t)3; at < to; at += 4 * (uint64_t)kWave) {
                const uint64_t i = at + 4 * (uint64_t)lane;
                int4 k[NP];
                double2 f0[NP], f1[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) { k[q] = int4{0, 0, 0, 0}; f0[q] = double2{0.0, 0.0}; f1[q] = double2{0.0, 0.0}; }
                if (i < to && i + 4 <= n_sites) {
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        k[q] = *reinterpret_cast<const int4 *>(cols.c[q] + i);
                        f0[q] = *reinterpret_cast<const double2 *>(cols.f[q] + i);
                        f1[q] = *reinterpret_cast<const double2 *>(cols.f[q] + i + 2);
                    }
                } else if (i < to) {  // the column's last quad
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        if (i < n_sites) { k[q].x = cols.c[q][i]; f0[q].x = cols.f[q][i]; }
                        if (i + 1 < n_sites) { k[q].y = cols.c[q][i + 1]; f0[q].y = cols.f[q][i + 1]; }
                        if (i + 2 < n_sites) { k[q].z = cols.c[q][i + 2]; f1[q].x = cols.f[q][i + 2]; }
                    }
                }
                bool in[4];  // site i + e lies in [from, to)
#pragma unroll
                for (int e = 0; e < 4; ++e) in[e] = i + e >= from && i + e < to;
                double p[NP];
                int c[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) { p[q] = f0[q].x; c[q] = in[0] ? k[q].x : 0; }
                fst_pops_site<NP, Est>(acc, scnt, p, c, minind);
#pragma unroll
                for (int q = 0; q < NP; ++q) { p[q] = f0[q].y; c[q] = in[1] ? k[q].y : 0; }
                fst_pops_site<NP, Est>(acc, scnt, p, c, minind);
#pragma unroll
                for (int q = 0; q < NP; ++q) { p[q] = f1[q].x; c[q] = in[2] ? k[q].z : 0; }
                fst_pops_site<NP, Est>(acc, scnt, p, c, minind);
#pragma unroll
                for (int q = 0; q < NP; ++q) { p[q] = f1[q].y; c[q] = in[3] ? k[q].w : 0; }
                fst_pops_site<NP, Est>(acc, scnt, p, c, minind);
            }
        };
        auto add_node = [&](int slot, uint64_t i) {
            const double *s = sum_node<NP>(tv, slot, i);
            const uint32_t *c = cnt_node<NP>(tv, slot, i);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += s[v];
#pragma unroll
            for (int v = 0; v < P; ++v) ncnt[v] += c[v];
        };
        auto sum_nodes = [&](int level, uint64_t from, uint64_t to) {
            for (uint64_t i = from + lane; i < to; i += kWave) add_node(level - 1, i);
        };
        // the range descent: the same loop as in af_query_kernel and dxy_pops_query_kernel, where its rule is explained (each
        // kernel keeps its copy: a change to one belongs in the others too)
        uint64_t clo = lo, chi = hi;
        for (int k = 0;; ++k) {
            const bool top = k == tv.n_levels;
            const uint64_t r = k == 0 ? (uint64_t)kLeaf : (k == 1 ? (uint64_t)kRadix1 : (uint64_t)kRadix);
            const uint64_t ulo = (clo + r - 1) / r, uhi = chi / r;
            if (top || ulo >= uhi) {
                if (k == 0) sum_sites(clo, chi); else sum_nodes(k, clo, chi);
                break;
            }
            if (k == 0) { sum_sites(clo, ulo * r); sum_sites(uhi * r, chi); }
            else {
                // both ragged sides of a node level in one trip when each holds at most 32 nodes (always on level 1)
                const uint64_t nl = ulo * r - clo, nr = chi - uhi * r;
                if (nl <= 32 && nr <= 32) {
                    const uint64_t q = (uint64_t)(lane & 31);
                    if (lane < 32 ? q < nl : q < nr) add_node(k - 1, lane < 32 ? clo + q : uhi * r + q);
                } else {
                    sum_nodes(k, clo, ulo * r);
                    sum_nodes(k, uhi * r, chi);
                }
            }
            clo = ulo;
            chi = uhi;
        }
        double sa = 0.0, sb = 0.0;
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < P; ++v) {
            const double av = wave_sum(acc[v]);
            const double bv = wave_sum(acc[P + v]);
            const uint32_t cv = wave_sum(ncnt[v]) + scnt[v];
            if (v == lane) { sa = av; sb = bv; c = cv; }
        }
        if (lane < P) {  // lane p finishes pair p
            pgt_fst_row r;
            r.start = start;
            r.end = end;
            r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
            r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
            r.asum = sa + 0.0;
            r.bsum = sb + 0.0;
            r.fst = r.bsum != 0.0 ? r.asum / r.bsum : 0.0;  // fstWindow.cpp:85
            out[(uint64_t)lane * n_win + w] = r;
        }
    }
}

template <int NP>
constexpr size_t stage_bytes() { return (size_t)4 * kRadix1 * Shape<NP>::kPairs * 20; }

template <int NP, class Est>
int launch_np(const PopCols &cols, const uint32_t *pos, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
              pgt_fst_row *out, pgt_fst_total *tot, FstPopsTree tv, const TreeLayout &tl, hipStream_t s, void *ev_b0,
              void *ev_b1, void *ev_q1, std::string *err) {
    if (int rc = record_event(ev_b0, s, err)) return rc;
    tv.n_partials = 0;
    if (n > 0) {
        constexpr bool w1 = NP >= kOneWaveFrom;
        const auto [blocks, n_partials] = pops_build_grid(tl.count[1], w1);
        tv.n_partials = n_partials;
        if constexpr (w1)
            hipLaunchKernelGGL((fst_pops_build_kernel_w1<NP, Est>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        else
            hipLaunchKernelGGL((fst_pops_build_kernel<NP, Est>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        if (int rc = hip_fail(hipGetLastError(), "fst_pops_build_kernel", err)) return rc;
        if (int rc = launch_upper_levels(fst_pops_up_kernel, "fst_pops_up_kernel", Shape<NP>::kSums, tv, tl, s, err)) return rc;
    }
    if (int rc = record_event(ev_b1, s, err)) return rc;
    if (n_win > 0 || tot) {
        hipLaunchKernelGGL((fst_pops_query_kernel<NP, Est>), dim3(wave_grid(n_win + (tot ? 1 : 0))), dim3(256), 0, s, cols, minind, pos, tv, win, n_win, out, tot, n);
        if (int rc = hip_fail(hipGetLastError(), "fst_pops_query_kernel", err)) return rc;
    }
    return record_event(ev_q1, s, err);
}

template <int NP, class Est>
void allow_lds() {
    if constexpr (NP >= kOneWaveFrom)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fst_pops_build_kernel_w1<NP, Est>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
    else
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fst_pops_build_kernel<NP, Est>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
}

template <class Est>
void allow_lds_all() {
    allow_lds<2, Est>(); allow_lds<3, Est>(); allow_lds<4, Est>(); allow_lds<5, Est>(); allow_lds<6, Est>(); allow_lds<7, Est>(); allow_lds<8, Est>();
}

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_fst_pops_kernels(std::string *err) {
    allow_lds_all<WeirCockerham>();
    allow_lds_all<Hudson>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

int launch_fst_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                    int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot, void *tree,
                    void *stream, void *ev_build0, void *ev_build1, void *ev_query1, std::string *err, const Hints &hints,
                    FstPopsEstimator estimator) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 2 <= n_pops <= 8 and minind >= 1: checked by the caller; both estimators share the tree's layout
    const TreeLayout tl = tree_layout(PGT_STAT_FST, n);  // node counts of the f64 layout (levels 2 and up; level 1: a quarter)
    const FstPopsTree tv = fst_pops_tree_view(tl, (int)(n_pops * (n_pops - 1) / 2), tree, useful_levels(tl, PGT_STAT_FST, hints.max_window));
    PopCols cols{};
    for (uint32_t k = 0; k < n_pops; ++k) { cols.f[k] = freq[k]; cols.c[k] = nind[k]; }
    return dispatch_n_pops(n_pops, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        if (estimator == FstPopsEstimator::Hudson)
            return launch_np<NP, Hudson>(cols, pos, n, minind, win, n_win, out, tot, tv, tl, s, ev_build0, ev_build1, ev_query1, err);
        return launch_np<NP, WeirCockerham>(cols, pos, n, minind, win, n_win, out, tot, tv, tl, s, ev_build0, ev_build1, ev_query1, err);
    });
}

}  // namespace pgt
