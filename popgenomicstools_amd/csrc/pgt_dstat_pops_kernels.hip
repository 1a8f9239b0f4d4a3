// pgt_dstat_pops_kernels.hip — the ABBA-BABA site patterns (Patterson's D; Green et al. 2010, Durand et al. 2011) of ALL trios
// i < j < k of the ingroup populations against one outgroup, from 4 ... 7 populations' own MAF columns (allele frequency f64 +
// individual count i32: 12 B/site/population) in ONE pass, with dxyWindow's -minind predicate over the four populations.
//
// Spec (include/pgtwin.h, pgt_dstat_pops_reduce_dev): the last population o = NP-1 is the outgroup, the first NP-1 the ingroup;
// trio (i, j, k), i < j < k < NP-1, in lexicographic order.  The site counts iff all four populations have at least minind
// individuals, and then contributes, with p_x the frequency and q_x = 1 - p_x, every operation rounded on its own:
//     bbaa = (p_i*p_j)*(q_k*q_o) + (q_i*q_j)*(p_k*p_o)
//     abba = (q_i*p_j)*(p_k*q_o) + (p_i*q_j)*(q_k*p_o)
//     baba = (p_i*q_j)*(p_k*q_o) + (q_i*p_j)*(q_k*p_o)
// (the second term is the pattern with the two alleles' roles swapped: Dsuite's form).  The four products of an ingroup pair
// (i, j) and the four products of (k, o) are computed once per site and shared by every trio that holds them: at 7
// populations 40 + 16 products and 7 subtractions serve 20 trios of 6 products and 3 additions each.  A window's row is the
// three sums and the number of counted sites; d = (abba - baba) / (abba + baba).  A site that is not counted is never added
// (a select, not a product with 0): its frequencies may be anything.
//
// Tree, build walk, reduce-scatter, LDS-staged node block, per-wave partials and the one-wave-per-window query: those of
// pgt_fst_pops_kernels.hip with "a pair keeps two sums and a count" replaced by "a trio keeps three sums and a count": a node
// is 3 T doubles (bbaa of trio 0 .. T-1, then abba, then baba) and T u32, T = C(NP-1, 3) = 1 / 4 / 10 / 20.  The counts decide
// nothing but the predicate, so they travel as in pgt_dxy_pops_kernels.hip, the cheaper of the two exchanges: each lane
// packs "population k has enough individuals at site 4L+c" into bit 4k+c of ONE register and the lane that owns the sites in
// the frequency layout fetches that register (one ds_bpermute per piece for all populations; the FST build moves the count
// VALUES, four per population and piece).  Per population the bits become lane masks, a trio's predicate is the AND of four
// of them, its neff the popcount of that AND (scalar, wave-uniform).
//
// Rows of a trio are functions of the trio's and the outgroup's eight columns and the window alone: every trio's arithmetic
// reads only its four populations' registers, and the order of all additions is fixed by the site index and the window.
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

constexpr int trio_count(int np) { return (np - 1) * (np - 2) * (np - 3) / 6; }  // C(np - 1, 3)

template <int NP>
struct Shape {
    static_assert(NP >= 4 && NP <= 7, "three ingroup populations and an outgroup; 20 trios at most");
    static constexpr int kTrios = trio_count(NP);  // lexicographic (i < j < k < NP-1): (0,1,2),(0,1,3),..,(0,2,3),..
    static constexpr int kSums = 3 * kTrios;       // Σbbaa of every trio, then Σabba of every trio, then Σbaba of every trio
};

struct PopCols {
    const double *f[kPopsMaxPops];
    const int32_t *c[kPopsMaxPops];
};

// ---- per-site contribution ---------------------------------------------------------------------------------------------
// One site of this lane into the lane's 3 T running sums and the wave's T counters.  okbits: bit 4k = population k has at
// least minind individuals at this site.  MUST be called by all 64 lanes together (the counters are popcounts of ballots).
template <int NP>
__device__ __forceinline__ void dstat_pops_site(double *acc, uint32_t *cnt, const double *p, uint32_t okbits) {
    constexpr int G = NP - 1;  // ingroup populations; G is the outgroup's index
    constexpr int T = Shape<NP>::kTrios;
    double q[NP];
    bool ok[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        q[k] = __dsub_rn(1.0, p[k]);
        ok[k] = ((okbits >> (4 * k)) & 1u) != 0;
    }
    // the four products of (k, o), once per site for every trio with k as its third population (k >= 2)
    double k_qq[G], k_pp[G], k_pq[G], k_qp[G];
#pragma unroll
    for (int k = 2; k < G; ++k) {
        k_qq[k] = __dmul_rn(q[k], q[G]);
        k_pp[k] = __dmul_rn(p[k], p[G]);
        k_pq[k] = __dmul_rn(p[k], q[G]);
        k_qp[k] = __dmul_rn(q[k], p[G]);
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < G; ++i)
#pragma unroll
        for (int j = i + 1; j + 1 < G; ++j) {
            // the four products of the ingroup pair (i, j), once per site for every trio (i, j, k > j)
            const double pp = __dmul_rn(p[i], p[j]), qq = __dmul_rn(q[i], q[j]);
            const double qp = __dmul_rn(q[i], p[j]), pq = __dmul_rn(p[i], q[j]);
            const bool ok_ij = ok[i] && ok[j] && ok[G];
#pragma unroll
            for (int k = j + 1; k < G; ++k) {
                const bool counted = ok_ij && ok[k];
                const double bbaa = __dadd_rn(__dmul_rn(pp, k_qq[k]), __dmul_rn(qq, k_pp[k]));
                const double abba = __dadd_rn(__dmul_rn(qp, k_pq[k]), __dmul_rn(pq, k_qp[k]));
                const double baba = __dadd_rn(__dmul_rn(pq, k_pq[k]), __dmul_rn(qp, k_qp[k]));
                acc[t] = __dadd_rn(acc[t], counted ? bbaa : 0.0);
                acc[T + t] = __dadd_rn(acc[T + t], counted ? abba : 0.0);
                acc[2 * T + t] = __dadd_rn(acc[2 * T + t], counted ? baba : 0.0);
                cnt[t] += (uint32_t)__popcll(__ballot(counted));
                ++t;
            }
        }
}

// A pair of 128-site pieces in registers: the counts of the pair's 256 sites (lane L: sites 4L .. 4L+3 of the pair) and
// the frequencies of its two pieces (lane l: sites 2l, 2l+1 of piece h).
template <int NP>
struct PieceSet {
    int4 k[NP];
    double2 f[2][NP];
};
// bit 4k+c: population k has at least minind individuals at site 4L+c of the pair (count layout)
template <int NP>
__device__ __forceinline__ uint32_t pop_ok_bits(const int4 *k, int minind) {
    uint32_t b = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        b |= (k[q].x >= minind ? 1u : 0u) << (4 * q);
        b |= (k[q].y >= minind ? 2u : 0u) << (4 * q);
        b |= (k[q].z >= minind ? 4u : 0u) << (4 * q);
        b |= (k[q].w >= minind ? 8u : 0u) << (4 * q);
    }
    return b;
}
// The lane's four sites of a pair of pieces, in site order, into the running sums.
template <int NP>
__device__ __forceinline__ void dstat_pops_accumulate(double *acc, uint32_t *cnt, const PieceSet<NP> &s, uint32_t okb, int lane) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // the bits of this lane's sites 2l, 2l+1 of piece h = pair sites 128h + 2l + q: count lane 32h + (l >> 1), component 2(l & 1) + q
        const uint32_t w = (uint32_t)__shfl((int)okb, 32 * h + (lane >> 1), kWave) >> (2 * (lane & 1));
        double px[NP], py[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) { px[k] = s.f[h][k].x; py[k] = s.f[h][k].y; }
        dstat_pops_site<NP>(acc, cnt, px, w);
        dstat_pops_site<NP>(acc, cnt, py, w >> 1);
    }
}

template <int NP>
__device__ __forceinline__ double *sum_node(const DstatPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<double *>(tv.base + tv.sum_off[slot]) + i * Shape<NP>::kSums;
}
template <int NP>
__device__ __forceinline__ uint32_t *cnt_node(const DstatPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[slot]) + i * Shape<NP>::kTrios;
}

// ---- BUILD: one wave per level-2 tile (64 pieces of 128 sites = 16 leaf nodes of 512 sites) -----------------------------
// The walk of fst_pops_build_body: a PAIR of pieces is the unit (a 16-byte count load spans two pieces), two register sets
// swap roles, a full tile is walked from a piece of the wave's own, the tile's level-1 nodes are staged in LDS and leave as
// contiguous blocks of nt stores.  A leaf's sums do not depend on the wave or on where its walk started: a lane adds its 8
// sites of the leaf in site order, the reduce-scatter is a fixed tree, and the level-2 node adds the 16 leaf nodes in leaf order.
template <int NP>
__device__ __forceinline__ void dstat_pops_build_body(const PopCols &cols, int minind, uint64_t n, uint64_t n_l2, const DstatPopsTree &tv) {
    constexpr int T = Shape<NP>::kTrios;
    constexpr int V = Shape<NP>::kSums;
    static_assert(V <= kWave, "the reduce-scatter leaves one total per lane");
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int my = rs_my_index<V>(lane);
    const uint32_t lane_bytes = (uint32_t)lane * 16u;
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    // the wave's LDS stage: 16 nodes x 3 T doubles, then 16 nodes x T u32 (private to the wave: no barrier)
    extern __shared__ __attribute__((aligned(16))) char dstat_pops_stage[];
    char *stage = dstat_pops_stage + (size_t)(threadIdx.x >> 6) * (kRadix1 * T * 28);
    double *stage_s = reinterpret_cast<double *>(stage);
    uint32_t *stage_c = reinterpret_cast<uint32_t *>(stage + kRadix1 * V * 8);

    double tot_s = 0.0;   // lane `my`: Σ of the level-2 nodes this wave wrote, in tile order (the genome-wide line's partial)
    uint32_t tot_c = 0;   // lane t < T: their neff

    for (uint64_t t = wave0; t < n_l2; t += n_waves) {
        const uint64_t base = t * kTile2;
        const bool full = base + kTile2 <= n;
        // a multiple of the leaf's pieces below 64 (see tile_rotation in pgt_kernels.hip); the partial last tile is walked from its start
        const int rot = full ? (int)(((wave0 * 0x9E3779B1ull) >> 13) & (uint64_t)(kRadix - kPieces)) : 0;
        double acc[V];
        uint32_t cnt[T];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < T; ++v) cnt[v] = 0u;
        auto finish_leaf = [&](int node) {  // the leaf's 3 T sums and T counts into the stage; the running sums start again
            rs_steps<V, 0>(acc, lane);
            if (my >= 0) stage_s[node * V + my] = acc[0];
            uint32_t cv = 0;
#pragma unroll
            for (int v = 0; v < T; ++v) cv = lane == v ? cnt[v] : cv;
            if (lane < T) stage_c[node * T + lane] = cv;
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
            for (int v = 0; v < T; ++v) cnt[v] = 0u;
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
                dstat_pops_accumulate<NP>(acc, cnt, a, pop_ok_bits<NP>(a.k, minind), lane);
                if (i + kPieces < kRadix) load_full(a, (j + kPieces) & (kRadix - 1));
                dstat_pops_accumulate<NP>(acc, cnt, b, pop_ok_bits<NP>(b.k, minind), lane);
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
                    uint32_t valid = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) valid |= (c0 + e < n ? 1u : 0u) << e;
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
                    dstat_pops_accumulate<NP>(acc, cnt, s, pop_ok_bits<NP>(s.k, minind) & (valid * 0x11111111u), lane);
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
        if (lane < T) {
            uint32_t c2 = 0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) c2 += stage_c[q * T + lane];
            cnt_node<NP>(tv, 1, t)[lane] = c2;
            tot_c += c2;
        }
        // the tile's 16 level-1 nodes: one contiguous block of 384 T bytes of sums and one of 64 T bytes of counts
        flush_stage<V * kRadix1>(sum_node<NP>(tv, 0, t * kRadix1), stage_s, lane);
        {
            uint4 *cdst = reinterpret_cast<uint4 *>(cnt_node<NP>(tv, 0, t * kRadix1));
            const uint4 *csrc = reinterpret_cast<const uint4 *>(stage_c);
            constexpr int kCVec = T * kRadix1 / 4;
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
    // one partial {Σbbaa, Σabba, Σbaba, neff} per trio and build wave: the genome-wide lines are their sums in wave order (fixed
    // by the static grid, a function of n alone); a wave without a tile leaves the identity
    if (my >= 0) reinterpret_cast<double *>(tv.base + tv.part_sum)[wave0 * V + my] = tot_s;
    if (lane < T) reinterpret_cast<uint32_t *>(tv.base + tv.part_cnt)[wave0 * T + lane] = tot_c;
}

// Two occupancies of the one body (as fst_pops_build_kernel / _w1): two waves per SIMD with 256 registers each, or one with
// the whole file.
template <int NP>
__global__ __launch_bounds__(256, 2) void dstat_pops_build_kernel(PopCols cols, int minind, uint64_t n, uint64_t n_l2, DstatPopsTree tv) {
    dstat_pops_build_body<NP>(cols, minind, n, n_l2, tv);
}
template <int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dstat_pops_build_kernel_w1(PopCols cols, int minind, uint64_t n, uint64_t n_l2, DstatPopsTree tv) {
    dstat_pops_build_body<NP>(cols, minind, n, n_l2, tv);
}
// populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r12/dstat_pops.md) shows
// the two-wave build at 182 registers with 4 populations and spilling from 5 on (52 / 404 / 912 bytes of scratch per lane at
// 5 / 6 / 7: two register sets of 12 NP and 6 T running values), the one-wave build without scratch at every count
constexpr int kOneWaveFrom = 5;

// ---- upper levels: parent = Σ of 64 children, per sum (blockIdx.y < 3 T; the first T also carry the trio's count) --------
__global__ __launch_bounds__(256) void dstat_pops_up_kernel(DstatPopsTree tv, int child_slot, uint64_t n_child, uint64_t n_parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int v = blockIdx.y, T = tv.n_pairs, V = 3 * T;
    const double *cs = reinterpret_cast<const double *>(tv.base + tv.sum_off[child_slot]);
    const uint32_t *cc = reinterpret_cast<const uint32_t *>(tv.base + tv.cnt_off[child_slot]);
    double *ps = reinterpret_cast<double *>(tv.base + tv.sum_off[child_slot + 1]);
    uint32_t *pc = reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[child_slot + 1]);
    for (uint64_t p = wave0; p < n_parent; p += n_waves) {
        const uint64_t i = p * kRadix + lane;
        double x = i < n_child ? cs[i * V + v] : 0.0;
        x = wave_sum(x);
        if (lane == 0) ps[p * V + v] = x;
        if (v < T) {
            uint32_t c = i < n_child ? cc[i * T + v] : 0u;
            c = wave_sum(c);
            if (lane == 0) pc[p * T + v] = c;
        }
    }
}

// ---- QUERY: one wave per window, all trios at once; one more item for the genome-wide lines ------------------------------
// fst_pops_query_kernel with three sums per trio: a lane takes the QUAD of sites 4L .. 4L+3 of a 256-site stride that starts at
// a multiple of 4 (one 16-byte load per count column, two per frequency column); sites of the quad outside [from, to) are
// never counted; the column's last quad, when n is not a multiple of 4, is read site by site.  A lane adds its items in an
// order that depends on the window alone: left sites, right sites, then per level the left and right ragged nodes.
template <int NP>
__global__ __launch_bounds__(256, (NP >= 6 ? 1 : 2)) void dstat_pops_query_kernel(PopCols cols, int minind, const uint32_t *__restrict__ pos, DstatPopsTree tv,
                                                               const pgt_win *__restrict__ win, uint64_t n_win,
                                                               pgt_dstat_row *__restrict__ out, pgt_dstat_total *__restrict__ tot, uint64_t n_sites) {
    constexpr int T = Shape<NP>::kTrios;
    constexpr int V = Shape<NP>::kSums;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_items = n_win + (tot ? 1 : 0);

    for (uint64_t w = wave0; w < n_items; w += n_waves) {
        double acc[V];      // per lane
        uint32_t ncnt[T];   // per lane: neff of the nodes this lane read
        uint32_t scnt[T];   // wave-uniform: neff of the ragged sites
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < T; ++v) { ncnt[v] = 0u; scnt[v] = 0u; }
        if (w == n_win) {  // the genome-wide lines: the build waves' partials, lane l adds partials l, l + 64, .. in turn
            const double *ps = reinterpret_cast<const double *>(tv.base + tv.part_sum);
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(tv.base + tv.part_cnt);
            for (uint32_t i = (uint32_t)lane; i < tv.n_partials; i += kWave) {
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += ps[(uint64_t)i * V + v];
#pragma unroll
                for (int v = 0; v < T; ++v) ncnt[v] += pc[(uint64_t)i * T + v];
            }
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            uint32_t c = 0;
#pragma unroll
            for (int v = 0; v < T; ++v) {
                const double v0 = wave_sum(acc[v]);
                const double v1 = wave_sum(acc[T + v]);
                const double v2 = wave_sum(acc[2 * T + v]);
                const uint32_t cv = wave_sum(ncnt[v]);
                if (v == lane) { s0 = v0; s1 = v1; s2 = v2; c = cv; }
            }
            if (lane < T) {
                pgt_dstat_total r;
                r.bbaa = s0 + 0.0;
                r.abba = s1 + 0.0;
                r.baba = s2 + 0.0;
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
                uint32_t in = 0;  // bit e: site i + e lies in [from, to) (and below n_sites: to <= n_sites)
#pragma unroll
                for (int e = 0; e < 4; ++e) in |= (i + e >= from && i + e < to ? 1u : 0u) << e;
                const uint32_t okb = pop_ok_bits<NP>(k, minind) & (in * 0x11111111u);
                double p[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].x;
                dstat_pops_site<NP>(acc, scnt, p, okb);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].y;
                dstat_pops_site<NP>(acc, scnt, p, okb >> 1);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].x;
                dstat_pops_site<NP>(acc, scnt, p, okb >> 2);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].y;
                dstat_pops_site<NP>(acc, scnt, p, okb >> 3);
            }
        };
        auto add_node = [&](int slot, uint64_t i) {
            const double *s = sum_node<NP>(tv, slot, i);
            const uint32_t *c = cnt_node<NP>(tv, slot, i);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += s[v];
#pragma unroll
            for (int v = 0; v < T; ++v) ncnt[v] += c[v];
        };
        auto sum_nodes = [&](int level, uint64_t from, uint64_t to) {
            for (uint64_t i = from + lane; i < to; i += kWave) add_node(level - 1, i);
        };
        // the range descent: the same loop as in af_query_kernel, dxy_pops_query_kernel and fst_pops_query_kernel, where its
        // rule is explained (each kernel keeps its copy: a change to one belongs in the others too)
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
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < T; ++v) {
            const double v0 = wave_sum(acc[v]);
            const double v1 = wave_sum(acc[T + v]);
            const double v2 = wave_sum(acc[2 * T + v]);
            const uint32_t cv = wave_sum(ncnt[v]) + scnt[v];
            if (v == lane) { s0 = v0; s1 = v1; s2 = v2; c = cv; }
        }
        if (lane < T) {  // lane t finishes trio t
            pgt_dstat_row r;
            r.start = start;
            r.end = end;
            r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
            r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
            r.bbaa = s0 + 0.0;
            r.abba = s1 + 0.0;
            r.baba = s2 + 0.0;
            const double den = __dadd_rn(r.abba, r.baba);
            r.d = den != 0.0 ? __ddiv_rn(__dsub_rn(r.abba, r.baba), den) : 0.0;  // Patterson's D of ((i,j),k)
            out[(uint64_t)lane * n_win + w] = r;
        }
    }
}

template <int NP>
constexpr size_t stage_bytes() { return (size_t)4 * kRadix1 * Shape<NP>::kTrios * 28; }

template <int NP>
int launch_np(const PopCols &cols, const uint32_t *pos, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
              pgt_dstat_row *out, pgt_dstat_total *tot, DstatPopsTree tv, const TreeLayout &tl, hipStream_t s, void *ev_b0,
              void *ev_b1, void *ev_q1, std::string *err) {
    if (int rc = record_event(ev_b0, s, err)) return rc;
    tv.n_partials = 0;
    if (n > 0) {
        constexpr bool w1 = NP >= kOneWaveFrom;
        const auto [blocks, n_partials] = pops_build_grid(tl.count[1], w1);
        tv.n_partials = n_partials;
        if constexpr (w1)
            hipLaunchKernelGGL((dstat_pops_build_kernel_w1<NP>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        else
            hipLaunchKernelGGL((dstat_pops_build_kernel<NP>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        if (int rc = hip_fail(hipGetLastError(), "dstat_pops_build_kernel", err)) return rc;
        if (int rc = launch_upper_levels(dstat_pops_up_kernel, "dstat_pops_up_kernel", Shape<NP>::kSums, tv, tl, s, err)) return rc;
    }
    if (int rc = record_event(ev_b1, s, err)) return rc;
    if (n_win > 0 || tot) {
        hipLaunchKernelGGL((dstat_pops_query_kernel<NP>), dim3(wave_grid(n_win + (tot ? 1 : 0))), dim3(256), 0, s, cols, minind, pos, tv, win, n_win, out, tot, n);
        if (int rc = hip_fail(hipGetLastError(), "dstat_pops_query_kernel", err)) return rc;
    }
    return record_event(ev_q1, s, err);
}

template <int NP>
void allow_lds() {
    if constexpr (NP >= kOneWaveFrom)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dstat_pops_build_kernel_w1<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
    else
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dstat_pops_build_kernel<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
}

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_dstat_pops_kernels(std::string *err) {
    allow_lds<4>(); allow_lds<5>(); allow_lds<6>(); allow_lds<7>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

int launch_dstat_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                      int minind, const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, pgt_dstat_total *tot, void *tree,
                      void *stream, void *ev_build0, void *ev_build1, void *ev_query1, std::string *err, const Hints &hints) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 4 <= n_pops <= 7 and minind >= 1: checked by the caller
    const TreeLayout tl = tree_layout(PGT_STAT_FST, n);  // node counts of the f64 layout (levels 2 and up; level 1: a quarter)
    const DstatPopsTree tv = dstat_pops_tree_view(tl, trio_count((int)n_pops), tree, useful_levels(tl, PGT_STAT_FST, hints.max_window));
    PopCols cols{};
    for (uint32_t k = 0; k < n_pops; ++k) { cols.f[k] = freq[k]; cols.c[k] = nind[k]; }
    auto go = [&](auto np) {
        constexpr int NP = decltype(np)::value;
        return launch_np<NP>(cols, pos, n, minind, win, n_win, out, tot, tv, tl, s, ev_build0, ev_build1, ev_query1, err);
    };
    switch (n_pops) {  // (dispatch_n_pops of pgt_pops_common.h would instantiate 2, 3 and 8 populations too)
        case 4: return go(std::integral_constant<int, 4>{});
        case 5: return go(std::integral_constant<int, 5>{});
        case 6: return go(std::integral_constant<int, 6>{});
        case 7: return go(std::integral_constant<int, 7>{});
        default: return PGT_EARG;
    }
}

}  // namespace pgt
