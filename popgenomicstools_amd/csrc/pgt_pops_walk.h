// pgt_pops_walk.h — the ONE walk behind the (freq, nInd) front ends for all pairs or trios of up to 8 populations
// (pgt_dxy_pops_kernels.hip, pgt_fst_pops_kernels.hip, pgt_dstat_pops_kernels.hip): the tree build with its two occupancies,
// the upper-level kernel, the one-wave-per-window query, launch_np / allow_lds and the body of an entry point, templated on a
// statistic and on the population count NP.  A statistic file holds its per-site arithmetic and declares
//     kMinPops, kMaxPops     the population counts it is instantiated for
//     items(np)              pairs or trios: what a node, a row table and a finishing lane are numbered by
//     kSumsPerItem           S: a node is S * items doubles (sum 0 of every item, then sum 1, ..) and items u32 (neff)
//     kOneWaveFrom           populations from which the build takes one wave per SIMD; kOneWaveKnob: an environment variable
//                            that lowers it for measuring (both occupancies are then instantiated below it), or nullptr
//     kQueryOneWaveFrom      the same for the query's __launch_bounds__
//     kKernelNames           build, up, query: what a failed launch is reported as
//     Counts                 CountBits or CountValues below: how the counts reach the lane that owns the frequencies
//     site<NP>(acc, cnt, p, c)   one site of this lane into the lane's S * items running sums and the wave's items counters;
//                            c.ok(k): population k has at least minind individuals here; c.n(k): its count (CountValues only).
//                            Called by all 64 lanes together (the counters are popcounts of ballots)
//     Row, Total, finish_row, finish_total   the closing arithmetic of a window's row and of a genome-wide line
//
// Tree: as the allele-frequency front end (pgt_af_kernels.hip) — 512-site level-1 nodes, 16 per 8192-site level-2 node, radix
// 64 above; a level is two node-major arrays (pgt_internal.h: PopsTree).  The order of every addition is fixed by the site
// index and the window alone.  pgt_set_window_step is ignored: every table is answered by the one-wave-per-window query.
#pragma once

#include <hip/hip_runtime.h>

#include "pgt_device.h"
#include "pgt_internal.h"
#include "pgt_pops_common.h"

namespace pgt {
namespace dev {

constexpr int kPieces = kPopsLeafPieces;   // 128-site pieces per level-1 node
constexpr int kLeaf = kPieces * kLeafF64;  // sites per level-1 node (512: the level-1 bytes written are 12 P / 512 per site, 0.7 % of the bytes read by dxy at 8 populations; see pgt_af_kernels.hip on what node stores cost)
constexpr int kRadix1 = kRadix / kPieces;  // level-1 nodes per level-2 node
static_assert(kPieces == 4, "the build walks a leaf as two pairs of pieces");

constexpr int trio_count(int np) { return (np - 1) * (np - 2) * (np - 3) / 6; }  // C(np - 1, 3): ingroup trios, the last population is the outgroup
constexpr int all_trio_count(int np) { return np * (np - 1) * (np - 2) / 6; }     // C(np, 3): the trios of ALL populations (f3: no outgroup)
constexpr int all_quartet_count(int np) { return np * (np - 1) * (np - 2) * (np - 3) / 24; }  // C(np, 4): the quartets of ALL populations (f4)
constexpr int middle_triple_count(int np) { return (np - 2) * (np - 3) * (np - 4) / 6; }  // C(np - 2, 3): the triples between the first and the last population (f4-ratio)

struct PopCols {
    const double *f[kPopsMaxPops];
    const int32_t *c[kPopsMaxPops];
};

// A pair of 128-site pieces in registers: the counts of the pair's 256 sites (lane L: sites 4L .. 4L+3 of the pair) and
// the frequencies of its two pieces (lane l: sites 2l, 2l+1 of piece h).
template <int NP>
struct PieceSet {
    int4 k[NP];
    double2 f[2][NP];
};

// bytes of a build wave's LDS stage per item and level-1 node: S doubles and a u32
constexpr int stage_item_bytes(int sums_per_item) { return 8 * sums_per_item + 4; }

// ---- the count transports ----------------------------------------------------------------------------------------------
// The counts are read by 16-byte loads in the layout of count_pair_pred (pgt_kernels.hip): lane L holds sites 4L .. 4L+3 of a
// PAIR of 128-site pieces, while the lane that owns sites 2l, 2l+1 of piece h in the frequency layout needs them: it fetches
// them from lane 32h + (l >> 1), components 2(l & 1), 2(l & 1) + 1.  pack: the lane's four sites in the count layout, with `in`
// a site whose bit e is clear (outside the range) never counted; pack_padded: the same for sites beyond n, whose counts were
// loaded as 0; fetch: the two sites of piece h as components 0 and 1; view<E>: what the per-site function sees of component E.

// The predicate alone: "population k has enough individuals at site 4L+c" is bit 4k+c of ONE register (8 populations x 4
// sites = 32 bits), one ds_bpermute per piece for all populations.  The per-population bits become lane masks (v_cmp into a
// scalar register pair), an item's predicate the AND of some of them (scalar), its neff the popcount of that AND.
struct CountBits {
    template <int NP>
    using Packed = uint32_t;  // (a plain word, not a struct of one: returned by value a struct loses `noundef`, and the compiler then freezes every count)
    struct View {
        uint32_t b;
        __device__ __forceinline__ bool ok(int k) const { return ((b >> (4 * k)) & 1u) != 0; }
    };
    template <int NP>
    static __device__ __forceinline__ Packed<NP> pack(const int4 *k, int minind) {
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
    template <int NP>
    static __device__ __forceinline__ Packed<NP> pack(const int4 *k, int minind, uint32_t in) {
        return pack<NP>(k, minind) & (in * 0x11111111u);
    }
    template <int NP>  // (minind may be 0 or less: a count of 0 is masked, not trusted to fail the predicate)
    static __device__ __forceinline__ Packed<NP> pack_padded(const int4 *k, int minind, uint32_t valid) { return pack<NP>(k, minind, valid); }
    template <int NP>
    using Fetched = uint32_t;
    template <int NP>
    static __device__ __forceinline__ void fetch(Fetched<NP> &d, Packed<NP> s, int h, int lane) {
        d = (uint32_t)__shfl((int)s, 32 * h + (lane >> 1), kWave) >> (2 * (lane & 1));
    }
    template <int NP, int E>
    static __device__ __forceinline__ View view(Packed<NP> s) { return {s >> E}; }
};

// The VALUES (FST needs the sample sizes): four ds_bpermute per population and piece; a site that is not `in` carries a
// count of 0 (never counted: minind >= 1).  Nothing is copied: a Packed points at the caller's counts (which the masked pack
// zeroes in place), a view at one component of them or at one of the two fetched sites.
struct CountValues {
    template <int NP>
    struct Packed {
        const int4 *k;
        int minind;
    };
    template <int NP>
    struct Fetched {
        int c[2][NP];
        int minind;
    };
    template <int STRIDE>
    struct View {
        const int *c;
        int minind;
        __device__ __forceinline__ bool ok(int k) const { return c[STRIDE * k] >= minind; }
        __device__ __forceinline__ int n(int k) const { return c[STRIDE * k]; }
    };
    template <int NP>
    static __device__ __forceinline__ Packed<NP> pack(const int4 *k, int minind) { return {k, minind}; }
    template <int NP>
    static __device__ __forceinline__ Packed<NP> pack(int4 *k, int minind, uint32_t in) {
#pragma unroll
        for (int q = 0; q < NP; ++q) k[q] = int4{in & 1u ? k[q].x : 0, in & 2u ? k[q].y : 0, in & 4u ? k[q].z : 0, in & 8u ? k[q].w : 0};
        return {k, minind};
    }
    template <int NP>  // (a count of 0 is never counted: minind >= 1)
    static __device__ __forceinline__ Packed<NP> pack_padded(const int4 *k, int minind, uint32_t) { return {k, minind}; }
    template <int NP>
    static __device__ __forceinline__ void fetch(Fetched<NP> &d, const Packed<NP> &s, int h, int lane) {
        const int src = 32 * h + (lane >> 1);
        const bool odd = (lane & 1) != 0;
        d.minind = s.minind;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int x = __shfl(s.k[k].x, src, kWave), y = __shfl(s.k[k].y, src, kWave);
            const int z = __shfl(s.k[k].z, src, kWave), w = __shfl(s.k[k].w, src, kWave);
            d.c[0][k] = odd ? z : x;
            d.c[1][k] = odd ? w : y;
        }
    }
    template <int NP, int E>
    static __device__ __forceinline__ View<1> view(const Fetched<NP> &s) { return {s.c[E], s.minind}; }
    template <int NP, int E>
    static __device__ __forceinline__ View<4> view(const Packed<NP> &s) { return {&s.k[0].x + E, s.minind}; }
};

// The lane's four sites of a pair of pieces, in site order, into the running sums.
template <class Stat, int NP, class Packed>
__device__ __forceinline__ void pops_accumulate(double *acc, uint32_t *cnt, const PieceSet<NP> &s, const Packed &packed, int lane) {
    using C = typename Stat::Counts;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        typename C::template Fetched<NP> w;
        C::template fetch<NP>(w, packed, h, lane);
        double px[NP], py[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) { px[k] = s.f[h][k].x; py[k] = s.f[h][k].y; }
        Stat::template site<NP>(acc, cnt, px, C::template view<NP, 0>(w));
        Stat::template site<NP>(acc, cnt, py, C::template view<NP, 1>(w));
    }
}

template <int V>
__device__ __forceinline__ double *sum_node(const PopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<double *>(tv.base + tv.sum_off[slot]) + i * V;
}
template <int I>
__device__ __forceinline__ uint32_t *cnt_node(const PopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[slot]) + i * I;
}

// ---- BUILD: one wave per level-2 tile (64 pieces of 128 sites = 16 leaf nodes of 512 sites) -----------------------------
// The walk of pgt_af_kernels.hip (piece by piece over all populations, software-pipelined over two register sets that swap
// roles; the tile walked from a piece of the wave's own; the tile's level-1 nodes staged in LDS and written as one
// contiguous block of nt stores), with a PAIR of pieces as the unit, because a 16-byte count load spans two pieces.
// A leaf's sums do not depend on the wave or on where its walk started: a lane adds its 8 sites of the leaf in site order,
// the reduce-scatter is a fixed tree, and the level-2 node adds the 16 leaf nodes in leaf order.
template <class Stat, int NP>
__device__ __forceinline__ void pops_build_body(const PopCols &cols, int minind, uint64_t n, uint64_t n_l2, const PopsTree &tv) {
    using C = typename Stat::Counts;
    constexpr int I = Stat::items(NP);
    constexpr int V = Stat::kSumsPerItem * I;
    static_assert(V <= kWave, "the reduce-scatter leaves one total per lane");
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int my = rs_my_index<V>(lane);
    const uint32_t lane_bytes = (uint32_t)lane * 16u;
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    // the wave's LDS stage: 16 nodes x V doubles, then 16 nodes x I u32 (private to the wave: no barrier)
    extern __shared__ __attribute__((aligned(16))) char pops_stage[];
    char *stage = pops_stage + (size_t)(threadIdx.x >> 6) * (kRadix1 * I * stage_item_bytes(Stat::kSumsPerItem));
    double *stage_s = reinterpret_cast<double *>(stage);
    uint32_t *stage_c = reinterpret_cast<uint32_t *>(stage + kRadix1 * V * 8);

    double tot_s = 0.0;   // lane `my`: Σ of the level-2 nodes this wave wrote, in tile order (the genome-wide line's partial)
    uint32_t tot_c = 0;   // lane v < I: their neff

    for (uint64_t t = wave0; t < n_l2; t += n_waves) {
        const uint64_t base = t * kTile2;
        const bool full = base + kTile2 <= n;
        // a multiple of the leaf's pieces below 64 (see tile_rotation in pgt_kernels.hip); the partial last tile is walked from its start
        const int rot = full ? (int)(((wave0 * 0x9E3779B1ull) >> 13) & (uint64_t)(kRadix - kPieces)) : 0;
        double acc[V];
        uint32_t cnt[I];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < I; ++v) cnt[v] = 0u;
        auto finish_leaf = [&](int node) {  // the leaf's V sums and I counts into the stage; the running sums start again
            rs_steps<V, 0>(acc, lane);
            if (my >= 0) stage_s[node * V + my] = acc[0];
            uint32_t cv = 0;
#pragma unroll
            for (int v = 0; v < I; ++v) cv = lane == v ? cnt[v] : cv;
            if (lane < I) stage_c[node * I + lane] = cv;
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
            for (int v = 0; v < I; ++v) cnt[v] = 0u;
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
                pops_accumulate<Stat, NP>(acc, cnt, a, C::template pack<NP>(a.k, minind), lane);
                if (i + kPieces < kRadix) load_full(a, (j + kPieces) & (kRadix - 1));
                pops_accumulate<Stat, NP>(acc, cnt, b, C::template pack<NP>(b.k, minind), lane);
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
                    pops_accumulate<Stat, NP>(acc, cnt, s, C::template pack_padded<NP>(s.k, minind, valid), lane);
                }
                finish_leaf(q);
            }
        }
        // the level-2 node = the tile's leaf nodes added in LEAF order, whatever order they were produced in
        if (my >= 0) {
            double l2 = 0.0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) l2 += stage_s[q * V + my];
            sum_node<V>(tv, 1, t)[my] = l2;
            tot_s += l2;
        }
        if (lane < I) {
            uint32_t c2 = 0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) c2 += stage_c[q * I + lane];
            cnt_node<I>(tv, 1, t)[lane] = c2;
            tot_c += c2;
        }
        // the tile's 16 level-1 nodes: one contiguous block of 128 V bytes of sums and one of 64 I bytes of counts
        flush_stage<V * kRadix1>(sum_node<V>(tv, 0, t * kRadix1), stage_s, lane);
        flush_count_stage<I * kRadix1>(cnt_node<I>(tv, 0, t * kRadix1), stage_c, lane);
    }
    // one partial {sums, neff} per item and build wave: the genome-wide lines are their sums in wave order (fixed by the static
    // grid, a function of n alone); a wave without a tile leaves the identity
    if (my >= 0) reinterpret_cast<double *>(tv.base + tv.part_sum)[wave0 * V + my] = tot_s;
    if (lane < I) reinterpret_cast<uint32_t *>(tv.base + tv.part_cnt)[wave0 * I + lane] = tot_c;
}

// Two occupancies of the one body (as af_build_kernel / af_build_kernel_w1): two waves per SIMD with 256 registers each, or
// one with the whole file — from how many populations on the second is taken is the statistic's kOneWaveFrom.
template <class Stat, int NP>
__global__ __launch_bounds__(256, 2) void pops_build_kernel(PopCols cols, int minind, uint64_t n, uint64_t n_l2, PopsTree tv) {
    pops_build_body<Stat, NP>(cols, minind, n, n_l2, tv);
}
template <class Stat, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void pops_build_kernel_w1(PopCols cols, int minind, uint64_t n, uint64_t n_l2, PopsTree tv) {
    pops_build_body<Stat, NP>(cols, minind, n, n_l2, tv);
}

// ---- upper levels: parent = Σ of 64 children, per sum (blockIdx.y < S * items; the first `items` also carry the item's count)
// Templated on S alone: statistics that differ only in their per-site function share the kernel.
template <int S>
__global__ __launch_bounds__(256) void pops_up_kernel(PopsTree tv, int child_slot, uint64_t n_child, uint64_t n_parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int v = blockIdx.y, I = tv.n_items, V = S * I;
    const double *cs = reinterpret_cast<const double *>(tv.base + tv.sum_off[child_slot]);
    const uint32_t *cc = reinterpret_cast<const uint32_t *>(tv.base + tv.cnt_off[child_slot]);
    double *ps = reinterpret_cast<double *>(tv.base + tv.sum_off[child_slot + 1]);
    uint32_t *pc = reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[child_slot + 1]);
    for (uint64_t p = wave0; p < n_parent; p += n_waves) {
        const uint64_t i = p * kRadix + lane;
        double x = i < n_child ? cs[i * V + v] : 0.0;
        if constexpr (S == 1) {  // every value carries its count: both loads before the sums
            uint32_t c = i < n_child ? cc[i * I + v] : 0u;
            x = wave_sum(x);
            c = wave_sum(c);
            if (lane == 0) { ps[p * V + v] = x; pc[p * I + v] = c; }
        } else {
            x = wave_sum(x);
            if (lane == 0) ps[p * V + v] = x;
            if (v < I) {
                uint32_t c = i < n_child ? cc[i * I + v] : 0u;
                c = wave_sum(c);
                if (lane == 0) pc[p * I + v] = c;
            }
        }
    }
}

// ---- QUERY: one wave per window, all items at once; one more item for the genome-wide lines ------------------------------
// Ragged sites: a lane takes the QUAD of sites 4L .. 4L+3 of a 256-site stride that starts at a multiple of 4 (the columns
// are 16-byte aligned: one 16-byte load per count column, two per frequency column); sites of the quad outside [from, to)
// are not counted; the column's last quad, when n is not a multiple of 4, is read site by site.  A lane adds its items in an
// order that depends on the window alone: left sites, right sites, then per level the left and right ragged nodes.
// (two waves per SIMD below the statistic's kQueryOneWaveFrom: above, the running sums and a stride's columns need more than 256 registers)
template <class Stat, int NP>
__global__ __launch_bounds__(256, (NP >= Stat::kQueryOneWaveFrom ? 1 : 2)) void pops_query_kernel(PopCols cols, int minind, const uint32_t *__restrict__ pos, PopsTree tv,
                                                             const pgt_win *__restrict__ win, uint64_t n_win,
                                                             typename Stat::Row *__restrict__ out, typename Stat::Total *__restrict__ tot, uint64_t n_sites) {
    using C = typename Stat::Counts;
    constexpr int S = Stat::kSumsPerItem;
    constexpr int I = Stat::items(NP);
    constexpr int V = S * I;
    static_assert(S >= 1 && S <= 3, "the row epilogue names the sums of an item");
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_items = n_win + (tot ? 1 : 0);

    for (uint64_t w = wave0; w < n_items; w += n_waves) {
        double acc[V];      // per lane
        uint32_t ncnt[I];   // per lane: neff of the nodes this lane read
        uint32_t scnt[I];   // wave-uniform: neff of the ragged sites
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll
        for (int v = 0; v < I; ++v) { ncnt[v] = 0u; scnt[v] = 0u; }
        if (w == n_win) {  // the genome-wide lines: the build waves' partials, lane l adds partials l, l + 64, .. in turn
            const double *ps = reinterpret_cast<const double *>(tv.base + tv.part_sum);
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(tv.base + tv.part_cnt);
            for (uint32_t i = (uint32_t)lane; i < tv.n_partials; i += kWave) {
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += ps[(uint64_t)i * V + v];
#pragma unroll
                for (int v = 0; v < I; ++v) ncnt[v] += pc[(uint64_t)i * I + v];
            }
            double s[3] = {0.0, 0.0, 0.0};  // lane v < I keeps the wave's sums and count of item v, which it finishes
            uint32_t c = 0;
#pragma unroll
            for (int v = 0; v < I; ++v) {
                double x[3] = {0.0, 0.0, 0.0};
                x[0] = wave_sum(acc[v]);
                if constexpr (S > 1) x[1] = wave_sum(acc[I + v]);
                if constexpr (S > 2) x[2] = wave_sum(acc[2 * I + v]);
                const uint32_t cv = wave_sum(ncnt[v]);
                if (v == lane) { s[0] = x[0]; s[1] = x[1]; s[2] = x[2]; c = cv; }
            }
            if (lane < I) {
                typename Stat::Total r;
                Stat::finish_total(r, s, c, n_sites);
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
                const auto own = C::template pack<NP>(k, minind, in);
                double p[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].x;
                Stat::template site<NP>(acc, scnt, p, C::template view<NP, 0>(own));
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].y;
                Stat::template site<NP>(acc, scnt, p, C::template view<NP, 1>(own));
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].x;
                Stat::template site<NP>(acc, scnt, p, C::template view<NP, 2>(own));
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].y;
                Stat::template site<NP>(acc, scnt, p, C::template view<NP, 3>(own));
            }
        };
        auto add_node = [&](int slot, uint64_t i) {
            const double *ns = sum_node<V>(tv, slot, i);
            const uint32_t *nc = cnt_node<I>(tv, slot, i);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += ns[v];
#pragma unroll
            for (int v = 0; v < I; ++v) ncnt[v] += nc[v];
        };
        auto sum_nodes = [&](int level, uint64_t from, uint64_t to) {
            for (uint64_t i = from + lane; i < to; i += kWave) add_node(level - 1, i);
        };
        // the range descent: the same loop as in af_query_kernel, where its rule is explained (that kernel keeps its copy: as one
        // function shared between the two DIFFERENT kernels the compiler gave both other code; a change to one belongs in the other)
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
        double s[3] = {0.0, 0.0, 0.0};  // the selection of the genome-wide lines again (as a function of its own, or with a loop
        uint32_t c = 0;                 // over S, the compiler turned it into other code than the kernels had)
#pragma unroll
        for (int v = 0; v < I; ++v) {
            double x[3] = {0.0, 0.0, 0.0};
            x[0] = wave_sum(acc[v]);
            if constexpr (S > 1) x[1] = wave_sum(acc[I + v]);
            if constexpr (S > 2) x[2] = wave_sum(acc[2 * I + v]);
            const uint32_t cv = wave_sum(ncnt[v]) + scnt[v];
            if (v == lane) { s[0] = x[0]; s[1] = x[1]; s[2] = x[2]; c = cv; }
        }
        if (lane < I) {  // lane v finishes item v
            typename Stat::Row r;
            Stat::finish_row(r, start, end, hi - lo, s, c);
            out[(uint64_t)lane * n_win + w] = r;
        }
    }
}

}  // namespace dev

// ---- host side ---------------------------------------------------------------------------------------------------------
// populations from which the one-wave-per-SIMD build is taken (the statistic's knob: clamped to what fits the registers,
// 2 .. kOneWaveFrom)
template <class Stat>
int one_wave_from() {
    if constexpr (Stat::kOneWaveKnob == nullptr) {
        return Stat::kOneWaveFrom;
    } else {
        static const int v = env_int(Stat::kOneWaveKnob, Stat::kOneWaveFrom);
        return v < 2 ? 2 : (v > Stat::kOneWaveFrom ? Stat::kOneWaveFrom : v);
    }
}

template <class Stat, int NP>
constexpr size_t stage_bytes() { return (size_t)4 * dev::kRadix1 * Stat::items(NP) * dev::stage_item_bytes(Stat::kSumsPerItem); }

template <class Stat, int NP>
int launch_np(const dev::PopCols &cols, const uint32_t *pos, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
              typename Stat::Row *out, typename Stat::Total *tot, PopsTree tv, const TreeLayout &tl, hipStream_t s, const LaunchEnv &e) {
    std::string *err = e.err;
    if (int rc = record_event(e.ev_build0, s, err)) return rc;
    tv.n_partials = 0;
    if (n > 0) {
        const bool w1 = NP >= one_wave_from<Stat>();
        const auto [blocks, n_partials] = pops_build_grid(tl.count[1], w1);
        tv.n_partials = n_partials;
        constexpr size_t lds = stage_bytes<Stat, NP>();
        if constexpr (NP >= Stat::kOneWaveFrom || Stat::kOneWaveKnob != nullptr) {
            if (w1) hipLaunchKernelGGL((dev::pops_build_kernel_w1<Stat, NP>), dim3(blocks), dim3(256), lds, s, cols, minind, n, tl.count[1], tv);
        }
        if constexpr (NP < Stat::kOneWaveFrom) {
            if (!w1) hipLaunchKernelGGL((dev::pops_build_kernel<Stat, NP>), dim3(blocks), dim3(256), lds, s, cols, minind, n, tl.count[1], tv);
        }
        if (int rc = hip_fail(hipGetLastError(), Stat::kKernelNames[0], err)) return rc;
        if (int rc = launch_upper_levels(dev::pops_up_kernel<Stat::kSumsPerItem>, Stat::kKernelNames[1], Stat::kSumsPerItem * Stat::items(NP), tv, tl, s, err)) return rc;
    }
    if (int rc = record_event(e.ev_build1, s, err)) return rc;
    if (n_win > 0 || tot) {
        hipLaunchKernelGGL((dev::pops_query_kernel<Stat, NP>), dim3(wave_grid(n_win + (tot ? 1 : 0))), dim3(256), 0, s, cols, minind, pos, tv, win, n_win, out, tot, n);
        if (int rc = hip_fail(hipGetLastError(), Stat::kKernelNames[2], err)) return rc;
    }
    return record_event(e.ev_query1, s, err);
}

// every build kernel of the statistic may use its stage (called once from pgt_open through the statistic's init function, so
// that no attribute call can fall inside a caller's stream capture)
template <class Stat, int NP = Stat::kMinPops>
void allow_lds() {
    if constexpr (NP <= Stat::kMaxPops) {
        if constexpr (NP >= Stat::kOneWaveFrom || Stat::kOneWaveKnob != nullptr)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dev::pops_build_kernel_w1<Stat, NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<Stat, NP>());
        if constexpr (NP < Stat::kOneWaveFrom)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dev::pops_build_kernel<Stat, NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<Stat, NP>());
        allow_lds<Stat, NP + 1>();
    }
}

// The body of an entry point; kMinPops <= n_pops <= kMaxPops (and what else the statistic asks of minind): checked by the caller
template <class Stat>
int launch_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                int minind, const pgt_win *win, uint64_t n_win, typename Stat::Row *out, typename Stat::Total *tot, void *tree,
                const LaunchEnv &e) {
    hipStream_t s = static_cast<hipStream_t>(e.stream);
    const TreeLayout tl = tree_layout(PGT_STAT_FST, n);  // node counts of the f64 layout (levels 2 and up; level 1: a quarter)
    const PopsTree tv = pops_tree_view(tl, Stat::items((int)n_pops), Stat::kSumsPerItem, tree, useful_levels(tl, PGT_STAT_FST, e.hints.max_window));
    dev::PopCols cols{};
    for (uint32_t k = 0; k < n_pops; ++k) { cols.f[k] = freq[k]; cols.c[k] = nind[k]; }
    return dispatch_pops<Stat::kMinPops, Stat::kMaxPops>(n_pops, [&](auto np) {
        return launch_np<Stat, decltype(np)::value>(cols, pos, n, minind, win, n_win, out, tot, tv, tl, s, e);
    });
}

}  // namespace pgt
