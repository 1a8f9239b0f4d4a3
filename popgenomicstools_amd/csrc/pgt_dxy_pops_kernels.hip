// pgt_dxy_pops_kernels.hip — dxyWindow's window statistic for ALL pairs i < j of up to 8 populations in ONE pass over
// the populations' own columns (allele frequency f64 + individual count i32: 12 B/site/population, 96 B/site for 8
// populations) instead of one pass per pair over the pair's four columns (24 B/site/pair, 672 B/site for 28 pairs).
//
// Spec, per pair (i, j): dxyWindow.cpp:381 — a site is counted when nInd_i >= minind && nInd_j >= minind and then contributes
// d = p_i (1 - p_j) + p_j (1 - p_i); dxyWindow.cpp:172-209 — a window's row is Σd over its counted sites, neffective = their
// number, nskip = the others.  The predicate belongs to the PAIR (it does not factor into per-population sums), so every
// pair keeps its own {Σd, neff}; d is evaluated with exactly the roundings of the two-population path (dxy_site_pred in
// pgt_kernels.hip: no contraction, products and sums rounded one by one, as the host's SSE2 code does), so a one-site
// window carries the same bits.  nskip is not stored: every site of a window's range is a data site (the placeholders of
// the base-pair mode are not sites of the range), hence nskip = (hi - lo) - neff.  Domain: frequencies in [0, 1] (what the
// MAF ingest admits), where d >= +0.0 and "add d or +0.0" is bit for bit "add d or skip".
//
// Tree: as the allele-frequency front end (pgt_af_kernels.hip) — 512-site level-1 nodes, 16 per 8192-site level-2 node,
// radix 64 above; a level is two node-major arrays, P doubles and P u32 per node (pgt_internal.h: DxyPopsTree).
//
// The counts decide nothing but the predicate.  They are read by 16-byte loads in the layout of count_pair_pred
// (pgt_kernels.hip): lane L holds sites 4L .. 4L+3 of a PAIR of 128-site pieces.  Each lane packs "population k has enough
// individuals at site 4L+c" into bit 4k+c of ONE register (8 populations x 4 sites = 32 bits), and the lane that owns sites
// 2l, 2l+1 of piece h in the frequency layout fetches that register from lane 32h + (l >> 1) — one ds_bpermute per piece
// for all populations.  The per-population bits become lane masks (v_cmp into a scalar register pair), a pair's predicate
// is the AND of two of them (scalar), its neff the popcount of that AND (scalar, wave-uniform: no vector registers, no
// cross-lane reduction), and the same mask selects d or +0.0 for the pair's sum.
//
// pgt_set_window_step is ignored by this entry point: every table is answered by the one-wave-per-window query.
#include <hip/hip_runtime.h>

#include "pgt_device.h"
#include "pgt_internal.h"
#include "pgt_pops_common.h"

namespace pgt {
namespace {

using namespace dev;

constexpr int kPieces = kPopsLeafPieces;   // 128-site pieces per level-1 node
constexpr int kLeaf = kPieces * kLeafF64;     // sites per level-1 node (512: the level-1 bytes written are 12 P / 512 per site, 0.7 % of the bytes read at 8 populations; see pgt_af_kernels.hip on what node stores cost)
constexpr int kRadix1 = kRadix / kPieces;     // level-1 nodes per level-2 node
static_assert(kPieces == 4, "the build walks a leaf as two pairs of pieces");

template <int NP>
struct Shape {
    static constexpr int kPairs = pair_count(NP);  // lexicographic (i < j): (0,1),(0,2),..,(0,NP-1),(1,2),..
};

struct PopCols {
    const double *f[kPopsMaxPops];
    const int32_t *c[kPopsMaxPops];
};

// (the reduce-scatter of a leaf's P sums across the wave: rs_steps / rs_my_index of pgt_pops_common.h)

// ---- per-site contribution ---------------------------------------------------------------------------------------------
// One site of this lane into the lane's P running sums and the wave's P counters.  okbits: bit 4k = population k has at
// least minind individuals at this site.  MUST be called by all 64 lanes together (the counters are popcounts of ballots).
// d: exactly dxy_site_pred of pgt_kernels.hip (dxyWindow.cpp:381) with p1 = p_i, p2 = p_j.
template <int NP>
__device__ __forceinline__ void dxy_pops_site(double *acc, uint32_t *cnt, const double *p, uint32_t okbits) {
    double om[NP];
    bool ok[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        om[k] = __dsub_rn(1.0, p[k]);
        ok[k] = ((okbits >> (4 * k)) & 1u) != 0;
    }
    int v = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int j = i + 1; j < NP; ++j) {
            const bool counted = ok[i] && ok[j];
            const double d = __dadd_rn(__dmul_rn(p[i], om[j]), __dmul_rn(p[j], om[i]));
            acc[v] = __dadd_rn(acc[v], counted ? d : 0.0);
            cnt[v] += (uint32_t)__popcll(__ballot(counted));
            ++v;
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
__device__ __forceinline__ void dxy_pops_accumulate(double *acc, uint32_t *cnt, const PieceSet<NP> &s, uint32_t okb, int lane) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // the bits of this lane's sites 2l, 2l+1 of piece h = pair sites 128h + 2l + q: count lane 32h + (l >> 1), component 2(l & 1) + q
        const uint32_t w = (uint32_t)__shfl((int)okb, 32 * h + (lane >> 1), kWave) >> (2 * (lane & 1));
        double px[NP], py[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) { px[k] = s.f[h][k].x; py[k] = s.f[h][k].y; }
        dxy_pops_site<NP>(acc, cnt, px, w);
        dxy_pops_site<NP>(acc, cnt, py, w >> 1);
    }
}

template <int NP>
__device__ __forceinline__ double *sum_node(const DxyPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<double *>(tv.base + tv.sum_off[slot]) + i * Shape<NP>::kPairs;
}
template <int NP>
__device__ __forceinline__ uint32_t *cnt_node(const DxyPopsTree &tv, int slot, uint64_t i) {
    return reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[slot]) + i * Shape<NP>::kPairs;
}

// ---- BUILD: one wave per level-2 tile (64 pieces of 128 sites = 16 leaf nodes of 512 sites) -----------------------------
// The walk of pgt_af_kernels.hip (piece by piece over all populations, software-pipelined over two register sets that swap
// roles; the tile walked from a piece of the wave's own; the tile's level-1 nodes staged in LDS and written as one
// contiguous block of nt stores), with a PAIR of pieces as the unit, because a 16-byte count load spans two pieces.
// A leaf's sums do not depend on the wave or on where its walk started: a lane adds its 8 sites of the leaf in site order,
// the reduce-scatter is a fixed tree, and the level-2 node adds the 16 leaf nodes in leaf order.
template <int NP>
__device__ __forceinline__ void dxy_pops_build_body(const PopCols &cols, int minind, uint64_t n, uint64_t n_l2, const DxyPopsTree &tv) {
    constexpr int P = Shape<NP>::kPairs;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int my = rs_my_index<P>(lane);
    const uint32_t lane_bytes = (uint32_t)lane * 16u;
    constexpr uint64_t kTile2 = (uint64_t)kLeafF64 * kRadix;
    // the wave's LDS stage: 16 nodes x P doubles, then 16 nodes x P u32 (private to the wave: no barrier)
    extern __shared__ __attribute__((aligned(16))) char dxy_pops_stage[];
    char *stage = dxy_pops_stage + (size_t)(threadIdx.x >> 6) * (kRadix1 * P * 12);
    double *stage_s = reinterpret_cast<double *>(stage);
    uint32_t *stage_c = reinterpret_cast<uint32_t *>(stage + kRadix1 * P * 8);

    double tot_s = 0.0;   // lane `my`: Σ of the level-2 nodes this wave wrote, in tile order (the genome-wide line's partial)
    uint32_t tot_c = 0;   // lane p < P: their neff

    for (uint64_t t = wave0; t < n_l2; t += n_waves) {
        const uint64_t base = t * kTile2;
        const bool full = base + kTile2 <= n;
        // a multiple of the leaf's pieces below 64 (see tile_rotation in pgt_kernels.hip); the partial last tile is walked from its start
        const int rot = full ? (int)(((wave0 * 0x9E3779B1ull) >> 13) & (uint64_t)(kRadix - kPieces)) : 0;
        double acc[P];
        uint32_t cnt[P];
#pragma unroll
        for (int v = 0; v < P; ++v) { acc[v] = 0.0; cnt[v] = 0u; }
        auto finish_leaf = [&](int node) {  // the leaf's P sums and counts into the stage; the running sums start again
            rs_steps<P, 0>(acc, lane);
            if (my >= 0) stage_s[node * P + my] = acc[0];
            uint32_t cv = 0;
#pragma unroll
            for (int v = 0; v < P; ++v) cv = lane == v ? cnt[v] : cv;
            if (lane < P) stage_c[node * P + lane] = cv;
#pragma unroll
            for (int v = 0; v < P; ++v) { acc[v] = 0.0; cnt[v] = 0u; }
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
                dxy_pops_accumulate<NP>(acc, cnt, a, pop_ok_bits<NP>(a.k, minind), lane);
                if (i + kPieces < kRadix) load_full(a, (j + kPieces) & (kRadix - 1));
                dxy_pops_accumulate<NP>(acc, cnt, b, pop_ok_bits<NP>(b.k, minind), lane);
                finish_leaf(j / kPieces);
            }
        } else {  // the last, partial tile (one wave, once): guarded loads; a site beyond n is never counted
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
                    dxy_pops_accumulate<NP>(acc, cnt, s, pop_ok_bits<NP>(s.k, minind) & (valid * 0x11111111u), lane);
                }
                finish_leaf(q);
            }
        }
        // the level-2 node = the tile's leaf nodes added in LEAF order, whatever order they were produced in
        if (my >= 0) {
            double l2 = 0.0;
#pragma unroll 8
            for (int q = 0; q < kRadix1; ++q) l2 += stage_s[q * P + my];
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
        // the tile's 16 level-1 nodes: one contiguous block of 128 P bytes of sums and one of 64 P bytes of counts
        flush_stage<P * kRadix1>(sum_node<NP>(tv, 0, t * kRadix1), stage_s, lane);
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
    // one partial {Σd, neff} per pair and build wave: the genome-wide lines are their sums in wave order (fixed by the static
    // grid, a function of n alone); a wave without a tile leaves the identity
    if (my >= 0) reinterpret_cast<double *>(tv.base + tv.part_sum)[wave0 * P + my] = tot_s;
    if (lane < P) reinterpret_cast<uint32_t *>(tv.base + tv.part_cnt)[wave0 * P + lane] = tot_c;
}

// Two occupancies of the one body (as af_build_kernel / af_build_kernel_w1): two waves per SIMD with 256 registers each, or
// one with the whole file — from how many populations on the second is taken is decided in launch_np.
template <int NP>
__global__ __launch_bounds__(256, 2) void dxy_pops_build_kernel(PopCols cols, int minind, uint64_t n, uint64_t n_l2, DxyPopsTree tv) {
    dxy_pops_build_body<NP>(cols, minind, n, n_l2, tv);
}
template <int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void dxy_pops_build_kernel_w1(PopCols cols, int minind, uint64_t n, uint64_t n_l2, DxyPopsTree tv) {
    dxy_pops_build_body<NP>(cols, minind, n, n_l2, tv);
}
constexpr int kOneWaveFrom = 5;  // populations from which the two-waves-per-SIMD build would not fit its registers

// ---- upper levels: parent = Σ of 64 children, per pair (blockIdx.y) -------------------------------------------------------
__global__ __launch_bounds__(256) void dxy_pops_up_kernel(DxyPopsTree tv, int child_slot, uint64_t n_child, uint64_t n_parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const int v = blockIdx.y, P = tv.n_pairs;
    const double *cs = reinterpret_cast<const double *>(tv.base + tv.sum_off[child_slot]);
    const uint32_t *cc = reinterpret_cast<const uint32_t *>(tv.base + tv.cnt_off[child_slot]);
    double *ps = reinterpret_cast<double *>(tv.base + tv.sum_off[child_slot + 1]);
    uint32_t *pc = reinterpret_cast<uint32_t *>(tv.base + tv.cnt_off[child_slot + 1]);
    for (uint64_t p = wave0; p < n_parent; p += n_waves) {
        const uint64_t i = p * kRadix + lane;
        double x = i < n_child ? cs[i * P + v] : 0.0;
        uint32_t c = i < n_child ? cc[i * P + v] : 0u;
        x = wave_sum(x);
        c = wave_sum(c);
        if (lane == 0) { ps[p * P + v] = x; pc[p * P + v] = c; }
    }
}

// ---- QUERY: one wave per window, all pairs at once; one more item for the genome-wide lines ------------------------------
// Ragged sites: a lane takes the QUAD of sites 4L .. 4L+3 of a 256-site stride that starts at a multiple of 4 (the columns
// are 16-byte aligned: one 16-byte load per count column, two per frequency column); sites of the quad outside [from, to)
// are not counted; the column's last quad, when n is not a multiple of 4, is read site by site.  A lane adds its items in an
// order that depends on the window alone: left sites, right sites, then per level the left and right ragged nodes.
// (two waves per SIMD; with 7 and 8 populations the 2 x 21 / 2 x 28 running sums and a stride's columns need more than 256 registers)
template <int NP>
__global__ __launch_bounds__(256, (NP >= 7 ? 1 : 2)) void dxy_pops_query_kernel(PopCols cols, int minind, const uint32_t *__restrict__ pos, DxyPopsTree tv,
                                                             const pgt_win *__restrict__ win, uint64_t n_win,
                                                             pgt_dxy_row *__restrict__ out, pgt_dxy_total *__restrict__ tot, uint64_t n_sites) {
    constexpr int P = Shape<NP>::kPairs;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_items = n_win + (tot ? 1 : 0);

    for (uint64_t w = wave0; w < n_items; w += n_waves) {
        double acc[P];      // per lane
        uint32_t ncnt[P];   // per lane: neff of the nodes this lane read
        uint32_t scnt[P];   // wave-uniform: neff of the ragged sites
#pragma unroll
        for (int v = 0; v < P; ++v) { acc[v] = 0.0; ncnt[v] = 0u; scnt[v] = 0u; }
        if (w == n_win) {  // the genome-wide lines: the build waves' partials, lane l adds partials l, l + 64, .. in turn
            const double *ps = reinterpret_cast<const double *>(tv.base + tv.part_sum);
            const uint32_t *pc = reinterpret_cast<const uint32_t *>(tv.base + tv.part_cnt);
            for (uint32_t i = (uint32_t)lane; i < tv.n_partials; i += kWave) {
#pragma unroll
                for (int v = 0; v < P; ++v) { acc[v] += ps[(uint64_t)i * P + v]; ncnt[v] += pc[(uint64_t)i * P + v]; }
            }
            double s = 0.0;
            uint32_t c = 0;
#pragma unroll
            for (int v = 0; v < P; ++v) {
                const double sv = wave_sum(acc[v]);
                const uint32_t cv = wave_sum(ncnt[v]);
                if (v == lane) { s = sv; c = cv; }
            }
            if (lane < P) {
                pgt_dxy_total r;
                r.sum = s + 0.0;
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
                uint32_t in = 0;  // bit e: site i + e lies in [from, to)
#pragma unroll
                for (int e = 0; e < 4; ++e) in |= (i + e >= from && i + e < to ? 1u : 0u) << e;
                const uint32_t okb = pop_ok_bits<NP>(k, minind) & (in * 0x11111111u);
                double p[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].x;
                dxy_pops_site<NP>(acc, scnt, p, okb);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f0[q].y;
                dxy_pops_site<NP>(acc, scnt, p, okb >> 1);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].x;
                dxy_pops_site<NP>(acc, scnt, p, okb >> 2);
#pragma unroll
                for (int q = 0; q < NP; ++q) p[q] = f1[q].y;
                dxy_pops_site<NP>(acc, scnt, p, okb >> 3);
            }
        };
        auto add_node = [&](int slot, uint64_t i) {
            const double *s = sum_node<NP>(tv, slot, i);
            const uint32_t *c = cnt_node<NP>(tv, slot, i);
#pragma unroll
            for (int v = 0; v < P; ++v) { acc[v] += s[v]; ncnt[v] += c[v]; }
        };
        auto sum_nodes = [&](int level, uint64_t from, uint64_t to) {
            for (uint64_t i = from + lane; i < to; i += kWave) add_node(level - 1, i);
        };
        // the range descent: the same loop as in af_query_kernel, where its rule is explained (each kernel keeps its copy: as one
        // shared function the compiler gave both kernels other code; a change to one belongs in the other too)
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
        double s = 0.0;
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < P; ++v) {
            const double sv = wave_sum(acc[v]);
            const uint32_t cv = wave_sum(ncnt[v]) + scnt[v];
            if (v == lane) { s = sv; c = cv; }
        }
        if (lane < P) {  // lane p finishes pair p
            pgt_dxy_row r;
            r.start = start;
            r.end = end;
            r.neff = c;
            r.nskip = (uint32_t)(hi - lo) - c;  // dxyWindow.cpp:179-186: every site of the range is counted or skipped
            r.sum = s + 0.0;
            out[(uint64_t)lane * n_win + w] = r;
        }
    }
}

// populations from which the one-wave-per-SIMD build is taken (PGT_DXY_POPS_ONE_WAVE_FROM: a measuring knob, clamped to
// what fits the registers: 2 .. kOneWaveFrom)
inline int one_wave_from() {
    static const int v = env_int("PGT_DXY_POPS_ONE_WAVE_FROM", kOneWaveFrom);
    return v < 2 ? 2 : (v > kOneWaveFrom ? kOneWaveFrom : v);
}

template <int NP>
constexpr size_t stage_bytes() { return (size_t)4 * kRadix1 * Shape<NP>::kPairs * 12; }

template <int NP>
int launch_np(const PopCols &cols, const uint32_t *pos, uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
              pgt_dxy_row *out, pgt_dxy_total *tot, DxyPopsTree tv, const TreeLayout &tl, hipStream_t s, void *ev_b0,
              void *ev_b1, void *ev_q1, std::string *err) {
    if (int rc = record_event(ev_b0, s, err)) return rc;
    tv.n_partials = 0;
    if (n > 0) {
        const bool w1 = NP >= one_wave_from();
        const auto [blocks, n_partials] = pops_build_grid(tl.count[1], w1);
        tv.n_partials = n_partials;
        if constexpr (NP < kOneWaveFrom) {
            if (w1)
                hipLaunchKernelGGL((dxy_pops_build_kernel_w1<NP>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
            else
                hipLaunchKernelGGL((dxy_pops_build_kernel<NP>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        } else {  // (one_wave_from() <= kOneWaveFrom: always the one-wave form here)
            hipLaunchKernelGGL((dxy_pops_build_kernel_w1<NP>), dim3(blocks), dim3(256), stage_bytes<NP>(), s, cols, minind, n, tl.count[1], tv);
        }
        if (int rc = hip_fail(hipGetLastError(), "dxy_pops_build_kernel", err)) return rc;
        if (int rc = launch_upper_levels(dxy_pops_up_kernel, "dxy_pops_up_kernel", Shape<NP>::kPairs, tv, tl, s, err)) return rc;
    }
    if (int rc = record_event(ev_b1, s, err)) return rc;
    if (n_win > 0 || tot) {
        hipLaunchKernelGGL((dxy_pops_query_kernel<NP>), dim3(wave_grid(n_win + (tot ? 1 : 0))), dim3(256), 0, s, cols, minind, pos, tv, win, n_win, out, tot, n);
        if (int rc = hip_fail(hipGetLastError(), "dxy_pops_query_kernel", err)) return rc;
    }
    return record_event(ev_q1, s, err);
}

template <int NP>
void allow_lds() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dxy_pops_build_kernel_w1<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
    if constexpr (NP < kOneWaveFrom)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(dxy_pops_build_kernel<NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_bytes<NP>());
}

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_dxy_pops_kernels(std::string *err) {
    allow_lds<2>(); allow_lds<3>(); allow_lds<4>(); allow_lds<5>(); allow_lds<6>(); allow_lds<7>(); allow_lds<8>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

int launch_dxy_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                    int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot, void *tree,
                    void *stream, void *ev_build0, void *ev_build1, void *ev_query1, std::string *err, const Hints &hints) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 2 <= n_pops <= 8: checked by the caller
    const TreeLayout tl = tree_layout(PGT_STAT_FST, n);  // node counts of the f64 layout (levels 2 and up; level 1: a quarter)
    const DxyPopsTree tv = dxy_pops_tree_view(tl, (int)(n_pops * (n_pops - 1) / 2), tree, useful_levels(tl, PGT_STAT_FST, hints.max_window));
    PopCols cols{};
    for (uint32_t k = 0; k < n_pops; ++k) { cols.f[k] = freq[k]; cols.c[k] = nind[k]; }
    return dispatch_n_pops(n_pops, [&](auto np) {
        return launch_np<decltype(np)::value>(cols, pos, n, minind, win, n_win, out, tot, tv, tl, s, ev_build0, ev_build1, ev_query1, err);
    });
}

}  // namespace pgt
