// pgt_pops_common.h — what the "all pairs of up to 8 populations in one pass" front ends share (pgt_af_kernels.hip: FST from
// allele frequencies; pgt_pops_walk.h: the one walk of the (freq, nInd) front ends pgt_dxy_pops_kernels.hip,
// pgt_fst_pops_kernels.hip and pgt_dstat_pops_kernels.hip): the pair count, the wave reduce-scatter, the flushes of a build
// wave's LDS stage, and the host side of a launch (error mapping, event records, grids, the upper-level loop, the dispatch on
// the population count, the measuring knobs).  The static balanced build grid of the (freq, nInd) front ends is
// pops_build_grid below; the layout of their trees is pops_tree_view in pgt_internal.h (the C ABI sizes workspaces with it).
// pgt_kernels.hip keeps helpers of its own: it does not include this header.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <type_traits>

#include "pgt_device.h"
#include "pgt_internal.h"

namespace pgt {
namespace dev {

// ---- pairs of populations --------------------------------------------------------------------------
constexpr int pair_count(int np) { return np * (np - 1) / 2; }
// The pairs i < j are numbered in lexicographic order, (0,1),(0,2),..,(0,NP-1),(1,2),..: the order of the pair values inside a
// tree node, of the lanes that finish a window's rows and of the row tables (`for i: for j > i: ++p` wherever pairs are walked).

// ---- reduce-scatter across the wave ----------------------------------------------------------------
// V sums per leaf node would be V six-step butterflies; a reduce-scatter halves the live values at every exchange step
// (18+9+5+3+2+1 = 38 exchanges for 36 values), leaving each total in exactly one lane.
// Step order: the steps with the MOST exchanges (18 and 9 of the 38 at 8 populations) pair lanes across the wave halves and
// across 16-lane rows, where gfx950 has an instruction made for exactly this exchange: v_permlane32_swap / v_permlane16_swap
// swap the upper lanes of one register with the lower lanes of another, so that "keep one half of my values, receive the
// other half of my partner's" is two swaps (low and high dword) and ONE addition — no select, no LDS crossbar.  Until round
// 6 these two steps came last (xor 16 by ds_swizzle, xor 32 by ds_bpermute) and the 27 busiest exchanges cost 4 v_cndmask +
// 2 DPP moves + 1 add each (profiles/r06/af8_issue_stall.md: 29 % of the wave cycles were instruction-issue waits, the
// kernel ran 2 waves per SIMD at 228 VGPRs).  The remaining steps (5 + 3 + 2 + 1 exchanges) stay on DPP / ds_swizzle.
constexpr int kRsMask[6] = {32, 16, 1, 2, 8, 4};
template <int STEP>
__device__ __forceinline__ double xchg(double v) {
    static_assert(STEP >= 2, "steps 0 and 1 are swaps (rs_swap)");
    int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (STEP == 2) {         // xor 1: quad_perm [1,0,3,2]
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xF, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xF, 0xF, false);
    } else if constexpr (STEP == 3) {  // xor 2: quad_perm [2,3,0,1]
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xF, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xF, 0xF, false);
    } else if constexpr (STEP == 4) {  // xor 8: row_ror:8 inside the 16-lane row
        lo = __builtin_amdgcn_update_dpp(lo, lo, 0x128, 0xF, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(hi, hi, 0x128, 0xF, 0xF, false);
    } else {                           // xor 4: ds_swizzle bit mode (and 0x1f, or 0, xor 4)
        lo = __builtin_amdgcn_ds_swizzle(lo, 0x101F);
        hi = __builtin_amdgcn_ds_swizzle(hi, 0x101F);
    }
    return __hiloint2double(hi, lo);
}

// lower lanes (mask bit clear) keep `a` and receive the partner's `a`; upper lanes keep `b` and receive the partner's `b`:
// after the swaps register A holds {own a | partner's b} and B {partner's a | own b}, so A + B is the exchange's result
// in every lane (an addition is commutative bit for bit: own + received = received + own).
template <int STEP>
__device__ __forceinline__ double rs_swap(double a, double b) {
    const int alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
    if constexpr (STEP == 0) {
        const auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        return __hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]);
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        return __hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]);
    }
}

// One reduce-scatter step: C live values -> (C+1)/2.  A lane whose mask bit is set keeps the upper
// half and sends the lower half, its partner does the opposite; an odd C is padded with 0.
template <int C, int STEP>
__device__ __forceinline__ void rs_steps(double *v, int lane) {
    if constexpr (STEP < 6) {
        constexpr int H = (C + 1) / 2;
        if constexpr (STEP < 2) {
#pragma unroll
            for (int k = 0; k < H; ++k) v[k] = rs_swap<STEP>(v[k], (k + H < C) ? v[k + H] : 0.0);
        } else {
            const bool up = (lane & kRsMask[STEP]) != 0;
#pragma unroll
            for (int k = 0; k < H; ++k) {
                const double lo_v = v[k];
                const double hi_v = (k + H < C) ? v[k + H] : 0.0;
                const double keep = up ? hi_v : lo_v;
                const double send = up ? lo_v : hi_v;
                v[k] = keep + xchg<STEP>(send);
            }
        }
        rs_steps<H, STEP + 1>(v, lane);
    }
}

// Which of the V values ends up in this lane (-1: a padding slot)
template <int V>
__device__ __forceinline__ int rs_my_index(int lane) {
    int base = 0, real = V, c = V;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int H = (c + 1) / 2;
        if (lane & kRsMask[s]) { base += H; real = real > H ? real - H : 0; }
        else real = real < H ? real : H;
        c = H;
    }
    return real >= 1 ? base : -1;
}

// ---- BUILD: the flush of a wave's LDS stage --------------------------------------------------------
// N doubles (even; stage and destination 16-byte aligned) leave as ONE contiguous block of non-temporal 16-byte stores,
// 1 KiB per wave store.  The stage belongs to the wave alone and LDS operations of a wave complete in order: no barrier.
template <int N>
__device__ __forceinline__ void flush_stage(double *node_block, const double *stage, int lane) {
    static_assert(N % 2 == 0, "whole 16-byte elements");
    double2 *dst = reinterpret_cast<double2 *>(node_block);
    const double2 *src = reinterpret_cast<const double2 *>(stage);
#pragma unroll 4
    for (int e = lane; e < N / 2; e += kWave) {
        const double2 w = src[e];
        __builtin_nontemporal_store(w.x, &dst[e].x);
        __builtin_nontemporal_store(w.y, &dst[e].y);
    }
}
// N u32 (a multiple of 4; stage and destination 16-byte aligned): the counts beside those sums, 16 bytes per lane and store
template <int N>
__device__ __forceinline__ void flush_count_stage(uint32_t *node_block, const uint32_t *stage, int lane) {
    static_assert(N % 4 == 0, "whole 16-byte elements");
    uint4 *dst = reinterpret_cast<uint4 *>(node_block);
    const uint4 *src = reinterpret_cast<const uint4 *>(stage);
#pragma unroll 2
    for (int e = lane; e < N / 4; e += kWave) {
        const uint4 w = src[e];
        __builtin_nontemporal_store(w.x, &dst[e].x);
        __builtin_nontemporal_store(w.y, &dst[e].y);
        __builtin_nontemporal_store(w.z, &dst[e].z);
        __builtin_nontemporal_store(w.w, &dst[e].w);
    }
}

// ---- the population branch statistic from six sums ------------------------------------------------
// One text for the rows of pgt_pbs_pops_kernels.hip and for the block jackknife of those rows (pgt_dstat_jack_kernels.hip), so
// that both carry the same bits for the same sums.
// T = -log(1 - fst), fst = den != 0 ? num / den : 0 (fstWindow.cpp:85): a negative fst gives a negative T, fst == 1 gives +inf
__device__ __forceinline__ double branch(double num, double den) {
    const double fst = den != 0.0 ? __ddiv_rn(num, den) : 0.0;
    return -log(__dsub_rn(1.0, fst));
}
// the three branch statistics from the six sums (inf - inf is NaN: the IEEE results stand)
__device__ __forceinline__ void pbs_of(const double *num, const double *den, double &pbs_i, double &pbs_j, double &pbs_k) {
    const double t_ij = branch(num[0], den[0]), t_ik = branch(num[1], den[1]), t_jk = branch(num[2], den[2]);
    pbs_i = __dadd_rn(__dmul_rn(__dsub_rn(__dadd_rn(t_ij, t_ik), t_jk), 0.5), 0.0);
    pbs_j = __dadd_rn(__dmul_rn(__dsub_rn(__dadd_rn(t_ij, t_jk), t_ik), 0.5), 0.0);
    pbs_k = __dadd_rn(__dmul_rn(__dsub_rn(__dadd_rn(t_ik, t_jk), t_ij), 0.5), 0.0);
}

}  // namespace dev

// ---- host side of a launch -------------------------------------------------------------------------
inline int hip_fail(hipError_t e, const char *what, std::string *err) {
    if (e == hipSuccess) return PGT_OK;
    if (err) *err = std::string(what) + ": " + hipGetErrorString(e);
    return PGT_EDEVICE;
}

// ev: a hipEvent_t as void*, or NULL (the phase is not timed)
inline int record_event(void *ev, hipStream_t s, std::string *err) {
    return ev ? hip_fail(hipEventRecord(static_cast<hipEvent_t>(ev), s), "hipEventRecord", err) : PGT_OK;
}

// workgroups of 4 waves for kernels that give one wave an item at a time (a parent node, a window) by a grid stride
inline unsigned wave_grid(uint64_t items) {
    const uint64_t b = (items + 3) / 4;
    return (unsigned)(b > 65536 ? 65536 : b);
}

// The build grid of the (freq, nInd) front ends (launch_np of pgt_pops_walk.h) over
// `n_tiles` level-2 tiles (tl.count[1] > 0): a static balanced grid of what is resident at once (one wave per SIMD: 256
// workgroups of 4 waves; two: 512): every wave walks `rounds` tiles, all waves run in near lockstep and flush their node
// blocks at about the same times.  (launch_af_np picks its round count by how full the last generation is; that choice is
// unmeasured here, and the per-wave partials want a grid that depends on n alone.)  n_partials = the waves of the grid, one
// partial each: <= kMaxBuildWaves, what the workspace reserves.
struct PopsBuildGrid {
    unsigned blocks;
    uint32_t n_partials;
};
inline PopsBuildGrid pops_build_grid(uint64_t n_tiles, bool one_wave_per_simd) {
    const uint64_t max_waves = one_wave_per_simd ? 1024 : (uint64_t)kMaxBuildWaves;
    const uint64_t rounds = (n_tiles + max_waves - 1) / max_waves;
    const uint64_t waves = (n_tiles + rounds - 1) / rounds;
    const uint64_t blocks = (waves + 3) / 4;
    return {(unsigned)blocks, (uint32_t)(blocks * 4)};
}

// levels 3 and up, one launch each: parent = Σ of 64 children, per value of a node (blockIdx.y < n_vals)
template <class Tree>
int launch_upper_levels(void (*up)(Tree, int, uint64_t, uint64_t), const char *name, int n_vals, const Tree &tv,
                        const TreeLayout &tl, hipStream_t s, std::string *err) {
    for (int k = 2; k < tv.n_levels; ++k) {
        hipLaunchKernelGGL(up, dim3(wave_grid(tl.count[k]), (unsigned)n_vals), dim3(256), 0, s, tv, k - 1, tl.count[k - 1], tl.count[k]);
        if (int rc = hip_fail(hipGetLastError(), name, err)) return rc;
    }
    return PGT_OK;
}

// f(std::integral_constant<int, NP>{}) for the NP = n_pops in LO .. HI, and only those are instantiated; the callers reject
// any other count before they get here
template <int LO, int HI, class F>
int dispatch_pops(uint32_t n_pops, const F &f) {
    if constexpr (LO > HI) return PGT_EARG;
    else return n_pops == LO ? f(std::integral_constant<int, LO>{}) : dispatch_pops<LO + 1, HI>(n_pops, f);
}
template <class F>
int dispatch_n_pops(uint32_t n_pops, const F &f) { return dispatch_pops<2, 8>(n_pops, f); }

// a measuring knob from the environment (read once by its caller: `static const int v = env_int(..)`)
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

}  // namespace pgt
