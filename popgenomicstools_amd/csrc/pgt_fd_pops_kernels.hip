// pgt_fd_pops_kernels.hip — f_d (Martin, Davey & Jiggins 2015) and f_dM (Malinsky et al. 2015) of ALL trios i < j < k of the
// ingroup populations against one outgroup: the statistics to scan windows with where Patterson's D misleads.  Input, predicate,
// trio order and walk are those of pgt_dstat_pops_kernels.hip (4 ... 7 populations' own MAF columns, 12 B/site/population, ONE pass).
//
// Spec (include/pgtwin.h, pgt_fd_pops_reduce_dev): trio (i, j, k) is read as ((P1 = i, P2 = j), P3 = k), o = NP-1 the outgroup;
// a counted site contributes, with p_x the frequency and q_x = 1 - p_x, every operation rounded on its own:
//     num  = abba - baba                                 (abba, baba: the two lines of pgt_dstat_pops_reduce_dev)
//     H = (p_j >= p_k) ? j : k        L = (p_j <= p_k) ? j : k        G = (p_i >= p_k) ? i : k        S = (p_i <= p_k) ? i : k
//     B1 = (q_i*p_H)*(p_H*q_o) - (p_i*q_H)*(p_H*q_o)      A1 = (p_i*q_L)*(q_L*p_o) - (q_i*p_L)*(q_L*p_o)
//     B2 = (p_G*q_j)*(p_G*q_o) - (q_G*p_j)*(p_G*q_o)      A2 = (q_S*p_j)*(q_S*p_o) - (p_S*q_j)*(q_S*p_o)
//     fd_den  = B1 + A1
//     fdm_den = (p_j >= p_i ? B1 : B2) + (p_j <= p_i ? A1 : A2)
// Every one of the eight candidate terms is "the two products of an ingroup PAIR (a, b), each times one product of (x, o),
// subtracted", so a site shares them as the D kernel shares its products: per ingroup population x the two products p_x*q_o
// and q_x*p_o, per ingroup pair a < b the two products q_a*p_b and p_a*q_b and from them
//     hi_b = (q_a*p_b)*(p_b*q_o) - (p_a*q_b)*(p_b*q_o)     B1 with H = b of trios (a, b, .) and (a, ., b); B2 with G = b of (., a, b)
//     lo_b = (p_a*q_b)*(q_b*p_o) - (q_a*p_b)*(q_b*p_o)     A1 with L = b of the same trios;               A2 with S = b of (., a, b)
//     hi_a = (p_a*q_b)*(p_a*q_o) - (q_a*p_b)*(p_a*q_o)     B2 with G = a of trios (a, b, .)
//     lo_a = (q_a*p_b)*(q_a*p_o) - (p_a*q_b)*(q_a*p_o)     A2 with S = a of trios (a, b, .)
// (products commute bit for bit, so (p_k*q_j) of B2 with G = k is q_j*p_k of the pair (j, k)).  A trio then takes two pairs of
// products for abba and baba, one subtraction, six selects ON THE RESULTS (the same bits as selects on the operands: both
// candidates are the definition's line for their choice) and two additions.
//
// The loops below are written trio by trio (i, then j, then k), every value named where it is used.  Up to 6 populations the
// compiler sees equal expressions and shares them: each pair's products and terms once per site.  At 7 populations that sharing
// keeps 15 pairs' terms alive beside the walk's 60 running sums and two register sets, more than a wave's 512 registers
// (profiles/r15/fd_pops.md), so there the frequencies pass through fresh() once per i and once per (i, j): the same bits under a
// new name, from which a pair's products and terms are computed AGAIN where they are used instead of being kept (10 + 10 pairs
// a site more), and sites are kept apart in the schedule.  The results do not depend on it, bit for bit.
//
// Tree, build walk and query: pgt_pops_walk.h, with three sums per TRIO: a node is 3 T doubles (num of trio 0 .. T-1, then
// fd_den, then fdm_den) and T u32, T = C(NP-1, 3) = 1 / 4 / 10 / 20: the node, the stage and the tree size of the D kernel.
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct FdPops {
    static constexpr int kMinPops = 4, kMaxPops = 7;  // three ingroup populations and an outgroup; 20 trios at most
    static constexpr int items(int np) { return trio_count(np); }  // lexicographic (i < j < k < NP-1), as DstatPops
    static constexpr int kSumsPerItem = 3;                         // Σnum of every trio, then Σfd_den of every trio, then Σfdm_den
    // populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r15/fd_pops.md) shows
    // the two-wave build at 196 registers with 4 populations and spilling from 5 on, the one-wave build without scratch at
    // every count (at 7 only with kRecompute); the query needs more than 256 registers from 6 populations on
    static constexpr int kOneWaveFrom = 5;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 6;
    static constexpr const char *kKernelNames[3] = {"fd_pops_build_kernel", "fd_pops_up_kernel", "fd_pops_query_kernel"};
    using Counts = CountBits;
    using Row = pgt_fd_row;
    using Total = pgt_fd_total;

    // populations from which a pair's products and terms are computed again instead of being kept (see the head of the file)
    template <int NP>
    static constexpr bool kRecompute = NP >= 7;

    // u*w - v*w: one candidate term, the two products of a pair each times one product of (x, o)
    static __device__ __forceinline__ double term(double u, double v, double w) { return __dsub_rn(__dmul_rn(u, w), __dmul_rn(v, w)); }

    // x itself; with AGAIN under a new name: each half moved through a DPP move that reads the lane's own value (quad_perm
    // 0,1,2,3; `id` is the move's unused old value and only tells one use from another), which the compiler does not see through
    template <bool AGAIN>
    static __device__ __forceinline__ double fresh(double x, int id) {
        if constexpr (AGAIN) {
            const int lo = __builtin_amdgcn_update_dpp(id, __double2loint(x), 0xE4, 0xF, 0xF, true);
            const int hi = __builtin_amdgcn_update_dpp(id, __double2hiint(x), 0xE4, 0xF, 0xF, true);
            return __hiloint2double(hi, lo);
        } else {
            return x;
        }
    }

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int G = NP - 1;  // ingroup populations; G is the outgroup's index
        constexpr int T = trio_count(NP);
        constexpr bool R = kRecompute<NP>;
        double q[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            q[k] = __dsub_rn(1.0, p[k]);
            ok[k] = c.ok(k);
        }
        // the two products of (x, o), once per site for every term weighted by population x
        double x_pq[G], x_qp[G];
#pragma unroll
        for (int x = 0; x < G; ++x) {
            x_pq[x] = __dmul_rn(p[x], q[G]);
            x_qp[x] = __dmul_rn(q[x], p[G]);
        }
        int t = 0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            // the terms of the pairs (i, b) weighted by b, for every trio that starts with i
            double pf[G], qf[G], hi_b[G], lo_b[G];
#pragma unroll
            for (int b = i + 1; b < G; ++b) {
                pf[b] = i > 0 ? fresh<R>(p[b], i) : p[b];
                qf[b] = __dsub_rn(1.0, pf[b]);
                const double qp = __dmul_rn(q[i], pf[b]), pq = __dmul_rn(p[i], qf[b]);
                hi_b[b] = term(qp, pq, x_pq[b]);
                lo_b[b] = term(pq, qp, x_qp[b]);
            }
#pragma unroll
            for (int j = i + 1; j + 1 < G; ++j) {
                // the products of the pair (i, j) and its terms weighted by i, for every trio (i, j, k > j)
                const double p_j = fresh<R>(p[j], 16 + 8 * i + j);
                const double qp = __dmul_rn(q[i], p_j), pq = __dmul_rn(p[i], __dsub_rn(1.0, p_j));
                const double hi_a = term(pq, qp, x_pq[i]);
                const double lo_a = term(qp, pq, x_qp[i]);
                const bool ok_ij = ok[i] && ok[j] && ok[G];
                const bool j_ge_i = p[j] >= p[i], j_le_i = p[j] <= p[i];
#pragma unroll
                for (int k = j + 1; k < G; ++k) {
                    const bool counted = ok_ij && ok[k];
                    const double abba = __dadd_rn(__dmul_rn(qp, x_pq[k]), __dmul_rn(pq, x_qp[k]));
                    const double baba = __dadd_rn(__dmul_rn(pq, x_pq[k]), __dmul_rn(qp, x_qp[k]));
                    const double num = __dsub_rn(abba, baba);
                    // the pair (j, k) weighted by k
                    const double qp_jk = __dmul_rn(qf[j], pf[k]), pq_jk = __dmul_rn(pf[j], qf[k]);
                    const double b1 = p[j] >= p[k] ? hi_b[j] : hi_b[k];
                    const double a1 = p[j] <= p[k] ? lo_b[j] : lo_b[k];
                    const double b2 = p[i] >= p[k] ? hi_a : term(qp_jk, pq_jk, x_pq[k]);
                    const double a2 = p[i] <= p[k] ? lo_a : term(pq_jk, qp_jk, x_qp[k]);
                    const double fd_den = __dadd_rn(b1, a1);
                    const double fdm_den = __dadd_rn(j_ge_i ? b1 : b2, j_le_i ? a1 : a2);
                    acc[t] = __dadd_rn(acc[t], counted ? num : 0.0);
                    acc[T + t] = __dadd_rn(acc[T + t], counted ? fd_den : 0.0);
                    acc[2 * T + t] = __dadd_rn(acc[2 * T + t], counted ? fdm_den : 0.0);
                    cnt[t] += (uint32_t)__popcll(__ballot(counted));
                    ++t;
                }
            }
        }
        if constexpr (R) __builtin_amdgcn_sched_barrier(0);  // the next site's arithmetic stays behind this one's
    }

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
        r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
        r.num = s[0] + 0.0;
        r.fd_den = s[1] + 0.0;
        r.fdm_den = s[2] + 0.0;
        r.fd = r.fd_den != 0.0 ? __ddiv_rn(r.num, r.fd_den) : 0.0;     // f_d of ((i,j),k), whatever its sign
        r.fdm = r.fdm_den != 0.0 ? __ddiv_rn(r.num, r.fdm_den) : 0.0;  // f_dM
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.num = s[0] + 0.0;
        r.fd_den = s[1] + 0.0;
        r.fdm_den = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_fd_pops_kernels(std::string *err) {
    allow_lds<FdPops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 4 <= n_pops <= 7 and minind >= 1: checked by the caller
int launch_fd_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                   int minind, const pgt_win *win, uint64_t n_win, pgt_fd_row *out, pgt_fd_total *tot, void *tree,
                   const LaunchEnv &e) {
    return launch_pops<FdPops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
