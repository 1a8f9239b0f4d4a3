// pgt_f4_pops_kernels.hip — the 4-population statistic f4 (Reich et al. 2009; Patterson et al. 2012; treemix's fourpop,
// ADMIXTOOLS' qpDstat -f4mode) of ALL quartets i < j < k < l of 4 ... 6 populations, each quartet in its three pairings
// (ij;kl), (ik;jl), (il;jk), from the populations' own MAF columns (allele frequency f64 + individual count i32:
// 12 B/site/population) in ONE pass.  There is no outgroup: all populations are equal.
//
// Spec (include/pgtwin.h, pgt_f4_pops_reduce_dev): quartet (i, j, k, l), i < j < k < l < NP, in lexicographic order.  The site
// counts for a quartet iff all four populations have at least minind individuals, and then contributes, with p_x the frequency,
// every operation rounded on its own:
//     d_ab = p_a - p_b                 per pair a < b
//     s0 = d_ij * d_kl                 f4(i, j; k, l)
//     s1 = d_ik * d_jl                 f4(i, k; j, l)
//     s2 = d_il * d_jk                 f4(i, l; j, k)
// No division and no bias term: the counts enter through the predicate alone.  The differences are per pair and site, shared by
// every quartet that holds the pair; a quartet takes three products.  A site that is not counted is selected away, never
// multiplied: its frequencies may be anything.  In real arithmetic s0 - s1 + s2 = 0; all three are kept, so that the row has the
// layout and the three items of pgt_f3_row (the jackknife's loader: pgt_dstat_jack_kernels.hip, Mean).  A window's row is the
// three SUMS and the number of counted sites: the means are the caller's division (and the jackknife's).
//
// Tree, build walk and query: pgt_pops_walk.h, with three sums per QUARTET: a node is 3 Q doubles (s0 of quartet 0 .. Q-1, then
// s1, then s2) and Q u32, Q = C(NP, 4) = 1 / 5 / 15: 45 running sums at 6 populations against f3's 60.  The counts decide nothing
// but the predicate, so they travel as packed bits (CountBits), as in pgt_dstat_pops_kernels.hip.  Rows of a quartet are
// functions of the quartet's own eight columns and the window alone.
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct F4Pops {
    static constexpr int kMinPops = 4, kMaxPops = 6;  // 15 quartets at most (7 populations: 35 quartets, 105 sums per node)
    static constexpr int items(int np) { return all_quartet_count(np); }  // lexicographic (i < j < k < l < NP): (0,1,2,3),(0,1,2,4),..
    static constexpr int kSumsPerItem = 3;                                // Σs0 of every quartet, then Σs1 of every quartet, then Σs2
    // populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r19/f4_pops.md) shows
    // the two-wave build at 176 registers with 4 populations and spilling from 5 on (28 bytes of scratch per lane at 5), the
    // one-wave build without scratch at every count (256 + 6 / 256 + 132 registers at 5 / 6); the query fits 256 registers up to
    // 5 populations (171) and needs 256 + 64 at 6
    static constexpr int kOneWaveFrom = 5;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 6;
    static constexpr const char *kKernelNames[3] = {"f4_pops_build_kernel", "f4_pops_up_kernel", "f4_pops_query_kernel"};
    using Counts = CountBits;
    using Row = pgt_f4_row;
    using Total = pgt_f4_total;

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int Q = all_quartet_count(NP);
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) ok[k] = c.ok(k);
        // the differences of the pairs a < b, once per site for every quartet that holds the pair
        double d[NP][NP];
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int b = a + 1; b < NP; ++b) d[a][b] = __dsub_rn(p[a], p[b]);
        int t = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool ok_ij = ok[i] && ok[j];
#pragma unroll
                for (int k = j + 1; k < NP; ++k) {
                    const bool ok_ijk = ok_ij && ok[k];
#pragma unroll
                    for (int l = k + 1; l < NP; ++l) {
                        const bool counted = ok_ijk && ok[l];
                        const double s0 = __dmul_rn(d[i][j], d[k][l]);
                        const double s1 = __dmul_rn(d[i][k], d[j][l]);
                        const double s2 = __dmul_rn(d[i][l], d[j][k]);
                        acc[t] = __dadd_rn(acc[t], counted ? s0 : 0.0);
                        acc[Q + t] = __dadd_rn(acc[Q + t], counted ? s1 : 0.0);
                        acc[2 * Q + t] = __dadd_rn(acc[2 * Q + t], counted ? s2 : 0.0);
                        cnt[t] += (uint32_t)__popcll(__ballot(counted));
                        ++t;
                    }
                }
            }
    }

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
        r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
        r.reserved_ = 0.0;
        r.f4_ij_kl = s[0] + 0.0;
        r.f4_ik_jl = s[1] + 0.0;
        r.f4_il_jk = s[2] + 0.0;
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.f4_ij_kl = s[0] + 0.0;
        r.f4_ik_jl = s[1] + 0.0;
        r.f4_il_jk = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_f4_pops_kernels(std::string *err) {
    allow_lds<F4Pops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 4 <= n_pops <= 6 and minind >= 1: checked by the caller
int launch_f4_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                   int minind, const pgt_win *win, uint64_t n_win, pgt_f4_row *out, pgt_f4_total *tot, void *tree,
                   const LaunchEnv &e) {
    return launch_pops<F4Pops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
