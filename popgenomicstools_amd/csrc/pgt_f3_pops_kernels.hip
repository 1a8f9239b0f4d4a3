// pgt_f3_pops_kernels.hip — the 3-population statistic f3 (Reich et al. 2009; Patterson et al. 2012; treemix's threepop,
// ADMIXTOOLS' qp3Pop without its normalisation) of ALL trios i < j < k of 3 ... 6 populations, each trio with every one of its
// three populations as the target, from the populations' own MAF columns (allele frequency f64 + individual count i32:
// 12 B/site/population) in ONE pass.  There is no outgroup: all populations are equal.
//
// Spec (include/pgtwin.h, pgt_f3_pops_reduce_dev): trio (i, j, k), i < j < k < NP, in lexicographic order.  The site counts for a
// trio iff all three populations have at least minind individuals (minind >= 1), and then contributes, with p_x the frequency
// and n_x the individual count, every operation rounded on its own:
//     h_x  = (p_x * (1 - p_x)) / (2 n_x - 1)          per population: the bias of p_x^2 (Hudson::site's grouping and divisor)
//     d_ab = p_a - p_b                                per pair a < b
//     s0 = d_ij * d_ik - h_i          f3(i; j, k)
//     s1 = (-d_ij) * d_jk - h_j       f3(j; i, k)
//     s2 = d_ik * d_jk - h_k          f3(k; i, j)
// The only division is per population and site (2 n - 1: odd, at least 1 wherever it is used), the differences are per pair and
// site; a trio takes three products and three subtractions.  A site that is not counted is selected away, never multiplied: its
// frequencies and counts may be anything (n <= 0: a negative divisor).  A window's row is the three SUMS and the number of
// counted sites: the means are the caller's division (and the jackknife's: pgt_dstat_jack_kernels.hip, F3Mean).
//
// Tree, build walk and query: pgt_pops_walk.h, with three sums per TRIO: a node is 3 T doubles (s0 of trio 0 .. T-1, then s1,
// then s2) and T u32, T = C(NP, 3) = 1 / 4 / 10 / 20: the node, the stage and the tree size of the D kernel at one population
// fewer.  The counts are needed as VALUES (CountValues), as in pgt_fst_pops_kernels.hip.  Rows of a trio are functions of the
// trio's own six columns and the window alone.
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct F3Pops {
    static constexpr int kMinPops = 3, kMaxPops = 6;  // 20 trios at most: the D kernel's 60 running sums
    static constexpr int items(int np) { return all_trio_count(np); }  // lexicographic (i < j < k < NP): (0,1,2),(0,1,3),..,(0,2,3),..
    static constexpr int kSumsPerItem = 3;                             // Σs0 of every trio, then Σs1 of every trio, then Σs2
    // populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r16/f3_pops.md) shows
    // the two-wave build at 174 / 229 registers with 3 / 4 populations and spilling from 5 on (260 / 876 bytes of scratch per
    // lane at 5 / 6), the one-wave build without scratch at every count; the query fits 256 registers up to 5 populations (254)
    // and needs more at 6
    static constexpr int kOneWaveFrom = 5;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 6;
    static constexpr const char *kKernelNames[3] = {"f3_pops_build_kernel", "f3_pops_up_kernel", "f3_pops_query_kernel"};
    using Counts = CountValues;
    using Row = pgt_f3_row;
    using Total = pgt_f3_total;

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int T = all_trio_count(NP);
        double h[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            ok[k] = c.ok(k);
            const double m = __dsub_rn(__dmul_rn(2.0, (double)c.n(k)), 1.0);  // haploid sample size minus one
            h[k] = __ddiv_rn(__dmul_rn(p[k], __dsub_rn(1.0, p[k])), m);
        }
        // the differences of the pairs a < b, once per site for every trio that holds the pair
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
                const double nd_ij = -d[i][j];
#pragma unroll
                for (int k = j + 1; k < NP; ++k) {
                    const bool counted = ok_ij && ok[k];
                    const double s0 = __dsub_rn(__dmul_rn(d[i][j], d[i][k]), h[i]);
                    const double s1 = __dsub_rn(__dmul_rn(nd_ij, d[j][k]), h[j]);
                    const double s2 = __dsub_rn(__dmul_rn(d[i][k], d[j][k]), h[k]);
                    acc[t] = __dadd_rn(acc[t], counted ? s0 : 0.0);
                    acc[T + t] = __dadd_rn(acc[T + t], counted ? s1 : 0.0);
                    acc[2 * T + t] = __dadd_rn(acc[2 * T + t], counted ? s2 : 0.0);
                    cnt[t] += (uint32_t)__popcll(__ballot(counted));
                    ++t;
                }
            }
    }

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
        r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
        r.reserved_ = 0.0;
        r.f3_i = s[0] + 0.0;
        r.f3_j = s[1] + 0.0;
        r.f3_k = s[2] + 0.0;
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.f3_i = s[0] + 0.0;
        r.f3_j = s[1] + 0.0;
        r.f3_k = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_f3_pops_kernels(std::string *err) {
    allow_lds<F3Pops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 3 <= n_pops <= 6 and minind >= 1: checked by the caller
int launch_f3_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                   int minind, const pgt_win *win, uint64_t n_win, pgt_f3_row *out, pgt_f3_total *tot, void *tree,
                   const LaunchEnv &e) {
    return launch_pops<F3Pops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
