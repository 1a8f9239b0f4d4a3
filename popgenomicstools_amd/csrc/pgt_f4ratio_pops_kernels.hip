// pgt_f4ratio_pops_kernels.hip — the sums behind the f4-ratio admixture proportions (Patterson et al. 2012; ADMIXTOOLS'
// qpF4ratio), alpha = f4(A,O; X,C) / f4(A,O; B,C), for ALL triples of the middle populations of 5 ... 7 populations, from the
// populations' own MAF columns (allele frequency f64 + individual count i32: 12 B/site/population) in ONE pass.
//
// Spec (include/pgtwin.h, pgt_f4ratio_pops_reduce_dev): population 0 is A, population NP-1 the outgroup O, populations
// 1 .. NP-2 the m = NP-2 middle ones; an item is a middle triple (i, j, k), 1 <= i < j < k <= NP-2, in lexicographic order.  The
// site counts for a triple iff A, O and the triple's three populations have at least minind individuals each — FIVE
// populations, so numerator and denominator of every ratio are counted over the same sites — and then contributes, with p_x the
// frequency, every operation rounded on its own:
//     e    = p_0 - p_{NP-1}            once per site
//     d_ab = p_a - p_b                 per middle pair a < b, shared by the triples that hold it
//     s0 = e * d_ij                    f4(A,O; i,j)
//     s1 = e * d_ik                    f4(A,O; i,k)
//     s2 = e * d_jk                    f4(A,O; j,k)
// No division and no bias term: the counts enter through the predicate alone.  A site that is not counted is selected away,
// never multiplied: its frequencies may be anything, in A and O as well.  In real arithmetic s0 - s1 + s2 = 0; all three are
// kept, so that the row has the layout of pgt_f4_row (the jackknife's loader: pgt_dstat_jack_kernels.hip, Ratio).  A window's
// row is the three SUMS and the number of counted sites: the six ratios of a triple are the caller's division (and the
// jackknife's), as f4's means are.
//
// Tree, build walk and query: pgt_pops_walk.h, with three sums per TRIPLE: a node is 3 T doubles (s0 of triple 0 .. T-1, then
// s1, then s2) and T u32, T = C(NP-2, 3) = 1 / 4 / 10: 30 running sums at 7 populations against f4's 45 at 6.  The counts
// travel as packed bits (CountBits), as in pgt_f4_pops_kernels.hip.  Rows of a triple are functions of the ten columns of A, O
// and the triple, and the window alone.
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct F4RatioPops {
    static constexpr int kMinPops = 5, kMaxPops = 7;  // A, three to five middle populations, O (8 populations: 20 triples, 60 sums per node)
    static constexpr int items(int np) { return middle_triple_count(np); }  // lexicographic (1 <= i < j < k <= NP-2): (1,2,3),(1,2,4),..
    static constexpr int kSumsPerItem = 3;                                  // Σs0 of every triple, then Σs1 of every triple, then Σs2
    // populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r20/f4ratio_pops.md)
    // shows the two-wave build at 206 registers with 5 populations and spilling from 6 on (116 / 464 bytes of scratch per lane
    // at 6 / 7), the one-wave build without scratch at every count (255 + 28 / 256 + 112 registers at 6 / 7); the query fits
    // 256 registers up to 6 populations (118 / 174) and needs 256 + 13 at 7
    static constexpr int kOneWaveFrom = 6;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 7;
    static constexpr const char *kKernelNames[3] = {"f4ratio_pops_build_kernel", "f4ratio_pops_up_kernel", "f4ratio_pops_query_kernel"};
    using Counts = CountBits;
    using Row = pgt_f4ratio_row;
    using Total = pgt_f4ratio_total;

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int T = middle_triple_count(NP);
        constexpr int O = NP - 1;
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) ok[k] = c.ok(k);
        const bool ok_ao = ok[0] && ok[O];
        const double e = __dsub_rn(p[0], p[O]);
        // the differences of the middle pairs a < b, once per site for every triple that holds the pair
        double d[NP][NP];
#pragma unroll
        for (int a = 1; a < O; ++a)
#pragma unroll
            for (int b = a + 1; b < O; ++b) d[a][b] = __dsub_rn(p[a], p[b]);
        int t = 0;
#pragma unroll
        for (int i = 1; i < O; ++i)
#pragma unroll
            for (int j = i + 1; j < O; ++j) {
                const bool ok_ij = ok_ao && ok[i] && ok[j];
#pragma unroll
                for (int k = j + 1; k < O; ++k) {
                    const bool counted = ok_ij && ok[k];
                    const double s0 = __dmul_rn(e, d[i][j]);
                    const double s1 = __dmul_rn(e, d[i][k]);
                    const double s2 = __dmul_rn(e, d[j][k]);
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
        r.g_ij = s[0] + 0.0;
        r.g_ik = s[1] + 0.0;
        r.g_jk = s[2] + 0.0;
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.g_ij = s[0] + 0.0;
        r.g_ik = s[1] + 0.0;
        r.g_jk = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_f4ratio_pops_kernels(std::string *err) {
    allow_lds<F4RatioPops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 5 <= n_pops <= 7 and minind >= 1: checked by the caller
int launch_f4ratio_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                        int minind, const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out, pgt_f4ratio_total *tot, void *tree,
                        const LaunchEnv &e) {
    return launch_pops<F4RatioPops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
