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
// Tree, build walk and query: pgt_pops_walk.h, with three sums per TRIO: a node is 3 T doubles (bbaa of trio 0 .. T-1, then
// abba, then baba) and T u32, T = C(NP-1, 3) = 1 / 4 / 10 / 20.  The counts decide nothing but the predicate, so they travel
// as packed bits (CountBits), the cheaper of the two exchanges; a trio's predicate is the AND of four populations' lane masks.
// Rows of a trio are functions of the trio's and the outgroup's eight columns and the window alone.
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct DstatPops {
    static constexpr int kMinPops = 4, kMaxPops = 7;  // three ingroup populations and an outgroup; 20 trios at most (2, 3 and 8 are not instantiated)
    static constexpr int items(int np) { return trio_count(np); }  // lexicographic (i < j < k < NP-1): (0,1,2),(0,1,3),..,(0,2,3),..
    static constexpr int kSumsPerItem = 3;                         // Σbbaa of every trio, then Σabba of every trio, then Σbaba of every trio
    // populations from which the build takes one wave per SIMD: the compiler's resource report (profiles/r12/dstat_pops.md) shows
    // the two-wave build at 182 registers with 4 populations and spilling from 5 on (52 / 404 / 912 bytes of scratch per lane at
    // 5 / 6 / 7: two register sets of 12 NP and 6 T running values), the one-wave build without scratch at every count
    static constexpr int kOneWaveFrom = 5;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 6;
    static constexpr const char *kKernelNames[3] = {"dstat_pops_build_kernel", "dstat_pops_up_kernel", "dstat_pops_query_kernel"};
    using Counts = CountBits;
    using Row = pgt_dstat_row;
    using Total = pgt_dstat_total;

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int G = NP - 1;  // ingroup populations; G is the outgroup's index
        constexpr int T = trio_count(NP);
        double q[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            q[k] = __dsub_rn(1.0, p[k]);
            ok[k] = c.ok(k);
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

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
        r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
        r.bbaa = s[0] + 0.0;
        r.abba = s[1] + 0.0;
        r.baba = s[2] + 0.0;
        const double den = __dadd_rn(r.abba, r.baba);
        r.d = den != 0.0 ? __ddiv_rn(__dsub_rn(r.abba, r.baba), den) : 0.0;  // Patterson's D of ((i,j),k)
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.bbaa = s[0] + 0.0;
        r.abba = s[1] + 0.0;
        r.baba = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_dstat_pops_kernels(std::string *err) {
    allow_lds<DstatPops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 4 <= n_pops <= 7 and minind >= 1: checked by the caller
int launch_dstat_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                      int minind, const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, pgt_dstat_total *tot, void *tree,
                      const LaunchEnv &e) {
    return launch_pops<DstatPops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
