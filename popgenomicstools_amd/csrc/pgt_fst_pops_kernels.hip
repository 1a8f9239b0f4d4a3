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
// Tree, build walk and query: pgt_pops_walk.h, with two sums per pair.  The counts are needed as VALUES here, not only for
// the predicate (CountValues).  Rows of a pair are functions of the pair's own four columns and the window alone: every
// pair's arithmetic reads only its two populations' registers.
#include "pgt_fst_site.h"
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

// ---- per-site contribution ---------------------------------------------------------------------------------------------
// The estimator is a compile-time tag with a static per-site function (WeirCockerham, Hudson: pgt_fst_site.h, where the trio
// statistic of pgt_pbs_pops_kernels.hip finds the same arithmetic): the walk knows only that a pair keeps two sums (acc[v],
// acc[P + v]) and a count (cnt[v]).
// Two statistics that share everything but `site` (the estimator's)
template <class Est>
struct FstPops : Est {
    static constexpr int kMinPops = 2, kMaxPops = 8;
    static constexpr int items(int np) { return pair_count(np); }  // lexicographic (i < j): (0,1),(0,2),..,(0,NP-1),(1,2),..
    static constexpr int kSumsPerItem = 2;                         // Σa of every pair, then Σ(a+b) of every pair
    static constexpr int kOneWaveFrom = 5;  // populations from which the build takes one wave per SIMD (two register sets of 12 NP and 3 P running values)
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 5;
    static constexpr const char *kKernelNames[3] = {"fst_pops_build_kernel", "fst_pops_up_kernel", "fst_pops_query_kernel"};
    using Counts = CountValues;
    using Row = pgt_fst_row;
    using Total = pgt_fst_total;

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.mid = (uint32_t)(start + end) / 2u;  // fstWindow.cpp:73
        r.n = c;                               // counted sites; the caller derives nskip = (hi - lo) - n
        r.asum = s[0] + 0.0;
        r.bsum = s[1] + 0.0;
        r.fst = r.bsum != 0.0 ? r.asum / r.bsum : 0.0;  // fstWindow.cpp:85
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.asum = s[0] + 0.0;
        r.bsum = s[1] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_fst_pops_kernels(std::string *err) {
    allow_lds<FstPops<WeirCockerham>>();
    allow_lds<FstPops<Hudson>>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 2 <= n_pops <= 8 and minind >= 1: checked by the caller; both estimators share the tree's layout
int launch_fst_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                    int minind, const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot, void *tree,
                    const LaunchEnv &e, FstPopsEstimator estimator) {
    if (estimator == FstPopsEstimator::Hudson)
        return launch_pops<FstPops<Hudson>>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
    return launch_pops<FstPops<WeirCockerham>>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
