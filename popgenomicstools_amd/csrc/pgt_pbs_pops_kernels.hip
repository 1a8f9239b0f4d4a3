// pgt_pbs_pops_kernels.hip — the population branch statistic (PBS; Yi et al. 2010) of ALL trios i < j < k of 3 ... 6 populations,
// every population of a trio as the focal one, from the populations' own MAF columns (allele frequency f64 + individual count
// i32: 12 B/site/population).  All populations are equal.
//
// Spec (include/pgtwin.h, pgt_pbs_pops_reduce_dev): trio (i, j, k), i < j < k < NP, in lexicographic order.  The site counts for a
// trio iff all three populations have at least minind individuals (minind >= 1), and then contributes for each of the trio's
// pairs (x, y) = (i, j), (i, k), (j, k) exactly the two values the all-pairs FST front end adds for that pair
// (pgt_fst_site.h: WeirCockerham a and a + b, Hudson num and den).  A site that is not counted is selected away, never
// multiplied.  A window's row is the six SUMS over the sites counted FOR THE TRIO — not the pair's own sites, which is what
// makes the three branch lengths those of one tree — their number, and
//     fst_xy = den_xy != 0 ? num_xy / den_xy : 0        T_xy = -log(1 - fst_xy)
//     pbs_i = ((T_ij + T_ik) - T_jk) * 0.5 + 0.0        pbs_j = ((T_ij + T_jk) - T_ik) * 0.5 + 0.0        pbs_k = ((T_ik + T_jk) - T_ij) * 0.5 + 0.0
// every operation rounded on its own, nothing clamped.
//
// Six sums per trio do not fit the walk's node (pgt_pops_walk.h: three sums per item, at most 64 values per node), so the
// columns are walked TWICE through the unchanged walk, as two statistics with three sums per trio: PbsPass<Est, 0> the three
// numerators, PbsPass<Est, 1> the three denominators, both with the trio predicate and the counts as values.  A site computes
// each pair's value once (C(NP, 2) pairs) and hands it to the trios that hold the pair; the half of `pair` a pass does not use is
// dead code.  The passes write scratch rows and scratch totals behind the tree in the caller's workspace (the tree itself is
// reused by the second pass); pbs_finish_kernel, one thread per (trio, window) and per total, merges them into the rows.
// Tree, build walk and query of a pass: pgt_pops_walk.h; a node is 3 T doubles and T u32, T = C(NP, 3) = 1 / 4 / 10 / 20: the
// node of pgt_f3_pops_kernels.hip.  Rows of a trio are functions of the trio's own six columns and the window alone.
#include "pgt_fst_site.h"
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

// HALF 0: the numerators (a / num), 1: the denominators (a + b / den)
template <class Est, int HALF>
struct PbsPass {
    static constexpr int kMinPops = 3, kMaxPops = 6;  // 20 trios at most
    static constexpr int items(int np) { return all_trio_count(np); }  // lexicographic (i < j < k < NP), as F3Pops
    static constexpr int kSumsPerItem = 3;                             // the value of (i,j) of every trio, then of (i,k), then of (j,k)
    // populations from which the build and the query take one wave per SIMD: the compiler's resource report
    // (profiles/r18/pbs_pops.md), chosen so that no launched kernel uses scratch memory
    static constexpr int kOneWaveFrom = 5;
    static constexpr const char *kOneWaveKnob = nullptr;
    static constexpr int kQueryOneWaveFrom = 6;
    static constexpr const char *kKernelNames[3] = {"pbs_pops_build_kernel", "pbs_pops_up_kernel", "pbs_pops_query_kernel"};
    using Counts = CountValues;
    using Row = PbsPassRow;
    using Total = PbsPassTotal;

    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        constexpr int T = all_trio_count(NP);
        typename Est::template Terms<NP> s;
        s.prepare(p, c);
        // this pass's value of the pairs a < b, once per site for every trio that holds the pair
        double val[NP][NP];
#pragma unroll
        for (int a = 0; a < NP; ++a)
#pragma unroll
            for (int b = a + 1; b < NP; ++b) {
                double num, den;
                s.pair(p, a, b, num, den);
                val[a][b] = HALF == 0 ? num : den;
            }
        int t = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool ok_ij = s.ok[i] && s.ok[j];
#pragma unroll
                for (int k = j + 1; k < NP; ++k) {
                    const bool counted = ok_ij && s.ok[k];
                    acc[t] = __dadd_rn(acc[t], counted ? val[i][j] : 0.0);
                    acc[T + t] = __dadd_rn(acc[T + t], counted ? val[i][k] : 0.0);
                    acc[2 * T + t] = __dadd_rn(acc[2 * T + t], counted ? val[j][k] : 0.0);
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
        r.s[0] = s[0] + 0.0;
        r.s[1] = s[1] + 0.0;
        r.s[2] = s[2] + 0.0;
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.s[0] = s[0] + 0.0;
        r.s[1] = s[1] + 0.0;
        r.s[2] = s[2] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

// branch, pbs_of: the closing arithmetic of a row (pgt_pops_common.h, shared with the block jackknife of these rows)

// One thread per scratch row (n_rows = T * n_win, trio-major as the passes wrote them) and, behind them, per scratch total
// (n_tot = T, or 0): the two passes' sums side by side, and the closing arithmetic.  Both passes counted the same sites.
__global__ __launch_bounds__(256) void pbs_finish_kernel(const PbsPassRow *__restrict__ num_rows, const PbsPassRow *__restrict__ den_rows, uint64_t n_rows,
                                                         pgt_pbs_row *__restrict__ out, const PbsPassTotal *__restrict__ num_tot,
                                                         const PbsPassTotal *__restrict__ den_tot, uint32_t n_tot, pgt_pbs_total *__restrict__ tot) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) {
        const PbsPassRow a = num_rows[i], b = den_rows[i];
        pgt_pbs_row r;
        r.start = a.start;
        r.end = a.end;
        r.mid = a.mid;
        r.n = a.n;
        r.num_ij = a.s[0]; r.num_ik = a.s[1]; r.num_jk = a.s[2];
        r.den_ij = b.s[0]; r.den_ik = b.s[1]; r.den_jk = b.s[2];
        pbs_of(a.s, b.s, r.pbs_i, r.pbs_j, r.pbs_k);
        out[i] = r;
    } else if (i - n_rows < n_tot) {
        const uint64_t t = i - n_rows;
        const PbsPassTotal a = num_tot[t], b = den_tot[t];
        pgt_pbs_total r;
        r.num_ij = a.s[0]; r.num_ik = a.s[1]; r.num_jk = a.s[2];
        r.den_ij = b.s[0]; r.den_ik = b.s[1]; r.den_jk = b.s[2];
        pbs_of(a.s, b.s, r.pbs_i, r.pbs_j, r.pbs_k);
        r.neff = a.neff;
        r.nskip = a.nskip;
        tot[t] = r;
    }
}

template <class Est>
int launch_pbs(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
               const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot, void *work, const LaunchEnv &e) {
    const PbsWork w = pbs_work(n_pops, n, n_win);
    char *base = static_cast<char *>(work);
    PbsPassRow *rows[2] = {reinterpret_cast<PbsPassRow *>(base + w.rows[0]), reinterpret_cast<PbsPassRow *>(base + w.rows[1])};
    PbsPassTotal *tots[2] = {tot ? reinterpret_cast<PbsPassTotal *>(base + w.tot[0]) : nullptr, tot ? reinterpret_cast<PbsPassTotal *>(base + w.tot[1]) : nullptr};
    // the events of a profiled call: the first pass and the second pass's build count as the build, the second query and the
    // finish as the query
    const LaunchEnv first{e.stream, e.ev_build0, nullptr, nullptr, e.err, e.hints}, second{e.stream, nullptr, e.ev_build1, nullptr, e.err, e.hints};
    if (int rc = launch_pops<PbsPass<Est, 0>>(pos, freq, nind, n_pops, n, minind, win, n_win, rows[0], tots[0], work, first)) return rc;
    if (int rc = launch_pops<PbsPass<Est, 1>>(pos, freq, nind, n_pops, n, minind, win, n_win, rows[1], tots[1], work, second)) return rc;
    const uint64_t n_rows = (uint64_t)w.n_trios * n_win, n_threads = n_rows + (tot ? w.n_trios : 0);
    if (n_threads > 0) {  // n_win == 0 without tot: the tree-only call, which builds (both passes) and has nothing to finish
        hipLaunchKernelGGL(pbs_finish_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(e.stream), rows[0], rows[1], n_rows, out,
                           tots[0], tots[1], tot ? w.n_trios : 0u, tot);
        if (int rc = hip_fail(hipGetLastError(), "pbs_finish_kernel", e.err)) return rc;
    }
    return record_event(e.ev_query1, static_cast<hipStream_t>(e.stream), e.err);
}

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_pbs_pops_kernels(std::string *err) {
    allow_lds<PbsPass<WeirCockerham, 0>>();
    allow_lds<PbsPass<WeirCockerham, 1>>();
    allow_lds<PbsPass<Hudson, 0>>();
    allow_lds<PbsPass<Hudson, 1>>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

// 3 <= n_pops <= 6, minind >= 1: checked by the caller (n_win == 0 without tot passes those checks whenever n > 0)
int launch_pbs_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                    int minind, const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot, void *work,
                    const LaunchEnv &e, FstPopsEstimator estimator) {
    if (estimator == FstPopsEstimator::Hudson) return launch_pbs<Hudson>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, work, e);
    return launch_pbs<WeirCockerham>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, work, e);
}

}  // namespace pgt
