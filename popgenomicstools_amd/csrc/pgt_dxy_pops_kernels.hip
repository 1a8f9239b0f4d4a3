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
// Tree, build walk and query: pgt_pops_walk.h, with one sum per pair.  The counts decide nothing but the predicate: they
// travel as packed bits (CountBits), and minind may be anything (a site outside a range is masked, not given a count of 0).
#include "pgt_pops_walk.h"

namespace pgt {
namespace {

using namespace dev;

struct DxyPops {
    static constexpr int kMinPops = 2, kMaxPops = 8;
    static constexpr int items(int np) { return pair_count(np); }  // lexicographic (i < j): (0,1),(0,2),..,(0,NP-1),(1,2),..
    static constexpr int kSumsPerItem = 1;
    static constexpr int kOneWaveFrom = 5;  // populations from which the two-waves-per-SIMD build would not fit its registers
    static constexpr const char *kOneWaveKnob = "PGT_DXY_POPS_ONE_WAVE_FROM";  // tools/measure_dxy_pops.py
    static constexpr int kQueryOneWaveFrom = 7;  // with 7 and 8 populations the 2 x 21 / 2 x 28 running sums and a stride's columns need more than 256 registers
    static constexpr const char *kKernelNames[3] = {"dxy_pops_build_kernel", "dxy_pops_up_kernel", "dxy_pops_query_kernel"};
    using Counts = CountBits;
    using Row = pgt_dxy_row;
    using Total = pgt_dxy_total;

    // d: exactly dxy_site_pred of pgt_kernels.hip (dxyWindow.cpp:381) with p1 = p_i, p2 = p_j.
    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *p, const C &c) {
        double om[NP];
        bool ok[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            om[k] = __dsub_rn(1.0, p[k]);
            ok[k] = c.ok(k);
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

    static __device__ __forceinline__ void finish_row(Row &r, uint32_t start, uint32_t end, uint64_t range, const double *s, uint32_t c) {
        r.start = start;
        r.end = end;
        r.neff = c;
        r.nskip = (uint32_t)range - c;  // dxyWindow.cpp:179-186: every site of the range is counted or skipped
        r.sum = s[0] + 0.0;
    }
    static __device__ __forceinline__ void finish_total(Total &r, const double *s, uint32_t c, uint64_t n_sites) {
        r.sum = s[0] + 0.0;
        r.neff = c;
        r.nskip = n_sites - c;
    }
};

}  // namespace

// Called once from pgt_open, so that no attribute call can fall inside a caller's stream capture.
int init_dxy_pops_kernels(std::string *err) {
    allow_lds<DxyPops>();
    return hip_fail(hipGetLastError(), "hipFuncSetAttribute", err);
}

int launch_dxy_pops(const uint32_t *pos, const double *const *freq, const int32_t *const *nind, uint32_t n_pops, uint64_t n,
                    int minind, const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot, void *tree,
                    const LaunchEnv &e) {
    return launch_pops<DxyPops>(pos, freq, nind, n_pops, n, minind, win, n_win, out, tot, tree, e);
}

}  // namespace pgt
