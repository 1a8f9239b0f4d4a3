// pgt_fst_site.h — the per-site arithmetic of the two FST estimators over (freq, nInd) columns, shared by the all-pairs FST
// kernels (pgt_fst_pops_kernels.hip, where the spec and the derivation of the divisions stand) and the trio statistic built
// from the same two values per pair (pgt_pbs_pops_kernels.hip).  An estimator is a tag with
//     Terms<NP>                what a site computes once per population: prepare(f, c) with f[k], c.n(k) population k's frequency
//                              and individual count at the site
//     Terms<NP>::pair(f, i, j, num, den)    the two values the pair i < j adds at a counted site
//     site<NP>(acc, cnt, f, c) one site into the running sums of ALL pairs: acc[v] += num, acc[P + v] += den, cnt[v] += counted
// Every value is a function of the pair's own two populations alone.  A site that is not counted may have n1 n2 = 0 (q infinite,
// a NaN) or a negative divisor: its values are selected away by the caller, never multiplied.
#pragma once

#include <hip/hip_runtime.h>

#include "pgt_pops_common.h"

namespace pgt {
namespace dev {

// 1/d for d >= 1 (finite): the hardware estimate and two Newton steps
__device__ __forceinline__ double recip(double d) {
    double x = __builtin_amdgcn_rcp(d);
    x = fma(x, fma(-d, x, 1.0), x);
    x = fma(x, fma(-d, x, 1.0), x);
    return x;
}

// The Weir–Cockerham components (the spec at the top of pgt_fst_pops_kernels.hip): num = a, den = a + b
struct WeirCockerham {
    template <int NP>
    struct Terms {
        double nd[NP], n4[NP], na[NP];
        bool ok[NP];  // the -minind predicate of every population at the site
        template <class C>
        __device__ __forceinline__ void prepare(const double *f, const C &c) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                nd[k] = (double)c.n(k);
                ok[k] = c.ok(k);
                n4[k] = 4.0 * nd[k];
                na[k] = nd[k] * ((2.0 * f[k]) * (1.0 - f[k]));  // n_k alpha_k, betaAFOutlier.R:408-410
            }
        }
        __device__ __forceinline__ void pair(const double *f, int i, int j, double &a, double &ab) const {
            const double npool = nd[i] + nd[j];
            const double p4 = n4[i] * nd[j];                // 4 n1 n2
            const double q = recip((npool - 1.0) * p4);
            const double t = (na[i] + na[j]) * q;
            const double b = t * p4;
            const double d = f[i] - f[j];
            a = d * d - t * npool;
            ab = a + b;
        }
    };
    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *f, const C &c) {
        constexpr int P = pair_count(NP);
        Terms<NP> s;
        s.prepare(f, c);
        int v = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool counted = s.ok[i] && s.ok[j];
                double a, ab;
                s.pair(f, i, j, a, ab);
                acc[v] = acc[v] + (counted ? a : 0.0);
                acc[P + v] = acc[P + v] + (counted ? ab : 0.0);
                cnt[v] += (uint32_t)__popcll(__ballot(counted));
                ++v;
            }
    }
};

// Hudson's estimator as a ratio of averages (Hudson, Slatkin & Maddison 1992; Bhatia et al. 2013, eq. 10), the definition of
// pgt_fst_hudson_pops_reduce_dev in include/pgtwin.h: num = (p1 - p2)^2 - h_1 - h_2 with h_k = p_k (1 - p_k) / (2 n_k - 1),
// den = p1 (1 - p2) + p2 (1 - p1) — dxy_site_pred's roundings (pgt_kernels.hip), so a pair's denominator IS its dxy.
// Every operation is rounded on its own.  The only division is per population and site (pi_site's divisor 2 n - 1: odd, never
// 0), not per pair; an uncounted site (n_k <= 0: a negative divisor; any frequency) is selected away, never multiplied.
struct Hudson {
    template <int NP>
    struct Terms {
        double om[NP], h[NP];
        bool ok[NP];
        template <class C>
        __device__ __forceinline__ void prepare(const double *f, const C &c) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                ok[k] = c.ok(k);
                om[k] = __dsub_rn(1.0, f[k]);
                const double m = __dsub_rn(__dmul_rn(2.0, (double)c.n(k)), 1.0);  // haploid sample size minus one
                h[k] = __ddiv_rn(__dmul_rn(f[k], om[k]), m);
            }
        }
        __device__ __forceinline__ void pair(const double *f, int i, int j, double &num, double &den) const {
            const double d = __dsub_rn(f[i], f[j]);
            num = __dsub_rn(__dsub_rn(__dmul_rn(d, d), h[i]), h[j]);
            den = __dadd_rn(__dmul_rn(f[i], om[j]), __dmul_rn(f[j], om[i]));
        }
    };
    template <int NP, class C>
    static __device__ __forceinline__ void site(double *acc, uint32_t *cnt, const double *f, const C &c) {
        constexpr int P = pair_count(NP);
        Terms<NP> s;
        s.prepare(f, c);
        int v = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int j = i + 1; j < NP; ++j) {
                const bool counted = s.ok[i] && s.ok[j];
                double num, den;
                s.pair(f, i, j, num, den);
                acc[v] = acc[v] + (counted ? num : 0.0);
                acc[P + v] = acc[P + v] + (counted ? den : 0.0);
                cnt[v] += (uint32_t)__popcll(__ballot(counted));
                ++v;
            }
    }
};

}  // namespace dev
}  // namespace pgt
