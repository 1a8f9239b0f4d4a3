/*
 * pgtwin.h — C-ABI of libpgtwin: the MI355X (gfx950) window-scan engine that replaces the
 * per-window reduction of PopGenomicsTools' fstWindow / hetWindow / dxyWindow.
 *
 * The reference has no FFI or plugin interface; the seam this library replaces is the
 * function `calcWindow` and the bookkeeping around its call sites (file:line in the reference):
 *     fstWindow.cpp:69-107   called from fstWindow.cpp:134,137,151
 *     hetWindow.cpp:66-105   called from hetWindow.cpp:132,135,149
 *     dxyWindow.cpp:172-209  called from dxyWindow.cpp:346,354,358,366,377,416,425
 * The reference calls it once per window on a W-entry buffer it owns and re-sums; this library
 * is called once per input: the host describes every window as a range [lo,hi) of the global
 * site index (pgt_build_windows_*), and the device reduces all of them from structure-of-arrays
 * columns resident in HBM (pgt_*_reduce*).
 *
 * Conventions
 *   - plain C types only; every function returns PGT_OK (0) or a PGT_E* code; the message is
 *     retrievable with pgt_last_error(ctx) (ctx may be NULL for the ctx-less functions);
 *     the reference's tools exit 255 on error (`return -1`, fstWindow.cpp:42,48,55) and the
 *     retained C++ hosts do the same after printing that message;
 *   - the caller owns every buffer; the library retains none of the caller's memory past return (a context keeps
 *     its own scratch between calls: the pinned staging ring and the window / row / tree workspace of the host-buffer
 *     entry points, 64 MiB + about 1 % of the largest input seen; pgt_close frees them);
 *   - one pgt_ctx per GPU and per thread (one process per GPU); a ctx is not thread-safe;
 *   - there is NO CPU fallback: without a usable gfx950 device pgt_open fails.
 *
 * Values the columns admit (tests/test_special_values.py)
 *   - a, b (fst) and score (ihs / xpehh): ANY f64, NaN and +-inf included.  Sums and the one division per row follow IEEE 754
 *     as the reference's own `+=` and `/` do (fstWindow.cpp:76-85): a NaN or an infinity reaches exactly the rows of the windows
 *     that hold it, a sum starts at +0.0 (never -0.0), fst is ONE correctly rounded division, denormals included.  The sign and
 *     payload of a COMPUTED NaN are unspecified.  For the score see pgt_ext_row below.
 *   - allele frequencies (p1, p2, freq[k]): in [0, 1] at every COUNTED site (both populations have at least minind individuals
 *     there); at a site that is not counted the frequency is never used and may hold anything, NaN included.  pgt_fst_af_reduce_dev
 *     has no counts: every site is counted; a NaN there stays in the rows of the pairs with that population.
 *   - genotypes: any int8 (non-missing is g >= 0, heterozygous g == 1, hetWindow.cpp:78-80); counts (n1, n2, nind[k]) and minind:
 *     any int32, compared as signed integers (dxyWindow.cpp:381).
 *   - the K-population entry points (pgt_dxy_pops / fst_pops / fst_hudson_pops / pi_pops / dstat_pops / fd_pops / f3_pops / pbs_pops / pbs_hudson_pops / f4_pops / f4ratio_pops _reduce_dev;
 *     tests/test_special_values_pops.py, for f3_pops tests/test_special_values_f3.py, for pbs_pops / pbs_hudson_pops tests/test_special_values_pbs.py,
 *     for f4_pops tests/test_special_values_f4.py, for f4ratio_pops tests/test_special_values_f4ratio.py): a NaN or an infinity in ONE population's frequency at a COUNTED site reaches exactly the
 *     rows (and genome-wide lines) of the items — pairs, trios, the population itself — that hold that population, and of them
 *     exactly the windows that hold the site, with the value the per-site definition gives on the IEEE operands, every operation
 *     rounded on its own (for pgt_fd_pops_reduce_dev the definition's comparisons are all false with a NaN, so NaN in P2 leaves
 *     fd_den finite and NaN in P1 leaves fdm_den finite); every other row keeps its bits.  Sums add by IEEE 754 in an
 *     unspecified order: a NaN term gives NaN, +inf and -inf together NaN, infinities of one sign that infinity.  Frequencies
 *     at the edge of [0, 1] (-0.0, denormals, 1 - 2^-53, 0, 1) are ordinary values; sums may be denormal; a ratio is 0 where its
 *     denominator sum is 0.  Counts and minind are any int32, compared signed; where the counts are values (fst_pops,
 *     fst_hudson_pops, pi_pops, pbs_pops, pbs_hudson_pops) any count from minind (>= 1) to INT32_MAX is converted exactly.
 *     The Weir-Cockerham values (fst_pops, pbs_pops) are an identity of their definition evaluated with one reciprocal per pair:
 *     at a counted site with an INFINITE frequency a and a + b are non-finite (NaN or an infinity; which one is unspecified), so
 *     a window that holds such a site and no NaN has non-finite sums for the pairs with that population, and a window that holds
 *     a NaN frequency has NaN; Hudson's values are the definition's own operations (num = +inf, den = NaN there).  pgt_dxy_pops_reduce_dev takes
 *     minind < 1 as well; a site beyond n, padded into the last tile, never counts, whatever minind is.
 *   - pgt_dstat_jackknife_dev: a block's weight is any u32 (pgt_dstat_row.n); their sum is kept in u64 and is exact in the f64
 *     arithmetic while it stays below 2^53.
 */
#ifndef PGTWIN_H
#define PGTWIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 5): the i32 count columns of the dxy entry points must be 16-byte aligned (8 sufficed); pgt_tree_bytes(PGT_STAT_DXY)
 * includes the build waves' partial sums; pgt_extreme_reduce_cols, PGT_TOK_CHR_PREFIX and 12 tokens per line (added under
 * version 4 in round 4) are part of it.  A binding written for one version never calls a library of another. */
/* 6 (round 6): pgt_prepare_host_io added; the host-buffer entry points stage their uploads through a per-context pinned
 * ring and keep a per-context workspace (no argument list changed).
 * Still 6: pgt_dxy_pops_tree_bytes / pgt_dxy_pops_reduce_dev / pgt_dxy_pops_reduce added (additive: nothing that existed changed).
 * Still 6: pgt_align_segments / pgt_align_workspace_bytes / pgt_sites_align / pgt_gather_dev added (additive as well).
 * Still 6: pgt_fst_total, pgt_fst_pops_tree_bytes / pgt_fst_pops_reduce_dev / pgt_fst_pops_reduce added (additive as well).
 * Still 6: pgt_pi_pops_tree_bytes / pgt_pi_pops_reduce_dev / pgt_pi_pops_reduce added (additive as well).
 * Still 6: pgt_fst_hudson_pops_tree_bytes / pgt_fst_hudson_pops_reduce_dev / pgt_fst_hudson_pops_reduce added (additive as well).
 * Still 6: pgt_dstat_row, pgt_dstat_total, pgt_dstat_pops_tree_bytes / pgt_dstat_pops_reduce_dev / pgt_dstat_pops_reduce added (additive as well).
 * Still 6: pgt_dstat_jack, pgt_dstat_jackknife_work_bytes / pgt_dstat_jackknife_dev / pgt_dstat_jackknife added (additive as well).
 * Still 6: pgt_fd_row, pgt_fd_total, pgt_fd_pops_tree_bytes / pgt_fd_pops_reduce_dev / pgt_fd_pops_reduce added (additive as well).
 * Still 6: pgt_f3_row, pgt_f3_total, pgt_f3_jack, pgt_f3_pops_tree_bytes / pgt_f3_pops_reduce_dev / pgt_f3_pops_reduce and
 *          pgt_f3_jackknife_work_bytes / pgt_f3_jackknife_dev / pgt_f3_jackknife added (additive as well).
 * Still 6: pgt_pbs_row, pgt_pbs_total, pgt_pbs_pops_work_bytes / pgt_pbs_pops_reduce_dev / pgt_pbs_hudson_pops_reduce_dev /
 *          pgt_pbs_pops_reduce / pgt_pbs_hudson_pops_reduce added (additive as well).
 * Still 6: pgt_f4_row, pgt_f4_total, pgt_f4_jack, pgt_f4_pops_tree_bytes / pgt_f4_pops_reduce_dev / pgt_f4_pops_reduce and
 *          pgt_f4_jackknife_work_bytes / pgt_f4_jackknife_dev / pgt_f4_jackknife added (additive as well).
 * Still 6: pgt_f4ratio_row, pgt_f4ratio_total, pgt_f4ratio_jack, pgt_f4ratio_pops_tree_bytes / pgt_f4ratio_pops_reduce_dev /
 *          pgt_f4ratio_pops_reduce and pgt_f4ratio_jackknife_work_bytes / pgt_f4ratio_jackknife_dev / pgt_f4ratio_jackknife
 *          added (additive as well).
 * Still 6: pgt_pbs_jack, pgt_pbs_jackknife_work_bytes / pgt_pbs_jackknife_dev / pgt_pbs_jackknife added (additive as well). */
#define PGT_ABI_VERSION 6

enum {
    PGT_OK = 0,
    PGT_EARG = 1,     /* bad argument (NULL, S>W, misaligned device pointer, ...) */
    PGT_ECAP = 2,     /* output capacity too small; *n_out holds the required count */
    PGT_EDEVICE = 3,  /* HIP error / no gfx950 device */
    PGT_EDOMAIN = 4,  /* input outside the reference's defined domain */
    PGT_ENOMEM = 5
};

typedef struct pgt_ctx pgt_ctx;

/* One window = one call of the reference's calcWindow.
 * flags bit0 (PGT_WIN_COORDS): start/end are given here (dxy bp mode: bp-slot coordinates,
 * dxyWindow.cpp:347,367,389); otherwise the reduce fills them from pos[lo], pos[hi-1]
 * (fstWindow.cpp:71-72). */
#define PGT_WIN_COORDS 1u
typedef struct {
    uint64_t lo, hi;    /* global site index range [lo,hi) reduced by this window; lo==hi allowed */
    uint32_t label_run; /* chromosome run whose name labels the row */
    uint32_t flags;
    uint32_t start, end;
} pgt_win;

typedef struct { /* fstWindow.cpp:88 row: chr start end mid fst nsites */
    uint32_t start, end, mid, n;
    double fst;        /* bsum != 0 ? asum/bsum : 0   (fstWindow.cpp:85) */
    double asum, bsum; /* the two window sums, full precision */
} pgt_fst_row;

typedef struct { /* hetWindow.cpp:87 row: chr start end mid h nonmissing */
    uint32_t start, end, mid, nonmissing;
    uint32_t nhet, pad_;
    double h; /* nonmissing ? nhet/nonmissing : 0   (hetWindow.cpp:84) */
} pgt_het_row;

typedef struct { /* dxyWindow.cpp:190 row: chr start end dxy neffective nskip */
    uint32_t start, end, neff, nskip;
    double sum;
} pgt_dxy_row;

typedef struct { /* dxyWindow.cpp:429-433 genome-wide line */
    double sum;
    uint64_t neff, nskip;
} pgt_dxy_total;

typedef struct { /* genomeFst (betaAFOutlier.R:440-446) of one pair over its counted sites: fst = asum / bsum */
    double asum, bsum;
    uint64_t neff, nskip;
} pgt_fst_total;

typedef struct { /* ABBA-BABA window row of one trio ((i,j),k) against the outgroup: pgt_dstat_pops_reduce_dev */
    uint32_t start, end, mid, n;
    double d;                /* (abba + baba) != 0 ? (abba - baba) / (abba + baba) : 0   Patterson's D */
    double bbaa, abba, baba; /* the three window sums, full precision */
} pgt_dstat_row;

typedef struct { /* the three sums of one trio over all its counted sites */
    double bbaa, abba, baba;
    uint64_t neff, nskip;
} pgt_dstat_total;

typedef struct { /* f_d / f_dM window row of one trio ((i,j),k) against the outgroup: pgt_fd_pops_reduce_dev (56 bytes) */
    uint32_t start, end, mid, n;
    double fd;                   /* fd_den != 0 ? num / fd_den : 0     f_d (Martin et al. 2015), reported whatever its sign */
    double fdm;                  /* fdm_den != 0 ? num / fdm_den : 0   f_dM (Malinsky et al. 2015) */
    double num, fd_den, fdm_den; /* the three window sums, full precision */
} pgt_fd_row;

typedef struct { /* the three sums of one trio over all its counted sites (40 bytes) */
    double num, fd_den, fdm_den;
    uint64_t neff, nskip;
} pgt_fd_total;

typedef struct { /* block jackknife of one trio and topology: pgt_dstat_jackknife_dev (48 bytes) */
    double d, d_jack, se, z; /* D of all used blocks, its jackknife estimate, standard error, d_jack / se */
    uint64_t n_sites;        /* counted sites of the used blocks */
    uint32_t n_blocks, pad_; /* used blocks (rows with n > 0) */
} pgt_dstat_jack;

typedef struct { /* f3 window row of one trio (i, j, k), each population as the target: pgt_f3_pops_reduce_dev (48 bytes) */
    uint32_t start, end, mid, n;
    double reserved_;       /* +0.0 */
    double f3_i, f3_j, f3_k; /* the three window SUMS, full precision, at the offsets of pgt_dstat_row's bbaa / abba / baba:
                                sum / n is f3(i; j, k), f3(j; i, k), f3(k; i, j) of the window (the caller divides) */
} pgt_f3_row;

typedef struct { /* the three sums of one trio over all its counted sites (40 bytes) */
    double f3_i, f3_j, f3_k;
    uint64_t neff, nskip;
} pgt_f3_total;

typedef struct { /* block jackknife of one trio and target: pgt_f3_jackknife_dev (48 bytes) */
    double f3, f3_jack, se, z; /* f3 of all used blocks, its jackknife estimate, standard error, f3_jack / se */
    uint64_t n_sites;          /* counted sites of the used blocks */
    uint32_t n_blocks, pad_;   /* used blocks (rows with n > 0) */
} pgt_f3_jack;

typedef struct { /* f4 window row of one quartet (i, j, k, l) in its three pairings: pgt_f4_pops_reduce_dev (48 bytes) */
    uint32_t start, end, mid, n;
    double reserved_;                    /* +0.0 */
    double f4_ij_kl, f4_ik_jl, f4_il_jk; /* the three window SUMS, full precision, at the offsets of pgt_f3_row's f3_i / f3_j /
                                            f3_k: sum / n is f4(i,j; k,l), f4(i,k; j,l), f4(i,l; j,k) of the window (the caller divides) */
} pgt_f4_row;

typedef struct { /* the three sums of one quartet over all its counted sites (40 bytes) */
    double f4_ij_kl, f4_ik_jl, f4_il_jk;
    uint64_t neff, nskip;
} pgt_f4_total;

typedef struct { /* block jackknife of one quartet and pairing: pgt_f4_jackknife_dev (48 bytes, the layout of pgt_f3_jack) */
    double f4, f4_jack, se, z; /* f4 of all used blocks, its jackknife estimate, standard error, f4_jack / se */
    uint64_t n_sites;          /* counted sites of the used blocks */
    uint32_t n_blocks, pad_;   /* used blocks (rows with n > 0) */
} pgt_f4_jack;

typedef struct { /* f4-ratio window row of one middle triple (i, j, k) between A and O: pgt_f4ratio_pops_reduce_dev (48 bytes) */
    uint32_t start, end, mid, n;
    double reserved_;          /* +0.0 */
    double g_ij, g_ik, g_jk;   /* the three window SUMS of (p_A - p_O)(p_x - p_y), full precision, at the offsets of pgt_f4_row's
                                  sums: f4(A,O; i,j), f4(A,O; i,k), f4(A,O; j,k) times n.  The six ratios are the caller's division */
} pgt_f4ratio_row;

typedef struct { /* the three sums of one middle triple over all its counted sites (40 bytes) */
    double g_ij, g_ik, g_jk;
    uint64_t neff, nskip;
} pgt_f4ratio_total;

typedef struct { /* block jackknife of one admixture proportion: pgt_f4ratio_jackknife_dev (48 bytes, the layout of pgt_f4_jack) */
    double alpha, alpha_jack, se, z; /* alpha of all used blocks, its jackknife estimate, standard error, alpha_jack / se */
    uint64_t n_sites;                /* counted sites of the used blocks */
    uint32_t n_blocks, pad_;         /* used blocks (rows with n > 0) */
} pgt_f4ratio_jack;

typedef struct { /* population-branch-statistic window row of one trio (i, j, k): pgt_pbs_pops_reduce_dev (88 bytes) */
    uint32_t start, end, mid, n;    /* offsets 0, 4, 8, 12 */
    double pbs_i, pbs_j, pbs_k;     /* offsets 16, 24, 32: PBS with i, j, k as the focal population, from the six sums below */
    double num_ij, num_ik, num_jk;  /* offsets 40, 48, 56: the FST numerators of the trio's pairs over the TRIO's counted sites */
    double den_ij, den_ik, den_jk;  /* offsets 64, 72, 80: the FST denominators over the same sites; fst_xy = num_xy / den_xy */
} pgt_pbs_row;

typedef struct { /* the same nine doubles of one trio over all its counted sites (88 bytes) */
    double pbs_i, pbs_j, pbs_k;     /* offsets 0, 8, 16 */
    double num_ij, num_ik, num_jk;  /* offsets 24, 32, 40 */
    double den_ij, den_ik, den_jk;  /* offsets 48, 56, 64 */
    uint64_t neff, nskip;           /* offsets 72, 80 */
} pgt_pbs_total;

typedef struct { /* block jackknife of PBS or PBSn1 of one trio and focal population: pgt_pbs_jackknife_dev (48 bytes, the layout of pgt_f4_jack) */
    double stat, stat_jack, se, z; /* the statistic of all used blocks, its jackknife estimate, standard error, stat_jack / se */
    uint64_t n_sites;              /* counted sites of the used blocks */
    uint32_t n_blocks, pad_;       /* used blocks (rows with n > 0) */
} pgt_pbs_jack;

/* ---- context ------------------------------------------------------------------------- */
/* device: HIP ordinal, or -1 for the current device.  Fails (NULL, message via
 * pgt_last_error(NULL)) when no HIP device is usable. */
pgt_ctx *pgt_open(int device);
void pgt_close(pgt_ctx *ctx);
const char *pgt_last_error(const pgt_ctx *ctx);
int pgt_abi_version(void);
/* Optional: allocate the pinned staging ring of the host-buffer entry points (pgt_*_reduce with host columns) now
 * (~15 ms of hipHostMalloc + the runtime's one-time 30 … 60 ms set-up of the first copies of a process) instead of inside the
 * first such call — the retained hosts call it on the thread that opens the device, beside the text parse.
 * expected_column_bytes: what the caller expects to upload per call (0 = unknown); below 32 MiB uploads do not take the ring
 * and it is not allocated (only the set-up is paid).  Replaces nothing in the reference (its calcWindow reads the caller's
 * buffer in place, fstWindow.cpp:76-83); it exists because the columns have to cross PCIe here. */
int pgt_prepare_host_io(pgt_ctx *ctx, uint64_t expected_column_bytes);

/* ---- window tables (host, O(#windows + #runs), no device needed) ------------------------ */
/* Site-count windows of fstWindow / hetWindow / dxyWindow -fixedsite 1: the emission rules of
 * fstWindow.cpp:132-138,150-152 applied to the chromosome run lengths (run_len[r] = number of
 * consecutive sites carrying the same chromosome name).  Requires 1 <= S <= W (Q9).
 * out may be NULL (count only).  Returns PGT_ECAP when cap < *n_out. */
int pgt_build_windows_sites(const uint64_t *run_len, size_t n_runs, uint32_t W, uint32_t S,
                            pgt_win *out, size_t cap, size_t *n_out);

/* Base-pair windows of dxyWindow (-fixedsite 0): the slot machine of dxyWindow.cpp:334-378,
 * 407-426 over bp slots 1..chr_len of every run; pos (host pointer, n sites, strictly
 * increasing inside a run) locates the data sites of each window.  chr_len[r] is the -sizefile
 * length of run r's chromosome.  Rows carry PGT_WIN_COORDS. */
int pgt_build_windows_bp(const uint32_t *pos, const uint64_t *run_len, const uint32_t *chr_len,
                         size_t n_runs, uint32_t W, uint32_t S, pgt_win *out, size_t cap,
                         size_t *n_out);

/* ---- reductions, host buffers (copy in, reduce on the GPU, copy out; synchronous) ------- */
int pgt_fst_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b, uint64_t n,
                   const pgt_win *win, uint64_t n_win, pgt_fst_row *out);
int pgt_het_reduce(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n,
                   const pgt_win *win, uint64_t n_win, pgt_het_row *out);
/* tot may be NULL.  n_win may be 0 (global only: dxyWindow -winsize 0 -fixedsite 1). */
int pgt_dxy_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2,
                   const int32_t *n1, const int32_t *n2, uint64_t n, int minind,
                   const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot);

/* ---- reductions, device-resident columns (asynchronous on `stream`) --------------------- */
/* Every pointer is a DEVICE pointer on ctx's device; the f64, i32 (n1, n2) and i8 columns must be 16-byte
 * aligned (they are read by 16-byte loads; the i32 columns since round 5 — 8 bytes sufficed before).
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).  `tree` is caller
 * workspace of at least pgt_tree_bytes(stat, n) bytes, 256-byte aligned: it receives the
 * radix-64 range tree and may be reused by later calls.
 * ABI 4: every row output carries its CAPACITY in bytes (`out_bytes`, right after the pointer, as
 * `tree_bytes` follows `tree`): a call whose rows would not fit returns PGT_EARG before anything is
 * launched.  In the multi-GPU peer mode `out` points into ANOTHER GPU's row buffer (pgt_rowbuf_open),
 * where an overrun would be a silent cross-device write. */
enum { PGT_STAT_FST = 0, PGT_STAT_HET = 1, PGT_STAT_DXY = 2, PGT_STAT_EXT = 3 };
size_t pgt_tree_bytes(int stat, uint64_t n_sites);

int pgt_fst_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b,
                       uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out,
                       size_t out_bytes, void *tree, size_t tree_bytes, void *stream);
int pgt_het_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n,
                       const pgt_win *win, uint64_t n_win, pgt_het_row *out, size_t out_bytes,
                       void *tree, size_t tree_bytes, void *stream);
/* tot: device pointer to one pgt_dxy_total (the genome-wide line, dxyWindow.cpp:382-385,429-433), or NULL.  Its counts are
 * exact; its sum is added from one partial sum per build wave, in wave order — a function of n alone (the build grid is static),
 * within 1e-15 relative of any other order of the same additions. */
int pgt_dxy_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2,
                       const int32_t *n1, const int32_t *n2, uint64_t n, int minind,
                       const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, size_t out_bytes,
                       pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream);

/* dxyWindow + hetWindow of two genotype columns over ONE position column and ONE window table
 * (BASELINE config 3): one build launch streams all six columns (26 B/site), one query launch
 * answers the three tables.  tree must hold pgt_tree_bytes(PGT_STAT_DXY, n) +
 * 2 * pgt_tree_bytes(PGT_STAT_HET, n) bytes.  Rows equal those of the separate calls bit for bit.
 * het_out_bytes is the capacity of EACH of the two genotype tables. */
int pgt_dxy_het_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2,
                           const int32_t *n1, const int32_t *n2, const int8_t *g1, const int8_t *g2,
                           uint64_t n, int minind, const pgt_win *win, uint64_t n_win,
                           pgt_dxy_row *dxy_out, size_t dxy_out_bytes, pgt_dxy_total *tot,
                           pgt_het_row *het_out1, pgt_het_row *het_out2, size_t het_out_bytes,
                           void *tree, size_t tree_bytes, void *stream);

/* Batched population pairs sharing one position column and one window table (BASELINE
 * config 5): a[p], b[p] are HOST arrays of n_pairs DEVICE column pointers; out holds
 * n_pairs * n_win rows, pair-major; tree holds n_pairs trees (n_pairs * pgt_tree_bytes). */
int pgt_fst_reduce_pairs_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *a,
                             const double *const *b, uint32_t n_pairs, uint64_t n,
                             const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes,
                             void *tree, size_t tree_bytes, void *stream);

/* ---- allele-frequency front end ------------------------------------------ */
/* Population allele frequencies -> Reynolds / Weir-Cockerham variance components exactly as WCFst()
 * of the reference's betaAFOutlier.R:400-418 (per site a and a+b: the two columns fstWindow reads),
 * then fstWindow's window statistic Σa / Σ(a+b) (fstWindow.cpp:76-85), for ALL pairs i<j of n_pops
 * populations in one pass over the frequency columns (8 B/site/population instead of 16 B/site/pair).
 *   freq   host array of n_pops DEVICE pointers: f64 allele frequency per site, 16-byte aligned
 *   nsamp  host array of n_pops diploid sample sizes (the R arguments n1, n2)
 *   out    n_pairs * n_win rows, pair-major, pairs ordered (0,1),(0,2),..,(0,n_pops-1),(1,2),..;
 *          asum = Σa, bsum = Σ(a+b), n = sites in the window
 *   tree   pgt_af_tree_bytes(n_pops, n) bytes.    2 <= n_pops <= 8.
 * Parity note: the reference side is an R function with no runnable oracle in this image; the rows
 * are checked against a literal C restatement of those lines (oracle/, parity unpinned). */
size_t pgt_af_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_fst_af_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq, const double *nsamp,
                          uint32_t n_pops, uint64_t n, const pgt_win *win, uint64_t n_win, pgt_fst_row *out,
                          size_t out_bytes, void *tree, size_t tree_bytes, void *stream);

/* ---- dxy of all population pairs from per-population columns ----------------------------------- */
/* dxyWindow's window rows for ALL pairs i<j of n_pops populations over ONE position column and ONE window table, in one
 * pass over each population's own columns (12 B/site/population) instead of one pgt_dxy_reduce_dev per pair (24 B/site/pair).
 *   pos    DEVICE pointer, u32 position per site; may be NULL only when there is no window (n_win == 0) or no site
 *   freq   host array of n_pops DEVICE pointers: f64 allele frequency per site (in [0,1], as the MAF ingest admits), 16-byte aligned
 *   nind   host array of n_pops DEVICE pointers: i32 individuals with data per site, 16-byte aligned
 *   out    n_pairs * n_win rows, pair-major, pairs ordered (0,1),(0,2),..,(0,n_pops-1),(1,2),.. as for pgt_fst_af_reduce_dev
 *   tot    DEVICE array of n_pairs genome-wide lines, or NULL; n_win == 0 with tot: the global-only form (-winsize 0 -fixedsite 1)
 *   tree   pgt_dxy_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 2 ... 8).    2 <= n_pops <= 8, n < 2^32.
 * Per pair the semantics are those of dxyWindow.cpp:172-209,381-385 as pgt_dxy_reduce_dev implements them on the pair's columns:
 * a site counts when both populations have at least minind individuals and then adds p_i(1-p_j) + p_j(1-p_i), rounded
 * exactly as there (a one-site window has the same bits); neff and coordinates are equal, sums agree to the last bits (the
 * tree has 512-site leaves here, 128-site ones there); nskip is (sites of the window) - neff: every site of a range is a data
 * site.  The pointer arrays are read before the call returns (the columns are kernel arguments: the call can be captured
 * into a graph).  pgt_set_max_window is honoured; pgt_set_window_step is ignored (always one wave per window; rows do not
 * depend on the window table's other rows).  Parity note: held to the two-population path and the CPU restatement (oracle/);
 * dxy parity itself is unpinned.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the n_pairs totals in host memory. */
size_t pgt_dxy_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_dxy_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                            const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                            const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, size_t out_bytes,
                            pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_dxy_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                        const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                        const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot);

/* ---- FST of all population pairs from per-population MAF columns ------------------------------ */
/* fstWindow's window rows for ALL pairs i<j of n_pops populations from each population's own (freq, nInd) columns — what K
 * ANGSD .mafs files hold — over ONE position column and ONE window table, in one pass (12 B/site/population).  Unlike
 * pgt_fst_af_reduce_dev (one scalar sample size per population) the sample sizes are the PER-SITE nInd, and a site counts
 * for a pair only when both populations have at least minind individuals there:
 *   counting   nind_i[s] >= minind && nind_j[s] >= minind (dxyWindow.cpp:381, as pgt_dxy_pops_reduce_dev); minind >= 1 is
 *              required (PGT_EARG otherwise): it makes npool >= 2 and n1 n2 > 0 at every counted site
 *   per site   the two columns of WCFst() (betaAFOutlier.R:405-417) with n1 = nind_i[s], n2 = nind_j[s], f1 = freq_i[s],
 *              f2 = freq_j[s]: npool = n1+n2; alpha_k = 2 f_k (1-f_k); b = (n1 alpha1 + n2 alpha2)/(npool-1);
 *              a = (4 n1 (f1-fpool)^2 + 4 n2 (f2-fpool)^2 - b)/(4 n1 n2/npool), evaluated as (f1-f2)^2 - b npool/(4 n1 n2)
 *   row        asum = Σa, bsum = Σ(a+b) over the window's counted sites, n = their number (nskip = (hi - lo) - n),
 *              fst = bsum != 0 ? asum/bsum : 0 (fstWindow.cpp:85); start / end / mid as pgt_fst_reduce_dev fills them
 *   tot        DEVICE array of n_pairs genome-wide lines (genomeFst, betaAFOutlier.R:440-446, over the counted sites), or
 *              NULL; n_win == 0 with tot: the global-only form
 *   tree       pgt_fst_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 2 ... 8).    2 <= n_pops <= 8, n < 2^32.
 * Arguments, alignment, the order of the pairs and of the rows, graph capture and the hints: those of
 * pgt_dxy_pops_reduce_dev.  Rows of a pair do not depend, bit for bit, on the other populations' columns or on the other
 * rows of the table.  Sums are added in a fixed order (bitwise reproducible); against an exact evaluation of the lines
 * above they stay within 1e-9 relative + 1e-12.  Parity note: the reference side is an R function with no runnable
 * oracle here (parity unpinned, as for pgt_fst_af_reduce_dev); the rows are held to an exact-rational evaluation.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the n_pairs totals in host memory. */
size_t pgt_fst_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_fst_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                            const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                            const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes,
                            pgt_fst_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_fst_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                        const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                        const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot);

/* ---- Hudson's FST of all population pairs from per-population MAF columns ---------------------------- */
/* The rows of pgt_fst_pops_reduce_dev with the other estimator: Hudson's FST as a RATIO OF AVERAGES (Hudson, Slatkin &
 * Maddison 1992; Bhatia, Patterson, Sankararaman & Price 2013, eq. 10, who recommend it for populations of unequal, per-site
 * varying sample size — what MAF files from low-coverage data hold).  Same columns, window table, pair order, row and total
 * types as pgt_fst_pops_reduce_dev; a row's asum is the window's Σ numerator, its bsum the Σ denominator.  Per site the
 * denominator is dxy (pgt_dxy_pops_reduce_dev's term, bit for bit) and the numerator the net divergence dxy - (pi_i + pi_j)/2
 * with pi as pgt_pi_pops_reduce_dev defines it: (p1-p2)^2 - h1 - h2 = D - [p1(1-p1)+h1] - [p2(1-p2)+h2].
 * It has NO counterpart in the reference (WCFst() is its only frequency-based FST): the definition below is the contract.
 * For pair (i, j), i < j, and site s:
 *   counting   nind_i[s] >= minind && nind_j[s] >= minind   (signed int32 compare; minind >= 1 required,
 *              PGT_EARG otherwise: it makes 2 nind - 1 >= 1 at every counted site)
 *   per site   p1 = freq_i[s], p2 = freq_j[s]; for k in {1, 2}, every operation rounded on its own, no contraction:
 *                  m_k = 2.0 * (double)nind_k[s] - 1.0          haploid sample size minus one
 *                  h_k = (p_k * (1.0 - p_k)) / m_k              ONE correctly rounded IEEE division per population and site
 *              d   = p1 - p2
 *              num = (d * d - h_1) - h_2                        h_1 is population i's, h_2 population j's
 *              den = p1 * (1.0 - p2) + p2 * (1.0 - p1)          dxy_site_pred's roundings, bit for bit
 *              a site that is not counted is selected away, never multiplied (its frequency may be NaN, its nind 0 or negative)
 *   row        pgt_fst_row: asum = Σ num, bsum = Σ den over the window's counted sites, each from +0.0; n = their number
 *              (nskip = (hi - lo) - n); fst = bsum != 0 ? asum / bsum : 0; start / end / mid as pgt_fst_pops_reduce_dev
 *   tot        pgt_fst_total per pair: the same sums over all counted sites, from one partial per build wave in wave order
 * A one-site window carries exactly the bits of `num`, `den` and `num/den` above.
 *   tree       pgt_fst_hudson_pops_tree_bytes(n_pops, n) = pgt_fst_pops_tree_bytes(n_pops, n): one buffer may serve both
 *              entry points in turn, never two calls in flight.    2 <= n_pops <= 8, n < 2^32.
 * Arguments, alignment, refusals (each names its argument; nothing is launched), the order of the pairs and of the rows,
 * graph capture and the hints: those of pgt_fst_pops_reduce_dev (pgt_set_max_window honoured, pgt_set_window_step ignored).
 * Rows of a pair do not depend, bit for bit, on the other populations' columns or on the other rows of the table.  Sums are
 * added in a fixed order (bitwise reproducible); against an exact evaluation of the lines above they stay within 1e-9
 * relative + 1e-12.  Parity: none to pin; held to this definition, to an exact-rational fixture
 * (tests/golden/hudson_exact.json) and to the dxy and pi entry points.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the n_pairs totals in host memory. */
size_t pgt_fst_hudson_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_fst_hudson_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                                   const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                                   const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes,
                                   pgt_fst_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_fst_hudson_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                               const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                               const pgt_win *win, uint64_t n_win, pgt_fst_row *out, pgt_fst_total *tot);

/* ---- nucleotide diversity (pi) per population from per-population MAF columns --------------------- */
/* Windowed within-population nucleotide diversity of each of n_pops populations from its own (freq, nInd) columns — the
 * columns pgt_dxy_pops_reduce_dev and pgt_fst_pops_reduce_dev read — over ONE position column and ONE window table, in one
 * pass (12 B/site/population).  The statistic dxy and FST scans are read against: net divergence is dxy - (pi_1 + pi_2)/2.
 * It has NO counterpart in the reference (none of its tools computes pi): the definition below is the contract.
 *   counting   nind[s] >= minind, compared as signed int32; minind >= 1 is required (PGT_EARG otherwise, the rule of
 *              pgt_fst_pops_reduce_dev): it makes 2 nind - 1 >= 1 at every counted site
 *   per site   with p = freq[s], dn = (double)nind[s] (exact), every operation rounded on its own:
 *                  c = (2.0*dn) / (2.0*dn - 1.0)      one correctly rounded IEEE division: the finite-sample factor
 *                  h = (2.0*p) * (1.0 - p)
 *                  pi = h * c
 *              a site that is not counted is selected away, never multiplied: its frequency may be NaN
 *   row        pgt_dxy_row: sum = Σ pi over the window's counted sites, starting from +0.0 (like dxyWindow.cpp:190 the row
 *              carries the SUM: divide by neff or by the window length); neff = the counted sites; nskip = (hi - lo) - neff;
 *              start / end as pgt_dxy_reduce_dev fills them (PGT_WIN_COORDS honoured).  A one-site window has exactly the bits
 *              of `pi` above
 *   out        n_pops * n_win rows, population-major
 *   tot        DEVICE array of n_pops genome-wide lines (pgt_dxy_total: exact counts; the sum added from one partial per
 *              build wave, in wave order, as for pgt_dxy_reduce_dev), or NULL; n_win == 0 with tot: the global-only form
 *   tree       pgt_pi_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 1 ... 8).    1 <= n_pops <= 8, n < 2^32.
 * Arguments, alignment (freq[k], nind[k] 16-byte aligned), refusals (each names its argument; nothing is launched) and graph
 * capture (the pointer arrays are read before the call returns) are those of pgt_dxy_pops_reduce_dev.  Unlike the all-pairs
 * calls, a population's predicate is its own, so the generic range tree answers the windows: pgt_set_max_window,
 * pgt_set_window_step and pgt_set_typical_window are ALL honoured, with the strategies of pgt_dxy_reduce_dev (one wave per
 * window, the sliding query, the group query).  A population's rows do not depend, bit for bit, on the other populations
 * in the call (n_pops = 1 gives the same bits), and a row does not depend on the other rows of the table under one set of
 * hints.  Sums are added in a fixed order (bitwise reproducible); against an exact evaluation of the lines above they stay
 * within 1e-9 relative + 1e-12.  Parity: to this definition and to an exact-rational fixture (tests/golden/pi_exact.json).
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the n_pops totals in host memory; hints
 * that are not set are derived from the table, as in the other host-buffer calls. */
size_t pgt_pi_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_pi_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                           const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                           const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, size_t out_bytes,
                           pgt_dxy_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_pi_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                       const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                       const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, pgt_dxy_total *tot);

/* ---- ABBA-BABA (Patterson's D) of all ingroup trios against an outgroup, from per-population MAF columns -------------- */
/* The window rows of an introgression scan (Green et al. 2010; Durand et al. 2011; Martin et al. 2015; what Dsuite's Dtrios /
 * Dinvestigate compute from frequencies) for ALL trios of the ingroup populations at once, from each population's own
 * (freq, nInd) columns — the input of pgt_fst_pops_reduce_dev — over ONE position column and ONE window table, in one pass
 * (12 B/site/population).  It has NO counterpart in the reference: the definition below is the contract.
 * n_pops = K populations, 4 <= K <= 7.  The LAST population (index K-1) is the outgroup o, the first K-1 are the ingroup.  A
 * trio is (i, j, k) with i < j < k < K-1; trios are numbered in lexicographic order (0,1,2),(0,1,3),..,(0,1,K-2),(0,2,3),..;
 * there are T = C(K-1, 3) of them: 1 / 4 / 10 / 20 at K = 4 / 5 / 6 / 7.  For trio (i, j, k) and site s:
 *   counting   nind_i[s] >= minind && nind_j[s] >= minind && nind_k[s] >= minind && nind_o[s] >= minind   (signed int32 compare;
 *              minind >= 1 required, PGT_EARG otherwise, as in the other *_pops calls); a site that is not counted is selected
 *              away, never multiplied (its frequencies may be NaN, its counts 0 or negative)
 *   per site   p_x = freq_x[s], q_x = 1.0 - p_x; every operation rounded on its own, no contraction, in exactly this grouping:
 *                  bbaa = (p_i*p_j)*(q_k*q_o) + (q_i*q_j)*(p_k*p_o)
 *                  abba = (q_i*p_j)*(p_k*q_o) + (p_i*q_j)*(q_k*p_o)
 *                  baba = (p_i*q_j)*(p_k*q_o) + (q_i*p_j)*(q_k*p_o)
 *              The second term of each line is the pattern with the roles of the two alleles swapped (Dsuite's form): the three
 *              values do not depend on which allele the columns report, provided all populations report the same one.  (The
 *              four products of an ingroup pair and the four products of (k, o) are computed once per site and shared by every
 *              trio that contains them.)
 *   row        pgt_dstat_row: bbaa / abba / baba = the three sums over the window's counted sites, each from +0.0; n = their
 *              number (nskip = (hi - lo) - n); start / end / mid as pgt_fst_pops_reduce_dev fills them (PGT_WIN_COORDS
 *              honoured); d = (abba + baba) != 0 ? (abba - baba) / (abba + baba) : 0 — Patterson's D for the topology ((i,j),k),
 *              from the row's own three sums with one correctly rounded subtraction, addition and division.  The other two
 *              topologies of the trio follow from the same three sums — ((i,k),j): (bbaa - baba) / (bbaa + baba);
 *              ((j,k),i): (bbaa - abba) / (bbaa + abba) — and are not carried by the row
 *   out        T * n_win rows, trio-major: out[t * n_win + w]
 *   tot        DEVICE array of T pgt_dstat_total (the same sums over all counted sites, from one partial per build wave in wave
 *              order), or NULL; n_win == 0 with tot: the global-only form
 *   tree       pgt_dstat_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 4 ... 7).    4 <= n_pops <= 7, n < 2^32.
 * K = 8 (35 trios, 105 sums per node) is not offered: the running sums and the build's two register sets would not fit a wave.
 * A one-site window carries exactly the bits of `bbaa`, `abba`, `baba` and `d` above.
 * Arguments, alignment, refusals (each names its argument; nothing is launched), graph capture and the hints: those of
 * pgt_fst_pops_reduce_dev (pgt_set_max_window honoured, pgt_set_window_step ignored).  Rows of a trio do not depend, bit for
 * bit, on the populations outside the trio and the outgroup, nor on the other rows of the table.  Sums are added in a fixed
 * order that depends on the site index and the window alone (bitwise reproducible); against an exact evaluation of the lines
 * above they stay within 1e-9 relative + 1e-12.  Parity: none to pin; held to this definition, to an exact-rational fixture
 * (tests/golden/dstat_exact.json) and to a NumPy model (tests/dstat_pops_model.py).  f_d / f_dM of the same trios come from
 * pgt_fd_pops_reduce_dev below; user-chosen trio lists are not computed; block-jackknife standard errors and Z scores come from pgt_dstat_jackknife_dev below, over the rows of a table of
 * disjoint windows (the blocks).
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the T totals in host memory. */
size_t pgt_dstat_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_dstat_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                              const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                              const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, size_t out_bytes,
                              pgt_dstat_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_dstat_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                          const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                          const pgt_win *win, uint64_t n_win, pgt_dstat_row *out, pgt_dstat_total *tot);

/* ---- f_d and f_dM of all ingroup trios against an outgroup ------------------------------------------------------------- */
/* The admixture-proportion statistics to scan windows with where Patterson's D misleads (small windows: high variance, inflated
 * where diversity is low): f_d (Martin, Davey & Jiggins 2015, MBE 32:244) and f_dM (Malinsky et al. 2015, Science 350:1493) —
 * what Dsuite's Dinvestigate prints beside D.  It has NO counterpart in the reference: the definition below is the contract.
 * Populations, trios, their order and the counting predicate are those of pgt_dstat_pops_reduce_dev: the LAST population o is
 * the outgroup; trio (i, j, k), i < j < k < n_pops - 1, in lexicographic order, is read as ((P1 = i, P2 = j), P3 = k); a site
 * counts for a trio iff all four populations have at least minind individuals; a site that is not counted is selected away,
 * never multiplied by 0 (its columns may hold anything).  4 <= n_pops <= 7, minind >= 1, n < 2^32.
 *   per site   p_x = freq_x[s], q_x = 1.0 - p_x; every operation rounded on its own, no contraction; abba and baba exactly the
 *              two lines of pgt_dstat_pops_reduce_dev; in exactly this grouping:
 *                  num  = abba - baba
 *                  H = (p_j >= p_k) ? j : k        L = (p_j <= p_k) ? j : k        the larger / smaller of P2, P3
 *                  G = (p_i >= p_k) ? i : k        S = (p_i <= p_k) ? i : k        the larger / smaller of P1, P3
 *                  B1 = (q_i*p_H)*(p_H*q_o) - (p_i*q_H)*(p_H*q_o)      S(P1, PD, PD, O), PD of {P2,P3}; reported allele derived
 *                  A1 = (p_i*q_L)*(q_L*p_o) - (q_i*p_L)*(q_L*p_o)      the same with the two alleles' roles swapped
 *                  B2 = (p_G*q_j)*(p_G*q_o) - (q_G*p_j)*(p_G*q_o)      -S(PD, P2, PD, O), PD of {P1,P3}
 *                  A2 = (q_S*p_j)*(q_S*p_o) - (p_S*q_j)*(q_S*p_o)      the same, roles swapped
 *                  fd_den  = B1 + A1
 *                  fdm_den = (p_j >= p_i ? B1 : B2) + (p_j <= p_i ? A1 : A2)
 *              The allele-symmetric form of the D lines: each term is the pattern with the reported allele as derived, weighted
 *              by the outgroup's ancestral frequency q_o, plus the same pattern with the alleles' roles swapped, weighted by
 *              p_o.  With a fixed outgroup (p_o 0 or 1) it is Martin's and Malinsky's formula.  Ties need no rule: equal p give
 *              equal q and the products commute, so either choice gives the same bits.  The selects compare the INPUT
 *              frequencies, never the rounded q.  With a NaN frequency at a counted site every comparison is false and
 *              the lines above are evaluated as written ("Values the columns admit"), for that trio's rows only.
 *   row        pgt_fd_row (56 bytes): num / fd_den / fdm_den = the three sums over the window's counted sites, each from +0.0;
 *              n = their number; start / end / mid as pgt_dstat_row's are filled;
 *                  fd = fd_den != 0 ? num / fd_den : 0          fdm = fdm_den != 0 ? num / fdm_den : 0
 *              one correctly rounded division of the row's own sums each.  num is the sum of per-site differences, not the
 *              difference of the D row's two sums: the two agree within rounding, not in bits.
 *   out        T * n_win rows, trio-major: out[t * n_win + w]
 *   tot        DEVICE array of T pgt_fd_total (40 bytes: the same three sums over all counted sites, neff, nskip), or NULL
 *   tree       pgt_fd_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 4 ... 7): the size pgt_dstat_pops_tree_bytes gives,
 *              so one buffer serves both calls in turn.
 * f_d is meant for windows with D >= 0 (gene flow P3 -> P2); the row reports it whatever its sign.
 * f_dM covers both directions (P3 -> P2 positive, P3 -> P1 negative) and lies within +-1.
 * Only the topology ((i,j),k) is computed — f_d is no function of three shared sums as D is — so the order of the columns chooses it.
 * A one-site window carries exactly the bits of `num`, `fd_den` and `fdm_den` above.  Arguments, alignment, refusals (messages
 * begin "pgt_fd_pops_reduce: "), graph capture, hints, bitwise reproducibility and trio isolation: those of
 * pgt_dstat_pops_reduce_dev.  The sums' site terms have both signs: against an exact evaluation a sum stays within
 * 1e-9 * A + 1e-12, A the window's sum of |site term|.  Held to this definition, to an exact-rational fixture
 * (tests/golden/fd_exact.json) and to a NumPy model (tests/fd_pops_model.py).  d_f, f_G / f_hom, the other two topologies, a
 * block jackknife of f_d and K = 8 are not computed.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the T totals in host memory. */
size_t pgt_fd_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_fd_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                           const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                           const pgt_win *win, uint64_t n_win, pgt_fd_row *out, size_t out_bytes,
                           pgt_fd_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_fd_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                       const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                       const pgt_win *win, uint64_t n_win, pgt_fd_row *out, pgt_fd_total *tot);

/* ---- block-jackknife standard error and Z of Patterson's D, all trios and topologies ----------------------------------- */
/* The weighted (delete-m_j) block jackknife of Busing, Meijer & van der Leeden (1999) — the one ADMIXTOOLS and ANGSD's
 * ABBA-BABA use — over the window rows pgt_dstat_pops_reduce_dev wrote.  It has NO counterpart in the reference: the definition
 * below is the contract.
 *   rows     DEVICE pointer to the n_trios x n_win trio-major table rows[t * n_win + w], 16-byte aligned.  Every window of the
 *            table is one block.  The caller guarantees that the windows are DISJOINT (-stepsize >= -winsize); the call cannot
 *            check that and does not.  Only n, bbaa, abba and baba of a row are read.
 *   items    trio t has three items u = 3 t + c, one per topology; each takes (x, y) from a row:
 *                c = 0  ((i,j),k)  x = abba, y = baba
 *                c = 1  ((i,k),j)  x = bbaa, y = baba
 *                c = 2  ((j,k),i)  x = bbaa, y = abba       (the three D's of pgt_dstat_row above)
 *   blocks   block j is USED iff its row has n > 0; m_j = n.  Over the used blocks: g = their number, n = Σ m_j (u64),
 *            X = Σ x_j, Y = Σ y_j.  A row that is not used is selected away, never added: its sums may be NaN
 *   per item all in f64, every operation rounded on its own, no contraction:
 *                ratio(a, b) = (a + b) != 0 ? (a - b) / (a + b) : 0         the row's own convention
 *                theta       = ratio(X, Y)
 *                theta_-j    = ratio(X - x_j, Y - y_j)
 *                h_j         = n / m_j
 *                theta_J     = g * theta - Σ_j (1 - m_j / n) * theta_-j
 *                tau_j       = theta + (h_j - 1) * (theta - theta_-j)        = h_j theta - (h_j - 1) theta_-j, well conditioned
 *                sigma^2     = (1 / g) * Σ_j (tau_j - theta_J)^2 / (h_j - 1)
 *   out      pgt_dstat_jack per item, item-major: d = theta, d_jack = theta_J, se = sqrt(sigma^2),
 *            z = se > 0 ? theta_J / se : NaN, n_blocks = g, n_sites = n, pad_ = 0.
 *            g < 2: d_jack = d, se = z = NaN.  g == 0 (n_win == 0 included): d = d_jack = 0, se = z = NaN.
 *            NaN or infinite sums in a used row reach that item's outputs and no other item's.
 *   work     DEVICE workspace of pgt_dstat_jackknife_work_bytes(n_trios, n_win) bytes (0 for n_trios outside 1 ... 20; 256 at
 *            least otherwise), 16-byte aligned.  Every byte of it that is read is written earlier in the same call.
 * 1 <= n_trios <= 20; the call is not tied to C(K-1, 3): any subset of a table's trios may be passed (whole trios, contiguous).
 * Three dependent reductions (the totals; Σ (1 - m_j/n) theta_-j; the variance sum, which needs theta_J — the last two are NOT
 * merged by expanding the square, which would subtract two large, nearly equal sums) and one closing kernel.  No atomics: a
 * wave sums a fixed run of consecutive 64-block chunks, leaves one partial per phase (at most 1024 per item), and the partials
 * are added in an order that is a function of n_win alone.  The outputs are bitwise reproducible, and an item's outputs are a
 * function, bit for bit, of its own trio's rows alone: not of n_trios, not of the other trios' rows.  Against an exact
 * evaluation of the lines above d, d_jack and se stay within 1e-9 relative + 1e-12 (tests/dstat_jack_model.py).
 * Refusals (PGT_EARG, each names its argument; nothing is launched): NULL rows (with n_win > 0), out or work; rows or work not
 * 16-byte aligned, out not 8-byte aligned; out_bytes below 3 * n_trios * sizeof(pgt_dstat_jack); work_bytes too small;
 * n_trios out of range.  Asynchronous on `stream`; no allocation and no attribute call: it can be captured into a graph.
 * pgt_set_profiling / pgt_last_kernel_ms report the call's time as the query time and 0 as the build time.
 * Host-buffer form: rows and out in host memory; synchronous. */
size_t pgt_dstat_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win);
int pgt_dstat_jackknife_dev(pgt_ctx *ctx, const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios,
                            pgt_dstat_jack *out /* 3 * n_trios, item-major u = 3t + c */, size_t out_bytes,
                            void *work, size_t work_bytes, void *stream);
int pgt_dstat_jackknife(pgt_ctx *ctx, const pgt_dstat_row *rows, uint64_t n_win, uint32_t n_trios, pgt_dstat_jack *out);

/* ---- f3 of ALL trios of the populations, every population of a trio as the target --------------------------------------- */
/* The 3-population statistic f3(C; A, B) = E[(c - a)(c - b)] (Reich et al. 2009; Patterson et al. 2012; treemix's threepop,
 * ADMIXTOOLS' qp3Pop / f3 without the normalisation) with the unbiased estimator of the target's p^2, from each population's own
 * (freq, nInd) columns — the input of pgt_fst_pops_reduce_dev — over ONE position column and ONE window table, in one pass
 * (12 B/site/population).  A significantly negative f3(C; A, B) shows that C is admixed between relatives of A and B; with an
 * outgroup O as the target, f3(O; A, B) measures the drift A and B share.  It has NO counterpart in the reference: the
 * definition below is the contract.
 * n_pops = K populations, 3 <= K <= 6.  ALL populations are equal: there is no outgroup.  A trio is (i, j, k) with
 * i < j < k < K; trios are numbered in lexicographic order (0,1,2),(0,1,3),..,(0,1,K-1),(0,2,3),..; there are T = C(K, 3) of
 * them: 1 / 4 / 10 / 20 at K = 3 / 4 / 5 / 6.  For trio (i, j, k) and site s:
 *   counting   nind_i[s] >= minind && nind_j[s] >= minind && nind_k[s] >= minind   (signed int32 compare; minind >= 1 required,
 *              PGT_EARG otherwise: 2 n - 1 >= 1 wherever a term is used); a site that is not counted is selected away, never
 *              multiplied (its frequencies may be NaN, its counts 0 or negative)
 *   per site   p_x = freq_x[s], n_x = nind_x[s] converted exactly; every operation rounded on its own, no contraction, in
 *              exactly this grouping:
 *                  h_x  = (p_x * (1 - p_x)) / (2*n_x - 1)       per population (the term of pgt_fst_hudson_pops_reduce_dev)
 *                  d_ab = p_a - p_b                              per pair a < b
 *                  s0 = d_ij*d_ik - h_i                          target i:  f3(i; j, k)
 *                  s1 = (-d_ij)*d_jk - h_j                       target j:  f3(j; i, k)
 *                  s2 = d_ik*d_jk - h_k                          target k:  f3(k; i, j)
 *              One division per population and site, one subtraction per pair and site, shared by every trio that holds them.
 *              The three values do not depend on which allele the columns report, provided all populations report the same one
 *              (with frequencies that are multiples of 2^-10, bit for bit).  s0 + s1 = (p_i - p_j)^2 - h_i - h_j up to rounding:
 *              the numerator of pgt_fst_hudson_pops_reduce_dev for the pair (i, j).
 *   row        pgt_f3_row (48 bytes): f3_i / f3_j / f3_k = the three SUMS of s0 / s1 / s2 over the window's counted sites, each
 *              from +0.0; n = their number (nskip = (hi - lo) - n); start / end / mid as pgt_dstat_row's are filled
 *              (PGT_WIN_COORDS honoured); reserved_ = +0.0.  The means are NOT formed: f3 of the window is sum / n, the
 *              caller's division.  The sums sit at the offsets of pgt_dstat_row's bbaa / abba / baba.
 *   out        T * n_win rows, trio-major: out[t * n_win + w]
 *   tot        DEVICE array of T pgt_f3_total (40 bytes: the same three sums over all counted sites, neff, nskip), or NULL;
 *              n_win == 0 with tot: the global-only form
 *   tree       pgt_f3_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 3 ... 6): a node is 3 T doubles and T u32, the node
 *              of pgt_dstat_pops_reduce_dev at one population more.    3 <= n_pops <= 6, n < 2^32.
 * K = 7 (35 trios, 105 sums per node) is not offered: the running sums and the build's two register sets would not fit a wave.
 * A one-site window carries exactly the bits of s0, s1 and s2 above.  Arguments, alignment, refusals (PGT_EARG; messages begin
 * "pgt_f3_pops_reduce: " and name their argument; a refused call launches nothing and writes nothing), graph capture and the
 * hints: those of pgt_dstat_pops_reduce_dev (asynchronous on `stream`, no allocation, no attribute call; pgt_set_max_window
 * honoured, pgt_set_window_step ignored).  Trio isolation: the rows of a trio are a function, bit for bit, of its own three
 * populations' columns and the window alone — not of the other populations, of K, or of the other rows of the table.  Sums are
 * added in a fixed order that depends on the site index and the window alone (bitwise reproducible).  The site terms have both
 * signs: against an exact evaluation a sum stays within 1e-9 * A + 1e-12, A the window's sum of |product| + |h|.  "Values the
 * columns admit" above holds as for the other K-population calls (tests/test_special_values_f3.py).  Held to this definition,
 * to an exact-rational fixture (tests/golden/f3_exact.json) and to a NumPy model (tests/f3_pops_model.py).  f3 normalised by the
 * target's heterozygosity (qp3Pop's default), f4, user-chosen trio lists and K = 7 are not computed; standard errors and Z
 * come from pgt_f3_jackknife_dev below.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the T totals in host memory. */
size_t pgt_f3_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_f3_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                           const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                           const pgt_win *win, uint64_t n_win, pgt_f3_row *out, size_t out_bytes,
                           pgt_f3_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_f3_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                       const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                       const pgt_win *win, uint64_t n_win, pgt_f3_row *out, pgt_f3_total *tot);

/* ---- block-jackknife standard error and Z of f3, all trios and targets -------------------------------------------------- */
/* The block jackknife of pgt_dstat_jackknife_dev above — the same plan, workspace, phases and order of every addition — with a
 * MEAN as the estimator, over the window rows pgt_f3_pops_reduce_dev wrote.
 *   rows     DEVICE pointer to the n_trios x n_win trio-major table, 16-byte aligned; every window is one block; the caller
 *            guarantees that the windows are DISJOINT.  Only n, f3_i, f3_j and f3_k of a row are read.
 *   items    trio t has three items u = 3 t + c, c = 0 / 1 / 2 the target i / j / k; x_j = sum c of block j's row
 *   blocks   block j is USED iff its row has n > 0; m_j = n.  Over the used blocks: g = their number, n = Σ m_j (u64, then f64),
 *            X = Σ x_j.  A row that is not used is selected away, never added: its sums may be NaN
 *   per item all in f64, every operation rounded on its own, no contraction:
 *                mean(a, b)  = b != 0 ? a / b : 0
 *                theta       = mean(X, n)
 *                theta_-j    = mean(X - x_j, n - m_j)
 *            and h_j, theta_J, tau_j and sigma^2 exactly as in pgt_dstat_jackknife_dev
 *   out      pgt_f3_jack per item, item-major: f3 = theta, f3_jack = theta_J, se = sqrt(sigma^2),
 *            z = se > 0 ? theta_J / se : NaN, n_blocks = g, n_sites = n, pad_ = 0.
 *            g < 2: f3_jack = f3, se = z = NaN.  g == 0 (n_win == 0 included): f3 = f3_jack = 0, se = z = NaN.
 *   work     DEVICE workspace of pgt_f3_jackknife_work_bytes(n_trios, n_win) bytes: the value pgt_dstat_jackknife_work_bytes
 *            gives, 16-byte aligned.  Every byte of it that is read is written earlier in the same call.
 * 1 <= n_trios <= 20.  Bitwise reproducible; an item's outputs are a function, bit for bit, of its own trio's rows alone: not of
 * n_trios, not of the other trios' rows.  Against an exact evaluation f3, f3_jack and se stay within 1e-9 relative + 1e-12
 * (tests/f3_jack_model.py).  Z < -3 is the customary threshold for "the target is admixed".
 * Refusals (PGT_EARG, messages begin "pgt_f3_jackknife: " and name their argument; nothing is launched, nothing written): those
 * of pgt_dstat_jackknife_dev.  Asynchronous on `stream`; no allocation and no attribute call: it can be captured into a graph.
 * Host-buffer form: rows and out in host memory; synchronous. */
size_t pgt_f3_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win);
int pgt_f3_jackknife_dev(pgt_ctx *ctx, const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios,
                         pgt_f3_jack *out /* 3 * n_trios, item-major u = 3t + c */, size_t out_bytes,
                         void *work, size_t work_bytes, void *stream);
int pgt_f3_jackknife(pgt_ctx *ctx, const pgt_f3_row *rows, uint64_t n_win, uint32_t n_trios, pgt_f3_jack *out);

/* ---- f4 of ALL quartets of the populations, every quartet in its three pairings ------------------------------------------ */
/* The 4-population statistic f4(A, B; C, D) = E[(a - b)(c - d)] (Reich et al. 2009; Patterson et al. 2012; treemix's fourpop,
 * ADMIXTOOLS' qpDstat in f4mode), the treeness test: its expectation is 0 when ((A,B),(C,D)) is the tree.  It needs no
 * designated outgroup (pgt_dstat_pops_reduce_dev does) and has no finite-sample bias term (f3 has).  From each population's own
 * (freq, nInd) columns — the input of pgt_f3_pops_reduce_dev — over ONE position column and ONE window table, in one pass
 * (12 B/site/population).  It has NO counterpart in the reference: the definition below is the contract.
 * n_pops = K populations, 4 <= K <= 6.  ALL populations are equal.  A quartet is (i, j, k, l) with i < j < k < l < K; quartets
 * are numbered in lexicographic order (0,1,2,3),(0,1,2,4),..,(0,1,3,4),..; there are Q = C(K, 4) of them: 1 / 5 / 15 at
 * K = 4 / 5 / 6.  For quartet (i, j, k, l) and site s:
 *   counting   nind_x[s] >= minind for x = i, j, k and l (signed int32 compare; minind >= 1 required, PGT_EARG otherwise, as
 *              pgt_dstat_pops_reduce_dev refuses it); a site that is not counted is selected away, never multiplied (its
 *              frequencies may be NaN, its counts 0 or negative).  The counts enter through this predicate ONLY.
 *   per site   p_x = freq_x[s]; every operation rounded on its own, no contraction, in exactly this grouping:
 *                  d_ab = p_a - p_b                              per pair a < b, shared by every quartet that holds the pair
 *                  s0 = d_ij * d_kl                              f4(i, j; k, l)
 *                  s1 = d_ik * d_jl                              f4(i, k; j, l)
 *                  s2 = d_il * d_jk                              f4(i, l; j, k)
 *              No division, no bias term.  In real arithmetic s0 - s1 + s2 = 0; the three are stored all the same, so that the
 *              row has the layout and the three items per row of pgt_f3_row.  The three values do not depend on which allele
 *              the columns report, provided all populations report the same one (with frequencies that are multiples of
 *              2^-10, bit for bit).  With an outgroup O as the last population, f4(i, j; k, O) is the numerator of Patterson's D:
 *              baba - abba of pgt_dstat_pops_reduce_dev's trio (i, j, k) = (p_i - p_j)(p_k - p_O).
 *   row        pgt_f4_row (48 bytes): f4_ij_kl / f4_ik_jl / f4_il_jk = the three SUMS of s0 / s1 / s2 over the window's counted
 *              sites, each from +0.0; n = their number (nskip = (hi - lo) - n); start / end / mid as pgt_dstat_row's are filled
 *              (PGT_WIN_COORDS honoured); reserved_ = +0.0.  The means are NOT formed: f4 of the window is sum / n, the
 *              caller's division.  The sums sit at the offsets of pgt_f3_row's f3_i / f3_j / f3_k.
 *   out        Q * n_win rows, quartet-major: out[q * n_win + w]
 *   tot        DEVICE array of Q pgt_f4_total (40 bytes: the same three sums over all counted sites, neff, nskip), or NULL;
 *              n_win == 0 with tot: the global-only form
 *   tree       pgt_f4_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 4 ... 6): a node is 3 Q doubles (s0 of quartet
 *              0 .. Q-1, then s1, then s2) and Q u32.    4 <= n_pops <= 6, n < 2^32.
 * K = 7 (35 quartets, 105 sums per node) is not offered, for the reason pgt_f3_pops_reduce_dev stops at 6.
 * A one-site window carries exactly the bits of s0, s1 and s2 above.  Arguments, alignment, refusals (PGT_EARG; messages begin
 * "pgt_f4_pops_reduce: " and name their argument; a refused call launches nothing and writes nothing), graph capture and the
 * hints: those of pgt_f3_pops_reduce_dev (asynchronous on `stream`, no allocation, no attribute call; pgt_set_max_window
 * honoured, pgt_set_window_step ignored).  Quartet isolation: the rows of a quartet are a function, bit for bit, of its own four
 * populations' columns and the window alone — not of the other populations, of K, or of the other rows of the table.  Sums are
 * added in a fixed order that depends on the site index and the window alone (bitwise reproducible).  The site terms have both
 * signs: against an exact evaluation a sum stays within 1e-9 * A + 1e-12, A the window's sum of |product| (of the same pairing);
 * no bound relative to the value is given.  "Values the columns admit" above holds as for the other K-population calls
 * (tests/test_special_values_f4.py).  Held to this definition, to an exact-rational fixture (tests/golden/f4_exact.json) and to
 * a NumPy model (tests/f4_pops_model.py).  Not computed: user-chosen quartet lists and K = 7; standard errors and Z come
 * from pgt_f4_jackknife_dev below, f4-ratio admixture proportions from pgt_f4ratio_pops_reduce_dev further down.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the Q totals in host memory. */
size_t pgt_f4_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_f4_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                           const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                           const pgt_win *win, uint64_t n_win, pgt_f4_row *out, size_t out_bytes,
                           pgt_f4_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_f4_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                       const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                       const pgt_win *win, uint64_t n_win, pgt_f4_row *out, pgt_f4_total *tot);

/* ---- block-jackknife standard error and Z of f4, all quartets and pairings ---------------------------------------------- */
/* The block jackknife of the MEAN of pgt_f3_jackknife_dev above — the same estimator, arithmetic, plan, workspace, phases and
 * order of every addition — over the window rows pgt_f4_pops_reduce_dev wrote: the same bytes viewed as pgt_f3_row and given
 * to pgt_f3_jackknife_dev yield the same bits.
 *   rows     DEVICE pointer to the n_quartets x n_win quartet-major table, 16-byte aligned; every window is one block; the
 *            caller guarantees that the windows are DISJOINT.  Only n and the three sums of a row are read.
 *   items    quartet q has three items u = 3 q + c, c = 0 / 1 / 2 the pairing (ij;kl) / (ik;jl) / (il;jk); x_j = sum c of
 *            block j's row
 *   blocks, per item: as pgt_f3_jackknife_dev (a row that is not used is selected away, never added: its sums may be NaN)
 *   out      pgt_f4_jack per item, item-major: f4 = theta, f4_jack = theta_J, se = sqrt(sigma^2),
 *            z = se > 0 ? theta_J / se : NaN, n_blocks = g, n_sites = n, pad_ = 0.
 *            g < 2: f4_jack = f4, se = z = NaN.  g == 0 (n_win == 0 included): f4 = f4_jack = 0, se = z = NaN.
 *   work     DEVICE workspace of pgt_f4_jackknife_work_bytes(n_quartets, n_win) bytes (0 for n_quartets outside 1 ... 15): the
 *            value pgt_dstat_jackknife_work_bytes gives, 16-byte aligned.  Every byte of it that is read is written earlier in
 *            the same call.
 * 1 <= n_quartets <= 15.  Bitwise reproducible; an item's outputs are a function, bit for bit, of its own quartet's rows alone:
 * not of n_quartets, not of the other quartets' rows.  Against an exact evaluation f4, f4_jack and se stay within 1e-9
 * relative + 1e-12 (tests/f3_jack_model.py).  |Z| above about 3 rejects the tree ((a,b),(c,d)) of the pairing.
 * Refusals (PGT_EARG, messages begin "pgt_f4_jackknife: " and name their argument; nothing is launched, nothing written): those
 * of pgt_dstat_jackknife_dev.  Asynchronous on `stream`; no allocation and no attribute call: it can be captured into a graph.
 * Host-buffer form: rows and out in host memory; synchronous. */
size_t pgt_f4_jackknife_work_bytes(uint32_t n_quartets, uint64_t n_win);
int pgt_f4_jackknife_dev(pgt_ctx *ctx, const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets,
                         pgt_f4_jack *out /* 3 * n_quartets, item-major u = 3q + c */, size_t out_bytes,
                         void *work, size_t work_bytes, void *stream);
int pgt_f4_jackknife(pgt_ctx *ctx, const pgt_f4_row *rows, uint64_t n_win, uint32_t n_quartets, pgt_f4_jack *out);

/* ---- f4-ratio: the sums behind the admixture proportions of ALL middle triples between A and an outgroup ----------------- */
/* The f4-ratio (Patterson et al. 2012; ADMIXTOOLS' qpF4ratio) answers "how much": alpha = f4(A,O; X,C) / f4(A,O; B,C) is the
 * share of B-related ancestry in X, where A is a relative of B that took no part in the admixture, C the other source and O an
 * outgroup.  Numerator and denominator must be counted over the SAME sites, all five populations present, and the standard error
 * of the ratio needs a jackknife that drops a block from both together: neither can be had from the .f4 tables of
 * pgt_f4_pops_reduce_dev, whose two quartets {A,O,X,C} and {A,O,B,C} are counted wherever their own four populations have data.
 * From each population's own (freq, nInd) columns, the input of pgt_f4_pops_reduce_dev, in one pass (12 B/site/population).  It
 * has NO counterpart in the reference: the definition below is the contract.
 * n_pops = K populations, 5 <= K <= 7.  Roles come from the order of the columns: population 0 is A, population K-1 the outgroup
 * O, populations 1 ... K-2 the m = K-2 MIDDLE populations.  An item is an unordered middle triple (i, j, k), 1 <= i < j < k <= K-2,
 * numbered in lexicographic order; there are T = C(m, 3) = 1 / 4 / 10 of them at K = 5 / 6 / 7.  For triple (i, j, k) and site s:
 *   counting   nind_x[s] >= minind for x = 0, K-1, i, j and k: FIVE populations (signed int32 compare; minind >= 1 required,
 *              PGT_EARG otherwise); a site that is not counted is selected away, never multiplied (its frequencies may be NaN or
 *              infinite, in A or O as well, its counts 0 or negative).  The counts enter through this predicate ONLY.
 *   per site   p_x = freq_x[s]; every operation rounded on its own, no contraction, in exactly this grouping:
 *                  e    = p_0 - p_{K-1}                           once per site
 *                  d_ab = p_a - p_b                               per middle pair a < b, shared by the triples that hold it
 *                  s0 = e * d_ij                                  f4(A,O; i,j)
 *                  s1 = e * d_ik                                  f4(A,O; i,k)
 *                  s2 = e * d_jk                                  f4(A,O; j,k)
 *              In real arithmetic s0 - s1 + s2 = 0; the three are stored all the same, so that the row has the layout of
 *              pgt_f4_row.  The values do not depend on which allele the columns report, provided all populations report the
 *              same one (with frequencies that are multiples of 2^-10, bit for bit).
 *   row        pgt_f4ratio_row (48 bytes): g_ij / g_ik / g_jk = the three SUMS of s0 / s1 / s2 over the window's counted sites,
 *              each from +0.0; n = their number; start / end / mid as pgt_f4_row's are filled; reserved_ = +0.0.
 *   ratios     NOT formed here.  With S0, S1, S2 the sums of a row (or of a total) and q(a, b) = b != 0 ? a / b : 0, the six
 *              admixture proportions alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C) of the triple are the caller's division:
 *                  c = 0  (B,X,C) = (i,j,k)  q(+S2, +S1)        c = 1  (j,i,k)  q(+S1, +S2)
 *                  c = 2  (i,k,j)            q(-S2, +S0)        c = 3  (k,i,j)  q(+S0, -S2)
 *                  c = 4  (j,k,i)            q(+S1, +S0)        c = 5  (k,j,i)  q(+S0, +S1)
 *              Nothing is clamped: an alpha outside [0, 1] is what the data say.
 *   out        T * n_win rows, triple-major: out[t * n_win + w]
 *   tot        DEVICE array of T pgt_f4ratio_total (40 bytes: the same three sums over all counted sites, neff, nskip), or NULL;
 *              n_win == 0 with tot: the global-only form
 *   tree       pgt_f4ratio_pops_tree_bytes(n_pops, n) bytes (0 for n_pops outside 5 ... 7): a node is 3 T doubles (s0 of triple
 *              0 .. T-1, then s1, then s2) and T u32.    5 <= n_pops <= 7, n < 2^32.
 * A one-site window carries exactly the bits of s0, s1 and s2 above.  Arguments, alignment, refusals (PGT_EARG; messages begin
 * "pgt_f4ratio_pops_reduce: " and name their argument; a refused call launches nothing and writes nothing), graph capture and
 * the hints: those of pgt_f4_pops_reduce_dev.  Triple isolation: the rows of a triple are a function, bit for bit, of the columns
 * of A, O and its own three populations and the window alone — not of the other middle populations, of K, or of the other rows
 * of the table.  With the columns (A, i, j, O) and A's count zeroed wherever population k falls below minind,
 * pgt_f4_pops_reduce_dev's f4_il_jk sum and n are g_ij and n, bit for bit on grid frequencies.  Sums are added in a fixed order
 * that depends on the site index and the window alone (bitwise reproducible); against an exact evaluation a sum stays within
 * 1e-9 * A + 1e-12, A the window's sum of |product|.  "Values the columns admit" above holds as for the other K-population calls
 * (tests/test_special_values_f4ratio.py).  Held to this definition, to an exact-rational fixture
 * (tests/golden/f4ratio_exact.json) and to a NumPy model (tests/f4ratio_pops_model.py).  User-chosen quintet lists, K = 8 and
 * qpAdm-style multi-source fits are not computed.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the T totals in host memory. */
size_t pgt_f4ratio_pops_tree_bytes(uint32_t n_pops, uint64_t n_sites);
int pgt_f4ratio_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                                const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                                const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out, size_t out_bytes,
                                pgt_f4ratio_total *tot, void *tree, size_t tree_bytes, void *stream);
int pgt_f4ratio_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                            const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                            const pgt_win *win, uint64_t n_win, pgt_f4ratio_row *out, pgt_f4ratio_total *tot);

/* ---- block-jackknife standard error and Z of the f4-ratio, all middle triples, six proportions each ---------------------- */
/* The weighted block jackknife of pgt_dstat_jackknife_dev — h_j, theta_J, tau_j, sigma^2, the rule "used iff n > 0, weight
 * m_j = n", the plan, the chunking and the order of every addition — with a third estimator, the SIGNED RATIO OF TWO BLOCK SUMS,
 * over the window rows pgt_f4ratio_pops_reduce_dev wrote.  Numerator and denominator lose a block together:
 *   rows     DEVICE pointer to the n_triples x n_win triple-major table, 16-byte aligned; every window is one block; the
 *            caller guarantees that the windows are DISJOINT.  Only n and the three sums of a row are read.
 *   items    triple t has SIX items u = 6 t + c, c the (B, X, C) of the table above with its (numerator, denominator) = (N_c,
 *            D_c) among +-S0, +-S1, +-S2; with q(a, b) = b != 0 ? a / b : 0 and n_cj, d_cj the same of block j's row
 *                theta(c) = q(N_c, D_c)           theta_-j(c) = q(N_c - n_cj, D_c - d_cj)
 *            (negation is exact: the sign is applied to the sums before the subtraction)
 *   blocks, per item: as pgt_dstat_jackknife_dev (a row that is not used is selected away, never added: its sums may be NaN)
 *   out      pgt_f4ratio_jack per item, item-major: alpha = theta, alpha_jack = theta_J, se = sqrt(sigma^2),
 *            z = se > 0 ? theta_J / se : NaN, n_blocks = g, n_sites = n, pad_ = 0.
 *            g < 2: alpha_jack = alpha, se = z = NaN.  g == 0 (n_win == 0 included): alpha = alpha_jack = 0, se = z = NaN.
 *   work     DEVICE workspace of pgt_f4ratio_jackknife_work_bytes(n_triples, n_win) bytes (0 for n_triples outside 1 ... 10),
 *            16-byte aligned: the three-item estimators' layout with six partials per wave in phases 2 and 3.  Every byte of it
 *            that is read is written earlier in the same call.
 * 1 <= n_triples <= 10.  Bitwise reproducible; an item's outputs are a function, bit for bit, of its own triple's rows alone:
 * not of n_triples, not of the other triples' rows.  Against an exact evaluation alpha, alpha_jack and se stay within 1e-9
 * relative + 1e-12 while no denominator, whole or with a block left out, is close to zero against its terms
 * (tests/f4ratio_jack_model.py).  Refusals (PGT_EARG, messages begin "pgt_f4ratio_jackknife: " and name their argument; nothing
 * is launched, nothing written): those of pgt_dstat_jackknife_dev.  Asynchronous on `stream`; no allocation and no attribute
 * call: it can be captured into a graph.
 * Host-buffer form: rows and out in host memory; synchronous. */
size_t pgt_f4ratio_jackknife_work_bytes(uint32_t n_triples, uint64_t n_win);
int pgt_f4ratio_jackknife_dev(pgt_ctx *ctx, const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples,
                              pgt_f4ratio_jack *out /* 6 * n_triples, item-major u = 6t + c */, size_t out_bytes,
                              void *work, size_t work_bytes, void *stream);
int pgt_f4ratio_jackknife(pgt_ctx *ctx, const pgt_f4ratio_row *rows, uint64_t n_win, uint32_t n_triples, pgt_f4ratio_jack *out);

/* ---- the population branch statistic (PBS) of ALL trios, every population of a trio as the focal one -------------------- */
/* PBS (Yi et al. 2010), the windowed selection scan for a focal population against two others, from each population's own
 * (freq, nInd) columns — the input of pgt_fst_pops_reduce_dev — over ONE position column and ONE window table.  It has NO
 * counterpart in the reference: the definition below is the contract.
 * n_pops = K populations, 3 <= K <= 6.  ALL populations are equal.  A trio is (i, j, k) with i < j < k < K; trios are numbered
 * as pgt_f3_pops_reduce_dev numbers them, T = C(K, 3) = 1 / 4 / 10 / 20.  For trio (i, j, k) and site s:
 *   counting   nind_i[s] >= minind && nind_j[s] >= minind && nind_k[s] >= minind   (signed int32 compare; minind >= 1 required,
 *              PGT_EARG otherwise); a site that is not counted is selected away, never multiplied: its columns may hold
 *              anything.  This is the TRIO's site set.  It is NOT the site set of the pair tables of pgt_fst_pops_reduce_dev,
 *              which count a pair's site whatever the third population holds: wherever the third population lacks data, three
 *              pair tables cover three different site sets and their FSTs are not branches of one tree.  Here the three pairs
 *              of a trio are summed over the same sites (as ANGSD's realSFS fst does with three populations).
 *   per site   for each of the trio's pairs (x, y) = (i, j), (i, k), (j, k) exactly the two values the all-pairs FST call adds
 *              for that pair at a counted site, with the site's own sample sizes:
 *                  pgt_pbs_pops_reduce_dev          num = a, den = a + b of pgt_fst_pops_reduce_dev (Weir-Cockerham)
 *                  pgt_pbs_hudson_pops_reduce_dev   num, den of pgt_fst_hudson_pops_reduce_dev, every operation rounded on its own
 *   row        pgt_pbs_row (88 bytes; offsets at the struct): start / end / mid as pgt_f3_row's are filled (PGT_WIN_COORDS
 *              honoured); n = the trio's counted sites (nskip = (hi - lo) - n); num_ij, num_ik, num_jk, den_ij, den_ik, den_jk =
 *              the six SUMS over those sites, each from +0.0; and from the row's own sums, every operation ONE rounding:
 *                  fst_xy = den_xy != 0 ? num_xy / den_xy : 0           (fstWindow.cpp:85)
 *                  T_xy   = -log(1 - fst_xy)                            (double log of the device library, at most 1 ulp)
 *                  pbs_i  = ((T_ij + T_ik) - T_jk) * 0.5 + 0.0
 *                  pbs_j  = ((T_ij + T_jk) - T_ik) * 0.5 + 0.0
 *                  pbs_k  = ((T_ik + T_jk) - T_ij) * 0.5 + 0.0
 *              NOTHING IS CLAMPED; the IEEE results stand: a negative FST gives a negative T (and may give a negative PBS);
 *              fst == 1 (a window of fixed differences only) gives T = +inf and PBS = +/-inf; inf - inf gives NaN (two pairs of
 *              the trio fixed); a NaN sum gives NaN.  A window without a counted site has all six sums and all three pbs +0.0.
 *              The FSTs are not stored: they are the caller's division, and a caller who wants another rule (FST truncated at
 *              0, PBSn1) applies it to the sums.
 *   out        T * n_win rows, trio-major: out[t * n_win + w]
 *   tot        DEVICE array of T pgt_pbs_total (88 bytes: the same nine doubles over all counted sites, neff, nskip), or NULL;
 *              n_win == 0 with tot: the global-only form (no row is written).  n_win == 0 with tot == NULL and n > 0: the
 *              tree-only call, as for the other K-population statistics — both passes build in `work`, the merging kernel is
 *              not launched, out and tot are not touched, PGT_OK
 *   work       DEVICE workspace of pgt_pbs_pops_work_bytes(n_pops, n, n_win) bytes (0 for n_pops outside 3 ... 6), 16-byte
 *              aligned: the tree of pgt_f3_pops_reduce_dev (3 T doubles and T u32 per node) and, behind it, 2 T n_win scratch rows
 *              and 2 T scratch totals of 40 bytes.  The columns are walked twice (the numerators, then the denominators: six
 *              sums per trio do not fit a node), the tree is reused, and a third kernel merges the passes.  Every byte that
 *              is read is written earlier in the same call.    3 <= n_pops <= 6, n < 2^32.
 * Arguments, alignment, refusals (PGT_EARG; the messages of BOTH estimators begin "pgt_pbs_pops_reduce: " and name their
 * argument: "n_pops must be 3 ... 6", "minind must be at least 1", "work is not 16-byte aligned", "work_bytes too small",
 * "out_bytes"; a refused call launches nothing and writes nothing), graph capture and the hints: those of
 * pgt_f3_pops_reduce_dev (asynchronous, ONE chain of kernels on `stream`, no allocation, no attribute call;
 * pgt_set_max_window honoured, pgt_set_window_step ignored; a profiled call reports the first pass and the second build as
 * the build, the rest as the query).  Trio isolation: the rows of a trio are a function, bit for bit, of its own three
 * populations' columns and the window alone.  Sums are added in a fixed order that depends on the site index and the window
 * alone (bitwise reproducible).  A one-site window carries, with the Hudson estimator, exactly the bits of num and den.
 * Against an exact evaluation a sum stays within 1e-9 * A + 1e-12, A the window's sum of the absolute values of the terms a
 * site's value is built from.  Held to this definition, to an exact-rational fixture (tests/golden/pbs_exact.json) and to a
 * NumPy model (tests/pbs_pops_model.py).  PBSn1 and the block jackknife of both: pgt_pbs_jackknife_dev below.  Not computed:
 * truncation of negative FST, user-chosen trio lists, K = 7.
 * Host-buffer form: columns (host arrays of n_pops HOST pointers), table, rows and the T totals in host memory. */
size_t pgt_pbs_pops_work_bytes(uint32_t n_pops, uint64_t n_sites, uint64_t n_win);
int pgt_pbs_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                            const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                            const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, size_t out_bytes,
                            pgt_pbs_total *tot, void *work, size_t work_bytes, void *stream);
int pgt_pbs_hudson_pops_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                                   const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                                   const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, size_t out_bytes,
                                   pgt_pbs_total *tot, void *work, size_t work_bytes, void *stream);
int pgt_pbs_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                        const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                        const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot);
int pgt_pbs_hudson_pops_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *const *freq,
                               const int32_t *const *nind, uint32_t n_pops, uint64_t n, int minind,
                               const pgt_win *win, uint64_t n_win, pgt_pbs_row *out, pgt_pbs_total *tot);

/* ---- block-jackknife standard error and Z of PBS and PBSn1, all trios, every focal population ------------------------------ */
/* The weighted block jackknife of pgt_dstat_jackknife_dev — g, n, h_j, theta_J, tau_j, sigma^2, the rule "used iff n > 0, weight
 * m_j = n", the plan, chunks of 64 rows with one row per lane, the order of every addition, no atomics — with a fourth
 * estimator, a NON-LINEAR function of SIX block sums, over the window rows pgt_pbs_pops_reduce_dev (or its Hudson form) wrote:
 *   rows     DEVICE pointer to the n_trios x n_win trio-major table, 8-byte aligned (an 88-byte row at an odd index is not
 *            16-byte aligned); every window is one block; the caller guarantees that the windows are DISJOINT.  Only n and the
 *            six sums of a row are read: the pbs_* fields and the coordinates are never looked at.
 *   E(S)     of six sums S = (num_ij, num_ik, num_jk, den_ij, den_ik, den_jk), every operation ONE rounding, nothing contracted:
 *                fst_xy  = den_xy != 0 ? num_xy / den_xy : 0
 *                T_xy    = -log(1 - fst_xy)                       (double log of the device library, as in the rows)
 *                pbs_i   = ((T_ij + T_ik) - T_jk) * 0.5 + 0.0     (pbs_j, pbs_k as in pgt_pbs_row)
 *                s       = (pbs_i + pbs_j) + pbs_k
 *                pbsn1_x = pbs_x / (1.0 + s)                      (PBSn1, Malaspinas et al. 2016; no clamp, no special case)
 *   items    trio t has SIX items u = 6 t + c: c = 0, 1, 2 PBS with i, j, k as the focal population, c = 3, 4, 5 PBSn1 of the same;
 *                theta(c) = E(S_total)[c]         theta_-j(c) = E(S_total - s_j)[c]
 *            each of the six sums losing block j with one rounding.  S_total is the jackknife's own sum of the used rows' sums
 *            in its own order: theta is the row arithmetic on THOSE sums and need not carry the bits of a pgt_pbs_total, whose
 *            sums come from the tree.  E is evaluated once per block (three logs) for all six items.
 *   blocks   as pgt_dstat_jackknife_dev (a row that is not used is selected away, never added: its sums may be NaN).  A NaN in
 *            any sum of a USED block makes all six items of its trio NaN (every item reads all six sums), and no other trio's.
 *   out      pgt_pbs_jack per item, item-major: stat = theta, stat_jack = theta_J, se = sqrt(sigma^2),
 *            z = se > 0 ? theta_J / se : NaN, n_blocks = g, n_sites = n, pad_ = 0.  8-byte aligned.
 *            g < 2: stat_jack = stat, se = z = NaN.  g == 0 (n_win == 0 included): stat = stat_jack = +0.0, se = z = NaN.
 *            NOTHING IS CLAMPED: inf and NaN from FST = 1, whole or with a block left out, are the IEEE results and stand.
 *   work     DEVICE workspace of pgt_pbs_jackknife_work_bytes(n_trios, n_win) bytes (0 for n_trios outside 1 ... 20), 16-byte
 *            aligned: per wave 8 words of phase 1 (six sums, Σn, g) and 6 doubles each of phases 2 and 3, rounded up to 256
 *            bytes.  Every byte of it that is read is written earlier in the same call.
 * 1 <= n_trios <= 20.  Bitwise reproducible; an item's outputs are a function, bit for bit, of its own trio's rows alone: not of
 * n_trios, not of the other trios' rows.  Against an exact evaluation stat, stat_jack and se stay within 1e-9 relative + 1e-12
 * while no 1 - fst and no 1 + s, whole or with a block left out, is close to zero (tests/pbs_jack_model.py).  Refusals (PGT_EARG,
 * messages begin "pgt_pbs_jackknife: " and name their argument, "n_trios must be 1 ... 20" among them; nothing is launched,
 * nothing written): those of pgt_dstat_jackknife_dev, with "rows is not 8-byte aligned".  Asynchronous on `stream`; no
 * allocation and no attribute call: it can be captured into a graph.
 * Host-buffer form: rows and out in host memory; synchronous. */
size_t pgt_pbs_jackknife_work_bytes(uint32_t n_trios, uint64_t n_win);
int pgt_pbs_jackknife_dev(pgt_ctx *ctx, const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios,
                          pgt_pbs_jack *out /* 6 * n_trios, item-major u = 6t + c */, size_t out_bytes,
                          void *work, size_t work_bytes, void *stream);
int pgt_pbs_jackknife(pgt_ctx *ctx, const pgt_pbs_row *rows, uint64_t n_win, uint32_t n_trios, pgt_pbs_jack *out);

/* ---- the sites common to K files, aligned on the device ------------------------------------------ */
/* Replaces the two-file synchronisation of dxyWindow.cpp:315-331 (one current line per file; the file that is behind reads
 * on until chromosome and position agree), generalised to 2 <= K <= 8 files as the intersection by (chromosome, position):
 * what those loops produce where they are defined (identical or nested site lists), and defined for any
 * lists.  The result is one u32 index column per file — idx[k][m] is the row of common site m in file k — with which
 * pgt_gather_dev brings every column of every file onto ONE shared position column: the input pgt_dxy_pops_reduce_dev
 * (and every other *_dev entry point over several files' columns) expects.  Exact integers: the result does not depend on
 * how the work is cut.
 *
 * pgt_align_segments (host, no device): per file the chromosome id of every run (the caller maps names to ids: equal names,
 * equal ids) and the run lengths -> one pgt_seg {first row, rows} per (matched chromosome, file), chromosome-major, in file
 * 0's order.  A chromosome is matched when every file has it.  PGT_EDOMAIN when a file lists an id in two runs or the matched
 * chromosomes do not come in the same relative order in every file ("Both input MAF files need to have the same chromosomes
 * in the same order", dxyWindow.cpp:49); the message names the id.  out may be NULL (count only); PGT_ECAP when cap < *n_out.
 *
 * pgt_sites_align: pos = HOST array of n_files DEVICE pointers (u32 positions, strictly increasing inside a segment; below
 * 2^32 - 1 rows per file); seg = the plan above (n_seg = n_files * matched chromosomes, at most 4096 of them); idx = HOST
 * array of n_files DEVICE pointers with room for cap u32 each; seg_count (n_seg / n_files common sites per matched
 * chromosome) and n_common are HOST outputs.  Synchronous: the caller needs n_common to size what follows.  PGT_ECAP with
 * *n_common (and seg_count) set when cap is too small; the first cap sites are then written and nothing beyond.
 * work: pgt_align_workspace_bytes(n_files, n_rows[0]) bytes of DEVICE memory, 16-byte aligned — at most
 * 4 * (n_files + 1) * n_rows_file0 + 1 MiB; 0 for n_files outside 2 ... 8.  File 0 is the pivot: pass the shortest list
 * first where there is a choice.
 *
 * pgt_gather_dev: dst[m] = src[idx[m]], m < n, elements of 4 or 8 bytes; asynchronous on `stream`; dst and src must not
 * overlap.  16-byte stores where dst and idx are 16-byte aligned. */
typedef struct { uint64_t off, len; } pgt_seg;
int pgt_align_segments(const uint32_t *const *run_chr, const uint64_t *const *run_len, const size_t *n_runs, uint32_t n_files,
                       pgt_seg *out, size_t cap, size_t *n_out);
size_t pgt_align_workspace_bytes(uint32_t n_files, uint64_t n_rows_file0);
int pgt_sites_align(pgt_ctx *ctx, const uint32_t *const *pos, const uint64_t *n_rows, uint32_t n_files, const pgt_seg *seg,
                    size_t n_seg, uint32_t *const *idx, uint64_t cap, uint64_t *seg_count, uint64_t *n_common, void *work,
                    size_t work_bytes, void *stream);
int pgt_gather_dev(pgt_ctx *ctx, void *dst, const void *src, const uint32_t *idx, uint64_t n, uint32_t elem_bytes /* 4 or 8 */,
                   void *stream);

/* ---- ihsWindow / xpehhWindow: extreme score in non-overlapping bp windows ---- */
/* Replaces the window bookkeeping and per-window scan of ihsWindow.cpp:123-221 and
 * xpehhWindow.cpp:126-232: the most extreme score of the window (first occurrence on ties), its
 * position, and the number of scores beyond the cutoff. */
enum {
    PGT_EXT_IHS = 0,    /* extreme = largest |s|, count |s| > cutoff           (ihsWindow.cpp:193-205)   */
    PGT_EXT_XP_MAX = 1, /* extreme = largest s,   count s > cutoff (cutoff>=0) (xpehhWindow.cpp:213-216) */
    PGT_EXT_XP_MIN = 2  /* extreme = smallest s,  count s < cutoff (cutoff<0)  (xpehhWindow.cpp:210-212) */
};
typedef struct { /* ihsWindow.cpp:101-110 row: chr start end score position proportion nsites */
    uint32_t start, end, nsites, nbig;
    uint32_t position, pad_; /* position of the extreme score; 0 when nsites == 0 (the tool prints NA) */
    double value;            /* the extreme score (signed): a copy of the input, bit for bit; 0.0 when nsites == 0 */
} pgt_ext_row;
/* NaN scores, as the reference's loop treats them (ihsWindow.cpp:194-205): the window's FIRST site is the running extreme
 * unconditionally and a later site replaces it only when its key is strictly greater.  So a window whose first score is NaN
 * reports that site (value = that NaN, with its position) whatever follows; a NaN at a later site never wins; a NaN is never
 * beyond the cutoff (nbig).  +-inf are ordinary keys (ties: the first occurrence).  The rule depends on the window alone:
 * rows do not depend on the query strategy or on the sharding. */
/* The tools' window rules applied site by site on the host (they are history dependent: a site at
 * pos >= window end opens the next window, ihsWindow.cpp:176-190): fixed bp windows [1,W],[W+1,2W],..
 * per chromosome, clamped to chr_len[r] where given (0 = not given; chr_len may be NULL), empty
 * windows included, trailing windows up to the chromosome length.  O(n).  Rows carry
 * PGT_WIN_COORDS.  PGT_EDOMAIN for n == 0 or a position beyond a given chromosome length (the
 * reference prints a nameless window / loops forever there). */
int pgt_build_windows_extreme(const uint32_t *pos, const uint64_t *run_len, const uint32_t *chr_len,
                              size_t n_runs, uint32_t W, pgt_win *out, size_t cap, size_t *n_out);
int pgt_extreme_reduce(pgt_ctx *ctx, const uint32_t *pos, const double *score, uint64_t n, int mode,
                       double cutoff, const pgt_win *win, uint64_t n_win, pgt_ext_row *out);
/* device-resident form; tree: pgt_tree_bytes(PGT_STAT_EXT, n) bytes */
int pgt_extreme_reduce_dev(pgt_ctx *ctx, const uint32_t *pos, const double *score, uint64_t n, int mode,
                           double cutoff, const pgt_win *win, uint64_t n_win, pgt_ext_row *out,
                           size_t out_bytes, void *tree, size_t tree_bytes, void *stream);

/* ---- performance hint ------------------------------------------------------------------- */
/* Longest window (in sites) the following *_dev calls will be asked for; 0 (the default) = unknown.
 * Tree levels whose nodes are larger than this are not built (a query never touches them).  The
 * hint only affects speed: a longer window is still answered correctly from the levels that
 * exist.  The host-buffer / *_cols entry points derive a hint from the table only while it is unknown (0): a caller
 * that reduces SLICES of one table on several GPUs sets both hints from the whole table (W, S), so that every
 * slice — and the single-GPU run — takes the same query strategy: rows are bitwise independent of the number of
 * GPUs only under identical hints (the strategies add in different orders).
 * The value also stands for the TYPICAL window length when the query strategy is chosen (pgt_set_window_step): pass the
 * tools' W, not a loose upper bound — the group strategy is taken for windows of at least two level-2 tiles, and with
 * windows much shorter than the hint it degenerates to one range query after the other (correct, slow). */
int pgt_set_max_window(pgt_ctx *ctx, uint64_t max_window_sites);
/* Typical distance, in sites, between the starts of consecutive windows of the following *_dev calls
 * (the tools' step size S); 0 (the default) = unknown: one wave per window.  The step selects the query
 * strategy for the regime `-winsize W -stepsize S` with S << W, where the reference re-sums W sites and
 * shifts W-S per window (fstWindow.cpp:80-83,95-99):
 *   GROUP    1 <= S <= 1024 and a longest-window hint of at least two level-2 tiles (16384 sites for the f64
 *            trees, 131072 for the genotype tree): one wave answers up to 64 CONSECUTIVE windows, one per lane;
 *            they share the scans of the 128-site tiles under their ends (S <= 64), the scans of the level-1
 *            nodes beside those and ONE tree query per distinct interior;
 *   SLIDING  S <= 32 with shorter (or unknown) windows: per-site suffix / prefix scans of the 128-site tiles a
 *            group of 128/S + 1 windows starts and ends in, and one tree query for the interior they share.
 * Speed only: any table is answered correctly whatever the hint (windows a strategy does not fit fall back to
 * the plain range query); the strategies add in different orders, so the last bits of a float may differ between
 * them — under one pair of hints, rows are bitwise independent of which windows share a wave and of the number of
 * GPUs.  The host-buffer entry points derive the hint from the table while it is unset. */
int pgt_set_window_step(pgt_ctx *ctx, uint64_t step_sites);
/* Tables whose windows vary in length (dxyWindow's base-pair windows): the typical (median) window length, which then
 * decides between the strategies instead of the longest.  Call it AFTER pgt_set_max_window (which resets it to "the same").
 * pgt_table_hints gives the three values exactly as the host-buffer entry points derive them from a table while the hints
 * are unset: a caller that reduces SLICES of one table on several GPUs sets them on every context, so that every slice
 * is reduced as the whole table would be (rows bitwise independent of the slicing).  The step comes back as UINT64_MAX
 * where the table has no typical positive step (0 would mean "unknown" and let every slice estimate its own). */
int pgt_set_typical_window(pgt_ctx *ctx, uint64_t typical_sites);
int pgt_table_hints(const pgt_win *win, uint64_t n_win, uint64_t *max_window, uint64_t *typical_window, uint64_t *window_step);

/* ---- per-kernel timing (HIP events on the launch stream; for bench.py's roofline) ------- */
/* When enabled, the *_dev entry points bracket the tree-build kernel and the window-query
 * kernel with HIP events; pgt_last_kernel_ms synchronises on them and returns both. */
int pgt_set_profiling(pgt_ctx *ctx, int enabled);
int pgt_last_kernel_ms(pgt_ctx *ctx, float *build_ms, float *query_ms);

/* ---- multi-GPU sharding plan (host) ----------------------------------------------------- */
/* Split a window table into n_ranks contiguous blocks balanced by reduced sites.  Rank r owns
 * windows [win_begin, win_end) and needs the site columns [site_lo, site_hi); site_lo is
 * rounded down to a multiple of max(65536, the largest power of two <= the longest window), so
 * that every tree node a query can touch (nodes are powers of two of sites for every statistic)
 * has the same boundaries as in the single-GPU tree: results are bitwise independent of n_ranks. */
typedef struct {
    uint64_t win_begin, win_end;
    uint64_t site_lo, site_hi;
} pgt_shard;
int pgt_plan_shards(const pgt_win *win, uint64_t n_win, uint32_t n_ranks, pgt_shard *out);

/* ---- multi-GPU row exchange without a per-step collective ----------------- */
/* The reference prints each window's row as soon as calcWindow has reduced it (fstWindow.cpp:88); in
 * the sharded form rank 0 prints, so every rank's rows must reach rank 0.  Instead of a gather per
 * scan, rank 0 creates ONE row buffer for the whole window table and exports it; every other rank
 * (one process per GPU) opens it and passes `base + its first window * row size` as the `out`
 * pointer of its *_dev call: the query kernel's row stores then travel over xGMI straight into rank
 * 0's HBM.  After every rank has synchronised its stream (plus one barrier of the caller's process
 * group) rank 0 holds the assembled table.  Rows of different ranks should start on 256-byte
 * boundaries of the buffer (pad between blocks) so that no cache line is written by two GPUs.
 *   create  hipMalloc on ctx's device + hipIpcGetMemHandle; the handle is 64 plain bytes that the
 *           caller ships to the other processes (e.g. torch.distributed.broadcast_object_list)
 *   open    hipIpcOpenMemHandle on ctx's device (peer mapping); fails in the creating process
 *   close   owner != 0: hipFree;  owner == 0: hipIpcCloseMemHandle
 *   read    rank 0: device -> host copy of the assembled rows, ordered after `stream` */
#define PGT_IPC_HANDLE_BYTES 64
typedef struct { unsigned char opaque[PGT_IPC_HANDLE_BYTES]; } pgt_ipc_handle;
/* PGT_OK when ctx's device can address memory of HIP device `peer_device` (peer access is enabled as a side
 * effect); every rank checks this against the creating rank's device before it opens the buffer and falls
 * back to a gather otherwise.  peer_device == ctx's own device is always OK. */
int pgt_peer_access(pgt_ctx *ctx, int peer_device);
int pgt_rowbuf_create(pgt_ctx *ctx, size_t bytes, void **dev_ptr, pgt_ipc_handle *handle);
int pgt_rowbuf_open(pgt_ctx *ctx, const pgt_ipc_handle *handle, void **dev_ptr);
int pgt_rowbuf_close(pgt_ctx *ctx, void *dev_ptr, int owner);
int pgt_rowbuf_read(pgt_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes, void *stream);
/* Self-test of a mapping before it is trusted: a kernel on ctx's device stores the 8-byte words
 * splitmix64(seed + i), i = 0 .. bytes/8 - 1, to dev_ptr with the same plain global stores the query kernels
 * use for their rows (asynchronous on `stream`; bytes a multiple of 8, dev_ptr 8-byte aligned).  Every rank
 * fills its slice of the shared buffer, the owner reads it back (pgt_rowbuf_read) and compares. */
int pgt_rowbuf_fill(pgt_ctx *ctx, void *dev_ptr, size_t bytes, uint64_t seed, void *stream);

/* ---- plain device buffers (for callers without a HIP binding of their own: the C++ hosts' multi-GPU path) --------
 * One process may hold one pgt_ctx per GPU (one thread each).  pgt_dev_copy moves bytes between buffers of two
 * contexts — the same device, or two devices (peer copy where the link allows it, staged by the runtime otherwise);
 * it is synchronous and may be called from the thread of either context. */
int pgt_dev_alloc(pgt_ctx *ctx, size_t bytes, void **dev_ptr);
/* free and total memory of ctx's device in bytes (the hosts decide with it whether a table must be reduced in passes) */
int pgt_dev_memory(pgt_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
int pgt_dev_free(pgt_ctx *ctx, void *dev_ptr);
/* host memory -> a buffer of ctx's device (synchronous) */
int pgt_dev_upload(pgt_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int pgt_dev_copy(pgt_ctx *dst_ctx, void *dst, pgt_ctx *src_ctx, const void *src, size_t bytes);

/* ---- device-side text ingest ------------------------------------------------ */
/* Replaces the per-line text parse of the reference's streaming loops (fstWindow.cpp:123-146 `chr pos a b`,
 * hetWindow.cpp:121-144 `chr pos genotype`, dxyWindow.cpp:141-153,399-403 `chr pos major minor ref freq nInd`):
 * the raw text is copied to the GPU once and parsed there into the structure-of-arrays columns the
 * *_reduce_dev entry points take, together with the chromosome runs pgt_build_windows_* take.
 *   text, len   the lines to parse, in HOST memory (a header line, if any, already skipped by the caller)
 *   tokens      what the whitespace-separated tokens of a line are, in order; tokens[0] must be PGT_TOK_CHR or PGT_TOK_CHR_PREFIX
 *               (2 <= n_tokens <= 12); tokens beyond n_tokens are ignored, as the tools ignore extra columns
 * Semantics of the tools' own loops are kept: a blank line ends the data (fstWindow.cpp:125); a last line
 * without newline is accepted; \r counts as blank.  Numbers the kernel cannot convert exactly in one f64
 * operation (more than 15 significant digits, |power of ten| > 22, inf, nan, odd signs) are converted on the
 * host with the correctly rounded library routine, so every value has the bits `ss >> double` gives.
 * pgt_ingest_bad_line: 0-based index of the first line (before the end of data) that cannot be parsed, or -1;
 * rows then holds the number of good lines before it, and the caller reports the error as the tools would.
 * PGT_EDOMAIN: a line longer than 64 KiB, or more than 2^20 chromosome runs or irregular lines — such an
 * input is not one of the tools' tables; parse it on the host.
 * Column k (pgt_ingest_column) belongs to token k: u32 for PGT_TOK_U32, f64 for _F64 / _FREQ, i8 for _I8,
 * i32 for _I32, NULL for _CHR / _SKIP; DEVICE pointers, rows elements, owned by the ingest object.
 * pgt_ingest_runs: run lengths, and for every run the byte offset and length of its name inside `text`. */
enum {
    PGT_TOK_CHR = 0,  /* chromosome name: delimits the runs, not stored */
    PGT_TOK_SKIP = 1, /* ignored (MAF major / minor / ref) */
    PGT_TOK_U32 = 2,  /* position */
    PGT_TOK_F64 = 3,  /* any double */
    PGT_TOK_I8 = 4,   /* integer, clamped to int8 (hetWindow genotype: only >= 0 and == 1 are ever tested) */
    PGT_TOK_I32 = 5,  /* integer, clamped to int32 (MAF nInd) */
    PGT_TOK_FREQ = 6, /* double that must lie in [0,1] (MAF allele frequency), else the line is an error */
    PGT_TOK_CHR_PREFIX = 7 /* as PGT_TOK_CHR (allowed as tokens[0] only), the chromosome being the token UP TO ITS FIRST '_':
                            * selscan locus ids `chr_position` (extractChr, ihsWindow.cpp:80-92; xpehhWindow.cpp:82-94); a token
                            * without '_' is the name as a whole (ABI 5) */
};
typedef struct pgt_ingest pgt_ingest;
/* reductions over DEVICE columns (pgt_ingest_column) with the window table and the rows in HOST memory:
 * the host-buffer entry points minus the column upload; synchronous */
int pgt_fst_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_a, const double *d_b, uint64_t n,
                        const pgt_win *win, uint64_t n_win, pgt_fst_row *out, size_t out_bytes);
int pgt_het_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const int8_t *d_g, uint64_t n,
                        const pgt_win *win, uint64_t n_win, pgt_het_row *out, size_t out_bytes);
int pgt_dxy_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_p1, const double *d_p2,
                        const int32_t *d_n1, const int32_t *d_n2, uint64_t n, int minind,
                        const pgt_win *win, uint64_t n_win, pgt_dxy_row *out, size_t out_bytes, pgt_dxy_total *tot);
/* ihsWindow.cpp:123-221 / xpehhWindow.cpp:126-232 over device columns (the device-parsed *.norm table) */
int pgt_extreme_reduce_cols(pgt_ctx *ctx, const uint32_t *d_pos, const double *d_score, uint64_t n, int mode, double cutoff,
                            const pgt_win *win, uint64_t n_win, pgt_ext_row *out, size_t out_bytes);
/* device column of token `token` -> host (bytes <= rows * element size, else PGT_EARG) */
int pgt_ingest_download(pgt_ctx *ctx, const pgt_ingest *ing, int token, void *host_dst, size_t bytes);
int pgt_ingest_text(pgt_ctx *ctx, const char *text, size_t len, const uint8_t *tokens, int n_tokens, pgt_ingest **out);
/* The same, with room for `rows_in_front` more rows BEFORE the parsed ones in every column: a caller that parses the head
 * of a text itself (the shipped hosts do, beside HIP start-up) uploads its rows there (pgt_dev_upload to
 * pgt_ingest_column_base) and has one contiguous column without a copy.  pgt_ingest_column still points at the first
 * parsed row, pgt_ingest_rows counts the parsed rows only. */
int pgt_ingest_text_behind(pgt_ctx *ctx, const char *text, size_t len, const uint8_t *tokens, int n_tokens,
                           uint64_t rows_in_front, pgt_ingest **out);
void *pgt_ingest_column_base(const pgt_ingest *ing, int token);
uint64_t pgt_ingest_rows(const pgt_ingest *ing);
/* 1 when the data ended at a blank line of `text`, be it its last line (the tools stop reading there, fstWindow.cpp:125):
 * a caller that hands consecutive pieces of one file to several GPUs must drop the pieces behind such a one. */
int pgt_ingest_blank_before_end(const pgt_ingest *ing);
int64_t pgt_ingest_bad_line(const pgt_ingest *ing);
void *pgt_ingest_column(const pgt_ingest *ing, int token);
size_t pgt_ingest_runs(const pgt_ingest *ing, const uint64_t **run_len, const uint64_t **name_off, const uint32_t **name_len);
void pgt_ingest_free(pgt_ingest *ing);

/* ---- window tables built ON the device (the `-stepsize 1` regime) -------------------
 * With one window per site the table of pgt_build_windows_sites is as large as the columns (32 B per window)
 * and the host spends its time filling and uploading it.  pgt_wintab_sites builds the SAME table — same rules
 * (fstWindow.cpp:132-138,150-152 with calcWindow's carry :92-103), same bytes — in GPU memory from the
 * chromosome run lengths: the host plans every run in O(#runs), a kernel writes the windows.
 * pgt_wintab_first: n_runs + 1 values, the index of every run's first window (the last = the number of windows):
 * row i carries the name of the run r with first[r] <= i < first[r+1] (pgt_win.label_run of the host table).
 * pgt_wintab_device: the table itself, a DEVICE pointer usable as `win` of the *_dev calls.
 * *_reduce_tab: the host-buffer entry points (cols_on_device = 0: pos / a / b ... are host arrays, uploaded here)
 * or the *_reduce_cols ones (cols_on_device = 1) over such a table; rows come back to HOST memory (out_bytes =
 * capacity of `out`, at least pgt_wintab_size rows); synchronous. */
typedef struct pgt_wintab pgt_wintab;
int pgt_wintab_sites(pgt_ctx *ctx, const uint64_t *run_len, size_t n_runs, uint32_t W, uint32_t S, pgt_wintab **out);
uint64_t pgt_wintab_size(const pgt_wintab *tab);
const uint64_t *pgt_wintab_first(const pgt_wintab *tab);
const pgt_win *pgt_wintab_device(const pgt_wintab *tab);
void pgt_wintab_free(pgt_wintab *tab);
int pgt_fst_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const double *a, const double *b, uint64_t n, int cols_on_device,
                       const pgt_wintab *tab, pgt_fst_row *out, size_t out_bytes);
int pgt_het_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const int8_t *g, uint64_t n, int cols_on_device,
                       const pgt_wintab *tab, pgt_het_row *out, size_t out_bytes);
int pgt_dxy_reduce_tab(pgt_ctx *ctx, const uint32_t *pos, const double *p1, const double *p2, const int32_t *n1,
                       const int32_t *n2, uint64_t n, int minind, int cols_on_device, const pgt_wintab *tab,
                       pgt_dxy_row *out, size_t out_bytes, pgt_dxy_total *tot);

#ifdef __cplusplus
}
#endif
#endif /* PGTWIN_H */
