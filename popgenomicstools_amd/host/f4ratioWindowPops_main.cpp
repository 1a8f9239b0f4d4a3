// f4ratioWindowPops (MI355X host) — sliding-window f4-ratio admixture proportions (Patterson et al. 2012; ADMIXTOOLS'
// qpF4ratio) from the ANGSD .mafs files (plain, gzip or bgzf) of 5 ... 7 populations: the FIRST file is A, the LAST the outgroup
// O, and every triple of the files between them is analysed in all six readings (B, X, C) of
//     alpha = f4(A,O; X,C) / f4(A,O; B,C)        the share of B-related ancestry in X
// After "is there admixture" (dstatWindowPops, f3WindowPops, f4WindowPops) this answers "how much".
// The reference has no such tool; the definition is that of pgt_f4ratio_pops_reduce_dev (include/pgtwin.h).
//
//   f4ratioWindowPops [dxyWindow's options] [-jackknife 0|1] -out PREFIX <maf A> <maf M1> ... <maf Mm> <maf O>      5 <= K <= 7
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): the sites (chromosome, position) that ALL
// files list are found on the GPU and every file's columns are gathered onto them.  One pgt_f4ratio_pops_reduce_dev call then
// reduces all C(K-2, 3) triples: per site (p_A - p_O)(p_x - p_y) for the three pairs of the triple, counted where A, O and the
// triple's three populations — all five — have at least -minind individuals, so that numerator and denominator of every ratio
// cover the same sites; per window their sums, and the six ratios formed here (0 where the denominator is 0, never clamped).
// Triple (i, j, k) -> PREFIX.pop<i>_pop<j>_pop<k>.f4ratio, i, j, k the files' numbers on the command line (`chr start end mid
// alpha_c0 .. alpha_c5 neff nskip`); the genome-wide lines -> PREFIX.global (`i j k alpha_c0 .. alpha_c5 neff nskip`).
// stdout stays empty.
// -jackknife 1 (disjoint windows only: -stepsize not below -winsize): one pgt_f4ratio_jackknife_dev call on the device rows
// gives the delete-m_j block jackknife of every ratio, numerator and denominator losing a block together, the run's windows
// being the blocks -> PREFIX.jackknife (`B X C alpha alpha_jack SE Z nblocks nsites`, six lines per triple).  Every other file
// is the same with and without it.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\nf4ratioWindowPops [options] -out PREFIX <maf A> <maf M1> ... <maf Mm> <maf O>      (5 <= K <= 7 files, m = K-2 between A and O)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each of the five populations with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8s(1) Write PREFIX.jackknife: block-jackknife standard error and Z score of every admixture proportion [0]\n"
                "\nNotes:\n"
                "* The FIRST file is A, a relative of one source that took no part in the admixture; the LAST file is the outgroup O;\n"
                "  the files between them are the middle populations (3 to 5 of them)\n"
                "* Every triple i < j < k of middle populations is analyzed in all six readings (B, X, C): C(K-2,3) triples\n"
                "* Definition: alpha(B, X, C) = f4(A,O; X,C) / f4(A,O; B,C), the share of B-related ancestry in X when X is a mixture of\n"
                "  relatives of B and C, with f4(A,O; x,y) the mean over the analyzed sites of (p_A - p_O)(p_x - p_y)\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* A site counts for a triple when ALL FIVE populations (A, O and the three of the triple) each have at least -minind\n"
                "  individuals with data: numerator and denominator of a ratio are always taken over the same sites\n"
                "* The ratios are symmetric in the two alleles: it does not matter which allele the MAF files report,\n"
                "  but ALL files must report the frequency of the SAME allele at every site\n"
                "* alpha is NOT clamped to [0, 1]: a value outside says that (B, X, C) does not fit the data (or is noise); it is printed as it is\n"
                "* A ratio whose denominator is exactly zero is printed as 0 (as is every ratio of a window without an analyzed site)\n"
                "* -jackknife 1: weighted (delete-m) block jackknife of the ratio (Busing et al. 1999; as ADMIXTOOLS): a block is left out of\n"
                "  numerator and denominator together. The blocks are the run's windows, weighted by their number of analyzed sites;\n"
                "  windows without an analyzed site are left out.\n"
                "  The windows must not overlap: -winsize > 0 and -stepsize not below -winsize. -fixedsite 1 windows hold the same number\n"
                "  of sites and so give blocks of (nearly) equal weight; -skip_missing does not change the blocks\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic\n"
                "\nLimits:\n"
                "* Not computed: user-chosen quintet lists, K = 8, qpAdm-style multi-source fits\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>_pop<k>.f4ratio for every triple i < j < k of middle files, numbered as on the command line (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n"
                "(5) alpha(B,X,C) for (i,j,k)\n(6) for (j,i,k)\n(7) for (i,k,j)\n(8) for (k,i,j)\n(9) for (j,k,i)\n(10) for (k,j,i)\n"
                "(11) number sites in MAF input that were analyzed\n"
                "(12) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per triple:\n(1) i\n(2) j\n(3) k\n(4)-(9) the six alpha in the order above\n(10) number of sites analyzed\n(11) number of sites skipped\n"
                "PREFIX.jackknife (with -jackknife 1), six lines per triple i < j < k, in the order above:\n"
                "(1) B\n(2) X\n(3) C\n(4) alpha(B,X,C) over all blocks\n(5) jackknife estimate of alpha\n(6) standard error\n"
                "(7) Z = (5) / (6) (nan with fewer than two blocks or a standard error of zero)\n(8) number of blocks\n(9) number of sites in the blocks\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-jackknife", "INT");
}

static double q(double num, double den) { return den != 0.0 ? num / den : 0.0; }

struct F4RatioPops : PopsTool {
    static constexpr const char *name = "f4ratioWindowPops";
    static constexpr int min_files = 5, max_files = 7;
    static constexpr auto help = ::help;
    static constexpr int arity = 3;  // all triples of the files between the first (A) and the last (O)
    static constexpr bool outgroup = true;
    static constexpr bool first_apart = true;
    using Row = pgt_f4ratio_row;
    using Total = pgt_f4ratio_total;
    static constexpr const char *ext = ".f4ratio";
    static constexpr size_t row_bytes = 260;
    static constexpr auto tree_bytes = pgt_f4ratio_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_f4ratio_pops_reduce_dev;
    JackknifeOption jackknife;
    bool own(const char *o, const char *v, int argc, char **argv) { return jackknife.take(o, v, argc, argv); }
    // chr start end mid alpha_c0 .. alpha_c5 neff nskip; the genome-wide ratios from the totals by the row's rule
    static PopsLine line(const Row &r, uint32_t sites) {
        return {{r.start, r.end, r.mid}, {q(r.g_jk, r.g_ik), q(r.g_ik, r.g_jk), q(-r.g_jk, r.g_ij), q(r.g_ij, -r.g_jk), q(r.g_ik, r.g_ij), q(r.g_ij, r.g_ik)}, r.n, sites - r.n};
    }
    static PopsLine total(const Total &g) {
        return {{}, {q(g.g_jk, g.g_ik), q(g.g_ik, g.g_jk), q(-g.g_jk, g.g_ij), q(g.g_ij, -g.g_jk), q(g.g_ik, g.g_ij), q(g.g_ij, g.g_ik)}, g.neff, g.nskip};
    }
    // B X C alpha alpha_jack SE Z nblocks nsites: triple order, then (i,j,k), (j,i,k), (i,k,j), (k,i,j), (j,k,i), (k,j,i)
    static constexpr int readings[6][3] = {{0, 1, 2}, {1, 0, 2}, {0, 2, 1}, {2, 0, 1}, {1, 2, 0}, {2, 1, 0}};
    void more(PopsRun &run, const Row *d_rows) {
        if (jackknife.on) pops_jackknife(run, d_rows, pgt_f4ratio_jackknife_dev, pgt_f4ratio_jackknife_work_bytes, readings);
    }
};

int main(int argc, char **argv) { return run_pops_tool<F4RatioPops>(argc, argv); }
