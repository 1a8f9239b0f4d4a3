// f4WindowPops (MI355X host) — sliding-window f4 (Reich et al. 2009; Patterson et al. 2012; treemix's fourpop, ADMIXTOOLS'
// qpDstat in f4mode) for ALL quartets of 4 ... 6 populations, every quartet in its three pairings, from their ANGSD .mafs files
// (plain, gzip or bgzf): the treeness test that goes with the .dstat and .f3 files of dstatWindowPops / f3WindowPops; it needs
// no outgroup and has no finite-sample bias term.
// The reference has no such tool; the definition is that of pgt_f4_pops_reduce_dev (include/pgtwin.h).
//
//   f4WindowPops [dxyWindow's options] [-jackknife 0|1] -out PREFIX <maf 1> ... <maf K>        4 <= K <= 6
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): the sites (chromosome, position) that ALL
// files list are found on the GPU and every file's columns are gathered onto them.  One pgt_f4_pops_reduce_dev call then
// reduces all C(K, 4) quartets: per site (p_a - p_b)(p_c - p_d) for each pairing (a,b; c,d) of the quartet, counted where all
// four populations have at least -minind individuals; per window their sums, and the mean f4 = sum / neff formed here.
// Quartet (i, j, k, l) -> PREFIX.pop<i+1>_pop<j+1>_pop<k+1>_pop<l+1>.f4 (`chr start end mid f4_ij_kl f4_ik_jl f4_il_jk neff
// nskip`); the genome-wide lines -> PREFIX.global (`i+1 j+1 k+1 l+1 f4_ij_kl f4_ik_jl f4_il_jk neff nskip`).  stdout stays empty.
// -jackknife 1 (disjoint windows only: -stepsize not below -winsize): one pgt_f4_jackknife_dev call on the device rows gives
// the delete-m_j block jackknife of every quartet and pairing, the run's windows being the blocks -> PREFIX.jackknife
// (`a b c d f4 f4_jack SE Z nblocks nsites` for f4(a,b; c,d)).  Every other file is the same with and without it.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\nf4WindowPops [options] -out PREFIX <pop1 maf file> ... <popK maf file>      (4 <= K <= 6)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each of the four populations with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8s(1) Write PREFIX.jackknife: block-jackknife standard error and Z score of f4 for every quartet and pairing [0]\n"
                "\nNotes:\n"
                "* ALL populations are equal: there is no outgroup file (K between 4 and 6 files)\n"
                "* Every quartet i < j < k < l of populations is analyzed in its three pairings (i,j; k,l), (i,k; j,l), (i,l; j,k): C(K,4) quartets\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* Per site, with p the frequencies: f4(a,b; c,d) = (p_a - p_b)(p_c - p_d); a window's value is the MEAN over its analyzed\n"
                "  sites (0 for a window without one). There is no bias term: the numbers of individuals decide only whether a site counts\n"
                "* The three values of a quartet satisfy f4(i,j; k,l) - f4(i,k; j,l) + f4(i,l; j,k) = 0 up to rounding\n"
                "* The statistic is symmetric in the two alleles: it does not matter which allele the MAF files report,\n"
                "  but ALL files must report the frequency of the SAME allele at every site\n"
                "* A site counts for a quartet when its four populations each have at least -minind individuals with data\n"
                "* Treeness test: f4(a,b; c,d) is zero in expectation when ((a,b),(c,d)) is the tree; |Z| above about 3 rejects\n"
                "  the tree ((a,b),(c,d))\n"
                "* With an outgroup O as the LAST file, f4(i,j; k,O) is the numerator of Patterson's D of dstatWindowPops for the trio (i,j,k)\n"
                "* -jackknife 1: weighted (delete-m) block jackknife of f4 (Busing et al. 1999; as ADMIXTOOLS). The blocks are the\n"
                "  run's windows, weighted by their number of analyzed sites; windows without an analyzed site are left out.\n"
                "  The windows must not overlap: -winsize > 0 and -stepsize not below -winsize. -fixedsite 1 windows hold the same number\n"
                "  of sites and so give blocks of (nearly) equal weight; -skip_missing does not change the blocks\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic\n"
                "\nLimits:\n"
                "* Not computed: f4-ratio admixture proportions (see f4ratioWindowPops), user-chosen quartet lists, K = 7\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>_pop<k>_pop<l>.f4 for every quartet i < j < k < l (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) f4(i,j; k,l)\n(6) f4(i,k; j,l)\n(7) f4(i,l; j,k)\n"
                "(8) number sites in MAF input that were analyzed\n"
                "(9) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per quartet:\n(1) i\n(2) j\n(3) k\n(4) l\n(5) f4(i,j; k,l)\n(6) f4(i,k; j,l)\n(7) f4(i,l; j,k)\n(8) number of sites analyzed\n(9) number of sites skipped\n"
                "PREFIX.jackknife (with -jackknife 1), three lines per quartet i < j < k < l: (i,j; k,l), (i,k; j,l), (i,l; j,k):\n"
                "(1) a\n(2) b\n(3) c\n(4) d\n(5) f4(a,b; c,d) over all blocks\n(6) jackknife estimate of f4\n(7) standard error\n"
                "(8) Z = (6) / (7) (nan with fewer than two blocks or a standard error of zero)\n(9) number of blocks\n(10) number of sites in the blocks\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-jackknife", "INT");
}

static double mean_of(double sum, uint64_t neff) { return neff ? sum / (double)neff : 0.0; }

struct F4Pops : PopsTool {
    static constexpr const char *name = "f4WindowPops";
    static constexpr int min_files = 4, max_files = 6;
    static constexpr auto help = ::help;
    static constexpr int arity = 4;  // all quartets
    using Row = pgt_f4_row;
    using Total = pgt_f4_total;
    static constexpr const char *ext = ".f4";
    static constexpr size_t row_bytes = 200;
    static constexpr auto tree_bytes = pgt_f4_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_f4_pops_reduce_dev;
    JackknifeOption jackknife;
    bool own(const char *o, const char *v, int argc, char **argv) { return jackknife.take(o, v, argc, argv); }
    // chr start end mid f4_ij_kl f4_ik_jl f4_il_jk neff nskip; the genome-wide means from the totals by the row's rule
    static PopsLine line(const Row &r, uint32_t sites) {
        return {{r.start, r.end, r.mid}, {mean_of(r.f4_ij_kl, r.n), mean_of(r.f4_ik_jl, r.n), mean_of(r.f4_il_jk, r.n)}, r.n, sites - r.n};
    }
    static PopsLine total(const Total &g) {
        return {{}, {mean_of(g.f4_ij_kl, g.neff), mean_of(g.f4_ik_jl, g.neff), mean_of(g.f4_il_jk, g.neff)}, g.neff, g.nskip};
    }
    // a b c d f4 f4_jack SE Z nblocks nsites: quartet order, then (i,j; k,l), (i,k; j,l), (i,l; j,k)
    static constexpr int pairings[3][4] = {{0, 1, 2, 3}, {0, 2, 1, 3}, {0, 3, 1, 2}};
    void more(PopsRun &run, const Row *d_rows) {
        if (jackknife.on) pops_jackknife(run, d_rows, pgt_f4_jackknife_dev, pgt_f4_jackknife_work_bytes, pairings);
    }
};

int main(int argc, char **argv) { return run_pops_tool<F4Pops>(argc, argv); }
