// f3WindowPops (MI355X host) — sliding-window f3 (Reich et al. 2009; Patterson et al. 2012; treemix's threepop, ADMIXTOOLS'
// qp3Pop without its normalisation) for ALL trios of 3 ... 6 populations, every population of a trio as the target, from their
// ANGSD .mafs files (plain, gzip or bgzf): the admixture test that goes with the .dxy / .fst / .pi / .dstat files of
// dxyWindowPops / fstWindowPops / piWindowPops / dstatWindowPops, and it needs no outgroup.
// The reference has no such tool; the definition is that of pgt_f3_pops_reduce_dev (include/pgtwin.h).
//
//   f3WindowPops [dxyWindow's options] -out PREFIX <maf 1> ... <maf K>        3 <= K <= 6
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): the sites (chromosome, position) that ALL
// files list are found on the GPU and every file's columns are gathered onto them.  One pgt_f3_pops_reduce_dev call then
// reduces all C(K, 3) trios: per site (p_x - p_a)(p_x - p_b) - p_x (1 - p_x) / (2 n_x - 1) for each target x of the trio and its
// two sources a, b, counted where all three populations have at least -minind individuals; per window their sums, and the
// mean f3 = sum / neff formed here.
// Trio (i, j, k) -> PREFIX.pop<i+1>_pop<j+1>_pop<k+1>.f3 (`chr start end mid f3_i f3_j f3_k neff nskip`); the genome-wide
// lines -> PREFIX.global (`i+1 j+1 k+1 f3_i f3_j f3_k neff nskip`).  stdout stays empty.
// -jackknife 1 (disjoint windows only: -stepsize not below -winsize): one pgt_f3_jackknife_dev call on the device rows gives
// the delete-m_j block jackknife of every trio and target, the run's windows being the blocks -> PREFIX.jackknife
// (`target src1 src2 f3 f3_jack SE Z nblocks nsites`).  Every other file is the same with and without it.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\nf3WindowPops [options] -out PREFIX <pop1 maf file> ... <popK maf file>      (3 <= K <= 6)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each of the three populations with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8s(1) Write PREFIX.jackknife: block-jackknife standard error and Z score of f3 for every trio and target [0]\n"
                "\nNotes:\n"
                "* ALL populations are equal: there is no outgroup file (K between 3 and 6 files)\n"
                "* Every trio i < j < k of populations is analyzed three times, with i, j and k in turn as the target: C(K,3) trios\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* Per site, with p the frequencies and n the numbers of individuals with data, for the target x and its sources a, b:\n"
                "  f3(x; a, b) = (p_x - p_a)(p_x - p_b) - p_x (1 - p_x)/(2 n_x - 1); a window's value is the MEAN over its analyzed sites\n"
                "  (0 for a window without one). The second term removes the bias the target's finite sample adds to p_x^2\n"
                "* The statistic is symmetric in the two alleles: it does not matter which allele the MAF files report,\n"
                "  but ALL files must report the frequency of the SAME allele at every site\n"
                "* A site counts for a trio when its three populations each have at least -minind individuals with data\n"
                "* A significantly NEGATIVE f3(x; a, b) (Z below about -3) shows that x is admixed between populations related to a and b;\n"
                "  a value that is not negative proves nothing\n"
                "* Outgroup f3: with an outgroup O among the files, f3(O; a, b) measures the genetic drift a and b share since they split\n"
                "  from O: the larger, the closer a and b\n"
                "* -jackknife 1: weighted (delete-m) block jackknife of f3 (Busing et al. 1999; as ADMIXTOOLS). The blocks are the\n"
                "  run's windows, weighted by their number of analyzed sites; windows without an analyzed site are left out.\n"
                "  The windows must not overlap: -winsize > 0 and -stepsize not below -winsize. -fixedsite 1 windows hold the same number\n"
                "  of sites and so give blocks of (nearly) equal weight; -skip_missing does not change the blocks\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic\n"
                "\nLimits:\n"
                "* Not computed: f3 normalised by the target's heterozygosity (qp3Pop's default), f4, user-chosen trio lists\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>_pop<k>.f3 for every trio i < j < k (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) f3(i; j, k): population i as the target\n"
                "(6) f3(j; i, k)\n(7) f3(k; i, j)\n"
                "(8) number sites in MAF input that were analyzed\n"
                "(9) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per trio:\n(1) i\n(2) j\n(3) k\n(4) f3(i; j, k)\n(5) f3(j; i, k)\n(6) f3(k; i, j)\n(7) number of sites analyzed\n(8) number of sites skipped\n"
                "PREFIX.jackknife (with -jackknife 1), three lines per trio i < j < k: (i; j,k), (j; i,k), (k; i,j):\n"
                "(1) target\n(2) source 1\n(3) source 2\n(4) f3 over all blocks\n(5) jackknife estimate of f3\n(6) standard error\n"
                "(7) Z = (5) / (6) (nan with fewer than two blocks or a standard error of zero)\n(8) number of blocks\n(9) number of sites in the blocks\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-jackknife", "INT");
}

static double mean_of(double sum, uint64_t neff) { return neff ? sum / (double)neff : 0.0; }

struct F3Pops : PopsTool {
    static constexpr const char *name = "f3WindowPops";
    static constexpr int min_files = 3, max_files = 6;
    static constexpr auto help = ::help;
    static constexpr int arity = 3;  // all trios
    using Row = pgt_f3_row;
    using Total = pgt_f3_total;
    static constexpr const char *ext = ".f3";
    static constexpr size_t row_bytes = 200;
    static constexpr auto tree_bytes = pgt_f3_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_f3_pops_reduce_dev;
    JackknifeOption jackknife;
    bool own(const char *o, const char *v, int argc, char **argv) { return jackknife.take(o, v, argc, argv); }
    // chr start end mid f3_i f3_j f3_k neff nskip; the genome-wide means from the totals by the row's rule
    static PopsLine line(const Row &r, uint32_t sites) {
        return {{r.start, r.end, r.mid}, {mean_of(r.f3_i, r.n), mean_of(r.f3_j, r.n), mean_of(r.f3_k, r.n)}, r.n, sites - r.n};
    }
    static PopsLine total(const Total &g) { return {{}, {mean_of(g.f3_i, g.neff), mean_of(g.f3_j, g.neff), mean_of(g.f3_k, g.neff)}, g.neff, g.nskip}; }
    // target src1 src2 f3 f3_jack SE Z nblocks nsites: trio order, then (i; j,k), (j; i,k), (k; i,j)
    static constexpr int targets[3][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}};
    void more(PopsRun &run, const Row *d_rows) {
        if (jackknife.on) pops_jackknife(run, d_rows, pgt_f3_jackknife_dev, pgt_f3_jackknife_work_bytes, targets);
    }
};

int main(int argc, char **argv) { return run_pops_tool<F3Pops>(argc, argv); }
