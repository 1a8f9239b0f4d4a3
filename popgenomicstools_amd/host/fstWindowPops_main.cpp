// fstWindowPops (MI355X host) — sliding-window FST of ALL pairs of 2 ... 8 populations from their ANGSD .mafs files
// (plain, gzip or bgzf), one output file per pair: the FST counterpart of dxyWindowPops beside this file.
//
//   fstWindowPops [dxyWindow's options] -out PREFIX <maf 1> <maf 2> ... <maf K>
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): the sites (chromosome, position) that ALL
// files list are found on the GPU and every file's columns are gathered onto them.  One pgt_fst_pops_reduce_dev call then
// reduces all K(K-1)/2 pairs: per site and pair the two columns of WCFst() (betaAFOutlier.R:405-417) with the site's nInd
// as the sample sizes, counted where both populations have at least -minind individuals (dxyWindow.cpp:381); per window
// fstWindow's statistic Σa / Σ(a+b) (fstWindow.cpp:85).
// -estimator hudson: pgt_fst_hudson_pops_reduce_dev instead — Hudson's ratio of averages, Σ[(p1-p2)² - h1 - h2] / Σ dxy with
// h = p(1-p)/(2 nInd - 1) (include/pgtwin.h); files, rows and counts are laid out the same.  -estimator wc is the default.
// Pair (i, j) of pair order (0,1),(0,2),..,(1,2),.. -> PREFIX.pop<i+1>_pop<j+1>.fst with fstWindow's row and the skipped
// count (`chr start end mid fst neff nskip`); the genome-wide lines of all pairs (genomeFst, betaAFOutlier.R:440-446)
// -> PREFIX.global (`i+1  j+1  fst  neff  nskip`).  stdout stays empty.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\nfstWindowPops [options] -out PREFIX <pop1 maf file> <pop2 maf file> ... <popK maf file>      (2 <= K <= 8)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each population with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8sFST estimator: wc (Weir-Cockerham components) or hudson (Hudson's ratio of averages) [wc]\n"
                "\nNotes:\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* FST is the ratio of the summed Reynolds / Weir-Cockerham variance components, the per-site sample sizes being the MAF files' nInd\n"
                "* -estimator hudson: FST is sum[(p1-p2)^2 - h1 - h2] / sum[dxy] with h = p(1-p)/(2 nInd - 1): its denominator is dxy (dxyWindowPops' sum)\n"
                "* A site counts for a pair when both populations have at least -minind individuals with data\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic across populations\n"
                "\nLimits:\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>.fst for every pair i < j (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint position\n(5) Fst\n"
                "(6) number sites in MAF input that were analyzed\n"
                "(7) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per pair:\n(1) i\n(2) j\n(3) Fst\n(4) number of sites analyzed\n(5) number of sites skipped\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-estimator", "STRING");
}

struct FstPops : PopsTool {
    static constexpr const char *name = "fstWindowPops";
    static constexpr int min_files = 2;
    static constexpr auto help = ::help;
    static constexpr int arity = 2;  // all pairs
    using Row = pgt_fst_row;
    using Total = pgt_fst_total;
    static constexpr const char *ext = ".fst";
    static constexpr size_t row_bytes = 100;
    static constexpr auto tree_bytes = pgt_fst_pops_tree_bytes;  // one size for both estimators
    decltype(&pgt_fst_pops_reduce_dev) reduce_dev = pgt_fst_pops_reduce_dev;
    bool own(const char *o, const char *v, int, char **) {
        if (std::strcmp(o, "-estimator")) return false;
        if (!std::strcmp(v, "hudson")) reduce_dev = pgt_fst_hudson_pops_reduce_dev;
        else if (!std::strcmp(v, "wc")) reduce_dev = pgt_fst_pops_reduce_dev;
        else die(std::string("-estimator must be wc or hudson (given: ") + v + ")");
        return true;
    }
    // chr start end mid fst neff nskip: fstWindow's row (fstWindow.cpp:88) and the skipped count
    static PopsLine line(const Row &r, uint32_t sites) { return {{r.start, r.end, r.mid}, {r.fst}, r.n, sites - r.n}; }
    static PopsLine total(const Total &g) { return {{}, {g.bsum != 0.0 ? g.asum / g.bsum : 0.0}, g.neff, g.nskip}; }
};

int main(int argc, char **argv) { return run_pops_tool<FstPops>(argc, argv); }
