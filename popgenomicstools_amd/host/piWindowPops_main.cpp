// piWindowPops (MI355X host) — sliding-window nucleotide diversity (pi) of each of 1 ... 8 populations from their ANGSD
// .mafs files (plain, gzip or bgzf), one output file per population: the within-population statistic that the .dxy and
// .fst files of dxyWindowPops / fstWindowPops beside this file are read against (net divergence = dxy - (pi_1 + pi_2)/2).
// The reference has no tool that computes pi; the definition is that of pgt_pi_pops_reduce_dev (include/pgtwin.h).
//
//   piWindowPops [dxyWindow's options] -out PREFIX <maf 1> ... <maf K>
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): with K >= 2 the sites (chromosome, position)
// that ALL files list are found on the GPU and every file's columns are gathered onto them, so the rows line up with the
// .dxy / .fst rows of the same files; ONE file is analysed at all its sites.  One pgt_pi_pops_reduce_dev call then reduces
// all K populations: per site 2p(1-p) 2n/(2n-1) with n the site's nInd, counted where the population has at least -minind
// individuals; per window the SUM over the counted sites, as dxyWindow prints its sum (dxyWindow.cpp:190).
// Population i -> PREFIX.pop<i+1>.pi with dxyWindow's row (`chr start end pi_sum neff nskip`); the genome-wide lines
// -> PREFIX.global (`i+1  pi_sum  neff  nskip`).  stdout stays empty.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\npiWindowPops [options] -out PREFIX <pop1 maf file> ... <popK maf file>      (1 <= K <= 8)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in the population with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "\nNotes:\n"
                "* With more than one MAF file only the sites (chromosome, position) present in ALL of them are analyzed\n"
                "* Per site pi is 2p(1-p) * 2n/(2n-1), n being the MAF file's nInd; a window's value is the SUM over its analyzed sites\n"
                "* A site counts for a population when it has at least -minind individuals with data\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic\n"
                "\nLimits:\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>.pi for every population i (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) pi (sum over the analyzed sites)\n"
                "(5) number sites in MAF input that were analyzed\n"
                "(6) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per population:\n(1) i\n(2) pi (sum)\n(3) number of sites analyzed\n(4) number of sites skipped\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing);
}

struct PiPops : PopsTool {
    static constexpr const char *name = "piWindowPops";
    static constexpr int min_files = 1;
    static constexpr auto help = ::help;
    static constexpr int arity = 1;  // each population
    using Row = pgt_dxy_row;
    using Total = pgt_dxy_total;
    static constexpr const char *ext = ".pi";
    static constexpr size_t row_bytes = 80;
    static constexpr auto tree_bytes = pgt_pi_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_pi_pops_reduce_dev;
    static constexpr bool window_hints = true;  // the only one of the five tools that sets them
    // chr start end pi_sum neff nskip: dxyWindow's row (dxyWindow.cpp:190), the skipped count the library's
    static PopsLine line(const Row &r, uint32_t) { return {{r.start, r.end}, {r.sum}, r.neff, r.nskip}; }
    static PopsLine total(const Total &g) { return {{}, {g.sum}, g.neff, g.nskip}; }
};

int main(int argc, char **argv) { return run_pops_tool<PiPops>(argc, argv); }
