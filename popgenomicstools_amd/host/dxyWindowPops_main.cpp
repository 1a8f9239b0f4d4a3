// dxyWindowPops (MI355X host) — sliding-window dxy of ALL pairs of 2 ... 8 populations from their ANGSD .mafs files
// (plain, gzip or bgzf), one output file per pair.
//
//   dxyWindowPops [dxyWindow's options] -out PREFIX <maf 1> <maf 2> ... <maf K>
//
// Options, defaults, messages, exit codes and the row format are those of the dxyWindow host beside this file (the
// reference's dxyWindow.cpp:34-61 help, :63-139 arguments, :190 row, :429-433 genome-wide line).  What is new is the
// K-file form of the reference's site synchronisation (dxyWindow.cpp:315-331): the sites (chromosome, position) that ALL
// files list are found on the GPU (pgt_align_segments + pgt_sites_align), every file's columns are gathered onto them
// (pgt_gather_dev), and one pgt_dxy_pops_reduce_dev call reduces all K(K-1)/2 pairs over the shared position column.
// Pair (i, j) of pair order (0,1),(0,2),..,(1,2),.. -> PREFIX.pop<i+1>_pop<j+1>.dxy; the genome-wide lines of all pairs
// -> PREFIX.global (`i+1  j+1  dxy  neff  nskip`).  stdout stays empty.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered (the
// reference's catch-up loops are defined for two files only).
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\ndxyWindowPops [options] -out PREFIX <pop1 maf file> <pop2 maf file> ... <popK maf file>      (2 <= K <= 8)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each population with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "\nNotes:\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* -winsize 1 -stepsize 1 calculates per site dxy\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic across populations\n"
                "* Input MAF files can contain all sites (including monomorphic sites) or just variable sites\n"
                "\nLimits:\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>.dxy for every pair i < j (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) dxy\n"
                "(5) number sites in MAF input that were analyzed\n"
                "(6) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per pair:\n(1) i\n(2) j\n(3) dxy\n(4) number of sites analyzed\n(5) number of sites skipped\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing);
}


struct DxyPops : PopsTool {
    static constexpr const char *name = "dxyWindowPops";
    static constexpr int min_files = 2;
    static constexpr auto help = ::help;
    static constexpr int arity = 2;  // all pairs
    using Row = pgt_dxy_row;
    using Total = pgt_dxy_total;
    static constexpr const char *ext = ".dxy";
    static constexpr size_t row_bytes = 80;
    static constexpr auto tree_bytes = pgt_dxy_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_dxy_pops_reduce_dev;
    // chr start end dxy neff nskip: dxyWindow's row (dxyWindow.cpp:190), the skipped count the library's
    static PopsLine line(const Row &r, uint32_t) { return {{r.start, r.end}, {r.sum}, r.neff, r.nskip}; }
    static PopsLine total(const Total &g) { return {{}, {g.sum}, g.neff, g.nskip}; }
};

int main(int argc, char **argv) { return run_pops_tool<DxyPops>(argc, argv); }
