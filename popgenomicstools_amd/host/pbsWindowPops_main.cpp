// pbsWindowPops (MI355X host) — the sliding-window population branch statistic (PBS; Yi et al. 2010) for ALL trios of 3 ... 6
// populations, every population of a trio as the focal one, from their ANGSD .mafs files (plain, gzip or bgzf): the selection
// scan that goes with the .dxy / .fst / .pi / .dstat / .f3 files of the other K-population tools.
// The reference has no such tool; the definition is that of pgt_pbs_pops_reduce_dev (include/pgtwin.h).
//
//   pbsWindowPops [dxyWindow's options] [-estimator wc|hudson] [-pbsn1 0|1] [-blockjack 0|1] -out PREFIX <maf 1> ... <maf K>        3 <= K <= 6
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes) with fstWindowPops' -estimator, and so is the front end (pops_common.h): the sites
// (chromosome, position) that ALL files list are found on the GPU and every file's columns are gathered onto them.  One
// pgt_pbs_pops_reduce_dev (or pgt_pbs_hudson_pops_reduce_dev) call then reduces all C(K, 3) trios: per window the FST numerator
// and denominator of the trio's three pairs summed over the sites where ALL THREE populations have at least -minind
// individuals, and from them T = -log(1 - FST) per pair and PBS = (T_focal,a + T_focal,b - T_a,b) / 2 per focal population.
// Trio (i, j, k) -> PREFIX.pop<i+1>_pop<j+1>_pop<k+1>.pbs (`chr start end mid pbs_i pbs_j pbs_k fst_ij fst_ik fst_jk neff nskip`);
// the genome-wide lines -> PREFIX.global (`i+1 j+1 k+1 pbs_i pbs_j pbs_k fst_ij fst_ik fst_jk neff nskip`).  stdout stays empty.
// -pbsn1 1: PBSn1 = PBS / (1 + PBS_i + PBS_j + PBS_k) (Malaspinas et al. 2016) of every row and genome-wide line, formed here from
// the row's own three PBS -> PREFIX.pop<i+1>_pop<j+1>_pop<k+1>.pbsn1 (`chr start end mid pbsn1_i pbsn1_j pbsn1_k neff nskip`) and
// PREFIX.pbsn1.global.
// -blockjack 1 (disjoint windows only: -stepsize not below -winsize): one pgt_pbs_jackknife_dev call on the device rows gives the
// delete-m_j block jackknife of the genome-wide PBS and PBSn1 of every trio and focal population, the run's windows being the
// blocks -> PREFIX.jackknife (`stat focal other1 other2 value value_jack SE Z nblocks nsites`, six lines per trio).  The option is
// not called -jackknife: this tool has always answered `Unknown command` to that name.  Every other file is the same with and
// without either option.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include <limits>

#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\npbsWindowPops [options] -out PREFIX <pop1 maf file> ... <popK maf file>      (3 <= K <= 6)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each of the three populations with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8sFST estimator: wc (Weir-Cockerham components) or hudson (Hudson's ratio of averages) [wc]\n"
                "%-14s%-8s(1) Write PREFIX.pop<i>_pop<j>_pop<k>.pbsn1 and PREFIX.pbsn1.global: the normalised branch statistic PBSn1 [0]\n"
                "%-14s%-8s(1) Write PREFIX.jackknife: block jackknife standard error and Z score of the genome-wide PBS and PBSn1 [0]\n"
                "\nNotes:\n"
                "* ALL populations are equal (K between 3 and 6 files): every trio i < j < k of populations is analyzed, and reported\n"
                "  with i, j and k in turn as the focal population: C(K,3) trios\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* A site counts for a trio when ALL THREE of its populations have at least -minind individuals with data. The FST of\n"
                "  each of the trio's pairs is the ratio of that pair's summed numerator and denominator over THESE sites, so that the\n"
                "  three branch lengths are measured on the same sites (as ANGSD's realSFS fst does with three populations)\n"
                "* The .fst files of fstWindowPops count a pair's site whatever the third population holds: they differ from the FST\n"
                "  columns here wherever the third population lacks data\n"
                "* Per pair T = -log(1 - FST); PBS of the focal population x with the others a, b is (T_xa + T_xb - T_ab) / 2\n"
                "* FST is the estimator of fstWindowPops: the summed Weir-Cockerham components with the MAF files' nInd as the sample\n"
                "  sizes, or with -estimator hudson sum[(p1-p2)^2 - h1 - h2] / sum[dxy], h = p(1-p)/(2 nInd - 1)\n"
                "* Nothing is clamped: a negative FST gives a negative T and may give a negative PBS. inf: a pair of the trio has\n"
                "  FST = 1 in the window (fixed differences only), so its T is infinite. nan: two such pairs cancel (inf - inf)\n"
                "* A window without an analyzed site reports 0 in every column\n"
                "* -pbsn1 1: PBSn1 of the focal population x is PBS_x / (1 + PBS_i + PBS_j + PBS_k) (Malaspinas et al. 2016): raw PBS is\n"
                "  inflated wherever all three branches are long; PBSn1 is comparable between regions. It is not clamped either\n"
                "* -blockjack 1: weighted (delete-m) block jackknife (Busing et al. 1999) of the genome-wide PBS and PBSn1: a block is left\n"
                "  out of all six FST sums of the trio together. The blocks are the run's windows, weighted by their number of analyzed\n"
                "  sites; windows without an analyzed site are left out.\n"
                "  The windows must not overlap: -winsize > 0 and -stepsize not below -winsize. -fixedsite 1 windows hold the same number\n"
                "  of sites and so give blocks of (nearly) equal weight; -skip_missing does not change the blocks\n"
                "* The block jackknife is -blockjack, not -jackknife: this tool answers Unknown command to -jackknife, as it always has\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic across populations\n"
                "\nLimits:\n"
                "* Not computed: FST truncated at 0, user-chosen trio lists\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>_pop<k>.pbs for every trio i < j < k (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) PBS with population i as the focal one\n"
                "(6) PBS of j\n(7) PBS of k\n(8) Fst of (i, j) over the trio's sites\n(9) Fst of (i, k)\n(10) Fst of (j, k)\n"
                "(11) number sites in MAF input that were analyzed\n"
                "(12) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per trio:\n(1) i\n(2) j\n(3) k\n(4) PBS of i\n(5) PBS of j\n(6) PBS of k\n(7) Fst of (i, j)\n(8) Fst of (i, k)\n"
                "(9) Fst of (j, k)\n(10) number of sites analyzed\n(11) number of sites skipped\n"
                "PREFIX.pop<i>_pop<j>_pop<k>.pbsn1 (with -pbsn1 1; not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) PBSn1 with population i as the focal one\n"
                "(6) PBSn1 of j\n(7) PBSn1 of k\n(8) number of sites analyzed\n(9) number of sites skipped\n"
                "PREFIX.pbsn1.global (with -pbsn1 1), one line per trio:\n(1) i\n(2) j\n(3) k\n(4) PBSn1 of i\n(5) PBSn1 of j\n(6) PBSn1 of k\n"
                "(7) number of sites analyzed\n(8) number of sites skipped\n"
                "PREFIX.jackknife (with -blockjack 1), six lines per trio i < j < k: pbs of i, j, k, then pbsn1 of i, j, k:\n"
                "(1) pbs or pbsn1\n(2) focal population\n(3) (4) the other two\n(5) the statistic over all blocks\n(6) its jackknife estimate\n"
                "(7) standard error\n(8) Z = (6) / (7) (nan with fewer than two blocks or a standard error of zero)\n(9) number of blocks\n"
                "(10) number of sites in the blocks\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-estimator", "STRING", "-pbsn1", "INT", "-blockjack", "INT");
}

static double fst_of(double num, double den) { return den != 0.0 ? num / den : 0.0; }  // fstWindow.cpp:85
// a NaN is printed as `nan` whatever its sign bit
static double plain(double v) { return v != v ? std::numeric_limits<double>::quiet_NaN() : v; }

// PBSn1 of the three focal populations from a row's (or a total's) own three PBS: s = (pbs_i + pbs_j) + pbs_k, pbs_x / (1.0 + s)
template <class R>
static PopsLine pbsn1_values(std::initializer_list<uint32_t> lead, const R &r, uint64_t n, uint64_t nskip) {
    const double s = (r.pbs_i + r.pbs_j) + r.pbs_k;
    const double one_s = 1.0 + s;
    return {lead, {plain(r.pbs_i / one_s), plain(r.pbs_j / one_s), plain(r.pbs_k / one_s)}, n, nskip};
}
// the files of -pbsn1 1, from the rows and totals of the one reduction
struct Pbsn1Files {
    static constexpr const char *ext = ".pbsn1";
    static constexpr const char *global_ext = ".pbsn1.global";
    static constexpr size_t row_bytes = 200;
    static PopsLine line(const pgt_pbs_row &r, uint32_t sites) { return pbsn1_values({r.start, r.end, r.mid}, r, r.n, sites - r.n); }
    static PopsLine total(const pgt_pbs_total &g) { return pbsn1_values({}, g, g.neff, g.nskip); }
};

struct PbsPops : PopsTool {
    static constexpr const char *name = "pbsWindowPops";
    static constexpr int min_files = 3, max_files = 6;
    static constexpr auto help = ::help;
    static constexpr int arity = 3;  // all trios
    using Row = pgt_pbs_row;
    using Total = pgt_pbs_total;
    static constexpr const char *ext = ".pbs";
    static constexpr size_t row_bytes = 300;
    static constexpr auto tree_bytes = pgt_pbs_pops_work_bytes;  // one size for both estimators; it knows the window count
    decltype(&pgt_pbs_pops_reduce_dev) reduce_dev = pgt_pbs_pops_reduce_dev;
    JackknifeOption blockjack;
    bool pbsn1 = false;
    bool own(const char *o, const char *v, int argc, char **argv) {
        if (blockjack.take(o, v, argc, argv, "-blockjack")) return true;
        if (!std::strcmp(o, "-pbsn1")) {
            if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(std::string("-pbsn1 must be 0 or 1 (given: ") + v + ")");
            pbsn1 = v[0] == '1';
            return true;
        }
        if (std::strcmp(o, "-estimator")) return false;
        if (!std::strcmp(v, "hudson")) reduce_dev = pgt_pbs_hudson_pops_reduce_dev;
        else if (!std::strcmp(v, "wc")) reduce_dev = pgt_pbs_pops_reduce_dev;
        else die(std::string("-estimator must be wc or hudson (given: ") + v + ")");
        return true;
    }
    // chr start end mid pbs_i pbs_j pbs_k fst_ij fst_ik fst_jk neff nskip
    template <class R>
    static PopsLine values(std::initializer_list<uint32_t> lead, const R &r, uint64_t n, uint64_t nskip) {
        return {lead, {plain(r.pbs_i), plain(r.pbs_j), plain(r.pbs_k), plain(fst_of(r.num_ij, r.den_ij)), plain(fst_of(r.num_ik, r.den_ik)),
                       plain(fst_of(r.num_jk, r.den_jk))}, n, nskip};
    }
    static PopsLine line(const Row &r, uint32_t sites) { return values({r.start, r.end, r.mid}, r, r.n, sites - r.n); }
    static PopsLine total(const Total &g) { return values({}, g, g.neff, g.nskip); }
    // stat focal other1 other2 value value_jack SE Z nblocks nsites: trio order, then pbs of i, j, k and pbsn1 of i, j, k
    static constexpr int items[6][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}, {0, 1, 2}, {1, 0, 2}, {2, 0, 1}};
    static constexpr const char *labels[6] = {"pbs", "pbs", "pbs", "pbsn1", "pbsn1", "pbsn1"};
    static constexpr bool host_rows = true;  // the .pbsn1 files are written from the rows of the one reduction
    void more(PopsRun &run, const Row *d_rows, const PopsHostRows<Row, Total> &host) {
        if (pbsn1) pops_queue_files<Pbsn1Files>(run, host.rows, host.tot);
        if (blockjack.on) pops_jackknife(run, d_rows, pgt_pbs_jackknife_dev, pgt_pbs_jackknife_work_bytes, items, labels);
    }
};

int main(int argc, char **argv) { return run_pops_tool<PbsPops>(argc, argv); }
