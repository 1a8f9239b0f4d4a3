// dstatWindowPops (MI355X host) — sliding-window ABBA-BABA site patterns and Patterson's D (Green et al. 2010; Durand et al.
// 2011) for ALL trios of 3 ... 6 ingroup populations against one outgroup, from their ANGSD .mafs files (plain, gzip or bgzf):
// the introgression scan that goes with the .dxy / .fst / .pi files of dxyWindowPops / fstWindowPops / piWindowPops.
// The reference has no such tool; the definition is that of pgt_dstat_pops_reduce_dev (include/pgtwin.h).
//
//   dstatWindowPops [dxyWindow's options] -out PREFIX <maf P1> ... <maf P(K-1)> <maf outgroup>        4 <= K <= 7
//
// Options, defaults, messages and exit codes are dxyWindowPops's (-winsize -stepsize -minind -fixedsite -sizefile
// -skip_missing, both window modes), and so is the front end (pops_common.h): the sites (chromosome, position) that ALL
// files list are found on the GPU and every file's columns are gathered onto them.  One pgt_dstat_pops_reduce_dev call then
// reduces all C(K-1, 3) trios: per site the expected BBAA, ABBA and BABA pattern frequencies of ((i,j),k) against the
// outgroup, counted where all four populations have at least -minind individuals; per window their sums and
// D = (ABBA - BABA) / (ABBA + BABA).
// Trio (i, j, k) -> PREFIX.pop<i+1>_pop<j+1>_pop<k+1>.dstat (`chr start end mid D BBAA ABBA BABA neff nskip`); the
// genome-wide lines -> PREFIX.global (`i+1 j+1 k+1 D BBAA ABBA BABA neff nskip`).  stdout stays empty.
// -jackknife 1 (disjoint windows only: -stepsize equal to -winsize): one pgt_dstat_jackknife_dev call on the device rows gives
// the delete-m_j block jackknife of every trio and topology, the run's windows being the blocks -> PREFIX.jackknife
// (`P1 P2 P3 D D_jack SE Z nblocks nsites`, D that of ((P1,P2),P3)).  Every other file is the same with and without it.
// -fd 1: one pgt_fd_pops_reduce_dev call more on the aligned columns still on the device (in the D tree's buffer, once D's rows
// are read: the two sizes are equal) gives f_d (Martin et al. 2015) and f_dM (Malinsky et al. 2015) of every trio ((i,j),k) ->
// PREFIX.pop<i+1>_pop<j+1>_pop<k+1>.fd (`chr start end mid f_d f_dM num fd_den fdm_den neff nskip`) and PREFIX.fd.global
// (`i+1 j+1 k+1 f_d f_dM num fd_den fdm_den neff nskip`).  Every other file is the same with and without it.
//
// Limits: one GPU (the first of PGT_DEVICES); no passes mode — the K parsed files and the aligned columns must fit the
// card (and PGT_MAX_RESIDENT_SITES, where set) or the run is refused; PGT_DXY_SYNC=reference is not offered.
#include "pops_common.h"

using namespace pgthost;

static void help(const DxyOptions &o) {
    std::printf("\ndstatWindowPops [options] -out PREFIX <pop1 maf file> ... <pop(K-1) maf file> <outgroup maf file>      (4 <= K <= 7)\n\nOptions:\n"
                "%-14s%-8sPrefix of the output files (REQUIRED)\n"
                "%-14s%-8sWindow size in base pairs (0 for global calculation) [%u]\n"
                "%-14s%-8sNumber of base pairs to progress window [%u]\n"
                "%-14s%-8sMinimum number of individuals in each of the four populations with data [%d]\n"
                "%-14s%-8s(1) Use fixed number of sites from MAF input for each window (window sizes may vary) or (0) constant window size [%d]\n"
                "%-14s%-8sTwo-column TSV file with each row having (1) chromsome name (2) chromosome size in base pairs\n"
                "%-14s%-8sDo not print windows with zero effective sites if INT=1 [%d]\n"
                "%-14s%-8s(1) Write PREFIX.jackknife: block-jackknife standard error and Z score of D for every trio and topology [0]\n"
                "%-14s%-8s(1) Write PREFIX.pop<i>_pop<j>_pop<k>.fd and PREFIX.fd.global: f_d and f_dM for every trio ((i,j),k) [0]\n"
                "\nNotes:\n"
                "* The LAST MAF file is the outgroup; the K-1 files before it are the ingroup populations (K between 4 and 7 files)\n"
                "* Every trio i < j < k of ingroup populations is analyzed as ((i,j),k) against the outgroup: C(K-1,3) trios\n"
                "* Only the sites (chromosome, position) present in ALL MAF files are analyzed\n"
                "* Per site, with p the frequencies and q = 1-p: BBAA = p_i p_j q_k q_o + q_i q_j p_k p_o, ABBA = q_i p_j p_k q_o + p_i q_j q_k p_o,\n"
                "  BABA = p_i q_j p_k q_o + q_i p_j q_k p_o; a window's values are the SUMS over its analyzed sites, D = (ABBA - BABA)/(ABBA + BABA)\n"
                "* The patterns are symmetric in the two alleles: it does not matter which allele the MAF files report,\n"
                "  but ALL files must report the frequency of the SAME allele at every site\n"
                "* The other two topologies of a trio follow from the same three sums: ((i,k),j): D = (BBAA - BABA)/(BBAA + BABA);\n"
                "  ((j,k),i): D = (BBAA - ABBA)/(BBAA + ABBA)\n"
                "* A site counts for a trio when its three populations and the outgroup each have at least -minind individuals with data\n"
                "* -jackknife 1: weighted (delete-m) block jackknife of D (Busing et al. 1999; as ADMIXTOOLS and ANGSD). The blocks are the\n"
                "  run's windows, weighted by their number of analyzed sites; windows without an analyzed site are left out.\n"
                "  The windows must not overlap: -winsize > 0 and -stepsize equal to -winsize. -fixedsite 1 windows hold the same number\n"
                "  of sites and so give blocks of (nearly) equal weight; -skip_missing does not change the blocks\n"
                "* -fd 1: f_d (Martin, Davey & Jiggins 2015) and f_dM (Malinsky et al. 2015) of ((i,j),k) = ((P1,P2),P3), in one more pass.\n"
                "  Per analyzed site num = ABBA - BABA; fd_den is the same difference with P2 and P3 both replaced by whichever of the two\n"
                "  has the higher frequency of the allele (the lower one in the term with the alleles' roles swapped); fdm_den is fd_den\n"
                "  where p_2 >= p_1, and otherwise the difference with P1 and P3 both replaced by the higher (lower) of those two.\n"
                "  A window's values are the SUMS over its analyzed sites, f_d = num/fd_den and f_dM = num/fdm_den (0 where the sum is 0)\n"
                "* f_d is meant for windows with D >= 0 (gene flow P3 -> P2); the row reports it whatever its sign\n"
                "* f_dM covers both directions: positive for P3 -> P2, negative for P3 -> P1, between -1 and 1\n"
                "* Only the topology ((i,j),k) is computed for f_d and f_dM, so the order of the MAF files chooses it\n"
                "* -fd 1 and -jackknife 1 may be given together; neither changes what the other writes\n"
                "* -sizefile is REQUIRED(!) with -fixedsite 0 (the default)\n"
                "* All input MAF files need to have the same chromosomes in the same order\n"
                "* Assumes SNPs are biallelic\n"
                "\nLimits:\n"
                "* One GPU is used (the first entry of PGT_DEVICES)\n"
                "* No passes mode: input whose parsed files plus aligned columns do not fit the GPU, or PGT_MAX_RESIDENT_SITES, is refused\n"
                "* PGT_DXY_SYNC=reference is not offered: the reference's catch-up loops are defined for two files only\n"
                "\nOutput:\nPREFIX.pop<i>_pop<j>_pop<k>.dstat for every trio i < j < k (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) D of ((i,j),k)\n(6) BBAA (sum)\n(7) ABBA (sum)\n(8) BABA (sum)\n"
                "(9) number sites in MAF input that were analyzed\n"
                "(10) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.global, one line per trio:\n(1) i\n(2) j\n(3) k\n(4) D\n(5) BBAA\n(6) ABBA\n(7) BABA\n(8) number of sites analyzed\n(9) number of sites skipped\n"
                "PREFIX.jackknife (with -jackknife 1), three lines per trio i < j < k: ((i,j),k), ((i,k),j), ((j,k),i):\n"
                "(1) P1\n(2) P2\n(3) P3: the topology ((P1,P2),P3)\n(4) D over all blocks\n(5) jackknife estimate of D\n(6) standard error\n"
                "(7) Z = (5) / (6) (nan with fewer than two blocks or a standard error of zero)\n(8) number of blocks\n(9) number of sites in the blocks\n"
                "PREFIX.pop<i>_pop<j>_pop<k>.fd (with -fd 1) for every trio i < j < k (not with -winsize 0):\n"
                "(1) chromosome\n(2) Window start\n(3) Window end\n(4) Window midpoint\n(5) f_d of ((i,j),k)\n(6) f_dM of ((i,j),k)\n(7) num (sum)\n"
                "(8) fd_den (sum)\n(9) fdm_den (sum)\n(10) number sites in MAF input that were analyzed\n"
                "(11) number of sites in MAF input that were skipped due to too few individuals\n"
                "PREFIX.fd.global (with -fd 1), one line per trio:\n(1) i\n(2) j\n(3) k\n(4) f_d\n(5) f_dM\n(6) num\n(7) fd_den\n(8) fdm_den\n"
                "(9) number of sites analyzed\n(10) number of sites skipped\n\n",
                "-out", "STRING", "-winsize", "INT", o.W, "-stepsize", "INT", o.S, "-minind", "INT", o.minind, "-fixedsite", "INT", o.fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", o.skip_missing, "-jackknife", "INT", "-fd", "INT");
}

// -fd 1: a second pass over the same columns and trios, in the D tree's buffer (the two sizes are equal; D's rows are read)
struct FdPass {
    using Row = pgt_fd_row;
    using Total = pgt_fd_total;
    static constexpr const char *ext = ".fd", *global_ext = ".fd.global";
    static constexpr size_t row_bytes = 200;
    static constexpr auto reduce_dev = pgt_fd_pops_reduce_dev;
    // chr start end mid f_d f_dM num fd_den fdm_den neff nskip; the genome-wide ratios from the totals by the row's rule
    static PopsLine line(const Row &r, uint32_t sites) { return {{r.start, r.end, r.mid}, {r.fd, r.fdm, r.num, r.fd_den, r.fdm_den}, r.n, sites - r.n}; }
    static PopsLine total(const Total &g) {
        return {{}, {g.fd_den != 0.0 ? g.num / g.fd_den : 0.0, g.fdm_den != 0.0 ? g.num / g.fdm_den : 0.0, g.num, g.fd_den, g.fdm_den}, g.neff, g.nskip};
    }
};

struct DstatPops : PopsTool {
    static constexpr const char *name = "dstatWindowPops";
    static constexpr int min_files = 4, max_files = 7;
    static constexpr auto help = ::help;
    static constexpr int arity = 3;  // all trios of the ingroups
    static constexpr bool outgroup = true;
    using Row = pgt_dstat_row;
    using Total = pgt_dstat_total;
    static constexpr const char *ext = ".dstat";
    static constexpr size_t row_bytes = 200;
    static constexpr auto tree_bytes = pgt_dstat_pops_tree_bytes;
    static constexpr auto reduce_dev = pgt_dstat_pops_reduce_dev;
    JackknifeOption jackknife;
    bool fd = false;
    bool own(const char *o, const char *v, int argc, char **argv) {
        if (std::strcmp(o, "-fd")) return jackknife.take(o, v, argc, argv);
        if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(std::string("-fd must be 0 or 1 (given: ") + v + ")");
        fd = v[0] == '1';
        return true;
    }
    // chr start end mid D BBAA ABBA BABA neff nskip; the genome-wide D from the totals
    static PopsLine line(const Row &r, uint32_t sites) { return {{r.start, r.end, r.mid}, {r.d, r.bbaa, r.abba, r.baba}, r.n, sites - r.n}; }
    static PopsLine total(const Total &g) {
        const double den = g.abba + g.baba;
        return {{}, {den != 0.0 ? (g.abba - g.baba) / den : 0.0, g.bbaa, g.abba, g.baba}, g.neff, g.nskip};
    }
    // P1 P2 P3 D D_jack SE Z nblocks nsites: trio order, then ((i,j),k), ((i,k),j), ((j,k),i)
    static constexpr int topologies[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
    void more(PopsRun &run, const Row *d_rows) {
        if (jackknife.on) pops_jackknife(run, d_rows, pgt_dstat_jackknife_dev, pgt_dstat_jackknife_work_bytes, topologies);
        if (fd) pops_pass(FdPass{}, run);
    }
};

int main(int argc, char **argv) { return run_pops_tool<DstatPops>(argc, argv); }
