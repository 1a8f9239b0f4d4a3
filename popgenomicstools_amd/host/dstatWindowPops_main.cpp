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

// chr start end mid D BBAA ABBA BABA neff nskip
static size_t put_dstat_row(char *o, const std::string &chr, const pgt_dstat_row &r, uint32_t nskip) {
    char *p = o;
    std::memcpy(p, chr.data(), chr.size());
    p += chr.size();
    for (uint32_t u : {r.start, r.end, r.mid}) { *p++ = '\t'; p = put_u32(p, u); }
    for (double g : {r.d, r.bbaa, r.abba, r.baba}) { *p++ = '\t'; p += fmt_g6(g, p); }
    for (uint32_t u : {r.n, nskip}) { *p++ = '\t'; p = put_u32(p, u); }
    *p++ = '\n';
    return (size_t)(p - o);
}

// chr start end mid f_d f_dM num fd_den fdm_den neff nskip
static size_t put_fd_row(char *o, const std::string &chr, const pgt_fd_row &r, uint32_t nskip) {
    char *p = o;
    std::memcpy(p, chr.data(), chr.size());
    p += chr.size();
    for (uint32_t u : {r.start, r.end, r.mid}) { *p++ = '\t'; p = put_u32(p, u); }
    for (double g : {r.fd, r.fdm, r.num, r.fd_den, r.fdm_den}) { *p++ = '\t'; p += fmt_g6(g, p); }
    for (uint32_t u : {r.n, nskip}) { *p++ = '\t'; p = put_u32(p, u); }
    *p++ = '\n';
    return (size_t)(p - o);
}

int main(int argc, char **argv) {
    const std::string tool = "dstatWindowPops";
    int jackknife = 0, fd = 0;
    const PopsArgs args = parse_pops_args(tool, argc, argv, help, 4, [&](const char *o, const char *v) {
        if (!std::strcmp(o, "-fd")) {
            if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(std::string("-fd must be 0 or 1 (given: ") + v + ")");
            fd = v[0] == '1';
            return true;
        }
        if (std::strcmp(o, "-jackknife")) return false;
        if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(std::string("-jackknife must be 0 or 1 (given: ") + v + ")");
        jackknife = v[0] == '1';
        if (!jackknife) return true;
        // refused here, while the options are read and before any file is opened: the blocks are the run's windows, which
        // must exist and be disjoint (the option pairs are walked as parse_pops_args walks them; the last value counts)
        DxyOptions w;
        for (int i = 1; i + 1 < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2)
            if (!std::strcmp(argv[i], "-winsize") || !std::strcmp(argv[i], "-stepsize")) dxy_option(w, argv[i], argv[i + 1]);
        if (w.W == 0) die("-jackknife 1 needs windows as its blocks: -winsize must be > 0");
        if (w.S < w.W)
            die("-jackknife 1 needs windows that do not overlap: -stepsize (" + std::to_string(w.S) + ") must not be below -winsize (" + std::to_string(w.W) + ")");
        return true;
    }, 7);
    const int K = args.K;
    const char *prefix = args.prefix;
    const uint32_t W = args.opt.W;
    const int minind = args.opt.minind, skip_missing = args.opt.skip_missing;

    PhaseTimer timer;
    DeviceOpener device(std::vector<int>{devices_from_env()[0]});  // one GPU; HIP start-up runs beside the opening of the files
    const PopsSites s = load_pops(tool, args, timer, device);
    pgt_ctx *ctx = s.ctx;
    const std::vector<pgt_win> &win = s.win;
    const Runs &runs = s.runs;
    const size_t n_trios = (size_t)(K - 1) * (size_t)(K - 2) * (size_t)(K - 3) / 6, n_win = win.size();
    pgt_dstat_row *d_rows = pops_dev_alloc<pgt_dstat_row>(ctx, n_trios * n_win);
    pgt_dstat_total *d_tot = pops_dev_alloc<pgt_dstat_total>(ctx, n_trios);
    const size_t tree_bytes = pgt_dstat_pops_tree_bytes((uint32_t)K, s.n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    check(pgt_dstat_pops_reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
                                    n_win ? d_rows : nullptr, n_trios * n_win * sizeof(pgt_dstat_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_dstat_row> rows(n_trios * n_win);
    std::vector<pgt_dstat_total> tot(n_trios);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_trios * n_win * sizeof(pgt_dstat_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_trios * sizeof(pgt_dstat_total), nullptr), ctx);
    std::vector<pgt_dstat_jack> jack;
    if (jackknife) {  // the rows are still on the device: every window of the table is a block
        const size_t work_bytes = pgt_dstat_jackknife_work_bytes((uint32_t)n_trios, n_win);
        void *work = nullptr;
        check(pgt_dev_alloc(ctx, work_bytes, &work), ctx);
        pgt_dstat_jack *d_jack = pops_dev_alloc<pgt_dstat_jack>(ctx, 3 * n_trios);
        check(pgt_dstat_jackknife_dev(ctx, d_rows, n_win, (uint32_t)n_trios, d_jack, 3 * n_trios * sizeof(pgt_dstat_jack), work, work_bytes, nullptr), ctx);
        jack.resize(3 * n_trios);
        check(pgt_rowbuf_read(ctx, jack.data(), d_jack, 3 * n_trios * sizeof(pgt_dstat_jack), nullptr), ctx);
    }
    RowArray<pgt_fd_row> fd_rows(fd ? n_trios * n_win : 0);
    std::vector<pgt_fd_total> fd_tot(fd ? n_trios : 0);
    if (fd) {  // a second reduction of the aligned columns; D's rows are read, so its tree's buffer (the same size) is free
        pgt_fd_row *d_fd_rows = pops_dev_alloc<pgt_fd_row>(ctx, n_trios * n_win);
        pgt_fd_total *d_fd_tot = pops_dev_alloc<pgt_fd_total>(ctx, n_trios);
        check(pgt_fd_pops_reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
                                     n_win ? d_fd_rows : nullptr, n_trios * n_win * sizeof(pgt_fd_row), d_fd_tot, tree, tree_bytes, nullptr), ctx);
        check(pgt_rowbuf_read(ctx, fd_rows.data(), d_fd_rows, n_trios * n_win * sizeof(pgt_fd_row), nullptr), ctx);
        check(pgt_rowbuf_read(ctx, fd_tot.data(), d_fd_tot, n_trios * sizeof(pgt_fd_total), nullptr), ctx);
    }
    timer.lap("gpu reduce");

    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    size_t t = 0;
    for (int a = 0; a < K - 1; ++a)
        for (int b = a + 1; b < K - 1; ++b)
            for (int c = b + 1; c < K - 1; ++c, ++t) {
                if (W > 0) {
                    const std::string path = std::string(prefix) + ".pop" + std::to_string(a + 1) + "_pop" + std::to_string(b + 1) + "_pop" + std::to_string(c + 1) + ".dstat";
                    FILE *f = open_out(path);
                    const pgt_dstat_row *r = rows.data() + t * n_win;
                    write_rows(n_win, longest_name(runs) + 200, [&](size_t i, char *o) -> size_t {  // -skip_missing as dxyWindow.cpp:189
                        if (!(r[i].n > 0 || !skip_missing)) return 0;
                        return put_dstat_row(o, runs.name[win[i].label_run], r[i], (uint32_t)(win[i].hi - win[i].lo) - r[i].n);
                    }, f);
                    close_out(f, path);
                }
                const double den = tot[t].abba + tot[t].baba;
                const double d = den != 0.0 ? (tot[t].abba - tot[t].baba) / den : 0.0;
                std::fprintf(global, "%d\t%d\t%d\t%g\t%g\t%g\t%g\t%llu\t%llu\n", a + 1, b + 1, c + 1, d, tot[t].bbaa, tot[t].abba, tot[t].baba,
                             (unsigned long long)tot[t].neff, (unsigned long long)tot[t].nskip);
            }
    close_out(global, global_path);
    if (jackknife) {  // P1 P2 P3 D D_jack SE Z nblocks nsites: trio order, then ((i,j),k), ((i,k),j), ((j,k),i)
        const std::string path = std::string(prefix) + ".jackknife";
        FILE *f = open_out(path);
        t = 0;
        for (int a = 0; a < K - 1; ++a)
            for (int b = a + 1; b < K - 1; ++b)
                for (int c = b + 1; c < K - 1; ++c, ++t) {
                    const int topo[3][3] = {{a, b, c}, {a, c, b}, {b, c, a}};
                    for (int u = 0; u < 3; ++u) {
                        const pgt_dstat_jack &r = jack[3 * t + (size_t)u];
                        auto g6 = [](double v) { char b_[64]; if (v != v) return std::string("nan"); std::snprintf(b_, sizeof b_, "%g", v); return std::string(b_); };
                        std::fprintf(f, "%d\t%d\t%d\t%s\t%s\t%s\t%s\t%u\t%llu\n", topo[u][0] + 1, topo[u][1] + 1, topo[u][2] + 1, g6(r.d).c_str(),
                                     g6(r.d_jack).c_str(), g6(r.se).c_str(), g6(r.z).c_str(), r.n_blocks, (unsigned long long)r.n_sites);
                    }
                }
        close_out(f, path);
    }
    if (fd) {  // the .fd files and PREFIX.fd.global: the loops of the .dstat files and PREFIX.global above
        const std::string fd_global_path = std::string(prefix) + ".fd.global";
        FILE *fd_global = open_out(fd_global_path);
        t = 0;
        for (int a = 0; a < K - 1; ++a)
            for (int b = a + 1; b < K - 1; ++b)
                for (int c = b + 1; c < K - 1; ++c, ++t) {
                    if (W > 0) {
                        const std::string path = std::string(prefix) + ".pop" + std::to_string(a + 1) + "_pop" + std::to_string(b + 1) + "_pop" + std::to_string(c + 1) + ".fd";
                        FILE *f = open_out(path);
                        const pgt_fd_row *r = fd_rows.data() + t * n_win;
                        write_rows(n_win, longest_name(runs) + 200, [&](size_t i, char *o) -> size_t {
                            if (!(r[i].n > 0 || !skip_missing)) return 0;
                            return put_fd_row(o, runs.name[win[i].label_run], r[i], (uint32_t)(win[i].hi - win[i].lo) - r[i].n);
                        }, f);
                        close_out(f, path);
                    }
                    const pgt_fd_total &g = fd_tot[t];  // the ratios from the totals by the row's rule
                    std::fprintf(fd_global, "%d\t%d\t%d\t%g\t%g\t%g\t%g\t%g\t%llu\t%llu\n", a + 1, b + 1, c + 1, g.fd_den != 0.0 ? g.num / g.fd_den : 0.0,
                                 g.fdm_den != 0.0 ? g.num / g.fdm_den : 0.0, g.num, g.fd_den, g.fdm_den, (unsigned long long)g.neff, (unsigned long long)g.nskip);
                }
        close_out(fd_global, fd_global_path);
    }
    finish(timer);
}
