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

// chr start end mid f3_i f3_j f3_k neff nskip
static size_t put_f3_row(char *o, const std::string &chr, const pgt_f3_row &r, uint32_t nskip) {
    char *p = o;
    std::memcpy(p, chr.data(), chr.size());
    p += chr.size();
    for (uint32_t u : {r.start, r.end, r.mid}) { *p++ = '\t'; p = put_u32(p, u); }
    for (double g : {mean_of(r.f3_i, r.n), mean_of(r.f3_j, r.n), mean_of(r.f3_k, r.n)}) { *p++ = '\t'; p += fmt_g6(g, p); }
    for (uint32_t u : {r.n, nskip}) { *p++ = '\t'; p = put_u32(p, u); }
    *p++ = '\n';
    return (size_t)(p - o);
}

int main(int argc, char **argv) {
    const std::string tool = "f3WindowPops";
    int jackknife = 0;
    const PopsArgs args = parse_pops_args(tool, argc, argv, help, 3, [&](const char *o, const char *v) {
        if (std::strcmp(o, "-jackknife")) return false;
        if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(std::string("-jackknife must be 0 or 1 (given: ") + v + ")");
        jackknife = v[0] == '1';
        if (!jackknife) return true;
        // refused here, while the options are read and before any file is opened, as dstatWindowPops does: the blocks are the
        // run's windows, which must exist and be disjoint (the last value of an option counts)
        DxyOptions w;
        for (int i = 1; i + 1 < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2)
            if (!std::strcmp(argv[i], "-winsize") || !std::strcmp(argv[i], "-stepsize")) dxy_option(w, argv[i], argv[i + 1]);
        if (w.W == 0) die("-jackknife 1 needs windows as its blocks: -winsize must be > 0");
        if (w.S < w.W)
            die("-jackknife 1 needs windows that do not overlap: -stepsize (" + std::to_string(w.S) + ") must not be below -winsize (" + std::to_string(w.W) + ")");
        return true;
    }, 6);
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
    const size_t n_trios = (size_t)K * (size_t)(K - 1) * (size_t)(K - 2) / 6, n_win = win.size();
    pgt_f3_row *d_rows = pops_dev_alloc<pgt_f3_row>(ctx, n_trios * n_win);
    pgt_f3_total *d_tot = pops_dev_alloc<pgt_f3_total>(ctx, n_trios);
    const size_t tree_bytes = pgt_f3_pops_tree_bytes((uint32_t)K, s.n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    check(pgt_f3_pops_reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
                                 n_win ? d_rows : nullptr, n_trios * n_win * sizeof(pgt_f3_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_f3_row> rows(n_trios * n_win);
    std::vector<pgt_f3_total> tot(n_trios);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_trios * n_win * sizeof(pgt_f3_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_trios * sizeof(pgt_f3_total), nullptr), ctx);
    std::vector<pgt_f3_jack> jack;
    if (jackknife) {  // the rows are still on the device: every window of the table is a block
        const size_t work_bytes = pgt_f3_jackknife_work_bytes((uint32_t)n_trios, n_win);
        void *work = nullptr;
        check(pgt_dev_alloc(ctx, work_bytes, &work), ctx);
        pgt_f3_jack *d_jack = pops_dev_alloc<pgt_f3_jack>(ctx, 3 * n_trios);
        check(pgt_f3_jackknife_dev(ctx, d_rows, n_win, (uint32_t)n_trios, d_jack, 3 * n_trios * sizeof(pgt_f3_jack), work, work_bytes, nullptr), ctx);
        jack.resize(3 * n_trios);
        check(pgt_rowbuf_read(ctx, jack.data(), d_jack, 3 * n_trios * sizeof(pgt_f3_jack), nullptr), ctx);
    }
    timer.lap("gpu reduce");

    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    size_t t = 0;
    for (int a = 0; a < K; ++a)
        for (int b = a + 1; b < K; ++b)
            for (int c = b + 1; c < K; ++c, ++t) {
                if (W > 0) {
                    const std::string path = std::string(prefix) + ".pop" + std::to_string(a + 1) + "_pop" + std::to_string(b + 1) + "_pop" + std::to_string(c + 1) + ".f3";
                    FILE *f = open_out(path);
                    const pgt_f3_row *r = rows.data() + t * n_win;
                    write_rows(n_win, longest_name(runs) + 200, [&](size_t i, char *o) -> size_t {  // -skip_missing as dxyWindow.cpp:189
                        if (!(r[i].n > 0 || !skip_missing)) return 0;
                        return put_f3_row(o, runs.name[win[i].label_run], r[i], (uint32_t)(win[i].hi - win[i].lo) - r[i].n);
                    }, f);
                    close_out(f, path);
                }
                const pgt_f3_total &g = tot[t];  // the means from the totals by the row's rule
                std::fprintf(global, "%d\t%d\t%d\t%g\t%g\t%g\t%llu\t%llu\n", a + 1, b + 1, c + 1, mean_of(g.f3_i, g.neff), mean_of(g.f3_j, g.neff),
                             mean_of(g.f3_k, g.neff), (unsigned long long)g.neff, (unsigned long long)g.nskip);
            }
    close_out(global, global_path);
    if (jackknife) {  // target src1 src2 f3 f3_jack SE Z nblocks nsites: trio order, then (i; j,k), (j; i,k), (k; i,j)
        const std::string path = std::string(prefix) + ".jackknife";
        FILE *f = open_out(path);
        t = 0;
        for (int a = 0; a < K; ++a)
            for (int b = a + 1; b < K; ++b)
                for (int c = b + 1; c < K; ++c, ++t) {
                    const int target[3][3] = {{a, b, c}, {b, a, c}, {c, a, b}};
                    for (int u = 0; u < 3; ++u) {
                        const pgt_f3_jack &r = jack[3 * t + (size_t)u];
                        auto g6 = [](double v) { char b_[64]; if (v != v) return std::string("nan"); std::snprintf(b_, sizeof b_, "%g", v); return std::string(b_); };
                        std::fprintf(f, "%d\t%d\t%d\t%s\t%s\t%s\t%s\t%u\t%llu\n", target[u][0] + 1, target[u][1] + 1, target[u][2] + 1, g6(r.f3).c_str(),
                                     g6(r.f3_jack).c_str(), g6(r.se).c_str(), g6(r.z).c_str(), r.n_blocks, (unsigned long long)r.n_sites);
                    }
                }
        close_out(f, path);
    }
    finish(timer);
}
