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

int main(int argc, char **argv) {
    const std::string tool = "fstWindowPops";
    bool hudson = false;
    const PopsArgs args = parse_pops_args(tool, argc, argv, help, 2, [&](const char *o, const char *v) {
        if (std::strcmp(o, "-estimator")) return false;
        if (!std::strcmp(v, "hudson")) hudson = true;
        else if (!std::strcmp(v, "wc")) hudson = false;
        else die(std::string("-estimator must be wc or hudson (given: ") + v + ")");
        return true;
    });
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
    const size_t n_pairs = (size_t)K * (size_t)(K - 1) / 2, n_win = win.size();
    pgt_fst_row *d_rows = pops_dev_alloc<pgt_fst_row>(ctx, n_pairs * n_win);
    pgt_fst_total *d_tot = pops_dev_alloc<pgt_fst_total>(ctx, n_pairs);
    const size_t tree_bytes = pgt_fst_pops_tree_bytes((uint32_t)K, s.n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    check((hudson ? pgt_fst_hudson_pops_reduce_dev : pgt_fst_pops_reduce_dev)(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
            n_win ? d_rows : nullptr, n_pairs * n_win * sizeof(pgt_fst_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_fst_row> rows(n_pairs * n_win);
    std::vector<pgt_fst_total> tot(n_pairs);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_pairs * n_win * sizeof(pgt_fst_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_pairs * sizeof(pgt_fst_total), nullptr), ctx);
    timer.lap("gpu reduce");

    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    size_t p = 0;
    for (int a = 0; a < K; ++a)
        for (int b = a + 1; b < K; ++b, ++p) {
            if (W > 0) {
                const std::string path = pair_path(prefix, a, b, ".fst");
                FILE *f = open_out(path);
                const pgt_fst_row *r = rows.data() + p * n_win;
                // chr start end mid fst neff nskip: fstWindow's row (fstWindow.cpp:88) and the skipped count; -skip_missing as dxyWindow.cpp:189
                write_rows(n_win, longest_name(runs) + 100, [&](size_t i, char *o) -> size_t {
                    if (!(r[i].n > 0 || !skip_missing)) return 0;
                    const uint32_t nskip = (uint32_t)(win[i].hi - win[i].lo) - r[i].n;
                    return put_row(o, runs.name[win[i].label_run], {r[i].start, r[i].end, r[i].mid}, r[i].fst, {r[i].n, nskip});
                }, f);
                close_out(f, path);
            }
            const double fst = tot[p].bsum != 0.0 ? tot[p].asum / tot[p].bsum : 0.0;
            std::fprintf(global, "%d\t%d\t%g\t%llu\t%llu\n", a + 1, b + 1, fst, (unsigned long long)tot[p].neff, (unsigned long long)tot[p].nskip);
        }
    close_out(global, global_path);
    finish(timer);
}
