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

int main(int argc, char **argv) {
    const std::string tool = "piWindowPops";
    const PopsArgs args = parse_pops_args(tool, argc, argv, help, 1);
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
    const size_t n_pops = (size_t)K, n_win = win.size();
    pgt_dxy_row *d_rows = pops_dev_alloc<pgt_dxy_row>(ctx, n_pops * n_win);
    pgt_dxy_total *d_tot = pops_dev_alloc<pgt_dxy_total>(ctx, n_pops);
    const size_t tree_bytes = pgt_pi_pops_tree_bytes((uint32_t)K, s.n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    if (n_win) {  // the table is known here: the hints choose the query strategy (rows do not depend on them beyond the last bits)
        uint64_t max_window = 0, typical = 0, step = 0;
        check(pgt_table_hints(win.data(), n_win, &max_window, &typical, &step), ctx);
        check(pgt_set_max_window(ctx, max_window), ctx);
        check(pgt_set_typical_window(ctx, typical), ctx);
        check(pgt_set_window_step(ctx, step), ctx);
    }
    check(pgt_pi_pops_reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
                                 n_win ? d_rows : nullptr, n_pops * n_win * sizeof(pgt_dxy_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_dxy_row> rows(n_pops * n_win);
    std::vector<pgt_dxy_total> tot(n_pops);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_pops * n_win * sizeof(pgt_dxy_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_pops * sizeof(pgt_dxy_total), nullptr), ctx);
    timer.lap("gpu reduce");

    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    for (int a = 0; a < K; ++a) {
        if (W > 0) {
            const std::string path = std::string(prefix) + ".pop" + std::to_string(a + 1) + ".pi";
            FILE *f = open_out(path);
            write_dxy_rows(rows.data() + (size_t)a * n_win, n_win, runs, [&](size_t w) { return win[w].label_run; }, skip_missing, f);
            close_out(f, path);
        }
        std::fprintf(global, "%d\t%g\t%llu\t%llu\n", a + 1, tot[(size_t)a].sum, (unsigned long long)tot[(size_t)a].neff, (unsigned long long)tot[(size_t)a].nskip);
    }
    close_out(global, global_path);
    finish(timer);
}
