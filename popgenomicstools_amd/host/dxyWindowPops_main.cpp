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

static void help(unsigned W, unsigned S, int minind, int fixedsite, int skip_missing) {
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
                "-out", "STRING", "-winsize", "INT", W, "-stepsize", "INT", S, "-minind", "INT", minind, "-fixedsite", "INT", fixedsite,
                "-sizefile", "FILE", "-skip_missing", "INT", skip_missing);
}

int main(int argc, char **argv) {
    const std::string tool = "dxyWindowPops";
    const PopsArgs args = parse_pops_args(tool, argc, argv, [](const DxyOptions &o) { help(o.W, o.S, o.minind, o.fixedsite, o.skip_missing); });
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
    pgt_dxy_row *d_rows = pops_dev_alloc<pgt_dxy_row>(ctx, n_pairs * n_win);
    pgt_dxy_total *d_tot = pops_dev_alloc<pgt_dxy_total>(ctx, n_pairs);
    const size_t tree_bytes = pgt_dxy_pops_tree_bytes((uint32_t)K, s.n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    check(pgt_dxy_pops_reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)K, s.n_sites, minind, n_win ? s.d_win : nullptr, n_win,
                                  n_win ? d_rows : nullptr, n_pairs * n_win * sizeof(pgt_dxy_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_dxy_row> rows(n_pairs * n_win);
    std::vector<pgt_dxy_total> tot(n_pairs);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_pairs * n_win * sizeof(pgt_dxy_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_pairs * sizeof(pgt_dxy_total), nullptr), ctx);
    timer.lap("gpu reduce");

    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    size_t p = 0;
    for (int a = 0; a < K; ++a)
        for (int b = a + 1; b < K; ++b, ++p) {
            if (W > 0) {
                const std::string path = pair_path(prefix, a, b, ".dxy");
                FILE *f = open_out(path);
                write_dxy_rows(rows.data() + p * n_win, n_win, runs, [&](size_t w) { return win[w].label_run; }, skip_missing, f);
                close_out(f, path);
            }
            std::fprintf(global, "%d\t%d\t%g\t%llu\t%llu\n", a + 1, b + 1, tot[p].sum, (unsigned long long)tot[p].neff, (unsigned long long)tot[p].nskip);
        }
    close_out(global, global_path);
    finish(timer);
}
