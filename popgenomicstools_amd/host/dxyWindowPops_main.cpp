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
#include "dxy_common.h"

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

// one parsed file: columns on the device (pos / freq / nind), chromosome runs on the host
struct Maf : MafTable {
    DeviceTable dev;  // set when the file was parsed on the GPU: pos / freq / nind are tokens 1 / 5 / 6 there
    const uint32_t *d_pos = nullptr;  // (the host parser's columns are uploaded, then unused)
    const double *d_freq = nullptr;
    const int32_t *d_nind = nullptr;
};

template <class T>
static T *dev_alloc(pgt_ctx *ctx, size_t elems) {
    void *p = nullptr;
    check(pgt_dev_alloc(ctx, elems * sizeof(T) + 16, &p), ctx);
    return static_cast<T *>(p);
}

int main(int argc, char **argv) {
    DxyOptions opt;
    const char *prefix = nullptr;
    if (argc < 2) {
        help(opt.W, opt.S, opt.minind, opt.fixedsite, opt.skip_missing);
        return 0;
    }
    // option/value pairs first; what follows the last pair are the MAF files
    int i = 1;
    for (; i < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2) {
        const char *o = argv[i];
        if (i + 1 >= argc) die(std::string("Missing value for ") + o);
        if (!std::strcmp(o, "-out")) prefix = argv[i + 1];
        else if (!dxy_option(opt, o, argv[i + 1])) unknown_dxy_option(o);
    }
    const int K = argc - i;
    char **paths = argv + i;
    if (K < 2 || K > 8) die("dxyWindowPops: between 2 and 8 MAF files are needed (" + std::to_string(std::max(K, 0)) + " given)");
    if (!prefix || !*prefix) die("Must supply -out PREFIX");
    check_dxy_options(opt);
    const uint32_t W = opt.W, S = opt.S;
    const int minind = opt.minind, fixedsite = opt.fixedsite, skip_missing = opt.skip_missing;
    std::map<std::string, uint32_t> chrsize;
    if (!fixedsite) chrsize = read_sizefile(opt.sizefile);

    PhaseTimer timer;
    DeviceOpener device(std::vector<int>{devices_from_env()[0]});  // one GPU; HIP start-up runs beside the opening of the files
    // the texts are never unmapped or freed (as in the dxyWindow host: the process ends by _exit)
    std::vector<Text *> text((size_t)K);
    std::vector<char> opened((size_t)K, 0);
    {
        std::vector<std::thread> th;
        for (int k = 0; k < K; ++k) {
            text[(size_t)k] = new Text;
            th.emplace_back([&, k] { opened[(size_t)k] = text[(size_t)k]->open(paths[k]) ? 1 : 0; });
        }
        for (auto &t : th) t.join();
    }
    for (int k = 0; k < K; ++k)
        if (!opened[(size_t)k]) die("Unable to open Pop" + std::to_string(k + 1) + " MAF file: " + paths[k]);
    timer.lap("open");

    // no passes mode: what does not fit is refused, never truncated.  On the card per site and file: the parsed columns
    // (16 B), their aligned copies (16 B), an index column and the alignment workspace (8 B).
    const char *resident_env = std::getenv("PGT_MAX_RESIDENT_SITES");
    size_t smallest = SIZE_MAX, largest_k = 0;
    for (int k = 0; k < K; ++k) {
        smallest = std::min(smallest, text[(size_t)k]->size());
        if (text[(size_t)k]->size() > text[largest_k]->size()) largest_k = (size_t)k;
    }
    if (!resident_env && resident_limit(text[largest_k]->begin(), text[largest_k]->end(), (size_t)K * 40, [&] { return device.get(); }, K))
        die("dxyWindowPops: the MAF files and their aligned columns do not fit the GPU; this tool has no passes mode");

    std::vector<Maf> maf((size_t)K);
    pgt_ctx *ctx = nullptr;
    const bool on_gpu = gpu_ingest_wanted(smallest);
    if (on_gpu) {
        ctx = device.get();
        timer.lap("wait for HIP");
    }
    for (int k = 0; k < K; ++k) {
        Maf &m = maf[(size_t)k];
        const Text &t = *text[(size_t)k];
        Cursor hdr{t.begin(), t.end()};
        hdr.next_line();  // header (dxyWindow.cpp:284)
        bool parsed = false;
        if (on_gpu) {
            parsed = ingest_on_device(ctx, hdr.p, t.end(), kMafSpec, 7, kMafWhat, paths[k], 2, m.dev, m.runs);
            if (parsed) {
                m.n = m.dev.n;
                m.d_pos = m.dev.col<uint32_t>(1); m.d_freq = m.dev.col<double>(5); m.d_nind = m.dev.col<int32_t>(6);
            } else {  // too many irregular lines for the device parser
                if (m.dev.ing) pgt_ingest_free(m.dev.ing);
                m.dev.ing = nullptr;
                m.runs = Runs{};
            }
        }
        if (!parsed) m.n = parse_table(hdr.p, t.end(), m, m.runs, kMafWhat, paths[k], 2);
        if (m.n == 0) die("dxyWindowPops: a MAF file holds no sites");
        if (resident_env && std::atoll(resident_env) > 0 && m.n > (size_t)std::atoll(resident_env))
            die("dxyWindowPops: " + std::string(paths[k]) + " holds " + std::to_string(m.n) + " sites, more than PGT_MAX_RESIDENT_SITES=" +
                resident_env + "; this tool has no passes mode");
        if (m.n >= 0xFFFFFFFFull) die("dxyWindowPops: at most 2^32-2 sites per MAF file");
    }
    timer.lap(on_gpu ? "gpu parse" : "parse");
    for (int k = 1; k < K; ++k)
        if (maf[(size_t)k].runs.name[0] != maf[0].runs.name[0]) die("Chromosomes in MAF files differ");  // dxyWindow.cpp:295-298

    // chromosome names -> ids (equal names, equal ids), then the segments of the chromosomes every file has
    std::map<std::string, uint32_t> id_of;
    std::vector<std::string> name_of;
    std::vector<std::vector<uint32_t>> run_chr((size_t)K);
    std::vector<const uint32_t *> p_chr((size_t)K);
    std::vector<const uint64_t *> p_len((size_t)K);
    std::vector<size_t> n_runs((size_t)K);
    for (int k = 0; k < K; ++k) {
        const Runs &r = maf[(size_t)k].runs;
        for (const std::string &nm : r.name) {
            auto it = id_of.insert({nm, (uint32_t)name_of.size()});
            if (it.second) name_of.push_back(nm);
            run_chr[(size_t)k].push_back(it.first->second);
        }
        p_chr[(size_t)k] = run_chr[(size_t)k].data();
        p_len[(size_t)k] = r.len.data();
        n_runs[(size_t)k] = r.len.size();
    }
    size_t n_seg = 0;
    int rc = pgt_align_segments(p_chr.data(), p_len.data(), n_runs.data(), (uint32_t)K, nullptr, 0, &n_seg);
    std::vector<pgt_seg> seg(n_seg);
    if (rc == PGT_OK && n_seg) rc = pgt_align_segments(p_chr.data(), p_len.data(), n_runs.data(), (uint32_t)K, seg.data(), seg.size(), &n_seg);
    if (rc == PGT_EDOMAIN) {  // the library names the id; the user knows the name
        const std::string msg = pgt_last_error(nullptr);
        const char *tag = "chromosome id ";
        const size_t at = msg.find(tag);
        const size_t id = at == std::string::npos ? name_of.size() : (size_t)std::strtoull(msg.c_str() + at + std::strlen(tag), nullptr, 10);
        if (id >= name_of.size()) die("dxyWindowPops: " + msg);
        die("dxyWindowPops: chromosome " + name_of[id] + (msg.find("two runs") != std::string::npos
                ? " appears in two separate blocks of a MAF file"
                : " is not in the same order in all MAF files") + " (all MAF files need the same chromosomes in the same order)");
    }
    check(rc, nullptr);
    const size_t n_chr = n_seg / (size_t)K;
    uint64_t cap = 0;  // no chromosome has more common sites than its shortest list
    for (size_t m = 0; m < n_chr; ++m) {
        uint64_t least = UINT64_MAX;
        for (int k = 0; k < K; ++k) least = std::min(least, seg[m * (size_t)K + (size_t)k].len);
        cap += least;
    }
    if (cap == 0) die("dxyWindowPops: the MAF files share no site");
    timer.lap("segments");

    if (!ctx) {
        ctx = device.get();
        timer.lap("wait for HIP");
    }
    for (int k = 0; k < K; ++k) {  // the host parser's columns go to the device as they are
        Maf &m = maf[(size_t)k];
        if (m.d_pos) continue;
        uint32_t *dp = dev_alloc<uint32_t>(ctx, m.n);
        double *df = dev_alloc<double>(ctx, m.n);
        int32_t *dn = dev_alloc<int32_t>(ctx, m.n);
        check(pgt_dev_upload(ctx, dp, m.pos.data(), m.n * sizeof(uint32_t)), ctx);
        check(pgt_dev_upload(ctx, df, m.freq.data(), m.n * sizeof(double)), ctx);
        check(pgt_dev_upload(ctx, dn, m.nind.data(), m.n * sizeof(int32_t)), ctx);
        m.d_pos = dp; m.d_freq = df; m.d_nind = dn;
    }
    if (!on_gpu) timer.lap("upload");

    // the common sites: one index column per file, then every column gathered onto them
    std::vector<const uint32_t *> d_pos((size_t)K);
    std::vector<uint64_t> rows_of((size_t)K);
    std::vector<uint32_t *> d_idx((size_t)K);
    for (int k = 0; k < K; ++k) {
        d_pos[(size_t)k] = maf[(size_t)k].d_pos;
        rows_of[(size_t)k] = maf[(size_t)k].n;
        d_idx[(size_t)k] = dev_alloc<uint32_t>(ctx, cap);
    }
    const size_t work_bytes = pgt_align_workspace_bytes((uint32_t)K, rows_of[0]);
    void *work = nullptr;
    check(pgt_dev_alloc(ctx, work_bytes, &work), ctx);
    std::vector<uint64_t> seg_count(n_chr, 0);
    uint64_t n_sites = 0;
    check(pgt_sites_align(ctx, d_pos.data(), rows_of.data(), (uint32_t)K, seg.data(), n_seg, d_idx.data(), cap, seg_count.data(), &n_sites,
                          work, work_bytes, nullptr), ctx);
    check(pgt_dev_free(ctx, work), ctx);
    if (n_sites == 0) die("dxyWindowPops: the MAF files share no site");
    uint32_t *a_pos = dev_alloc<uint32_t>(ctx, n_sites);
    std::vector<const double *> a_freq((size_t)K);
    std::vector<const int32_t *> a_nind((size_t)K);
    check(pgt_gather_dev(ctx, a_pos, d_pos[0], d_idx[0], n_sites, 4, nullptr), ctx);
    for (int k = 0; k < K; ++k) {
        double *f = dev_alloc<double>(ctx, n_sites);
        int32_t *c = dev_alloc<int32_t>(ctx, n_sites);
        check(pgt_gather_dev(ctx, f, maf[(size_t)k].d_freq, d_idx[(size_t)k], n_sites, 8, nullptr), ctx);
        check(pgt_gather_dev(ctx, c, maf[(size_t)k].d_nind, d_idx[(size_t)k], n_sites, 4, nullptr), ctx);
        a_freq[(size_t)k] = f;
        a_nind[(size_t)k] = c;
    }
    Runs runs;  // chromosomes left with no common site are dropped (as the dxyWindow host does)
    for (size_t m = 0; m < n_chr; ++m) {
        if (!seg_count[m]) continue;
        // the matched chromosome's name: file 0's run that starts at its segment
        const Runs &r0 = maf[0].runs;
        uint64_t off = 0;
        size_t r = 0;
        while (off != seg[m * (size_t)K].off || r0.len[r] != seg[m * (size_t)K].len) off += r0.len[r++];
        runs.name.push_back(r0.name[r]);
        runs.len.push_back(seg_count[m]);
    }
    timer.lap("align");

    std::vector<pgt_win> win;
    if (W > 0) {
        if (fixedsite) {
            win = site_windows(runs, W, S);
        } else {
            const std::vector<uint32_t> chr_len = chr_lengths(runs, chrsize);
            Column<uint32_t> pos;  // the bp table is built from the aligned positions: 4 B per site, one download
            pos.alloc(n_sites);
            check(pgt_rowbuf_read(ctx, pos.data(), a_pos, n_sites * sizeof(uint32_t), nullptr), ctx);
            win = bp_windows(pos.data(), runs, chr_len, W, S);
        }
    }
    timer.lap("window table");

    const size_t n_pairs = (size_t)K * (size_t)(K - 1) / 2, n_win = win.size();
    for (int k = 0; k < K; ++k) check(pgt_dev_free(ctx, d_idx[(size_t)k]), ctx);
    pgt_win *d_win = dev_alloc<pgt_win>(ctx, n_win);
    check(pgt_dev_upload(ctx, d_win, win.data(), n_win * sizeof(pgt_win)), ctx);
    pgt_dxy_row *d_rows = dev_alloc<pgt_dxy_row>(ctx, n_pairs * n_win);
    pgt_dxy_total *d_tot = dev_alloc<pgt_dxy_total>(ctx, n_pairs);
    const size_t tree_bytes = pgt_dxy_pops_tree_bytes((uint32_t)K, n_sites);
    void *tree = nullptr;
    check(pgt_dev_alloc(ctx, tree_bytes, &tree), ctx);
    check(pgt_dxy_pops_reduce_dev(ctx, a_pos, a_freq.data(), a_nind.data(), (uint32_t)K, n_sites, minind, n_win ? d_win : nullptr, n_win,
                                  n_win ? d_rows : nullptr, n_pairs * n_win * sizeof(pgt_dxy_row), d_tot, tree, tree_bytes, nullptr), ctx);
    RowArray<pgt_dxy_row> rows(n_pairs * n_win);
    std::vector<pgt_dxy_total> tot(n_pairs);
    check(pgt_rowbuf_read(ctx, rows.data(), d_rows, n_pairs * n_win * sizeof(pgt_dxy_row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot.data(), d_tot, n_pairs * sizeof(pgt_dxy_total), nullptr), ctx);
    timer.lap("gpu reduce");

    auto open_out = [](const std::string &path) {
        FILE *f = std::fopen(path.c_str(), "w");
        if (!f) die("Unable to open output file: " + path);
        return f;
    };
    auto close_out = [](FILE *f, const std::string &path) {
        if (std::fflush(f) != 0 || std::ferror(f) || std::fclose(f) != 0) die("Error writing the output: " + path);
    };
    const std::string global_path = std::string(prefix) + ".global";
    FILE *global = open_out(global_path);
    size_t p = 0;
    for (int a = 0; a < K; ++a)
        for (int b = a + 1; b < K; ++b, ++p) {
            if (W > 0) {
                const std::string path = std::string(prefix) + ".pop" + std::to_string(a + 1) + "_pop" + std::to_string(b + 1) + ".dxy";
                FILE *f = open_out(path);
                write_dxy_rows(rows.data() + p * n_win, n_win, runs, [&](size_t w) { return win[w].label_run; }, skip_missing, f);
                close_out(f, path);
            }
            std::fprintf(global, "%d\t%d\t%g\t%llu\t%llu\n", a + 1, b + 1, tot[p].sum, (unsigned long long)tot[p].neff, (unsigned long long)tot[p].nskip);
        }
    close_out(global, global_path);
    finish(timer);
}
