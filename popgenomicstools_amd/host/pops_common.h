// pops_common.h — the K-population hosts (dxyWindowPops, fstWindowPops, piWindowPops, dstatWindowPops, f3WindowPops, f4WindowPops, f4ratioWindowPops, pbsWindowPops) are one
// program, run_pops_tool<Tool>: the command line (dxyWindow's options, the tool's own, -out PREFIX, the tool's number of MAF
// files), from the opened files to the aligned columns and the window table on the device (load_pops — open, parse on the host or
// the device, the resident-size refusals, chromosome ids, pgt_align_segments, upload, pgt_sites_align, pgt_gather_dev, the runs of
// the common sites, the window table), one reduction of all the tool's tables (pops_pass), and PREFIX.pop<i>[_pop<j>[_pop<k>[_pop<l>]]]<ext>
// per table with PREFIX.global.  The K-file form of the reference's site synchronisation (dxyWindow.cpp:315-331): the sites
// (chromosome, position) that ALL files list are found on the GPU (a single file is its own site list: nothing to align).
// Messages carry the tool's name.  A tool is a struct (derived from PopsTool, which holds what most tools leave alone) with
//     name, min_files, max_files, help(options)      the help text is the tool's own, verbatim
//     own(option, value, argc, argv)                  an option of this tool alone: taken (or refused by die()) -> true
//     arity, outgroup, first_apart                    its tables: all pairs (2), each population (1), all trios (3), all quartets (4) of the K files —
//                                                     of the K-1 before the last with an outgroup, of those behind the first with first_apart
//     Row, Total, ext, global_ext, row_bytes, tree_bytes, reduce_dev    the reduction and its files; tree_bytes(K, sites), or
//                                                     (K, sites, windows) where the workspace holds more than the tree
//     line(row, sites of the window), total(total)    the numbers of a row behind `chr`, of a PREFIX.global line behind the indices
//     window_hints                                    the window table's hints are set before the reduction (piWindowPops alone)
//     more(run, rows on the device)                   further device work on the same columns: pops_jackknife, a second pops_pass
//     host_rows                                       more() also gets the pass's rows and totals on the host (further files from them)
// and its main is `return run_pops_tool<Tool>(argc, argv);`.
#pragma once

#include <cstddef>
#include <functional>
#include <memory>
#include <type_traits>

#include "dxy_common.h"

namespace pgthost {

// one parsed file: columns on the device (pos / freq / nind), chromosome runs on the host
struct PopsMaf : MafTable {
    DeviceTable dev;  // set when the file was parsed on the GPU: pos / freq / nind are tokens 1 / 5 / 6 there
    const uint32_t *d_pos = nullptr;  // (the host parser's columns are uploaded, then unused)
    const double *d_freq = nullptr;
    const int32_t *d_nind = nullptr;
};

template <class T>
inline T *pops_dev_alloc(pgt_ctx *ctx, size_t elems) {
    void *p = nullptr;
    check(pgt_dev_alloc(ctx, elems * sizeof(T) + 16, &p), ctx);
    return static_cast<T *>(p);
}

// ---- the command line ---------------------------------------------------------------------------------------------------
struct PopsArgs {
    DxyOptions opt;
    const char *prefix = nullptr;
    int K = 0;
    char **paths = nullptr;
    std::map<std::string, uint32_t> chrsize;
};
// option/value pairs first; what follows the last pair are the MAF files (Tool::min_files ... Tool::max_files of them).
// Tool::help(opt) prints the tool's usage (no argument: exit 0).  tool.own(option, value, argc, argv) -> true when the pair is an
// option of this tool alone, which it has taken (or refused by die()); a tool without one keeps answering `Unknown command:` for
// every option that is not dxyWindow's.  The refusals come in this order, all before a file is opened or the device is touched.
template <class Tool>
inline PopsArgs parse_pops_args(Tool &tool, int argc, char **argv) {
    PopsArgs a;
    if (argc < 2) {
        Tool::help(a.opt);
        std::exit(0);
    }
    int i = 1;
    for (; i < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2) {
        const char *o = argv[i];
        if (i + 1 >= argc) die(std::string("Missing value for ") + o);
        if (!std::strcmp(o, "-out")) a.prefix = argv[i + 1];
        else if (tool.own(o, argv[i + 1], argc, argv)) continue;
        else if (!dxy_option(a.opt, o, argv[i + 1])) unknown_dxy_option(o);
    }
    a.K = argc - i;
    a.paths = argv + i;
    if (a.K < Tool::min_files || a.K > Tool::max_files)
        die(std::string(Tool::name) + ": between " + std::to_string(Tool::min_files) + " and " + std::to_string(Tool::max_files) + " MAF files are needed (" + std::to_string(std::max(a.K, 0)) + " given)");
    if (!a.prefix || !*a.prefix) die("Must supply -out PREFIX");
    check_dxy_options(a.opt);
    if (!a.opt.fixedsite) a.chrsize = read_sizefile(a.opt.sizefile);
    return a;
}

// -jackknife 0|1 of the trio tools.  With 1 the run is refused here, while the options are read and before any file is opened,
// unless its windows exist and are disjoint: they are the blocks (the option pairs are walked as parse_pops_args walks them, so
// the last value of -winsize / -stepsize counts wherever -jackknife stands).  `name`: the option's name where it is not
// -jackknife (pbsWindowPops: -blockjack); the messages name it.
struct JackknifeOption {
    bool on = false;
    bool take(const char *o, const char *v, int argc, char **argv, const char *name = "-jackknife") {
        const std::string opt = name;
        if (std::strcmp(o, name)) return false;
        if (std::strcmp(v, "0") && std::strcmp(v, "1")) die(opt + " must be 0 or 1 (given: " + v + ")");
        on = v[0] == '1';
        if (!on) return true;
        DxyOptions w;
        for (int i = 1; i + 1 < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2)
            if (!std::strcmp(argv[i], "-winsize") || !std::strcmp(argv[i], "-stepsize")) dxy_option(w, argv[i], argv[i + 1]);
        if (w.W == 0) die(opt + " 1 needs windows as its blocks: -winsize must be > 0");
        if (w.S < w.W)
            die(opt + " 1 needs windows that do not overlap: -stepsize (" + std::to_string(w.S) + ") must not be below -winsize (" + std::to_string(w.W) + ")");
        return true;
    }
};

// ---- from the files to the aligned columns ------------------------------------------------------------------------------
// everything the reduction needs, on the device: the shared position column, every file's frequency and count column
// gathered onto it, the window table; on the host the runs of the common sites and the table
struct PopsSites {
    pgt_ctx *ctx = nullptr;
    uint64_t n_sites = 0;
    const uint32_t *a_pos = nullptr;
    std::vector<const double *> a_freq;
    std::vector<const int32_t *> a_nind;
    Runs runs;
    std::vector<pgt_win> win;
    pgt_win *d_win = nullptr;
    std::shared_ptr<std::vector<PopsMaf>> single;  // ONE file: the parsed file, owner of the device columns above (else empty)
};

inline PopsSites load_pops(const std::string &tool, const PopsArgs &args, PhaseTimer &timer, DeviceOpener &device) {
    const int K = args.K;
    char **paths = args.paths;
    const uint32_t W = args.opt.W, S = args.opt.S;
    const int fixedsite = args.opt.fixedsite;
    const std::map<std::string, uint32_t> &chrsize = args.chrsize;
    using Maf = PopsMaf;
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
    // ONE file is not aligned: only its parsed columns (16 B per site) live on the card.
    const size_t site_bytes = K == 1 ? (size_t)16 : (size_t)K * 40;
    if (!resident_env && resident_limit(text[largest_k]->begin(), text[largest_k]->end(), site_bytes, [&] { return device.get(); }, K))
        die(tool + (K == 1 ? ": the MAF file does not fit the GPU; this tool has no passes mode"
                           : ": the MAF files and their aligned columns do not fit the GPU; this tool has no passes mode"));

    auto files = std::make_shared<std::vector<Maf>>((size_t)K);
    std::vector<Maf> &maf = *files;
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
        if (m.n == 0) die(tool + ": a MAF file holds no sites");
        if (resident_env && std::atoll(resident_env) > 0 && m.n > (size_t)std::atoll(resident_env))
            die(tool + ": " + std::string(paths[k]) + " holds " + std::to_string(m.n) + " sites, more than PGT_MAX_RESIDENT_SITES=" +
                resident_env + "; this tool has no passes mode");
        if (m.n >= 0xFFFFFFFFull) die(tool + ": at most 2^32-2 sites per MAF file");
    }
    timer.lap(on_gpu ? "gpu parse" : "parse");
    for (int k = 1; k < K; ++k)
        if (maf[(size_t)k].runs.name[0] != maf[0].runs.name[0]) die("Chromosomes in MAF files differ");  // dxyWindow.cpp:295-298

    // K >= 2: the sites all files share are found on the GPU (pgt_sites_align is defined for 2 ... 8 files); ONE file is its own
    // site list: its columns and runs are used as they are
    std::vector<pgt_seg> seg;
    size_t n_seg = 0, n_chr = 0;
    uint64_t cap = 0;  // no chromosome has more common sites than its shortest list
    if (K > 1) {
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
        int rc = pgt_align_segments(p_chr.data(), p_len.data(), n_runs.data(), (uint32_t)K, nullptr, 0, &n_seg);
        seg.resize(n_seg);
        if (rc == PGT_OK && n_seg) rc = pgt_align_segments(p_chr.data(), p_len.data(), n_runs.data(), (uint32_t)K, seg.data(), seg.size(), &n_seg);
        if (rc == PGT_EDOMAIN) {  // the library names the id; the user knows the name
            const std::string msg = pgt_last_error(nullptr);
            const char *tag = "chromosome id ";
            const size_t at = msg.find(tag);
            const size_t id = at == std::string::npos ? name_of.size() : (size_t)std::strtoull(msg.c_str() + at + std::strlen(tag), nullptr, 10);
            if (id >= name_of.size()) die(tool + ": " + msg);
            die(tool + ": chromosome " + name_of[id] + (msg.find("two runs") != std::string::npos
                    ? " appears in two separate blocks of a MAF file"
                    : " is not in the same order in all MAF files") + " (all MAF files need the same chromosomes in the same order)");
        }
        check(rc, nullptr);
        n_chr = n_seg / (size_t)K;
        for (size_t m = 0; m < n_chr; ++m) {
            uint64_t least = UINT64_MAX;
            for (int k = 0; k < K; ++k) least = std::min(least, seg[m * (size_t)K + (size_t)k].len);
            cap += least;
        }
        if (cap == 0) die(tool + ": the MAF files share no site");
        timer.lap("segments");
    }

    if (!ctx) {
        ctx = device.get();
        timer.lap("wait for HIP");
    }
    for (int k = 0; k < K; ++k) {  // the host parser's columns go to the device as they are
        Maf &m = maf[(size_t)k];
        if (m.d_pos) continue;
        uint32_t *dp = pops_dev_alloc<uint32_t>(ctx, m.n);
        double *df = pops_dev_alloc<double>(ctx, m.n);
        int32_t *dn = pops_dev_alloc<int32_t>(ctx, m.n);
        check(pgt_dev_upload(ctx, dp, m.pos.data(), m.n * sizeof(uint32_t)), ctx);
        check(pgt_dev_upload(ctx, df, m.freq.data(), m.n * sizeof(double)), ctx);
        check(pgt_dev_upload(ctx, dn, m.nind.data(), m.n * sizeof(int32_t)), ctx);
        m.d_pos = dp; m.d_freq = df; m.d_nind = dn;
    }
    if (!on_gpu) timer.lap("upload");

    uint64_t n_sites = 0;
    const uint32_t *a_pos = nullptr;
    std::vector<const double *> a_freq((size_t)K);
    std::vector<const int32_t *> a_nind((size_t)K);
    std::vector<uint32_t *> d_idx;
    Runs runs;
    if (K == 1) {
        n_sites = maf[0].n;
        a_pos = maf[0].d_pos;
        a_freq[0] = maf[0].d_freq;
        a_nind[0] = maf[0].d_nind;
        runs = maf[0].runs;
    } else {
        // the common sites: one index column per file, then every column gathered onto them
        std::vector<const uint32_t *> d_pos((size_t)K);
        std::vector<uint64_t> rows_of((size_t)K);
        d_idx.resize((size_t)K);
        for (int k = 0; k < K; ++k) {
            d_pos[(size_t)k] = maf[(size_t)k].d_pos;
            rows_of[(size_t)k] = maf[(size_t)k].n;
            d_idx[(size_t)k] = pops_dev_alloc<uint32_t>(ctx, cap);
        }
        const size_t work_bytes = pgt_align_workspace_bytes((uint32_t)K, rows_of[0]);
        void *work = nullptr;
        check(pgt_dev_alloc(ctx, work_bytes, &work), ctx);
        std::vector<uint64_t> seg_count(n_chr, 0);
        check(pgt_sites_align(ctx, d_pos.data(), rows_of.data(), (uint32_t)K, seg.data(), n_seg, d_idx.data(), cap, seg_count.data(), &n_sites,
                              work, work_bytes, nullptr), ctx);
        check(pgt_dev_free(ctx, work), ctx);
        if (n_sites == 0) die(tool + ": the MAF files share no site");
        uint32_t *g_pos = pops_dev_alloc<uint32_t>(ctx, n_sites);
        a_pos = g_pos;
        check(pgt_gather_dev(ctx, g_pos, d_pos[0], d_idx[0], n_sites, 4, nullptr), ctx);
        for (int k = 0; k < K; ++k) {
            double *f = pops_dev_alloc<double>(ctx, n_sites);
            int32_t *c = pops_dev_alloc<int32_t>(ctx, n_sites);
            check(pgt_gather_dev(ctx, f, maf[(size_t)k].d_freq, d_idx[(size_t)k], n_sites, 8, nullptr), ctx);
            check(pgt_gather_dev(ctx, c, maf[(size_t)k].d_nind, d_idx[(size_t)k], n_sites, 4, nullptr), ctx);
            a_freq[(size_t)k] = f;
            a_nind[(size_t)k] = c;
        }
        for (size_t m = 0; m < n_chr; ++m) {  // chromosomes left with no common site are dropped (as the dxyWindow host does)
            if (!seg_count[m]) continue;
            // the matched chromosome's name: file 0's run that starts at its segment
            const Runs &r0 = maf[0].runs;
            uint64_t off = 0;
            size_t r = 0;
            while (off != seg[m * (size_t)K].off || r0.len[r] != seg[m * (size_t)K].len) off += r0.len[r++];
            runs.name.push_back(r0.name[r]);
            runs.len.push_back(seg_count[m]);
        }
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

    const size_t n_win = win.size();
    for (uint32_t *idx : d_idx) check(pgt_dev_free(ctx, idx), ctx);
    pgt_win *d_win = pops_dev_alloc<pgt_win>(ctx, n_win);
    check(pgt_dev_upload(ctx, d_win, win.data(), n_win * sizeof(pgt_win)), ctx);
    PopsSites r;
    r.ctx = ctx;
    r.n_sites = n_sites;
    r.a_pos = a_pos;
    r.a_freq = std::move(a_freq);
    r.a_nind = std::move(a_nind);
    r.runs = std::move(runs);
    r.win = std::move(win);
    r.d_win = d_win;
    if (K == 1) r.single = std::move(files);  // a_pos / a_freq / a_nind are that file's own columns: it lives as long as they are used
    return r;
}

// ---- output files -------------------------------------------------------------------------------------------------------
inline FILE *open_out(const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) die("Unable to open output file: " + path);
    return f;
}
inline void close_out(FILE *f, const std::string &path) {
    if (std::fflush(f) != 0 || std::ferror(f) || std::fclose(f) != 0) die("Error writing the output: " + path);
}

// ---- the tables of a call -----------------------------------------------------------------------------------------------
// one table: the (0-based) populations of a pair, a population, a trio or a quartet
struct PopsIndex {
    int n;
    int pop[4];
};
// all i < j < .. of the populations first .. pops - 1, `arity` of them each, in the library's table order: (0,1),(0,2),..,(1,2),..
// (a loop beyond the arity runs once; what it leaves in `pop` is not looked at)
inline std::vector<PopsIndex> pops_tuples(int arity, int pops, int first = 0) {
    std::vector<PopsIndex> t;
    for (int a = first; a < pops; ++a)
        for (int b = arity > 1 ? a + 1 : pops - 1; b < pops; ++b)
            for (int c = arity > 2 ? b + 1 : pops - 1; c < pops; ++c)
                for (int d = arity > 3 ? c + 1 : pops - 1; d < pops; ++d) t.push_back({arity, {a, b, c, d}});
    return t;
}
// `pop1_pop2_pop3` of a file name ("pop", "_"), `1 2 3` at the head of a PREFIX.global line ("", "\t")
inline std::string tuple_text(const PopsIndex &ix, const char *before, const char *between) {
    std::string s;
    for (int k = 0; k < ix.n; ++k) s += std::string(k ? between : "") + before + std::to_string(ix.pop[k] + 1);
    return s;
}

// ---- one line of a table's file, or of PREFIX.global --------------------------------------------------------------------
// a row: `chr start end [mid]`, its doubles, `n nskip`; a genome-wide line: the table's indices, its doubles, `neff nskip`
struct PopsLine {
    uint32_t lead[3];
    double g[6];
    int n_lead = 0, n_g = 0;
    uint64_t n, nskip;
    PopsLine(std::initializer_list<uint32_t> lead_, std::initializer_list<double> g_, uint64_t n_, uint64_t nskip_) : n(n_), nskip(nskip_) {
        for (uint32_t u : lead_) lead[n_lead++] = u;
        for (double v : g_) g[n_g++] = v;
    }
};
// the row as put_row writes it, with any number of %g columns
inline size_t put_pops_line(char *o, const std::string &chr, const PopsLine &l) {
    char *p = o;
    std::memcpy(p, chr.data(), chr.size());
    p += chr.size();
    for (int k = 0; k < l.n_lead; ++k) { *p++ = '\t'; p = put_u32(p, l.lead[k]); }
    for (int k = 0; k < l.n_g; ++k) { *p++ = '\t'; p += fmt_g6(l.g[k], p); }
    for (uint32_t u : {(uint32_t)l.n, (uint32_t)l.nskip}) { *p++ = '\t'; p = put_u32(p, u); }
    *p++ = '\n';
    return (size_t)(p - o);
}

// ---- the run ------------------------------------------------------------------------------------------------------------
// What the passes of a run share.  A pass reduces and reads its results back at once, and queues what writes its files: every
// reduction of a run is done, under the "gpu reduce" lap, before the first output file is opened.
struct PopsRun {
    const PopsArgs &args;
    const PopsSites &s;
    std::vector<PopsIndex> tables;
    void *tree = nullptr;  // one buffer for the passes, one after the other: a later pass has the size of the first
    size_t tree_bytes = 0;
    std::vector<std::function<void()>> writers;
};
// the rows and totals of one pass on the host, for a tool whose more() writes further files from them (Tool::host_rows)
template <class Row, class Total>
struct PopsHostRows {
    std::shared_ptr<RowArray<Row>> rows;
    std::shared_ptr<std::vector<Total>> tot;
};

template <class Files, class Row, class Total>
void pops_queue_files(PopsRun &run, std::shared_ptr<RowArray<Row>> rows, std::shared_ptr<std::vector<Total>> tot);

// One reduction of the aligned columns over all tables of the run, and its files: PREFIX.<table><ext> per table (not with
// -winsize 0) and PREFIX<global_ext>.  -> the rows on the device, table after table; host, where given: the same rows and the totals
template <class Pass>
typename Pass::Row *pops_pass(const Pass &pass, PopsRun &run, PopsHostRows<typename Pass::Row, typename Pass::Total> *host = nullptr) {
    using Row = typename Pass::Row;
    using Total = typename Pass::Total;
    const PopsSites &s = run.s;
    pgt_ctx *ctx = s.ctx;
    const size_t n_tab = run.tables.size(), n_win = s.win.size();
    Row *d_rows = pops_dev_alloc<Row>(ctx, n_tab * n_win);
    Total *d_tot = pops_dev_alloc<Total>(ctx, n_tab);
    check(pass.reduce_dev(ctx, s.a_pos, s.a_freq.data(), s.a_nind.data(), (uint32_t)run.args.K, s.n_sites, run.args.opt.minind, n_win ? s.d_win : nullptr, n_win,
                          n_win ? d_rows : nullptr, n_tab * n_win * sizeof(Row), d_tot, run.tree, run.tree_bytes, nullptr), ctx);
    auto rows = std::make_shared<RowArray<Row>>(n_tab * n_win);
    auto tot = std::make_shared<std::vector<Total>>(n_tab);
    check(pgt_rowbuf_read(ctx, rows->data(), d_rows, n_tab * n_win * sizeof(Row), nullptr), ctx);
    check(pgt_rowbuf_read(ctx, tot->data(), d_tot, n_tab * sizeof(Total), nullptr), ctx);
    if (host) *host = {rows, tot};
    pops_queue_files<Pass>(run, rows, tot);
    return d_rows;
}

// The files of one set of rows and totals on the host, queued behind the run's reductions.  Files: ext, global_ext, row_bytes,
// line(row, sites of the window), total(total) — a pass itself, or further columns a tool derives from its rows (PBSn1)
template <class Files, class Row, class Total>
void pops_queue_files(PopsRun &run, std::shared_ptr<RowArray<Row>> rows, std::shared_ptr<std::vector<Total>> tot) {
    using Pass = Files;
    const size_t n_win = run.s.win.size();
    run.writers.push_back([&run, rows, tot, n_win] {
        const char *prefix = run.args.prefix;
        const int skip_missing = run.args.opt.skip_missing;
        const std::vector<pgt_win> &win = run.s.win;
        const Runs &runs = run.s.runs;
        const std::string global_path = std::string(prefix) + Pass::global_ext;
        FILE *global = open_out(global_path);
        for (size_t t = 0; t < run.tables.size(); ++t) {
            const PopsIndex &ix = run.tables[t];
            if (run.args.opt.W > 0) {
                const std::string path = std::string(prefix) + "." + tuple_text(ix, "pop", "_") + Pass::ext;
                FILE *f = open_out(path);
                const Row *r = rows->data() + t * n_win;
                write_rows(n_win, longest_name(runs) + Pass::row_bytes, [&](size_t i, char *o) -> size_t {  // -skip_missing as dxyWindow.cpp:189
                    const PopsLine l = Pass::line(r[i], (uint32_t)(win[i].hi - win[i].lo));
                    if (!(l.n > 0 || !skip_missing)) return 0;
                    return put_pops_line(o, runs.name[win[i].label_run], l);
                }, f);
                close_out(f, path);
            }
            const PopsLine g = Pass::total((*tot)[t]);
            std::fputs(tuple_text(ix, "", "\t").c_str(), global);
            for (int k = 0; k < g.n_g; ++k) std::fprintf(global, "\t%g", g.g[k]);
            std::fprintf(global, "\t%llu\t%llu\n", (unsigned long long)g.n, (unsigned long long)g.nskip);
        }
        close_out(global, global_path);
    });
}

// -jackknife 1: the delete-m_j block jackknife of every trio of the run on its rows still on the device, every window of the table
// a block -> PREFIX.jackknife, three lines per trio (`P1 P2 P3 estimate jackknife_estimate SE Z nblocks nsites`) or quartet
// (`P1 P2 P3 P4 ..`); U lines per table where the estimator has U items (the f4-ratio: six).  order[u]: which of the table's
// populations line u names first, second, third (and fourth).  label[u], where given, stands in front of line u (the name of
// its statistic).  The entry points' results are one layout.
struct PopsJack {
    double est, est_jack, se, z;
    uint64_t n_sites;
    uint32_t n_blocks, pad_;
};
template <class Row, class Jack, size_t U, size_t N>
void pops_jackknife(PopsRun &run, const Row *d_rows, int (*jackknife_dev)(pgt_ctx *, const Row *, uint64_t, uint32_t, Jack *, size_t, void *, size_t, void *),
                    size_t (*work_bytes)(uint32_t, uint64_t), const int (&order)[U][N], const char *const *label = nullptr) {
    static_assert(sizeof(Jack) == sizeof(PopsJack) && offsetof(Jack, se) == offsetof(PopsJack, se) && offsetof(Jack, z) == offsetof(PopsJack, z) &&
                  offsetof(Jack, n_sites) == offsetof(PopsJack, n_sites) && offsetof(Jack, n_blocks) == offsetof(PopsJack, n_blocks),
                  "the estimate and its jackknife estimate, then se, z, n_sites, n_blocks");
    pgt_ctx *ctx = run.s.ctx;
    const size_t n_trios = run.tables.size(), n_win = run.s.win.size();
    const size_t bytes = work_bytes((uint32_t)n_trios, n_win);
    void *work = nullptr;
    check(pgt_dev_alloc(ctx, bytes, &work), ctx);
    Jack *d_jack = pops_dev_alloc<Jack>(ctx, U * n_trios);
    check(jackknife_dev(ctx, d_rows, n_win, (uint32_t)n_trios, d_jack, U * n_trios * sizeof(Jack), work, bytes, nullptr), ctx);
    auto jack = std::make_shared<std::vector<PopsJack>>(U * n_trios);
    check(pgt_rowbuf_read(ctx, jack->data(), d_jack, U * n_trios * sizeof(Jack), nullptr), ctx);
    run.writers.push_back([&run, jack, &order, label] {  // (order, label: constants of the tool)
        const std::string path = std::string(run.args.prefix) + ".jackknife";
        FILE *f = open_out(path);
        auto g6 = [](double v) { char b_[64]; if (v != v) return std::string("nan"); std::snprintf(b_, sizeof b_, "%g", v); return std::string(b_); };
        for (size_t t = 0; t < run.tables.size(); ++t)
            for (size_t u = 0; u < U; ++u) {
                const int *pop = run.tables[t].pop;
                const PopsJack &r = (*jack)[U * t + u];
                if (label) std::fprintf(f, "%s\t", label[u]);
                for (size_t k = 0; k < N; ++k) std::fprintf(f, "%d\t", pop[order[u][k]] + 1);
                std::fprintf(f, "%s\t%s\t%s\t%s\t%u\t%llu\n", g6(r.est).c_str(), g6(r.est_jack).c_str(), g6(r.se).c_str(), g6(r.z).c_str(), r.n_blocks,
                             (unsigned long long)r.n_sites);
            }
        close_out(f, path);
    });
}

// ---- the tool -----------------------------------------------------------------------------------------------------------
// what most tools leave as it is
struct PopsTool {
    static constexpr int max_files = 8;
    static constexpr bool outgroup = false;      // the LAST file is the outgroup: it is in no table
    static constexpr bool first_apart = false;   // the FIRST file has a role of its own (the f4-ratio's A): it is in no table either
    static constexpr bool window_hints = false;  // the hints choose the query strategy, and rows may differ in their last bits between strategies
    static constexpr const char *global_ext = ".global";
    static constexpr bool host_rows = false;     // more(run, rows on the device, PopsHostRows) instead of more(run, rows on the device)
    bool own(const char *, const char *, int, char **) { return false; }
    template <class Row>
    void more(PopsRun &, const Row *) {}
};

template <class Tool>
int run_pops_tool(int argc, char **argv) {
    Tool tool;
    const PopsArgs args = parse_pops_args(tool, argc, argv);
    PhaseTimer timer;
    DeviceOpener device(std::vector<int>{devices_from_env()[0]});  // one GPU; HIP start-up runs beside the opening of the files
    const PopsSites s = load_pops(Tool::name, args, timer, device);
    pgt_ctx *ctx = s.ctx;
    PopsRun run{args, s, pops_tuples(Tool::arity, args.K - (Tool::outgroup ? 1 : 0), Tool::first_apart ? 1 : 0)};
    if constexpr (std::is_invocable_v<decltype(Tool::tree_bytes), uint32_t, uint64_t, uint64_t>)
        run.tree_bytes = Tool::tree_bytes((uint32_t)args.K, s.n_sites, s.win.size());  // the table is known here
    else
        run.tree_bytes = Tool::tree_bytes((uint32_t)args.K, s.n_sites);
    check(pgt_dev_alloc(ctx, run.tree_bytes, &run.tree), ctx);
    if (Tool::window_hints && !s.win.empty()) {  // the table is known here
        uint64_t max_window = 0, typical = 0, step = 0;
        check(pgt_table_hints(s.win.data(), s.win.size(), &max_window, &typical, &step), ctx);
        check(pgt_set_max_window(ctx, max_window), ctx);
        check(pgt_set_typical_window(ctx, typical), ctx);
        check(pgt_set_window_step(ctx, step), ctx);
    }
    if constexpr (Tool::host_rows) {
        PopsHostRows<typename Tool::Row, typename Tool::Total> host;
        const typename Tool::Row *d_rows = pops_pass(tool, run, &host);
        tool.more(run, d_rows, host);
    } else {
        tool.more(run, pops_pass(tool, run));
    }
    timer.lap("gpu reduce");
    for (const auto &write : run.writers) write();
    finish(timer);
}

}  // namespace pgthost
