// pops_common.h — the K-file front end the all-pairs hosts (dxyWindowPops, fstWindowPops), piWindowPops and dstatWindowPops share: the command
// line (dxyWindow's options, -out PREFIX, 2 ... 8 MAF files; piWindowPops admits one, dstatWindowPops takes 4 ... 7), and from the opened files to the aligned columns and the window
// table on the device — open, parse on the host or the device, the resident-size refusals, chromosome ids,
// pgt_align_segments, upload, pgt_sites_align, pgt_gather_dev, the runs of the common sites, the window table.
// The K-file form of the reference's site synchronisation (dxyWindow.cpp:315-331): the sites (chromosome, position) that
// ALL files list are found on the GPU (a single file is its own site list: nothing to align).  Messages carry the tool's name.
#pragma once

#include <memory>

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
// option/value pairs first; what follows the last pair are the MAF files (min_files ... max_files of them).  help(opt) prints the tool's
// usage (no argument: exit 0).  own(option, value) -> true when the pair is an option of this tool alone, which it has taken
// (or refused by die()); a tool without one keeps answering `Unknown command:` for every option that is not dxyWindow's
struct NoOwnOption {
    bool operator()(const char *, const char *) const { return false; }
};
template <class Help, class Own = NoOwnOption>
inline PopsArgs parse_pops_args(const std::string &tool, int argc, char **argv, Help help, int min_files = 2, Own own = Own{}, int max_files = 8) {
    PopsArgs a;
    if (argc < 2) {
        help(a.opt);
        std::exit(0);
    }
    int i = 1;
    for (; i < argc && argv[i][0] == '-' && argv[i][1] != '\0'; i += 2) {
        const char *o = argv[i];
        if (i + 1 >= argc) die(std::string("Missing value for ") + o);
        if (!std::strcmp(o, "-out")) a.prefix = argv[i + 1];
        else if (own(o, argv[i + 1])) continue;
        else if (!dxy_option(a.opt, o, argv[i + 1])) unknown_dxy_option(o);
    }
    a.K = argc - i;
    a.paths = argv + i;
    if (a.K < min_files || a.K > max_files)
        die(tool + ": between " + std::to_string(min_files) + " and " + std::to_string(max_files) + " MAF files are needed (" + std::to_string(std::max(a.K, 0)) + " given)");
    if (!a.prefix || !*a.prefix) die("Must supply -out PREFIX");
    check_dxy_options(a.opt);
    if (!a.opt.fixedsite) a.chrsize = read_sizefile(a.opt.sizefile);
    return a;
}

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
inline std::string pair_path(const char *prefix, int a, int b, const char *ext) {
    return std::string(prefix) + ".pop" + std::to_string(a + 1) + "_pop" + std::to_string(b + 1) + ext;
}

}  // namespace pgthost
