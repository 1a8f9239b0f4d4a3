// dxy_common.h — what the dxyWindow and dxyWindowPops hosts share: the MAF row parser, the options and their refusals
// (dxyWindow.cpp:63-139), the size file (:155-170), the window tables, the row writer (:189-191) with the genome-wide
// line (:429-433), and dxyWindow's site synchronisation (:315-331) as plain functions over parsed columns.
// Everything is inline or a template and nothing here takes a pgt_ctx, so a program that calls none of the window
// builders (tests/host_parse_check.cpp) needs no libpgtwin.
#pragma once

#include <map>

#include "host_common.h"

namespace pgthost {

// ---- one parsed MAF file ------------------------------------------------------------------------------------------------
// chr pos major minor ref freq nind — only chr, pos, freq, nind are used (dxyWindow.cpp:141-153).  On the device parser
// pos / freq / nind are tokens 1 / 5 / 6.
struct MafTable {
    Runs runs;
    Column<uint32_t> pos;
    Column<double> freq;
    Column<int32_t> nind;
    size_t n = 0;
    void alloc(size_t rows) { pos.alloc(rows); freq.alloc(rows); nind.alloc(rows); }
    bool parse_line(Cursor &c, size_t i, Runs &r) {
        const Tok chr = c.token();
        long long k;
        bool ok = to_u32(c.token(), pos[i]);
        c.token(); c.token(); c.token();  // major minor ref
        ok = ok && to_f64(c.token(), freq[i]) && to_i64(c.token(), k);
        // a frequency outside [0,1] would make dxy negative, which the reference neither counts nor
        // skips (dxyWindow.cpp:180-185): refuse it
        if (!ok || !(freq[i] >= 0.0 && freq[i] <= 1.0)) return false;
        nind[i] = (int32_t)std::max<long long>(std::min<long long>(k, INT32_MAX), INT32_MIN);
        r.add(chr.first, chr.second);
        return true;
    }
};

static const char *const kMafWhat = "dxyWindow: cannot parse MAF line (chr pos major minor ref freq nind, freq in [0,1])";
static const uint8_t kMafSpec[] = {PGT_TOK_CHR, PGT_TOK_U32, PGT_TOK_SKIP, PGT_TOK_SKIP, PGT_TOK_SKIP, PGT_TOK_FREQ, PGT_TOK_I32};

// ---- options (dxyWindow.cpp:97-126, defaults :529-534) ----------------------------------------------------------------------
struct DxyOptions {
    uint32_t W = 0, S = 0;
    int minind = 1, fixedsite = 0, skip_missing = 0;
    const char *sizefile = nullptr;
};
// one `opt val` pair; false: not an option the two tools share
inline bool dxy_option(DxyOptions &o, const char *opt, const char *val) {
    if (!std::strcmp(opt, "-winsize")) o.W = (uint32_t)std::atoi(val);
    else if (!std::strcmp(opt, "-stepsize")) o.S = (uint32_t)std::atoi(val);
    else if (!std::strcmp(opt, "-minind")) {
        o.minind = std::atoi(val);
        if (o.minind <= 0) die("-minind must be at least 1");
    } else if (!std::strcmp(opt, "-sizefile")) o.sizefile = val;
    else if (!std::strcmp(opt, "-fixedsite")) o.fixedsite = std::atoi(val);
    else if (!std::strcmp(opt, "-skip_missing")) o.skip_missing = std::atoi(val);
    else return false;
    return true;
}
[[noreturn]] inline void unknown_dxy_option(const char *opt) { die(std::string("Unknown command: ") + opt); }
inline void check_dxy_options(const DxyOptions &o) {
    if (o.W > 0 && o.S < 1) die("Must specify a -stepsize > 0 when -winsize is > 0");
    if (!o.fixedsite && !o.sizefile) die("Must supply size file unless -fixedsite 1");
    if (o.W > 0 && o.S > o.W) die("-stepsize must not exceed -winsize");                      // reference: crash (Q9)
    if (o.W == 0 && !o.fixedsite) die("-winsize 0 (global dxy) requires -fixedsite 1");      // reference: crash (Q10)
}

// -sizefile: chromosome name, size in base pairs; the first entry of a name is kept (dxyWindow.cpp:155-170)
inline std::map<std::string, uint32_t> read_sizefile(const char *path) {
    std::map<std::string, uint32_t> chrsize;
    Text text;
    if (!text.open(path)) die(std::string("Unable to open sizefile: ") + path);
    Cursor c{text.begin(), text.end()};
    while (c.p < c.end) {
        auto name = c.token();
        uint32_t len = 0;
        if (name.first == name.second || !to_u32(c.token(), len) || len == 0)
            die("Unable to correctly parse chromosome size file");
        chrsize.insert({std::string(name.first, name.second), len});
        c.next_line();
    }
    return chrsize;
}

// ---- window tables ------------------------------------------------------------------------------------------------------
// the size of every run's chromosome (dxyWindow.cpp:340-343)
inline std::vector<uint32_t> chr_lengths(const Runs &runs, const std::map<std::string, uint32_t> &chrsize) {
    std::vector<uint32_t> chr_len(runs.name.size());
    for (size_t r = 0; r < runs.name.size(); ++r) {
        auto it = chrsize.find(runs.name[r]);
        if (it == chrsize.end()) die("Unable to determine size for " + runs.name[r]);
        chr_len[r] = it->second;
    }
    return chr_len;
}
// Count, then fill.  With a NULL output the builders only count, so a table of no window needs no second call.
inline std::vector<pgt_win> bp_windows(const uint32_t *pos, const Runs &runs, const std::vector<uint32_t> &chr_len, uint32_t W, uint32_t S) {
    size_t n_win = 0;
    check(pgt_build_windows_bp(pos, runs.len.data(), chr_len.data(), runs.len.size(), W, S, nullptr, 0, &n_win), nullptr);
    std::vector<pgt_win> win(n_win);
    if (n_win) check(pgt_build_windows_bp(pos, runs.len.data(), chr_len.data(), runs.len.size(), W, S, win.data(), win.size(), &n_win), nullptr);
    return win;
}
inline std::vector<pgt_win> site_windows(const Runs &runs, uint32_t W, uint32_t S) {  // -fixedsite 1, table on the host
    size_t n_win = 0;
    check(pgt_build_windows_sites(runs.len.data(), runs.len.size(), W, S, nullptr, 0, &n_win), nullptr);
    std::vector<pgt_win> win(n_win);
    if (n_win) check(pgt_build_windows_sites(runs.len.data(), runs.len.size(), W, S, win.data(), win.size(), &n_win), nullptr);
    return win;
}

// ---- output -------------------------------------------------------------------------------------------------------------
// chr start end dxy neffective nskip, unless -skip_missing drops the row (dxyWindow.cpp:189-191); label(i): the run of row i
template <class Label>
void write_dxy_rows(const pgt_dxy_row *rows, size_t n, const Runs &runs, Label label, int skip_missing, FILE *out = stdout) {
    write_rows(n, longest_name(runs) + 80, [&](size_t i, char *o) -> size_t {
        if (!(rows[i].neff > 0 || !skip_missing)) return 0;
        return put_row(o, runs.name[label(i)], {rows[i].start, rows[i].end}, rows[i].sum, {rows[i].neff, rows[i].nskip});
    }, out);
}
// genome-wide line: stdout for the global run, stderr beside windows (dxyWindow.cpp:429-433)
inline void print_dxy_total(const pgt_dxy_total &tot, uint32_t W) {
    std::fprintf(W == 0 ? stdout : stderr, "%g\t%llu\t%llu\n", tot.sum, (unsigned long long)tot.neff, (unsigned long long)tot.nskip);
}

// ---- site synchronisation of two files (dxyWindow) ----------------------------------------------------------------------
// the synchronised sites: Pop1's position, both frequencies and counts, the chromosome runs
struct DxySites {
    Runs runs;
    std::vector<uint32_t> pos;
    std::vector<double> p1, p2;
    std::vector<int32_t> n1, n2;
    void add(const MafTable &m1, size_t i, const MafTable &m2, size_t j) {
        pos.push_back(m1.pos[i]);
        p1.push_back(m1.freq[i]); p2.push_back(m2.freq[j]);
        n1.push_back(m1.nind[i]); n2.push_back(m2.nind[j]);
    }
};

// The sites common to both files, by (chromosome run, position), in file 1's order.  A chromosome left with no common site
// has no run in the result.
inline void intersect_sites(const MafTable &m1, const MafTable &m2, DxySites &s) {
    size_t r1 = 0, r2 = 0, o1 = 0, o2 = 0;
    while (r1 < m1.runs.name.size() && r2 < m2.runs.name.size()) {
        const std::string &chr1 = m1.runs.name[r1], &chr2 = m2.runs.name[r2];
        if (chr1 != chr2) {  // skip the run that the other file does not have next
            bool later_in_1 = false;
            for (size_t k = r1 + 1; k < m1.runs.name.size() && !later_in_1; ++k) later_in_1 = m1.runs.name[k] == chr2;
            if (later_in_1) { o1 += m1.runs.len[r1]; ++r1; } else { o2 += m2.runs.len[r2]; ++r2; }
            continue;
        }
        size_t i = o1, j = o2;
        const size_t e1 = o1 + m1.runs.len[r1], e2 = o2 + m2.runs.len[r2];
        const size_t before = s.pos.size();
        while (i < e1 && j < e2) {
            if (m1.pos[i] < m2.pos[j]) ++i;
            else if (m2.pos[j] < m1.pos[i]) ++j;
            else s.add(m1, i++, m2, j++);
        }
        if (s.pos.size() > before) s.runs.add(chr1.data(), chr1.data() + chr1.size(), s.pos.size() - before);
        o1 = e1; o2 = e2; ++r1; ++r2;
    }
}

// ---- PGT_DXY_SYNC=reference: dxyWindow.cpp:315-331 replayed over the two parsed site lists ----------------------------
// The reference keeps one current line per file and, when chromosome or position differ, advances ONE of them:
//   Pop1 (`:317-323`) when the names agree and Pop1's position is smaller, or the names differ and Pop2's name is not the
//        chromosome of the last processed site — until the POSITIONS are equal (names are not looked at), or Pop1 ends;
//   Pop2 (`:324-330`) otherwise — while its position is SMALLER — and gives the whole run up unless the positions then agree.
// What it then processes is Pop1's line with Pop2's frequency and count beside it, under Pop1's chromosome name (`:332`).  A
// give-up ends the main loop exactly as the end of a file does (`:323,329` break to `:406`), so the reference's output is that
// of its window machine on the pairs processed so far: the list this function returns.  "getline fails" is "no further
// parsed line" here (both parsers stop at the first empty line as `while (!maf1line.empty())` does, `:313`).
// -> the pairs (index in file 1, index in file 2); `last_chr`: the chromosome the closing code (`:407-426`) works on —
// the last pair's, or the first line's when nothing was paired.
inline std::vector<std::pair<size_t, size_t>> pair_as_the_reference(const MafTable &m1, const MafTable &m2, std::string &last_chr) {
    auto run_of = [](const Runs &r) {  // site index -> run index, by a cursor that only moves forward
        return [&r, run = (size_t)0, end = (size_t)(r.len.empty() ? 0 : r.len[0])](size_t i) mutable {
            while (i >= end && run + 1 < r.len.size()) end += r.len[++run];
            return run;
        };
    };
    auto r1 = run_of(m1.runs), r2 = run_of(m2.runs);
    std::vector<std::pair<size_t, size_t>> pairs;
    size_t i = 0, j = 0;
    std::string chr = m1.runs.name[0];
    for (;;) {
        const std::string &c1 = m1.runs.name[r1(i)], &c2 = m2.runs.name[r2(j)];
        if (m1.pos[i] != m2.pos[j] || c1 != c2) {  // :316
            if ((c1 == c2 && m1.pos[i] < m2.pos[j]) || (c1 != c2 && c2 != chr)) {  // :317
                while (m1.pos[i] != m2.pos[j] && i + 1 < m1.n) ++i;  // :319-322
                if (m1.pos[i] != m2.pos[j]) break;                     // :323
            } else {
                while (m2.pos[j] < m1.pos[i] && j + 1 < m2.n) ++j;    // :326-329
                if (m1.pos[i] != m2.pos[j]) break;                     // :330
            }
        }
        chr = m1.runs.name[r1(i)];  // :332
        pairs.emplace_back(i, j);
        if (i + 1 >= m1.n) break;   // :399
        ++i;
        if (j + 1 >= m2.n) break;   // :402
        ++j;
    }
    last_chr = chr;
    return pairs;
}
// the pairs as columns: Pop1's line, Pop2's frequency and count beside it, under Pop1's chromosome name
inline void sites_of_pairs(const MafTable &m1, const MafTable &m2, const std::vector<std::pair<size_t, size_t>> &pairs, DxySites &s) {
    size_t run1 = 0, end1 = m1.runs.len[0];
    for (const auto &pr : pairs) {
        while (pr.first >= end1) end1 += m1.runs.len[++run1];
        const std::string &chr1 = m1.runs.name[run1];
        s.add(m1, pr.first, m2, pr.second);
        s.runs.add(chr1.data(), chr1.data() + chr1.size());
    }
}

// The reference's closing code on a chromosome of `len` base pairs of which NO site was processed (`:407-426` with nsites = 0,
// positer = 1): every slot is a placeholder, every window `chr start end 0 0 0` (case H10 of tests/golden/dxy_hand_walked.json).
inline void print_placeholder_chromosome(const std::string &chr, uint64_t len, uint64_t W, uint64_t S, int skip_missing) {
    if (skip_missing) return;  // neffective == 0: the row is dropped (`:189`)
    uint64_t first = 1, n = 0, p = 1;
    while (p <= len) {
        if (n == W) {  // `:413`: the buffer is full before the next slot goes in
            std::printf("%s\t%llu\t%llu\t0\t0\t0\n", chr.c_str(), (unsigned long long)first, (unsigned long long)(first + W - 1));
            first += S;
            n = W - S;
        }
        const uint64_t take = std::min<uint64_t>(W - n, len - p + 1);
        n += take;
        p += take;
    }
    if (n > W - S && n <= W)  // `:424`
        std::printf("%s\t%llu\t%llu\t0\t0\t0\n", chr.c_str(), (unsigned long long)first, (unsigned long long)(first + n - 1));
}

}  // namespace pgthost
