// hetWindow (MI355X host) — sliding-window individual heterozygosity = #het / #non-missing.
// Same command line and TSV as the reference tool (hetWindow.cpp:20-32 usage, :34-64 arguments,
// :87 row format: column 6 is the NON-MISSING count); reduction on the GPU via include/pgtwin.h.
//
//   hetWindow <genotypes file> [window size (sites)] [step size (sites)]
//   input lines:  chr  pos  g   (g: 0/1/2, negative = missing)
#include <algorithm>

#include "site_common.h"

using namespace pgthost;

namespace {  // internal linkage: parse_line is inlined into the parse loop, as when the table was local to main
struct HetWindow {
    static constexpr const char *name = "hetWindow";
    static constexpr const char *open_error = "Unable to open genotypes file ";
    static constexpr const char *what = "hetWindow: cannot parse 'chr pos genotype'";
    static constexpr uint8_t spec[] = {PGT_TOK_CHR, PGT_TOK_U32, PGT_TOK_I8};

    static void usage(unsigned W, unsigned S) {
        std::printf("\nUsage:\n"
                    "hetWindow [genotypes file] [window size (number sites)] [step size (number sites)]\n"
                    "default window size: %u\ndefault step size: %u\n\n"
                    "Output:\n(1) chromosome\n(2) window start\n(3) window end\n(4) window midpoint position\n"
                    "(5) heterozygosity\n(6) Number sites in window\n\n", W, S);
    }

    // chr pos genotype  (hetWindow.cpp:128,139)
    struct Table {
        Column<uint32_t> pos;
        Column<int8_t> g;
        auto columns() { return std::make_tuple(SiteColumn<uint32_t>{1, pos}, SiteColumn<int8_t>{2, g}); }
        void alloc(size_t rows) { alloc_columns(columns(), rows); }
        bool parse_line(Cursor &c, size_t i, Runs &runs) {
            const Tok chr = c.token();
            long long v;
            if (!to_u32(c.token(), pos[i]) || !to_i64(c.token(), v)) return false;
            // only `>= 0` and `== 1` are ever tested (hetWindow.cpp:78-80): clamping to int8 keeps both
            g[i] = (int8_t)std::clamp<long long>(v, -128, 127);
            runs.add(chr.first, chr.second);
            return true;
        }
    };

    using Row = pgt_het_row;
    // chr start end mid h nonmissing (hetWindow.cpp:87); inlined into both TSV loops (resident, passes), as the two lambdas it replaces were
    [[gnu::always_inline]] static size_t put(char *o, const std::string &chr, const Row &r) { return put_row(o, chr, {r.start, r.end, r.mid}, r.h, {r.nonmissing}); }
    static constexpr auto reduce = pgt_het_reduce;
    static constexpr auto reduce_cols = pgt_het_reduce_cols;
    static constexpr auto reduce_tab = pgt_het_reduce_tab;
};
}  // namespace

int main(int argc, char **argv) { return run_site_tool<HetWindow>(argc, argv); }
