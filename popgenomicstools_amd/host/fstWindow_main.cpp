// fstWindow (MI355X host) — sliding-window FST = Σa/Σb from ANGSD variance components.
// Same command line and TSV as the reference tool (fstWindow.cpp:23-35 usage, :37-67 arguments,
// :88 row format); the per-window reduction runs on the GPU through include/pgtwin.h.
//
//   fstWindow <variance component file> [window size (sites)] [step size (sites)]
//   input lines:  chr  pos  a  b          output: chr start end mid fst nsites
#include "site_common.h"

using namespace pgthost;

namespace {  // internal linkage: parse_line is inlined into the parse loop, as when the table was local to main
struct FstWindow {
    static constexpr const char *name = "fstWindow";
    static constexpr const char *open_error = "Unable to open Fst variance components file ";
    static constexpr const char *what = "fstWindow: cannot parse 'chr pos a b'";
    static constexpr uint8_t spec[] = {PGT_TOK_CHR, PGT_TOK_U32, PGT_TOK_F64, PGT_TOK_F64};

    static void usage(unsigned W, unsigned S) {
        std::printf("\nUsage:\n"
                    "fstWindow [ANGSD fst variance component file] [window size (number sites)] [step size (number sites)]\n"
                    "default window size: %u\ndefault step size: %u\n\n"
                    "Output:\n(1) chromosome\n(2) window start\n(3) window end\n(4) window midpoint position\n"
                    "(5) Fst\n(6) Number sites in window\n\n", W, S);
    }

    // chr pos a b  (fstWindow.cpp:130,141)
    struct Table {
        Column<uint32_t> pos;
        Column<double> a, b;
        auto columns() { return std::make_tuple(SiteColumn<uint32_t>{1, pos}, SiteColumn<double>{2, a}, SiteColumn<double>{3, b}); }
        void alloc(size_t rows) { alloc_columns(columns(), rows); }
        bool parse_line(Cursor &c, size_t i, Runs &runs) {
            const Tok chr = c.token();
            if (!to_u32(c.token(), pos[i]) || !to_f64(c.token(), a[i]) || !to_f64(c.token(), b[i])) return false;
            runs.add(chr.first, chr.second);
            return true;
        }
    };

    using Row = pgt_fst_row;
    // chr start end mid fst nsites (fstWindow.cpp:88); inlined into both TSV loops (resident, passes), as the two lambdas it replaces were
    [[gnu::always_inline]] static size_t put(char *o, const std::string &chr, const Row &r) { return put_row(o, chr, {r.start, r.end, r.mid}, r.fst, {r.n}); }
    static constexpr auto reduce = pgt_fst_reduce;
    static constexpr auto reduce_cols = pgt_fst_reduce_cols;
    static constexpr auto reduce_tab = pgt_fst_reduce_tab;
};
}  // namespace

int main(int argc, char **argv) { return run_site_tool<FstWindow>(argc, argv); }
