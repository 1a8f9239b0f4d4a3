// site_common.h — shared by the fstWindow and hetWindow hosts: both tools are one run (fstWindow.cpp:109-155,
// hetWindow.cpp:107-153) over a table of sites with windows counted in sites; only the columns, the messages and the
// row differ.  A tool is a struct with
//     name, open_error, what        the tag of its `die` texts and of its column cache, and its two messages
//     spec[]                        the device parser's token spec of one line
//     Table                         the host columns: parse_line(Cursor&, row, Runs&) and columns() — a tuple of SiteColumn,
//                                   the ONE statement of the columns from which everything else is derived, alloc(rows) too
//     Row, put(o, chr, row)         the library's row and its TSV line
//     reduce, reduce_cols, reduce_tab    the three library calls (host columns / device columns / device window table)
//     usage(W, S)
// and its main is `return run_site_tool<Tool>(argc, argv);`.  Everything is resolved at compile time: the parse loop and
// the TSV writer are the same instantiations of parse_table and write_rows that each tool used to spell out itself.
#pragma once

#include <tuple>

#include "host_common.h"

namespace pgthost {

// One column: its token in the device parser's spec and the host column; the element size is the column's type.
template <class T>
struct SiteColumn {
    int token;
    Column<T> &col;
    static constexpr size_t elem = sizeof(T);
    T *host() const { return col.data(); }
    T *on(const DeviceTable &d) const { return d.col<T>(token); }      // the same column of a table parsed on the GPU
    T *gathered(void *d) const { return static_cast<T *>(d); }         // ... of a GPU's gathered slice (reduce_on_devices)
    void borrow(void *mapped) const { col.borrow(static_cast<T *>(mapped)); }
};

// The folds over a tool's columns (a tuple), each in column order: f(column); a vector of f(column); a tuple of f(column).
template <class Cols, class F>
void each_column(const Cols &cols, F f) {
    std::apply([&](auto... c) { (f(c), ...); }, cols);
}
template <class E, class Cols, class F>
std::vector<E> list_columns(const Cols &cols, F f) {
    return std::apply([&](auto... c) { return std::vector<E>{f(c)...}; }, cols);
}
template <class Cols, class F>
auto map_columns(const Cols &cols, F f) {
    return std::apply([&](auto... c) { return std::tuple{f(c)...}; }, cols);
}
// what a Table's alloc(rows) is
template <class Cols>
void alloc_columns(const Cols &cols, size_t rows) {
    each_column(cols, [&](auto c) { c.col.alloc(rows); });
}

// f(ctx, column pointers..., rest...): how the three library calls receive a tuple of column pointers
template <class F, class Ptrs, class... Rest>
int call_with_columns(F f, pgt_ctx *ctx, const Ptrs &ptrs, Rest... rest) {
    return std::apply([&](auto... p) { return f(ctx, p..., rest...); }, ptrs);
}

template <class Tool>
int run_site_tool(int argc, char **argv) {
    using Table = typename Tool::Table;
    using Row = typename Tool::Row;
    const std::string name = Tool::name;
    uint32_t W = 1, S = 1;  // fstWindow.cpp:161-162, hetWindow.cpp:159-160
    if (argc < 2) {
        Tool::usage(W, S);
        return 0;
    }
    PhaseTimer timer;
    {   // the reference opens the file before it looks at the other arguments (fstWindow.cpp:45-49, hetWindow.cpp:42-46)
        FILE *probe = std::fopen(argv[1], "rb");
        if (!probe) die(std::string(Tool::open_error) + argv[1]);
        std::fclose(probe);
    }
    parse_window_args(argc, argv, W, S);
    DeviceOpener device;  // HIP start-up runs beside the parse; PGT_DEVICES=0,1,..: one context and host thread per GPU
    const bool multi = device.count() > 1;
    std::vector<DevicePiece> pieces;  // multi-GPU device ingest: one parsed piece of the text per GPU

    // what is derived from the tool's columns
    auto host_ptrs = [](Table &t) { return map_columns(t.columns(), [](auto c) { return c.host(); }); };
    auto device_ptrs = [](Table &t, const DeviceTable &d) { return map_columns(t.columns(), [&](auto c) { return c.on(d); }); };
    auto hybrid_columns = [](Table &t) { return list_columns<HybridColumn>(t.columns(), [](auto c) { return HybridColumn{c.token, c.elem, c.host()}; }); };
    Table tab;  // parsed in parallel chunks straight into the columns
    const auto columns = tab.columns();
    std::vector<ColumnCache::Col> cols = list_columns<ColumnCache::Col>(columns, [](auto c) { return ColumnCache::Col{nullptr, c.elem}; });
    const std::vector<GatherColumn> gather = list_columns<GatherColumn>(columns, [](auto c) { return GatherColumn{c.token, c.elem}; });
    size_t site_bytes = 0;  // on the GPU, per site
    each_column(columns, [&](auto c) { site_bytes += c.elem; });
    const int n_tokens = (int)sizeof(Tool::spec);

    const size_t row_bytes_max = 80;  // of a TSV row, behind its chromosome's name
    Runs runs;
    size_t n = 0;
    DeviceTable dtab;  // the table when it was parsed on the GPU
    Text text;         // the input text (not opened when the column cache answers)
    ColumnCache cache(Tool::name, argv[1]);  // only with PGT_COLUMN_CACHE=<dir>
    bool on_device = false;
    if (cache.load(n, runs, cols)) {
        device.plan_host_io(true);  // host columns will be uploaded: stage and warm up beside what is left to do
        size_t k = 0;
        each_column(columns, [&](auto c) { c.borrow(cols[k++].data); });
        timer.lap("cache map");
    } else {
        if (!text.open(argv[1])) die(std::string(Tool::open_error) + argv[1]);
        const char *what = Tool::what;
        const uint8_t *spec = Tool::spec;
        if (const uint64_t resident = resident_limit(text.begin(), text.end(), site_bytes, [&] { return device.get(); })) {
            // larger than the GPU (or PGT_MAX_RESIDENT_SITES): block by block, rows printed as the blocks finish
            const std::string miscount = name + ": a pass parsed another number of rows than the first scan counted";
            reduce_in_passes<Row>(
                device, text.begin(), text.end(), W, S, resident, runs, timer,
                [&](pgt_ctx *c, const char *pb, const char *pe, uint64_t first_row, uint64_t n_rows, const pgt_win *w, size_t nw, Row *out, std::string *error) {
                    DeviceTable piece;
                    Runs piece_runs;
                    Table t;
                    if (ingest_on_device(c, pb, pe, spec, n_tokens, what, argv[1], first_row + 1, piece, piece_runs, error)) {
                        if (error && !error->empty()) return;
                        if (piece.n != n_rows) die(miscount);
                        if (nw) check(call_with_columns(Tool::reduce_cols, c, device_ptrs(t, piece), piece.n, w, nw, out, nw * sizeof(*out)), c);
                    } else {
                        const size_t k = parse_table(pb, pe, t, piece_runs, what, argv[1], first_row + 1, error);
                        if (error && !error->empty()) return;
                        if (k != n_rows) die(miscount);
                        if (nw) check(call_with_columns(Tool::reduce, c, host_ptrs(t), k, w, nw, out), c);
                    }
                },
                [&](const Row *r, size_t nw, const pgt_win *w) {
                    write_rows(nw, longest_name(runs) + row_bytes_max, [&](size_t i, char *o) { return Tool::put(o, runs.name[w[i].label_run], r[i]); });
                });
            finish(timer);
        }
        bool parsed = false;  // by the hybrid path, into the host table (the data ended inside its head)
        if (gpu_ingest_wanted(text.size()) && !multi) {  // large inputs: head on the host beside HIP start-up, tail on the GPU
            const int h = ingest_hybrid(device, text.begin(), text.end(), spec, n_tokens, what, argv[1], tab, hybrid_columns, dtab, runs, &n, timer);
            on_device = h == 1;
            parsed = h == 2;
        }
        if (gpu_ingest_wanted(text.size()) && !on_device && !parsed) {
            pgt_ctx *c = device.get();
            timer.lap("wait for HIP");
            if (multi) {
                on_device = ingest_on_devices(device, text.begin(), text.end(), spec, n_tokens, what, argv[1], pieces, runs, &n);
            } else {
                on_device = ingest_on_device(c, text.begin(), text.end(), spec, n_tokens, what, argv[1], 1, dtab, runs);
                n = dtab.n;
            }
            timer.lap(on_device ? "gpu parse" : "gpu parse (refused)");
        }
        if (!on_device && !parsed) {
            device.plan_host_io(true, text.size());  // the host parser's columns will be uploaded: staging ring (inputs from 32 MiB) + first-copy set-up beside the parse
            n = parse_table(text.begin(), text.end(), tab, runs, what, argv[1], 1);
            timer.lap("parse");
            if (cache.enabled()) {
                size_t k = 0;
                each_column(columns, [&](auto c) { cols[k++].data = c.host(); });
                cache.store(n, runs, cols);
                timer.lap("cache write");
            }
        }
    }

    SiteWindows sw;
    sw.build(runs, W, S, [&] { return device.get(); }, &timer, multi);
    const size_t n_win = sw.n;
    if (n_win == 0) return 0;

    timer.lap("window table");
    pgt_ctx *ctx = device.get();
    RowArray<Row> rows(n_win);
    timer.lap("wait for HIP");
    set_site_hints(ctx, W, S);  // the strategy follows the tool's arguments, on one GPU as on several
    const auto ptrs = on_device && !multi ? device_ptrs(tab, dtab) : host_ptrs(tab);
    if (multi) {
        reduce_on_devices<Row>(
            device, sw.win, W, S, pieces, gather, rows.data(),
            [&](pgt_ctx *c, uint64_t lo, uint64_t n_k, const pgt_win *w, size_t nw, Row *out, size_t) {
                return call_with_columns(Tool::reduce, c, map_columns(ptrs, [&](auto p) { return p + lo; }), n_k, w, nw, out);
            },
            [&](pgt_ctx *c, void *const *d, uint64_t n_k, const pgt_win *w, size_t nw, Row *out, size_t bytes) {
                size_t k = 0;
                return call_with_columns(Tool::reduce_cols, c, map_columns(columns, [&](auto col) { return col.gathered(d[k++]); }), n_k, w, nw, out, bytes);
            });
        free_pieces(pieces);
    } else if (sw.tab)
        check(call_with_columns(Tool::reduce_tab, ctx, ptrs, n, on_device, sw.tab, rows.data(), rows.size() * sizeof(rows[0])), ctx);
    else if (on_device)
        check(call_with_columns(Tool::reduce_cols, ctx, ptrs, n, sw.win.data(), n_win, rows.data(), rows.size() * sizeof(rows[0])), ctx);
    else
        check(call_with_columns(Tool::reduce, ctx, ptrs, n, sw.win.data(), n_win, rows.data()), ctx);
    timer.lap("gpu reduce");

    write_rows(n_win, longest_name(runs) + row_bytes_max, [&](size_t i, char *o) { return Tool::put(o, runs.name[sw.label(i)], rows[i]); });
    finish(timer);
}

}  // namespace pgthost
