// args.h -- the host-side argument checks the one-shot entries of Steps 3-5 share, once: everything a kernel later uses as an index is
// looked at here before the device is touched.  Host-only (no HIP header: a plain C++ compiler reads it, and the checks run under a host
// sanitizer in tests/arg_checks_main.cc).
//
// The pieces are function templates over the input struct: w2rap_step4_in, w2rap_step5_in and w2rap_step5_open_in name their fields
// alike (w2rap_step3_in those of the edges and the paths).  A struct without edge_byte_off carries no bases, one without read_byte_off no
// reads: the checks of those arrays compile away.  Each piece answers Err{0} or the code and message of the FIRST fault it meets; an
// entry calls them in the order its checks have always had, with its own checks in between, so which fault of several is reported is
// the entry's decision and is pinned by tests/test_arg_errors.py.
#pragma once
#include <stdint.h>
#include <type_traits>
#include <vector>
#include "../../include/w2rap_step2.h"

namespace w2 {
namespace args {

struct Err { int code; const char* msg; };
constexpr Err OK{0, nullptr};
inline Err bad(const char* m) { return Err{W2RAP_E_ARG, m}; }
// in an entry with a fail(code, message) in scope
#define W2_ARGS(piece)                                        \
    do {                                                      \
        const w2::args::Err e__ = (piece);                    \
        if (e__.code) return fail(e__.code, e__.msg);         \
    } while (0)

template <class In, class = void> struct has_bases : std::false_type {};
template <class In> struct has_bases<In, std::void_t<decltype(In::edge_byte_off)>> : std::true_type {};
template <class In, class = void> struct has_reads : std::false_type {};
template <class In> struct has_reads<In, std::void_t<decltype(In::read_byte_off)>> : std::true_type {};
template <class In, class = void> struct has_placements : std::false_type {};       // path_offset and read_len (w2rap_step7_in has neither)
template <class In> struct has_placements<In, std::void_t<decltype(In::path_offset)>> : std::true_type {};

// ---- sizes and null arrays.  (What a size beyond the limit is answered with differs from entry to entry: theirs to say)
template <class In> bool too_large(const In& in, uint64_t reads_end) {
    return in.n_edge_objs >= (1ull << 31) || in.n_vertices >= (1ull << 31) || in.n_paths >= reads_end;
}
constexpr uint64_t READS_END = (1ull << 32) - 2;
constexpr const char* TOO_LARGE = "more than 2^31 edge objects or vertices, or 2^32 reads";      // (Step 4 and PartnersToEnds, at READS_END)
constexpr const char* ODD_PATHS = "n_paths is odd: reads r and r ^ 1 are mates";                  // (PartnersToEnds and the opening)
// graph_also_null: an array of the entry's own that every edge object needs is null
template <class In> Err null_arrays(const In& in, bool graph_also_null = false) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices, n = in.n_paths;
    bool g = !in.edge_len || !in.from_v || !in.from_e || !in.to_e || graph_also_null, r = !in.path_off;
    if constexpr (has_placements<In>::value) r = r || !in.path_offset || !in.read_len;
    if constexpr (has_bases<In>::value) g = g || !in.edge_packed || !in.edge_byte_off;
    if constexpr (has_reads<In>::value) r = r || !in.read_byte_off || !in.qual_off;
    if (E && g) return bad("null graph array");
    if (NV && (!in.from_off || !in.to_off)) return bad("null adjacency offsets");
    if (E && !NV) return bad("edge objects without vertices");
    if (n && r) return bad("null input array");
    return OK;
}

// ---- edge bases: edge_byte_off starts at 0; every object has K bases or more (and fewer than len_end) in ceil(len / 4) bytes
template <class In> Err edge_off_start(const In& in) {
    return in.n_edge_objs && in.edge_byte_off[0] != 0 ? bad("edge_byte_off must start at 0") : OK;
}
template <class In> Err edge_lens(const In& in, uint64_t len_end = 1ull << 32) {
    for (uint64_t o = 0; o < in.n_edge_objs; ++o) {
        if (in.edge_len[o] < (uint32_t)in.K || in.edge_len[o] >= len_end) return bad("an edge object shorter than K bases");
        if constexpr (has_bases<In>::value)
            if (in.edge_byte_off[o + 1] < in.edge_byte_off[o] || in.edge_byte_off[o + 1] - in.edge_byte_off[o] != ((uint64_t)in.edge_len[o] + 3) / 4)
                return bad("edge_byte_off does not match edge_len");
    }
    return OK;
}

// ---- adjacency lists: the offsets start at 0, ascend and end at E; from_v in [0, NV); from_e and to_e in [0, E), every object once in each
template <class In> Err adjacency(const In& in) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices;
    if (!NV) return OK;
    if (in.from_off[0] != 0 || in.to_off[0] != 0) return bad("from_off / to_off must start at 0");
    for (uint64_t v = 0; v < NV; ++v) if (in.from_off[v + 1] < in.from_off[v] || in.to_off[v + 1] < in.to_off[v]) return bad("from_off / to_off is not ascending");
    const char* const once = "the adjacency lists do not hold every edge object once";
    if (in.from_off[NV] != E || in.to_off[NV] != E) return bad(once);
    std::vector<char> sf(E, 0), st(E, 0);
    for (uint64_t i = 0; i < E; ++i) {
        if (in.from_v[i] < 0 || (uint64_t)in.from_v[i] >= NV) return bad("from_v names a vertex that does not exist");
        if (in.from_e[i] < 0 || (uint64_t)in.from_e[i] >= E || in.to_e[i] < 0 || (uint64_t)in.to_e[i] >= E) return bad("the adjacency lists name an edge object that does not exist");
        if (sf[in.from_e[i]]++ || st[in.to_e[i]]++) return bad(once);
    }
    return OK;
}
// behind adjacency(), Step 4: from_v[i] is the vertex to_e says edge from_e[i] enters
template <class In> Err from_v_agrees(const In& in) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices;
    if (!NV) return OK;
    std::vector<int32_t> right(E, -1);
    for (uint64_t v = 0; v < NV; ++v) for (uint64_t i = in.to_off[v]; i < in.to_off[v + 1]; ++i) right[in.to_e[i]] = (int32_t)v;
    for (uint64_t i = 0; i < E; ++i) if (right[in.from_e[i]] != in.from_v[i]) return bad("from_v and to_e disagree about the vertex an edge enters");
    return OK;
}
// behind adjacency(), AddNewStuff: a vertex's crossings (edges in x edges out) are counted in 32 bits
template <class In> Err crossings(const In& in) {
    for (uint64_t v = 0; v < in.n_vertices; ++v)
        if ((in.to_off[v + 1] - in.to_off[v]) * (in.from_off[v + 1] - in.from_off[v]) >= (1ull << 32)) return Err{W2RAP_E_LIMIT, "more than 2^32 crossings of one vertex"};
    return OK;
}

// ---- the involution: inv[e] in [0, E) and inv[inv[e]] == e (inv is not null)
template <class In> Err involution(const In& in) {
    const uint64_t E = in.n_edge_objs;
    for (uint64_t e = 0; e < E; ++e) if (in.inv[e] < 0 || (uint64_t)in.inv[e] >= E) return bad("inv names an edge object that does not exist");
    for (uint64_t e = 0; e < E; ++e) if ((uint64_t)in.inv[in.inv[e]] != e) return bad("inv is not an involution: inv[inv[e]] != e");
    return OK;
}

// ---- the lines of Step 7 (w2rap_step7_in): three nested CSRs, line -> cell -> path -> edge
// one level: off[0 .. n] starts at 0 and ascends
inline Err csr_level(const uint64_t* off, uint64_t n, const char* null_msg, const char* start_msg, const char* order_msg) {
    if (!off) return bad(null_msg);
    if (off[0] != 0) return bad(start_msg);
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return bad(order_msg);
    return OK;
}
// The shape MakeGaps and GetLineLengths rely on: an odd number of cells in every line; no cell without a path (so the first and the last
// cell hold one); the first path of the first and of the last cell holds an edge; every edge id in [0, E)
template <class In> Err lines(const In& in) {
    const uint64_t NL = in.n_lines;
    if (NL >= (1ull << 31)) return bad("2^31 lines or more: line ids are 32-bit");
    if (!NL) return OK;
    if (const Err e = csr_level(in.line_off, NL, "null line_off", "line_off must start at 0", "line_off is not ascending"); e.code) return e;
    const uint64_t NC = in.line_off[NL];
    if (const Err e = csr_level(in.cell_off, NC, "null cell_off", "cell_off must start at 0", "cell_off is not ascending"); e.code) return e;
    const uint64_t NLP = in.cell_off[NC];
    if (const Err e = csr_level(in.lpath_off, NLP, "null lpath_off", "lpath_off must start at 0", "lpath_off is not ascending"); e.code) return e;
    const uint64_t NE = in.lpath_off[NLP];
    if (NE && !in.line_edges) return bad("null line_edges");
    for (uint64_t i = 0; i < NE; ++i) if (in.line_edges[i] < 0 || (uint64_t)in.line_edges[i] >= in.n_edge_objs) return bad("a line names an edge object that does not exist");
    for (uint64_t l = 0; l < NL; ++l) {
        const uint64_t c0 = in.line_off[l], c1 = in.line_off[l + 1];
        if (((c1 - c0) & 1) == 0) return bad("a line with an even number of cells");
        for (uint64_t cl = c0; cl < c1; ++cl) if (in.cell_off[cl + 1] == in.cell_off[cl]) return bad(cl == c0 || cl == c1 - 1 ? "the first or last cell of a line is empty" : "a cell without a path");
        for (const uint64_t cl : {c0, c1 - 1}) { const uint64_t p = in.cell_off[cl]; if (in.lpath_off[p + 1] == in.lpath_off[p]) return bad("the first path of a line's first or last cell is empty"); }
    }
    return OK;
}
// behind lines(): every edge object belongs to a line (GetTol leaves -1 otherwise, and MakeGaps indexes llens with it)
template <class In> Err lines_cover(const In& in) {
    std::vector<char> seen(in.n_edge_objs, 0);
    const uint64_t NE = in.n_lines ? in.lpath_off[in.cell_off[in.line_off[in.n_lines]]] : 0;
    for (uint64_t i = 0; i < NE; ++i) seen[in.line_edges[i]] = 1;
    for (uint64_t e = 0; e < in.n_edge_objs; ++e) if (!seen[e]) return bad("an edge object that belongs to no line");
    return OK;
}
// behind lines() and edge_lens(): no line of 2^31 K-mers or more (a bound: every path of every cell counted in full)
template <class In> Err line_lengths(const In& in) {
    for (uint64_t l = 0; l < in.n_lines; ++l) {
        uint64_t sum = 0;
        for (uint64_t i = in.lpath_off[in.cell_off[in.line_off[l]]]; i < in.lpath_off[in.cell_off[in.line_off[l + 1]]]; ++i) sum += (uint64_t)in.edge_len[in.line_edges[i]] - (uint64_t)in.K + 1;
        if (sum >= (1ull << 31)) return Err{W2RAP_E_LIMIT, "a line of 2^31 K-mers or more"};
    }
    return OK;
}
// npairs: one entry per line when given; `needed`: it must be given
template <class In> Err npairs_given(const In& in, bool needed) {
    if (!in.npairs) return needed && in.n_lines ? bad("LINKS without LINES needs npairs") : (in.n_npairs ? bad("null npairs") : OK);
    return in.n_npairs != in.n_lines ? bad("npairs must have one entry per line") : OK;
}

// ---- read paths, reads and qualities
constexpr const char* PATH_OFF_DESCENDS = "path_off is not ascending";
template <class In> Err path_off_start(const In& in) {
    return in.n_paths && in.path_off[0] != 0 ? bad("path_off must start at 0") : OK;
}
template <class In> Err null_path_edges(const In& in) {
    return in.n_paths && in.path_off[in.n_paths] && !in.path_edges ? bad("null path_edges") : OK;
}
template <class In> Err path_off_ascends(const In& in) {
    for (uint64_t r = 0; r < in.n_paths; ++r) if (in.path_off[r + 1] < in.path_off[r]) return bad(PATH_OFF_DESCENDS);
    return OK;
}
// every entry in [0, E) (path_off ascends, path_edges is not null)
template <class In> Err path_entries(const In& in) {
    const uint64_t npe = in.n_paths ? in.path_off[in.n_paths] : 0;
    for (uint64_t i = 0; i < npe; ++i) if (in.path_edges[i] < 0 || (uint64_t)in.path_edges[i] >= in.n_edge_objs) return bad("a path names an edge object that does not exist");
    return OK;
}
// One walk over the reads: path_off starts at 0 and ascends; with reads, read_byte_off and qual_off start at 0 and match read_len, and
// read_packed and quals are not null; path_edges is not null and every entry lies in [0, E).  each(r): the entry's own look at read r,
// behind the shared checks of that read (Err; anything but OK ends the walk)
template <class In, class Each> Err reads_and_paths(const In& in, Each each) {
    const uint64_t n = in.n_paths;
    if (!n) return OK;
    if constexpr (has_reads<In>::value) {
        if (in.path_off[0] != 0 || in.read_byte_off[0] != 0 || in.qual_off[0] != 0) return bad("path_off, read_byte_off and qual_off must start at 0");
    } else if (const Err e = path_off_start(in); e.code) return e;
    for (uint64_t r = 0; r < n; ++r) {
        if (in.path_off[r + 1] < in.path_off[r]) return bad(PATH_OFF_DESCENDS);
        if constexpr (has_reads<In>::value) {
            if (in.read_byte_off[r + 1] < in.read_byte_off[r] || in.read_byte_off[r + 1] - in.read_byte_off[r] != ((uint64_t)in.read_len[r] + 3) / 4)
                return bad("read_byte_off does not match read_len");
            if (in.qual_off[r + 1] < in.qual_off[r] || in.qual_off[r + 1] - in.qual_off[r] != in.read_len[r]) return bad("qual_off does not match read_len");
        }
        const Err e = each(r);
        if (e.code) return e;
    }
    if (const Err e = null_path_edges(in); e.code) return e;
    if constexpr (has_reads<In>::value) {
        if (in.read_byte_off[n] && !in.read_packed) return bad("null read_packed");
        if (in.qual_off[n] && !in.quals) return bad("null quals");
    }
    return path_entries(in);
}
template <class In> Err reads_and_paths(const In& in) { return reads_and_paths(in, [](uint64_t) { return OK; }); }

// ---- each edge object's two vertices from the adjacency lists (which adjacency() has passed), -1: none
template <class In> void edge_ends(const In& in, std::vector<int32_t>& vleft, std::vector<int32_t>& vright) {
    vleft.assign(in.n_edge_objs, -1); vright.assign(in.n_edge_objs, -1);
    for (uint64_t v = 0; v < in.n_vertices; ++v) {
        for (uint64_t i = in.from_off[v]; i < in.from_off[v + 1]; ++i) vleft[in.from_e[i]] = (int32_t)v;
        for (uint64_t i = in.to_off[v]; i < in.to_off[v + 1]; ++i) vright[in.to_e[i]] = (int32_t)v;
    }
}

}  // namespace args
}  // namespace w2
