// step7_args_main.cc -- the argument checks of w2rap_step7_links that live in w2rap_contigger_amd/csrc/args.h (the lines, the involution,
// npairs, and the shared graph and path pieces on w2rap_step7_in) on malformed inputs, stand-alone, for a build with
// -fsanitize=address,undefined: a check that reads past an array while it refuses the input ends this program.
//
// stdin: the cases tests/test_step7_arg_errors.py writes, one block each
//     case <name>
//     s <scalar field> <value>
//     a <array field> <count> <values ...>          the array in a heap block of exactly that size
//     a <array field> null                          a null pointer
//     end
// stdout: "<name> <code> <message>" per case -- what the pieces answer, called in the order the entry calls them and without the entry's
// own checks in between (code 0, no message: they pass).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

#include "../include/w2rap_step7.h"
#include "../w2rap_contigger_amd/csrc/args.h"

using namespace w2::args;

namespace {

struct Case {
    std::map<std::string, long long> s;
    std::map<std::string, std::unique_ptr<char[]>> a;      // exact-size blocks (an empty array: a block of size 0)
    long long scalar(const std::string& k) const { auto it = s.find(k); return it == s.end() ? 0 : it->second; }
    template <class T> const T* arr(const std::string& k) const { auto it = a.find(k); return it == a.end() ? nullptr : (const T*)it->second.get(); }
};

template <class T> void fill(Case& c, const std::string& k, std::istringstream& line, size_t n) {
    std::unique_ptr<char[]> block(new char[n * sizeof(T)]);
    for (size_t i = 0; i < n; ++i) { long long v; line >> v; T x = (T)v; std::memcpy(block.get() + i * sizeof(T), &x, sizeof(T)); }
    c.a[k] = std::move(block);
}

bool is64(const std::string& k) { return k.size() > 3 && k.compare(k.size() - 4, 4, "_off") == 0; }

#define TRY(piece) do { const Err e__ = (piece); if (e__.code) return e__; } while (0)

Err run(const Case& c) {
    w2rap_step7_in in{};
    in.K = (int32_t)c.scalar("K"); in.n_edge_objs = c.scalar("n_edge_objs"); in.n_vertices = c.scalar("n_vertices"); in.n_paths = c.scalar("n_paths");
    in.n_lines = c.scalar("n_lines"); in.n_npairs = c.scalar("n_npairs");
    in.edge_len = c.arr<uint32_t>("edge_len");
    in.from_off = c.arr<uint64_t>("from_off"); in.from_v = c.arr<int32_t>("from_v"); in.from_e = c.arr<int32_t>("from_e");
    in.to_off = c.arr<uint64_t>("to_off"); in.to_e = c.arr<int32_t>("to_e"); in.inv = c.arr<int32_t>("inv");
    in.path_off = c.arr<uint64_t>("path_off"); in.path_edges = c.arr<int32_t>("path_edges");
    in.line_off = c.arr<uint64_t>("line_off"); in.cell_off = c.arr<uint64_t>("cell_off"); in.lpath_off = c.arr<uint64_t>("lpath_off");
    in.line_edges = c.arr<int32_t>("line_edges"); in.npairs = c.arr<int32_t>("npairs");
    if (too_large(in, READS_END)) return bad(TOO_LARGE);
    if (in.n_paths & 1) return bad(ODD_PATHS);
    TRY(null_arrays(in, !in.inv)); TRY(edge_lens(in, 1ull << 31)); TRY(adjacency(in)); TRY(from_v_agrees(in)); TRY(involution(in)); TRY(reads_and_paths(in));
    TRY(lines(in)); TRY(lines_cover(in)); TRY(line_lengths(in));
    return npairs_given(in, c.scalar("links_only") != 0);
}

}  // namespace

int main() {
    std::string text, name;
    Case c;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        std::string what, k;
        line >> what;
        if (what == "case") { c = Case{}; line >> name; }
        else if (what == "s") { line >> k; line >> c.s[k]; }
        else if (what == "a") {
            std::string count;
            line >> k >> count;
            if (count == "null") continue;
            const size_t n = std::stoull(count);
            if (is64(k)) fill<uint64_t>(c, k, line, n); else fill<uint32_t>(c, k, line, n);      // (int32 and uint32 alike: four bytes)
        } else if (what == "end") {
            const Err e = run(c);
            std::printf("%s %d %s\n", name.c_str(), e.code, e.msg ? e.msg : "");
        }
    }
    return 0;
}
