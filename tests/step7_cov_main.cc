// step7_cov_main.cc -- the host half of w2rap_step7_coverage (w2rap_contigger_amd/csrc/step7_peak.h: the argument checks, the candidates,
// the peak finder, the grouping of the cells) stand-alone, for a build with -fsanitize=address,undefined: a check that reads past an array
// while it refuses the input, or a peak finder that steps outside its vectors, ends this program.
//
// stdin: the cases tests/test_step7_cov_arg_errors.py writes, one block each
//     case <name>
//     s <scalar field> <value>
//     a <array field> <count> <values ...>          the array in a heap block of exactly that size
//     a <array field> null                          a null pointer
//     end
// stdout per case: "<name> <code> <message>" for a refused input; for one that passes "<name> 0 <base_cov as 16 hex digits> <way>
// <candidates> <groups> <edges of all z>", llens and npairs being given with the case.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

#include "../w2rap_contigger_amd/csrc/step7_peak.h"

namespace {

struct Case {
    std::map<std::string, long long> s;
    std::map<std::string, std::unique_ptr<char[]>> a;
    long long scalar(const std::string& k) const { auto it = s.find(k); return it == s.end() ? 0 : it->second; }
    template <class T> const T* arr(const std::string& k) const { auto it = a.find(k); return it == a.end() ? nullptr : (const T*)it->second.get(); }
};

template <class T> void fill(Case& c, const std::string& k, std::istringstream& line, size_t n) {
    std::unique_ptr<char[]> block(new char[n * sizeof(T)]);
    for (size_t i = 0; i < n; ++i) { long long v; line >> v; T x = (T)v; std::memcpy(block.get() + i * sizeof(T), &x, sizeof(T)); }
    c.a[k] = std::move(block);
}

bool is64(const std::string& k) { return k.size() > 3 && k.compare(k.size() - 4, 4, "_off") == 0; }

void run(const std::string& name, const Case& c) {
    w2rap_step7_cov_in in{};
    in.K = (int32_t)c.scalar("K"); in.n_edge_objs = c.scalar("n_edge_objs"); in.n_paths = c.scalar("n_paths"); in.n_lines = c.scalar("n_lines");
    in.edge_len = c.arr<uint32_t>("edge_len"); in.inv = c.arr<int32_t>("inv"); in.path_off = c.arr<uint64_t>("path_off"); in.path_edges = c.arr<int32_t>("path_edges");
    in.line_off = c.arr<uint64_t>("line_off"); in.cell_off = c.arr<uint64_t>("cell_off"); in.lpath_off = c.arr<uint64_t>("lpath_off"); in.line_edges = c.arr<int32_t>("line_edges");
    w2rap_step7_cov_params P{};
    P.flags = (uint32_t)c.scalar("flags"); P.frac = 0.1; P.min_edge_size = (int32_t)c.scalar("min_edge_size");
    char err[256] = {0};
    const int rc = w2::cov::check(&in, &P, err, sizeof err);
    if (rc) { std::printf("%s %d %s\n", name.c_str(), rc, err); return; }
    w2::cov::Candidates C;
    w2::cov::candidates(c.arr<int32_t>("llens"), c.arr<int32_t>("npairs"), in.n_lines, C);
    w2::cov::PeakCounters n;
    const double base = w2::cov::find_peak(C.covx, C.mass, n);
    w2::cov::CellGroups G;
    w2::cov::cell_groups(in, G);
    unsigned long long bits;
    std::memcpy(&bits, &base, 8);
    std::printf("%s 0 %016llx %llu %zu %zu %zu\n", name.c_str(), bits, (unsigned long long)n.way, C.covx.size(), G.line.size(), G.z.size());
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
        } else if (what == "end") run(name, c);
    }
    return 0;
}
