// arg_checks_main.cc -- the shared argument checks (w2rap_contigger_amd/csrc/args.h) on malformed inputs, stand-alone, for a build with
// -fsanitize=address,undefined: a check that reads past an array while it refuses the input ends this program.
//
// stdin: the cases tests/test_arg_errors.py writes, one block each
//     case <name> <entry>
//     s <scalar field> <value>
//     a <array field> <count> <values ...>          the array in a heap block of exactly that size
//     a <array field> null | set                    a null pointer | an array the checks only compare with null
//     end
// stdout: "<name> <entry> <code> <message>" per case -- what the pieces of args.h answer, called in the order the entry calls them and
// without the entry's own checks in between (code 0, no message: they pass).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

#include "../include/w2rap_step3.h"
#include "../include/w2rap_step4.h"
#include "../include/w2rap_step5.h"
#include "../w2rap_contigger_amd/csrc/args.h"

using namespace w2::args;

namespace {

struct Case {
    std::map<std::string, long long> s;
    std::map<std::string, std::unique_ptr<char[]>> a;      // exact-size blocks (an empty array: a block of size 0)
    std::map<std::string, bool> present;
    uint8_t opaque = 0;
    long long scalar(const std::string& k) const { auto it = s.find(k); return it == s.end() ? 0 : it->second; }
    template <class T> const T* arr(const std::string& k) const {
        auto it = a.find(k);
        if (it != a.end()) return (const T*)it->second.get();
        auto p = present.find(k);
        return p != present.end() && p->second ? (const T*)&opaque : nullptr;
    }
};

template <class T> void fill(Case& c, const std::string& k, std::istringstream& line, size_t n) {
    std::unique_ptr<char[]> block(new char[n * sizeof(T)]);
    for (size_t i = 0; i < n; ++i) { long long v; line >> v; T x = (T)v; std::memcpy(block.get() + i * sizeof(T), &x, sizeof(T)); }
    c.a[k] = std::move(block);
}

bool is64(const std::string& k) { return k.size() > 3 && k.compare(k.size() - 4, 4, "_off") == 0; }

template <class In> void graph_of(const Case& c, In& in) {
    in.K = (int32_t)c.scalar("K"); in.n_edge_objs = c.scalar("n_edge_objs"); in.n_vertices = c.scalar("n_vertices"); in.n_paths = c.scalar("n_paths");
    in.edge_len = c.arr<uint32_t>("edge_len");
    in.from_off = c.arr<uint64_t>("from_off"); in.from_v = c.arr<int32_t>("from_v"); in.from_e = c.arr<int32_t>("from_e");
    in.to_off = c.arr<uint64_t>("to_off"); in.to_e = c.arr<int32_t>("to_e");
    in.path_offset = c.arr<int32_t>("path_offset"); in.path_off = c.arr<uint64_t>("path_off"); in.path_edges = c.arr<int32_t>("path_edges");
    in.read_len = c.arr<uint32_t>("read_len");
}
template <class In> void bases_and_reads_of(const Case& c, In& in) {
    in.edge_packed = c.arr<uint8_t>("edge_packed"); in.edge_byte_off = c.arr<uint64_t>("edge_byte_off");
    in.n_reads = c.scalar("n_reads");
    in.read_packed = c.arr<uint8_t>("read_packed"); in.read_byte_off = c.arr<uint64_t>("read_byte_off");
    in.quals = c.arr<uint8_t>("quals"); in.qual_off = c.arr<uint64_t>("qual_off");
}

#define TRY(piece) do { const Err e__ = (piece); if (e__.code) return e__; } while (0)

Err run(const std::string& entry, const Case& c) {
    if (entry == "step4") {
        w2rap_step4_in in{}; graph_of(c, in); bases_and_reads_of(c, in);
        TRY(null_arrays(in)); TRY(edge_off_start(in)); TRY(edge_lens(in)); TRY(adjacency(in)); TRY(from_v_agrees(in));
        return reads_and_paths(in);
    }
    if (entry == "partners" || entry == "add") {
        w2rap_step5_in in{}; graph_of(c, in); bases_and_reads_of(c, in);
        TRY(null_arrays(in)); TRY(edge_off_start(in)); TRY(edge_lens(in)); TRY(adjacency(in));
        if (entry == "partners") return reads_and_paths(in);
        TRY(crossings(in));
        return reads_and_paths(in, [&](uint64_t r) { return in.read_len[r] >= (1u << 31) ? Err{W2RAP_E_LIMIT, "a read of 2^31 bases"} : OK; });
    }
    if (entry == "open") {
        w2rap_step5_open_in in{}; graph_of(c, in); in.inv = c.arr<int32_t>("inv");
        TRY(null_arrays(in, !in.inv)); TRY(edge_lens(in, 1ull << 31)); TRY(adjacency(in));
        return reads_and_paths(in);
    }
    if (entry == "step3") {
        w2rap_step3_in in{};
        in.K = (int32_t)c.scalar("K"); in.n_edge_objs = c.scalar("n_edge_objs"); in.n_paths = c.scalar("n_paths");
        in.edge_packed = c.arr<uint8_t>("edge_packed"); in.edge_byte_off = c.arr<uint64_t>("edge_byte_off"); in.edge_len = c.arr<uint32_t>("edge_len");
        in.path_offset = c.arr<int32_t>("path_offset"); in.path_off = c.arr<uint64_t>("path_off"); in.path_edges = c.arr<int32_t>("path_edges");
        TRY(path_off_start(in)); TRY(null_path_edges(in)); TRY(edge_off_start(in)); TRY(path_off_ascends(in)); TRY(path_entries(in));
        return edge_lens(in);
    }
    return Err{-1, "unknown entry"};
}

}  // namespace

int main() {
    std::string text, name, entry;
    Case c;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        std::string what, k;
        line >> what;
        if (what == "case") { c = Case{}; line >> name >> entry; }
        else if (what == "s") { line >> k; line >> c.s[k]; }
        else if (what == "a") {
            std::string count;
            line >> k >> count;
            if (count == "null" || count == "set") { c.present[k] = count == "set"; continue; }
            const size_t n = std::stoull(count);
            if (is64(k)) fill<uint64_t>(c, k, line, n); else fill<uint32_t>(c, k, line, n);      // (int32 and uint32 alike: four bytes)
        } else if (what == "end") {
            const Err e = run(entry, c);
            std::printf("%s %s %d %s\n", name.c_str(), entry.c_str(), e.code, e.msg ? e.msg : "");
        }
    }
    return 0;
}
