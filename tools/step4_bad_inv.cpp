// step4_bad_inv.cpp -- the host graph edit of Step 4 (edit_graph, csrc/step4_host.hip) on an inv that the library's argument check accepts
// (an involution of edges of equal length) but that does not mirror runs onto runs: the reference's walk along the "mirror run"
// (GapToyTools3.cc:150-175) then leaves the graph or goes round a circle.  edit_graph has to answer W2RAP_E_GRAPH, with a message that names
// inv.  A CPU program with its own main, to be built with the host sanitizers; it touches no device:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I w2rap_contigger_amd/csrc tools/step4_bad_inv.cpp w2rap_contigger_amd/csrc/step4_host.hip -o step4_bad_inv
//   ./step4_bad_inv good && ./step4_bad_inv self && ./step4_bad_inv swap && ./step4_bad_inv circle
//
// (tests/test_step4_edit_model.py does exactly that).  The graphs are those of tests/step4_edit_cases.bad_inv_cases(): a vertex and its
// mirror are v and v ^ 1, an edge and its mirror e and e ^ 1, K = 20.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "step4_edit.h"
#include "../include/w2rap_step2.h"

using namespace w2;

// step4_host.hip also holds the host editor's uploads; of the rest of the library they need this one symbol, which nothing here calls
extern "C" int w2rap_step2_trim_cached(void) { return 0; }

namespace {

struct Build {
    HostGraph g;
    uint32_t state = 12345;
    Build() { g.K = 20; }
    int vertex() { for (int k = 0; k < 2; ++k) { g.frm.emplace_back(); g.frm_e.emplace_back(); g.to.emplace_back(); g.to_e.emplace_back(); } return (int)g.frm.size() - 2; }
    void one(int u, int v, const std::vector<uint8_t>& s) {
        const int e = (int)g.edges.size();
        g.edges.push_back(s);
        g.frm[u].push_back(v); g.frm_e[u].push_back(e); g.to[v].push_back(u); g.to_e[v].push_back(e);
    }
    int edge(int u, int v, int inner) {                       // u -> v of 2 (K - 1) + inner bases, and its mirror v' -> u'
        std::vector<uint8_t> s(2 * (g.K - 1) + inner), r(s.size());
        for (auto& b : s) { state = state * 1664525u + 1013904223u; b = (uint8_t)(state >> 30); }
        for (size_t i = 0; i < s.size(); ++i) r[i] = (uint8_t)(3 - s[s.size() - 1 - i]);
        one(u, v, s); one(v ^ 1, u ^ 1, r);
        return (int)g.edges.size() - 2;
    }
    std::vector<int> chain(int n_edges, const int* inner) {
        std::vector<int> vs, es;
        for (int i = 0; i <= n_edges; ++i) vs.push_back(vertex());
        for (int i = 0; i < n_edges; ++i) es.push_back(edge(vs[i], vs[i + 1], inner[i]));
        return es;
    }
    std::vector<int> mirror_inv() const { std::vector<int> inv(g.edges.size()); for (size_t e = 0; e < inv.size(); ++e) inv[e] = (int)e ^ 1; return inv; }
};

void swap_partners(std::vector<int>& inv, int a, int b) {     // a <-> b' and b <-> a' (was a <-> a', b <-> b')
    inv[a] = b ^ 1; inv[b ^ 1] = a; inv[b] = a ^ 1; inv[a ^ 1] = b;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    Build b;
    std::vector<int> inv;
    bool bad = true;
    if (which == "good" || which == "self") {
        const int inner[3] = {30, 31, 32};
        const auto r = b.chain(3, inner);
        inv = b.mirror_inv();
        if (which == "self") { inv[r[2]] = r[2]; inv[r[2] ^ 1] = r[2] ^ 1; } else bad = false;
    } else if (which == "swap") {
        const int inner[2] = {30, 33};
        const auto x = b.chain(2, inner), y = b.chain(2, inner);
        inv = b.mirror_inv();
        swap_partners(inv, x[1], y[1]);
    } else if (which == "circle") {
        const int inner[2] = {30, 33};
        const auto x = b.chain(2, inner);
        const int c[3] = {b.vertex(), b.vertex(), b.vertex()};
        int ce[3];
        for (int i = 0; i < 3; ++i) ce[i] = b.edge(c[i], c[(i + 1) % 3], 33);
        inv = b.mirror_inv();
        swap_partners(inv, x[1], ce[0] ^ 1);
    } else {
        std::fprintf(stderr, "usage: %s good|self|swap|circle\n", argv[0]);
        return 2;
    }
    for (size_t e = 0; e < inv.size(); ++e)
        if (inv[inv[e]] != (int)e || b.g.edges[inv[e]].size() != b.g.edges[e].size()) { std::fprintf(stderr, "%s: not an inv the library accepts\n", which.c_str()); return 2; }
    std::vector<char> dead(b.g.edges.size(), 0);
    std::vector<int32_t> deleted, map, add;
    uint64_t merged = 0;
    std::string err;
    const int rc = edit_graph(b.g, inv, dead, 0, true, deleted, map, add, merged, err);
    std::printf("%s: rc %d, merged %llu, \"%s\"\n", which.c_str(), rc, (unsigned long long)merged, err.c_str());
    if (bad) return rc == W2RAP_E_GRAPH && err.find("inv") != std::string::npos ? 0 : 1;
    return rc == 0 && merged == 2 && b.g.edges.size() == 2 && b.g.edges[0].size() == 38u * 3 + 30 + 31 + 32 - 2 * 19 ? 0 : 1;
}
