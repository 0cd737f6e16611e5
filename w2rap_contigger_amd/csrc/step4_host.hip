// step4_host.hip -- Step 4's graph edit on the host, as the reference runs it on ordered adjacency lists: the judge the device edit
// (step4_edit.hip) is tested against, what W2RAP_STEP4_EDIT_ON_HOST and VOTE_ONLY run, and what a call starts over with when a precondition
// of the device edit does not hold.  HostEditor4 wraps edit_graph() for the driver's pass loop (step4_clean.hip).  No kernel is launched here.
#include <cstring>
#include <unordered_map>
#include "step4_edit.h"

namespace w2 {

void unpack_edges(uint64_t E, const uint8_t* packed, const uint64_t* byte_off, const uint32_t* len, std::vector<std::vector<uint8_t>>& edges) {
    edges.resize(E);
    for (uint64_t e = 0; e < E; ++e) {
        edges[e].resize(len[e]);
        const uint8_t* s = packed + byte_off[e];
        for (uint32_t i = 0; i < len[e]; ++i) edges[e][i] = (s[i >> 2] >> (2 * (i & 3))) & 3u;
    }
}

// HyperBasevector::Involution (HyperBasevector.cc:648-660) for a graph whose edge sequences are distinct: the object holding the reverse complement
int host_involution(const HostGraph& g, std::vector<int>& inv, std::string& err) {
    std::unordered_map<std::string, int> where;
    where.reserve(g.edges.size() * 2);
    for (size_t e = 0; e < g.edges.size(); ++e) {
        if (!where.emplace(std::string(g.edges[e].begin(), g.edges[e].end()), (int)e).second) { err = "Involution: two edge objects with the same sequence"; return W2RAP_E_GRAPH; }
    }
    inv.assign(g.edges.size(), -1);
    std::string rc;
    for (size_t e = 0; e < g.edges.size(); ++e) {
        const auto& s = g.edges[e];
        rc.resize(s.size());
        for (size_t i = 0; i < s.size(); ++i) rc[i] = (char)(3 - s[s.size() - 1 - i]);
        auto it = where.find(rc);
        if (it == where.end()) { err = "Involution: an edge object has no reverse complement in the graph (HyperBasevector.cc:648-660 needs every edge's RC)"; return W2RAP_E_GRAPH; }
        inv[e] = it->second;
    }
    return 0;
}

// one pass's edit.  in: dead[e] from the vote (ids of g).  out: the sorted unique deleted list, g and inv edited,
// map[e] (old id -> final id, -1: deleted) and add[e] (offsets[e]) for the path kernels, the number of merged runs.
// -> 0, or W2RAP_E_GRAPH (g and inv are then half edited and of no use): the reference walks a pushed run's mirror image
// (inv[eright], inv[eleft]) along the single out-edges of its kill vertices without a look (GapToyTools3.cc:150-175); an inv that does
// not mirror runs onto runs sends that walk off the graph or round a circle, so here every step of it is checked
int edit_graph(HostGraph& g, std::vector<int>& inv, std::vector<char>& dead, unsigned min_size, bool edit, std::vector<int32_t>& deleted,
               std::vector<int32_t>& map, std::vector<int32_t>& add, uint64_t& n_merged, std::string& err) {
    const size_t NV = g.frm.size(), E0 = g.edges.size();
    if (min_size > 0) {                                                      // Clean200.cc:370-380
        for (size_t v = 0; v < NV; ++v) {
            if (!g.to[v].empty() || g.frm[v].size() != 1) continue;
            const int w = g.frm[v][0];
            if ((int)v == w || g.to[w].size() != 1 || !g.frm[w].empty()) continue;
            const int e = g.frm_e[v][0];
            if (g.kmers(e) > (int)min_size) continue;
            dead[e] = 1;
        }
    }
    deleted.clear();
    for (size_t e = 0; e < E0; ++e) if (dead[e]) deleted.push_back((int32_t)e);
    n_merged = 0;
    if (!edit) return 0;
    g.delete_edges(dead);
    // Cleanup: a path is cut at its first edge that is no longer in the graph (`alive` below)
    std::vector<char> alive;
    g.used(alive);
    // RemoveUnneededVertices2
    std::vector<int> to_left, to_right;
    g.left_right(to_left, to_right);
    std::vector<char> kill(NV, 0);
    std::vector<int> queue;
    for (size_t v = 0; v < NV; ++v)
        if (g.frm[v].size() == 1 && g.to[v].size() == 1 && g.frm[v][0] != g.to[v][0] && !g.edges[g.frm_e[v][0]].empty() && !g.edges[g.to_e[v][0]].empty()) {
            kill[v] = 1; queue.push_back((int)v);
        }
    std::vector<std::pair<int, int>> bound;
    while (!queue.empty()) {
        const int v = queue.back(); queue.pop_back();
        if (!kill[v]) continue;
        int eleft, vl = v;
        do { kill[vl] = 0; eleft = g.to_e[vl][0]; vl = g.to[vl][0]; } while (kill[vl]);
        int eright, vr = v;
        do { kill[vr] = 0; eright = g.frm_e[vr][0]; vr = g.frm[vr][0]; } while (kill[vr]);
        if (eleft < inv[eright]) { bound.emplace_back(eleft, eright); bound.emplace_back(inv[eright], inv[eleft]); }
    }
    std::vector<int> renum(E0), offsets(E0, 0), new_nos;
    for (size_t e = 0; e < E0; ++e) renum[e] = (int)e;
    std::vector<char> dead2(E0, 0);
    while (!bound.empty()) {
        const auto b = bound.back(); bound.pop_back();
        const int new_no = (int)g.edges.size();
        int off = g.kmers(b.first);
        renum[b.first] = new_no; dead2[b.first] = 1;
        // the first walk checks every step; the second one below repeats it on the unchanged graph
        size_t steps = 0;
        for (int v = to_right[b.first]; v != to_right[b.second]; v = g.frm[v][0]) {
            if (g.frm[v].size() != 1 || ++steps > NV) {
                err = "inv does not mirror runs onto runs: the walk from inv[eright] of a merged run does not reach inv[eleft] along single out-edges";
                return W2RAP_E_GRAPH;
            }
            const int e = g.frm_e[v][0];
            dead2[e] = 1; offsets[e] = off; renum[e] = new_no; off += g.kmers(e);
        }
        std::vector<uint8_t> ne(g.edges[b.first]);
        ne.reserve((size_t)off + g.K - 1);
        for (int v = to_right[b.first]; v != to_right[b.second]; v = g.frm[v][0]) {
            const int e = g.frm_e[v][0];
            ne.resize((size_t)offsets[e]);
            ne.insert(ne.end(), g.edges[e].begin(), g.edges[e].end());
        }
        g.add_edge(to_left[b.first], to_right[b.second], std::move(ne));
        new_nos.push_back(new_no);
    }
    n_merged = new_nos.size();
    dead2.resize(g.edges.size(), 0);
    g.delete_edges(dead2);
    inv.resize(g.edges.size(), -1);
    for (size_t k = 0; k + 1 < new_nos.size(); k += 2) { inv[new_nos[k]] = new_nos[k + 1]; inv[new_nos[k + 1]] = new_nos[k]; }
    // CleanupCore
    std::vector<char> u;
    g.used(u);
    std::vector<int> to_new(u.size(), -1);
    int c = 0;
    for (size_t i = 0; i < u.size(); ++i) if (u[i]) to_new[i] = c++;
    std::vector<int> inv2; inv2.reserve(c);
    for (size_t i = 0; i < u.size(); ++i) if (u[i]) inv2.push_back(inv[i] < 0 ? -1 : to_new[inv[i]]);
    inv.swap(inv2);
    std::vector<std::vector<uint8_t>> ed; ed.reserve(c);
    for (size_t i = 0; i < u.size(); ++i) if (u[i]) ed.push_back(std::move(g.edges[i]));
    g.edges.swap(ed);
    std::vector<int> newv(NV, -1);
    int nv = 0;
    for (size_t v = 0; v < NV; ++v) if (!g.frm[v].empty() || !g.to[v].empty()) newv[v] = nv++;
    HostGraph h; h.K = g.K;
    h.frm.resize(nv); h.frm_e.resize(nv); h.to.resize(nv); h.to_e.resize(nv);
    for (size_t v = 0; v < NV; ++v) {
        if (newv[v] < 0) continue;
        const int x = newv[v];
        h.frm[x].swap(g.frm[v]); h.frm_e[x].swap(g.frm_e[v]); h.to[x].swap(g.to[v]); h.to_e[x].swap(g.to_e[v]);
        for (auto& w : h.frm[x]) w = newv[w];
        for (auto& w : h.to[x]) w = newv[w];
        for (auto& e : h.frm_e[x]) e = to_new[e];
        for (auto& e : h.to_e[x]) e = to_new[e];
    }
    h.edges.swap(g.edges);
    g = std::move(h);
    map.assign(E0, -1); add.assign(E0, 0);
    for (size_t e = 0; e < E0; ++e) if (alive[e]) { map[e] = to_new[renum[e]]; add[e] = offsets[e]; }
    return 0;
}

void pack_edges(const HostGraph& g, std::vector<uint8_t>& packed, std::vector<uint64_t>& boff, std::vector<uint32_t>& len) {
    const size_t E = g.edges.size();
    boff.assign(E + 1, 0); len.resize(E);
    for (size_t e = 0; e < E; ++e) { len[e] = (uint32_t)g.edges[e].size(); boff[e + 1] = boff[e] + (g.edges[e].size() + 3) / 4; }
    packed.assign(boff[E], 0);
    for (size_t e = 0; e < E; ++e) {
        uint8_t* d = packed.data() + boff[e];
        const auto& s = g.edges[e];
        for (size_t i = 0; i < s.size(); ++i) d[i >> 2] |= (uint8_t)(s[i] << (2 * (i & 3)));
    }
}

void make_csr(const HostGraph& g, Csr& c) {
    const size_t NV = g.frm.size(), E = g.edges.size();
    c.from_off.assign(NV + 1, 0); c.to_off.assign(NV + 1, 0);
    c.from_v.clear(); c.from_e.clear(); c.to_v.clear(); c.to_e.clear();
    c.vleft.assign(E, -1); c.vright.assign(E, -1);
    for (size_t v = 0; v < NV; ++v) {
        for (size_t i = 0; i < g.frm[v].size(); ++i) { c.from_v.push_back(g.frm[v][i]); c.from_e.push_back(g.frm_e[v][i]); c.vleft[g.frm_e[v][i]] = (int32_t)v; }
        for (size_t i = 0; i < g.to[v].size(); ++i) { c.to_v.push_back(g.to[v][i]); c.to_e.push_back(g.to_e[v][i]); c.vright[g.to_e[v][i]] = (int32_t)v; }
        c.from_off[v + 1] = c.from_v.size(); c.to_off[v + 1] = c.to_v.size();
    }
}

int upload_graph4(Ctx& c, Graph4& g, const uint8_t* packed, const uint64_t* boff, const uint32_t* elen, const uint64_t* from_off, const int32_t* from_v,
                  const int32_t* from_e, const uint64_t* to_off, const int32_t* to_v, const int32_t* to_e, const int32_t* vleft, const int32_t* vright,
                  const int32_t* inv) {
    const uint64_t E = g.E, NV = g.NV;
    W2_TRY(up_pooled(c, &g.ebits, packed, g.ebytes_cap, 32));
    W2_TRY(up_pooled(c, &g.ebyte, boff, boff ? E + 1 : 0));
    W2_TRY(up_pooled(c, &g.elen, elen, E));
    W2_TRY(up_pooled(c, &g.from_off, from_off, from_off ? NV + 1 : 0));
    W2_TRY(up_pooled(c, &g.from_v, from_v, E));
    W2_TRY(up_pooled(c, &g.from_e, from_e, E));
    W2_TRY(up_pooled(c, &g.to_off, to_off, to_off ? NV + 1 : 0));
    W2_TRY(up_pooled(c, &g.to_v, to_v, E));
    W2_TRY(up_pooled(c, &g.to_e, to_e, E));
    W2_TRY(up_pooled(c, &g.vleft, vleft, E));
    W2_TRY(up_pooled(c, &g.vright, vright, E));
    return up_pooled(c, &g.inv, inv, E);
}

int HostEditor4::tasks(Ctx& c, const Graph4&, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T) {
    std::vector<int32_t> bvert, boutdeg;
    std::vector<Task> tasks;
    for (size_t v = 0; v < g.frm.size(); ++v) {
        if (g.to[v].empty() || g.frm[v].size() <= 1) continue;
        const uint32_t b = (uint32_t)bvert.size();
        bvert.push_back((int32_t)v); boutdeg.push_back((int32_t)g.frm[v].size());
        for (int e : g.to_e[v]) tasks.push_back(Task{b, 0u, e, 0u});
        for (int e : g.frm_e[v]) tasks.push_back(Task{b, 1u, e, 0u});
        for (int e : g.to_e[v]) tasks.push_back(Task{b, 2u, inv[e], 0u});
        for (int e : g.frm_e[v]) tasks.push_back(Task{b, 3u, inv[e], 0u});
    }
    *B = bvert.size(); *T = tasks.size(); *d_bvert = nullptr; *d_outdeg = nullptr; *d_tasks = nullptr;
    if (!*B || *B >= (1ull << 27)) return 0;
    W2_TRY(up_pooled(c, d_bvert, (const int32_t*)bvert.data(), *B));
    W2_TRY(up_pooled(c, d_outdeg, (const int32_t*)boutdeg.data(), *B));
    W2_TRY(up_pooled(c, d_tasks, (const Task*)tasks.data(), *T));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the host vectors have been read)
    return 0;
}

int HostEditor4::pass(Ctx& c, const Graph4& gd, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
                      std::vector<int32_t>* deleted, uint64_t* n_merged) {
    const uint64_t E0 = g.edges.size();
    std::vector<char> dead(E0, 0);
    if (E0) W2_HIP(hipMemcpyAsync(dead.data(), d_dead, E0, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    std::vector<int32_t> map, add;
    W2_TRY(edit_graph(g, inv, dead, min_size, edit, *deleted, map, add, *n_merged, c.err));
    *d_map = nullptr; *d_add = nullptr;
    if (!edit) { *next = gd; return 0; }
    // ---- the next pass's graph on the device
    std::vector<uint8_t> packed; std::vector<uint64_t> boff; std::vector<uint32_t> elen;
    Csr csr;
    pack_edges(g, packed, boff, elen);
    make_csr(g, csr);
    Graph4 n; n.K = gd.K; n.E = g.edges.size(); n.NV = g.frm.size(); n.ebytes_cap = packed.size();
    W2_TRY(upload_graph4(c, n, packed.data(), boff.data(), elen.data(), csr.from_off.data(), csr.from_v.data(), csr.from_e.data(), csr.to_off.data(),
                         csr.to_v.data(), csr.to_e.data(), csr.vleft.data(), csr.vright.data(), inv.data()));
    W2_TRY(up_pooled(c, d_map, (const int32_t*)map.data(), E0));
    W2_TRY(up_pooled(c, d_add, (const int32_t*)add.data(), E0));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the host vectors have been read)
    *next = n;
    return 0;
}

}  // namespace w2
