// step4_edit.h -- what step4_clean.hip (the vote and the driver of Step 4), step4_edit.hip (the graph edit on the device) and
// step4_host.hip (the same edit on the host) share.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "ctx.h"

namespace w2 {

// one pass's graph on the device: the arrays the vote kernels read (packed 2-bit edges, byte offsets, lengths, from/to CSR, vright, inv)
// and the rest of what w2rap_step4_out holds (from_v, to_v, vleft), so that the last pass's graph is downloaded as it stands
struct Graph4 {
    unsigned K = 0; uint64_t E = 0, NV = 0;
    uint64_t ebytes_cap = 0;                 // bytes of `ebits` that may be in use (an upper bound; ebyte[E] is the exact number)
    uint8_t* ebits = nullptr; uint64_t* ebyte = nullptr; uint32_t* elen = nullptr;
    uint64_t* from_off = nullptr; int32_t* from_v = nullptr; int32_t* from_e = nullptr;
    uint64_t* to_off = nullptr; int32_t* to_v = nullptr; int32_t* to_e = nullptr;
    int32_t* vleft = nullptr; int32_t* vright = nullptr; int32_t* inv = nullptr;
};

static_assert(sizeof(int) == sizeof(int32_t), "the host graph's ids (int) are uploaded as int32_t");
struct Task { uint32_t bv; uint32_t role; int32_t edge; uint32_t pad; };     // role 0: in-edge, 1: out-edge, 2: inv[in-edge], 3: inv[out-edge]

constexpr int EDIT4_FALLBACK = -4001;       // a precondition of the device edit does not hold: the caller starts over with the host edit

// ---- who edits the graph: the only part of a pass that differs between the device path and the host path (step4_clean.hip: passes())
struct Editor4 {
    virtual ~Editor4() = default;
    // the branch vertices (an edge in, two or more out) of g in ascending order, their out-degrees, and per vertex its tasks: in-edges,
    // out-edges, inv[in-edges], inv[out-edges], each in list order; device arrays, null when there is no branch vertex
    virtual int tasks(Ctx& c, const Graph4& g, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T) = 0;
    // one pass's edit: min_size, the deleted list, DeleteEdges, RemoveUnneededVertices2 and CleanupCore.
    // in: g, dead[e] from the vote.  out: the next pass's graph (fresh blocks), map[e] / add[e] for the path kernels (ids of g), the sorted
    // deleted list (host vector), the number of new edges.  An editor that edits nothing (VOTE_ONLY) returns g itself and no map.
    // Either function may return EDIT4_FALLBACK, without having changed anything the caller holds.
    virtual int pass(Ctx& c, const Graph4& g, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
                     std::vector<int32_t>* deleted, uint64_t* n_merged) = 0;
};

// ---- the device editor (step4_edit.hip, kernels k4e_*).  Its preconditions: every adjacency list is in ascending order of the neighbour
// vertex (tasks), every merged run's mirror image is a run, and the graph has an edge (pass)
struct DeviceEditor4 : Editor4 {
    int tasks(Ctx& c, const Graph4& g, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T) override;
    int pass(Ctx& c, const Graph4& g, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
             std::vector<int32_t>* deleted, uint64_t* n_merged) override;
};

// ---- the host editor (step4_host.hip): the judge the device editor is tested against, and what a call falls back to
// the graph on the host (digraphE<basevector>: ordered adjacency lists, edge objects as base codes)
struct HostGraph {
    int K = 0;
    std::vector<std::vector<int>> frm, frm_e, to, to_e;
    std::vector<std::vector<uint8_t>> edges;
    int kmers(int e) const { return (int)edges[e].size() - K + 1; }
    void left_right(std::vector<int>& tl, std::vector<int>& tr) const {
        tl.assign(edges.size(), -1); tr.assign(edges.size(), -1);
        for (size_t v = 0; v < frm.size(); ++v) { for (int e : frm_e[v]) tl[e] = (int)v; for (int e : to_e[v]) tr[e] = (int)v; }
    }
    void used(std::vector<char>& u) const { u.assign(edges.size(), 0); for (auto& l : to_e) for (int e : l) u[e] = 1; }
    void add_edge(int v, int w, std::vector<uint8_t>&& seq) {              // DigraphTemplate.h:1829-1839
        const int n = (int)edges.size();
        edges.push_back(std::move(seq));
        const size_t i = std::upper_bound(frm[v].begin(), frm[v].end(), w) - frm[v].begin();
        frm[v].insert(frm[v].begin() + i, w); frm_e[v].insert(frm_e[v].begin() + i, n);
        const size_t j = std::upper_bound(to[w].begin(), to[w].end(), v) - to[w].begin();
        to[w].insert(to[w].begin() + j, v); to_e[w].insert(to_e[w].begin() + j, n);
    }
    void delete_edges(const std::vector<char>& dead) {                     // DigraphTemplate.h:2017-2027: the lists keep their order
        for (size_t v = 0; v < frm.size(); ++v) {
            size_t k = 0;
            for (size_t i = 0; i < frm_e[v].size(); ++i) if (!dead[frm_e[v][i]]) { frm[v][k] = frm[v][i]; frm_e[v][k] = frm_e[v][i]; ++k; }
            frm[v].resize(k); frm_e[v].resize(k);
            k = 0;
            for (size_t i = 0; i < to_e[v].size(); ++i) if (!dead[to_e[v][i]]) { to[v][k] = to[v][i]; to_e[v][k] = to_e[v][i]; ++k; }
            to[v].resize(k); to_e[v].resize(k);
        }
    }
};
struct Csr { std::vector<uint64_t> from_off, to_off; std::vector<int32_t> from_v, from_e, to_v, to_e, vleft, vright; };

// packed 2-bit edge objects -> one base code per byte
void unpack_edges(uint64_t E, const uint8_t* packed, const uint64_t* byte_off, const uint32_t* len, std::vector<std::vector<uint8_t>>& edges);
int host_involution(const HostGraph& g, std::vector<int>& inv, std::string& err);
int edit_graph(HostGraph& g, std::vector<int>& inv, std::vector<char>& dead, unsigned min_size, bool edit, std::vector<int32_t>& deleted,
               std::vector<int32_t>& map, std::vector<int32_t>& add, uint64_t& n_merged, std::string& err);
void pack_edges(const HostGraph& g, std::vector<uint8_t>& packed, std::vector<uint64_t>& boff, std::vector<uint32_t>& len);
void make_csr(const HostGraph& g, Csr& c);
// host arrays of a graph whose K, E, NV and ebytes_cap are set in g -> fresh blocks in g (`ebits` with the 32 bytes of slack that k4_walks
// and k4e_gather read past the last edge); boff / from_off / to_off may be null when the graph has no edge / no vertex
int upload_graph4(Ctx& c, Graph4& g, const uint8_t* packed, const uint64_t* boff, const uint32_t* elen, const uint64_t* from_off, const int32_t* from_v,
                  const int32_t* from_e, const uint64_t* to_off, const int32_t* to_v, const int32_t* to_e, const int32_t* vleft, const int32_t* vright,
                  const int32_t* inv);

// keeps its graph and involution on the host between the passes; every pass's Graph4 is packed and uploaded anew.  Launches no kernel.
// edit == false (VOTE_ONLY): min_size and the deleted list only
struct HostEditor4 : Editor4 {
    HostGraph g; std::vector<int> inv; bool edit = true;
    int tasks(Ctx& c, const Graph4& gd, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T) override;
    int pass(Ctx& c, const Graph4& gd, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
             std::vector<int32_t>* deleted, uint64_t* n_merged) override;
};

}  // namespace w2
