// step4_edit.h -- what step4_clean.hip (the orchestration of Step 4) and step4_edit.hip (the graph edit on the device) share.
#pragma once
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

struct Task { uint32_t bv; uint32_t role; int32_t edge; uint32_t pad; };     // role 0: in-edge, 1: out-edge, 2: inv[in-edge], 3: inv[out-edge]

// the branch vertices (an edge in, two or more out) in ascending order, their out-degrees, and per vertex its tasks: in-edges, out-edges,
// inv[in-edges], inv[out-edges], each in list order.  *sorted = every adjacency list is in ascending order of the neighbour vertex
int edit4_tasks(Ctx& c, const Graph4& g, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T, bool* sorted);

constexpr int EDIT4_FALLBACK = -4001;       // a precondition of the device edit does not hold: the caller runs the host edit instead

// one pass's edit: min_size, the deleted list, DeleteEdges, RemoveUnneededVertices2 and CleanupCore on the device.
// in: g, dead[e] from the vote.  out: the next pass's graph (fresh blocks), map[e] / add[e] for the path kernels (ids of g), the sorted
// deleted list (host vector), the number of new edges.  Returns EDIT4_FALLBACK without having changed anything the caller holds.
int edit4_pass(Ctx& c, const Graph4& g, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
               std::vector<int32_t>* deleted, uint64_t* n_merged);

}  // namespace w2
