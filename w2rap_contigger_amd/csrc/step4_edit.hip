// step4_edit.hip -- Step 4's graph edit on the device: what edit_graph() in step4_host.hip does on the host, statement for statement in
// effect, from one pass's Graph4 to the next one's without the graph leaving HBM.
//
//   k4e_min_size                        Clean200.cc:370-380, one thread per vertex
//   k4e_dead_flags / scan / k4e_dead_list    the sorted deleted list (downloaded as the pass's result only)
//   k4e_kill / scan / k4e_kill_list     surviving degrees, the single surviving in- and out-edge, kill[v]; the kill vertices as a list
//   k4e_rank_init / k4e_rank_step       pointer jumping along pred(v) over the kill vertices: per vertex the head of its run, its distance
//                                       from it, the k-mers in front of its out-edge (= offsets[e]), the largest vertex id seen, circle flag
//   k4e_runs / scan / k4e_records       per run its ends; pushed (eleft < inv[eright]) runs ranked by their largest kill vertex; the record of
//                                       the run's new edge and of its mirror's; the preconditions of the mirror
//   scan / k4e_members / k4e_keys       the member edges of every new edge with their offsets; dead2, renum, offsets
//   sort_pairs_u64 x 2                  the new edges by (from vertex, to vertex, id) and by (to vertex, from vertex, id)
//   k4e_used / scan, k4e_degrees / 3 scans   CleanupCore's to_new and newv, the new CSR offsets
//   k4e_adj                             per vertex: surviving old entries in order, new edges merged in (neighbour, old before new, id)
//   k4e_edge_meta / scan / k4e_gather   lengths, inv, map / add for the path kernels; the packed sequences in new order (threads over
//                                       output words, the source edge of a base by binary search over the run's member offsets)
//   k4e_check_sorted, k4e_branch_flags / 2 scans / k4e_branch_fill     the precondition on the lists; branch vertices, out-degrees, tasks
// Counting is by scan throughout; no kernel shares an atomic cursor.
#include <algorithm>
#include <vector>
#include "step4_edit.h"

namespace w2 {
namespace {

constexpr uint32_t NIL = 0xFFFFFFFFu;

#define RUN4(name, kern, n, ...)                                                                              \
    do {                                                                                                      \
        if (n) LAUNCH(c, name, kern, dim3((unsigned)(((uint64_t)(n) + 255) / 256)), dim3(256), 0, __VA_ARGS__); \
    } while (0)

struct GV {
    unsigned K; uint32_t E, NV;
    const uint32_t* elen; const uint64_t* ebyte; const uint8_t* ebits;
    const uint64_t* from_off; const int32_t* from_e; const uint64_t* to_off; const int32_t* to_e;
    const int32_t* vleft; const int32_t* vright; const int32_t* inv;
};
GV view(const Graph4& g) { return GV{g.K, (uint32_t)g.E, (uint32_t)g.NV, g.elen, g.ebyte, g.ebits, g.from_off, g.from_e, g.to_off, g.to_e, g.vleft, g.vright, g.inv}; }

// ---- preconditions and task lists ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4e_check_sorted(GV g, uint32_t* __restrict__ fail) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    int prev = -1; bool bad = false;
    for (uint64_t i = g.from_off[v]; i < g.from_off[v + 1]; ++i) { const int w = g.vright[g.from_e[i]]; bad |= w < prev; prev = w; }
    prev = -1;
    for (uint64_t i = g.to_off[v]; i < g.to_off[v + 1]; ++i) { const int u = g.vleft[g.to_e[i]]; bad |= u < prev; prev = u; }
    if (bad) *fail = 1u;
}
__global__ __launch_bounds__(256) void k4e_branch_flags(GV g, uint32_t* __restrict__ isb, uint32_t* __restrict__ ntask) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    const uint32_t nin = (uint32_t)(g.to_off[v + 1] - g.to_off[v]), nout = (uint32_t)(g.from_off[v + 1] - g.from_off[v]);
    const bool b = nin > 0 && nout > 1;
    isb[v] = b; ntask[v] = b ? 2 * (nin + nout) : 0u;
}
__global__ __launch_bounds__(256) void k4e_branch_fill(GV g, const uint64_t* __restrict__ bidx, const uint64_t* __restrict__ toff,
                                                       int32_t* __restrict__ bvert, int32_t* __restrict__ outdeg, Task* __restrict__ tasks) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV || bidx[v + 1] == bidx[v]) return;
    const uint32_t b = (uint32_t)bidx[v];
    const uint64_t f0 = g.from_off[v], f1 = g.from_off[v + 1], t0 = g.to_off[v], t1 = g.to_off[v + 1];
    bvert[b] = (int32_t)v; outdeg[b] = (int32_t)(f1 - f0);
    uint64_t t = toff[v];
    for (uint64_t i = t0; i < t1; ++i) tasks[t++] = Task{b, 0u, g.to_e[i], 0u};
    for (uint64_t i = f0; i < f1; ++i) tasks[t++] = Task{b, 1u, g.from_e[i], 0u};
    for (uint64_t i = t0; i < t1; ++i) tasks[t++] = Task{b, 2u, g.inv[g.to_e[i]], 0u};
    for (uint64_t i = f0; i < f1; ++i) tasks[t++] = Task{b, 3u, g.inv[g.from_e[i]], 0u};
}

// ---- min_size, the deleted list ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4e_min_size(GV g, unsigned min_size, uint8_t* __restrict__ dead) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    if (g.to_off[v + 1] != g.to_off[v] || g.from_off[v + 1] - g.from_off[v] != 1) return;
    const int e = g.from_e[g.from_off[v]];
    const int w = g.vright[e];
    if ((uint32_t)w == v || g.to_off[w + 1] - g.to_off[w] != 1 || g.from_off[w + 1] != g.from_off[w]) return;
    if (g.elen[e] - g.K + 1 > min_size) return;
    dead[e] = 1;
}
__global__ __launch_bounds__(256) void k4e_dead_flags(uint32_t E, const uint8_t* __restrict__ dead, uint32_t* __restrict__ f) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e < E) f[e] = dead[e] ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k4e_dead_list(uint32_t E, const uint8_t* __restrict__ dead, const uint64_t* __restrict__ off, int32_t* __restrict__ list) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e < E && dead[e]) list[off[e]] = (int32_t)e;
}

// ---- kill vertices -------------------------------------------------------------------------------------------------------------
// o[v] / in[v]: the surviving out- / in-edge of a vertex that has exactly one; kill[v] as RemoveUnneededVertices2 has it (GapToyTools3.cc:101-107)
__global__ __launch_bounds__(256) void k4e_kill(GV g, const uint8_t* __restrict__ dead, int32_t* __restrict__ o, int32_t* __restrict__ in, uint32_t* __restrict__ kill) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    int no = 0, ni = 0, eo = -1, ei = -1;
    for (uint64_t i = g.from_off[v]; i < g.from_off[v + 1]; ++i) { const int e = g.from_e[i]; if (!dead[e]) { ++no; eo = e; } }
    for (uint64_t i = g.to_off[v]; i < g.to_off[v + 1]; ++i) { const int e = g.to_e[i]; if (!dead[e]) { ++ni; ei = e; } }
    o[v] = eo; in[v] = ei;
    kill[v] = no == 1 && ni == 1 && g.vright[eo] != g.vleft[ei];
}
__global__ __launch_bounds__(256) void k4e_kill_list(uint32_t NV, const uint32_t* __restrict__ kill, const uint64_t* __restrict__ off, uint32_t* __restrict__ list) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < NV && kill[v]) list[off[v]] = v;
}

// ---- runs: pointer jumping towards the head of the chain ---------------------------------------------------------------------
// After enough rounds: nxt == NIL on a chain (head = its first kill vertex, H = kill vertices in front of v, S = k-mers of eleft and of
// the out-edges of those vertices = offsets[o[v]], vm = the largest vertex id from the head to v); nxt != NIL on a circle made of kill
// vertices only (vm = the circle's largest vertex id)
struct Rk { uint32_t nxt, S, H, vm, head; };
__global__ __launch_bounds__(256) void k4e_rank_init(uint32_t NK, const uint32_t* __restrict__ klist, GV g, const int32_t* __restrict__ in, const uint32_t* __restrict__ kill, Rk* __restrict__ rk) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NK) return;
    const uint32_t v = klist[i];
    const int ei = in[v];
    const uint32_t p = (uint32_t)g.vleft[ei];
    const uint32_t nxt = kill[p] ? p : NIL;
    rk[v] = Rk{nxt, g.elen[ei] - g.K + 1, nxt != NIL ? 1u : 0u, v, v};
}
__global__ __launch_bounds__(256) void k4e_rank_step(uint32_t NK, const uint32_t* __restrict__ klist, const Rk* __restrict__ a, Rk* __restrict__ b) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NK) return;
    const uint32_t v = klist[i];
    Rk x = a[v];
    if (x.nxt != NIL) {
        const Rk u = a[x.nxt];
        x.S += u.S; x.H += u.H; x.vm = u.vm > x.vm ? u.vm : x.vm; x.head = u.head; x.nxt = u.nxt;
    }
    b[v] = x;
}

// the last kill vertex of every chain and the largest vertex of every circle: is the run pushed (GapToyTools3.cc:141)?  prim[m] = 1 at
// the run's largest kill vertex m, ptail[m] = the vertex that knows the run
__global__ __launch_bounds__(256) void k4e_runs(uint32_t NK, const uint32_t* __restrict__ klist, GV g, const int32_t* __restrict__ o, const int32_t* __restrict__ in,
                                                const uint32_t* __restrict__ kill, const Rk* __restrict__ rk, uint32_t* __restrict__ tail_of_head,
                                                uint32_t* __restrict__ prim, uint32_t* __restrict__ ptail) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NK) return;
    const uint32_t v = klist[i];
    const Rk a = rk[v];
    if (a.nxt == NIL) {
        if (kill[g.vright[o[v]]]) return;                    // not the last of its chain
        tail_of_head[a.head] = v;
        const int eleft = in[a.head], eright = o[v];
        if (eleft < g.inv[eright]) { prim[a.vm] = 1u; ptail[a.vm] = v; }
    } else if (a.vm == v) {                                  // the walk from the circle's largest vertex ends with (e, e), e its out-edge
        const int e = o[v];
        if (e < g.inv[e]) { prim[v] = 1u; ptail[v] = v; }
    }
}

struct NewEdge { int32_t vL, vR; uint32_t len; int32_t single; };       // single: the one member of a circle's copy, -1 for a chain
// pushed run number k (ascending largest kill vertex): the run itself becomes edge E + 2k + 1, its mirror E + 2k (popped from the back
// of `bound`).  The mirror's precondition: it is a run of this graph with the mirrored ends (a circle's: an edge of a circle)
__global__ __launch_bounds__(256) void k4e_records(uint32_t NK, const uint32_t* __restrict__ klist, GV g, const uint8_t* __restrict__ dead, const int32_t* __restrict__ o,
                                                   const int32_t* __restrict__ in, const uint32_t* __restrict__ kill, const Rk* __restrict__ rk,
                                                   const uint32_t* __restrict__ tail_of_head, const uint32_t* __restrict__ prim, const uint32_t* __restrict__ ptail,
                                                   const uint64_t* __restrict__ pk, NewEdge* __restrict__ ne, uint32_t* __restrict__ nmem, int32_t* __restrict__ run_newid,
                                                   uint8_t* __restrict__ dead2, int32_t* __restrict__ renum, uint32_t* __restrict__ fail) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NK) return;
    const uint32_t m = klist[i];
    if (!prim[m]) return;
    const uint32_t j0 = 2 * (uint32_t)pk[m], j1 = j0 + 1;
    const uint32_t t = ptail[m];
    const Rk a = rk[t];
    if (a.nxt == NIL) {
        const int eleft = in[a.head], eright = o[t];
        ne[j1] = NewEdge{g.vleft[eleft], g.vright[eright], a.S + g.elen[eright], -1};
        nmem[j1] = a.H + 2;
        run_newid[a.head] = (int32_t)(g.E + j1);
        const int f = g.inv[eright], l = g.inv[eleft];
        bool ok = f >= 0 && l >= 0 && !dead[f] && g.inv[f] == eright && g.inv[l] == eleft;
        uint32_t hB = 0, tB = NIL;
        if (ok) { hB = (uint32_t)g.vright[f]; ok = kill[hB] && in[hB] == f; }
        if (ok) { const Rk b = rk[hB]; ok = b.nxt == NIL && b.head == hB && b.H == 0; }
        if (ok) { tB = tail_of_head[hB]; ok = tB != NIL && o[tB] == l; }
        if (!ok) { *fail = 1u; return; }
        const Rk bt = rk[tB];
        ne[j0] = NewEdge{g.vleft[f], g.vright[l], bt.S + g.elen[l], -1};
        nmem[j0] = bt.H + 2;
        run_newid[hB] = (int32_t)(g.E + j0);
    } else {
        const int e = o[m];
        ne[j1] = NewEdge{g.vleft[e], g.vright[e], g.elen[e], e};
        nmem[j1] = 1;
        dead2[e] = 1; renum[e] = (int32_t)(g.E + j1);
        const int f = g.inv[e];
        bool ok = f >= 0 && !dead[f] && g.inv[f] == e;
        if (ok) { const uint32_t x = (uint32_t)g.vleft[f]; ok = kill[x] && o[x] == f && rk[x].nxt != NIL; }
        if (!ok) { *fail = 1u; return; }
        ne[j0] = NewEdge{g.vleft[f], g.vright[f], g.elen[f], f};
        nmem[j0] = 1;
        dead2[f] = 1; renum[f] = (int32_t)(g.E + j0);
    }
}
// every kill vertex of a merged chain: its out-edge (and the head's in-edge, eleft) joins the new edge at offsets[e]
__global__ __launch_bounds__(256) void k4e_members(uint32_t NK, const uint32_t* __restrict__ klist, uint32_t E, const int32_t* __restrict__ o, const int32_t* __restrict__ in,
                                                   const Rk* __restrict__ rk, const int32_t* __restrict__ run_newid, const uint64_t* __restrict__ ms,
                                                   uint8_t* __restrict__ dead2, int32_t* __restrict__ renum, int32_t* __restrict__ offs,
                                                   int32_t* __restrict__ mem_edge, uint32_t* __restrict__ mem_off) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NK) return;
    const uint32_t v = klist[i];
    const Rk a = rk[v];
    if (a.nxt != NIL) return;
    const int32_t id = run_newid[a.head];
    if (id < 0) return;
    const uint64_t base = ms[(uint32_t)id - E];
    const int e = o[v];
    dead2[e] = 1; renum[e] = id; offs[e] = (int32_t)a.S;
    mem_edge[base + a.H + 1] = e; mem_off[base + a.H + 1] = a.S;
    if (a.head == v) {
        const int el = in[v];
        dead2[el] = 1; renum[el] = id; offs[el] = 0;
        mem_edge[base] = el; mem_off[base] = 0;
    }
}
// sort keys of the new edges for the from lists (from vertex, to vertex) and the to lists (to vertex, from vertex); the value is the
// creation order, which a stable sort keeps among equal keys.  A circle's copy has its one member written here
__global__ __launch_bounds__(256) void k4e_keys(uint32_t M, const NewEdge* __restrict__ ne, const uint64_t* __restrict__ ms, uint64_t* __restrict__ kf, uint32_t* __restrict__ vf,
                                                uint64_t* __restrict__ kt, uint32_t* __restrict__ vt, int32_t* __restrict__ mem_edge, uint32_t* __restrict__ mem_off) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const NewEdge x = ne[j];
    kf[j] = (uint64_t)(uint32_t)x.vL << 32 | (uint32_t)x.vR; vf[j] = j;
    kt[j] = (uint64_t)(uint32_t)x.vR << 32 | (uint32_t)x.vL; vt[j] = j;
    if (x.single >= 0) { mem_edge[ms[j]] = x.single; mem_off[ms[j]] = 0; }
}

// ---- CleanupCore -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4e_used(uint32_t E, uint32_t M, const uint8_t* __restrict__ dead, const uint8_t* __restrict__ dead2, uint32_t* __restrict__ used) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < E + M) used[i] = i >= E || (!dead[i] && !dead2[i]);
}
__device__ inline uint32_t lower_bound_hi(const uint64_t* __restrict__ k, uint32_t n, uint32_t v) {        // first entry whose high word is >= v
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)(k[mid] >> 32) < v) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(256) void k4e_degrees(GV g, uint32_t M, const uint32_t* __restrict__ used, const uint64_t* __restrict__ kf, const uint64_t* __restrict__ kt,
                                                   uint32_t* __restrict__ fdeg, uint32_t* __restrict__ tdeg, uint32_t* __restrict__ has) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    uint32_t fd = 0, td = 0;
    for (uint64_t i = g.from_off[v]; i < g.from_off[v + 1]; ++i) fd += used[g.from_e[i]];
    for (uint64_t i = g.to_off[v]; i < g.to_off[v + 1]; ++i) td += used[g.to_e[i]];
    if (M) { fd += lower_bound_hi(kf, M, v + 1) - lower_bound_hi(kf, M, v); td += lower_bound_hi(kt, M, v + 1) - lower_bound_hi(kt, M, v); }
    fdeg[v] = fd; tdeg[v] = td; has[v] = (fd | td) != 0;
}
struct NextDev {
    uint64_t* from_off; int32_t* from_v; int32_t* from_e; uint64_t* to_off; int32_t* to_v; int32_t* to_e; int32_t* vleft; int32_t* vright;
};
// a vertex's final lists: add_edge puts a new edge at upper_bound of its neighbour (DigraphTemplate.h:1829-1839), so with lists sorted by
// neighbour: the surviving old entries in their order, the new edges merged in by (neighbour, old before new, creation order)
__global__ __launch_bounds__(256) void k4e_adj(GV g, uint32_t M, const uint32_t* __restrict__ used, const uint64_t* __restrict__ tn, const uint64_t* __restrict__ nvs,
                                               const uint64_t* __restrict__ fo, const uint64_t* __restrict__ to, const uint64_t* __restrict__ kf, const uint32_t* __restrict__ vf,
                                               const uint64_t* __restrict__ kt, const uint32_t* __restrict__ vt, NextDev n) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= g.NV) return;
    if (v == 0) { n.from_off[nvs[g.NV]] = fo[g.NV]; n.to_off[nvs[g.NV]] = to[g.NV]; }
    if (nvs[v + 1] == nvs[v]) return;
    const int32_t nv = (int32_t)nvs[v];
    n.from_off[nv] = fo[v]; n.to_off[nv] = to[v];
    for (int side = 0; side < 2; ++side) {
        const uint64_t* off = side ? g.to_off : g.from_off;
        const int32_t* le = side ? g.to_e : g.from_e;
        const int32_t* nb = side ? g.vleft : g.vright;          // the neighbour of an old entry
        const uint64_t* ks = side ? kt : kf; const uint32_t* vs = side ? vt : vf;
        uint64_t a = off[v]; const uint64_t a1 = off[v + 1];
        uint32_t b = 0, b1 = 0;
        if (M) { b = lower_bound_hi(ks, M, v); b1 = lower_bound_hi(ks, M, v + 1); }
        uint64_t out = side ? to[v] : fo[v];
        for (;;) {
            while (a < a1 && !used[le[a]]) ++a;
            int32_t w, id;
            if (a < a1 && (b >= b1 || (uint32_t)nb[le[a]] <= (uint32_t)ks[b])) { const int e = le[a++]; w = nb[e]; id = (int32_t)tn[e]; }
            else if (b < b1) { w = (int32_t)(uint32_t)ks[b]; id = (int32_t)tn[g.E + vs[b]]; ++b; }
            else break;
            const int32_t nw = (int32_t)nvs[w];
            if (side) { n.to_v[out] = nw; n.to_e[out] = id; n.vright[id] = nv; }
            else { n.from_v[out] = nw; n.from_e[out] = id; n.vleft[id] = nv; }
            ++out;
        }
    }
}
// per edge object of the edited graph (old ones, then the new ones): length, inv, where its bases come from; per OLD edge what the path
// kernels need: map[e] = to_new[renum[e]] (-1: deleted by the vote or min_size), add[e] = offsets[e]
__global__ __launch_bounds__(256) void k4e_edge_meta(GV g, uint32_t M, const uint32_t* __restrict__ used, const uint64_t* __restrict__ tn, const uint8_t* __restrict__ dead,
                                                     const int32_t* __restrict__ renum, const int32_t* __restrict__ offs, const NewEdge* __restrict__ ne,
                                                     uint32_t* __restrict__ nelen, int32_t* __restrict__ ninv, uint32_t* __restrict__ src, int32_t* __restrict__ map, int32_t* __restrict__ add) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.E + M) return;
    if (i < g.E) {
        const int32_t r = renum[i] < 0 ? (int32_t)i : renum[i];
        map[i] = dead[i] ? -1 : (int32_t)tn[r];
        add[i] = offs[i];
    }
    if (!used[i]) return;
    const uint64_t k = tn[i];
    src[k] = i;
    if (i < g.E) {
        const int x = g.inv[i];
        nelen[k] = g.elen[i]; ninv[k] = x >= 0 && used[x] ? (int32_t)tn[x] : -1;
    } else {
        nelen[k] = ne[i - g.E].len; ninv[k] = (int32_t)tn[g.E + ((i - g.E) ^ 1u)];
    }
}
// four output bytes per thread.  An old edge's bytes are copied (its padding bits cleared); a base of a new edge comes from the last member
// whose offset is not behind it (the host's resize-and-append: each member overwrites the K - 1 bases it shares with the one before)
__global__ __launch_bounds__(256) void k4e_gather(uint64_t nwords, GV g, uint32_t En, const uint64_t* __restrict__ nebyte, const uint32_t* __restrict__ nelen, const uint32_t* __restrict__ src,
                                                  const uint64_t* __restrict__ ms, const int32_t* __restrict__ mem_edge, const uint32_t* __restrict__ mem_off, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nwords) return;
    const uint64_t total = nebyte[En], B0 = 4 * t;
    if (B0 >= total) return;
    uint32_t lo = 0, hi = En;                                  // the edge holding byte B0: the last one that starts at or before it
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (nebyte[mid] <= B0) lo = mid; else hi = mid; }
    uint32_t n = lo, word = 0;
    for (unsigned q = 0; q < 4 && B0 + q < total; ++q) {
        const uint64_t B = B0 + q;
        while (B >= nebyte[n + 1]) ++n;
        const uint32_t s = src[n], len = nelen[n];
        const uint32_t b = (uint32_t)(B - nebyte[n]);
        uint32_t byte = 0;
        if (s < g.E) {
            byte = g.ebits[g.ebyte[s] + b];
            if (len - 4 * b < 4) byte &= (1u << (2 * (len - 4 * b))) - 1u;
        } else {
            const uint64_t m0 = ms[s - g.E], m1 = ms[s - g.E + 1];
            for (unsigned k = 0; k < 4 && 4 * b + k < len; ++k) {
                const uint32_t p = 4 * b + k;
                uint64_t l = m0, h = m1;
                while (h - l > 1) { const uint64_t mid = (l + h) >> 1; if (mem_off[mid] <= p) l = mid; else h = mid; }
                const int me = mem_edge[l];
                byte |= packed_base(g.ebits + g.ebyte[me], p - mem_off[l]) << (2 * k);
            }
        }
        word |= byte << (8 * q);
    }
    out[t] = word;
}

template <class T> void drop(Ctx& c, T*& p) { c.release(p); p = nullptr; }

}  // namespace

int DeviceEditor4::tasks(Ctx& c, const Graph4& g, int32_t** d_bvert, int32_t** d_outdeg, Task** d_tasks, uint64_t* B, uint64_t* T) {
    const uint64_t NV = g.NV;
    *B = *T = 0; *d_bvert = nullptr; *d_outdeg = nullptr; *d_tasks = nullptr;
    if (!NV) return 0;
    const GV G = view(g);
    uint32_t *isb = nullptr, *ntask = nullptr, *fail = nullptr; uint64_t *bidx = nullptr, *toff = nullptr;
    W2_ALLOC(isb, uint32_t, NV + 1); W2_ALLOC(ntask, uint32_t, NV + 1); W2_ALLOC(fail, uint32_t, 1); W2_ALLOC(bidx, uint64_t, NV + 2); W2_ALLOC(toff, uint64_t, NV + 2);
    W2_HIP(hipMemsetAsync(fail, 0, 4, c.stream));
    RUN4("k4e_check_sorted", k4e_check_sorted, NV, G, fail);
    RUN4("k4e_branch_flags", k4e_branch_flags, NV, G, isb, ntask);
    W2_TRY(exclusive_scan_u32_to_u64(c, isb, bidx, NV));
    W2_TRY(exclusive_scan_u32_to_u64(c, ntask, toff, NV));
    uint32_t h_fail = 0;
    W2_HIP(hipMemcpyAsync(B, bidx + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(T, toff + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(&h_fail, fail, 4, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (*B && *B < (1ull << 27)) {
        W2_ALLOC(*d_bvert, int32_t, *B + 1); W2_ALLOC(*d_outdeg, int32_t, *B + 1); W2_ALLOC(*d_tasks, Task, *T + 1);
        RUN4("k4e_branch_fill", k4e_branch_fill, NV, G, (const uint64_t*)bidx, (const uint64_t*)toff, *d_bvert, *d_outdeg, *d_tasks);
    }
    drop(c, isb); drop(c, ntask); drop(c, fail); drop(c, bidx); drop(c, toff);
    return h_fail ? EDIT4_FALLBACK : 0;
}

int DeviceEditor4::pass(Ctx& c, const Graph4& g, uint8_t* d_dead, unsigned min_size, Graph4* next, int32_t** d_map, int32_t** d_add,
                        std::vector<int32_t>* deleted, uint64_t* n_merged) {
    const uint64_t E = g.E, NV = g.NV;
    deleted->clear(); *n_merged = 0;
    if (!E || !NV) return EDIT4_FALLBACK;                      // nothing to run a kernel on: the host edit handles the empty graph
    const GV G = view(g);
    // ---- min_size, the deleted list, kill vertices
    if (min_size > 0) RUN4("k4e_min_size", k4e_min_size, NV, G, min_size, d_dead);
    uint32_t *dflag = nullptr, *kill = nullptr, *klist = nullptr, *fail = nullptr; uint64_t *doff = nullptr, *koff = nullptr; int32_t *dlist = nullptr, *o = nullptr, *in = nullptr;
    W2_ALLOC(dflag, uint32_t, E + 1); W2_ALLOC(doff, uint64_t, E + 2); W2_ALLOC(dlist, int32_t, E + 1);
    W2_ALLOC(kill, uint32_t, NV + 1); W2_ALLOC(koff, uint64_t, NV + 2); W2_ALLOC(klist, uint32_t, NV + 1); W2_ALLOC(o, int32_t, NV + 1); W2_ALLOC(in, int32_t, NV + 1);
    W2_ALLOC(fail, uint32_t, 1);
    W2_HIP(hipMemsetAsync(fail, 0, 4, c.stream));
    RUN4("k4e_dead_flags", k4e_dead_flags, E, (uint32_t)E, (const uint8_t*)d_dead, dflag);
    W2_TRY(exclusive_scan_u32_to_u64(c, dflag, doff, E));
    RUN4("k4e_dead_list", k4e_dead_list, E, (uint32_t)E, (const uint8_t*)d_dead, (const uint64_t*)doff, dlist);
    RUN4("k4e_kill", k4e_kill, NV, G, (const uint8_t*)d_dead, o, in, kill);
    W2_TRY(exclusive_scan_u32_to_u64(c, kill, koff, NV));
    RUN4("k4e_kill_list", k4e_kill_list, NV, (uint32_t)NV, (const uint32_t*)kill, (const uint64_t*)koff, klist);
    uint64_t n_dead = 0, NK = 0;
    W2_HIP(hipMemcpyAsync(&n_dead, doff + E, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(&NK, koff + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    deleted->resize(n_dead);
    if (n_dead) W2_HIP(hipMemcpyAsync(deleted->data(), dlist, n_dead * 4, hipMemcpyDeviceToHost, c.stream));
    // ---- runs
    uint8_t* dead2 = nullptr; int32_t *renum = nullptr, *offs = nullptr;
    W2_ALLOC(dead2, uint8_t, E + 1); W2_ALLOC(renum, int32_t, E + 1); W2_ALLOC(offs, int32_t, E + 1);
    W2_HIP(hipMemsetAsync(dead2, 0, E + 1, c.stream));
    W2_HIP(hipMemsetAsync(renum, 0xFF, (E + 1) * 4, c.stream));
    W2_HIP(hipMemsetAsync(offs, 0, (E + 1) * 4, c.stream));
    uint64_t M = 0;
    NewEdge* ne = nullptr; uint64_t* ms = nullptr; int32_t* mem_edge = nullptr; uint32_t* mem_off = nullptr;
    uint64_t *kf = nullptr, *kt = nullptr; uint32_t *vf = nullptr, *vt = nullptr;
    if (NK) {
        Rk *rk = nullptr, *rk2 = nullptr; uint32_t *tail_of_head = nullptr, *prim = nullptr, *ptail = nullptr; uint64_t* pk = nullptr;
        W2_ALLOC(rk, Rk, NV + 1); W2_ALLOC(rk2, Rk, NV + 1); W2_ALLOC(tail_of_head, uint32_t, NV + 1); W2_ALLOC(prim, uint32_t, NV + 1); W2_ALLOC(ptail, uint32_t, NV + 1);
        W2_ALLOC(pk, uint64_t, NV + 2);
        W2_HIP(hipMemsetAsync(tail_of_head, 0xFF, (NV + 1) * 4, c.stream));
        W2_HIP(hipMemsetAsync(prim, 0, (NV + 1) * 4, c.stream));
        RUN4("k4e_rank_init", k4e_rank_init, NK, (uint32_t)NK, (const uint32_t*)klist, G, (const int32_t*)in, (const uint32_t*)kill, rk);
        for (uint64_t span = 1; span < NK + 1; span <<= 1) {      // after r rounds a vertex has seen 2^r vertices of its run
            RUN4("k4e_rank_step", k4e_rank_step, NK, (uint32_t)NK, (const uint32_t*)klist, (const Rk*)rk, rk2);
            std::swap(rk, rk2);
        }
        RUN4("k4e_runs", k4e_runs, NK, (uint32_t)NK, (const uint32_t*)klist, G, (const int32_t*)o, (const int32_t*)in, (const uint32_t*)kill, (const Rk*)rk, tail_of_head, prim, ptail);
        W2_TRY(exclusive_scan_u32_to_u64(c, prim, pk, NV));
        uint64_t n_pushed = 0;
        W2_HIP(hipMemcpyAsync(&n_pushed, pk + NV, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        M = 2 * n_pushed;
        if (E + M >= (1ull << 31)) { c.err = "more than 2^31 edge objects while merging runs"; return W2RAP_E_LIMIT; }
        if (M) {
            uint32_t* nmem = nullptr; int32_t* run_newid = nullptr;
            W2_ALLOC(ne, NewEdge, M + 1); W2_ALLOC(nmem, uint32_t, M + 1); W2_ALLOC(ms, uint64_t, M + 2); W2_ALLOC(run_newid, int32_t, NV + 1);
            W2_ALLOC(mem_edge, int32_t, NK + M + 1); W2_ALLOC(mem_off, uint32_t, NK + M + 1);
            W2_ALLOC(kf, uint64_t, M + 1); W2_ALLOC(kt, uint64_t, M + 1); W2_ALLOC(vf, uint32_t, M + 1); W2_ALLOC(vt, uint32_t, M + 1);
            W2_HIP(hipMemsetAsync(run_newid, 0xFF, (NV + 1) * 4, c.stream));
            W2_HIP(hipMemsetAsync(nmem, 0, (M + 1) * 4, c.stream));
            W2_HIP(hipMemsetAsync(ne, 0, (M + 1) * sizeof(NewEdge), c.stream));
            RUN4("k4e_records", k4e_records, NK, (uint32_t)NK, (const uint32_t*)klist, G, (const uint8_t*)d_dead, (const int32_t*)o, (const int32_t*)in, (const uint32_t*)kill,
                 (const Rk*)rk, (const uint32_t*)tail_of_head, (const uint32_t*)prim, (const uint32_t*)ptail, (const uint64_t*)pk, ne, nmem, run_newid, dead2, renum, fail);
            // a precondition that does not hold leaves records unwritten: stop before anything is sized by them
            uint32_t h_fail = 0;
            W2_HIP(hipMemcpyAsync(&h_fail, fail, 4, hipMemcpyDeviceToHost, c.stream));
            W2_HIP(hipStreamSynchronize(c.stream));
            if (h_fail) return EDIT4_FALLBACK;
            W2_TRY(exclusive_scan_u32_to_u64(c, nmem, ms, M));
            RUN4("k4e_members", k4e_members, NK, (uint32_t)NK, (const uint32_t*)klist, (uint32_t)E, (const int32_t*)o, (const int32_t*)in, (const Rk*)rk, (const int32_t*)run_newid,
                 (const uint64_t*)ms, dead2, renum, offs, mem_edge, mem_off);
            RUN4("k4e_keys", k4e_keys, M, (uint32_t)M, (const NewEdge*)ne, (const uint64_t*)ms, kf, vf, kt, vt, mem_edge, mem_off);
            W2_TRY(sort_pairs_u64(c, kf, vf, M, 0, 64));
            W2_TRY(sort_pairs_u64(c, kt, vt, M, 0, 64));
        }
    }
    // ---- CleanupCore: to_new over the used edge objects, newv over the vertices that keep an edge
    uint32_t *used = nullptr, *fdeg = nullptr, *tdeg = nullptr, *has = nullptr; uint64_t *tn = nullptr, *fo = nullptr, *to = nullptr, *nvs = nullptr;
    W2_ALLOC(used, uint32_t, E + M + 1); W2_ALLOC(tn, uint64_t, E + M + 2);
    W2_ALLOC(fdeg, uint32_t, NV + 1); W2_ALLOC(tdeg, uint32_t, NV + 1); W2_ALLOC(has, uint32_t, NV + 1);
    W2_ALLOC(fo, uint64_t, NV + 2); W2_ALLOC(to, uint64_t, NV + 2); W2_ALLOC(nvs, uint64_t, NV + 2);
    RUN4("k4e_used", k4e_used, E + M, (uint32_t)E, (uint32_t)M, (const uint8_t*)d_dead, (const uint8_t*)dead2, used);
    W2_TRY(exclusive_scan_u32_to_u64(c, used, tn, E + M));
    RUN4("k4e_degrees", k4e_degrees, NV, G, (uint32_t)M, (const uint32_t*)used, (const uint64_t*)kf, (const uint64_t*)kt, fdeg, tdeg, has);
    W2_TRY(exclusive_scan_u32_to_u64(c, fdeg, fo, NV));
    W2_TRY(exclusive_scan_u32_to_u64(c, tdeg, to, NV));
    W2_TRY(exclusive_scan_u32_to_u64(c, has, nvs, NV));
    uint64_t En = 0, NVn = 0, nf = 0, nt = 0;
    W2_HIP(hipMemcpyAsync(&En, tn + E + M, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(&NVn, nvs + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(&nf, fo + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipMemcpyAsync(&nt, to + NV, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (nf != En || nt != En) { c.err = "device graph edit: the adjacency lists do not hold every edge object once"; return W2RAP_E_GRAPH; }
    // ---- the next pass's graph
    Graph4 n; n.K = g.K; n.E = En; n.NV = NVn; n.ebytes_cap = g.ebytes_cap;      // a merged edge never takes more bytes than its members did
    W2_ALLOC(n.ebits, uint8_t, n.ebytes_cap + 32); W2_ALLOC(n.ebyte, uint64_t, En + 2); W2_ALLOC(n.elen, uint32_t, En + 1);
    W2_ALLOC(n.from_off, uint64_t, NVn + 2); W2_ALLOC(n.from_v, int32_t, En + 1); W2_ALLOC(n.from_e, int32_t, En + 1);
    W2_ALLOC(n.to_off, uint64_t, NVn + 2); W2_ALLOC(n.to_v, int32_t, En + 1); W2_ALLOC(n.to_e, int32_t, En + 1);
    W2_ALLOC(n.vleft, int32_t, En + 1); W2_ALLOC(n.vright, int32_t, En + 1); W2_ALLOC(n.inv, int32_t, En + 1);
    uint32_t* src = nullptr;
    W2_ALLOC(src, uint32_t, En + 1); W2_ALLOC(*d_map, int32_t, E + 1); W2_ALLOC(*d_add, int32_t, E + 1);
    W2_HIP(hipMemsetAsync(n.ebits, 0, n.ebytes_cap + 32, c.stream));
    W2_HIP(hipMemsetAsync(n.from_off, 0, (NVn + 2) * 8, c.stream));
    W2_HIP(hipMemsetAsync(n.to_off, 0, (NVn + 2) * 8, c.stream));
    const NextDev nd{n.from_off, n.from_v, n.from_e, n.to_off, n.to_v, n.to_e, n.vleft, n.vright};
    RUN4("k4e_adj", k4e_adj, NV, G, (uint32_t)M, (const uint32_t*)used, (const uint64_t*)tn, (const uint64_t*)nvs, (const uint64_t*)fo, (const uint64_t*)to,
         (const uint64_t*)kf, (const uint32_t*)vf, (const uint64_t*)kt, (const uint32_t*)vt, nd);
    RUN4("k4e_edge_meta", k4e_edge_meta, E + M, G, (uint32_t)M, (const uint32_t*)used, (const uint64_t*)tn, (const uint8_t*)d_dead, (const int32_t*)renum, (const int32_t*)offs,
         (const NewEdge*)ne, n.elen, n.inv, src, *d_map, *d_add);
    if (En) W2_TRY(exclusive_scan_packed_bytes(c, n.elen, n.ebyte, En));
    else W2_HIP(hipMemsetAsync(n.ebyte, 0, 16, c.stream));
    const uint64_t nwords = (n.ebytes_cap + 3) / 4;
    if (En) RUN4("k4e_gather", k4e_gather, nwords, nwords, G, (uint32_t)En, (const uint64_t*)n.ebyte, (const uint32_t*)n.elen, (const uint32_t*)src, (const uint64_t*)ms,
                 (const int32_t*)mem_edge, (const uint32_t*)mem_off, reinterpret_cast<uint32_t*>(n.ebits));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the deleted list has landed)
    *next = n; *n_merged = M;
    return 0;
}

}  // namespace w2
