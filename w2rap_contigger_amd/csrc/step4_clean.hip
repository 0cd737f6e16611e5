// step4_clean.hip -- Step 4, "Cleaning graph": Clean200x (src/paths/long/large/Clean200.cc:202-389) on the large-K graph.
//
// Per pass (two of them):
//   device  k4_index_count / scan / k4_index_fill    invert(paths): per edge the reads whose path holds it, one listing per occurrence
//   device  k4_walks            GetExtensions (:445-470) for every branch vertex, one wavefront each: <= 10 walks, their bases gathered
//                               into a table [vertex][position][walk] (a byte per base, 16 walks' slots per position = one 16-B load)
//   device  k4_item_count / scan / k4_place_count / scan / k4_place_fill
//                               ONE flat list of placements (vertex, read, start, strand) over all branch vertices (:267-340)
//   device  k4_score            per placement <= 10 running sums over <= 250 + K - 1 positions (:292-309, :341-359) -> (out-edge, margin)
//   device  k4_reduce           the 16 threshold sums per (vertex, out-edge): a segmented reduction per tile of placements
//   device  k4_verdict          AnalyzeScores (:391-443) -> a dead flag per edge object
//   device  k4e_*               the graph edit (step4_edit.hip): min_size (:370-380), DeleteEdges, RemoveUnneededVertices2
//                               (GapToyTools3.cc:87-294), CleanupCore (GapToyTools.cc:417-453); the next pass's graph, branch vertices
//                               and tasks are made on the device, nothing of the graph crosses PCIe between the upload and the download
//   host    edit_graph          the same edit on the host (step4_host.hip): W2RAP_STEP4_EDIT_ON_HOST, and the fallback when a precondition
//                               of the device edit does not hold (adjacency lists not sorted by neighbour, a run whose mirror is not a run)
//   device  k4_path_len / scan / k4_path_write       Cleanup's truncation + both renumberings of the read paths in one go
// Integer arithmetic throughout; the order in which placements are listed does not matter (only sums of margins are used).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>
#include "args.h"
#include "step4_edit.h"
#include "../../include/w2rap_step4.h"

namespace w2 {
namespace {

constexpr int MAX_EXTS = 10, MAX_RL = 250, MAX_DEL = 15, MIN_WIN = 100, MAX_LOSE = 50, MIN_RATIO = 5;
constexpr unsigned WSLOTS = 16;           // table slots per position (walks 0..9 used)
constexpr unsigned NSUM = MAX_EXTS * (MAX_DEL + 1);   // threshold sums per branch vertex: [out-edge][d]

inline unsigned grid4(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

struct Place { uint32_t bv; uint32_t rid; int32_t start; uint32_t rc; };

// ---- paths index ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4_index_count(uint64_t total, const int32_t* __restrict__ pe, uint32_t* __restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) atomicAdd(&cnt[pe[i]], 1u);
}
// one thread per read: its entries in order (the listing order inside an edge does not matter to any sum)
__global__ __launch_bounds__(256) void k4_index_fill(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe,
                                                     const uint64_t* __restrict__ ioff, uint32_t* __restrict__ cursor, uint32_t* __restrict__ list) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    for (uint64_t i = poff[r]; i < poff[r + 1]; ++i) {
        const int32_t e = pe[i];
        list[ioff[e] + atomicAdd(&cursor[e], 1u)] = (uint32_t)r;
    }
}

// ---- walks ---------------------------------------------------------------------------------------------------------------
struct GraphDev {
    unsigned K; uint64_t E, NV;
    const uint32_t* elen; const uint64_t* ebyte; const uint8_t* ebits;
    const uint64_t* from_off; const int32_t* from_e; const uint64_t* to_off; const int32_t* to_e; const int32_t* vright; const int32_t* inv;
};

// bases [from, from + cnt) of edge e -> column `col` of the vertex's table from position `dst`, clipped at Lmax
__device__ inline void put_bases(uint8_t* tab, unsigned col, unsigned dst, const uint8_t* eb, unsigned from, unsigned cnt, unsigned Lmax, unsigned lane) {
    if (dst >= Lmax) return;
    if (cnt > Lmax - dst) cnt = Lmax - dst;
    for (unsigned t = lane; t < cnt; t += 64) tab[(uint64_t)(dst + t) * WSLOTS + col] = (uint8_t)packed_base(eb, from + t);
}

// one wavefront per branch vertex.  State in LDS, written by lane 0, read by all (uniform control flow).
__global__ __launch_bounds__(64) void k4_walks(uint32_t B, const int32_t* __restrict__ bvert, GraphDev g, unsigned Lmax,
                                               uint8_t* __restrict__ tabs, int32_t* __restrict__ nwalks, int32_t* __restrict__ depth_out, uint8_t* __restrict__ ei_out) {
    __shared__ int s_len[MAX_EXTS], s_last[MAX_EXTS], s_ei[MAX_EXTS];
    __shared__ int s_count, s_depth;
    const unsigned b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const int v = bvert[b];
    uint8_t* tab = tabs + (uint64_t)b * Lmax * WSLOTS;
    const int K = (int)g.K;
    const uint64_t f0 = g.from_off[v];
    const int n = (int)(g.from_off[v + 1] - f0);
    if (lane == 0) s_depth = MAX_RL;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        if (lane == 0) s_count = n;
        for (int j = 0; j < n && j < MAX_EXTS; ++j) {
            const int e = g.from_e[f0 + j];
            if (lane == 0) { s_len[j] = (int)g.elen[e] - K + 1; s_last[j] = e; s_ei[j] = j; }
            put_bases(tab, j, 0, g.ebits + g.ebyte[e], 0, g.elen[e], Lmax, lane);
        }
        __syncthreads();
        int i = 0;
        while (i < MAX_EXTS && i < s_count) {
            const int len = s_len[i], depth = s_depth;
            if (len >= depth) { ++i; continue; }
            const int w = g.vright[s_last[i]];
            const uint64_t w0 = g.from_off[w];
            const int deg = (int)(g.from_off[w + 1] - w0);
            if (deg == 0) {
                __syncthreads();
                if (lane == 0) s_depth = len < depth ? len : depth;
                __syncthreads();
                ++i;
                continue;
            }
            const unsigned cur = (unsigned)(len + K - 1);
            const int count0 = s_count, eii = s_ei[i];
            __syncthreads();                                 // everybody has read the state this step is based on
            for (int m = 0; m < deg; ++m) {
                const int e = g.from_e[w0 + m];
                const int col = m == 0 ? i : count0 + m - 1;
                if (col < MAX_EXTS) {
                    if (m) for (unsigned t = lane; t < cur && t < Lmax; t += 64) tab[(uint64_t)t * WSLOTS + col] = tab[(uint64_t)t * WSLOTS + i];
                    put_bases(tab, col, cur, g.ebits + g.ebyte[e], (unsigned)(K - 1), g.elen[e] - (unsigned)(K - 1), Lmax, lane);
                    if (lane == 0) { s_len[col] = len + (int)g.elen[e] - K + 1; s_last[col] = e; s_ei[col] = eii; }
                }
            }
            if (lane == 0) s_count = count0 + deg - 1;
            __syncthreads();
        }
        __syncthreads();
    }
    if (lane == 0) { nwalks[b] = s_count; depth_out[b] = s_depth; }
    if (lane < MAX_EXTS) ei_out[(uint64_t)b * WSLOTS + lane] = lane < (unsigned)s_count ? (uint8_t)s_ei[lane] : (uint8_t)0xFF;
}

// ---- placements ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k4_item_count(uint64_t T, const Task* __restrict__ tasks, const int32_t* __restrict__ nwalks,
                                                     const uint32_t* __restrict__ icnt, uint32_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    out[t] = nwalks[tasks[t].bv] > MAX_EXTS ? 0u : icnt[tasks[t].edge];
}

struct PlaceArgs {
    uint64_t T, n_items; const Task* tasks; const uint64_t* item_off;       // [T+1]
    const uint64_t* ioff; const uint32_t* ilist;
    const int32_t* p_offset; const uint64_t* p_off; const int32_t* p_edges; const int32_t* bvert;
};

// the placements of one item (task, listing k): every j with p[j] == edge, filtered and placed as Clean200.cc:267-340 does
template <bool WRITE>
__device__ inline uint32_t item_places(const PlaceArgs& a, const GraphDev& g, uint64_t item, Place* out) {
    uint64_t lo = 0, hi = a.T;                                // the last task whose first item is <= item
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.item_off[mid] <= item) lo = mid; else hi = mid; }
    const Task t = a.tasks[lo];
    const uint32_t rid = a.ilist[a.ioff[t.edge] + (item - a.item_off[lo])];
    const uint64_t p0 = a.p_off[rid], p1 = a.p_off[rid + 1];
    const int v = a.bvert[t.bv];
    const uint64_t t0 = g.to_off[v], t1 = g.to_off[v + 1];
    int start = a.p_offset[rid];
    uint32_t k = 0;
    for (uint64_t j = p0; j < p1; ++j) {
        const int32_t e = a.p_edges[j];
        const int km = (int)g.elen[e] - (int)g.K + 1;
        if (e == t.edge) {
            bool skip = false;
            if (t.role == 1 && j > p0) { const int32_t q = a.p_edges[j - 1]; for (uint64_t u = t0; u < t1; ++u) skip |= g.to_e[u] == q; }
            if (t.role == 3 && j + 1 < p1) { const int32_t q = a.p_edges[j + 1]; for (uint64_t u = t0; u < t1; ++u) skip |= g.inv[g.to_e[u]] == q; }
            if (!skip) {
                if (WRITE) out[k] = Place{t.bv, rid, (t.role == 0 || t.role == 3) ? start - km : start, t.role >= 2 ? 1u : 0u};
                ++k;
            }
        }
        start -= km;
    }
    return k;
}
__global__ __launch_bounds__(256) void k4_place_count(PlaceArgs a, GraphDev g, uint32_t* __restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_items) cnt[i] = item_places<false>(a, g, i, nullptr);
}
__global__ __launch_bounds__(256) void k4_place_fill(PlaceArgs a, GraphDev g, const uint64_t* __restrict__ poff, Place* __restrict__ places) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_items && poff[i + 1] > poff[i]) item_places<true>(a, g, i, places + poff[i]);
}

// ---- the vote ------------------------------------------------------------------------------------------------------------
struct ReadsDev { const uint8_t* bases; const uint64_t* boff; const uint32_t* len; const uint8_t* quals; const uint64_t* qoff; };

// one thread per placement: q[l] = sum of the qualities where the read differs from walk l; per out-edge the minimum over its walks;
// a strict winner scores the margin.  out: key = vertex * 16 + out-edge, margin (0: no score)
__global__ __launch_bounds__(256) void k4_score(uint64_t NP, const Place* __restrict__ places, ReadsDev R, unsigned K, unsigned Lmax,
                                                const uint8_t* __restrict__ tabs, const int32_t* __restrict__ nwalks, const int32_t* __restrict__ depth,
                                                const uint8_t* __restrict__ ei, const int32_t* __restrict__ outdeg, uint2* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NP) return;
    const Place p = places[i];
    const int N = nwalks[p.bv], n = outdeg[p.bv];
    const int L = depth[p.bv] + (int)K - 1;
    const int rl = (int)R.len[p.rid];
    const uint8_t* rb = R.bases + R.boff[p.rid];
    const uint8_t* rq = R.quals + R.qoff[p.rid];
    const uint4* tab = reinterpret_cast<const uint4*>(tabs + (uint64_t)p.bv * Lmax * WSLOTS);
    int lo, hi;       // positions whose read base exists
    if (!p.rc) { lo = p.start > 0 ? p.start : 0; hi = p.start + rl < L ? p.start + rl : L; }                       // rpos = pos - start
    else { const int a = (int)K - 1 - p.start; lo = a - rl > 0 ? a - rl : 0; hi = a < L ? a : L; }                // rpos = K - 2 - pos - start
    int q[MAX_EXTS];
#pragma unroll
    for (int l = 0; l < MAX_EXTS; ++l) q[l] = 0;
    for (int pos = lo; pos < hi; ++pos) {
        const int rpos = p.rc ? (int)K - 2 - pos - p.start : pos - p.start;
        unsigned base = packed_base(rb, (uint64_t)rpos);
        if (p.rc) base = 3u - base;                          // rbexts[l][s - pos - 1] is the complement of bexts[l][pos]
        const int qual = rq[rpos];
        const uint4 w = tab[pos];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int l = 0; l < MAX_EXTS; ++l) q[l] += ((ws[l >> 2] >> (8 * (l & 3))) & 0xFFu) != base ? qual : 0;
    }
    const uint8_t* e = ei + (uint64_t)p.bv * WSLOTS;
    int qq[MAX_EXTS];
#pragma unroll
    for (int j = 0; j < MAX_EXTS; ++j) qq[j] = 1000000000;
#pragma unroll
    for (int l = 0; l < MAX_EXTS; ++l) {
        const int j = l < N ? (int)e[l] : -1;
#pragma unroll
        for (int jj = 0; jj < MAX_EXTS; ++jj) if (jj == j && q[l] < qq[jj]) qq[jj] = q[l];
    }
    int best = 0x7FFFFFFF, arg = 0;
#pragma unroll
    for (int j = 0; j < MAX_EXTS; ++j) if (j < n && qq[j] < best) { best = qq[j]; arg = j; }
    int second = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < MAX_EXTS; ++j) if (j < n && j != arg && qq[j] < second) second = qq[j];
    out[i] = best < second ? make_uint2(p.bv * WSLOTS + (uint32_t)arg, (uint32_t)(second - best)) : make_uint2(p.bv * WSLOTS, 0u);
}

// tile of 256 consecutive placements (sorted by vertex): thread (out-edge j, threshold d) walks the tile in LDS and adds a vertex's
// partial sum to qsum[vertex][j][d] once per (tile, vertex): different addresses but for a vertex that spans several tiles
__global__ __launch_bounds__(256) void k4_reduce(uint64_t NP, const uint2* __restrict__ sc, unsigned long long* __restrict__ qsum) {
    __shared__ uint2 s[256];
    const uint64_t base = (uint64_t)blockIdx.x * 256;
    const unsigned t = threadIdx.x;
    const unsigned cnt = NP - base < 256 ? (unsigned)(NP - base) : 256u;
    if (t < cnt) s[t] = sc[base + t];
    __syncthreads();
    if (t >= NSUM) return;
    const unsigned j = t >> 4, d = t & 15u;
    unsigned long long acc = 0;
    uint32_t cur = s[0].x / WSLOTS;
    for (unsigned k = 0; k < cnt; ++k) {
        const uint2 x = s[k];
        const uint32_t bv = x.x / WSLOTS;
        if (bv != cur) { if (acc) atomicAdd(&qsum[(uint64_t)cur * NSUM + t], acc); acc = 0; cur = bv; }
        if ((x.x % WSLOTS) == j && x.y > d) acc += x.y;
    }
    if (acc) atomicAdd(&qsum[(uint64_t)cur * NSUM + t], acc);
}

// AnalyzeScores, version 3.  Sorting the sums is not needed: with top = the largest sum, the first r that passes deletes exactly the
// out-edges whose sum is <= max_lose and <= top / min_ratio (sums sorted descending: whoever follows a passing rank passes too).
__global__ __launch_bounds__(256) void k4_verdict(uint32_t B, const int32_t* __restrict__ bvert, GraphDev g, const int32_t* __restrict__ nwalks,
                                                  const unsigned long long* __restrict__ qsum, uint8_t* __restrict__ dead) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || nwalks[b] > MAX_EXTS) return;
    const int v = bvert[b];
    const uint64_t f0 = g.from_off[v];
    const int n = (int)(g.from_off[v + 1] - f0);
    const unsigned long long* qs = qsum + (uint64_t)b * NSUM;
    for (int d = 0; d <= MAX_DEL; ++d) {
        unsigned long long top = 0;
        for (int j = 0; j < n; ++j) top = qs[j * 16 + d] > top ? qs[j * 16 + d] : top;
        if (top < (unsigned long long)MIN_WIN) continue;
        bool any = false;
        for (int j = 0; j < n; ++j) {
            const unsigned long long x = qs[j * 16 + d];
            if (x <= (unsigned long long)MAX_LOSE && top >= (unsigned long long)MIN_RATIO * x) {
                const int e = g.from_e[f0 + j];
                dead[e] = 1; dead[g.inv[e]] = 1;
                any = true;
            }
        }
        if (any) break;
    }
}

// ---- read paths: Cleanup's truncation, RemoveUnneededVertices2's renumbering (first entry moves the offset, repeated ids collapse) and
// CleanupCore's renumbering at once.  map[e] = the edge's final id, or -1 for an edge object the pass deleted; add[e] = offsets[e]
__global__ __launch_bounds__(256) void k4_path_len(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe,
                                                   const int32_t* __restrict__ map, uint32_t* __restrict__ nlen) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    uint32_t k = 0; int32_t last = -1;
    for (uint64_t i = poff[r]; i < poff[r + 1]; ++i) {
        const int32_t m = map[pe[i]];
        if (m < 0) break;
        if (k == 0 || m != last) { ++k; last = m; }
    }
    nlen[r] = k;
}
__global__ __launch_bounds__(256) void k4_path_write(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ offs,
                                                     const int32_t* __restrict__ map, const int32_t* __restrict__ add, const uint64_t* __restrict__ noff,
                                                     int32_t* __restrict__ npe, int32_t* __restrict__ noffs) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    uint64_t o = noff[r]; const uint64_t o0 = o; int32_t last = -1;
    int32_t off = offs[r];
    for (uint64_t i = poff[r]; i < poff[r + 1]; ++i) {
        const int32_t m = map[pe[i]];
        if (m < 0) break;
        if (o == o0) off += add[pe[i]];
        if (o == o0 || m != last) { npe[o++] = m; last = m; }
    }
    noffs[r] = off;
}

std::string g_profile4;

// per-kernel times of this run and which editor ran -> w2rap_step4_profile
void save_profile4(Ctx& c, bool on_device) {
    g_profile4 = profile_text(c) + (on_device ? "edit_path_device 1 2\n" : "edit_path_device 0 0\n");
}

struct Ms { float index = 0, vote = 0, paths = 0, host = 0; };
struct PathsDev { uint64_t n = 0, npe = 0; int32_t* offset = nullptr; uint64_t* off = nullptr; int32_t* edges = nullptr; };

// one pass's paths index and vote: d_dead[e] (zeroed by the caller) is set for the edge objects the vote deletes
int vote_pass(Ctx& c, const GraphDev& G, uint64_t B, uint64_t T, const int32_t* d_bvert, const int32_t* d_outdeg, const Task* d_tasks, const ReadsDev& R,
              const PathsDev& P, unsigned Lmax, uint8_t* d_dead, Ms& ms, w2rap_step4_out& out) {
    const uint64_t E = G.E, n = P.n, npe = P.npe;
    const unsigned K = G.K;
    uint64_t n_places = 0;
    // ---- paths index
    uint32_t *d_icnt = nullptr, *d_cursor = nullptr, *d_ilist = nullptr; uint64_t* d_ioff = nullptr;
    {
        Timer t(c.stream);
        W2_ALLOC(d_icnt, uint32_t, E + 1); W2_ALLOC(d_cursor, uint32_t, E + 1); W2_ALLOC(d_ioff, uint64_t, E + 2); W2_ALLOC(d_ilist, uint32_t, npe + 1);
        W2_HIP(hipMemsetAsync(d_icnt, 0, (E + 1) * 4, c.stream));
        W2_HIP(hipMemsetAsync(d_cursor, 0, (E + 1) * 4, c.stream));
        if (npe) LAUNCH(c, "k4_index_count", k4_index_count, dim3(grid4(npe)), dim3(256), 0, npe, (const int32_t*)P.edges, d_icnt);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_icnt, d_ioff, E));
        if (npe) LAUNCH(c, "k4_index_fill", k4_index_fill, dim3(grid4(n)), dim3(256), 0, n, (const uint64_t*)P.off, (const int32_t*)P.edges, (const uint64_t*)d_ioff, d_cursor, d_ilist);
        ms.index = t.stop();
    }
    // ---- the vote
    Timer tv(c.stream);
    uint8_t *d_tabs = nullptr, *d_ei = nullptr; int32_t *d_nwalks = nullptr, *d_depth = nullptr;
    W2_ALLOC(d_tabs, uint8_t, B * (uint64_t)Lmax * WSLOTS + 16); W2_ALLOC(d_ei, uint8_t, B * WSLOTS); W2_ALLOC(d_nwalks, int32_t, B); W2_ALLOC(d_depth, int32_t, B);
    W2_HIP(hipMemsetAsync(d_tabs, 0, B * (uint64_t)Lmax * WSLOTS + 16, c.stream));
    W2_HIP(hipMemsetAsync(d_ei, 0xFF, B * WSLOTS, c.stream));
    LAUNCH(c, "k4_walks", k4_walks, dim3((unsigned)B), dim3(64), 0, (uint32_t)B, d_bvert, G, Lmax, d_tabs, d_nwalks, d_depth, d_ei);
    uint32_t* d_tcnt = nullptr; uint64_t* d_toff = nullptr;
    W2_ALLOC(d_tcnt, uint32_t, T + 1); W2_ALLOC(d_toff, uint64_t, T + 2);
    LAUNCH(c, "k4_item_count", k4_item_count, dim3(grid4(T)), dim3(256), 0, T, d_tasks, (const int32_t*)d_nwalks, (const uint32_t*)d_icnt, d_tcnt);
    W2_TRY(exclusive_scan_u32_to_u64(c, d_tcnt, d_toff, T));
    uint64_t n_items = 0;
    W2_HIP(hipMemcpyAsync(&n_items, d_toff + T, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (n_items >= (1ull << 32) * 200) { c.err = "too many (vertex, read) pairs for one vote"; return W2RAP_E_LIMIT; }
    if (n_items) {
        uint32_t* d_pcnt = nullptr; uint64_t* d_poff = nullptr;
        W2_ALLOC(d_pcnt, uint32_t, n_items + 1); W2_ALLOC(d_poff, uint64_t, n_items + 2);
        const PlaceArgs A{T, n_items, d_tasks, d_toff, d_ioff, d_ilist, P.offset, P.off, P.edges, d_bvert};
        LAUNCH(c, "k4_place_count", k4_place_count, dim3(grid4(n_items)), dim3(256), 0, A, G, d_pcnt);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_pcnt, d_poff, n_items));
        W2_HIP(hipMemcpyAsync(&n_places, d_poff + n_items, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        if (n_places) {
            Place* d_places = nullptr; uint2* d_sc = nullptr; unsigned long long* d_qsum = nullptr;
            W2_ALLOC(d_places, Place, n_places); W2_ALLOC(d_sc, uint2, n_places); W2_ALLOC(d_qsum, unsigned long long, B * NSUM);
            W2_HIP(hipMemsetAsync(d_qsum, 0, B * NSUM * 8, c.stream));
            LAUNCH(c, "k4_place_fill", k4_place_fill, dim3(grid4(n_items)), dim3(256), 0, A, G, (const uint64_t*)d_poff, d_places);
            LAUNCH(c, "k4_score", k4_score, dim3(grid4(n_places)), dim3(256), 0, n_places, (const Place*)d_places, R, K, Lmax, (const uint8_t*)d_tabs,
                   (const int32_t*)d_nwalks, (const int32_t*)d_depth, (const uint8_t*)d_ei, d_outdeg, d_sc);
            LAUNCH(c, "k4_reduce", k4_reduce, dim3(grid4(n_places)), dim3(256), 0, n_places, (const uint2*)d_sc, d_qsum);
            LAUNCH(c, "k4_verdict", k4_verdict, dim3(grid4(B)), dim3(256), 0, (uint32_t)B, d_bvert, G, (const int32_t*)d_nwalks,
                   (const unsigned long long*)d_qsum, d_dead);
        }
    }
    std::vector<int32_t> nw(B);
    W2_HIP(hipMemcpyAsync(nw.data(), d_nwalks, B * 4, hipMemcpyDeviceToHost, c.stream));
    ms.vote = tv.stop();
    W2_HIP(hipStreamSynchronize(c.stream));
    for (int32_t x : nw) if (x > MAX_EXTS) ++out.n_skipped_too_many_exts;
    out.n_placements += n_places;
    return 0;
}

// the read paths of one pass through map[] / add[] (ids of that pass's input graph): fresh blocks in `np`
int rewrite_paths(Ctx& c, const PathsDev& P, const int32_t* d_map, const int32_t* d_add, Ms& ms, PathsDev& np) {
    const uint64_t n = P.n;
    Timer t(c.stream);
    uint32_t* d_nlen = nullptr;
    np = PathsDev{}; np.n = n;
    W2_ALLOC(d_nlen, uint32_t, n + 1); W2_ALLOC(np.off, uint64_t, n + 2); W2_ALLOC(np.offset, int32_t, n + 1); W2_ALLOC(np.edges, int32_t, P.npe + 1);
    LAUNCH(c, "k4_path_len", k4_path_len, dim3(grid4(n)), dim3(256), 0, n, (const uint64_t*)P.off, (const int32_t*)P.edges, d_map, d_nlen);
    W2_TRY(exclusive_scan_u32_to_u64(c, d_nlen, np.off, n));
    LAUNCH(c, "k4_path_write", k4_path_write, dim3(grid4(n)), dim3(256), 0, n, (const uint64_t*)P.off, (const int32_t*)P.edges, (const int32_t*)P.offset,
           d_map, d_add, (const uint64_t*)np.off, np.edges, np.offset);
    W2_HIP(hipMemcpyAsync(&np.npe, np.off + n, 8, hipMemcpyDeviceToHost, c.stream));
    ms.paths = t.stop();
    W2_HIP(hipStreamSynchronize(c.stream));
    return 0;
}

// ---- the driver: upload, two passes on device-resident data, download.  The editor is the only part that differs between the device
// path and the host path (W2RAP_STEP4_EDIT_ON_HOST, VOTE_ONLY, and what a call goes on with after EDIT4_FALLBACK)
// the host editor's graph and involution from host arrays: the host half of both entries (upload() for w2rap_step4_run, host_graph_of()
// for w2rap_step2_run_step4_after_step3).  Edges already unpacked into ed.g.edges (upload() needs them for the involution) are taken as they are
void host_graph(HostEditor4& ed, int K, uint64_t E, uint64_t NV, const uint8_t* packed, const uint64_t* boff, const uint32_t* elen, const uint64_t* from_off,
                const int32_t* from_v, const int32_t* from_e, const uint64_t* to_off, const int32_t* to_v, const int32_t* to_e, const int32_t* inv) {
    HostGraph& hg = ed.g;
    hg.K = K;
    if (hg.edges.size() != E) unpack_edges(E, packed, boff, elen, hg.edges);
    hg.frm.assign(NV, {}); hg.frm_e.assign(NV, {}); hg.to.assign(NV, {}); hg.to_e.assign(NV, {});
    for (uint64_t v = 0; v < NV; ++v) {
        for (uint64_t i = from_off[v]; i < from_off[v + 1]; ++i) { hg.frm[v].push_back(from_v[i]); hg.frm_e[v].push_back(from_e[i]); }
        for (uint64_t i = to_off[v]; i < to_off[v + 1]; ++i) { hg.to[v].push_back(to_v[i]); hg.to_e[v].push_back(to_e[i]); }
    }
    ed.inv.assign(inv, inv + E);
}

// the one reader of `in`: its graph (with both ends of every edge and the involution, computed here if the caller gave none), reads and
// paths on the device; host != null: the same graph as the host editor keeps it
int upload(Ctx& c, const w2rap_step4_in& in, Graph4& g, ReadsDev& R, PathsDev& P, HostEditor4* host) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices;
    HostGraph tmp; HostGraph& hg = host ? host->g : tmp;        // the edges a byte per base: for the host editor, and for the involution
    hg.K = in.K;
    std::vector<int> inv;
    if (!in.inv) { unpack_edges(E, in.edge_packed, in.edge_byte_off, in.edge_len, hg.edges); W2_TRY(host_involution(hg, inv, c.err)); }
    std::vector<int32_t> vleft, vright, to_v(E, -1);
    args::edge_ends(in, vleft, vright);
    for (uint64_t i = 0; i < E; ++i) to_v[i] = vleft[in.to_e[i]];
    g = Graph4{}; g.K = (unsigned)in.K; g.E = E; g.NV = NV; g.ebytes_cap = E ? in.edge_byte_off[E] : 0;
    W2_TRY(upload_graph4(c, g, in.edge_packed, in.edge_byte_off, in.edge_len, in.from_off, in.from_v, in.from_e, in.to_off, to_v.data(), in.to_e,
                         vleft.data(), vright.data(), in.inv ? in.inv : inv.data()));
    if (host) host_graph(*host, in.K, E, NV, in.edge_packed, in.edge_byte_off, in.edge_len, in.from_off, in.from_v, in.from_e, in.to_off, to_v.data(), in.to_e,
                         in.inv ? in.inv : inv.data());
    // ---- the reads and their paths.  (The 16 bytes of slack behind the bases and the qualities are a margin, not a need: k4_score reads both
    // a byte at a time and only at positions inside the read, so the chained entry may hand it the context's read blocks whatever lies behind them)
    const uint64_t n = in.n_paths;
    uint8_t* b = nullptr; uint64_t* bo = nullptr; uint32_t* ln = nullptr; uint8_t* q = nullptr; uint64_t* qo = nullptr;
    W2_TRY(up_pooled(c, &b, in.read_packed, n ? in.read_byte_off[n] : 0, 16));
    W2_TRY(up_pooled(c, &bo, in.read_byte_off, in.read_byte_off ? n + 1 : 0));
    W2_TRY(up_pooled(c, &ln, in.read_len, n));
    W2_TRY(up_pooled(c, &q, in.quals, n ? in.qual_off[n] : 0, 16));
    W2_TRY(up_pooled(c, &qo, in.qual_off, in.qual_off ? n + 1 : 0));
    R = ReadsDev{b, bo, ln, q, qo};
    P.n = n; P.npe = n ? in.path_off[n] : 0;
    W2_TRY(up_pooled(c, &P.offset, in.path_offset, n));
    W2_TRY(up_pooled(c, &P.off, in.path_off, in.path_off ? n + 1 : 0));
    W2_TRY(up_pooled(c, &P.edges, in.path_edges, P.npe));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the host vectors above have been read)
    return 0;
}

// the host editor's graph from ONE download of a graph that lies on the device (the chained entry: EDIT_ON_HOST, VOTE_ONLY, and where it
// goes on after EDIT4_FALLBACK)
int host_graph_of(Ctx& c, const Graph4& g, HostEditor4& ed) {
    const uint64_t E = g.E, NV = g.NV;
    std::vector<uint64_t> boff(E + 1, 0), from_off(NV + 1, 0), to_off(NV + 1, 0);
    std::vector<uint32_t> elen(E);
    std::vector<int32_t> from_v(E), from_e(E), to_v(E), to_e(E), inv(E);
    auto down = [&](void* hst, const void* dev, uint64_t bytes) { return bytes ? hipMemcpyAsync(hst, dev, bytes, hipMemcpyDeviceToHost, c.stream) : hipSuccess; };
    W2_HIP(down(boff.data(), g.ebyte, (E + 1) * 8)); W2_HIP(down(elen.data(), g.elen, E * 4));
    W2_HIP(down(from_off.data(), g.from_off, (NV + 1) * 8)); W2_HIP(down(from_v.data(), g.from_v, E * 4)); W2_HIP(down(from_e.data(), g.from_e, E * 4));
    W2_HIP(down(to_off.data(), g.to_off, (NV + 1) * 8)); W2_HIP(down(to_v.data(), g.to_v, E * 4)); W2_HIP(down(to_e.data(), g.to_e, E * 4));
    W2_HIP(down(inv.data(), g.inv, E * 4));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (boff[E] > g.ebytes_cap) { c.err = "the edge bytes on the device exceed their block"; return W2RAP_E_GRAPH; }
    std::vector<uint8_t> packed(boff[E]);
    W2_HIP(down(packed.data(), g.ebits, boff[E]));
    W2_HIP(hipStreamSynchronize(c.stream));
    ed.g = HostGraph{};
    host_graph(ed, (int)g.K, E, NV, packed.data(), boff.data(), elen.data(), from_off.data(), from_v.data(), from_e.data(), to_off.data(), to_v.data(), to_e.data(),
               inv.data());
    return 0;
}

std::vector<void*> blocks(const Graph4& g) {
    return {g.ebits, g.ebyte, g.elen, g.from_off, g.from_v, g.from_e, g.to_off, g.to_v, g.to_e, g.vleft, g.vright, g.inv};
}

// the end of a pass that began with c.owned == before: every block allocated since goes back to the pool unless it is in `keep`, and so
// does every block in `gone` (the pass's inputs) that is not in `keep` as well (an editor that edits nothing hands its input on)
void retire(Ctx& c, const std::vector<void*>& before, const std::vector<void*>& gone, const std::vector<void*>& keep) {
    auto has = [](const std::vector<void*>& v, void* p) { return std::find(v.begin(), v.end(), p) != v.end(); };
    std::vector<void*> owned;
    for (void* p : c.owned) {
        if (has(keep, p) || (has(before, p) && !has(gone, p))) owned.push_back(p); else c.park(p);
    }
    c.owned.swap(owned);
}

// Clean200x's passes on device-resident data: g and pd are replaced by the clean graph and the paths on it, still on the device.
// Of `out` only the counters are touched (n_branch_vertices, n_runs_merged, and what vote_pass counts).
// at != null (the chained entry, whose input is gone once pass 1 has retired it): the passes start at *at, and when the editor answers
// EDIT4_FALLBACK, *at is the pass it did so in, with g, pd, the counters and the pool as they were when that pass began -- the caller
// goes on from there with the host editor.  at == null: all passes, EDIT4_FALLBACK leaves everything to the caller (who starts over)
int passes(Ctx& c, Graph4& g, const ReadsDev& R, PathsDev& pd, const w2rap_step4_params& P, Editor4& ed, std::vector<int32_t> deleted[2], Ms ms[2],
           w2rap_step4_out& out, int* at = nullptr) {
    const unsigned Lmax = (MAX_RL + g.K - 1 + 3) & ~3u;
    for (int pass = at ? *at : 0; pass < ((P.flags & W2RAP_STEP4_VOTE_ONLY) ? 1 : 2); ++pass) {
        const std::vector<void*> before = c.owned;
        const uint64_t counted[3] = {out.n_branch_vertices, out.n_skipped_too_many_exts, out.n_placements};
        auto one = [&]() -> int {
            int32_t *d_bvert = nullptr, *d_outdeg = nullptr; Task* d_tasks = nullptr;
            uint64_t B = 0, T = 0;
            W2_TRY(ed.tasks(c, g, &d_bvert, &d_outdeg, &d_tasks, &B, &T));
            if (B >= (1ull << 27)) { c.err = "more than 2^27 branch vertices"; return W2RAP_E_LIMIT; }
            out.n_branch_vertices += B;
            uint8_t* d_dead = nullptr;
            W2_ALLOC(d_dead, uint8_t, g.E + 1);
            W2_HIP(hipMemsetAsync(d_dead, 0, g.E + 1, c.stream));
            if (B) {
                const GraphDev G{g.K, g.E, g.NV, g.elen, g.ebyte, g.ebits, g.from_off, g.from_e, g.to_off, g.to_e, g.vright, g.inv};
                W2_TRY(vote_pass(c, G, B, T, d_bvert, d_outdeg, d_tasks, R, pd, Lmax, d_dead, ms[pass], out));
            }
            // ---- the graph edit
            Graph4 next;
            int32_t *d_map = nullptr, *d_add = nullptr;
            uint64_t merged = 0;
            {
                const auto t0 = std::chrono::steady_clock::now();
                W2_TRY(ed.pass(c, g, d_dead, P.min_size, &next, &d_map, &d_add, &deleted[pass], &merged));
                ms[pass].host = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            out.n_runs_merged[pass] = merged;
            // ---- the read paths (no map: nothing was edited)
            std::vector<void*> gone = blocks(g), keep = blocks(next);
            if (d_map && pd.n) {
                PathsDev np;
                W2_TRY(rewrite_paths(c, pd, d_map, d_add, ms[pass], np));
                gone.insert(gone.end(), {(void*)pd.offset, (void*)pd.off, (void*)pd.edges});
                keep.insert(keep.end(), {(void*)np.offset, (void*)np.off, (void*)np.edges});
                pd = np;
            }
            W2_HIP(hipStreamSynchronize(c.stream));
            g = next;
            // the new graph and paths replace the old ones; everything else of this pass goes back to the pool
            retire(c, before, gone, keep);
            return 0;
        };
        const int rc = one();
        if (rc == EDIT4_FALLBACK && at) {                        // (the editors answer it before they have changed g or pd)
            W2_HIP(hipStreamSynchronize(c.stream));
            out.n_branch_vertices = counted[0]; out.n_skipped_too_many_exts = counted[1]; out.n_placements = counted[2];
            deleted[pass].clear(); ms[pass] = Ms{};
            retire(c, before, {}, {});
            *at = pass;
        }
        if (rc) return rc;
    }
    return 0;
}

// the one download of the graph and the paths
int download(Ctx& c, const Graph4& g, const PathsDev& pd, const std::vector<int32_t> deleted[2], const Ms ms[2], w2rap_step4_out& out) {
    const uint64_t E = g.E, NV = g.NV;
    out.K = (int32_t)g.K;
    out.n_vertices = NV; out.n_edge_objs = E;
    W2_TRY(dl(c, &out.edge_byte_off, (const uint64_t*)g.ebyte, E + 1));
    W2_TRY(dl(c, &out.edge_len, (const uint32_t*)g.elen, E));
    W2_TRY(dl(c, &out.vleft, (const int32_t*)g.vleft, E)); W2_TRY(dl(c, &out.vright, (const int32_t*)g.vright, E));
    W2_TRY(dl(c, &out.from_off, (const uint64_t*)g.from_off, NV + 1)); W2_TRY(dl(c, &out.from_v, (const int32_t*)g.from_v, E)); W2_TRY(dl(c, &out.from_e, (const int32_t*)g.from_e, E));
    W2_TRY(dl(c, &out.to_off, (const uint64_t*)g.to_off, NV + 1)); W2_TRY(dl(c, &out.to_v, (const int32_t*)g.to_v, E)); W2_TRY(dl(c, &out.to_e, (const int32_t*)g.to_e, E));
    W2_TRY(dl(c, &out.inv, (const int32_t*)g.inv, E));
    W2_HIP(hipStreamSynchronize(c.stream));
    W2_TRY(dl(c, &out.edge_packed, (const uint8_t*)g.ebits, out.edge_byte_off[E]));
    for (int k = 0; k < 2; ++k) {
        out.n_deleted[k] = deleted[k].size(); out.deleted[k] = host_dup(deleted[k].data(), deleted[k].size());
        out.ms_index[k] = ms[k].index; out.ms_vote[k] = ms[k].vote; out.ms_paths[k] = ms[k].paths; out.ms_graph_edit_host[k] = ms[k].host;
    }
    out.n_paths = pd.n;
    W2_TRY(dl(c, &out.path_offset, (const int32_t*)pd.offset, pd.n));
    if (pd.n) { W2_TRY(dl(c, &out.path_off, (const uint64_t*)pd.off, pd.n + 1)); }
    else { out.path_off = (uint64_t*)host_result_alloc(8); if (out.path_off) out.path_off[0] = 0; }
    W2_TRY(dl(c, &out.path_edges, (const int32_t*)pd.edges, pd.npe));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (!out.edge_packed || !out.path_off || !out.inv) { c.err = "out of host memory"; return W2RAP_E_HIP; }
    return 0;
}

// Step 4 with the graph edit on the device or on the host.  EDIT4_FALLBACK (device only): a precondition of the device edit does not hold,
// nothing of `out` is to be used
int step4(Ctx& c, const w2rap_step4_in& in, const w2rap_step4_params& P, bool on_device, w2rap_step4_out& out) {
    Graph4 g; ReadsDev R{}; PathsDev pd;
    std::vector<int32_t> deleted[2];
    Ms ms[2];
    if (on_device) {
        DeviceEditor4 ed;
        W2_TRY(upload(c, in, g, R, pd, nullptr));
        W2_TRY(passes(c, g, R, pd, P, ed, deleted, ms, out));
    } else {
        HostEditor4 ed;
        ed.edit = !(P.flags & W2RAP_STEP4_VOTE_ONLY);
        W2_TRY(upload(c, in, g, R, pd, &ed));
        W2_TRY(passes(c, g, R, pd, P, ed, deleted, ms, out));
    }
    return download(c, g, pd, deleted, ms, out);
}

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" {

int w2rap_step4_run(const w2rap_step4_in* in, const w2rap_step4_params* P, w2rap_step4_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!in || !P || !out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640] (the reference runs Step 4 at the large K, 200 by default)");
    if (P->flags & ~(W2RAP_STEP4_VOTE_ONLY | W2RAP_STEP4_EDIT_ON_HOST)) return fail(W2RAP_E_ARG, "unknown flag");
    const uint64_t E = in->n_edge_objs;
    if (args::too_large(*in, args::READS_END)) return fail(W2RAP_E_LIMIT, args::TOO_LARGE);
    if (in->n_reads != in->n_paths) return fail(W2RAP_E_ARG, "n_reads differs from n_paths: Step 4 needs the bases and qualities of every pathed read");
    W2_ARGS(args::null_arrays(*in));
    W2_ARGS(args::edge_off_start(*in));
    W2_ARGS(args::edge_lens(*in));
    W2_ARGS(args::adjacency(*in));
    W2_ARGS(args::from_v_agrees(*in));
    if (in->inv) for (uint64_t e = 0; e < E; ++e) {
        if (in->inv[e] < 0 || (uint64_t)in->inv[e] >= E || in->inv[in->inv[e]] != (int32_t)e) return fail(W2RAP_E_ARG, "inv is not an involution of the edge objects");
        if (in->edge_len[in->inv[e]] != in->edge_len[e]) return fail(W2RAP_E_ARG, "inv pairs edge objects of different lengths");
    }
    W2_ARGS(args::reads_and_paths(*in));
    // VOTE_ONLY edits nothing, on either path
    bool on_device = !(P->flags & (W2RAP_STEP4_EDIT_ON_HOST | W2RAP_STEP4_VOTE_ONLY));
    auto body = [&](Ctx& c) -> int {
        int rc = step4(c, *in, *P, on_device, *out);
        if (rc == EDIT4_FALLBACK) {                              // start over with the host edit: same result, nothing kept from this attempt
            on_device = false;
            (void)hipStreamSynchronize(c.stream);
            c.presolve();
            c.prof_sums.clear();
            c.free_all();
            c.err.clear();
            w2rap_step4_free(out);
            rc = step4(c, *in, *P, false, *out);
        }
        return rc;
    };
    return one_shot(P->device, err, errlen, body, [&](Ctx& c) { save_profile4(c, on_device); }, [&] { w2rap_step4_free(out); });
}

// Step 4 straight behind Step 3 in one process (the reference's default flow, w2rap-contigger.cc:395-399 on the objects Steps 1-3 left in
// memory): the large-K graph, its involution and the read paths are the context's kept large-K result (W2RAP_STEP3_KEEP_DEVICE), the reads
// and their qualities are the context's own.  Nothing goes up; the clean graph and paths come down once.  The context's Step-2 state is
// not touched, whatever happens
int w2rap_step2_run_step4_after_step3(w2rap_step2_ctx* h, const w2rap_step4_params* P, w2rap_step4_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!h || !P || !out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (P->flags & ~(W2RAP_STEP4_VOTE_ONLY | W2RAP_STEP4_EDIT_ON_HOST)) return fail(W2RAP_E_ARG, "unknown flag");
    Ctx& c = h->c;
    if (P->device != c.device) return fail(W2RAP_E_ARG, "w2rap_step2_run_step4_after_step3: params->device is not the context's device");
    if (!c.kept.valid)
        return fail(W2RAP_E_STATE, "w2rap_step2_run_step4_after_step3: the context holds no large-K result of Step 3 (w2rap_step3_run_after_step2 with "
                                   "W2RAP_STEP3_KEEP_DEVICE comes first; a full Step 4, or anything that changes Step 2's state, gives the result up)");
    if (hipSetDevice(c.device) != hipSuccess) return fail(W2RAP_E_HIP, "hipSetDevice failed");
    const Ctx::Kept3 k = c.kept;
    auto give_up = [&](int code, const std::string& m) { c.drop_kept(); return fail(code, m); };
    if (c.quals_absent)
        return give_up(W2RAP_E_STATE, "w2rap_step2_run_step4_after_step3: the reads' raw qualities were never uploaded (Step 2's set_reads ran for a graph-only call): the vote needs them");
    if (k.n != c.n || (c.n && (!c.d_bases || !c.d_boff || !c.d_len || !c.d_quals || !c.d_qoff)))
        return give_up(W2RAP_E_STATE, "w2rap_step2_run_step4_after_step3: the context's reads (Step 2's set_reads) are not the ones the kept large-K paths belong to");
    if (const int rq = quals_wait(c)) { const std::string m = c.err; return give_up(rq, m); }     // a late quality upload still on its way
    c.prof_sums.clear();
    // the call takes the kept blocks over: from here on they are blocks of this call like any other, behind `mark` in c.owned
    const size_t mark = c.owned.size();
    for (void* p : k.blocks()) c.owned.push_back(p);
    c.kept = Ctx::Kept3{};
    Graph4 g; g.K = k.K2; g.E = k.E; g.NV = k.NV; g.ebytes_cap = k.edge_bytes;
    g.ebits = k.ebits; g.ebyte = k.ebyte; g.elen = k.elen; g.from_off = k.from_off; g.from_v = k.from_v; g.from_e = k.from_e;
    g.to_off = k.to_off; g.to_v = k.to_v; g.to_e = k.to_e; g.vleft = k.left; g.vright = k.right; g.inv = k.inv2;
    // (no slack is asked of the read blocks: see upload())
    const ReadsDev R{c.d_bases, c.d_boff, c.d_len, c.d_quals, c.d_qoff};
    PathsDev pd; pd.n = k.n; pd.npe = k.path_ints; pd.offset = k.p_offset; pd.off = k.p_off; pd.edges = k.p_edges;
    const bool vote_only = (P->flags & W2RAP_STEP4_VOTE_ONLY) != 0;
    bool on_device = !(P->flags & (W2RAP_STEP4_EDIT_ON_HOST | W2RAP_STEP4_VOTE_ONLY));
    auto body = [&]() -> int {
        std::vector<int32_t> deleted[2];
        Ms ms[2];
        int at = 0, rc = EDIT4_FALLBACK;
        if (on_device) { DeviceEditor4 ed; rc = passes(c, g, R, pd, *P, ed, deleted, ms, *out, &at); }
        if (rc == EDIT4_FALLBACK) {       // the host editor goes on where the device editor stopped (pass 1's input is gone once pass 1 is through)
            on_device = false;
            HostEditor4 ed;
            ed.edit = !vote_only;
            W2_TRY(host_graph_of(c, g, ed));
            rc = passes(c, g, R, pd, *P, ed, deleted, ms, *out, &at);
        }
        if (rc) return rc;
        return download(c, g, pd, deleted, ms, *out);
    };
    const int rc = body();
    const std::string msg = c.err;
    save_profile4(c, on_device);
    // VOTE_ONLY has edited nothing: the kept result stays.  Otherwise it is consumed (or, after a failure, given up); either way every
    // block this call allocated goes back to the pool
    const std::vector<void*> stay = (!rc && vote_only) ? k.blocks() : std::vector<void*>{};
    for (size_t i = mark; i < c.owned.size(); ++i)
        if (std::find(stay.begin(), stay.end(), c.owned[i]) == stay.end()) c.park(c.owned[i]);
    c.owned.resize(mark);
    if (!rc && vote_only) c.kept = k;
    if (rc) { w2rap_step4_free(out); return fail(rc, msg); }
    return 0;
}

void w2rap_step4_free(w2rap_step4_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->edge_packed, (void*)o->edge_byte_off, (void*)o->edge_len, (void*)o->vleft, (void*)o->vright, (void*)o->from_off, (void*)o->from_v,
                    (void*)o->from_e, (void*)o->to_off, (void*)o->to_v, (void*)o->to_e, (void*)o->inv, (void*)o->path_offset, (void*)o->path_off, (void*)o->path_edges,
                    (void*)o->deleted[0], (void*)o->deleted[1]})
        std::free(p);
    std::memset(o, 0, sizeof(*o));
}

size_t w2rap_step4_profile(char* buf, size_t len) {
    if (buf && len) std::snprintf(buf, len, "%s", g_profile4.c_str());
    return g_profile4.size() + 1;
}

}  // extern "C"
