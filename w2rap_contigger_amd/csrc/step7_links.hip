// step7_links.hip -- the read-sized passes of Step 7 (PE scaffolding): the pairs of every line and MakeGaps up to its accepted gaps.
//
//   LINES   GetTol, GetLineLengths, GetLineNpairs (src/paths/long/large/Lines.cc:329-355, Lines.h:74-117)
//     device  k7_path_len                                  K-mers of every path of every cell
//     device  k7_line_stats                                a thread per line: tol (atomicMax: the LAST line that names an edge wins),
//                                                          llens (one path / mean of two / median of more), the line's end edges
//     device  k7_pair_lines                                a thread per pair: the set of tol[e], tol[inv[e]] over both mates, a sorted
//                                                          list of PAIR_LINES per thread, the spill path beyond; atomics into npairs
//   LINKS   MakeGaps (src/paths/long/large/MakeGaps.cc:25-427)
//     host    edge_groups                                  :56-120  order-dependent (an edge reads what an earlier edge of the sweep wrote)
//     device  k7_nears<false> / scan / k7_nears<true> / sort   :122-207  a thread per (pair, pass); 64-bit offsets; keys e1 << ebits | e2
//     device  k7_heads / scan / k7_kinds / k7_kind_max     the runs of equal nears = the candidates and their counts; per-edge maxima
//     device  k7_close                                     :228-252  a wavefront per candidate, lanes over the first level
//     device  k7_link_flag / scan / k7_link_fill / sort    :253-263  the candidates that are not close, tom applied again, by (first, second)
//     device  k7_filter                                    :276-322  a thread per link, the first filter that rejects it
//     host    set_rules                                    :353-427  the list is no longer than the number of line ends
// Integer arithmetic but for the coverage ratio, which is IEEE double as in the reference (the file is built with -ffp-contract=off).
// Nothing on the device depends on the order in which pairs, nears or links are processed.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "ctx.h"
#include "step5_runs.h"
#include "../../include/w2rap_step7.h"

namespace w2 {
namespace {

constexpr int MAX_HANG = 800, MAX_INT = 1500, PASSES = 3, MAX_LINE_TO_IGNORE = 500;     // MakeGaps.cc:43-48 (max_depth 2 = the three levels of k7_close)
constexpr unsigned PAIR_LINES = W2RAP_STEP7_PAIR_LINES, NEAR_LIST = W2RAP_STEP7_NEAR_LIST;
constexpr unsigned CLOSE_WAVES = 4;                           // candidates per block of k7_close
constexpr uint32_t NOT_CLOSE = 4;

// word[i] += the threads of the block whose x[i] is set (as in step5_open.hip: ballots summed in LDS, one global atomic per block and counter)
template <unsigned N>
__device__ inline void count_block(const bool (&x)[N], unsigned long long* word) {
    __shared__ unsigned sum[N];
    if (threadIdx.x < N) sum[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (unsigned i = 0; i < N; ++i) {
        const unsigned long long b = __ballot(x[i]);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&sum[i], (unsigned)__builtin_popcountll(b));
    }
    __syncthreads();
    if (threadIdx.x < N && sum[threadIdx.x]) atomicAdd(&word[threadIdx.x], (unsigned long long)sum[threadIdx.x]);
}

// the graph as the kernels and the host rules read it
struct Graph {
    const uint64_t* from_off; const int32_t* from_v; const int32_t* from_e; const uint64_t* to_off; const int32_t* to_e;
    const int32_t* vleft; const int32_t* vright;
    __host__ __device__ uint64_t outdeg(int32_t v) const { return from_off[v + 1] - from_off[v]; }
    __host__ __device__ uint64_t indeg(int32_t v) const { return to_off[v + 1] - to_off[v]; }
};
// MakeGaps.cc:305-319 and :374-389: past up to three simple bubbles, to the right of e1 / to the left of e2
__host__ __device__ inline int32_t advance_right(const Graph& g, int32_t e) {
    for (int p = 0; p < PASSES; ++p) {
        const int32_t v = g.vright[e];
        if (g.indeg(v) != 1 || g.outdeg(v) != 2) break;
        const int32_t w = g.from_v[g.from_off[v]];
        if (w != g.from_v[g.from_off[v] + 1]) break;
        if (g.indeg(w) != 2 || g.outdeg(w) != 1) break;
        e = g.from_e[g.from_off[w]];
    }
    return e;
}
__host__ __device__ inline int32_t advance_left(const Graph& g, int32_t e) {
    for (int p = 0; p < PASSES; ++p) {
        const int32_t v = g.vleft[e];
        if (g.outdeg(v) != 1 || g.indeg(v) != 2) break;
        const int32_t w = g.vleft[g.to_e[g.to_off[v]]];
        if (w != g.vleft[g.to_e[g.to_off[v] + 1]]) break;
        if (g.outdeg(w) != 2 || g.indeg(w) != 1) break;
        e = g.to_e[g.to_off[w]];
    }
    return e;
}

// ---- LINES ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k7_path_len(uint64_t NLP, const uint64_t* __restrict__ lpath_off, const int32_t* __restrict__ ledges,
                                                   const uint32_t* __restrict__ elen, int32_t K, int32_t* __restrict__ plen) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NLP) return;
    int32_t sum = 0;                                           // (the argument checks bound a whole line below 2^31)
    for (uint64_t i = lpath_off[p]; i < lpath_off[p + 1]; ++i) sum += (int32_t)elen[ledges[i]] - K + 1;
    plen[p] = sum;
}

// the k-th smallest of x[0 .. n) without storage: the value with at most k smaller ones and more than k not larger
__device__ inline int32_t kth_smallest(const int32_t* __restrict__ x, uint64_t n, uint64_t k) {
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t xi = x[i];
        uint64_t less = 0, leq = 0;
        for (uint64_t j = 0; j < n; ++j) { less += x[j] < xi; leq += x[j] <= xi; }
        if (less <= k && k < leq) return xi;
    }
    return 0;                                                  // (not reached: some value has rank k)
}

// tol is filled with -1 before; a line's entries are contiguous in ledges
__global__ __launch_bounds__(256) void k7_line_stats(uint64_t NL, const uint64_t* __restrict__ line_off, const uint64_t* __restrict__ cell_off,
                                                     const uint64_t* __restrict__ lpath_off, const int32_t* __restrict__ ledges, const int32_t* __restrict__ plen,
                                                     int32_t* __restrict__ tol, int32_t* __restrict__ llens, int32_t* __restrict__ first_edge, int32_t* __restrict__ last_edge) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= NL) return;
    const uint64_t c0 = line_off[l], c1 = line_off[l + 1];
    for (uint64_t i = lpath_off[cell_off[c0]]; i < lpath_off[cell_off[c1]]; ++i) atomicMax(&tol[ledges[i]], (int32_t)l);
    int32_t sum = 0;
    for (uint64_t c = c0; c < c1; ++c) {                       // Lines.h:84-96
        const uint64_t p0 = cell_off[c], np = cell_off[c + 1] - p0;
        if (np == 1) sum += plen[p0];
        else if (np == 2) sum += (plen[p0] + plen[p0 + 1]) / 2;
        else if (np & 1) sum += kth_smallest(plen + p0, np, np / 2);
        else if (np) sum += (kth_smallest(plen + p0, np, np / 2) + kth_smallest(plen + p0, np, np / 2 - 1)) / 2;
    }
    llens[l] = sum;
    first_edge[l] = ledges[lpath_off[cell_off[c0]]];           // lines[l].front()[0][0] and .back()[0][0] (the checks have seen both exist)
    last_edge[l] = ledges[lpath_off[cell_off[c1 - 1]]];
}

// Lines.cc:346-355.  Reads 2p and 2p + 1 are neighbours in the paths' CSR: the pair's edges are pe[a0 .. a2), value 2i of the pair is
// tol[pe[a0 + i]], value 2i + 1 is tol[inv[pe[a0 + i]]]
__global__ __launch_bounds__(256) void k7_pair_lines(uint64_t NP, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ inv,
                                                     const int32_t* __restrict__ tol, int32_t* __restrict__ npairs, unsigned long long* __restrict__ cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool listed = false, spilled = false, no_path = false;
    if (p < NP) {
        const uint64_t a0 = poff[2 * p], nv = 2 * (poff[2 * p + 2] - a0);
        auto value = [&](uint64_t i) { const int32_t e = pe[a0 + (i >> 1)]; return tol[i & 1 ? inv[e] : e]; };
        int32_t list[PAIR_LINES];
        unsigned n = 0;
        for (uint64_t i = 0; i < nv && !spilled; ++i) {        // the short sorted list
            const int32_t v = value(i);
            unsigned at = 0;
            while (at < n && list[at] < v) ++at;
            if (at < n && list[at] == v) continue;
            if (n == PAIR_LINES) { spilled = true; break; }
            for (unsigned k = n; k > at; --k) list[k] = list[k - 1];
            list[at] = v; ++n;
        }
        if (!spilled) {
            listed = true; no_path = nv == 0;
            for (unsigned k = 0; k < n; ++k) atomicAdd(&npairs[list[k]], 1);
        } else {                                               // the spill path: a value counts where it occurs first
            for (uint64_t i = 0; i < nv; ++i) {
                const int32_t v = value(i);
                bool first = true;
                for (uint64_t j = 0; j < i && first; ++j) first = value(j) != v;
                if (first) atomicAdd(&npairs[v], 1);
            }
        }
    }
    const bool what[3] = {listed, spilled, no_path};
    count_block(what, cnt);
}

// ---- LINKS: nears ---------------------------------------------------------------------------------------------------------------
enum { N_PLACED, N_Y_LONG, N_NONE, N_NEAR_CNT };
// MakeGaps.cc:137-195, thread t = (pair t / 2, pass t % 2).  Pass 1: x = the edges of read 2p, y = inv of the edges of read 2p + 1,
// reversed; pass 2 is the same with the mates exchanged (swap, ReverseMe and inv on both come to exactly that).  A sequence after tom,
// the compression of consecutive duplicates and the llens filter is never stored but for up to NEAR_LIST edges of y: it is walked.
// FILL false: near_cnt[t] = the nears of the thread; true: their keys at near_off[t]
template <bool FILL>
__global__ __launch_bounds__(256) void k7_nears(uint64_t NP, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ inv,
                                                const int32_t* __restrict__ tom, const int32_t* __restrict__ tol, const int32_t* __restrict__ llens,
                                                uint32_t* __restrict__ near_cnt, const uint64_t* __restrict__ near_off, unsigned ebits, uint64_t* __restrict__ keys,
                                                unsigned long long* __restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool placed = false, y_long = false, none = false;
    if (t < 2 * NP) {
        const uint64_t p = t >> 1, rx = 2 * p + (t & 1), ry = rx ^ 1;
        const uint64_t xa = poff[rx], xn = poff[rx + 1] - xa, yb = poff[ry + 1], yn = yb - poff[ry];
        uint32_t total = 0;
        if (xn && yn) {
            placed = true;
            auto keep = [&](int32_t v) { return llens[tol[v]] > MAX_LINE_TO_IGNORE; };
            // f(v) for every edge v of y that is kept, in order; stops when f answers true
            auto walk_y = [&](auto f) {
                int32_t prev = -1;
                for (uint64_t j = 0; j < yn; ++j) {
                    const int32_t v = tom[inv[pe[yb - 1 - j]]];
                    if (j && v == prev) continue;
                    prev = v;
                    if (keep(v) && f(v)) return;
                }
            };
            int32_t yl[NEAR_LIST];
            uint32_t ny = 0;
            walk_y([&](int32_t v) { if (ny < NEAR_LIST) yl[ny] = v; ++ny; return false; });
            y_long = ny > NEAR_LIST;
            uint64_t o = FILL ? near_off[t] : 0;
            int32_t prev = -1;
            if (ny) for (uint64_t j = 0; j < xn; ++j) {
                const int32_t v = tom[pe[xa + j]];
                if (j && v == prev) continue;
                prev = v;
                if (!keep(v)) continue;
                bool in_y = false;
                if (!y_long) { for (uint32_t k = 0; k < ny; ++k) in_y |= yl[k] == v; }
                else walk_y([&](int32_t w) { in_y = w == v; return in_y; });
                if (in_y) continue;
                total += ny;
                if (FILL) {
                    if (!y_long) { for (uint32_t k = 0; k < ny; ++k) keys[o++] = (uint64_t)(uint32_t)v << ebits | (uint32_t)yl[k]; }
                    else walk_y([&](int32_t w) { keys[o++] = (uint64_t)(uint32_t)v << ebits | (uint32_t)w; return false; });
                }
            }
            none = total == 0;
        }
        if (!FILL) near_cnt[t] = total;
    }
    if (!FILL) {
        const bool what[3] = {placed, y_long, none};
        count_block(what, &cnt[N_PLACED]);
    }
}

__global__ __launch_bounds__(256) void k7_heads(uint64_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ head) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) head[j] = j == 0 || keys[j] != keys[j - 1];
}
// one candidate per run of equal nears
__global__ __launch_bounds__(256) void k7_kinds(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint64_t* __restrict__ hpos,
                                                unsigned ebits, int32_t* __restrict__ k1, int32_t* __restrict__ k2, uint64_t* __restrict__ kstart) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (head[j]) { const uint64_t k = hpos[j]; k1[k] = (int32_t)(keys[j] >> ebits); k2[k] = (int32_t)(keys[j] & ((1ull << ebits) - 1)); kstart[k] = j; }
    if (j == n - 1) kstart[hpos[n]] = n;
}
// count = the run length; near_max1[e] = the longest run of equal values in the reference's sorted nears1[e], near_max2 likewise
__global__ __launch_bounds__(256) void k7_kind_max(uint64_t NK, const uint64_t* __restrict__ kstart, const int32_t* __restrict__ k1, const int32_t* __restrict__ k2,
                                                   int32_t* __restrict__ kcount, int32_t* __restrict__ max1, int32_t* __restrict__ max2) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= NK) return;
    const uint64_t n = kstart[k + 1] - kstart[k];
    const int32_t c = n > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)n;       // (the reference's counts are int)
    kcount[k] = c;
    atomicMax(&max1[k1[k]], c); atomicMax(&max2[k2[k]], c);
}

// ---- LINKS: the search ------------------------------------------------------------------------------------------------------------
// MakeGaps.cc:233-252, one wavefront per candidate (e1, e2).  The reference's queue is a tree: the roots e1 and, when to_left[e1] has
// exactly one in-edge, that edge (depth -1, 0 K-mers); a node's children are the out-edges of its right vertex and the in-edges of its
// left vertex; every node is compared with e2, and a node is expanded only below depth 2 and with accumulated K-mers <= 1500.  Lanes take
// the roots' children (the first level) 64 at a time; a lane walks its node's children (second level) itself, and the third level is
// not enumerated: e2 is a child of c exactly when to_left[e2] == to_right[c] or to_right[e2] == to_left[c].
// outcome = the fewest steps (0: e2 is the predecessor root) or NOT_CLOSE, | 8 when the predecessor root exists
__global__ __launch_bounds__(64 * CLOSE_WAVES) void k7_close(uint64_t NK, const int32_t* __restrict__ k1, const int32_t* __restrict__ k2, Graph g,
                                                             const uint32_t* __restrict__ elen, int32_t K, uint32_t* __restrict__ outcome) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t k = (uint64_t)blockIdx.x * CLOSE_WAVES + (threadIdx.x >> 6);
    if (k >= NK) return;                                       // (wave-uniform)
    const int32_t e1 = k1[k], e2 = k2[k];
    const int32_t l2 = g.vleft[e2], r2 = g.vright[e2];
    const bool has_pred = g.indeg(g.vleft[e1]) == 1;
    const int32_t root[2] = {e1, has_pred ? g.to_e[g.to_off[g.vleft[e1]]] : e1};
    uint32_t best = has_pred && root[1] == e2 ? 0 : NOT_CLOSE;
    // the first level: per root its out-edges, then its in-edges
    uint64_t seg[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < (has_pred ? 2 : 1); ++r) { seg[2 * r + 1] = seg[2 * r] + g.outdeg(g.vright[root[r]]); seg[2 * r + 2] = seg[2 * r + 1] + g.indeg(g.vleft[root[r]]); }
    if (!has_pred) seg[3] = seg[4] = seg[2];
    auto kmers = [&](int32_t e) { return (int64_t)elen[e] - K + 1; };
    for (uint64_t i = lane; i < seg[4]; i += 64) {
        int s = 0;
        while (i >= seg[s + 1]) ++s;
        const int32_t r = root[s >> 1];
        const int32_t n = s & 1 ? g.to_e[g.to_off[g.vleft[r]] + (i - seg[s])] : g.from_e[g.from_off[g.vright[r]] + (i - seg[s])];
        if (n == e2) { best = best < 1 ? best : 1; continue; }
        const int64_t kn = kmers(n);
        if (kn > MAX_INT) continue;
        auto child = [&](int32_t c) {
            if (c == e2) { best = best < 2 ? best : 2; return; }
            if (kn + kmers(c) > MAX_INT) return;
            if (l2 == g.vright[c] || r2 == g.vleft[c]) best = best < 3 ? best : 3;
        };
        const int32_t v = g.vright[n], w = g.vleft[n];
        for (uint64_t q = g.from_off[v]; q < g.from_off[v + 1]; ++q) child(g.from_e[q]);
        for (uint64_t q = g.to_off[w]; q < g.to_off[w + 1]; ++q) child(g.to_e[q]);
    }
    uint32_t res = NOT_CLOSE;
    for (uint32_t lvl = 0; lvl < NOT_CLOSE; ++lvl) if (__ballot(best == lvl)) { res = lvl; break; }
    if (lane == 0) outcome[k] = res | (has_pred ? 8u : 0u);
}

enum { S_PRED, S_CLOSE0, S_CLOSE1, S_CLOSE2, S_CLOSE3, N_SEARCH_CNT };
__global__ __launch_bounds__(256) void k7_link_flag(uint64_t NK, const uint32_t* __restrict__ outcome, uint32_t* __restrict__ flag, unsigned long long* __restrict__ cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t o = 0xFFu;
    if (k < NK) { o = outcome[k]; flag[k] = (o & 7) == NOT_CLOSE; }
    const bool what[5] = {k < NK && (o & 8) != 0, k < NK && (o & 7) == 0, k < NK && (o & 7) == 1, k < NK && (o & 7) == 2, k < NK && (o & 7) == 3};
    count_block(what, &cnt[S_PRED]);
}
// MakeGaps.cc:256: tom a second time.  value = the candidate: the stable sort leaves links equal after tom in the order of their nears
__global__ __launch_bounds__(256) void k7_link_fill(uint64_t NK, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ lpos, const int32_t* __restrict__ k1,
                                                    const int32_t* __restrict__ k2, const int32_t* __restrict__ tom, unsigned ebits, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= NK || !flag[k]) return;
    keys[lpos[k]] = (uint64_t)(uint32_t)tom[k1[k]] << ebits | (uint32_t)tom[k2[k]]; vals[lpos[k]] = (uint32_t)k;
}

// ---- LINKS: the per-link filters --------------------------------------------------------------------------------------------------
// MakeGaps.cc:276-322, in its order; the first filter that rejects the link is its reason
__global__ __launch_bounds__(256) void k7_filter(uint64_t NLK, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, unsigned ebits, const int32_t* __restrict__ kcount,
                                                 const int32_t* __restrict__ tol, const int32_t* __restrict__ llens, const int32_t* __restrict__ npairs,
                                                 const int32_t* __restrict__ max1, const int32_t* __restrict__ max2, const int32_t* __restrict__ first_edge,
                                                 const int32_t* __restrict__ last_edge, Graph g, int32_t min_line, int32_t min_link_count,
                                                 int32_t* __restrict__ lfrom, int32_t* __restrict__ lto, int32_t* __restrict__ lcount, uint8_t* __restrict__ reason) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NLK) return;
    const int32_t e1 = (int32_t)(keys[i] >> ebits), e2 = (int32_t)(keys[i] & ((1ull << ebits) - 1)), count = kcount[vals[i]];
    lfrom[i] = e1; lto[i] = e2; lcount[i] = count;
    const int32_t t1 = tol[e1], t2 = tol[e2];
    uint8_t r = W2RAP_STEP7_R_ACCEPTED;
    if (count < min_link_count) r = W2RAP_STEP7_R_COUNT;
    else if (llens[t1] < min_line || llens[t2] < min_line) r = W2RAP_STEP7_R_LINE;
    else {
        double c1 = 100.0 * double(npairs[t1]) / double(llens[t1]), c2 = 100.0 * double(npairs[t2]) / double(llens[t2]);
        if (c1 < c2) { const double t = c1; c1 = c2; c2 = t; }
        const int32_t a1 = max1[e1], a2 = max2[e2];
        if (c1 / c2 - 1.0 > 20.0 / 100.0) r = W2RAP_STEP7_R_COVERAGE;       // (inf rejects, NaN passes)
        else if ((a1 > a2 ? a1 : a2) > count) r = W2RAP_STEP7_R_ALT;
        else {
            const int32_t e1x = advance_right(g, e1), e2x = advance_left(g, e2);
            if (last_edge[tol[e1x]] != e1x) r = W2RAP_STEP7_R_LEFT_END;
            else if (first_edge[tol[e2x]] != e2x) r = W2RAP_STEP7_R_RIGHT_END;
        }
    }
    reason[i] = r;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
std::string g_profile7;
void save_profile7(Ctx& c) { g_profile7 = profile_text(c); }

// launches nothing for n == 0 (a grid of no blocks is an error)
#define LAUNCH_N(n, ...) do { if (n) LAUNCH(__VA_ARGS__); } while (0)

// MakeGaps.cc:56-120 on the host, in edge order.  A sweep reads the graph through (F, T): zpass 2 the graph as given, zpass 1 the reversed
// one -- From and To exchanged with the order inside every list kept (digraphE::Reverse swaps the lists), to_right = the given to_left
struct Groups { std::vector<int32_t> tom, dist; std::vector<uint8_t> sink, source; uint64_t loop1 = 0, loop2 = 0; };
void edge_groups(const w2rap_step7_in& in, const std::vector<int32_t>& vleft, const std::vector<int32_t>& vright, Groups& G) {
    const int64_t E = (int64_t)in.n_edge_objs;
    G.tom.resize(E); G.dist.assign(E, 0); G.sink.assign(E, 0); G.source.assign(E, 0);
    for (int64_t e = 0; e < E; ++e) G.tom[e] = (int32_t)e;
    auto kmers = [&](int32_t e) { return (int64_t)in.edge_len[e] - in.K + 1; };
    for (int64_t e = 0; e < E; ++e) {
        if (in.from_off[vright[e] + 1] == in.from_off[vright[e]]) G.sink[e] = 1;
        if (in.to_off[vleft[e] + 1] == in.to_off[vleft[e]]) G.source[e] = 1;
    }
    for (int pass = 1; pass <= PASSES; ++pass)
        for (int zpass = 1; zpass <= 2; ++zpass) {
            const bool rev = zpass == 1;
            const uint64_t* Foff = rev ? in.to_off : in.from_off; const int32_t* Fe = rev ? in.to_e : in.from_e;
            const uint64_t* Toff = rev ? in.from_off : in.to_off;
            const std::vector<int32_t>& right = rev ? vleft : vright;
            std::vector<uint8_t>& like = rev ? G.source : G.sink;
            auto nF = [&](int32_t v) { return Foff[v + 1] - Foff[v]; };
            auto nT = [&](int32_t v) { return Toff[v + 1] - Toff[v]; };
            for (int64_t e = 0; e < E; ++e) {                  // :80-99
                const int32_t v = right[e];
                if (nF(v) != 2 || nT(v) != 1) continue;
                const int32_t e1 = Fe[Foff[v]], e2 = Fe[Foff[v] + 1], w1 = right[e1], w2 = right[e2];
                if (!like[e1] || !like[e2]) continue;
                if (w1 == w2 && nT(w1) != 2) continue;
                if (w1 != w2 && (nT(w1) != 1 || nT(w2) != 1)) continue;
                const int64_t d1 = kmers(e1) + G.dist[e1], d2 = kmers(e2) + G.dist[e2];
                if (d1 > MAX_HANG || d2 > MAX_HANG) continue;
                like[e] = 1; G.dist[e] = (int32_t)std::max(d1, d2);
                G.tom[e1] = G.tom[e]; G.tom[e2] = G.tom[e]; ++G.loop1;
            }
            for (int64_t e = 0; e < E; ++e) {                  // :100-119
                const int32_t v = right[e];
                if (nF(v) != 2 || nT(v) != 1) continue;
                const int32_t e1 = Fe[Foff[v]], e2 = Fe[Foff[v] + 1], w1 = right[e1], w2 = right[e2];
                if (w1 != w2) continue;
                if (nT(w1) != 2 || nF(w1) != 1) continue;
                const int32_t e3 = Fe[Foff[w1]], z = right[e3];
                if (nT(z) != 1) continue;
                if (!like[e3]) continue;
                const int64_t d1 = kmers(e1) + kmers(e3) + G.dist[e3], d2 = kmers(e2) + kmers(e3) + G.dist[e3];
                if (d1 > MAX_HANG || d2 > MAX_HANG) continue;
                like[e] = 1; G.dist[e] = (int32_t)std::max(d1, d2);
                G.tom[e1] = G.tom[e]; G.tom[e2] = G.tom[e]; G.tom[e3] = G.tom[e]; ++G.loop2;
            }
        }
}

// MakeGaps.cc:353-427 on the host, as written
using Pair = std::pair<int32_t, int32_t>;
void set_rules(const w2rap_step7_in& in, const Graph& g, std::vector<Pair> accepted, w2rap_step7_out& out, std::vector<Pair>& gaps, std::vector<int32_t>& gap_inv) {
    const uint64_t E = in.n_edge_objs;
    {   // one-to-one
        std::vector<int32_t> a1, a2;
        for (auto& a : accepted) { a1.push_back(a.first); a2.push_back(a.second); }
        std::sort(a1.begin(), a1.end()); std::sort(a2.begin(), a2.end());
        std::vector<Pair> kept;
        for (auto& a : accepted) {
            const auto r1 = std::equal_range(a1.begin(), a1.end(), a.first), r2 = std::equal_range(a2.begin(), a2.end(), a.second);
            if (r1.second - r1.first != 1 || r2.second - r2.first != 1) ++out.n_not_one_to_one; else kept.push_back(a);
        }
        accepted.swap(kept);
    }
    for (auto& a : accepted) {                                  // past simple bubbles
        const int32_t f = advance_right(g, a.first), t = advance_left(g, a.second);
        if (f != a.first || t != a.second) ++out.n_advanced;
        a = Pair(f, t);
    }
    auto unique_sort = [](std::vector<Pair>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
    unique_sort(accepted);
    const size_t na = accepted.size();
    out.n_unique = na;
    {   // forced symmetry
        std::vector<uint8_t> xa1(E, 0), xa2(E, 0);
        for (auto& a : accepted) { xa1[a.first] = 1; xa2[a.second] = 1; }
        std::vector<Pair> kept, added;
        for (auto& a : accepted) {
            const int32_t re1 = in.inv[a.first], re2 = in.inv[a.second];
            bool del = false;
            if (!std::binary_search(accepted.begin(), accepted.end(), Pair(re2, re1))) {
                if (!xa1[re2] && !xa2[re1]) added.push_back(Pair(re2, re1)); else del = true;
            }
            if (del) ++out.n_sym_deleted; else kept.push_back(a);
        }
        accepted.swap(kept);
        accepted.insert(accepted.end(), added.begin(), added.end());
        unique_sort(accepted);
        out.n_sym_added = (int64_t)accepted.size() - (int64_t)na;
    }
    {   // overlinked
        std::vector<uint32_t> cleft(E, 0), cright(E, 0);
        for (auto& a : accepted) { ++cleft[a.first]; ++cright[a.second]; }
        for (auto& a : accepted) {
            const bool over = cleft[a.first] > 1 || cright[a.first] > 1 || cleft[a.second] > 1 || cright[a.second] > 1;
            if (over) ++out.n_overlinked; else gaps.push_back(a);
        }
    }
    gap_inv.clear();
    for (auto& a : gaps) {
        const Pair r(in.inv[a.second], in.inv[a.first]);
        const auto it = std::lower_bound(gaps.begin(), gaps.end(), r);
        gap_inv.push_back(it != gaps.end() && *it == r ? (int32_t)(it - gaps.begin()) : -1);
    }
}

template <class T> int host_copy(Ctx& c, T** p, const std::vector<T>& v) {
    W2_TRY(host_zeros(c, p, v.size()));
    if (!v.empty()) std::memcpy(*p, v.data(), v.size() * sizeof(T));
    return 0;
}

int step7(Ctx& c, const w2rap_step7_in& in, const w2rap_step7_params& P, uint32_t parts, w2rap_step7_out& out) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices, n = in.n_paths, NP = n / 2, npe = n ? in.path_off[n] : 0, NL = in.n_lines;
    const uint64_t NC = NL ? in.line_off[NL] : 0, NLP = NL ? in.cell_off[NC] : 0, NLE = NL ? in.lpath_off[NLP] : 0;
    static const uint64_t zero = 0;
    std::vector<int32_t> vleft, vright;
    args::edge_ends(in, vleft, vright);

    // ---- uploads
    uint64_t *d_poff = nullptr, *d_line_off = nullptr, *d_cell_off = nullptr, *d_lpath_off = nullptr; int32_t *d_pe = nullptr, *d_inv = nullptr, *d_ledges = nullptr; uint32_t* d_elen = nullptr;
    W2_TRY(up_pooled(c, &d_poff, n ? in.path_off : &zero, n + 1)); W2_TRY(up_pooled(c, &d_pe, in.path_edges, npe)); W2_TRY(up_pooled(c, &d_inv, in.inv, E));
    W2_TRY(up_pooled(c, &d_elen, in.edge_len, E));
    W2_TRY(up_pooled(c, &d_line_off, NL ? in.line_off : &zero, NL + 1)); W2_TRY(up_pooled(c, &d_cell_off, NL ? in.cell_off : &zero, NC + 1));
    W2_TRY(up_pooled(c, &d_lpath_off, NL ? in.lpath_off : &zero, NLP + 1)); W2_TRY(up_pooled(c, &d_ledges, in.line_edges, NLE));

    // ---- tol, llens, the lines' ends (both parts read them), npairs (LINES)
    int32_t *d_plen = nullptr, *d_tol = nullptr, *d_llens = nullptr, *d_first = nullptr, *d_last = nullptr, *d_npairs = nullptr;
    unsigned long long* d_cnt = nullptr;
    W2_ALLOC(d_plen, int32_t, NLP); W2_ALLOC(d_tol, int32_t, E); W2_ALLOC(d_llens, int32_t, NL); W2_ALLOC(d_first, int32_t, NL); W2_ALLOC(d_last, int32_t, NL);
    W2_ALLOC(d_npairs, int32_t, NL); W2_ALLOC(d_cnt, unsigned long long, 16);
    {
        Timer t(c.stream);
        W2_HIP(hipMemsetAsync(d_tol, 0xFF, (E ? E : 1) * 4, c.stream)); W2_HIP(hipMemsetAsync(d_npairs, 0, (NL ? NL : 1) * 4, c.stream));
        W2_HIP(hipMemsetAsync(d_cnt, 0, 16 * 8, c.stream));
        LAUNCH_N(NLP, c, "k7_path_len", k7_path_len, dim3(grid5(NLP)), dim3(256), 0, NLP, (const uint64_t*)d_lpath_off, (const int32_t*)d_ledges, (const uint32_t*)d_elen, in.K, d_plen);
        LAUNCH_N(NL, c, "k7_line_stats", k7_line_stats, dim3(grid5(NL)), dim3(256), 0, NL, (const uint64_t*)d_line_off, (const uint64_t*)d_cell_off, (const uint64_t*)d_lpath_off,
                 (const int32_t*)d_ledges, (const int32_t*)d_plen, d_tol, d_llens, d_first, d_last);
        if (parts & W2RAP_STEP7_LINES)
            LAUNCH_N(NP, c, "k7_pair_lines", k7_pair_lines, dim3(grid5(NP)), dim3(256), 0, NP, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const int32_t*)d_inv, (const int32_t*)d_tol,
                     d_npairs, d_cnt);
        out.ms_lines = t.stop();
    }
    W2_TRY(dl(c, &out.tol, (const int32_t*)d_tol, E)); W2_TRY(dl(c, &out.llens, (const int32_t*)d_llens, NL));
    if (parts & W2RAP_STEP7_LINES) {
        unsigned long long cnt[3] = {0};
        W2_TRY(dl(c, &out.npairs, (const int32_t*)d_npairs, NL));
        W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        out.n_pairs = NP; out.n_pairs_listed = cnt[0]; out.n_pairs_spilled = cnt[1]; out.n_pairs_no_path = cnt[2];
        for (uint64_t l = 0; l < NL; ++l) out.n_line_hits += (uint64_t)out.npairs[l];
    }
    W2_HIP(hipStreamSynchronize(c.stream));

    if (parts & W2RAP_STEP7_LINKS) {
        if (in.npairs) W2_HIP(hipMemcpyAsync(d_npairs, in.npairs, NL * 4, hipMemcpyHostToDevice, c.stream));      // the given values, not LINES' own
        // ---- 1. edge groups (host)
        Groups G;
        edge_groups(in, vleft, vright, G);
        out.n_group_loop1 = G.loop1; out.n_group_loop2 = G.loop2;
        for (uint64_t e = 0; e < E; ++e) { out.n_group_sink += G.sink[e]; out.n_group_source += G.source[e]; }
        W2_TRY(host_copy(c, &out.tom, G.tom)); W2_TRY(host_copy(c, &out.dist_to_end, G.dist)); W2_TRY(host_copy(c, &out.sink_like, G.sink)); W2_TRY(host_copy(c, &out.source_like, G.source));
        int32_t *d_tom = nullptr, *d_vleft = nullptr, *d_vright = nullptr, *d_from_v = nullptr, *d_from_e = nullptr, *d_to_e = nullptr; uint64_t *d_from_off = nullptr, *d_to_off = nullptr;
        W2_TRY(up_pooled(c, &d_tom, (const int32_t*)G.tom.data(), E)); W2_TRY(up_pooled(c, &d_vleft, (const int32_t*)vleft.data(), E)); W2_TRY(up_pooled(c, &d_vright, (const int32_t*)vright.data(), E));
        W2_TRY(up_pooled(c, &d_from_off, NV ? in.from_off : &zero, NV + 1)); W2_TRY(up_pooled(c, &d_to_off, NV ? in.to_off : &zero, NV + 1));
        W2_TRY(up_pooled(c, &d_from_v, in.from_v, E)); W2_TRY(up_pooled(c, &d_from_e, in.from_e, E)); W2_TRY(up_pooled(c, &d_to_e, in.to_e, E));
        W2_HIP(hipStreamSynchronize(c.stream));                 // (the host vectors above have been read)
        const Graph dg{d_from_off, d_from_v, d_from_e, d_to_off, d_to_e, d_vleft, d_vright};
        const unsigned ebits = bits_for(E ? E : 1);

        // ---- 2. nears
        uint64_t NN = 0, NK = 0, NLK = 0;
        uint32_t* d_ncnt = nullptr; uint64_t *d_noff = nullptr, *d_keys = nullptr, *d_hpos = nullptr, *d_kstart = nullptr; uint32_t *d_vals = nullptr, *d_head = nullptr;
        int32_t *d_k1 = nullptr, *d_k2 = nullptr, *d_kcount = nullptr, *d_max1 = nullptr, *d_max2 = nullptr;
        W2_ALLOC(d_max1, int32_t, E); W2_ALLOC(d_max2, int32_t, E);
        {
            Timer t(c.stream);
            W2_HIP(hipMemsetAsync(d_max1, 0, (E ? E : 1) * 4, c.stream)); W2_HIP(hipMemsetAsync(d_max2, 0, (E ? E : 1) * 4, c.stream));
            W2_HIP(hipMemsetAsync(d_cnt, 0, 16 * 8, c.stream));
            W2_ALLOC(d_ncnt, uint32_t, 2 * NP + 1); W2_ALLOC(d_noff, uint64_t, 2 * NP + 2);
            if (NP) {
                LAUNCH(c, "k7_nears_count", k7_nears<false>, dim3(grid5(2 * NP)), dim3(256), 0, NP, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const int32_t*)d_inv, (const int32_t*)d_tom,
                       (const int32_t*)d_tol, (const int32_t*)d_llens, d_ncnt, (const uint64_t*)nullptr, ebits, (uint64_t*)nullptr, d_cnt);
                W2_TRY(exclusive_scan_u32_to_u64(c, d_ncnt, d_noff, 2 * NP));
                W2_HIP(hipMemcpyAsync(&NN, d_noff + 2 * NP, 8, hipMemcpyDeviceToHost, c.stream));
                W2_HIP(hipStreamSynchronize(c.stream));
            }
            if (NN) {
                W2_ALLOC(d_keys, uint64_t, NN + 1); W2_ALLOC(d_vals, uint32_t, NN + 1);
                W2_HIP(hipMemsetAsync(d_vals, 0, (NN + 1) * 4, c.stream));      // (the sort carries a value; the nears have none)
                LAUNCH(c, "k7_nears_fill", k7_nears<true>, dim3(grid5(2 * NP)), dim3(256), 0, NP, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const int32_t*)d_inv, (const int32_t*)d_tom,
                       (const int32_t*)d_tol, (const int32_t*)d_llens, (uint32_t*)nullptr, (const uint64_t*)d_noff, ebits, d_keys, d_cnt);
                W2_TRY(sort_pairs_u64(c, d_keys, d_vals, NN, 0, (int)(2 * ebits)));
                W2_ALLOC(d_head, uint32_t, NN + 1); W2_ALLOC(d_hpos, uint64_t, NN + 2);
                LAUNCH(c, "k7_heads", k7_heads, dim3(grid5(NN)), dim3(256), 0, NN, (const uint64_t*)d_keys, d_head);
                W2_TRY(exclusive_scan_u32_to_u64(c, d_head, d_hpos, NN));
                W2_HIP(hipMemcpyAsync(&NK, d_hpos + NN, 8, hipMemcpyDeviceToHost, c.stream));
                W2_HIP(hipStreamSynchronize(c.stream));
                if (NK >= (1ull << 32)) { c.err = "2^32 distinct nears or more"; return W2RAP_E_LIMIT; }
                W2_ALLOC(d_k1, int32_t, NK); W2_ALLOC(d_k2, int32_t, NK); W2_ALLOC(d_kstart, uint64_t, NK + 1); W2_ALLOC(d_kcount, int32_t, NK);
                LAUNCH(c, "k7_kinds", k7_kinds, dim3(grid5(NN)), dim3(256), 0, NN, (const uint64_t*)d_keys, (const uint32_t*)d_head, (const uint64_t*)d_hpos, ebits, d_k1, d_k2, d_kstart);
                LAUNCH(c, "k7_kind_max", k7_kind_max, dim3(grid5(NK)), dim3(256), 0, NK, (const uint64_t*)d_kstart, (const int32_t*)d_k1, (const int32_t*)d_k2, d_kcount, d_max1, d_max2);
            }
            out.ms_nears = t.stop();
            unsigned long long cnt[N_NEAR_CNT] = {0};
            W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
            W2_HIP(hipStreamSynchronize(c.stream));
            out.n_pass_placed = cnt[N_PLACED]; out.n_pass_y_long = cnt[N_Y_LONG]; out.n_pass_none = cnt[N_NONE]; out.n_nears = NN; out.n_near_kinds = NK;
            for (void* p : {(void*)d_ncnt, (void*)d_noff, (void*)d_keys, (void*)d_vals, (void*)d_head, (void*)d_hpos, (void*)d_kstart}) c.release(p);
        }
        W2_TRY(dl(c, &out.near_max1, (const int32_t*)d_max1, E)); W2_TRY(dl(c, &out.near_max2, (const int32_t*)d_max2, E));

        // ---- 3. the search, the links
        uint64_t* d_lkeys = nullptr; uint32_t* d_lvals = nullptr;
        {
            Timer t(c.stream);
            unsigned long long cnt[N_SEARCH_CNT] = {0};
            if (NK) {
                uint32_t *d_outcome = nullptr, *d_flag = nullptr; uint64_t* d_lpos = nullptr;
                W2_ALLOC(d_outcome, uint32_t, NK); W2_ALLOC(d_flag, uint32_t, NK + 1); W2_ALLOC(d_lpos, uint64_t, NK + 2);
                W2_HIP(hipMemsetAsync(d_cnt, 0, 16 * 8, c.stream));
                LAUNCH(c, "k7_close", k7_close, dim3(grid5(NK, CLOSE_WAVES)), dim3(64 * CLOSE_WAVES), 0, NK, (const int32_t*)d_k1, (const int32_t*)d_k2, dg, (const uint32_t*)d_elen, in.K, d_outcome);
                LAUNCH(c, "k7_link_flag", k7_link_flag, dim3(grid5(NK)), dim3(256), 0, NK, (const uint32_t*)d_outcome, d_flag, d_cnt);
                W2_TRY(exclusive_scan_u32_to_u64(c, d_flag, d_lpos, NK));
                W2_HIP(hipMemcpyAsync(&NLK, d_lpos + NK, 8, hipMemcpyDeviceToHost, c.stream));
                W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
                W2_HIP(hipStreamSynchronize(c.stream));
                if (NLK) {
                    W2_ALLOC(d_lkeys, uint64_t, NLK + 1); W2_ALLOC(d_lvals, uint32_t, NLK + 1);
                    LAUNCH(c, "k7_link_fill", k7_link_fill, dim3(grid5(NK)), dim3(256), 0, NK, (const uint32_t*)d_flag, (const uint64_t*)d_lpos, (const int32_t*)d_k1, (const int32_t*)d_k2,
                           (const int32_t*)d_tom, ebits, d_lkeys, d_lvals);
                    W2_TRY(sort_pairs_u64(c, d_lkeys, d_lvals, NLK, 0, (int)(2 * ebits)));
                }
                for (void* p : {(void*)d_outcome, (void*)d_flag, (void*)d_lpos}) c.release(p);
            }
            out.ms_search = t.stop();
            out.n_pred_start = cnt[S_PRED]; for (int i = 0; i < 4; ++i) out.n_close[i] = cnt[S_CLOSE0 + i];
            out.n_links = NLK;
        }

        // ---- 4. the filters
        {
            Timer t(c.stream);
            int32_t *d_lfrom = nullptr, *d_lto = nullptr, *d_lcount = nullptr; uint8_t* d_reason = nullptr;
            W2_ALLOC(d_lfrom, int32_t, NLK); W2_ALLOC(d_lto, int32_t, NLK); W2_ALLOC(d_lcount, int32_t, NLK); W2_ALLOC(d_reason, uint8_t, NLK);
            LAUNCH_N(NLK, c, "k7_filter", k7_filter, dim3(grid5(NLK)), dim3(256), 0, NLK, (const uint64_t*)d_lkeys, (const uint32_t*)d_lvals, ebits, (const int32_t*)d_kcount, (const int32_t*)d_tol,
                     (const int32_t*)d_llens, (const int32_t*)d_npairs, (const int32_t*)d_max1, (const int32_t*)d_max2, (const int32_t*)d_first, (const int32_t*)d_last, dg, P.min_line,
                     P.min_link_count, d_lfrom, d_lto, d_lcount, d_reason);
            out.ms_filter = t.stop();
            W2_TRY(dl(c, &out.link_from, (const int32_t*)d_lfrom, NLK)); W2_TRY(dl(c, &out.link_to, (const int32_t*)d_lto, NLK)); W2_TRY(dl(c, &out.link_count, (const int32_t*)d_lcount, NLK));
            W2_TRY(dl(c, &out.link_reason, (const uint8_t*)d_reason, NLK));
            W2_HIP(hipStreamSynchronize(c.stream));
            for (void* p : {(void*)d_lfrom, (void*)d_lto, (void*)d_lcount, (void*)d_reason}) c.release(p);
        }

        // ---- 5. the set rules (host)
        std::vector<Pair> accepted, gaps; std::vector<int32_t> gap_inv, gfrom, gto;
        for (uint64_t i = 0; i < NLK; ++i) {
            const unsigned r = out.link_reason[i] < 7 ? out.link_reason[i] : 0;
            ++out.n_reason[r];
            if (r == W2RAP_STEP7_R_ACCEPTED) accepted.push_back(Pair(out.link_from[i], out.link_to[i]));
        }
        const Graph hg{in.from_off, in.from_v, in.from_e, in.to_off, in.to_e, vleft.data(), vright.data()};
        set_rules(in, hg, accepted, out, gaps, gap_inv);
        for (auto& a : gaps) { gfrom.push_back(a.first); gto.push_back(a.second); }
        out.n_gaps = gaps.size();
        W2_TRY(host_copy(c, &out.gap_from, gfrom)); W2_TRY(host_copy(c, &out.gap_to, gto)); W2_TRY(host_copy(c, &out.gap_inv, gap_inv));
        for (void* p : {(void*)d_tom, (void*)d_vleft, (void*)d_vright, (void*)d_from_off, (void*)d_to_off, (void*)d_from_v, (void*)d_from_e, (void*)d_to_e, (void*)d_k1, (void*)d_k2,
                        (void*)d_kcount, (void*)d_max1, (void*)d_max2, (void*)d_lkeys, (void*)d_lvals}) c.release(p);
    }
    W2_HIP(hipStreamSynchronize(c.stream));
    for (void* p : {(void*)d_poff, (void*)d_pe, (void*)d_inv, (void*)d_elen, (void*)d_line_off, (void*)d_cell_off, (void*)d_lpath_off, (void*)d_ledges, (void*)d_plen, (void*)d_tol,
                    (void*)d_llens, (void*)d_first, (void*)d_last, (void*)d_npairs, (void*)d_cnt}) c.release(p);
    return 0;
}

// The argument checks: 0, or the code with the message in `err`.  Everything a kernel or a host rule uses as an index is looked at here
int step7_check(const w2rap_step7_in* in, const w2rap_step7_params* P, char* err, size_t errlen) {
    auto fail = [&](int code, const char* m) { if (err && errlen) std::snprintf(err, errlen, "%s", m); return code; };
    if (!in || !P) return fail(W2RAP_E_ARG, "null argument");
    if (P->flags & ~(W2RAP_STEP7_LINES | W2RAP_STEP7_LINKS)) return fail(W2RAP_E_ARG, "unknown flag");
    if (P->min_line < 0 || P->min_link_count < 0) return fail(W2RAP_E_ARG, "min_line and min_link_count must not be negative");
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640]");
    if (args::too_large(*in, args::READS_END)) return fail(W2RAP_E_ARG, args::TOO_LARGE);
    if (in->n_paths & 1) return fail(W2RAP_E_ARG, args::ODD_PATHS);
    W2_ARGS(args::null_arrays(*in, !in->inv));
    W2_ARGS(args::edge_lens(*in, 1ull << 31));
    W2_ARGS(args::adjacency(*in));
    W2_ARGS(args::from_v_agrees(*in));
    W2_ARGS(args::involution(*in));
    W2_ARGS(args::reads_and_paths(*in));
    W2_ARGS(args::lines(*in));
    W2_ARGS(args::lines_cover(*in));
    W2_ARGS(args::line_lengths(*in));
    const uint32_t parts = P->flags ? P->flags : (W2RAP_STEP7_LINES | W2RAP_STEP7_LINKS);
    W2_ARGS(args::npairs_given(*in, !(parts & W2RAP_STEP7_LINES)));
    return 0;
}

}  // namespace

// for step7_cov.hip (w2rap_step7_coverage): part LINES as above on the caller's context -- tol, llens, npairs and the LINES counters in
// `out` --, and the profile that w2rap_step7_profile reads
int step7_lines_part(Ctx& c, const w2rap_step7_in& in, w2rap_step7_out& out) {
    const w2rap_step7_params P{};
    return step7(c, in, P, W2RAP_STEP7_LINES, out);
}
void save_profile7_shared(Ctx& c) { save_profile7(c); }
}  // namespace w2

using namespace w2;

extern "C" int w2rap_step7_links(const w2rap_step7_in* in, const w2rap_step7_params* P, w2rap_step7_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (const int rc = step7_check(in, P, err, errlen)) return rc;
    const uint32_t parts = P->flags ? P->flags : (W2RAP_STEP7_LINES | W2RAP_STEP7_LINKS);
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return step7(c, *in, *P, parts, *out); }, save_profile7, [&] { w2rap_step7_free(out); });
}

extern "C" void w2rap_step7_free(w2rap_step7_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->tol, (void*)o->llens, (void*)o->npairs, (void*)o->tom, (void*)o->sink_like, (void*)o->source_like, (void*)o->dist_to_end, (void*)o->near_max1,
                    (void*)o->near_max2, (void*)o->link_from, (void*)o->link_to, (void*)o->link_count, (void*)o->link_reason, (void*)o->gap_from, (void*)o->gap_to, (void*)o->gap_inv})
        std::free(p);
    std::memset(o, 0, sizeof(*o));
}

extern "C" size_t w2rap_step7_profile(char* buf, size_t len) {
    if (buf && len) std::snprintf(buf, len, "%s", g_profile7.c_str());
    return g_profile7.size() + 1;
}
