// step7_cov.hip -- ComputeCoverage (src/paths/long/large/Lines.cc:442-624) and CNIntegerFraction (GapToyTools5.cc:1520-1538):
// w2rap_step7_coverage of include/w2rap_step7.h, where the semantics are written out.
//
//   device  part LINES of step7_links.hip                      npairs, llens (the kernels where they lie, unchanged)
//   host    cov::candidates, cov::find_peak (step7_peak.h)      covl, the candidates, mass, base_cov
//   host    cov::cell_groups                                    the (in, out) classes of every odd cell: e, z, the upper median
//   device  paths_index (step5_runs.h)                          only when a group or a long edge needs it
//   device  k7c_row_len / scan / k7c_emit / sort / k5_heads / scan / k5o_lower_bound / k7c_group_count
//                                                               the distinct pairs of every cell group
//   device  k7c_row_len / scan / k7c_single_flag / scan / k7c_single_count
//                                                               the distinct pairs of the long edges, one edge a group, without a sort (the
//                                                               sorted form on request: both are measured in tools/step7_time.py --coverage)
//   device  k7c_line_pos, k7c_cell_pos                          which write of the reference's loops reaches an edge last
//   device  k7c_edge_cov, k7c_need_fill, k7c_edge_long          the three rules per edge, the counts of CNIntegerFraction
// IEEE double with one rounding to float at Set; the file is built with -ffp-contract=off and no fast-math.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "step5_runs.h"
#include "step7_peak.h"
#include "../../include/w2rap_step7.h"

namespace w2 {
int step7_lines_part(Ctx& c, const w2rap_step7_in& in, w2rap_step7_out& out);      // step7_links.hip
void save_profile7_shared(Ctx& c);
namespace {

constexpr int MIN_LINE = cov::MIN_LINE;
// What the recorded runs of the reference (built with -Ofast) say about `x / base_cov` in its three loops: see w2rap_step7.h
constexpr bool RECIP_LINE = cov::RECIP_LINE, RECIP_CELL = cov::RECIP_CELL, RECIP_LONG = cov::RECIP_LONG, ABS_FLOATING = cov::ABS_FLOATING;

#define LAUNCH_N(n, ...) do { if (n) LAUNCH(__VA_ARGS__); } while (0)

// covcount::Set.  A NaN (0 / 0, with base_cov 0) is stored as the reference's x86-64 build stores it: the default NaN, sign bit set
template <bool RECIP> __device__ inline float set_cov(double x, double base, double rbase) {
    const float v = (float)(RECIP ? x * rbase : x / base);
    return v != v ? __uint_as_float(0xFFC00000u) : v;
}

// word[i] += the threads of the block whose x[i] is set: ballots summed in LDS, one global atomic per block and counter.  (count_block of
// step7_links.hip and step5_open.hip, copied: sharing it from a header would re-instantiate it inside the LINES file, whose kernels
// this change must not alter.)
template <unsigned N>
__device__ inline void count_block7c(const bool (&x)[N], unsigned long long* word) {
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

// ---- the distinct pairs of a group ------------------------------------------------------------------------------------------------
// item t = (entry t / 2 of the groups' edge list, pass t % 2): the index row of e in pass 0, of inv[e] in pass 1 (Pids reads both, an
// edge that is its own inverse twice)
__global__ __launch_bounds__(256) void k7c_row_len(uint64_t NT, const int32_t* __restrict__ gedges, const int32_t* __restrict__ inv, const uint64_t* __restrict__ ioff,
                                                   uint64_t* __restrict__ rlen) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= NT) return;
    const int32_t e = gedges[t >> 1], d = t & 1 ? inv[e] : e;
    rlen[t] = ioff[d + 1] - ioff[d];
}

// a thread per index entry of every row: key = group << pbits | read / 2.  gof: the group of every entry of the edge list, null: entry i
// is group i (the long edges).  roff[t] <= j < roff[t + 1] finds the row (rows of no entries are stepped over)
__global__ __launch_bounds__(256) void k7c_emit(uint64_t M, uint64_t NT, const uint64_t* __restrict__ roff, const int32_t* __restrict__ gedges, const uint32_t* __restrict__ gof,
                                                const int32_t* __restrict__ inv, const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ iread, unsigned pbits,
                                                uint64_t* __restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    uint64_t lo = 0, hi = NT - 1;                              // the answer lies in [lo, hi]: j < M = roff[NT]
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (roff[mid + 1] <= j) lo = mid + 1; else hi = mid; }
    const uint64_t i = lo >> 1;
    const int32_t e = gedges[i], d = lo & 1 ? inv[e] : e;
    const uint32_t r = iread[ioff[d] + (j - roff[lo])];
    keys[j] = ((uint64_t)(gof ? gof[i] : (uint32_t)i) << pbits) | (r >> 1);
}

// gstart[g] = the first sorted key of group g (k5o_lower_bound), hpos = the scanned head flags: the distinct keys of a group
__global__ __launch_bounds__(256) void k7c_group_count(uint64_t G, const uint64_t* __restrict__ gstart, const uint64_t* __restrict__ hpos, int64_t* __restrict__ count) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) count[g] = (int64_t)(hpos[gstart[g + 1]] - hpos[gstart[g]]);
}

// The sort-free form for groups of ONE edge.  An index row ascends in read id, so the entries of a pair are neighbours: flag[j] = entry j
// opens a pair of its row and -- in the row of inv[e] (pass 1) -- that pair has no entry in the row of e (binary search): the distinct
// pairs of row e, plus those of row inv[e], minus the pairs in both.  An edge that is its own inverse finds all of its second row in the first
__global__ __launch_bounds__(256) void k7c_single_flag(uint64_t M, uint64_t NT, const uint64_t* __restrict__ roff, const int32_t* __restrict__ gedges, const int32_t* __restrict__ inv,
                                                       const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ iread, uint32_t* __restrict__ flag) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    uint64_t lo = 0, hi = NT - 1;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (roff[mid + 1] <= j) lo = mid + 1; else hi = mid; }
    const int32_t e = gedges[lo >> 1], d = lo & 1 ? inv[e] : e;
    const uint64_t pos = ioff[d] + (j - roff[lo]);
    const uint32_t pid = iread[pos] >> 1;
    bool f = j == roff[lo] || (iread[pos - 1] >> 1) != pid;
    if (f && (lo & 1)) {
        uint64_t a = ioff[e], b = ioff[e + 1];
        while (a < b) { const uint64_t mid = (a + b) >> 1; if ((iread[mid] >> 1) < pid) a = mid + 1; else b = mid; }
        if (a < ioff[e + 1] && (iread[a] >> 1) == pid) f = false;
    }
    flag[j] = f;
}

// group g = the rows 2g and 2g + 1: the flags between their ends
__global__ __launch_bounds__(256) void k7c_single_count(uint64_t G, const uint64_t* __restrict__ roff, const uint64_t* __restrict__ fpos, int64_t* __restrict__ count) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) count[g] = (int64_t)(fpos[roff[2 * g + 2]] - fpos[roff[2 * g]]);
}

// ---- the rules ------------------------------------------------------------------------------------------------------------------
// Lines.cc:550-557: the loop position (the cell's global index + 1) of the last even cell of a line of 1000 K-mers or more that names e first
__global__ __launch_bounds__(256) void k7c_line_pos(uint64_t NL, const uint64_t* __restrict__ line_off, const uint64_t* __restrict__ cell_off, const uint64_t* __restrict__ lpath_off,
                                                    const int32_t* __restrict__ ledges, const int32_t* __restrict__ llens, uint32_t* __restrict__ pos_line) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= NL || llens[l] < MIN_LINE) return;
    for (uint64_t cl = line_off[l]; cl < line_off[l + 1]; cl += 2) atomicMax(&pos_line[ledges[lpath_off[cell_off[cl]]]], (uint32_t)cl + 1);
}

// Lines.cc:614-615: the last group (groups are numbered in loop order) whose z holds e
__global__ __launch_bounds__(256) void k7c_cell_pos(uint64_t NZ, const uint32_t* __restrict__ zgroup, const int32_t* __restrict__ z, uint32_t* __restrict__ pos_cell) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NZ) atomicMax(&pos_cell[z[i]], zgroup[i] + 1);
}

// the line rule, then the cell rule; need[e] = the long-edge rule is due (Lines.cc:621)
__global__ __launch_bounds__(256) void k7c_edge_cov(uint64_t E, const uint32_t* __restrict__ pos_line, const uint32_t* __restrict__ cell_line, const double* __restrict__ covl,
                                                    const uint32_t* __restrict__ pos_cell, const int64_t* __restrict__ gcount, const int32_t* __restrict__ glen, double base, double rbase,
                                                    const uint32_t* __restrict__ elen, int32_t K, float* __restrict__ cov, uint8_t* __restrict__ rule, uint32_t* __restrict__ need) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float v = -1.0f;
    uint8_t r = W2RAP_STEP7_RULE_NONE;
    if (pos_line[e]) { v = set_cov<RECIP_LINE>(covl[cell_line[pos_line[e] - 1]], base, rbase); r = W2RAP_STEP7_RULE_LINE; }
    if (pos_cell[e]) {
        const uint32_t g = pos_cell[e] - 1;
        v = set_cov<RECIP_CELL>(double(gcount[g]) / double(glen[g]), base, rbase); r = W2RAP_STEP7_RULE_CELL;
    }
    cov[e] = v; rule[e] = r;
    need[e] = !(v >= 0) && (int32_t)elen[e] - K + 1 >= MIN_LINE;
}

__global__ __launch_bounds__(256) void k7c_need_fill(uint64_t E, const uint32_t* __restrict__ need, const uint64_t* __restrict__ npos, int32_t* __restrict__ gedges) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E && need[e]) gedges[npos[e]] = (int32_t)e;
}

enum { C_RULE0, C_RULE1, C_RULE2, C_RULE3, C_UNDEF, C_CN_EDGES, C_CN_GOOD, N_CNT };
// the long-edge rule (Lines.cc:619-624), and CNIntegerFraction's two counts over the finished values
__global__ __launch_bounds__(256) void k7c_edge_long(uint64_t E, const uint32_t* __restrict__ need, const uint64_t* __restrict__ npos, const int64_t* __restrict__ count1,
                                                     const uint32_t* __restrict__ elen, int32_t K, double base, double rbase, double frac, int32_t min_edge_size,
                                                     float* __restrict__ cov, uint8_t* __restrict__ rule, unsigned long long* __restrict__ cnt) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool what[N_CNT] = {false, false, false, false, false, false, false};
    if (e < E) {
        float v = cov[e];
        uint8_t r = rule[e];
        if (need[e]) {
            v = set_cov<RECIP_LONG>(double(count1[npos[e]]) / double((int32_t)elen[e] - K + 1), base, rbase); r = W2RAP_STEP7_RULE_LONG;
            cov[e] = v; rule[e] = r;
        }
        what[r] = true;
        what[C_UNDEF] = !(v >= 0);
        if ((int64_t)elen[e] >= (int64_t)min_edge_size && v >= 0) {
            what[C_CN_EDGES] = true;
            const double fc = (double)v, t = fc + 0.5;
            const int ic = t >= 2147483648.0 ? 2147483647 : (int)t;
            what[C_CN_GOOD] = ABS_FLOATING ? fabs((double)ic - fc) <= frac : (double)abs((int)((double)ic - fc)) <= frac;
        }
    }
    count_block7c(what, cnt);
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
template <class T> int host_copy(Ctx& c, T** p, const std::vector<T>& v) {
    W2_TRY(host_zeros(c, p, v.size()));
    if (!v.empty()) std::memcpy(*p, v.data(), v.size() * sizeof(T));
    return 0;
}

struct Index { uint64_t *poff = nullptr, *keys = nullptr, *ioff = nullptr; int32_t* pe = nullptr; uint32_t* iread = nullptr; bool built = false; };

int build_index(Ctx& c, const w2rap_step7_cov_in& in, Index& X, w2rap_step7_cov_out& out) {
    if (X.built) return 0;
    const uint64_t E = in.n_edge_objs, n = in.n_paths, npe = n ? in.path_off[n] : 0;
    static const uint64_t zero = 0;
    Timer t(c.stream);
    W2_TRY(up_pooled(c, &X.poff, n ? in.path_off : &zero, n + 1)); W2_TRY(up_pooled(c, &X.pe, in.path_edges, npe));
    if (npe) W2_TRY(paths_index(c, X.poff, X.pe, n, npe, E, &X.keys, &X.iread, &X.ioff));
    else { W2_ALLOC(X.ioff, uint64_t, E + 2); W2_ALLOC(X.iread, uint32_t, 1); W2_HIP(hipMemsetAsync(X.ioff, 0, (E + 2) * 8, c.stream)); }       // no path entry: every row empty
    out.ms_index += t.stop();
    X.built = true; out.index_built = 1;
    return 0;
}

// count[g] = the distinct read / 2 over the index rows of every edge of group g and of its inverse.  d_gedges: the groups' edges, NGE of
// them; d_gof: the group of every entry (null: entry i is group i); G groups; NP pairs.  *entries = the keys sorted
// sort_free (one edge a group, d_gof null): no keys and no sort -- k7c_single_flag, a scan, k7c_single_count
int count_groups(Ctx& c, const Index& X, const int32_t* d_inv, const int32_t* d_gedges, const uint32_t* d_gof, uint64_t NGE, uint64_t G, uint64_t NP, int64_t** d_count, uint64_t* entries,
                 bool sort_free = false) {
    const uint64_t NT = 2 * NGE;
    uint64_t *rlen = nullptr, *roff = nullptr, *keys = nullptr, *hpos = nullptr, *gstart = nullptr; uint32_t *vals = nullptr, *head = nullptr;
    uint64_t M = 0, n_runs = 0;
    W2_ALLOC(*d_count, int64_t, G + 1);
    W2_HIP(hipMemsetAsync(*d_count, 0, (G + 1) * 8, c.stream));
    *entries = 0;
    if (!NT) return 0;
    W2_ALLOC(rlen, uint64_t, NT + 1); W2_ALLOC(roff, uint64_t, NT + 2);
    LAUNCH(c, "k7c_row_len", k7c_row_len, dim3(grid5(NT)), dim3(256), 0, NT, d_gedges, d_inv, (const uint64_t*)X.ioff, rlen);
    W2_TRY(exclusive_scan_u64(c, rlen, roff, NT));
    W2_HIP(hipMemcpyAsync(&M, roff + NT, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    *entries = M;
    if (M && sort_free) {
        W2_ALLOC(head, uint32_t, M + 1); W2_ALLOC(hpos, uint64_t, M + 2);
        LAUNCH(c, "k7c_single_flag", k7c_single_flag, dim3(grid5(M)), dim3(256), 0, M, NT, (const uint64_t*)roff, d_gedges, d_inv, (const uint64_t*)X.ioff, (const uint32_t*)X.iread, head);
        W2_TRY(exclusive_scan_u32_to_u64(c, head, hpos, M));
        LAUNCH(c, "k7c_single_count", k7c_single_count, dim3(grid5(G)), dim3(256), 0, G, (const uint64_t*)roff, (const uint64_t*)hpos, *d_count);
    } else if (M) {
        const unsigned pbits = bits_for(NP ? NP : 1), gbits = bits_for(G);
        W2_ALLOC(keys, uint64_t, M + 1); W2_ALLOC(vals, uint32_t, M + 1); W2_ALLOC(gstart, uint64_t, G + 2);
        // the library's one radix sort moves (key, 32-bit value) pairs and has no keys-only form; the value is not read here, so it is carried
        // as zeros (4 of the 12 bytes per entry and pass) rather than a second sort being added for this call
        W2_HIP(hipMemsetAsync(vals, 0, (M + 1) * 4, c.stream));
        LAUNCH(c, "k7c_emit", k7c_emit, dim3(grid5(M)), dim3(256), 0, M, NT, (const uint64_t*)roff, d_gedges, d_gof, d_inv, (const uint64_t*)X.ioff, (const uint32_t*)X.iread, pbits, keys);
        W2_TRY(sort_pairs_u64(c, keys, vals, M, 0, (int)(pbits + gbits)));
        W2_TRY(run_heads(c, "k7c_heads", keys, M, &head, &hpos, &n_runs));
        LAUNCH(c, "k5o_lower_bound", k5o_lower_bound, dim3(grid5(G + 1)), dim3(256), 0, G, (const uint64_t*)keys, M, pbits, gstart);
        LAUNCH(c, "k7c_group_count", k7c_group_count, dim3(grid5(G)), dim3(256), 0, G, (const uint64_t*)gstart, (const uint64_t*)hpos, *d_count);
    }
    W2_HIP(hipStreamSynchronize(c.stream));
    for (void* p : {(void*)rlen, (void*)roff, (void*)keys, (void*)vals, (void*)head, (void*)hpos, (void*)gstart}) c.release(p);
    return 0;
}

int coverage(Ctx& c, const w2rap_step7_cov_in& in, const w2rap_step7_cov_params& P, uint32_t parts, w2rap_step7_cov_out& out) {
    const uint64_t E = in.n_edge_objs, NP = in.n_paths / 2, NL = in.n_lines;
    const uint64_t NC = in.line_off[NL], NLP = in.cell_off[NC], NLE = in.lpath_off[NLP];
    // ---- npairs, llens: part LINES of w2rap_step7_links on this context (no adjacency is read there)
    {
        w2rap_step7_in s;
        std::memset(&s, 0, sizeof s);
        s.K = in.K; s.n_edge_objs = E; s.edge_len = in.edge_len; s.inv = in.inv; s.n_paths = in.n_paths; s.path_off = in.path_off; s.path_edges = in.path_edges;
        s.n_lines = NL; s.line_off = in.line_off; s.cell_off = in.cell_off; s.lpath_off = in.lpath_off; s.line_edges = in.line_edges;
        w2rap_step7_out lo;
        std::memset(&lo, 0, sizeof lo);
        const int rc = step7_lines_part(c, s, lo);
        if (rc) { w2rap_step7_free(&lo); return rc; }
        out.llens = lo.llens; out.npairs = lo.npairs; out.ms_lines = lo.ms_lines;
        lo.llens = lo.npairs = nullptr;
        w2rap_step7_free(&lo);
    }
    if (parts < W2RAP_STEP7_COV_PEAK) return 0;

    // ---- covl, the candidates, base_cov (host)
    cov::Candidates C;
    cov::candidates(out.llens, out.npairs, NL, C);
    cov::PeakCounters pc;
    out.base_cov = cov::find_peak(C.covx, C.mass, pc);
    out.max_len = C.max_len; out.min_len = C.min_len; out.n_candidates = C.covx.size();
    W2_TRY(host_copy(c, &out.covl, C.covl)); W2_TRY(host_copy(c, &out.covx, C.covx)); W2_TRY(host_copy(c, &out.mass, C.mass)); W2_TRY(host_copy(c, &out.ids, C.ids));
    out.n_simple = pc.n_simple; out.n_noise = pc.n_noise; out.n_edge = pc.n_edge; out.n_sparse = pc.n_sparse; out.n_not_window_max = pc.n_not_window_max; out.n_shallow = pc.n_shallow;
    out.n_centred = pc.n_centred; out.n_prefiltered = pc.n_prefiltered; out.n_peaks = pc.n_peaks; out.peak_way = pc.way; out.n_score_ties_taken = pc.n_score_ties_taken; out.halved = pc.halved;
    if (parts < W2RAP_STEP7_COV_EDGES) return 0;
    if (NC >= (1ull << 32) - 1) { c.err = "2^32 cells or more"; return W2RAP_E_LIMIT; }

    // ---- the cell groups (host)
    cov::CellGroups G;
    cov::cell_groups(in, G);
    const uint64_t NG = G.line.size(), NGE = G.e.size(), NZ = G.z.size();
    if (NG >= (1ull << 31)) { c.err = "2^31 cell groups or more"; return W2RAP_E_LIMIT; }
    out.n_groups = NG; out.n_cells = G.n_cells; out.n_cells_empty = G.n_cells_empty; out.n_cells_sizes = G.n_cells_sizes; out.n_cells_one_in = G.n_cells_one_in;
    out.n_classes = G.n_classes; out.n_classes_short = G.n_classes_short;
    W2_TRY(host_copy(c, &out.group_line, G.line)); W2_TRY(host_copy(c, &out.group_cell, G.cell)); W2_TRY(host_copy(c, &out.group_len, G.len));
    W2_TRY(host_copy(c, &out.group_z_off, G.z_off)); W2_TRY(host_copy(c, &out.group_z, G.z));
    std::vector<uint32_t> gof(NGE), zgroup(NZ), cell_line(NC);
    for (uint64_t g = 0; g < NG; ++g) {
        for (uint64_t i = G.e_off[g]; i < G.e_off[g + 1]; ++i) gof[i] = (uint32_t)g;
        for (uint64_t i = G.z_off[g]; i < G.z_off[g + 1]; ++i) zgroup[i] = (uint32_t)g;
    }
    for (uint64_t l = 0; l < NL; ++l) { for (uint64_t cl = in.line_off[l]; cl < in.line_off[l + 1]; ++cl) cell_line[cl] = (uint32_t)l; out.n_line_lines += out.llens[l] >= MIN_LINE; }

    // ---- uploads
    uint64_t *d_line_off = nullptr, *d_cell_off = nullptr, *d_lpath_off = nullptr; int32_t *d_ledges = nullptr, *d_inv = nullptr, *d_llens = nullptr, *d_glen = nullptr, *d_gedges = nullptr, *d_z = nullptr;
    uint32_t *d_elen = nullptr, *d_cell_line = nullptr, *d_gof = nullptr, *d_zgroup = nullptr, *d_pos_line = nullptr, *d_pos_cell = nullptr, *d_need = nullptr; double* d_covl = nullptr;
    float* d_cov = nullptr; uint8_t* d_rule = nullptr; uint64_t* d_npos = nullptr; int64_t *d_gcount = nullptr, *d_count1 = nullptr; int32_t* d_gedges1 = nullptr; unsigned long long* d_cnt = nullptr;
    W2_TRY(up_pooled(c, &d_line_off, in.line_off, NL + 1)); W2_TRY(up_pooled(c, &d_cell_off, in.cell_off, NC + 1)); W2_TRY(up_pooled(c, &d_lpath_off, in.lpath_off, NLP + 1));
    W2_TRY(up_pooled(c, &d_ledges, in.line_edges, NLE)); W2_TRY(up_pooled(c, &d_inv, in.inv, E)); W2_TRY(up_pooled(c, &d_elen, in.edge_len, E));
    W2_TRY(up_pooled(c, &d_llens, (const int32_t*)out.llens, NL)); W2_TRY(up_pooled(c, &d_covl, (const double*)C.covl.data(), NL));
    W2_TRY(up_pooled(c, &d_cell_line, (const uint32_t*)cell_line.data(), NC));
    W2_TRY(up_pooled(c, &d_glen, (const int32_t*)G.len.data(), NG)); W2_TRY(up_pooled(c, &d_gedges, (const int32_t*)G.e.data(), NGE)); W2_TRY(up_pooled(c, &d_gof, (const uint32_t*)gof.data(), NGE));
    W2_TRY(up_pooled(c, &d_z, (const int32_t*)G.z.data(), NZ)); W2_TRY(up_pooled(c, &d_zgroup, (const uint32_t*)zgroup.data(), NZ));
    W2_ALLOC(d_pos_line, uint32_t, E + 1); W2_ALLOC(d_pos_cell, uint32_t, E + 1); W2_ALLOC(d_need, uint32_t, E + 1); W2_ALLOC(d_npos, uint64_t, E + 2);
    W2_ALLOC(d_cov, float, E + 1); W2_ALLOC(d_rule, uint8_t, E + 1); W2_ALLOC(d_cnt, unsigned long long, 8);
    W2_HIP(hipMemsetAsync(d_pos_line, 0, (E + 1) * 4, c.stream)); W2_HIP(hipMemsetAsync(d_pos_cell, 0, (E + 1) * 4, c.stream)); W2_HIP(hipMemsetAsync(d_cnt, 0, 8 * 8, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));                    // (the host vectors above have been read)

    // ---- round 1: the distinct pairs of the cell groups
    Index X;
    if (NG) W2_TRY(build_index(c, in, X, out));
    {
        Timer t(c.stream);
        if (NG) W2_TRY(count_groups(c, X, d_inv, d_gedges, d_gof, NGE, NG, NP, &d_gcount, &out.n_group_entries[0]));
        else { W2_ALLOC(d_gcount, int64_t, 1); }
        out.ms_groups += t.stop();
    }
    W2_TRY(dl(c, &out.group_pairs, (const int64_t*)d_gcount, NG));

    // ---- the line rule and the cell rule; which edges the long-edge rule is due for
    const double base = out.base_cov, rbase = 1.0 / base;
    uint64_t NG1 = 0;
    {
        Timer t(c.stream);
        LAUNCH(c, "k7c_line_pos", k7c_line_pos, dim3(grid5(NL)), dim3(256), 0, NL, (const uint64_t*)d_line_off, (const uint64_t*)d_cell_off, (const uint64_t*)d_lpath_off, (const int32_t*)d_ledges,
               (const int32_t*)d_llens, d_pos_line);
        LAUNCH_N(NZ, c, "k7c_cell_pos", k7c_cell_pos, dim3(grid5(NZ)), dim3(256), 0, NZ, (const uint32_t*)d_zgroup, (const int32_t*)d_z, d_pos_cell);
        LAUNCH_N(E, c, "k7c_edge_cov", k7c_edge_cov, dim3(grid5(E)), dim3(256), 0, E, (const uint32_t*)d_pos_line, (const uint32_t*)d_cell_line, (const double*)d_covl, (const uint32_t*)d_pos_cell,
                 (const int64_t*)d_gcount, (const int32_t*)d_glen, base, rbase, (const uint32_t*)d_elen, in.K, d_cov, d_rule, d_need);
        if (E) {
            W2_TRY(exclusive_scan_u32_to_u64(c, d_need, d_npos, E));
            W2_HIP(hipMemcpyAsync(&NG1, d_npos + E, 8, hipMemcpyDeviceToHost, c.stream));
        }
        out.ms_rules += t.stop();
    }
    W2_HIP(hipStreamSynchronize(c.stream));
    out.n_long_asked = NG1;

    // ---- round 2: the long edges, one edge a group
    if (NG1) {
        W2_TRY(build_index(c, in, X, out));
        Timer t(c.stream);
        W2_ALLOC(d_gedges1, int32_t, NG1 + 1);
        LAUNCH(c, "k7c_need_fill", k7c_need_fill, dim3(grid5(E)), dim3(256), 0, E, (const uint32_t*)d_need, (const uint64_t*)d_npos, d_gedges1);
        W2_TRY(count_groups(c, X, d_inv, d_gedges1, nullptr, NG1, NG1, NP, &d_count1, &out.n_group_entries[1], P.long_form != W2RAP_STEP7_LONG_SORTED));
        out.ms_long = t.stop();
        out.ms_groups += out.ms_long;
        W2_TRY(dl(c, &out.long_edge, (const int32_t*)d_gedges1, NG1)); W2_TRY(dl(c, &out.long_pairs, (const int64_t*)d_count1, NG1));
    }
    {
        Timer t(c.stream);
        LAUNCH_N(E, c, "k7c_edge_long", k7c_edge_long, dim3(grid5(E)), dim3(256), 0, E, (const uint32_t*)d_need, (const uint64_t*)d_npos, (const int64_t*)d_count1, (const uint32_t*)d_elen, in.K,
                 base, rbase, P.frac, P.min_edge_size, d_cov, d_rule, d_cnt);
        out.ms_rules += t.stop();
    }
    unsigned long long cnt[8] = {0};
    W2_TRY(dl(c, &out.cov, (const float*)d_cov, E)); W2_TRY(dl(c, &out.rule, (const uint8_t*)d_rule, E));
    W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    for (int r = 0; r < 4; ++r) out.n_rule[r] = cnt[C_RULE0 + r];
    out.n_undefined = cnt[C_UNDEF]; out.n_cn_edges = cnt[C_CN_EDGES]; out.n_cn_good = cnt[C_CN_GOOD];
    out.cn_fraction = double(out.n_cn_good) / double(out.n_cn_edges);
    for (void* p : {(void*)d_line_off, (void*)d_cell_off, (void*)d_lpath_off, (void*)d_ledges, (void*)d_inv, (void*)d_llens, (void*)d_glen, (void*)d_gedges, (void*)d_z, (void*)d_elen,
                    (void*)d_cell_line, (void*)d_gof, (void*)d_zgroup, (void*)d_pos_line, (void*)d_pos_cell, (void*)d_need, (void*)d_covl, (void*)d_cov, (void*)d_rule, (void*)d_npos,
                    (void*)d_gcount, (void*)d_count1, (void*)d_gedges1, (void*)d_cnt, (void*)X.poff, (void*)X.keys, (void*)X.ioff, (void*)X.pe, (void*)X.iread}) c.release(p);
    return 0;
}

constexpr uint32_t ALL_PARTS = W2RAP_STEP7_COV_NPAIRS | W2RAP_STEP7_COV_PEAK | W2RAP_STEP7_COV_EDGES;

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" int w2rap_step7_coverage(const w2rap_step7_cov_in* in, const w2rap_step7_cov_params* P, w2rap_step7_cov_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (const int rc = cov::check(in, P, err, errlen)) return rc;
    const uint32_t f = P->flags ? P->flags : ALL_PARTS;
    const uint32_t parts = f & W2RAP_STEP7_COV_EDGES ? W2RAP_STEP7_COV_EDGES : f & W2RAP_STEP7_COV_PEAK ? W2RAP_STEP7_COV_PEAK : W2RAP_STEP7_COV_NPAIRS;
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return coverage(c, *in, *P, parts, *out); }, save_profile7_shared, [&] { w2rap_step7_coverage_free(out); });
}

extern "C" void w2rap_step7_coverage_free(w2rap_step7_cov_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->npairs, (void*)o->llens, (void*)o->covl, (void*)o->covx, (void*)o->mass, (void*)o->ids, (void*)o->cov, (void*)o->rule, (void*)o->group_line, (void*)o->group_cell,
                    (void*)o->group_len, (void*)o->group_pairs, (void*)o->group_z_off, (void*)o->group_z, (void*)o->long_edge, (void*)o->long_pairs}) std::free(p);
    std::memset(o, 0, sizeof(*o));
}
