// step5_open.hip -- the opening of Step 5: the three passes over all read paths that the reference runs before its first cluster exists.
//
//   INDEX   invert(pathsr, paths_inv, E) (src/VecUtilities.h:693, called at src/modules/w2rap-contigger.cc:427)
//     device  k5o_index_emit / sort / k5o_lower_bound      (edge, read) per path entry in read order; the stable sort by edge leaves the
//                                                          read ids of an edge ascending
//   LINKS   Phase 1 of Unsat (src/paths/long/large/Unsat.cc:142-207)
//     device  k5o_pair_filter / scan / k5o_pair_compact    :152-160: both mates placed, Meet2, v == w; the surviving (v, w, pid)
//     device  k5o_reach                                    :161-176: the bounded search, one wavefront per surviving pair
//     device  k5o_link_count / scan / k5o_link_fill / sort :179-187: two links per unsatisfied pair, ordered by (e, to, pid)
//     device  k5o_lower_bound / k5o_link_out / k5_heads / scan / k5o_kinds / k5o_kind_mult
//                                                          unsats[e] as a CSR; mult (:190-198) = the runs of equal (e, to)
//   LAYOUT  LayoutReads (src/paths/long/large/GapToyTools2.cc:550-588)
//     device  k5o_layout_count / scan / k5o_layout_fill / sort / k5o_lower_bound / k5o_layout_out
//                                                          0, 2 or 4 entries per read in (read, forward-first) order; one stable sort
//                                                          on (edge, pos + 2^31): the emission order is the tie rule
// Integer arithmetic throughout; nothing depends on the order in which reads or pairs are processed.
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "step5_runs.h"
#include "../../include/w2rap_step5.h"

namespace w2 {
namespace {

constexpr unsigned MAX_DEPTH = 15, MAX_VERTS = 50;            // Unsat.cc:131-132
constexpr unsigned REACH_WAVES = 4;                            // surviving pairs per block of k5o_reach
enum { C_PLACED, C_MEET, C_SAME_VERTEX, C_REACHED, C_DEPTH, C_OVERFLOW, C_SAME_END, N_CNT };     // (k5o_pair_filter counts the first three
static_assert(C_MEET == C_PLACED + 1 && C_SAME_VERTEX == C_PLACED + 2 && C_DEPTH == C_REACHED + 1 && C_OVERFLOW == C_REACHED + 2 && C_SAME_END == C_REACHED + 3,
              "as one group, k5o_link_count the last four)");
enum : uint32_t { R_REACHED = 0, R_DEPTH = 1, R_OVERFLOW = 2 };

// word[i] += the threads of the block whose x[i] is set, i < N: the waves' ballots are summed in LDS, then one global atomic per block
// and counter (every thread of the block calls it, once per kernel)
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

// ---- LINKS ---------------------------------------------------------------------------------------------------------------------
// Unsat.cc:152-160.  flag[p] = the pair goes on to the search
__global__ __launch_bounds__(256) void k5o_pair_filter(uint64_t NP, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ inv,
                                                       const int32_t* __restrict__ vleft, const int32_t* __restrict__ vright, uint32_t* __restrict__ flag,
                                                       unsigned long long* __restrict__ cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool placed = false, meet = false, same = false;
    if (p < NP) {
        const uint64_t a0 = poff[2 * p], a1 = poff[2 * p + 1], a2 = poff[2 * p + 2];
        if (a1 > a0 && a2 > a1) {
            placed = true;
            for (uint64_t j = a1; j < a2 && !meet; ++j) {      // Meet2(x1, x2): x2 is inv of p2's edges, in any order
                const int32_t e2 = inv[pe[j]];
                for (uint64_t i = a0; i < a1; ++i) meet |= pe[i] == e2;
            }
            if (!meet) same = vright[pe[a1 - 1]] == vleft[inv[pe[a2 - 1]]];
        }
        flag[p] = placed && !meet && !same;
    }
    const bool what[3] = {placed, meet, same};
    count_block(what, &cnt[C_PLACED]);
}
__global__ __launch_bounds__(256) void k5o_pair_compact(uint64_t NP, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ fpos, const uint64_t* __restrict__ poff,
                                                        const int32_t* __restrict__ pe, const int32_t* __restrict__ inv, const int32_t* __restrict__ vleft,
                                                        const int32_t* __restrict__ vright, int32_t* __restrict__ sv, int32_t* __restrict__ sw, uint32_t* __restrict__ spid) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NP || !flag[p]) return;
    const uint64_t s = fpos[p];
    sv[s] = vright[pe[poff[2 * p + 1] - 1]]; sw[s] = vleft[inv[pe[poff[2 * p + 2] - 1]]]; spid[s] = (uint32_t)p;
}

// Unsat.cc:161-176, one wavefront per pair.  The frontier (at most 50 vertices, a multiset) lies in one LDS row of 64 per wave, double-
// buffered; lane l owns entry l: it walks that vertex's successors, tests each against w and counts them.  A ballot settles "reached"
// -- looked at before the size, so a hit in a level that overflows still wins --, the wave's sum settles "more than 50" before anything
// is written, a wave prefix sum places the successors otherwise.  The waves of a block never meet: no block barrier
__global__ __launch_bounds__(64 * REACH_WAVES) void k5o_reach(uint64_t NS, const int32_t* __restrict__ sv, const int32_t* __restrict__ sw,
                                                              const uint64_t* __restrict__ from_off, const int32_t* __restrict__ from_v, uint32_t* __restrict__ outcome) {
    __shared__ int32_t frontier[REACH_WAVES][2][64];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * REACH_WAVES + wave;
    if (s >= NS) return;                                       // (wave-uniform)
    const int32_t w = sw[s];
    unsigned cur = 0, count = 1;
    if (lane == 0) frontier[wave][0][0] = sv[s];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    uint32_t result = R_DEPTH;
    for (unsigned d = 1; d <= MAX_DEPTH && count; ++d) {       // (an empty level stays empty: the reference falls out of its loop)
        uint64_t b = 0, e = 0;
        bool hit = false;
        if (lane < count) {
            const int32_t x = frontier[wave][cur][lane];
            b = from_off[x]; e = from_off[x + 1];
            for (uint64_t i = b; i < e; ++i) hit |= from_v[i] == w;
        }
        if (__ballot(hit)) { result = R_REACHED; break; }
        const uint32_t deg = (uint32_t)(e - b < MAX_VERTS + 1 ? e - b : MAX_VERTS + 1);      // (saturated: the sum stays small)
        uint32_t inc = deg;
#pragma unroll
        for (unsigned o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        const uint32_t total = __shfl(inc, 63);
        if (total > MAX_VERTS) { result = R_OVERFLOW; break; }
        int32_t* next = frontier[wave][cur ^ 1];
        for (uint32_t k = 0; k < deg; ++k) next[inc - deg + k] = from_v[b + k];               // (total <= 50: inside the row)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        cur ^= 1; count = total;
    }
    if (lane == 0) outcome[s] = result;
}

// Unsat.cc:179-184: links per surviving pair (0 or 2)
__global__ __launch_bounds__(256) void k5o_link_count(uint64_t NS, const uint32_t* __restrict__ outcome, const uint32_t* __restrict__ spid, const uint64_t* __restrict__ poff,
                                                      const int32_t* __restrict__ pe, uint32_t* __restrict__ nlinks, unsigned long long* __restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t r = 0xFFFFFFFFu; bool same_end = false;
    if (s < NS) {
        r = outcome[s];
        if (r != R_REACHED) { const uint64_t p = spid[s]; same_end = pe[poff[2 * p + 1] - 1] == pe[poff[2 * p + 2] - 1]; }
        nlinks[s] = r != R_REACHED && !same_end ? 2u : 0u;
    }
    const bool what[4] = {r == R_REACHED, r == R_DEPTH, r == R_OVERFLOW, same_end};
    count_block(what, &cnt[C_REACHED]);
}
// key = e << ebits | to (ebits = the bits of an edge id: no key bit the sort passes over is idle), value = pid.  Pairs are emitted by ascending pid and the two links of one pair never share (e, to) -- that would
// need p1.back == p2.back --, so one stable sort by key orders the links by (e, to, pid) and there is no duplicate for the reference's
// UniqueSort to remove
__global__ __launch_bounds__(256) void k5o_link_fill(uint64_t NS, const uint32_t* __restrict__ nlinks, const uint64_t* __restrict__ loff, const uint32_t* __restrict__ spid,
                                                     const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ inv,
                                                     unsigned ebits, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= NS || !nlinks[s]) return;
    const uint64_t p = spid[s], o = loff[s];
    const int32_t b1 = pe[poff[2 * p + 1] - 1], b2 = pe[poff[2 * p + 2] - 1];
    keys[o] = (uint64_t)(uint32_t)b1 << ebits | (uint32_t)inv[b2]; vals[o] = (uint32_t)p;
    keys[o + 1] = (uint64_t)(uint32_t)b2 << ebits | (uint32_t)inv[b1]; vals[o + 1] = (uint32_t)p;
}
__global__ __launch_bounds__(256) void k5o_link_out(uint64_t n, const uint64_t* __restrict__ keys, unsigned ebits, int32_t* __restrict__ to) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) to[j] = (int32_t)(keys[j] & ((1ull << ebits) - 1));
}
__global__ __launch_bounds__(256) void k5o_kinds(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint64_t* __restrict__ hpos,
                                                 unsigned ebits, int32_t* __restrict__ kfrom, int32_t* __restrict__ kto, uint64_t* __restrict__ kstart) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (head[j]) { const uint64_t k = hpos[j]; kfrom[k] = (int32_t)(keys[j] >> ebits); kto[k] = (int32_t)(keys[j] & ((1ull << ebits) - 1)); kstart[k] = j; }
    if (j == n - 1) kstart[hpos[n]] = n;
}
__global__ __launch_bounds__(256) void k5o_kind_mult(uint64_t NK, const uint64_t* __restrict__ kstart, uint32_t* __restrict__ mult) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < NK) mult[k] = (uint32_t)(kstart[k + 1] - kstart[k]);
}

// ---- LAYOUT --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k5o_layout_count(uint64_t n, const uint64_t* __restrict__ poff, uint32_t* __restrict__ cnt) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t len = poff[r + 1] - poff[r];
    cnt[r] = len == 0 ? 0u : len == 1 ? 2u : 4u;
}
// GapToyTools2.cc:556-584.  key = edge << 32 | (pos + 2^31), value = the entry's number in emission order
__global__ __launch_bounds__(256) void k5o_layout_fill(uint64_t n, int32_t K, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ offset,
                                                       const uint32_t* __restrict__ rlen, const uint32_t* __restrict__ elen, const int32_t* __restrict__ inv,
                                                       const uint64_t* __restrict__ loff, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       uint32_t* __restrict__ eid, uint8_t* __restrict__ efw) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t a = poff[r], z = poff[r + 1];
    if (a == z) return;
    uint64_t o = loff[r];
    auto put = [&](int32_t e, int32_t pos, bool fw) {
        keys[o] = (uint64_t)(uint32_t)e << 32 | ((uint32_t)pos ^ 0x80000000u); vals[o] = (uint32_t)o; eid[o] = (uint32_t)r; efw[o] = fw; ++o;
    };
    auto kmers = [&](int32_t e) { return (int32_t)elen[e] - K + 1; };
    const int32_t x0 = pe[a], xl = pe[z - 1];
    // forward: the first and the last edge; the interior edges are skipped BEFORE their length comes off (:563), so only x0's does
    put(x0, offset[r], true);
    if (z - a > 1) put(xl, offset[r] - kmers(x0), true);
    // reverse: y = inv of x, reversed; y[0] = inv[xl], y[n-1] = inv[x0]
    const int32_t y0 = inv[xl], yl = inv[x0];
    int32_t len = (int32_t)elen[y0];
    for (uint64_t k = a; k + 1 < z; ++k) len += kmers(inv[pe[k]]);                            // y[1..] = inv of x[n-2..0]
    const int32_t pos = len - (offset[r] + (int32_t)rlen[r]);
    put(y0, pos, false);
    if (z - a > 1) put(yl, pos - kmers(y0), false);
}
__global__ __launch_bounds__(256) void k5o_layout_out(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ eid,
                                                      const uint8_t* __restrict__ efw, int32_t* __restrict__ pos, uint32_t* __restrict__ id, uint8_t* __restrict__ fw) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    pos[j] = (int32_t)((uint32_t)keys[j] ^ 0x80000000u); id[j] = eid[vals[j]]; fw[j] = efw[vals[j]];
}

// ---- the host side -------------------------------------------------------------------------------------------------------------
struct Dev {                                                   // the inputs on the device (each part uploads what it reads)
    uint64_t* poff = nullptr; int32_t* pe = nullptr; int32_t* inv = nullptr;
};

int open_index(Ctx& c, const w2rap_step5_open_in& in, const Dev& d, w2rap_step5_open_out& out) {
    const uint64_t E = in.n_edge_objs, n = in.n_paths, N = n ? in.path_off[n] : 0;
    Timer t(c.stream);
    out.n_index = N;
    if (!N) { out.ms_index = t.stop(); W2_TRY(host_zeros(c, &out.index_off, E + 1)); return host_zeros(c, &out.index_read, 0); }
    uint64_t *d_keys = nullptr, *d_off = nullptr; uint32_t* d_vals = nullptr;
    W2_TRY(paths_index(c, d.poff, d.pe, n, N, E, &d_keys, &d_vals, &d_off));
    out.ms_index = t.stop();
    W2_TRY(dl(c, &out.index_off, (const uint64_t*)d_off, E + 1));
    W2_TRY(dl(c, &out.index_read, (const uint32_t*)d_vals, N));
    W2_HIP(hipStreamSynchronize(c.stream));
    c.release(d_keys); c.release(d_vals); c.release(d_off);
    return 0;
}

int open_links(Ctx& c, const w2rap_step5_open_in& in, const Dev& d, w2rap_step5_open_out& out) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices, NP = in.n_paths / 2;
    auto empty = [&]() -> int {
        W2_TRY(host_zeros(c, &out.link_off, E + 1)); W2_TRY(host_zeros(c, &out.link_to, 0)); W2_TRY(host_zeros(c, &out.link_pid, 0));
        W2_TRY(host_zeros(c, &out.kind_from, 0)); W2_TRY(host_zeros(c, &out.kind_to, 0)); return host_zeros(c, &out.kind_mult, 0);
    };
    if (!NP || !E) return empty();
    // each edge's two vertices, from the adjacency lists (the argument checks have seen every edge once in each)
    std::vector<int32_t> vleft, vright;
    args::edge_ends(in, vleft, vright);
    int32_t *d_vleft = nullptr, *d_vright = nullptr, *d_from_v = nullptr; uint64_t* d_from_off = nullptr;
    W2_TRY(up_pooled(c, &d_vleft, (const int32_t*)vleft.data(), E)); W2_TRY(up_pooled(c, &d_vright, (const int32_t*)vright.data(), E));
    W2_TRY(up_pooled(c, &d_from_off, in.from_off, NV + 1)); W2_TRY(up_pooled(c, &d_from_v, in.from_v, E));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the host vectors above have been read)
    Timer t(c.stream);
    unsigned long long* d_cnt = nullptr; uint32_t* d_flag = nullptr; uint64_t* d_fpos = nullptr;
    W2_ALLOC(d_cnt, unsigned long long, N_CNT); W2_ALLOC(d_flag, uint32_t, NP + 1); W2_ALLOC(d_fpos, uint64_t, NP + 2);
    W2_HIP(hipMemsetAsync(d_cnt, 0, N_CNT * 8, c.stream));
    LAUNCH(c, "k5o_pair_filter", k5o_pair_filter, dim3(grid5(NP)), dim3(256), 0, NP, (const uint64_t*)d.poff, (const int32_t*)d.pe, (const int32_t*)d.inv,
           (const int32_t*)d_vleft, (const int32_t*)d_vright, d_flag, d_cnt);
    W2_TRY(exclusive_scan_u32_to_u64(c, d_flag, d_fpos, NP));
    uint64_t NS = 0, NL = 0, NK = 0;
    const unsigned ebits = bits_for(E);
    W2_HIP(hipMemcpyAsync(&NS, d_fpos + NP, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    uint64_t *d_keys = nullptr; uint32_t* d_vals = nullptr;
    if (NS) {                                                  // (no pair survives the filter: no search, no links)
        int32_t *d_sv = nullptr, *d_sw = nullptr; uint32_t *d_spid = nullptr, *d_outcome = nullptr, *d_nl = nullptr; uint64_t* d_loff = nullptr;
        W2_ALLOC(d_sv, int32_t, NS); W2_ALLOC(d_sw, int32_t, NS); W2_ALLOC(d_spid, uint32_t, NS); W2_ALLOC(d_outcome, uint32_t, NS);
        W2_ALLOC(d_nl, uint32_t, NS + 1); W2_ALLOC(d_loff, uint64_t, NS + 2);
        LAUNCH(c, "k5o_pair_compact", k5o_pair_compact, dim3(grid5(NP)), dim3(256), 0, NP, (const uint32_t*)d_flag, (const uint64_t*)d_fpos, (const uint64_t*)d.poff,
               (const int32_t*)d.pe, (const int32_t*)d.inv, (const int32_t*)d_vleft, (const int32_t*)d_vright, d_sv, d_sw, d_spid);
        LAUNCH(c, "k5o_reach", k5o_reach, dim3(grid5(NS, REACH_WAVES)), dim3(64 * REACH_WAVES), 0, NS, (const int32_t*)d_sv, (const int32_t*)d_sw,
               (const uint64_t*)d_from_off, (const int32_t*)d_from_v, d_outcome);
        LAUNCH(c, "k5o_link_count", k5o_link_count, dim3(grid5(NS)), dim3(256), 0, NS, (const uint32_t*)d_outcome, (const uint32_t*)d_spid, (const uint64_t*)d.poff,
               (const int32_t*)d.pe, d_nl, d_cnt);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_nl, d_loff, NS));
        W2_HIP(hipMemcpyAsync(&NL, d_loff + NS, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        if (NL) {
            W2_ALLOC(d_keys, uint64_t, NL + 1); W2_ALLOC(d_vals, uint32_t, NL + 1);
            LAUNCH(c, "k5o_link_fill", k5o_link_fill, dim3(grid5(NS)), dim3(256), 0, NS, (const uint32_t*)d_nl, (const uint64_t*)d_loff, (const uint32_t*)d_spid,
                   (const uint64_t*)d.poff, (const int32_t*)d.pe, (const int32_t*)d.inv, ebits, d_keys, d_vals);
            W2_TRY(sort_pairs_u64(c, d_keys, d_vals, NL, 0, (int)(2 * ebits)));
        }
        for (void* p : {(void*)d_sv, (void*)d_sw, (void*)d_spid, (void*)d_outcome, (void*)d_nl, (void*)d_loff}) c.release(p);
    }
    unsigned long long cnt[N_CNT] = {0};
    W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (cnt is on the stack: nothing may return with the copy still queued)
    if (NL) {
        uint64_t *d_off = nullptr, *d_kstart = nullptr; int32_t *d_to = nullptr, *d_kfrom = nullptr, *d_kto = nullptr; uint32_t* d_mult = nullptr;
        W2_ALLOC(d_off, uint64_t, E + 2); W2_ALLOC(d_to, int32_t, NL);
        LAUNCH(c, "k5o_lower_bound", k5o_lower_bound, dim3(grid5(E + 1)), dim3(256), 0, E, (const uint64_t*)d_keys, NL, ebits, d_off);
        LAUNCH(c, "k5o_link_out", k5o_link_out, dim3(grid5(NL)), dim3(256), 0, NL, (const uint64_t*)d_keys, ebits, d_to);
        uint32_t* d_head = nullptr; uint64_t* d_hpos = nullptr;
        W2_TRY(run_heads(c, "k5_heads", d_keys, NL, &d_head, &d_hpos, &NK));
        W2_ALLOC(d_kfrom, int32_t, NK); W2_ALLOC(d_kto, int32_t, NK); W2_ALLOC(d_kstart, uint64_t, NK + 1); W2_ALLOC(d_mult, uint32_t, NK);
        LAUNCH(c, "k5o_kinds", k5o_kinds, dim3(grid5(NL)), dim3(256), 0, NL, (const uint64_t*)d_keys, (const uint32_t*)d_head, (const uint64_t*)d_hpos, ebits, d_kfrom, d_kto, d_kstart);
        LAUNCH(c, "k5o_kind_mult", k5o_kind_mult, dim3(grid5(NK)), dim3(256), 0, NK, (const uint64_t*)d_kstart, d_mult);
        out.ms_links = t.stop();
        W2_TRY(dl(c, &out.link_off, (const uint64_t*)d_off, E + 1)); W2_TRY(dl(c, &out.link_to, (const int32_t*)d_to, NL)); W2_TRY(dl(c, &out.link_pid, (const uint32_t*)d_vals, NL));
        W2_TRY(dl(c, &out.kind_from, (const int32_t*)d_kfrom, NK)); W2_TRY(dl(c, &out.kind_to, (const int32_t*)d_kto, NK)); W2_TRY(dl(c, &out.kind_mult, (const uint32_t*)d_mult, NK));
        W2_HIP(hipStreamSynchronize(c.stream));
        for (void* p : {(void*)d_off, (void*)d_to, (void*)d_head, (void*)d_hpos, (void*)d_kfrom, (void*)d_kto, (void*)d_kstart, (void*)d_mult, (void*)d_keys, (void*)d_vals}) c.release(p);
    } else {
        out.ms_links = t.stop();
        W2_HIP(hipStreamSynchronize(c.stream));
        W2_TRY(empty());
    }
    out.n_pairs_placed = cnt[C_PLACED]; out.n_meet = cnt[C_MEET]; out.n_same_vertex = cnt[C_SAME_VERTEX]; out.n_reached = cnt[C_REACHED];
    out.n_unsat_depth = cnt[C_DEPTH]; out.n_unsat_overflow = cnt[C_OVERFLOW]; out.n_unsat_same_end = cnt[C_SAME_END];
    out.n_links = NL; out.n_kinds = NK;
    for (void* p : {(void*)d_vleft, (void*)d_vright, (void*)d_from_off, (void*)d_from_v, (void*)d_cnt, (void*)d_flag, (void*)d_fpos}) c.release(p);
    return 0;
}

int open_layout(Ctx& c, const w2rap_step5_open_in& in, const Dev& d, w2rap_step5_open_out& out) {
    const uint64_t E = in.n_edge_objs, n = in.n_paths;
    auto empty = [&]() -> int {
        W2_TRY(host_zeros(c, &out.layout_off, E + 1)); W2_TRY(host_zeros(c, &out.layout_pos, 0)); W2_TRY(host_zeros(c, &out.layout_id, 0));
        return host_zeros(c, &out.layout_fw, 0);
    };
    if (!n || !E) return empty();
    int32_t* d_offset = nullptr; uint32_t *d_rlen = nullptr, *d_elen = nullptr;
    W2_TRY(up_pooled(c, &d_offset, in.path_offset, n)); W2_TRY(up_pooled(c, &d_rlen, in.read_len, n)); W2_TRY(up_pooled(c, &d_elen, in.edge_len, E));
    Timer t(c.stream);
    uint32_t* d_cnt = nullptr; uint64_t* d_loff = nullptr; uint64_t N = 0;
    W2_ALLOC(d_cnt, uint32_t, n + 1); W2_ALLOC(d_loff, uint64_t, n + 2);
    LAUNCH(c, "k5o_layout_count", k5o_layout_count, dim3(grid5(n)), dim3(256), 0, n, (const uint64_t*)d.poff, d_cnt);
    W2_TRY(exclusive_scan_u32_to_u64(c, d_cnt, d_loff, n));
    W2_HIP(hipMemcpyAsync(&N, d_loff + n, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    out.n_layout = N;
    if (N) {
        uint64_t *d_keys = nullptr, *d_off = nullptr; uint32_t *d_vals = nullptr, *d_eid = nullptr, *d_id = nullptr; uint8_t *d_efw = nullptr, *d_fw = nullptr; int32_t* d_pos = nullptr;
        W2_ALLOC(d_keys, uint64_t, N + 1); W2_ALLOC(d_vals, uint32_t, N + 1); W2_ALLOC(d_eid, uint32_t, N); W2_ALLOC(d_efw, uint8_t, N);
        W2_ALLOC(d_off, uint64_t, E + 2); W2_ALLOC(d_pos, int32_t, N); W2_ALLOC(d_id, uint32_t, N); W2_ALLOC(d_fw, uint8_t, N);
        LAUNCH(c, "k5o_layout_fill", k5o_layout_fill, dim3(grid5(n)), dim3(256), 0, n, in.K, (const uint64_t*)d.poff, (const int32_t*)d.pe, (const int32_t*)d_offset,
               (const uint32_t*)d_rlen, (const uint32_t*)d_elen, (const int32_t*)d.inv, (const uint64_t*)d_loff, d_keys, d_vals, d_eid, d_efw);
        W2_TRY(sort_pairs_u64(c, d_keys, d_vals, N, 0, (int)(32 + bits_for(E))));
        LAUNCH(c, "k5o_lower_bound", k5o_lower_bound, dim3(grid5(E + 1)), dim3(256), 0, E, (const uint64_t*)d_keys, N, 32u, d_off);
        LAUNCH(c, "k5o_layout_out", k5o_layout_out, dim3(grid5(N)), dim3(256), 0, N, (const uint64_t*)d_keys, (const uint32_t*)d_vals, (const uint32_t*)d_eid,
               (const uint8_t*)d_efw, d_pos, d_id, d_fw);
        out.ms_layout = t.stop();
        W2_TRY(dl(c, &out.layout_off, (const uint64_t*)d_off, E + 1)); W2_TRY(dl(c, &out.layout_pos, (const int32_t*)d_pos, N));
        W2_TRY(dl(c, &out.layout_id, (const uint32_t*)d_id, N)); W2_TRY(dl(c, &out.layout_fw, (const uint8_t*)d_fw, N));
        W2_HIP(hipStreamSynchronize(c.stream));
        for (void* p : {(void*)d_keys, (void*)d_vals, (void*)d_eid, (void*)d_efw, (void*)d_off, (void*)d_pos, (void*)d_id, (void*)d_fw}) c.release(p);
    } else {
        out.ms_layout = t.stop();
        W2_TRY(empty());
    }
    for (void* p : {(void*)d_offset, (void*)d_rlen, (void*)d_elen, (void*)d_cnt, (void*)d_loff}) c.release(p);
    return 0;
}

int opening(Ctx& c, const w2rap_step5_open_in& in, uint32_t parts, w2rap_step5_open_out& out) {
    const uint64_t E = in.n_edge_objs, n = in.n_paths, npe = n ? in.path_off[n] : 0;
    Dev d;
    static const uint64_t zero = 0;
    W2_TRY(up_pooled(c, &d.poff, n ? in.path_off : &zero, n + 1));
    W2_TRY(up_pooled(c, &d.pe, in.path_edges, npe));
    W2_TRY(up_pooled(c, &d.inv, in.inv, E));
    if (parts & W2RAP_STEP5_OPEN_INDEX) W2_TRY(open_index(c, in, d, out));
    if (parts & W2RAP_STEP5_OPEN_LINKS) W2_TRY(open_links(c, in, d, out));
    if (parts & W2RAP_STEP5_OPEN_LAYOUT) W2_TRY(open_layout(c, in, d, out));
    W2_HIP(hipStreamSynchronize(c.stream));
    c.release(d.poff); c.release(d.pe); c.release(d.inv);
    return 0;
}

// The argument checks: 0, or W2RAP_E_ARG with the message in `err`.  Everything a kernel uses as an index is looked at here
int open_check(const w2rap_step5_open_in* in, const w2rap_step5_params* P, char* err, size_t errlen) {
    auto fail = [&](int code, const char* m) { if (err && errlen) std::snprintf(err, errlen, "%s", m); return code; };
    if (!in || !P) return fail(W2RAP_E_ARG, "null argument");
    if (P->flags & ~(W2RAP_STEP5_OPEN_INDEX | W2RAP_STEP5_OPEN_LINKS | W2RAP_STEP5_OPEN_LAYOUT)) return fail(W2RAP_E_ARG, "unknown flag");
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640]");
    const uint64_t E = in->n_edge_objs;
    if (args::too_large(*in, 1ull << 30)) return fail(W2RAP_E_ARG, "more than 2^31 edge objects or vertices, or 2^30 reads: ids are 32-bit");
    if (in->n_paths & 1) return fail(W2RAP_E_ARG, args::ODD_PATHS);
    W2_ARGS(args::null_arrays(*in, !in->inv));
    W2_ARGS(args::edge_lens(*in, 1ull << 31));
    W2_ARGS(args::adjacency(*in));
    for (uint64_t e = 0; e < E; ++e) if (in->inv[e] < 0 || (uint64_t)in->inv[e] >= E) return fail(W2RAP_E_ARG, "inv names an edge object that does not exist");
    for (uint64_t e = 0; e < E; ++e) if ((uint64_t)in->inv[in->inv[e]] != e) return fail(W2RAP_E_ARG, "inv is not an involution: inv[inv[e]] != e");
    W2_ARGS(args::reads_and_paths(*in));
    return 0;
}

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" int w2rap_step5_open(const w2rap_step5_open_in* in, const w2rap_step5_params* P, w2rap_step5_open_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (const int rc = open_check(in, P, err, errlen)) return rc;
    const uint32_t parts = P->flags ? P->flags : (W2RAP_STEP5_OPEN_INDEX | W2RAP_STEP5_OPEN_LINKS | W2RAP_STEP5_OPEN_LAYOUT);
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return opening(c, *in, parts, *out); }, save_profile5, [&] { w2rap_step5_open_free(out); });
}

extern "C" void w2rap_step5_open_free(w2rap_step5_open_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->index_off, (void*)o->index_read, (void*)o->link_off, (void*)o->link_to, (void*)o->link_pid, (void*)o->kind_from, (void*)o->kind_to,
                    (void*)o->kind_mult, (void*)o->layout_off, (void*)o->layout_pos, (void*)o->layout_id, (void*)o->layout_fw}) std::free(p);
    std::memset(o, 0, sizeof(*o));
}
