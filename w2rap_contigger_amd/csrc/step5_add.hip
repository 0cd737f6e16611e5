// step5_add.hip -- AddNewStuff (src/paths/long/large/GapToyTools4.cc:133-368), the call in front of PartnersToEnds and the only place in
// Step 5 where the graph changes, on gfx950; C ABI in include/w2rap_step5.h (w2rap_step5_add_new_stuff).
//
//   reference                                              here
//   BuildAll + append(new_stuff)  :131-161, :238-241       k5a_junction_count, scan, k5a_layout, scans, k5a_fill: allx is written straight
//                                                          into the 2-bit word stream Step 3's dictionary stage reads
//   buildBigKHBVFromReads         :247                     step3_back / step3_through / step3_pack (step3_back.h): the builder RepathInMemory
//                                                          calls, shared, not copied
//   to3, left3                    :252-256                 k5a_map: sequence e's path and first skip, e an old edge object
//   TranslatePaths                :164-197                 k5a_tr_bound, scan, k5a_translate (thread per read; the OverlapAppend-ed vector of
//                                                          a read that has to walk lies in a scanned scratch array)
//   ExtendPath, mode 1            :289-356                 k5a_ext_pre (thread per read: the early returns), scan, k5a_ext_compact, k5a_extend
//                                                          (a wavefront per surviving read: the list in LDS, the lanes stride over the read's
//                                                          last `ext` bases), scan of the new lengths, k5a_ext_write
// Integer arithmetic throughout; nothing depends on the order in which reads are processed.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "step3_back.h"
#include "step5_runs.h"
#include "../../include/w2rap_step5.h"

namespace w2 {
namespace {

static inline unsigned grid_a(uint64_t n) { return (unsigned)((n + 255) / 256); }

// 2-bit sequences packed four bases to a byte, base p at bits 2(p&3) of byte p>>2; every buffer has 16 readable bytes behind it
__device__ inline unsigned a_base(const uint8_t* __restrict__ s, uint64_t pos) { return (s[pos >> 2] >> (2 * (pos & 3))) & 3u; }
__device__ inline uint64_t a_stream64(const uint8_t* __restrict__ s, uint64_t pos) {      // 32 bases from base position pos
    const uint64_t b = pos >> 2; const unsigned sh = 2 * (unsigned)(pos & 3);
    uint64_t x = reinterpret_cast<const U64u*>(s + b)->v;
    if (sh) x = (x >> sh) | ((uint64_t)s[b + 8] << (64 - sh));
    return x;
}
// largest i in [0, n) with a[i] <= x (a ascending, a[0] <= x)
__device__ inline uint64_t a_upper(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t m = (lo + hi) >> 1; if (a[m] <= x) lo = m; else hi = m; }
    return lo;
}
// one atomic per wavefront for a counter every lane may bump
__device__ inline void a_count(unsigned long long* cnt, bool mine) {
    const unsigned long long m = __ballot(mine);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(cnt, (unsigned long long)__popcll(m));
}

// ============================================================================= allx (BuildAll :131-161)
__global__ void __launch_bounds__(256) k5a_junction_count(uint64_t NV, const uint64_t* __restrict__ to_off, const uint64_t* __restrict__ from_off, uint32_t* __restrict__ cnt) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= NV) return;
    cnt[v] = (uint32_t)((to_off[v + 1] - to_off[v]) * (from_off[v + 1] - from_off[v]));
}
// sequence u of allx: an edge (u < E), a junction (u < E + NJ), a piece of new_stuff
__global__ void __launch_bounds__(256) k5a_layout(uint64_t U, uint64_t E, uint64_t NJ, unsigned K, const uint32_t* __restrict__ elen, const uint32_t* __restrict__ nlen,
                                                   uint32_t* __restrict__ nbases, uint32_t* __restrict__ nwords, uint32_t* __restrict__ nkm) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const uint32_t L = u < E ? elen[u] : u < E + NJ ? K + 1 : nlen[u - E - NJ];
    nbases[u] = L; nwords[u] = (L + 31) / 32 + 1; nkm[u] = L >= K ? L - K + 1 : 0;
}
// one thread per 32-base word of the stream
__global__ void __launch_bounds__(256) k5a_fill(uint64_t nwords_total, uint64_t U, uint64_t E, uint64_t NJ, uint64_t NV, unsigned K, const uint64_t* __restrict__ woff,
                                                 const uint32_t* __restrict__ nbases, const uint8_t* __restrict__ ebits, const uint64_t* __restrict__ ebyte,
                                                 const uint32_t* __restrict__ elen, const uint64_t* __restrict__ joff, const uint64_t* __restrict__ to_off,
                                                 const int32_t* __restrict__ to_e, const uint64_t* __restrict__ from_off, const int32_t* __restrict__ from_e,
                                                 const uint8_t* __restrict__ nbits, const uint64_t* __restrict__ nbyte, uint64_t* __restrict__ all) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords_total) return;
    const uint64_t u = a_upper(woff, U, w);
    const uint32_t L = nbases[u];
    const uint64_t t0 = (w - woff[u]) * 32;
    uint64_t out = 0;
    if (t0 < L) {
        const uint32_t n = L - t0 < 32 ? (uint32_t)(L - t0) : 32;
        if (u < E) out = a_stream64(ebits, 4 * ebyte[u] + t0);
        else if (u >= E + NJ) out = a_stream64(nbits, 4 * nbyte[u - E - NJ] + t0);
        else {
            const uint64_t j = u - E, v = a_upper(joff, NV, j), r = j - joff[v];
            const uint64_t nf = from_off[v + 1] - from_off[v];
            const int e1 = to_e[to_off[v] + r / nf], e2 = from_e[from_off[v] + r % nf];
            const uint64_t src = 4 * ebyte[e1] + elen[e1] - K;           // the last K bases of e1 ...
            if (t0 + n <= K) out = a_stream64(ebits, src + t0);
            else {                                                       // ... and base K-1 of e2 as base K
                for (uint32_t i = 0; i < n; ++i) {
                    const uint64_t t = t0 + i;
                    out |= (uint64_t)(t < K ? a_base(ebits, src + t) : a_base(ebits, 4 * ebyte[e2] + K - 1)) << (2 * i);
                }
            }
        }
        if (n < 32) out &= (1ull << (2 * n)) - 1;
    }
    all[w] = out;
}

// ============================================================================= to3, left3 (:252-256)
__global__ void __launch_bounds__(256) k5a_map(uint64_t E, const uint64_t* __restrict__ koff, const uint64_t* __restrict__ oex, const int32_t* __restrict__ starts,
                                                uint64_t* __restrict__ t3off, int32_t* __restrict__ left3) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > E) return;
    t3off[e] = oex[koff[e]];
    if (e < E) left3[e] = starts[e];        // (an edge has a K-mer: starts is set.  getFirstSkip: never negative)
}

// ============================================================================= TranslatePaths (:164-197)
struct Tr { uint64_t n; unsigned K; const int32_t* p_offset; const uint64_t* p_off; const int32_t* p_edges; const uint64_t* t3off; const int32_t* to3;
            const int32_t* left3; const uint32_t* olen; };
// how a read goes through: 0 empty, 1 cleared at once (its first edge maps to nothing), 2 one edge at `start`, 3 has to walk
__device__ inline int tr_kind(const Tr& T, uint64_t r, int* start) {
    const uint64_t a = T.p_off[r];
    if (T.p_off[r + 1] == a) return 0;
    const int e0 = T.p_edges[a];
    *start = T.p_offset[r] + T.left3[e0];
    if (T.t3off[e0 + 1] == T.t3off[e0]) return 1;
    if (*start < (int)T.olen[T.to3[T.t3off[e0]]]) return 2;
    return 3;
}
__global__ void __launch_bounds__(256) k5a_tr_bound(Tr T, uint32_t* __restrict__ bound) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= T.n) return;
    int start; uint32_t b = 0;
    if (tr_kind(T, r, &start) == 3)
        for (uint64_t k = T.p_off[r]; k < T.p_off[r + 1]; ++k) {
            const int e = T.p_edges[k]; const uint32_t m = (uint32_t)(T.t3off[e + 1] - T.t3off[e]);
            if (!m) break;
            b += m;
        }
    bound[r] = b;
}
// out: t_edge[r] (-1: no path), t_offset[r]; cnt[0..3] = empty, first, walked, cleared
__global__ void __launch_bounds__(256) k5a_translate(Tr T, const uint64_t* __restrict__ soff, int32_t* __restrict__ scratch, int32_t* __restrict__ t_edge,
                                                      int32_t* __restrict__ t_offset, unsigned long long* __restrict__ cnt) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int kind = -1, edge = -1, off = 0;
    if (r < T.n) {
        int start = 0;
        kind = tr_kind(T, r, &start);
        off = T.p_offset[r];                                   // clear() leaves the offset as it was (ReadPath derives from std::vector)
        if (kind == 2) { edge = T.to3[T.t3off[T.p_edges[T.p_off[r]]]]; off = start; kind = 1; }
        else if (kind == 1) kind = 3;
        else if (kind == 3) {
            int32_t* p = scratch + soff[r]; uint32_t np = 0;
            for (uint64_t k = T.p_off[r]; k < T.p_off[r + 1]; ++k) {
                const int e = T.p_edges[k]; const int32_t* v2 = T.to3 + T.t3off[e]; const uint32_t m = (uint32_t)(T.t3off[e + 1] - T.t3off[e]);
                if (!m) break;
                uint32_t best = 0;                             // OverlapAppend (Vec.h:612): the longest suffix of p that is a prefix of v2
                for (uint32_t ov = np < m ? np : m; ov; --ov) {
                    bool eq = true;
                    for (uint32_t i = 0; i < ov && eq; ++i) eq = p[np - ov + i] == v2[i];
                    if (eq) { best = ov; break; }
                }
                for (uint32_t i = best; i < m; ++i) p[np++] = v2[i];
            }
            uint32_t trim = 0;
            while (start >= (int)T.olen[p[trim]]) {
                start -= (int)T.olen[p[trim]] - (int)T.K + 1;
                if (++trim == np) break;
            }
            if (trim == np) kind = 3;
            else { edge = p[trim]; off = start; kind = 2; }
        }
        t_edge[r] = edge; t_offset[r] = off;
    }
    a_count(cnt + 0, kind == 0); a_count(cnt + 1, kind == 1); a_count(cnt + 2, kind == 2); a_count(cnt + 3, kind == 3);
}

// ============================================================================= ExtendPath, mode 1 (:289-356), on paths of one edge
struct Gr { unsigned K; const uint32_t* olen; const int32_t* right; const uint64_t* from_off; const int32_t* from_e; const uint8_t* obits; const uint64_t* obyte; };
// the early returns; flag[r] = 1: the read goes on to the search.  newlen[r] = 0 or 1 for now
__global__ void __launch_bounds__(256) k5a_ext_pre(uint64_t n, Gr G, const int32_t* __restrict__ t_edge, const int32_t* __restrict__ t_offset, const uint32_t* __restrict__ rlen,
                                                    uint32_t* __restrict__ flag, uint32_t* __restrict__ newlen) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int e = t_edge[r]; uint32_t f = 0;
    if (e >= 0) {
        const int start = t_offset[r];
        if (start >= 0) {
            const int ext = (int)rlen[r] - ((int)G.olen[e] - start);
            const int v = G.right[e];
            if (ext > 0 && G.from_off[v + 1] > G.from_off[v]) f = 1;
        }
    }
    flag[r] = f; newlen[r] = e >= 0 ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k5a_ext_compact(uint64_t n, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ pos, uint32_t* __restrict__ ids) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && flag[r]) ids[pos[r]] = (uint32_t)r;
}

// The reference gives up when its index passes 100, which happens exactly when the list comes to hold 102 entries (entry 0, the empty
// extension, included): 101 slots, and a push into a full list means "unchanged" at any out-degree.
constexpr int EXT_SLOTS = 101;
struct ExtList { int edge[EXT_SLOTS]; int len[EXT_SLOTS]; short parent[EXT_SLOTS]; };
// one lane builds the list in the reference's order (an entry whose length covers `ext` is not expanded); -> its size, or -1: too many
__device__ inline int ext_build(ExtList& X, const Gr& G, int v, int ext) {
    int cnt = 1;
    X.edge[0] = -1; X.len[0] = 0; X.parent[0] = -1;
    for (int j = 0; j < cnt; ++j) {
        if (X.len[j] >= ext) continue;
        const int y = j ? G.right[X.edge[j]] : v;
        for (uint64_t l = G.from_off[y]; l < G.from_off[y + 1]; ++l) {
            if (cnt == EXT_SLOTS) return -1;
            const int nn = G.from_e[l];
            X.edge[cnt] = nn; X.len[cnt] = X.len[j] + (int)G.olen[nn] - (int)G.K + 1; X.parent[cnt] = (short)j;
            ++cnt;
        }
    }
    return cnt;
}
__device__ inline int wave_sum(int x) {
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
// result[w]: 0 too many, 1 no cover, 2 ambiguous, 3 extended; bestj[w] = the chosen list entry, newlen[read] = 1 + its depth; cnt[0..3] by result
__global__ void __launch_bounds__(256) k5a_extend(uint64_t nc, const uint32_t* __restrict__ ids, Gr G, int min_gain, const int32_t* __restrict__ t_edge,
                                                   const int32_t* __restrict__ t_offset, const uint8_t* __restrict__ rbits, const uint64_t* __restrict__ rbyte,
                                                   const uint32_t* __restrict__ rlen, const uint8_t* __restrict__ quals, const uint64_t* __restrict__ qoff,
                                                   uint8_t* __restrict__ result, uint8_t* __restrict__ bestj, uint32_t* __restrict__ newlen,
                                                   unsigned long long* __restrict__ cnt) {
    __shared__ ExtList s_list[4];
    __shared__ int s_cnt[4];
    const unsigned wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wv;
    const bool valid = w < nc;
    ExtList& X = s_list[wv];
    uint32_t r = 0; int ext = 0, n = 0;
    if (valid) {
        r = ids[w];
        const int e = t_edge[r];
        n = (int)rlen[r];
        ext = n - ((int)G.olen[e] - t_offset[r]);
        if (lane == 0) s_cnt[wv] = ext_build(X, G, G.right[e], ext);
    }
    __syncthreads();                                               // (the only one: from here on the list is read, never written)
    if (!valid) return;
    const int cntl = s_cnt[wv];
    int res = 0, best_j = 0;
    if (cntl >= 0) {
        const uint64_t rb = 4 * rbyte[r] + (uint64_t)(n - ext); const uint8_t* q = quals + qoff[r] + (n - ext);
        int ncover = 0, best = 0x7FFFFFFF, second = 0x7FFFFFFF;
        for (int j = 1; j < cntl; ++j) {
            if (X.len[j] < ext) continue;
            int sum = 0;
            for (int k = j; k > 0; k = X.parent[k]) {              // piece k holds the bases [len[parent], len[k]) of the extension: its edge from base K-1 on
                const int lo = X.len[X.parent[k]]; const int hi = X.len[k] < ext ? X.len[k] : ext;
                const uint64_t eb = 4 * G.obyte[X.edge[k]] + (G.K - 1);
                for (int m = lo + (int)lane; m < hi; m += 64)
                    if (a_base(rbits, rb + m) != a_base(G.obits, eb + (m - lo))) sum += q[m];
            }
            sum = wave_sum(sum);
            ++ncover;
            if (sum < best) { second = best; best = sum; best_j = j; }
            else if (sum < second) second = sum;
        }
        // (min_gain >= 1: a tie for the best gives second - best = 0 and never extends, so which of the two SortSync puts first cannot matter)
        res = !ncover ? 1 : (ncover >= 2 && second - best < min_gain) ? 2 : 3;
    }
    if (lane == 0) {
        result[w] = (uint8_t)res; bestj[w] = (uint8_t)best_j;
        if (res == 3) {
            uint32_t depth = 0;
            for (int k = best_j; k > 0; k = X.parent[k]) ++depth;
            newlen[r] = 1 + depth;
        }
        atomicAdd(cnt + res, 1ull);
    }
}
// the new paths: every read's one edge ...
__global__ void __launch_bounds__(256) k5a_write_first(uint64_t n, const int32_t* __restrict__ t_edge, const uint64_t* __restrict__ ooff, int32_t* __restrict__ o_edges) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && t_edge[r] >= 0) o_edges[ooff[r]] = t_edge[r];
}
// ... and behind it the chosen extension of an extended read.  The list is a function of the graph, the edge and ext: lane 0 of the read's
// wavefront builds it again in LDS and walks the chosen entry's parents
__global__ void __launch_bounds__(256) k5a_ext_write(uint64_t nc, const uint32_t* __restrict__ ids, Gr G, const int32_t* __restrict__ t_edge, const int32_t* __restrict__ t_offset,
                                                      const uint32_t* __restrict__ rlen, const uint8_t* __restrict__ result, const uint8_t* __restrict__ bestj,
                                                      const uint32_t* __restrict__ newlen, const uint64_t* __restrict__ ooff, int32_t* __restrict__ o_edges) {
    __shared__ ExtList s_list[4];
    const unsigned wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wv;
    if (w >= nc || lane || result[w] != 3) return;
    ExtList& X = s_list[wv];
    const uint32_t r = ids[w];
    const int e = t_edge[r];
    const int ext = (int)rlen[r] - ((int)G.olen[e] - t_offset[r]);
    ext_build(X, G, G.right[e], ext);
    uint32_t at = newlen[r] - 1;
    for (int k = bestj[w]; k > 0; k = X.parent[k]) o_edges[ooff[r] + at--] = X.edge[k];
}


int add_new_stuff(Ctx& c, const w2rap_step5_in& in, uint64_t n_new, const uint8_t* new_packed, const uint64_t* new_byte_off, const uint32_t* new_len,
                  const w2rap_step5_add_params& P, w2rap_step5_add_out& out) {
    hipStream_t st = c.stream;
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices, n = in.n_paths, npe = n ? in.path_off[n] : 0;
    const unsigned K = (unsigned)in.K;
    // ---- upload
    uint8_t *d_ebits = nullptr, *d_nbits = nullptr, *d_rbits = nullptr, *d_quals = nullptr;
    uint64_t *d_ebyte = nullptr, *d_nbyte = nullptr, *d_rbyte = nullptr, *d_qoff = nullptr, *d_poff = nullptr, *d_from_off = nullptr, *d_to_off = nullptr;
    uint32_t *d_elen = nullptr, *d_nlen = nullptr, *d_rlen = nullptr;
    int32_t *d_from_e = nullptr, *d_to_e = nullptr, *d_poffset = nullptr, *d_pe = nullptr;
    W2_TRY(up_pooled(c, &d_ebits, in.edge_packed, E ? in.edge_byte_off[E] : 0, 32));
    W2_TRY(up_pooled(c, &d_ebyte, in.edge_byte_off, in.edge_byte_off ? E + 1 : 0));
    W2_TRY(up_pooled(c, &d_elen, in.edge_len, E));
    W2_TRY(up_pooled(c, &d_from_off, in.from_off, in.from_off ? NV + 1 : 0));
    W2_TRY(up_pooled(c, &d_to_off, in.to_off, in.to_off ? NV + 1 : 0));
    W2_TRY(up_pooled(c, &d_from_e, in.from_e, E));
    W2_TRY(up_pooled(c, &d_to_e, in.to_e, E));
    W2_TRY(up_pooled(c, &d_nbits, new_packed, n_new ? new_byte_off[n_new] : 0, 32));
    W2_TRY(up_pooled(c, &d_nbyte, new_byte_off, new_byte_off ? n_new + 1 : 0));
    W2_TRY(up_pooled(c, &d_nlen, new_len, n_new));
    W2_TRY(up_pooled(c, &d_rbits, in.read_packed, n ? in.read_byte_off[n] : 0, 16));
    W2_TRY(up_pooled(c, &d_rbyte, in.read_byte_off, in.read_byte_off ? n + 1 : 0));
    W2_TRY(up_pooled(c, &d_rlen, in.read_len, n));
    W2_TRY(up_pooled(c, &d_quals, in.quals, n ? in.qual_off[n] : 0, 16));
    W2_TRY(up_pooled(c, &d_qoff, in.qual_off, in.qual_off ? n + 1 : 0));
    W2_TRY(up_pooled(c, &d_poffset, in.path_offset, n));
    W2_TRY(up_pooled(c, &d_poff, in.path_off, in.path_off ? n + 1 : 0));
    W2_TRY(up_pooled(c, &d_pe, in.path_edges, npe));
    uint32_t* d_flags = nullptr; unsigned long long* d_cnt = nullptr;      // as step3_back wants them; d_cnt[0..3] translate, [8..11] extend
    W2_ALLOC(d_flags, uint32_t, 8); W2_ALLOC(d_cnt, unsigned long long, 112);
    W2_HIP(hipMemsetAsync(d_flags, 0, 32, st)); W2_HIP(hipMemsetAsync(d_cnt, 0, 112 * 8, st));
    // ---------------------------------------------------------------- allx
    Timer t_all(st);
    uint32_t* jcnt = nullptr; uint64_t* joff = nullptr;
    W2_ALLOC(jcnt, uint32_t, NV + 1); W2_ALLOC(joff, uint64_t, NV + 2);
    if (NV) LAUNCH(c, "k5a_junction_count", k5a_junction_count, dim3(grid_a(NV)), dim3(256), 0, NV, (const uint64_t*)d_to_off, (const uint64_t*)d_from_off, jcnt);
    W2_TRY(exclusive_scan_u32_to_u64(c, jcnt, joff, NV));
    uint64_t NJ = 0;
    W2_HIP(hipMemcpy(&NJ, joff + NV, 8, hipMemcpyDeviceToHost));
    const uint64_t U = E + NJ + n_new;
    if (U >= (1ull << 32) - 2) { c.err = "more than 2^32 sequences in allx"; return W2RAP_E_LIMIT; }
    uint32_t *nbases, *nwordsU, *nkm; uint64_t *woff, *koff;
    W2_ALLOC(nbases, uint32_t, U + 1); W2_ALLOC(nwordsU, uint32_t, U + 1); W2_ALLOC(nkm, uint32_t, U + 1); W2_ALLOC(woff, uint64_t, U + 2); W2_ALLOC(koff, uint64_t, U + 2);
    if (U) LAUNCH(c, "k5a_layout", k5a_layout, dim3(grid_a(U)), dim3(256), 0, U, E, NJ, K, (const uint32_t*)d_elen, (const uint32_t*)d_nlen, nbases, nwordsU, nkm);
    W2_TRY(exclusive_scan_u32_to_u64(c, nwordsU, woff, U));
    W2_TRY(exclusive_scan_u32_to_u64(c, nkm, koff, U));
    uint64_t nwords_all = 0, N2 = 0;
    W2_HIP(hipMemcpy(&nwords_all, woff + U, 8, hipMemcpyDeviceToHost));
    W2_HIP(hipMemcpy(&N2, koff + U, 8, hipMemcpyDeviceToHost));
    if (N2 >= (1ull << 32) - 2 || nwords_all * 32 >= (1ull << 40)) { c.err = "more than 2^32 K-mer occurrences in allx (32-bit occurrence ids)"; return W2RAP_E_LIMIT; }
    uint64_t* all = nullptr;
    W2_ALLOC(all, uint64_t, nwords_all + 4);
    W2_HIP(hipMemsetAsync(all + nwords_all, 0, 32, st));
    if (nwords_all) LAUNCH(c, "k5a_fill", k5a_fill, dim3(grid_a(nwords_all)), dim3(256), 0, nwords_all, U, E, NJ, NV, K, (const uint64_t*)woff, (const uint32_t*)nbases,
                           (const uint8_t*)d_ebits, (const uint64_t*)d_ebyte, (const uint32_t*)d_elen, (const uint64_t*)joff, (const uint64_t*)d_to_off, (const int32_t*)d_to_e,
                           (const uint64_t*)d_from_off, (const int32_t*)d_from_e, (const uint8_t*)d_nbits, (const uint64_t*)d_nbyte, all);
    uint32_t* kblk = nullptr;
    W2_TRY(step3_block_index(c, koff, U, N2 ? N2 : 1, &kblk));
    out.n_all = U; out.n_junctions = NJ; out.n_kmer_instances = N2;
    {   // the sum of the lengths of allx: the total of one more scan
        uint64_t* boff = nullptr;
        W2_ALLOC(boff, uint64_t, U + 2);
        W2_TRY(exclusive_scan_u32_to_u64(c, nbases, boff, U));
        W2_HIP(hipMemcpy(&out.n_all_bases, boff + U, 8, hipMemcpyDeviceToHost));
        c.release(boff);
    }
    out.ms_all = t_all.stop();
    // ---------------------------------------------------------------- the graph of allx: Step 3's back half (no UNIQUE_KMERS shortcut: new_stuff repeats the graph's K-mers)
    const Stream3 S3{U, N2, all, woff, nbases, koff, kblk};
    Back3 B;
    W2_TRY(step3_back(c, K, S3, nullptr, P.edge_order_hint, d_flags, d_cnt, B));
    out.ms_dict = B.ms_dict; out.ms_graph = B.ms_graph;
    out.n_kmers_distinct = B.D; out.n_unipaths = B.E;
    // ---------------------------------------------------------------- to3 / left3, TranslatePaths
    Timer t_tr(st);
    W2_TRY(step3_through(c, S3, B));
    W2_TRY(step3_pack(c, K, B));
    const uint64_t NO2 = B.NO2, NV2 = B.NV;
    uint64_t* t3off = nullptr; int32_t* left3 = nullptr;
    W2_ALLOC(t3off, uint64_t, E + 2); W2_ALLOC(left3, int32_t, E + 1);
    LAUNCH(c, "k5a_map", k5a_map, dim3(grid_a(E + 1)), dim3(256), 0, E, (const uint64_t*)koff, (const uint64_t*)B.oex, (const int32_t*)B.starts, t3off, left3);
    const Tr T{n, K, d_poffset, d_poff, d_pe, t3off, B.ipath, left3, B.olen};
    uint32_t* bound = nullptr; uint64_t* soff = nullptr; int32_t *scratch = nullptr, *t_edge = nullptr, *t_offset = nullptr;
    W2_ALLOC(bound, uint32_t, n + 1); W2_ALLOC(soff, uint64_t, n + 2); W2_ALLOC(t_edge, int32_t, n + 1); W2_ALLOC(t_offset, int32_t, n + 1);
    if (n) LAUNCH(c, "k5a_tr_bound", k5a_tr_bound, dim3(grid_a(n)), dim3(256), 0, T, bound);
    W2_TRY(exclusive_scan_u32_to_u64(c, bound, soff, n));
    uint64_t nscratch = 0;
    W2_HIP(hipMemcpy(&nscratch, soff + n, 8, hipMemcpyDeviceToHost));
    W2_ALLOC(scratch, int32_t, nscratch + 1);
    if (n) LAUNCH(c, "k5a_translate", k5a_translate, dim3(grid_a(n)), dim3(256), 0, T, (const uint64_t*)soff, scratch, t_edge, t_offset, d_cnt);
    out.ms_translate = t_tr.stop();
    // ---------------------------------------------------------------- ExtendPath
    Timer t_ext(st);
    const Gr G{K, B.olen, B.right, B.from_off, B.from_e, B.packed, B.byoff};
    uint32_t *flag = nullptr, *newlen = nullptr, *ids = nullptr; uint64_t *fpos = nullptr, *o_off = nullptr; uint8_t *result = nullptr, *bestj = nullptr; int32_t* o_edges = nullptr;
    W2_ALLOC(flag, uint32_t, n + 1); W2_ALLOC(newlen, uint32_t, n + 1); W2_ALLOC(fpos, uint64_t, n + 2); W2_ALLOC(o_off, uint64_t, n + 2);
    if (n) LAUNCH(c, "k5a_ext_pre", k5a_ext_pre, dim3(grid_a(n)), dim3(256), 0, n, G, (const int32_t*)t_edge, (const int32_t*)t_offset, (const uint32_t*)d_rlen, flag, newlen);
    W2_TRY(exclusive_scan_u32_to_u64(c, flag, fpos, n));
    uint64_t nc = 0;
    W2_HIP(hipMemcpy(&nc, fpos + n, 8, hipMemcpyDeviceToHost));
    W2_ALLOC(ids, uint32_t, nc + 1); W2_ALLOC(result, uint8_t, nc + 1); W2_ALLOC(bestj, uint8_t, nc + 1);
    if (nc) {
        LAUNCH(c, "k5a_ext_compact", k5a_ext_compact, dim3(grid_a(n)), dim3(256), 0, n, (const uint32_t*)flag, (const uint64_t*)fpos, ids);
        LAUNCH(c, "k5a_extend", k5a_extend, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, nc, (const uint32_t*)ids, G, (int)P.min_gain, (const int32_t*)t_edge, (const int32_t*)t_offset,
               (const uint8_t*)d_rbits, (const uint64_t*)d_rbyte, (const uint32_t*)d_rlen, (const uint8_t*)d_quals, (const uint64_t*)d_qoff, result, bestj, newlen, d_cnt + 8);
    }
    W2_TRY(exclusive_scan_u32_to_u64(c, newlen, o_off, n));
    uint64_t npath_ints = 0;
    W2_HIP(hipMemcpy(&npath_ints, o_off + n, 8, hipMemcpyDeviceToHost));
    W2_ALLOC(o_edges, int32_t, npath_ints + 1);
    if (n) LAUNCH(c, "k5a_write_first", k5a_write_first, dim3(grid_a(n)), dim3(256), 0, n, (const int32_t*)t_edge, (const uint64_t*)o_off, o_edges);
    if (nc) LAUNCH(c, "k5a_ext_write", k5a_ext_write, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, nc, (const uint32_t*)ids, G, (const int32_t*)t_edge, (const int32_t*)t_offset,
                   (const uint32_t*)d_rlen, (const uint8_t*)result, (const uint8_t*)bestj, (const uint32_t*)newlen, (const uint64_t*)o_off, o_edges);
    out.ms_extend = t_ext.stop();
    // ---------------------------------------------------------------- results
    uint32_t h_flags[4];
    W2_TRY(step3_check(c, d_flags, h_flags));
    unsigned long long h_cnt[16];
    W2_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    out.K = (int32_t)K; out.n_vertices = NV2; out.n_edge_objs = NO2; out.n_paths = n;
    W2_TRY(dl(c, &out.edge_packed, (const uint8_t*)B.packed, B.total_bytes)); W2_TRY(dl(c, &out.edge_byte_off, (const uint64_t*)B.byoff, NO2 + 1));
    W2_TRY(dl(c, &out.edge_len, (const uint32_t*)B.olen, NO2));
    W2_TRY(dl(c, &out.vleft, (const int32_t*)B.left, NO2)); W2_TRY(dl(c, &out.vright, (const int32_t*)B.right, NO2));
    W2_TRY(dl(c, &out.from_off, (const uint64_t*)B.from_off, NV2 + 1)); W2_TRY(dl(c, &out.from_v, (const int32_t*)B.from_v, NO2)); W2_TRY(dl(c, &out.from_e, (const int32_t*)B.from_e, NO2));
    W2_TRY(dl(c, &out.to_off, (const uint64_t*)B.to_off, NV2 + 1)); W2_TRY(dl(c, &out.to_v, (const int32_t*)B.to_v, NO2)); W2_TRY(dl(c, &out.to_e, (const int32_t*)B.to_e, NO2));
    W2_TRY(dl(c, &out.inv2, (const int32_t*)B.inv2, NO2));
    W2_TRY(dl(c, &out.path_offset, (const int32_t*)t_offset, n)); W2_TRY(dl(c, &out.path_off, (const uint64_t*)o_off, n + 1)); W2_TRY(dl(c, &out.path_edges, (const int32_t*)o_edges, npath_ints));
    if (P.flags & W2RAP_STEP5_ADD_KEEP_MAP) {
        uint64_t n3 = 0;
        W2_HIP(hipMemcpy(&n3, t3off + E, 8, hipMemcpyDeviceToHost));
        out.n_old_edge_objs = E;
        W2_TRY(dl(c, &out.to3_off, (const uint64_t*)t3off, E + 1)); W2_TRY(dl(c, &out.to3, (const int32_t*)B.ipath, n3)); W2_TRY(dl(c, &out.left3, (const int32_t*)left3, E));
    }
    W2_HIP(hipStreamSynchronize(st));
    if (!NV2) { out.from_off[0] = 0; out.to_off[0] = 0; }
    out.n_tr_empty = h_cnt[0]; out.n_tr_first = h_cnt[1]; out.n_tr_walked = h_cnt[2]; out.n_tr_cleared = h_cnt[3];
    out.n_ext_tried = nc; out.n_ext_too_many = h_cnt[8]; out.n_ext_no_cover = h_cnt[9]; out.n_ext_ambiguous = h_cnt[10]; out.n_ext_extended = h_cnt[11];
    return 0;
}

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" {

int w2rap_step5_add_new_stuff(const w2rap_step5_in* in, uint64_t n_new, const uint8_t* new_packed, const uint64_t* new_byte_off, const uint32_t* new_len,
                              const w2rap_step5_add_params* P, w2rap_step5_add_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!in || !P || !out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (in->K < 16 || in->K > 640 || (in->K & 1)) return fail(W2RAP_E_ARG, "K must be even and in [16, 640]: what the large-K graph builder of Step 3 supports");
    if (P->ext_mode != 1) return fail(W2RAP_E_ARG, "ext_mode must be 1: ExtendPath's mode 2 is not built");
    if (P->min_gain < 1) return fail(W2RAP_E_ARG, "min_gain must be at least 1: below it a tie for the best extension would extend, by an order the reference leaves unspecified");
    if (P->flags & ~W2RAP_STEP5_ADD_KEEP_MAP) return fail(W2RAP_E_ARG, "unknown flag");
    if (args::too_large(*in, args::READS_END) || n_new >= (1ull << 31)) return fail(W2RAP_E_LIMIT, "more than 2^31 edge objects, vertices or patches, or 2^32 reads");
    if (in->n_reads != in->n_paths) return fail(W2RAP_E_ARG, "n_reads differs from n_paths: ExtendPath needs the bases and qualities of every read");
    W2_ARGS(args::null_arrays(*in));
    if (n_new && (!new_byte_off || !new_len)) return fail(W2RAP_E_ARG, "null new_stuff array");
    W2_ARGS(args::edge_off_start(*in));
    W2_ARGS(args::edge_lens(*in));
    if (n_new) {
        if (new_byte_off[0] != 0) return fail(W2RAP_E_ARG, "new_byte_off must start at 0");
        for (uint64_t i = 0; i < n_new; ++i)
            if (new_byte_off[i + 1] < new_byte_off[i] || new_byte_off[i + 1] - new_byte_off[i] != ((uint64_t)new_len[i] + 3) / 4) return fail(W2RAP_E_ARG, "new_byte_off does not match new_len");
        if (new_byte_off[n_new] && !new_packed) return fail(W2RAP_E_ARG, "null new_packed");
    }
    W2_ARGS(args::adjacency(*in));
    W2_ARGS(args::crossings(*in));
    W2_ARGS(args::reads_and_paths(*in, [&](uint64_t r) { return in->read_len[r] >= (1u << 31) ? args::Err{W2RAP_E_LIMIT, "a read of 2^31 bases"} : args::OK; }));
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return add_new_stuff(c, *in, n_new, new_packed, new_byte_off, new_len, *P, *out); }, save_profile5,
                    [&] { w2rap_step5_add_free(out); });
}

void w2rap_step5_add_free(w2rap_step5_add_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->edge_packed, (void*)o->edge_byte_off, (void*)o->edge_len, (void*)o->vleft, (void*)o->vright, (void*)o->from_off, (void*)o->from_v, (void*)o->from_e,
                    (void*)o->to_off, (void*)o->to_v, (void*)o->to_e, (void*)o->inv2, (void*)o->path_offset, (void*)o->path_off, (void*)o->path_edges, (void*)o->to3_off,
                    (void*)o->to3, (void*)o->left3})
        std::free(p);
    std::memset(o, 0, sizeof(*o));
}

}  // extern "C"
