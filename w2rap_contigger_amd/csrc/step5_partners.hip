// step5_partners.hip -- the tail of Step 5: PartnersToEnds (src/paths/long/large/GapToyTools5.cc:1150-1517) on the clean large-K graph.
//
//   device  k5_not_sink / k5_relax        min(D, 501) per vertex, D = DistancesToEndArr's longest walk to a sink in K-mers
//                                         (graph/DigraphTemplate.h:1581-1619): saturating relaxation backwards from the sinks until a
//                                         round changes nothing (up to vertices + 501 rounds: a value moves one edge per round)
//   device  k5_flag / scan / k5_compact / scan
//                                         findInterestingReadIds (:1154-1194): unplaced, mate placed and ending near an end, >= 28 bases
//   device  k5_emit / sort / k5_heads / scan / k5_groups
//                                         MREReadProc (:1277-1327): every 28-mer of those reads, sorted; the distinct ones and their locations
//   device  k5_edge_npos / scan / k5_edge_lookup / k5_keep
//                                         MREEdgeProc (:1331-1361) and the remove_if (:1501): occurrences over all edge objects, both
//                                         multiplicity filters
//   device  k5_cand_count / scan / k5_cand_fill / sort / k5_heads / scan / k5_unique
//                                         EdgeProc::operator() and addLocs (:1378-1420): the distinct (read, edge, read offset - edge offset)
//   device  k5_verify                     isGood (:1424-1449), one wavefront per candidate
//   device  k5_decide / k5_path_len / scan / k5_path_write
//                                         :1393-1410: exactly one good candidate places the read; the new read paths
// Integer arithmetic throughout.  Nothing depends on the order in which candidates are found: a read is placed if and only if exactly
// one distinct candidate is good, which is what the reference's lock and its NOT_AN_EDGE mark compute in any thread order.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "step5_runs.h"
#include "../../include/w2rap_step5.h"

namespace w2 {
namespace {

constexpr unsigned KLEN = 28, MAX_MULT = 80, WINDOW = 60, MAX_MISMATCHES = 4, TRUSTED_QUAL = 30;
constexpr uint32_t GOOD_DIST = 500, SAT = GOOD_DIST + 1;     // distances saturate at 501: only D <= 500 is asked
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr unsigned ROUND_BATCH = 32;                          // relaxation rounds between two looks at the "changed" words
static_assert(ROUND_BATCH == 32, "the profile line of a batch is named k5_relax_x32");
constexpr uint64_t KMASK = (1ull << (2 * KLEN)) - 1;

// the 28-mer at base `pos` of a packed sequence: base pos + i at bits 2i.  Reads 8 bytes from byte pos / 4 on: the sequences' blocks
// carry 16 bytes of slack, and whatever lies behind base pos + 27 is masked off
__device__ inline uint64_t kmer28(const uint8_t* b, uint64_t pos) {
    const uint8_t* q = b + (pos >> 2);
    uint64_t w = 0;
#pragma unroll
    for (unsigned k = 0; k < 8; ++k) w |= (uint64_t)q[k] << (8 * k);
    return (w >> (2 * (pos & 3))) & KMASK;
}
// the last i in [0, n) with a[i] <= x (a ascending, a[0] <= x)
__device__ inline uint64_t last_le(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// ---- near an end ---------------------------------------------------------------------------------------------------------------
// W[v] = 0: no sink reached (yet); otherwise min(D(v), 501) + 1
__global__ __launch_bounds__(256) void k5_fill_u32(uint64_t n, uint32_t v, uint32_t* __restrict__ a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}
__global__ __launch_bounds__(256) void k5_not_sink(uint64_t E, const int32_t* __restrict__ vleft, uint32_t* __restrict__ W) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E) W[vleft[e]] = 0;
}
__global__ __launch_bounds__(256) void k5_relax(uint64_t E, unsigned K, const int32_t* __restrict__ vleft, const int32_t* __restrict__ vright,
                                                const uint32_t* __restrict__ elen, uint32_t* __restrict__ W, uint32_t* __restrict__ changed) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint32_t dv = __hip_atomic_load(&W[vright[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!dv) return;
    const uint64_t d = (uint64_t)(dv - 1) + (elen[e] - K + 1);
    const uint32_t nw = (uint32_t)(d < SAT ? d : SAT) + 1;
    if (atomicMax(&W[vleft[e]], nw) < nw) *changed = 1;
}

// ---- select --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k5_flag(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const uint32_t* __restrict__ rlen,
                                               const int32_t* __restrict__ vright, const uint32_t* __restrict__ W, uint32_t* __restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    uint32_t f = 0;
    const uint64_t m = r ^ 1;                                  // (n is even)
    if (poff[r + 1] == poff[r] && poff[m + 1] > poff[m] && rlen[r] >= KLEN) {
        const uint32_t w = W[vright[pe[poff[m + 1] - 1]]];
        f = w != 0 && w - 1 <= GOOD_DIST;
    }
    flag[r] = f;
}
__global__ __launch_bounds__(256) void k5_compact(uint64_t n, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ fpos, const uint32_t* __restrict__ rlen,
                                                  uint32_t* __restrict__ ids, uint32_t* __restrict__ kcnt) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n || !flag[r]) return;
    ids[fpos[r]] = (uint32_t)r; kcnt[fpos[r]] = rlen[r] - KLEN + 1;
}

// ---- the dictionary ------------------------------------------------------------------------------------------------------------
struct Seqs { const uint8_t* bits; const uint64_t* boff; const uint32_t* len; };

__global__ __launch_bounds__(256) void k5_emit(uint64_t NKM, uint64_t NI, const uint64_t* __restrict__ koff, const uint32_t* __restrict__ ids, Seqs R,
                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint2* __restrict__ loc) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= NKM) return;
    const uint64_t i = last_le(koff, NI, j);
    const uint32_t roff = (uint32_t)(j - koff[i]);
    keys[j] = kmer28(R.bits + R.boff[ids[i]], roff);
    vals[j] = (uint32_t)j;
    loc[j] = make_uint2((uint32_t)i, roff);
}
__global__ __launch_bounds__(256) void k5_groups(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint64_t* __restrict__ hpos,
                                                 uint64_t* __restrict__ ukey, uint32_t* __restrict__ ustart) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (head[j]) { ukey[hpos[j]] = keys[j]; ustart[hpos[j]] = (uint32_t)j; }
    if (j == n - 1) ustart[hpos[n]] = (uint32_t)n;
}

// ---- the edges' 28-mers --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k5_edge_npos(uint64_t E, const uint32_t* __restrict__ elen, uint32_t* __restrict__ npos) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < E) npos[e] = elen[e] >= KLEN ? elen[e] - KLEN + 1 : 0;
}
// hit[p] = the dictionary entry of the 28-mer at edge position p (not looked at further when the reads alone hold it more than 80 times)
__global__ __launch_bounds__(256) void k5_edge_lookup(uint64_t EP, uint64_t E, const uint64_t* __restrict__ eoff, Seqs G, uint64_t U, const uint64_t* __restrict__ ukey,
                                                      const uint32_t* __restrict__ ustart, uint32_t* __restrict__ ecnt, uint32_t* __restrict__ hit) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= EP) return;
    const uint64_t e = last_le(eoff, E, p);
    const uint64_t key = kmer28(G.bits + G.boff[e], p - eoff[e]);
    uint32_t h = NONE;
    if (ukey[0] <= key) {
        const uint64_t g = last_le(ukey, U, key);
        if (ukey[g] == key && ustart[g + 1] - ustart[g] <= MAX_MULT) { h = (uint32_t)g; atomicAdd(&ecnt[g], 1u); }
    }
    hit[p] = h;
}
__global__ __launch_bounds__(256) void k5_keep(uint64_t U, const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ ecnt, uint8_t* __restrict__ keep,
                                               unsigned long long* __restrict__ counters) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (g < U) {
        const uint32_t nr = ustart[g + 1] - ustart[g];
        k = nr <= MAX_MULT && (uint64_t)nr + ecnt[g] <= MAX_MULT;
        keep[g] = k;
    }
    const unsigned long long b = __ballot(k);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&counters[0], (unsigned long long)__builtin_popcountll(b));
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------
// A candidate's sort key: the read's rank among the interesting reads above `dbits` bits of diagonal number.  The diagonals of edge e are
// numbered doff(e) + (eOff - rOff + maxro), doff(e) = eoff[e] + e * maxro, maxro = the largest read offset of a 28-mer: distinct
// (edge, rOff - eOff) pairs get distinct numbers.
struct CandArgs {
    uint64_t EP, E, NI; const uint64_t* eoff; const uint32_t* hit; const uint8_t* keep; const uint64_t* ukey; const uint32_t* ustart;
    const uint32_t* vals; const uint2* loc; const uint32_t* ids; Seqs R; uint64_t maxro; unsigned dbits;
};
// the candidates edge position p contributes.  A location whose diagonal also matches a surviving 28-mer one position earlier is left to
// that position: every diagonal with a match keeps the first match of each of its runs, the sort removes the remaining repeats exactly
template <bool WRITE>
__device__ inline uint32_t cands_of(const CandArgs& a, uint64_t p, uint64_t* out) {
    const uint32_t g = a.hit[p];
    if (g == NONE || !a.keep[g]) return 0;
    const uint64_t e = last_le(a.eoff, a.E, p);
    const uint64_t eo = p - a.eoff[e];
    const uint32_t gp = eo ? a.hit[p - 1] : NONE;
    const bool prev = gp != NONE && a.keep[gp];
    const uint64_t pkey = prev ? a.ukey[gp] : 0;
    uint32_t k = 0;
    for (uint32_t s = a.ustart[g]; s < a.ustart[g + 1]; ++s) {
        const uint2 l = a.loc[a.vals[s]];
        if (prev && l.y && kmer28(a.R.bits + a.R.boff[a.ids[l.x]], l.y - 1) == pkey) continue;
        if (WRITE) out[k] = ((uint64_t)l.x << a.dbits) | (p + (e + 1) * a.maxro - l.y);
        ++k;
    }
    return k;
}
__global__ __launch_bounds__(256) void k5_cand_count(CandArgs a, uint32_t* __restrict__ cnt) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < a.EP) cnt[p] = cands_of<false>(a, p, nullptr);
}
__global__ __launch_bounds__(256) void k5_cand_fill(CandArgs a, const uint64_t* __restrict__ coff, uint64_t* __restrict__ ckeys) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < a.EP && coff[p + 1] > coff[p]) cands_of<true>(a, p, ckeys + coff[p]);
}
__global__ __launch_bounds__(256) void k5_unique(uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint64_t* __restrict__ hpos,
                                                 uint64_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n && head[j]) out[hpos[j]] = keys[j];
}

// ---- isGood: one wavefront per candidate ---------------------------------------------------------------------------------------
struct VerifyArgs {
    uint64_t NC, E; const uint64_t* cand; unsigned dbits; uint64_t maxro; const uint64_t* eoff; const uint32_t* ids;
    Seqs G, R; const uint8_t* quals; const uint64_t* qoff;
};
__global__ __launch_bounds__(256) void k5_verify(VerifyArgs a, uint32_t* __restrict__ ngood, int32_t* __restrict__ place_e, int32_t* __restrict__ place_off,
                                                 unsigned long long* __restrict__ counters) {
    const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63;
    if (c >= a.NC) return;                                     // (wave-uniform)
    const uint64_t key = a.cand[c];
    const uint64_t i = key >> a.dbits, gd = key & ((1ull << a.dbits) - 1);
    // the edge whose diagonals hold gd: doff(e) = eoff[e] + e * maxro is ascending
    uint64_t lo = 0, hi = a.E;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.eoff[mid] + mid * a.maxro <= gd) lo = mid; else hi = mid; }
    const uint64_t e = lo;
    const int64_t offset = (int64_t)(gd - (a.eoff[e] + e * a.maxro)) - (int64_t)a.maxro;      // eOff - rOff = -loc.getOffset()
    const uint32_t r = a.ids[i];
    const int64_t el = a.G.len[e], rl = a.R.len[r];
    const int64_t es = offset >= 0 ? offset : 0, rs = offset >= 0 ? 0 : -offset;
    if (el - es < (int64_t)WINDOW || rl - rs < (int64_t)WINDOW) return;
    const int64_t L = el - es < rl - rs ? el - es : rl - rs;                                   // the overlap
    const uint8_t* eb = a.G.bits + a.G.boff[e];
    const uint8_t* rb = a.R.bits + a.R.boff[r];
    const uint8_t* rq = a.quals + a.qoff[r];
    // the mismatch mask 64 positions at a time; the windows that start in a chunk are counted once the next chunk is known
    bool fatal = false, good = false;
    unsigned long long prev = 0;
    const int64_t nchunks = (L + 63) >> 6;
    for (int64_t ch = 0; ch <= nchunks; ++ch) {
        const int64_t t = ch * 64 + lane;
        bool mm = false;
        if (t < L) {
            mm = packed_base(eb, (uint64_t)(es + t)) != packed_base(rb, (uint64_t)(rs + t));
            fatal |= mm && rq[rs + t] >= TRUSTED_QUAL;
        }
        const unsigned long long cur = __ballot(mm);
        if (ch) {
            const int64_t w = (ch - 1) * 64 + lane;            // a window start
            unsigned long long bits = prev >> lane;
            if (lane) bits |= cur << (64 - lane);
            bits &= (1ull << WINDOW) - 1;
            good |= w + (int64_t)WINDOW <= L && (unsigned)__builtin_popcountll(bits) <= MAX_MISMATCHES;
        }
        prev = cur;
    }
    if (__ballot(fatal) || !__ballot(good)) return;
    if (lane == 0) {
        atomicAdd(&ngood[i], 1u);
        place_e[i] = (int32_t)e; place_off[i] = (int32_t)offset;  // (read only where ngood ends at 1: then this is the one writer)
        atomicAdd(&counters[1], 1ull);
    }
}

// ---- the decision and the new paths --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k5_decide(uint64_t NI, const uint32_t* __restrict__ ngood, unsigned long long* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t g = i < NI ? ngood[i] : 0;
    const unsigned long long one = __ballot(g == 1), many = __ballot(g > 1);
    if ((threadIdx.x & 63) == 0) {
        if (one) atomicAdd(&counters[2], (unsigned long long)__builtin_popcountll(one));
        if (many) atomicAdd(&counters[3], (unsigned long long)__builtin_popcountll(many));
    }
}
__global__ __launch_bounds__(256) void k5_path_len(uint64_t n, const uint64_t* __restrict__ poff, const uint32_t* __restrict__ flag, const uint64_t* __restrict__ fpos,
                                                   const uint32_t* __restrict__ ngood, uint32_t* __restrict__ nlen) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) nlen[r] = flag[r] ? (ngood[fpos[r]] == 1 ? 1u : 0u) : (uint32_t)(poff[r + 1] - poff[r]);
}
__global__ __launch_bounds__(256) void k5_path_write(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe, const int32_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ flag, const uint64_t* __restrict__ fpos, const uint32_t* __restrict__ ngood,
                                                     const int32_t* __restrict__ place_e, const int32_t* __restrict__ place_off, const uint64_t* __restrict__ noff,
                                                     int32_t* __restrict__ npe, int32_t* __restrict__ noffs) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (flag[r]) {
        const uint64_t i = fpos[r];
        const uint32_t g = ngood[i];
        if (g == 1) { npe[noff[r]] = place_e[i]; noffs[r] = place_off[i]; }
        else noffs[r] = g ? 0 : offs[r];                       // cleanAmbiguousPlacements (:1406-1410) sets the offset of an ambiguous read to 0
        return;
    }
    uint64_t o = noff[r];
    for (uint64_t k = poff[r]; k < poff[r + 1]; ++k) npe[o++] = pe[k];
    noffs[r] = offs[r];
}

std::string g_profile5;

}  // namespace

// (also called by step5_open.hip: w2rap_step5_profile reports the last Step-5 call of either kind)
void save_profile5(Ctx& c) { g_profile5 = profile_text(c); }

namespace {

int partners(Ctx& c, const w2rap_step5_in& in, uint32_t max_len, w2rap_step5_out& out) {
    const uint64_t E = in.n_edge_objs, NV = in.n_vertices, n = in.n_paths, npe = n ? in.path_off[n] : 0;
    const unsigned K = (unsigned)in.K;
    auto unchanged = [&]() -> int {                            // the reference returns at once: the paths as they came
        out.n_paths = n;
        out.path_offset = host_dup(in.path_offset, n); out.path_edges = host_dup(in.path_edges, npe);
        out.path_off = (uint64_t*)host_result_alloc((n + 1) * 8);
        if (!out.path_offset || !out.path_edges || !out.path_off) { c.err = "out of host memory"; return W2RAP_E_HIP; }
        if (n) std::memcpy(out.path_off, in.path_off, (n + 1) * 8); else out.path_off[0] = 0;
        return 0;
    };
    if (!n || !E) return unchanged();                          // no reads, or no edge a mate could lie on
    // ---- upload
    std::vector<int32_t> vleft, vright;
    args::edge_ends(in, vleft, vright);
    uint8_t *d_ebits = nullptr, *d_rbits = nullptr, *d_quals = nullptr;
    uint64_t *d_ebyte = nullptr, *d_rbyte = nullptr, *d_qoff = nullptr, *d_poff = nullptr;
    uint32_t *d_elen = nullptr, *d_rlen = nullptr;
    int32_t *d_vleft = nullptr, *d_vright = nullptr, *d_poffset = nullptr, *d_pe = nullptr;
    W2_TRY(up_pooled(c, &d_ebits, in.edge_packed, in.edge_byte_off[E], 16));
    W2_TRY(up_pooled(c, &d_ebyte, in.edge_byte_off, E + 1));
    W2_TRY(up_pooled(c, &d_elen, in.edge_len, E));
    W2_TRY(up_pooled(c, &d_vleft, (const int32_t*)vleft.data(), E));
    W2_TRY(up_pooled(c, &d_vright, (const int32_t*)vright.data(), E));
    W2_TRY(up_pooled(c, &d_rbits, in.read_packed, in.read_byte_off[n], 16));
    W2_TRY(up_pooled(c, &d_rbyte, in.read_byte_off, n + 1));
    W2_TRY(up_pooled(c, &d_rlen, in.read_len, n));
    W2_TRY(up_pooled(c, &d_quals, in.quals, in.qual_off[n], 16));
    W2_TRY(up_pooled(c, &d_qoff, in.qual_off, n + 1));
    W2_TRY(up_pooled(c, &d_poffset, in.path_offset, n));
    W2_TRY(up_pooled(c, &d_poff, in.path_off, n + 1));
    W2_TRY(up_pooled(c, &d_pe, in.path_edges, npe));
    W2_HIP(hipStreamSynchronize(c.stream));                     // (the host vectors above have been read)
    const Seqs G{d_ebits, d_ebyte, d_elen}, R{d_rbits, d_rbyte, d_rlen};

    // ---- a. near an end
    uint32_t* d_W = nullptr;
    {
        Timer t(c.stream);
        uint32_t* d_chg = nullptr;
        W2_ALLOC(d_W, uint32_t, NV + 1); W2_ALLOC(d_chg, uint32_t, ROUND_BATCH);
        LAUNCH(c, "k5_fill_u32", k5_fill_u32, dim3(grid5(NV)), dim3(256), 0, NV, 1u, d_W);
        LAUNCH(c, "k5_not_sink", k5_not_sink, dim3(grid5(E)), dim3(256), 0, E, (const int32_t*)d_vleft, d_W);
        // A launch moves a value at least one edge back from where it stood (k5_relax loads, then atomicMax-es) and promises no more, so
        // a vertex h edges from the nearest sink may wait h launches for its first value, and a saturated 501 travels back edge by edge
        // too: up to NV launches to reach everybody + 501 to saturate.  The loop ends on a launch that changed nothing -- no word was
        // written during it, so every edge was looked at with final values: the fixed point.  Launches are queued ROUND_BATCH at a time,
        // each with its own "changed" word, and timed per batch
        bool settled = false;
        for (uint64_t round = 0; round < NV + SAT + ROUND_BATCH && !settled; round += ROUND_BATCH) {
            uint32_t chg[ROUND_BATCH];
            W2_HIP(hipMemsetAsync(d_chg, 0, sizeof chg, c.stream));
            c.pbegin("k5_relax_x32");
            for (unsigned k = 0; k < ROUND_BATCH; ++k)
                hipLaunchKernelGGL(k5_relax, dim3(grid5(E)), dim3(256), 0, c.stream, E, K, (const int32_t*)d_vleft, (const int32_t*)d_vright, (const uint32_t*)d_elen, d_W, d_chg + k);
            c.pend();
            W2_HIP(hipMemcpyAsync(chg, d_chg, sizeof chg, hipMemcpyDeviceToHost, c.stream));
            W2_HIP(hipStreamSynchronize(c.stream));
            for (unsigned k = 0; k < ROUND_BATCH; ++k) settled |= chg[k] == 0;
        }
        if (!settled) { c.err = "the distances to the graph's ends did not settle"; return W2RAP_E_GRAPH; }
        out.ms_ends = t.stop();
    }
    // ---- b. select
    uint32_t *d_flag = nullptr, *d_ids = nullptr, *d_kcnt = nullptr; uint64_t *d_fpos = nullptr, *d_koff = nullptr;
    uint64_t NI = 0, NKM = 0;
    {
        Timer t(c.stream);
        W2_ALLOC(d_flag, uint32_t, n + 1); W2_ALLOC(d_fpos, uint64_t, n + 2);
        LAUNCH(c, "k5_flag", k5_flag, dim3(grid5(n)), dim3(256), 0, n, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const uint32_t*)d_rlen, (const int32_t*)d_vright,
               (const uint32_t*)d_W, d_flag);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_flag, d_fpos, n));
        W2_HIP(hipMemcpyAsync(&NI, d_fpos + n, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        out.n_interesting = NI;
        if (!NI) { out.ms_select = t.stop(); return unchanged(); }
        W2_ALLOC(d_ids, uint32_t, NI + 1); W2_ALLOC(d_kcnt, uint32_t, NI + 1); W2_ALLOC(d_koff, uint64_t, NI + 2);
        LAUNCH(c, "k5_compact", k5_compact, dim3(grid5(n)), dim3(256), 0, n, (const uint32_t*)d_flag, (const uint64_t*)d_fpos, (const uint32_t*)d_rlen, d_ids, d_kcnt);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_kcnt, d_koff, NI));
        W2_HIP(hipMemcpyAsync(&NKM, d_koff + NI, 8, hipMemcpyDeviceToHost, c.stream));
        out.ms_select = t.stop();
        W2_HIP(hipStreamSynchronize(c.stream));
        out.n_read_kmers = NKM;
    }
    if (NKM >= NONE) { c.err = "more than 2^32 28-mers in the unplaced reads"; return W2RAP_E_LIMIT; }
    // ---- c. the dictionary
    uint64_t *d_keys = nullptr, *d_ukey = nullptr; uint32_t *d_vals = nullptr, *d_ustart = nullptr; uint2* d_loc = nullptr;
    uint64_t U = 0;
    {
        Timer t(c.stream);
        W2_ALLOC(d_keys, uint64_t, NKM + 1); W2_ALLOC(d_vals, uint32_t, NKM + 1); W2_ALLOC(d_loc, uint2, NKM + 1);
        LAUNCH(c, "k5_emit", k5_emit, dim3(grid5(NKM)), dim3(256), 0, NKM, NI, (const uint64_t*)d_koff, (const uint32_t*)d_ids, R, d_keys, d_vals, d_loc);
        W2_TRY(sort_pairs_u64(c, d_keys, d_vals, NKM, 0, 2 * KLEN));
        uint32_t* d_head = nullptr; uint64_t* d_hpos = nullptr;
        W2_TRY(run_heads(c, "k5_heads", d_keys, NKM, &d_head, &d_hpos, &U));
        W2_ALLOC(d_ukey, uint64_t, U + 1); W2_ALLOC(d_ustart, uint32_t, U + 2);
        LAUNCH(c, "k5_groups", k5_groups, dim3(grid5(NKM)), dim3(256), 0, NKM, (const uint64_t*)d_keys, (const uint32_t*)d_head, (const uint64_t*)d_hpos, d_ukey, d_ustart);
        out.ms_dict = t.stop();
        c.release(d_head); c.release(d_hpos); c.release(d_keys); d_keys = nullptr;
    }
    // ---- d. the edges' 28-mers and both multiplicity filters
    uint32_t *d_hit = nullptr; uint8_t* d_keep = nullptr; uint64_t* d_eoff = nullptr; unsigned long long* d_cnt = nullptr;
    uint64_t EP = 0;
    {
        Timer t(c.stream);
        uint32_t *d_npos = nullptr, *d_ecnt = nullptr;
        W2_ALLOC(d_npos, uint32_t, E + 1); W2_ALLOC(d_eoff, uint64_t, E + 2); W2_ALLOC(d_ecnt, uint32_t, U + 1); W2_ALLOC(d_keep, uint8_t, U + 1);
        W2_ALLOC(d_cnt, unsigned long long, 4);
        W2_HIP(hipMemsetAsync(d_cnt, 0, 32, c.stream));
        W2_HIP(hipMemsetAsync(d_ecnt, 0, (U + 1) * 4, c.stream));
        LAUNCH(c, "k5_edge_npos", k5_edge_npos, dim3(grid5(E)), dim3(256), 0, E, (const uint32_t*)d_elen, d_npos);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_npos, d_eoff, E));
        W2_HIP(hipMemcpyAsync(&EP, d_eoff + E, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        if (EP >= (1ull << 39)) { c.err = "more than 2^39 28-mer positions in the edges"; return W2RAP_E_LIMIT; }       // (one thread each: the grid)
        W2_ALLOC(d_hit, uint32_t, EP + 1);
        if (EP) LAUNCH(c, "k5_edge_lookup", k5_edge_lookup, dim3(grid5(EP)), dim3(256), 0, EP, E, (const uint64_t*)d_eoff, G, U, (const uint64_t*)d_ukey,
                       (const uint32_t*)d_ustart, d_ecnt, d_hit);
        LAUNCH(c, "k5_keep", k5_keep, dim3(grid5(U)), dim3(256), 0, U, (const uint32_t*)d_ustart, (const uint32_t*)d_ecnt, d_keep, d_cnt);
        out.ms_edges = t.stop();
        c.release(d_npos); c.release(d_ecnt);
    }
    // ---- e. candidates
    const uint64_t maxro = max_len - KLEN;                      // (an interesting read exists, so max_len >= 28)
    if (E >= (1ull << 40) / (maxro + 1)) { c.err = "the edges' diagonals need more than 40 bits"; return W2RAP_E_LIMIT; }
    const unsigned dbits = bits_for(EP + E * maxro + 1), ibits = bits_for(NI);
    if (dbits + ibits > 64) { c.err = "a candidate's sort key needs more than 64 bits"; return W2RAP_E_LIMIT; }
    uint64_t* d_cand = nullptr; uint64_t NC = 0;
    {
        Timer t(c.stream);
        uint32_t* d_ccnt = nullptr; uint64_t* d_coff = nullptr; uint64_t NCR = 0;
        W2_ALLOC(d_ccnt, uint32_t, EP + 1); W2_ALLOC(d_coff, uint64_t, EP + 2);
        const CandArgs A{EP, E, NI, d_eoff, d_hit, d_keep, d_ukey, d_ustart, d_vals, d_loc, d_ids, R, maxro, dbits};
        if (EP) LAUNCH(c, "k5_cand_count", k5_cand_count, dim3(grid5(EP)), dim3(256), 0, A, d_ccnt);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_ccnt, d_coff, EP));
        W2_HIP(hipMemcpyAsync(&NCR, d_coff + EP, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        if (NCR >= (1ull << 39)) { c.err = "more than 2^39 candidates before deduplication"; return W2RAP_E_LIMIT; }
        if (NCR) {
            uint64_t* d_ckeys = nullptr; uint32_t* d_cvals = nullptr;
            W2_ALLOC(d_ckeys, uint64_t, NCR + 1); W2_ALLOC(d_cvals, uint32_t, NCR + 1);
            W2_HIP(hipMemsetAsync(d_cvals, 0, (NCR + 1) * 4, c.stream));       // (the sort moves pairs; the values carry nothing)
            LAUNCH(c, "k5_cand_fill", k5_cand_fill, dim3(grid5(EP)), dim3(256), 0, A, (const uint64_t*)d_coff, d_ckeys);
            W2_TRY(sort_pairs_u64(c, d_ckeys, d_cvals, NCR, 0, (int)(dbits + ibits)));
            uint32_t* d_head = nullptr; uint64_t* d_hpos = nullptr;
            W2_TRY(run_heads(c, "k5_heads", d_ckeys, NCR, &d_head, &d_hpos, &NC));
            W2_ALLOC(d_cand, uint64_t, NC + 1);
            LAUNCH(c, "k5_unique", k5_unique, dim3(grid5(NCR)), dim3(256), 0, NCR, (const uint64_t*)d_ckeys, (const uint32_t*)d_head, (const uint64_t*)d_hpos, d_cand);
            out.ms_candidates = t.stop();
            c.release(d_head); c.release(d_hpos); c.release(d_ckeys); c.release(d_cvals);
        } else out.ms_candidates = t.stop();
        c.release(d_ccnt); c.release(d_coff);
    }
    out.n_candidates = NC;
    // ---- f. verify
    uint32_t* d_ngood = nullptr; int32_t *d_place_e = nullptr, *d_place_off = nullptr;
    {
        Timer t(c.stream);
        W2_ALLOC(d_ngood, uint32_t, NI + 1); W2_ALLOC(d_place_e, int32_t, NI + 1); W2_ALLOC(d_place_off, int32_t, NI + 1);
        W2_HIP(hipMemsetAsync(d_ngood, 0, (NI + 1) * 4, c.stream));
        if (NC >= (1ull << 33) - 4) { c.err = "more than 2^33 candidates"; return W2RAP_E_LIMIT; }                        // (four to a block: the grid)
        const VerifyArgs V{NC, E, d_cand, dbits, maxro, d_eoff, d_ids, G, R, d_quals, d_qoff};
        if (NC) LAUNCH(c, "k5_verify", k5_verify, dim3(grid5(NC, 4)), dim3(256), 0, V, d_ngood, d_place_e, d_place_off, d_cnt);
        LAUNCH(c, "k5_decide", k5_decide, dim3(grid5(NI)), dim3(256), 0, NI, (const uint32_t*)d_ngood, d_cnt);
        out.ms_verify = t.stop();
    }
    // ---- g. the new paths
    {
        Timer t(c.stream);
        uint32_t* d_nlen = nullptr; uint64_t* d_noff = nullptr; int32_t *d_npe = nullptr, *d_noffs = nullptr;
        W2_ALLOC(d_nlen, uint32_t, n + 1); W2_ALLOC(d_noff, uint64_t, n + 2); W2_ALLOC(d_noffs, int32_t, n + 1); W2_ALLOC(d_npe, int32_t, npe + NI + 1);
        LAUNCH(c, "k5_path_len", k5_path_len, dim3(grid5(n)), dim3(256), 0, n, (const uint64_t*)d_poff, (const uint32_t*)d_flag, (const uint64_t*)d_fpos,
               (const uint32_t*)d_ngood, d_nlen);
        W2_TRY(exclusive_scan_u32_to_u64(c, d_nlen, d_noff, n));
        LAUNCH(c, "k5_path_write", k5_path_write, dim3(grid5(n)), dim3(256), 0, n, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const int32_t*)d_poffset,
               (const uint32_t*)d_flag, (const uint64_t*)d_fpos, (const uint32_t*)d_ngood, (const int32_t*)d_place_e, (const int32_t*)d_place_off,
               (const uint64_t*)d_noff, d_npe, d_noffs);
        out.ms_paths = t.stop();
        unsigned long long cnt[4] = {0, 0, 0, 0};
        W2_HIP(hipMemcpyAsync(cnt, d_cnt, 32, hipMemcpyDeviceToHost, c.stream));
        out.n_paths = n;
        W2_TRY(dl(c, &out.path_off, (const uint64_t*)d_noff, n + 1));
        W2_TRY(dl(c, &out.path_offset, (const int32_t*)d_noffs, n));
        W2_HIP(hipStreamSynchronize(c.stream));
        out.n_dict_kmers = cnt[0]; out.n_good = cnt[1]; out.n_placed = cnt[2]; out.n_ambiguous = cnt[3];
        if (out.path_off[n] != npe + out.n_placed) { c.err = "the new paths do not hold one edge per placed read"; return W2RAP_E_GRAPH; }
        W2_TRY(dl(c, &out.path_edges, (const int32_t*)d_npe, out.path_off[n]));
        W2_HIP(hipStreamSynchronize(c.stream));
    }
    return 0;
}

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" {

int w2rap_step5_partners_to_ends(const w2rap_step5_in* in, const w2rap_step5_params* P, w2rap_step5_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!in || !P || !out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640]");
    if (P->flags) return fail(W2RAP_E_ARG, "unknown flag");
    if (args::too_large(*in, args::READS_END)) return fail(W2RAP_E_LIMIT, args::TOO_LARGE);
    if (in->n_paths & 1) return fail(W2RAP_E_ARG, args::ODD_PATHS);
    if (in->n_reads != in->n_paths) return fail(W2RAP_E_ARG, "n_reads differs from n_paths: PartnersToEnds needs the bases and qualities of every read");
    W2_ARGS(args::null_arrays(*in));
    W2_ARGS(args::edge_off_start(*in));
    W2_ARGS(args::edge_lens(*in));
    W2_ARGS(args::adjacency(*in));
    uint32_t max_len = 0;
    W2_ARGS(args::reads_and_paths(*in, [&](uint64_t r) { max_len = std::max(max_len, in->read_len[r]); return args::OK; }));
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return partners(c, *in, max_len, *out); }, save_profile5, [&] { w2rap_step5_free(out); });
}

void w2rap_step5_free(w2rap_step5_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->path_offset, (void*)o->path_off, (void*)o->path_edges}) std::free(p);
    std::memset(o, 0, sizeof(*o));
}

size_t w2rap_step5_profile(char* buf, size_t len) {
    if (buf && len) std::snprintf(buf, len, "%s", g_profile5.c_str());
    return g_profile5.size() + 1;
}

}  // extern "C"
