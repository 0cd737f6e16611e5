// step2_count.hip -- phases a1..a6 of Step 2 on gfx950, all but the partition:
//   K0  k_good_len        quality window per read                 (BuildReadQGraph.cc:962-987)
//   K1, K2                the partition into super-k-mer records grouped by bucket: step2_partition.hip
//   K3  k_count_buckets   per-bucket LDS hash count/merge          (collapse_entries :1002-1013, combine_Entries :943-949,
//                         + min_freq filter + histogram             filter :1094-1104)
//   K4  k_table_insert    lookup table over solid k-mers           (new BRQ_Dict + insertEntryNoLocking :1092-1099)
//   K5  k_prune_local,    adjacency prune, bucket-local in LDS,    (kmers/ReadPather.h:317-346)
//       k_prune           then the open bits against the table
//
// Design (MI355X-first, integer/HBM work, no MFMA):
//  * reads are consumed wavefront-per-read, lane = k-mer position: no divergence, the
//    packed read block is loaded once (coalesced byte loads) into LDS;
//  * instead of shipping one 17-B record per k-mer instance to HBM and back, consecutive
//    k-mers that share a canonical minimizer bucket travel as ONE 32-B super-k-mer
//    record (<= 64 k-mers): ~1.6 B/k-mer of partition traffic instead of 34 B;
//  * every bucket is sized to fit an LDS hash table, so counting (count saturating add,
//    context OR) never touches HBM; only distinct solid k-mers are written back;
//  * bucket sizes are data dependent: a bucket whose distinct set overflows the LDS table
//    is re-processed in 2,4,.. hash sub-passes (same semantics as MapReduceEngine.h:288-291);
//  * the kernels are bound by instruction issue (K1, K3), device atomics (K2, K4: 27 G/s) or random 32-B sectors (K5), not
//    by HBM bytes: K3 (issue) and K4 (atomics) therefore run side by side on two streams, bucket slice by bucket slice.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "ctx.h"

namespace w2 {

// =============================================================================== K0
constexpr unsigned QSLOTS = 256;       // partial sums / maxima of k_good_len
// One read per lane; scans the raw qualities backwards for the rightmost window of K
// consecutive q >= min_qual.  good_len is stored as uint16 like the reference (:1056).
// MASK: the bits are given (qmask: bit i = quality i >= min_qual, made on the host side of an upload that sends the raw bytes later).
template <bool MASK>
__global__ void __launch_bounds__(256) k_good_len(uint64_t n, const uint8_t* __restrict__ quals, const uint32_t* __restrict__ qmask,
                                                   const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ len,
                                                   uint32_t min_qual, uint16_t* __restrict__ good,
                                                   unsigned long long* __restrict__ total_kmers,
                                                   uint32_t* __restrict__ max_len) {
    // The qualities of the block's 256 consecutive reads are contiguous.  They are read once with 16-byte loads and
    // reduced on the fly to ONE BIT per base (q >= min_qual) in LDS -- 5 KB per block instead of the 38 KB of raw bytes,
    // so the CU holds enough blocks to keep HBM busy -- and every lane then finds the rightmost run of K set bits of its
    // own read with shifted ANDs on 128-bit windows (a 150-base read is three windows).
    constexpr unsigned CH = 4096;                       // 16-byte chunks per block: 64 KB of qualities (256 reads x 256 bases)
    __shared__ __attribute__((aligned(16))) uint16_t gbits[CH + 16];
    __shared__ unsigned long long s_sum[4];
    __shared__ uint32_t s_max[4];
    const uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x;
    const uint64_t r = r0 + threadIdx.x;
    const uint64_t rend = r0 + blockDim.x < n ? r0 + blockDim.x : n;
    const uint64_t base0 = qoff[r0], endo = qoff[rend];
    const unsigned shift = MASK ? (unsigned)(base0 & 31) : (unsigned)((reinterpret_cast<uintptr_t>(quals) + base0) & 15);
    const unsigned n16 = (unsigned)((endo - base0 + shift + 15) >> 4);
    const bool in_lds = (endo - base0 + shift + 15) >> 4 <= CH;
    if (MASK && in_lds) {
        uint32_t* gw32 = reinterpret_cast<uint32_t*>(gbits);
        const uint32_t* src = qmask + (base0 >> 5);                  // (the mask has 17 zeroed words behind its last one)
        for (unsigned i = threadIdx.x; i < (n16 + 10 + 1) / 2; i += blockDim.x) gw32[i] = 2 * i < n16 + 1 ? src[i] : 0u;
    } else if (in_lds) {
        const uint4* src = reinterpret_cast<const uint4*>(quals + base0 - shift);
        for (unsigned i = threadIdx.x; i < n16 + 10; i += blockDim.x) {
            unsigned bits = 0;
            if (i < n16) {
                const uint4 v = src[i];
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (unsigned j = 0; j < 16; ++j) bits |= (((d[j >> 2] >> (8 * (j & 3))) & 0xFFu) >= min_qual ? 1u : 0u) << j;
            }
            gbits[i] = (uint16_t)bits;                  // zero chunks behind the data: the window loads below read defined bits
        }
    }
    __syncthreads();
    unsigned long long mine = 0;
    uint32_t L = 0;
    if (r < n) {
        L = len[r];
        const uint64_t o = qoff[r];
        uint32_t g = 0;
        if (in_lds) {
            const uint32_t* gw = reinterpret_cast<const uint32_t*>(gbits);
            const uint32_t b0 = shift + (uint32_t)(o - base0);                 // the read's first bit
            // windows of 64 start positions, from the top: Y[i] = X[i..i+59] all set needs the 123 bits from i on
            for (int32_t s0 = (int32_t)((L - 1) & ~63u); L >= K && s0 >= 0; s0 -= 64) {
                const uint32_t bit = b0 + (uint32_t)s0, wi = bit >> 5, sh = bit & 31;
                const uint32_t w0 = gw[wi], w1 = gw[wi + 1], w2 = gw[wi + 2], w3 = gw[wi + 3], w4 = gw[wi + 4];
                uint64_t lo = ((uint64_t)w0 | ((uint64_t)w1 << 32)) >> sh, hi = ((uint64_t)w2 | ((uint64_t)w3 << 32)) >> sh;
                if (sh) { lo |= (uint64_t)w2 << (64 - sh); hi |= (uint64_t)w4 << (64 - sh); }
                const uint32_t valid = L - (uint32_t)s0;                         // bits of this read from s0 on
                if (valid < 128) { if (valid <= 64) { hi = 0; lo &= valid == 64 ? ~0ull : ((1ull << valid) - 1); } else hi &= (1ull << (valid - 64)) - 1; }
                // runs of >= 2, 4, 8, 16, 32, 60 set bits starting at each position (128-bit shifts)
                auto step = [&](unsigned sft) { const uint64_t l2 = (lo >> sft) | (hi << (64 - sft)), h2 = hi >> sft; lo &= l2; hi &= h2; };
                step(1); step(2); step(4); step(8); step(16); step(28);
                if (lo) { g = (uint32_t)s0 + (63u - (uint32_t)__builtin_clzll(lo)) + K; break; }
            }
        } else {
            uint32_t run = 0;
            for (uint32_t i = L; i-- > 0;) {
                const bool ok = MASK ? ((qmask[(o + i) >> 5] >> ((o + i) & 31)) & 1u) != 0 : quals[o + i] >= min_qual;
                if (!ok) run = 0;
                else if (++run == K) { g = i + K; break; }
            }
        }
        uint16_t g16 = (uint16_t)g;
        good[r] = g16;
        if (g16 > K) mine = g16 - (K - 1);
    }
    // block reduce
    for (int o = 32; o > 0; o >>= 1) {
        mine += __shfl_down(mine, o);
        uint32_t m2 = __shfl_down(L, o);
        L = m2 > L ? m2 : L;
    }
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[w] = mine; s_max[w] = L; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        uint32_t m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        // a slot per block residue: 2 x 195 k atomics on ONE address serialise at ~11 ns each (4 ms, the whole kernel)
        if (t) atomicAdd(&total_kmers[blockIdx.x & (QSLOTS - 1)], t);
        if (m) atomicMax(&max_len[blockIdx.x & (QSLOTS - 1)], m);
    }
}

// PQVec -> raw qualities, one read per lane (feudal/PQVec.cc:129-188 semantics).
__global__ void __launch_bounds__(256) k_decode_pq(uint64_t n, const uint8_t* __restrict__ pq, const uint64_t* __restrict__ pqoff,
                                                    uint8_t* __restrict__ quals, const uint64_t* __restrict__ qoff) {
    uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint8_t* b = pq + pqoff[r];
    const uint8_t* bend = pq + pqoff[r + 1];
    uint8_t* out = quals + qoff[r];
    uint8_t* oend = quals + qoff[r + 1];
    while (b < bend) {
        unsigned nqs = *b++;
        if (!nqs) break;
        unsigned nbits = b[0] & 7;
        unsigned minq = ((b[0] >> 3) | ((unsigned)b[1] << 5)) & 63;
        unsigned nbytes = (nqs * nbits + 9 + 7) >> 3;
        unsigned bitpos = 9;
        unsigned mask = (1u << nbits) - 1;
        for (unsigned i = 0; i < nqs && out < oend; ++i) {
            unsigned v = 0;
            if (nbits) {
                unsigned by = bitpos >> 3, sh = bitpos & 7;
                unsigned w = b[by] | ((by + 1 < nbytes ? (unsigned)b[by + 1] : 0u) << 8);
                v = (w >> sh) & mask;
                bitpos += nbits;
            }
            *out++ = (uint8_t)(minq + v);
        }
        b += nbytes;
    }
    while (out < oend) *out++ = 0;           // a PQVec that holds fewer values than the read has bases (a damaged file): defined, quality 0
}

int decode_pq(Ctx& c, const uint8_t* d_pq, const uint64_t* d_pqoff, uint8_t* d_quals, const uint64_t* d_qoff) {
    if (!c.n) return 0;
    LAUNCH(c, "k_decode_pq", k_decode_pq, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, c.n, d_pq, d_pqoff, d_quals, d_qoff);
    W2_HIP(hipGetLastError());
    return 0;
}

// =============================================================================== K3
// Per-bucket LDS hash table: 16-B keys (hi, lo; hi == ~0 <=> empty, lo == ~0 <=> key being written)
// + one dword (bits 23:0 occurrence count, bits 31:24 OR of contexts) per slot.
//
// The kernel is a persistent, software-pipelined loop over buckets; nothing on the per-bucket
// critical path waits for HBM:
//  * bucket ids come from an atomic queue three buckets ahead, the record ranges of bucket i+2 and
//    the first record tile of bucket i+1 are loaded while bucket i is counted;
//  * a bucket's records (from all `nseg` source segments, as one logical dword stream) go through
//    LDS in tiles of TILE records with coalesced dword loads;
//  * inside a tile the k-mers of a wavefront's records are flattened (lane = k-mer): the record of
//    every lane comes from a per-wave bit vector of record starts (one uniform 64-bit word per
//    64-k-mer window, v_readlane + popcount; no search), the 124 stream bits of the k-mer and its
//    two flank bases are five LDS dwords, the reverse complement is the complement of the two
//    LSB-first halves swapped, and one probe is {key, count} read together followed by
//    fire-and-forget ds_add / ds_or;
//  * emit compacts the solid entries into an LDS staging area, reserves their output range with
//    ONE global atomic whose result is only consumed while the next bucket is emitted, and resets
//    exactly the slots that were occupied, so the table never needs a clearing pass.
// A bucket whose distinct set overflows the table is split by hash bits and recounted
// (= MapReduceEngine.h:288-291).
template <unsigned CAP, unsigned THREADS, bool PARK = true>
struct K3Cfg {
    static constexpr unsigned NW = THREADS / 64;
    static constexpr unsigned RPL = !PARK ? 16 : NW >= 16 ? 32 : 64;   // records per wave per tile (one per lane 0..RPL-1)
    static constexpr unsigned TILE = NW * RPL;                // records per tile
    static constexpr unsigned NPF = (TILE * REC_DWORDS + THREADS - 1) / THREADS;
    static constexpr unsigned SC = CAP / 8;                   // staging entries
    static constexpr unsigned QCAP = PARK ? 128 : 0;          // parked k-mers per wave (PARK = false: collisions are probed at once, no queue)
    static constexpr unsigned MAXSEG = 64;
    static constexpr unsigned LIMIT = CAP - THREADS - 8;
    static constexpr unsigned PER = CAP / THREADS;
    static constexpr unsigned LDS = CAP * 16 + SC * 16 + 3 * MAXSEG * 8 + NW * QCAP * 16 +
                                    (CAP + SC + TILE * REC_DWORDS + 4 + 3 * TILE + NW + NW * QCAP + 3 * (MAXSEG + 1) + 4 + 104 + 16 + 40 + 2 + 128) * 4;
};
enum { K3_FILL = 0, K3_OVF, K3_DEPTH, K3_CNT, K3_NPREV, K3_BASELO, K3_BASEHI, K3_B2LO, K3_B2HI, K3_WIN = 11 /* [10]: PROF */ };

__device__ inline uint32_t ld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void st32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline uint64_t ld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void st64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// inclusive prefix sum over the lanes of each 16-lane row (DPP row_shr, no LDS round trips) ...
__device__ inline uint32_t row_scan16(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
    return x;
}
// ... and over lanes 0..31 (row 0's total is added to row 1: row_bcast15 into rows 1 and 3)
__device__ inline uint32_t half_scan32(uint32_t x) {
    x = row_scan16(x);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
    return x;
}
// ... and over the whole wavefront (row_bcast31: lane 31's total into rows 2 and 3)
__device__ inline uint32_t wave_scan64(uint32_t x) {
    x = half_scan32(x);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
    return x;
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// 16-B LDS read that the compiler neither splits nor caches (the tag groups are polled)
__device__ inline u32x4 lds_read_b128(const uint32_t* p) {
    u32x4 v;
    const uint32_t a = (uint32_t)(uintptr_t)p;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(a) : "memory");
    return v;
}

// (PARK = false, MINW = 8: the round-3 experiment -- 2048 slots, 256-record tiles, no parking queue: 75 KB of LDS and <= 64 VGPRs, so that
//  TWO 1024-thread blocks share a CU, eight waves per SIMD instead of four; buckets of half the size)
template <unsigned CAP, unsigned THREADS, bool PROF = false, bool PARK = true, unsigned MINW = 1>
__global__ void __launch_bounds__(THREADS, MINW) k_count_buckets(uint32_t nb, uint32_t b_lo, uint32_t b_hi /* this launch counts buckets [b_lo, b_hi) of nb */,
                                                            uint32_t nseg, const uint64_t* __restrict__ roff,
                                                            const uint32_t* __restrict__ recs, uint32_t min_freq,
                                                            uint32_t* __restrict__ queue,
                                                            uint64_t* __restrict__ shi, uint64_t* __restrict__ slo,
                                                            uint32_t* __restrict__ scc, uint64_t solid_cap,
                                                            unsigned long long* __restrict__ counters /*0 solid | emits << 40,1 distinct,2 overflow passes,3 error*/,
                                                            unsigned long long* __restrict__ ghist,
                                                            uint64_t* __restrict__ chunk_start, uint32_t* __restrict__ chunk_cnt, uint32_t chunk_cap,
                                                            const uint32_t* __restrict__ blist /* null, or [0] = number of listed buckets, [2..] their ids:
                                                            the buckets k_count_fp deferred; `queue` then deals out list positions */, uint32_t blist_cap) {
    // Every emit reserves its output range AND a chunk number with one 64-bit atomic (count in bits 39:0, chunks above):
    // the solid k-mers of one bucket (class) lie contiguously, and the list of those chunks lets the adjacency prune work
    // bucket by bucket in LDS (k_prune_local) instead of probing the dictionary in HBM for every neighbour.
    constexpr unsigned long long SMASK = (1ull << 40) - 1;
    using C = K3Cfg<CAP, THREADS, PARK>;
    constexpr unsigned NW = C::NW, RPL = C::RPL, TILE = C::TILE, NPF = C::NPF, SC = C::SC, MAXSEG = C::MAXSEG, PER = C::PER, QCAP = C::QCAP;
    constexpr unsigned LOG_CAP = CAP == 4096 ? 12 : CAP == 2048 ? 11 : CAP == 1024 ? 10 : 13;
    static_assert((1u << LOG_CAP) == CAP, "CAP");
    constexpr uint64_t EMPTY = ~0ull;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);            // [CAP][2]: hi, lo
    uint64_t* sthi = keys + 2 * CAP;                               // staging
    uint64_t* stlo = sthi + SC;
    uint64_t* segbase = stlo + SC;                                 // [3][MAXSEG] dword index of a segment's share minus its logical start
    uint64_t* qhi = segbase + 3 * MAXSEG + (threadIdx.x >> 6) * QCAP;   // this wave's queue of parked k-mers
    uint64_t* qlo = qhi + NW * QCAP;
    uint32_t* cc = reinterpret_cast<uint32_t*>(segbase + 3 * MAXSEG + 2 * NW * QCAP);
    uint32_t* stcc = cc + CAP;
    uint32_t* tile = stcc + SC;                                    // TILE*9 (+4 pad)
    uint32_t* bv32 = tile + TILE * REC_DWORDS + 4;                 // [2*TILE] record-start bit vector of the tile's flattened k-mers
    uint32_t* Bw = bv32 + 2 * TILE;                                // [TILE] record covering the first position of each window
    uint32_t* wtot = Bw + TILE;                                    // [NW] k-mers per wave's records
    uint32_t* qmeta = wtot + NW + (threadIdx.x >> 6) * QCAP;       // parked k-mers: next slot to look at | ctx << 16
    uint32_t* segdpre = wtot + NW + NW * QCAP;                     // [3][MAXSEG+1] logical dword prefix of the segments
    uint32_t* bq = segdpre + 3 * (MAXSEG + 1);                     // ring of bucket ids
    uint32_t* lhist = bq + 4;                                      // 104
    uint32_t* misc = lhist + 104;                                  // 16
    uint32_t* stk = misc + 16;                                     // (class, P) pairs, depth <= 18
    uint64_t* dummy64 = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(stk + 40) + 7) & ~uintptr_t(7));   // [64] sink of the lanes that did not claim a slot
    const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the bucket behind ticket t of the queue: the t-th bucket of the range, or the t-th listed one
    const uint32_t nlist = blist ? (blist[0] < blist_cap ? blist[0] : blist_cap) : 0u;
    auto ticket = [&](uint32_t t) -> uint32_t { return blist ? (t < nlist ? blist[2 + t] : NONE32) : (t < b_hi - b_lo ? b_lo + t : NONE32); };

    // ---- segment table of bucket bb -> registers (wave 0, lane = segment), and from registers -> LDS ring slot
    auto seg_load = [&](uint32_t bb, uint64_t& r0, uint32_t& cnt) {
        r0 = 0; cnt = 0;
        if (tid < nseg && bb < b_hi) {
            // (SEG_PACKED in nb: roff[seg * nb + bb] is seg_pack(first record, records) -- the slab route's segments are no scan)
            const uint64_t at = (uint64_t)tid * (nb & ~SEG_PACKED) + bb;
            uint64_t a = roff[at], len;
            if (nb & SEG_PACKED) { len = a >> SEG_START_BITS; a &= (1ull << SEG_START_BITS) - 1; }
            else len = roff[at + 1] - a;
            r0 = a; cnt = (uint32_t)len;
            if (len >= (1ull << 26)) { cnt = 0; counters[3] = 2; }     // keeps 24-bit counts and 32-bit dword indices exact
        }
    };
    auto seg_store = [&](unsigned q, uint64_t r0, uint32_t cnt) {       // wave 0 only
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { uint32_t v = __shfl_up(incl, o); if ((int)lane >= o) incl += v; }
        uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (tot >= (1u << 26)) { tot = 0; incl = 0; cnt = 0; if (lane == 0) counters[3] = 2; }
        const uint32_t ex = incl - cnt;
        if (lane < nseg) { segdpre[q * (MAXSEG + 1) + lane] = ex * REC_DWORDS; segbase[q * MAXSEG + lane] = (r0 - ex) * REC_DWORDS; }
        if (lane == 0) segdpre[q * (MAXSEG + 1) + nseg] = tot * REC_DWORDS;
    };
    // ---- tile t of the bucket in ring slot q -> registers (coalesced dwords of the logical record stream)
    auto tile_load = [&](unsigned q, uint32_t t, uint32_t (&v)[NPF]) {
        const uint32_t* dp = segdpre + q * (MAXSEG + 1);
        const uint32_t dall = dp[nseg];
        const uint32_t d0 = t * (TILE * REC_DWORDS);
        const uint32_t dend = dall - d0 < TILE * REC_DWORDS ? dall : d0 + TILE * REC_DWORDS;
        // the segment of a dword = the number of segment boundaries at or below it: up to 8 segments the boundaries are read
        // once (independent LDS loads) and compared in registers instead of walked load by load
        constexpr unsigned NB_REG = 7;
        uint32_t bnd[NB_REG];
#pragma unroll
        for (unsigned i = 0; i < NB_REG; ++i) bnd[i] = (i + 1 < nseg && nseg <= NB_REG + 1) ? dp[i + 1] : 0xFFFFFFFFu;
#pragma unroll
        for (unsigned j = 0; j < NPF; ++j) {
            const uint32_t d = d0 + j * THREADS + tid;
            uint32_t x = 0;
            if (d0 < dall && d < dend) {
                unsigned s = 0;
                if (nseg <= NB_REG + 1) {
#pragma unroll
                    for (unsigned i = 0; i < NB_REG; ++i) s += d >= bnd[i] ? 1u : 0u;
                } else while (d >= dp[s + 1]) ++s;
                x = recs[segbase[q * MAXSEG + s] + d];
            }
            v[j] = x;
        }
    };
    auto tile_store = [&](const uint32_t (&v)[NPF]) {
#pragma unroll
        for (unsigned j = 0; j < NPF; ++j) { const unsigned i = j * THREADS + tid; if (i < TILE * REC_DWORDS) tile[i] = v[j]; }
    };

    // ---- init: empty table, first three bucket ids, segment tables of the first two, first tile
    for (unsigned i = tid; i < CAP; i += THREADS) { keys[2 * i] = EMPTY; keys[2 * i + 1] = EMPTY; cc[i] = 0; }
    for (unsigned i = tid; i < 104; i += THREADS) lhist[i] = 0;
    if (tid < 4) tile[TILE * REC_DWORDS + tid] = 0;
    if (tid < 16) misc[tid] = 0;
    if (tid == 0) { const uint32_t t0 = atomicAdd(queue, 3u); bq[0] = ticket(t0); bq[1] = ticket(t0 + 1); bq[2] = ticket(t0 + 2); bq[3] = NONE32; }
    __syncthreads();
    if (wv == 0) {
        uint64_t r0; uint32_t cnt;
        seg_load(bq[0], r0, cnt); seg_store(0, r0, cnt);
        seg_load(bq[1], r0, cnt); seg_store(1, r0, cnt);
    }
    __syncthreads();
    uint32_t pf[NPF];
    tile_load(0, 0, pf);
    unsigned long long pend_base = 0, my_distinct = 0;
    // PROF: shader-clock time of wave 0 per phase (stage-in, count, barrier A, flush+scan, barrier B, staging), summed into counters[106..]
    unsigned long long pt[6] = {0, 0, 0, 0, 0, 0}, tp = 0, ptmax = 0, wt[5] = {0, 0, 0, 0, 0}, wtp = 0, wcount = 0;
    auto wtick = [&](int ph) { if (PROF && wv == 0) { const unsigned long long now = __builtin_amdgcn_s_memtime(); if (ph >= 0) wt[ph] += now - wtp; wtp = now; } };
    auto tick = [&](int ph) { if (PROF) { const unsigned long long now = __builtin_amdgcn_s_memtime(); if (ph >= 0) pt[ph] += now - tp; tp = now; } };

    // ---- the full probe sequence for the lanes with `live`: find the key or claim a free slot from slot s on; count + context.
    //      Returns whether this lane inserted a NEW key.
    unsigned qn = 0;
    bool big = false;
    auto probe = [&](bool live, Kmer k, unsigned s, unsigned ctx) -> bool {
        bool isnew = false;
        if (live) {
            bool ok = false;
            int budget = 2 * (int)CAP;
            for (;;) {
                bool emp;
                for (;;) {                                           // search only: tight single-exit loop
                    const uint64_t khi = ld64(&keys[2 * s]), klo = ld64(&keys[2 * s + 1]);
                    const bool same_hi = khi == k.hi;
                    emp = khi == EMPTY;
                    const bool hit = same_hi & (klo == k.lo), busy = same_hi & (klo == EMPTY);
                    --budget;
                    if (hit | emp | (budget <= 0)) break;
                    s = busy ? s : ((s + 1) & (CAP - 1));
                }
                if (budget <= 0) break;                              // table full
                if (!emp) { ok = true; break; }
                const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&keys[2 * s]), (unsigned long long)EMPTY,
                                               (unsigned long long)k.hi);
                if (old == EMPTY) { st64(&keys[2 * s + 1], k.lo); isnew = true; ok = true; break; }
            }
            if (ok) {
                if (!big || (ld32(&cc[s]) & 0xFFFFFFu) < 0xFFF000u) atomicAdd(&cc[s], 1u);
                atomicOr(&cc[s], ctx << 24);
            } else st32(&misc[K3_OVF], 1u);                          // table full: recount in two classes
        }
        return isnew;
    };
    // ---- finish the top `cnt` (<= 64) parked k-mers of this wave; returns the new keys
    auto drain = [&](unsigned cnt) -> unsigned {
        wave_lds_fence();
        bool isnew = false;
        if (PARK) {
            const bool live = lane < cnt;
            const unsigned e = live ? qn - cnt + lane : 0u;
            Kmer k{0, 0}; uint32_t meta = 0;
            if (live) { k = Kmer{qhi[e], qlo[e]}; meta = qmeta[e]; }
            isnew = probe(live, k, meta & 0xFFFFu, meta >> 16);
        }
        qn -= cnt;
        wave_lds_fence();
        return (unsigned)__builtin_popcountll(__ballot(isnew));
    };

    for (uint32_t it = 0;; ++it) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&bq[it & 3]));       // block-uniform values are kept in SGPRs: scalar branches
        if (b >= b_hi) break;
        const unsigned q = it % 3;
        tick(-1);
        const uint32_t nrec = (uint32_t)__builtin_amdgcn_readfirstlane((int)segdpre[q * (MAXSEG + 1) + nseg]) / REC_DWORDS;
        const uint32_t ntiles = (nrec + TILE - 1) / TILE;
        big = nrec >= (1u << 18);
        // ---- stage in this bucket's first tile; start the look-ahead loads (consumed before barrier A)
        tile_store(pf);
        uint32_t la_b = 0;
        if (tid == 0) la_b = ticket(atomicAdd(queue, 1u));
        uint64_t la_r0 = 0; uint32_t la_cnt = 0;
        if (wv == 0) seg_load(ld32(&bq[(it + 2) & 3]), la_r0, la_cnt);
        tile_load((it + 1) % 3, 0, pf);
        if (tid == 0) { stk[0] = 0; stk[1] = 1; misc[K3_DEPTH] = 1; }
        bool first_pass = true;
        __syncthreads();                                             // S1
        tick(0);
        unsigned long long tp0 = 0; if (PROF) tp0 = __builtin_amdgcn_s_memtime();
        for (;;) {                                                   // (class, P) work stack; normally one pass
            const unsigned sp = ld32(&misc[K3_DEPTH]) - 1;
            const uint32_t cls = stk[2 * sp], P = stk[2 * sp + 1];
            for (uint32_t t = 0; t < ntiles; ++t) {
                if (t > 0 || (!first_pass && ntiles > 1)) {          // rare: bucket longer than one tile / recount
                    uint32_t tmp[NPF];
                    tile_load(q, t, tmp);
                    __syncthreads();
                    tile_store(tmp);
                    __syncthreads();
                }
                const unsigned nrec_tile = nrec - t * TILE < TILE ? nrec - t * TILE : TILE;
                // Flatten the tile's k-mers: record G = wv*32 + l (scanned by lane l of wave wv) occupies positions
                // [e, e+nk) of the tile-wide k-mer numbering.  bv = one bit per
                // position where a record starts; Bw[w] = (G << 16 | e) of the record covering position 64*w.
                // Window w (64 consecutive positions) is counted by wave w % NW, so every wave gets the same
                // number of k-mers whatever the records' lengths are.
                const unsigned myrec = wv * RPL + lane;
                const unsigned nk = (lane < RPL && myrec < nrec_tile) ? (tile[myrec * REC_DWORDS] & 63u) + 1u : 0u;
                const unsigned incl = RPL == 32 ? half_scan32(nk) : wave_scan64(nk);
                if (lane == RPL - 1) wtot[wv] = incl;
                for (unsigned i = tid; i < 2 * TILE; i += THREADS) bv32[i] = 0;
                if (tid == 0) misc[K3_WIN] = 2 * NW;                 // windows 0 .. 2 NW - 1 are dealt out statically, the rest on demand
                __syncthreads();                                     // X1
                const unsigned wsum = lane < NW ? wtot[lane] : 0u, wsc = row_scan16(wsum);
                const int wvu = __builtin_amdgcn_readfirstlane((int)wv);
                const unsigned base = (unsigned)__builtin_amdgcn_readlane((int)wsc, wvu) - (unsigned)__builtin_amdgcn_readlane((int)wsum, wvu);
                const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)wsc, NW - 1);
                if (nk) {
                    const unsigned e = base + incl - nk;
                    atomicOr(&bv32[e >> 5], 1u << (e & 31));
                    const unsigned w1 = (e + 63) >> 6;
                    if (64 * w1 < e + nk) Bw[w1] = (myrec << 16) | e;
                }
                __syncthreads();                                     // X2
                // ---- the windows of this wave, as three stages:
                //   A(w): locate every lane's k-mer (record, index) and fetch its 6 stream dwords;
                //   B(w): cut out the k-mer, canonicalise, hash, fetch the key at its home slot;
                //   C(w): hit -> count / free -> claim / anything else -> park.
                // (Interleaving the stages of three consecutive windows inside one wave -- B(w+1), A(w+2), C(w) -- was measured:
                // 165 VGPRs at 512 threads, 65 ms against 45 ms for this form with 16 waves per CU.)
                // The loop body is STRAIGHT-LINE, predicated code.  A wave issues one instruction per ~5 clocks whatever its
                // kind, and a divergent `if` (v_cmp -> s_and_saveexec -> ... -> s_or exec) costs ~37 clocks against ~18 for
                // v_cmp + v_cndmask (tools/issue_ubench.hip), so: the window counter and everything derived from it are
                // SCALAR (readfirstlane), LDS reads of lanes without a k-mer are clamped instead of masked, the claim is an
                // unconditional CAS (a lane that does not want the slot swaps EMPTY for EMPTY), lanes that did not win
                // store their low word into a per-lane dummy, count/context go through `add 0` / `or 0`, and every lane
                // writes one queue entry (parked lanes first, the others behind the new top).
                uint32_t fill_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&misc[K3_FILL])),
                         ovf_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&misc[K3_OVF]));
                const unsigned nwin = (total + 63) / 64;
                const unsigned wv_s = (unsigned)wvu;                 // this wave's number as a scalar
                uint32_t nM0 = 0, nM1 = 0, nB = 0;                   // start bits / covering record of the window handled next
                { const unsigned w0 = wv_s < nwin ? wv_s : 0u; nM0 = bv32[2 * w0]; nM1 = bv32[2 * w0 + 1]; nB = Bw[w0]; }
                const uint64_t lane_le = ~0ull >> (63 - lane);
                const unsigned dummy_at = (unsigned)(dummy64 - keys);
                const uint32_t lane_lt_lo = lane < 32 ? (1u << lane) - 1u : 0xFFFFFFFFu, lane_lt_hi = lane < 32 ? 0u : (1u << (lane - 32)) - 1u;
                // Windows are dealt out ON DEMAND: the hardware issues from the oldest wave first, so with a fixed share per wave
                // the waves of a block finish 30 % apart and everyone waits at barrier A for the youngest (measured: 52 M clocks
                // for waves 0-3, 72 M for waves 12-15).  Each wave starts with windows wv and wv + NW and draws the index of the
                // window after next from an LDS counter while it works on the current one.
                unsigned wnext = wv_s + NW;
                for (unsigned w = wv_s; w < nwin;) {
                    // the (one window stale) overflow checks, on scalars
                    if (ovf_seen) break;
                    if (fill_seen >= C::LIMIT) { if (lane == 0) st32(&misc[K3_OVF], 1u); break; }
                    const uint32_t fill_ld = ld32(&misc[K3_FILL]), ovf_ld = ld32(&misc[K3_OVF]);
                    uint32_t wdraw = 0;
                    if (lane == 0) wdraw = atomicAdd(&misc[K3_WIN], 1u);
                    wtick(-1);
                    // ---- A: locate every lane's k-mer (record, index) and fetch its 6 stream dwords
                    const uint32_t M0 = nM0, M1 = nM1, Bv = nB;
                    { const unsigned wn = wnext < nwin ? wnext : w; nM0 = bv32[2 * wn]; nM1 = bv32[2 * wn + 1]; nB = Bw[wn]; }
                    const unsigned g = w * 64 + lane;
                    bool active = g < total;
                    const uint32_t mle0 = M0 & (uint32_t)lane_le, mle1 = M1 & (uint32_t)(lane_le >> 32);
                    const unsigned c = (unsigned)__builtin_popcount(mle0 & ~1u) + (unsigned)__builtin_popcount(mle1);
                    // highest record start at or below this lane (bit 0 forced: defined for c == 0, where it is not used)
                    const unsigned top = mle1 ? 63u - (unsigned)__builtin_clz(mle1) : 31u - (unsigned)__builtin_clz(mle0 | 1u);
                    const unsigned idx = lane - (c ? top : (Bv & 0xFFFFu) - w * 64);
                    const unsigned rec = active ? (Bv >> 16) + c : 0u;
                    const uint32_t* wp = tile + rec * REC_DWORDS;
                    const unsigned q0 = active ? (idx + REC_HB / 2) >> 4 : 0u;      // the stream starts at bit REC_HB of the record: base t at bit REC_HB + 2 t
                    const uint32_t hdr = wp[0], d0 = wp[q0], d1 = wp[1 + q0], d2 = wp[2 + q0], d3 = wp[3 + q0], d4 = wp[4 + q0];
                    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); wtick(0); }
                    // ---- B: cut out the k-mer, canonicalise, hash, fetch the key at its home slot
                    const unsigned sh = ((idx + REC_HB / 2) & 15u) * 2u;
                    // 128 stream bits from base idx: 1:0 left flank, 2..121 the k-mer, 123:122 right flank (32-bit ops only)
                    const uint32_t e0 = __funnelshift_r(d0, d1, sh), e1 = __funnelshift_r(d1, d2, sh),
                                   e2 = __funnelshift_r(d2, d3, sh), e3 = __funnelshift_r(d3, d4, sh);
                    const uint32_t s0l = __funnelshift_r(e0, e1, 2), s0h = (e1 >> 2) & 0x0FFFFFFFu;       // bases 0..29, LSB first
                    const uint32_t s1l = __funnelshift_r(e1, e2, 30), s1h = __funnelshift_r(e2, e3, 30) & 0x0FFFFFFFu;
                    auto rev2_32 = [](uint32_t x) { x = __brev(x); return ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u); };
                    // MSB-first words: reverse the 30 groups of each half
                    const uint32_t a0 = rev2_32(s0l), b0 = rev2_32(s0h), a1 = rev2_32(s1l), b1 = rev2_32(s1h);
                    const uint32_t khh = a0 >> 4, khl = __funnelshift_r(b0, a0, 4), klh = a1 >> 4, kll = __funnelshift_r(b1, a1, 4);
                    // reverse complement = complemented LSB-first halves, swapped
                    const uint32_t rhh = ~s1h & 0x0FFFFFFFu, rhl = ~s1l, rlh = ~s0h & 0x0FFFFFFFu, rll = ~s0l;
                    const uint64_t khi_f = ((uint64_t)khh << 32) | khl, klo_f = ((uint64_t)klh << 32) | kll;
                    const uint64_t khi_r = ((uint64_t)rhh << 32) | rhl, klo_r = ((uint64_t)rlh << 32) | rll;
                    const bool rc = khi_r != khi_f ? khi_r < khi_f : klo_r < klo_f;
                    const Kmer k{rc ? khi_r : khi_f, rc ? klo_r : klo_f};
                    // context (KMerContext: bits 0..3 successors, 4..7 predecessors); under reverse complement the predecessor L
                    // becomes the successor 3-L and the successor R the predecessor 3-R: the shift amounts are L^4 | R forward, L^3 | R^7 reversed
                    const unsigned rnk_ = (hdr & 63u) + 1u;
                    const bool hasp = (idx > 0) | ((hdr & 64u) != 0), hass = (idx + 1 < rnk_) | ((hdr & 128u) != 0);
                    const unsigned shl_p = (e0 & 3u) ^ (rc ? 3u : 4u), shl_s = ((e3 >> 26) & 3u) ^ (rc ? 7u : 0u);
                    const unsigned ctx = (hasp ? 1u << shl_p : 0u) | (hass ? 1u << shl_s : 0u);
                    const uint32_t fa = (uint32_t)k.hi ^ (uint32_t)(k.lo >> 32), fb = (uint32_t)(k.hi >> 32) ^ (uint32_t)k.lo;
                    const uint32_t h1 = (fa + ((fb << 16) | (fb >> 16))) * 0x9E3779B1u;
                    const unsigned s = h1 >> (32 - LOG_CAP);
                    active &= ((h1 >> 2) & (P - 1)) == cls;
                    const uint64_t h0 = ld64(&keys[2 * s]), l0 = ld64(&keys[2 * s + 1]);
                    wtick(1);
                    // ---- C: ONE look at the key's home slot.  Hit -> count; free -> claim (64-bit CAS on hi, then lo); anything
                    //      else (another key there, a lost claim, an owner still writing) is parked in the wave's private queue and
                    //      finished later 64 at a time, so the data-dependent probe sequences never run with a handful of live lanes.
                    const bool hit = active & (h0 == k.hi) & (l0 == k.lo);
                    const bool want = active & !hit & (h0 == EMPTY);
                    const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&keys[2 * s]), (unsigned long long)EMPTY,
                                                   (unsigned long long)(want ? k.hi : EMPTY));
                    const bool won = want & (old == EMPTY);
                    st64(&keys[won ? 2 * s + 1 : dummy_at + lane], k.lo);                  // (an index select keeps it a ds_write; a pointer select becomes a FLAT store)
                    const bool done = hit | won;
                    // only min(255, count) is ever used (:943-949): 24 bits cannot wrap while the bucket has < 2^18 records
                    uint32_t inc = done ? 1u : 0u;
                    if (big) inc = (done && (ld32(&cc[s]) & 0xFFFFFFu) < 0xFFF000u) ? 1u : 0u;
                    atomicAdd(&cc[s], inc);
                    atomicOr(&cc[s], done ? ctx << 24 : 0u);
                    const bool parked = active & !done;
                    unsigned nnew = (unsigned)__builtin_popcountll(__ballot(won));
                    if (PARK) {
                        const unsigned long long pm = __ballot(parked);
                        const unsigned below = (unsigned)__builtin_popcount((uint32_t)pm & lane_lt_lo) + (unsigned)__builtin_popcount((uint32_t)(pm >> 32) & lane_lt_hi);
                        const unsigned npark = (unsigned)__builtin_popcountll(pm);
                        {   // parked lanes take qn .. qn+npark-1, the others the (unused) entries behind them: qn + 63 <= 126 < QCAP
                            const unsigned e = qn + (parked ? below : npark + lane - below);
                            qhi[e] = k.hi; qlo[e] = k.lo; qmeta[e] = s | (ctx << 16);
                        }
                        qn += npark;
                        if (qn >= 64) nnew += drain(64);
                    } else if (__any(parked)) {                      // (eight waves per SIMD cover the divergent probe sequences)
                        wave_lds_fence();
                        nnew += (unsigned)__builtin_popcountll(__ballot(probe(parked, k, s, ctx)));
                        wave_lds_fence();
                    }
                    if (nnew && lane == 0) atomicAdd(&misc[K3_FILL], nnew);
                    fill_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)fill_ld); ovf_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ovf_ld);
                    w = wnext; wnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)wdraw);
                    if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); wtick(3); if (wv == 0) wt[4] += 1; }
                }
                {   // leftovers of this tile
                    unsigned nnew = 0;
                    while (qn) nnew += drain(qn < 64 ? qn : 64);
                    if (nnew && lane == 0) atomicAdd(&misc[K3_FILL], nnew);
                }
            }
            if (PROF) { if (lane == 0) { const uint32_t dt = (uint32_t)(__builtin_amdgcn_s_memtime() - tp0); atomicMax(&misc[10], dt); wcount += dt; } }
            tick(1);
            // ---- publish the look-ahead results and last emit's output base (their loads had the whole count phase)
            if (first_pass) {
                if (wv == 0) seg_store((it + 2) % 3, la_r0, la_cnt);
                if (tid == 0) st32(&bq[(it + 3) & 3], la_b);
                first_pass = false;
            }
            if (tid == 0) { misc[K3_BASELO] = (uint32_t)pend_base; misc[K3_BASEHI] = (uint32_t)(pend_base >> 32); misc[K3_CNT] = 0; }
            __syncthreads();                                         // A: all inserts done
            tick(2);
            if (PROF && tid == 0) { ptmax += misc[10]; misc[10] = 0; }
            {   // flush the previous emit's staging area: coalesced 8-B / 4-B stores
                const uint32_t nprev = misc[K3_NPREV];
                const unsigned long long pk = (unsigned long long)misc[K3_BASELO] | ((unsigned long long)misc[K3_BASEHI] << 32);
                const unsigned long long gb = pk & SMASK;
                for (unsigned i = tid; i < nprev; i += THREADS)
                    if (gb + i < solid_cap) { shi[gb + i] = sthi[i]; slo[gb + i] = stlo[i]; scc[gb + i] = stcc[i]; }
                if (tid == 0 && nprev && chunk_start && (pk >> 40) < chunk_cap) { chunk_start[pk >> 40] = gb; chunk_cnt[pk >> 40] = nprev; }
            }
            if (ld32(&misc[K3_OVF])) {                               // distinct set does not fit: refine this class and retry
                __syncthreads();
                for (unsigned i = tid; i < CAP; i += THREADS) { keys[2 * i] = EMPTY; keys[2 * i + 1] = EMPTY; cc[i] = 0; }
                if (tid == 0) {
                    misc[K3_NPREV] = 0; misc[K3_FILL] = 0; misc[K3_OVF] = 0;
                    atomicAdd(&counters[2], 1ull);
                    if (P >= (1u << 16)) { counters[3] = 1; misc[K3_DEPTH] = sp; }
                    else { stk[2 * sp] = cls + P; stk[2 * sp + 1] = 2 * P; stk[2 * sp + 2] = cls; stk[2 * sp + 3] = 2 * P; misc[K3_DEPTH] = sp + 2; }
                }
                __syncthreads();
                if (ld32(&misc[K3_DEPTH]) == 0) break;
                continue;
            }
            // ---- emit: histogram over ALL distinct k-mers (:1097); solid ones (:1098-1100) -> staging
            uint32_t vals[PER];
            unsigned long long sm[PER];
            unsigned nsolid = 0;
#pragma unroll
            for (unsigned j = 0; j < PER; ++j) {
                const unsigned i = j * THREADS + tid;
                const uint32_t v = cc[i];
                const bool occ = (v & 0xFFFFFFu) != 0;
                uint32_t cnt = v & 0xFFFFFFu; if (cnt > 255) cnt = 255;          // :943-949 saturating u8
                const unsigned long long m1 = __ballot(occ && cnt == 1);           // singletons (sequencing errors) dominate
                if (m1 && lane == (unsigned)__builtin_ctzll(m1)) atomicAdd(&lhist[1], (uint32_t)__builtin_popcountll(m1));
                if (occ && cnt != 1) atomicAdd(&lhist[cnt > 100 ? 100 : cnt], 1u);
                if (occ) ++my_distinct;
                const bool solid = occ && cnt >= min_freq;
                if (occ) { cc[i] = 0; }
                if (occ && !solid) { keys[2 * i] = EMPTY; keys[2 * i + 1] = EMPTY; }
                vals[j] = solid ? (cnt | ((v >> 24) << 8) | 0x80000000u) : 0u;
                sm[j] = __ballot(solid);
                nsolid += (unsigned)__builtin_popcountll(sm[j]);
            }
            uint32_t wbase = 0;
            if (nsolid && lane == 0) wbase = atomicAdd(&misc[K3_CNT], nsolid);
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
            tick(3);
            __syncthreads();                                         // B: staging flushed, solid total known
            tick(4);
            const uint32_t tot = ld32(&misc[K3_CNT]);
            if (tot <= SC) {
                if (tid == 0) {
                    misc[K3_NPREV] = tot; misc[K3_FILL] = 0; misc[K3_DEPTH] = sp;
                    pend_base = tot ? atomicAdd(&counters[0], (1ull << 40) | tot) : 0ull;          // consumed at the next barrier A
                }
                unsigned run = wbase;
#pragma unroll
                for (unsigned j = 0; j < PER; ++j) {
                    if (vals[j] >> 31) {
                        const unsigned i = j * THREADS + tid;
                        const unsigned pos = run + (unsigned)__builtin_popcountll(sm[j] & ((1ull << lane) - 1));
                        sthi[pos] = keys[2 * i]; stlo[pos] = keys[2 * i + 1]; stcc[pos] = vals[j] & 0xFFFFu;
                        keys[2 * i] = EMPTY; keys[2 * i + 1] = EMPTY;
                    }
                    run += (unsigned)__builtin_popcountll(sm[j]);
                }
            } else {                                                 // more solid k-mers than the staging area holds: direct
                if (tid == 0) {
                    const unsigned long long pk = atomicAdd(&counters[0], (1ull << 40) | tot), base = pk & SMASK;
                    if (chunk_start && (pk >> 40) < chunk_cap) { chunk_start[pk >> 40] = base; chunk_cnt[pk >> 40] = tot; }
                    misc[K3_B2LO] = (uint32_t)base; misc[K3_B2HI] = (uint32_t)(base >> 32);
                    misc[K3_NPREV] = 0; misc[K3_FILL] = 0; misc[K3_DEPTH] = sp; pend_base = 0;
                }
                __syncthreads();
                const unsigned long long gb = (unsigned long long)misc[K3_B2LO] | ((unsigned long long)misc[K3_B2HI] << 32);
                unsigned run = wbase;
#pragma unroll
                for (unsigned j = 0; j < PER; ++j) {
                    if (vals[j] >> 31) {
                        const unsigned i = j * THREADS + tid;
                        const unsigned long long pos = gb + run + (unsigned)__builtin_popcountll(sm[j] & ((1ull << lane) - 1));
                        if (pos < solid_cap) { shi[pos] = keys[2 * i]; slo[pos] = keys[2 * i + 1]; scc[pos] = vals[j] & 0xFFFFu; }
                        keys[2 * i] = EMPTY; keys[2 * i + 1] = EMPTY;
                    }
                    run += (unsigned)__builtin_popcountll(sm[j]);
                }
            }
            tick(5);
            if (sp == 0) break;                                      // common case: the next bucket's barrier S1 closes this emit
            __syncthreads();                                         // C
        }
    }
    // ---- drain: last staging area, histogram, distinct count
    __syncthreads();
    if (tid == 0) { misc[K3_BASELO] = (uint32_t)pend_base; misc[K3_BASEHI] = (uint32_t)(pend_base >> 32); }
    __syncthreads();
    {
        const uint32_t nprev = misc[K3_NPREV];
        const unsigned long long pk = (unsigned long long)misc[K3_BASELO] | ((unsigned long long)misc[K3_BASEHI] << 32);
        const unsigned long long gb = pk & SMASK;
        for (unsigned i = tid; i < nprev; i += THREADS)
            if (gb + i < solid_cap) { shi[gb + i] = sthi[i]; slo[gb + i] = stlo[i]; scc[gb + i] = stcc[i]; }
        if (tid == 0 && nprev && chunk_start && (pk >> 40) < chunk_cap) { chunk_start[pk >> 40] = gb; chunk_cnt[pk >> 40] = nprev; }
    }
    for (unsigned i = tid; i < 101; i += THREADS) if (lhist[i]) atomicAdd(&ghist[i], (unsigned long long)lhist[i]);
    for (int o = 32; o > 0; o >>= 1) my_distinct += __shfl_down(my_distinct, o);
    if (lane == 0 && my_distinct) atomicAdd(&counters[1], my_distinct);
    if (PROF && tid == 0) { for (int i = 0; i < 6; ++i) atomicAdd(&counters[106 + i], pt[i]); atomicAdd(&counters[112], ptmax);
                            for (int i = 0; i < 5; ++i) atomicAdd(&counters[113 + i], wt[i]); }
    if (PROF && lane == 0) atomicAdd(&counters[124 + wv], wcount);          // count-phase clocks of every wave
}

// =============================================================================== K3, round 4: fingerprint + reference slots
// The same counting (collapse_entries :1002-1013, combine_Entries :943-949, filter + histogram :1094-1104) with an LDS table of
// 8 B per slot instead of 20: a slot holds a 16-bit TAG of the k-mer's hash and a 16-bit REFERENCE (record, index) to the first
// instance of that k-mer among the bucket's super-k-mer records, which stay resident in LDS for the whole bucket, plus the usual
// count | context word.  Equality is still decided by CONTENT: a tag match is verified against the referenced instance's 120 bits
// (five LDS dwords, compared with this instance as extracted and as its reverse complement -- the referenced instance needs no
// canonicalisation).  4096 slots + 640 records + staging are 76 KB, so TWO blocks share a CU at the bucket size that one 157-KB
// block of k_count_buckets needed: one block's barriers, stage-in and emit run under the other block's window loop.
// What does not fit this shape -- more records than the resident tile, more than MAXK k-mers, a distinct set beyond the table, more
// segments than MAXSEG -- is DEFERRED: the bucket's id goes to a list that k_count_buckets (list mode) counts afterwards.
// The resident tile keeps the records at their own stride, 8 dwords.  An ODD stride (-DW2RAP_FP_TS9: the five stream words of neighbouring
// records on different LDS banks, 30 % conflict cycles instead of 41 %) was measured in round 4 and is WORSE for the step: k_count_fp
// 39.6 -> 39.0 ms, but k_table_insert beside it on the side stream 17 -> 31 ms (its solo speed against half of it) and the step 108.6 -> 114.2
// ms -- the same pair of numbers the 36-B records (stride 9) gave.  Not the LDS footprint (W2RAP_K3=22 with stride 9 is as large as the
// default with stride 8 and as slow), not the registers, not the stream priorities (the other way round and level: unchanged); unexplained.
#ifdef W2RAP_FP_TS9
constexpr unsigned FP_TS = REC_DWORDS | 1u;
#else
constexpr unsigned FP_TS = REC_DWORDS;
#endif
__device__ inline unsigned fp_tile_index(unsigned d) { return FP_TS == REC_DWORDS ? d : d + d / REC_DWORDS; }   // dword d of the record stream -> its place in the tile
template <unsigned THREADS, unsigned TILE_, unsigned SC_>
struct FpCfg {
    static constexpr unsigned CAP = 4096, LOG_CAP = 12, NW = THREADS / 64;
    static constexpr unsigned TILE = TILE_;                                   // records resident per bucket (a reference holds 10 bits of record)
    static constexpr unsigned ROUNDS = (TILE + THREADS - 1) / THREADS;        // records per thread in the flatten scan
    static constexpr unsigned MAXK = 16384, MAXWIN = MAXK / 64;               // flattened k-mers per bucket
    static constexpr unsigned PFREC = TILE < 512 ? TILE : 512;                // records whose dwords are prefetched into registers one bucket ahead ...
    static constexpr unsigned NPF = (PFREC * REC_DWORDS + THREADS - 1) / THREADS;   // ... the rare rest of a big bucket is loaded when its turn comes
    static constexpr unsigned SC = SC_;                                       // solid k-mers per bucket (references staged in LDS; more: deferred)
    static constexpr unsigned QCAP = 128;                                     // parked references per wave
    static constexpr unsigned MAXSEG = 16;
    static constexpr unsigned LIMIT = CAP - THREADS - 8 < 3072 ? CAP - THREADS - 8 : 3072;
    static constexpr unsigned PER = CAP / THREADS;
    static constexpr unsigned OCAP = CAP;                                     // occupied slots a bucket can end with
    static constexpr unsigned LDS = 3 * MAXSEG * 8 +
                                    (2 * CAP + TILE * FP_TS + 8 + MAXK / 32 + 2 + MAXWIN + 2 + 2 * SC + NW * QCAP + 3 * (MAXSEG + 1) + 32 + 4 + 104 + 16 + 40 + (OCAP + 1) / 2) * 4;
    // record dedup (NOTES.md section 18): a table of record ids, at most half full, and 16-bit counts of each record's further copies; both are needed
    // from barrier S1 to the flatten only and lie over stcc / stref / the parking queues, which the window loop and the emit use.  What
    // lives through the window loop is one word per DISTINCT record (record | copies << 16), behind olist
    static constexpr unsigned DT = TILE <= 512 ? 1024 : 2048, LOG_DT = TILE <= 512 ? 10 : 11;
    static constexpr unsigned DAREA = DT + (TILE + 1) / 2;
    static constexpr unsigned LDS_DEDUP = LDS + TILE * 4;
    static_assert(TILE < 1023 && ROUNDS * NW <= 16 && (1u << LOG_CAP) == CAP, "FpCfg");
    static_assert(DT >= 2 * TILE && DAREA <= 2 * SC + NW * QCAP && TILE * 64 < 65536 && (OCAP & 1) == 0, "FpCfg: record dedup");
};
enum { FP_FILL = 0, FP_OVF, FP_CNT, FP_BASELO, FP_BASEHI, FP_WIN, FP_DEPTH };
#ifndef W2RAP_FP_TICKETS
#define W2RAP_FP_TICKETS 4
#endif
constexpr uint32_t FP_TICKETS = W2RAP_FP_TICKETS;          // buckets a block takes from the queue per atomic (a power of two)
static_assert((FP_TICKETS & (FP_TICKETS - 1)) == 0, "FP_TICKETS");

// one k-mer instance of the resident tile: the words every stage needs
struct FpInst {
    uint32_t s[4];                  // as extracted, LSB first: bases 0..15 | 16..29 | 30..45 | 46..59 (32 + 28 + 32 + 28 bits)
    uint32_t e0, e3;                // the stream words that carry the flanks
};
__device__ inline FpInst fp_fetch(const uint32_t* tile, unsigned rec, unsigned idx) {
    const uint32_t* wp = tile + rec * FP_TS;
    const unsigned q0 = (idx + REC_HB / 2) >> 4, sh = ((idx + REC_HB / 2) & 15u) * 2u;       // base t of the record at bit REC_HB + 2 t
    const uint32_t d0 = wp[q0], d1 = wp[1 + q0], d2 = wp[2 + q0], d3 = wp[3 + q0], d4 = wp[4 + q0];
    FpInst x;
    const uint32_t e0 = __funnelshift_r(d0, d1, sh), e1 = __funnelshift_r(d1, d2, sh), e2 = __funnelshift_r(d2, d3, sh), e3 = __funnelshift_r(d3, d4, sh);
    // 128 stream bits from base idx: 1:0 left flank, 2..121 the k-mer, 123:122 right flank
    x.s[0] = __funnelshift_r(e0, e1, 2); x.s[1] = (e1 >> 2) & 0x0FFFFFFFu;
    x.s[2] = __funnelshift_r(e1, e2, 30); x.s[3] = __funnelshift_r(e2, e3, 30) & 0x0FFFFFFFu;
    x.e0 = e0; x.e3 = e3;
    return x;
}
// the canonical form of an instance (MSB-first 2 x 60 bits as everywhere else), whether the reverse complement was taken, and the
// instance as extracted in MSB-first words (what a verification compares a reference's reverse complement with)
struct FpKey { uint64_t hi, lo; bool rc; uint32_t f[4]; };
__device__ inline FpKey fp_key(const FpInst& x) {
    // The bases of a word in reverse order are its bit reverse with the two bits of every base swapped back: two shifts and one bit-field
    // insert under 0xAAAAAAAA.  The upper word of a half (its last 14 bases, then 4 zero bits) takes the `>> 4` into those two shifts; the
    // lower word (bases 14 .. 29 of the half) is cut out of the half by one funnel shift BEFORE the reverse, so no 28-bit word is reversed
    // on its own and masked (9 instructions a half instead of 11)
    // (the insert is written out: the compiler, knowing the zero bits of a shifted word, narrows the two masks and then needs AND + AND-OR)
    auto pick = [](uint32_t odd, uint32_t even) { uint32_t r; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(0xAAAAAAAAu), "v"(odd), "v"(even)); return r; };
    const uint32_t r0 = __brev(x.s[0]), r1 = __brev(__funnelshift_r(x.s[0], x.s[1], 28)), r2 = __brev(x.s[2]), r3 = __brev(__funnelshift_r(x.s[2], x.s[3], 28));
    FpKey k;
    k.f[0] = pick(r0 >> 3, r0 >> 5); k.f[1] = pick(r1 << 1, r1 >> 1); k.f[2] = pick(r2 >> 3, r2 >> 5); k.f[3] = pick(r3 << 1, r3 >> 1);
    // reverse complement = complemented LSB-first halves, swapped
    const uint64_t khi_f = ((uint64_t)k.f[0] << 32) | k.f[1], klo_f = ((uint64_t)k.f[2] << 32) | k.f[3];
    const uint64_t khi_r = ((uint64_t)(~x.s[3] & 0x0FFFFFFFu) << 32) | (uint32_t)~x.s[2], klo_r = ((uint64_t)(~x.s[1] & 0x0FFFFFFFu) << 32) | (uint32_t)~x.s[0];
    k.rc = (khi_r < khi_f) | ((khi_r == khi_f) & (klo_r < klo_f));       // (three compares and two mask operations, no selects)
    k.hi = k.rc ? khi_r : khi_f; k.lo = k.rc ? klo_r : klo_f;
    return k;
}
__device__ inline uint32_t fp_hash(const FpKey& k) {
    const uint32_t fa = (uint32_t)k.hi ^ (uint32_t)(k.lo >> 32), fb = (uint32_t)(k.hi >> 32) ^ (uint32_t)k.lo;
    return (fa + ((fb << 16) | (fb >> 16))) * 0x9E3779B1u;
}
// is the instance (rec, idx) of the tile the same k-mer as (x, k), on either strand?
__device__ inline bool fp_same(const uint32_t* tile, unsigned ref, const FpInst& x, const FpKey& k) {
    const FpInst r = fp_fetch(tile, ref >> 6, ref & 63u);
    const uint32_t same = (r.s[0] ^ x.s[0]) | (r.s[1] ^ x.s[1]) | (r.s[2] ^ x.s[2]) | (r.s[3] ^ x.s[3]);
    // the reference's reverse complement, MSB first, is (~s3, ~s2, ~s1, ~s0): equal to this instance's forward words iff every XOR is all ones
    const uint32_t opp = ((r.s[3] ^ k.f[0]) | 0xF0000000u) & (r.s[2] ^ k.f[1]) & ((r.s[1] ^ k.f[2]) | 0xF0000000u) & (r.s[0] ^ k.f[3]);
    return same == 0u || opp == 0xFFFFFFFFu;
}

// Record dedup: is record `rec` of the tile byte-identical to a record that entered the table before it?  Then that record's copy count
// goes up by one and this one is not flattened.  Equality is decided by the eight dwords, never by the hash.  A table word is
// tag << 10 | record + 1 (0 = free; TILE < 1023), the tag being the bits of the record's hash below those that choose the slot; linear
// probing, and the table is at most half full, so a probe sequence always ends.  A lane reads a holder's record only where the tags are
// equal under `tag_mask10` (the kernel's tag mask << 10: all tag bits in production; 0, a test hook, makes every held slot a tag match --
// the form before the tag); any other held slot costs one XOR / AND / compare.  With the tile at the records' own stride a record is two
// 16-byte LDS reads; the odd stride of -DW2RAP_FP_TS9 keeps dword reads.
template <unsigned DT, unsigned LOG_DT>
__device__ inline bool fp_dedup(const uint32_t* tile, uint32_t* dtab, uint32_t* dmul, unsigned rec, uint32_t tag_mask10) {
    static_assert(REC_DWORDS == 8, "fp_dedup: a record is two 16-byte reads");
    constexpr unsigned TAG_BITS = 32 - LOG_DT < 22 ? 32 - LOG_DT : 22;       // hash bits that the slot index does not use, as far as the word has room
    auto rec_load = [&](unsigned r, uint32_t (&v)[REC_DWORDS]) {
        const uint32_t* p = tile + r * FP_TS;
        if constexpr (FP_TS == REC_DWORDS) {
            const u32x4 lo = *reinterpret_cast<const u32x4*>(p), hi = *reinterpret_cast<const u32x4*>(p + 4);
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) { v[i] = lo[i]; v[4 + i] = hi[i]; }
        } else {
#pragma unroll
            for (unsigned i = 0; i < REC_DWORDS; ++i) v[i] = p[i];
        }
    };
    uint32_t w[REC_DWORDS];
    rec_load(rec, w);
    auto rotl = [](uint32_t v, unsigned n) { return __funnelshift_l(v, v, n); };
    uint32_t x = w[0], y = w[REC_DWORDS - 1];
#pragma unroll
    for (unsigned i = 1; i + 1 < REC_DWORDS; i += 2) { x = rotl(x, 9) + w[i]; y = rotl(y, 13) ^ w[i + 1]; }
    uint32_t h = (x + rotl(y, 16)) * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA6Bu;
    unsigned s = h >> (32 - LOG_DT);
    const uint32_t word = ((h & ((1u << TAG_BITS) - 1u)) << 10) | (rec + 1u);
    for (;;) {
        uint32_t a = ld32(&dtab[s]);
        if (a == 0u) { a = atomicCAS(&dtab[s], 0u, word); if (a == 0u) return false; }
        if (((a ^ word) & tag_mask10) == 0u) {
            const unsigned holder = (a & 1023u) - 1u;
            uint32_t hw[REC_DWORDS];
            rec_load(holder, hw);
            uint32_t d = 0;
#pragma unroll
            for (unsigned i = 0; i < REC_DWORDS; ++i) d |= hw[i] ^ w[i];
            if (d == 0u) { atomicAdd(&dmul[holder >> 1], 1u << (16u * (holder & 1u))); return true; }
        }
        s = (s + 1u) & (DT - 1u);
    }
}

// The kernel's body.  DEDUP: byte-identical records of a bucket are counted once, with their multiplicity as the weight (k_count_fp_dedup);
// false: every record on its own, the form before it (k_count_fp; W2RAP_FP_DEDUP=0 launches it)
#define W2_FP_PARAMS                                                                                                                                  \
    uint32_t nb, uint32_t b_lo, uint32_t b_hi, uint32_t nseg, const uint64_t* __restrict__ roff, const uint32_t* __restrict__ recs, uint32_t min_freq, \
    uint32_t* __restrict__ queue, uint64_t* __restrict__ shi, uint64_t* __restrict__ slo, uint32_t* __restrict__ scc, uint64_t solid_cap,              \
    unsigned long long* __restrict__ counters, unsigned long long* __restrict__ ghist, uint64_t* __restrict__ chunk_start,                            \
    uint32_t* __restrict__ chunk_cnt, uint32_t chunk_cap, uint32_t* __restrict__ defer /* [0] count, [2..] deferred bucket ids */, uint32_t defer_cap, \
    uint32_t fill_limit /* <= LIMIT */, uint32_t solid_limit /* <= SC: smaller values are test hooks */,                                               \
    uint8_t* __restrict__ sctx, uint8_t* __restrict__ unres, uint32_t* __restrict__ nbr /* all three or none: the chunk-local adjacency prune         \
    (k_prune_local's outputs) done here, while the table still holds every distinct k-mer of the bucket with its count */,                            \
    uint32_t dedup_tag_mask /* record dedup: the tag bits that two table words are compared in; all ones, fewer are test hooks (see fp_dedup) */
#define W2_FP_ARGS                                                                                                                                    \
    nb, b_lo, b_hi, nseg, roff, recs, min_freq, queue, shi, slo, scc, solid_cap, counters, ghist, chunk_start, chunk_cnt, chunk_cap, defer, defer_cap, \
    fill_limit, solid_limit, sctx, unres, nbr, dedup_tag_mask
template <unsigned THREADS, unsigned TILE_, unsigned SC_, bool DEDUP>
__device__ __forceinline__ void count_fp_body(W2_FP_PARAMS) {
    constexpr unsigned long long SMASK = (1ull << 40) - 1;
    using C = FpCfg<THREADS, TILE_, SC_>;
    constexpr unsigned CAP = C::CAP, NW = C::NW, TILE = C::TILE, ROUNDS = C::ROUNDS, NPF = C::NPF, SC = C::SC, MAXSEG = C::MAXSEG, PER = C::PER, QCAP = C::QCAP,
                       MAXK = C::MAXK, MAXWIN = C::MAXWIN;
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* segbase = reinterpret_cast<uint64_t*>(smem);         // [3][MAXSEG]
    uint32_t* tab = reinterpret_cast<uint32_t*>(segbase + 3 * MAXSEG);   // [CAP] tag << 16 | record << 6 | index; ~0 = empty
    uint32_t* cc = tab + CAP;                                      // [CAP] count (23:0) | context (31:24)
    uint32_t* tile = cc + CAP;                                     // the bucket's records (+8 dwords of slack)
    uint32_t* bv32 = tile + TILE * FP_TS + 8;                 // [MAXK/32 + 2] record-start bits of the flattened k-mers
    uint32_t* Bw = bv32 + MAXK / 32 + 2;                           // [MAXWIN + 2] record covering the first position of each window
    uint32_t* stcc = Bw + MAXWIN + 2;                              // [SC] count | context of the bucket's solid k-mers, compacted ...
    uint32_t* stref = stcc + SC;                                   // [SC] ... and the instance each of them refers to
    uint32_t* qref = stref + SC + (threadIdx.x >> 6) * QCAP;       // this wave's parked instances
    uint32_t* segdpre = stref + SC + NW * QCAP;                    // [3][MAXSEG + 1]
    uint32_t* wtot = segdpre + 3 * (MAXSEG + 1);                   // [32] per-wave partial sums (flatten: k-mers; emit: occupied and solid slots)
    uint32_t* bq = wtot + 32;                                      // ring of bucket ids
    uint32_t* lhist = bq + 4;                                      // 104
    uint32_t* misc = lhist + 104;                                  // 16
    uint32_t* stk = misc + 16;                                     // (class, P) pairs of a bucket counted in hash classes, depth <= 18
    uint16_t* olist = reinterpret_cast<uint16_t*>(stk + 40);       // [OCAP] the occupied slots of the bucket being emitted
    uint32_t* rinfo = reinterpret_cast<uint32_t*>(olist + C::OCAP); // [TILE] DEDUP: the j-th distinct record of the bucket | its copies << 16
    uint32_t* dtab = stcc;                                         // [DT] DEDUP, S1 .. flatten: hash tag << 10 | record + 1 by content hash (0 = free) ...
    uint32_t* dmul = stcc + C::DT;                                 // [(TILE + 1) / 2] ... and the further copies of each record, 16 bits each
    const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    auto seg_load = [&](uint32_t bb, uint64_t& r0, uint32_t& cnt) {
        r0 = 0; cnt = 0;
        if (tid < nseg && bb < b_hi) {
            const uint64_t at = (uint64_t)tid * (nb & ~SEG_PACKED) + bb;                // (SEG_PACKED: see k_count_buckets)
            uint64_t a = roff[at], len;
            if (nb & SEG_PACKED) { len = a >> SEG_START_BITS; a &= (1ull << SEG_START_BITS) - 1; }
            else len = roff[at + 1] - a;
            r0 = a; cnt = len < (1ull << 20) ? (uint32_t)len : (1u << 20);              // (anything beyond the tile is deferred)
        }
    };
    auto seg_store = [&](unsigned q, uint64_t r0, uint32_t cnt) {       // wave 0 only
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { uint32_t v = __shfl_up(incl, o); if ((int)lane >= o) incl += v; }
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t ex = incl - cnt;
        if (lane < nseg) { segdpre[q * (MAXSEG + 1) + lane] = ex * REC_DWORDS; segbase[q * MAXSEG + lane] = (r0 - ex) * REC_DWORDS; }
        if (lane == 0) segdpre[q * (MAXSEG + 1) + nseg] = tot * REC_DWORDS;
    };
    // dword d of the logical record stream of the bucket in ring slot q (all segments as one stream)
    auto stream_dword = [&](unsigned q, const uint32_t* dp, const uint32_t (&bnd)[7], uint32_t d) -> uint32_t {
        unsigned s = 0;
        if (nseg <= 8) {
#pragma unroll
            for (unsigned i = 0; i < 7; ++i) s += d >= bnd[i] ? 1u : 0u;
        } else while (d >= dp[s + 1]) ++s;
        return recs[segbase[q * MAXSEG + s] + d];
    };
    // the first PFREC records of the bucket in ring slot q -> registers (coalesced dwords of the logical record stream)
    auto tile_load = [&](unsigned q, uint32_t (&v)[NPF]) {
        const uint32_t* dp = segdpre + q * (MAXSEG + 1);
        const uint32_t dall = dp[nseg];
        const uint32_t dend = dall < C::PFREC * REC_DWORDS ? dall : C::PFREC * REC_DWORDS;
        uint32_t bnd[7];
#pragma unroll
        for (unsigned i = 0; i < 7; ++i) bnd[i] = (i + 1 < nseg && nseg <= 8) ? dp[i + 1] : 0xFFFFFFFFu;
        // (16 B per lane and load -- a quarter of the loads and of the segment searches -- was measured in round 4: k_count_fp alone 36.9 -> 36.4 ms,
        //  but 39.6 -> 41.0 ms beside k_table_insert; the step 108.8 -> 110.2 ms.  Dword loads stay.)
#pragma unroll
        for (unsigned j = 0; j < NPF; ++j) {
            const uint32_t d = j * THREADS + tid;
            v[j] = d < dend ? stream_dword(q, dp, bnd, d) : 0u;
        }
    };
    auto tile_store = [&](const uint32_t (&v)[NPF]) {
#pragma unroll
        for (unsigned j = 0; j < NPF; ++j) { const unsigned i = j * THREADS + tid; if (i < C::PFREC * REC_DWORDS) tile[fp_tile_index(i)] = v[j]; }
    };
    // records PFREC .. TILE-1 of a bucket that has them: straight from global memory (its latency is not hidden: one bucket in six at most)
    auto tile_rest = [&](unsigned q) {
        if (TILE <= C::PFREC) return;
        const uint32_t* dp = segdpre + q * (MAXSEG + 1);
        const uint32_t dall = dp[nseg];
        const uint32_t dend = dall < TILE * REC_DWORDS ? dall : TILE * REC_DWORDS;
        uint32_t bnd[7];
#pragma unroll
        for (unsigned i = 0; i < 7; ++i) bnd[i] = (i + 1 < nseg && nseg <= 8) ? dp[i + 1] : 0xFFFFFFFFu;
        for (uint32_t d = C::PFREC * REC_DWORDS + tid; d < dend; d += THREADS) tile[fp_tile_index(d)] = stream_dword(q, dp, bnd, d);
    };
    // context bits of an instance (KMerContext: bits 0..3 successors, 4..7 predecessors; see k_count_buckets), at their place in a count word
    // (bits 31:24).  On the forward strand the left flank b is predecessor bit 4 + b and the right flank successor bit b; on the reverse
    // strand they are successor 3 - b and predecessor 4 + (3 - b): the forward byte with its bits in reverse order, so ONE bit reverse of the
    // word makes it, at bit 24 already.  A k-mer has a predecessor unless it is the record's first (idx 0) without header flag 64, a successor
    // unless it is the last (idx = header bits 5:0) without flag 128: idx <= 63, so both are one compare each
    auto ctx24_of = [&](const FpInst& x, bool rc, uint32_t hdr, unsigned idx) -> uint32_t {
        const bool hasp = ((hdr & 64u) | idx) != 0u, hass = (hdr & 0xBFu) > idx;
        const uint32_t fwd = (hasp ? 16u << (x.e0 & 3u) : 0u) | (hass ? 1u << ((x.e3 >> 26) & 3u) : 0u);
        return rc ? __brev(fwd) : fwd << 24;
    };

    // ---- init
    for (unsigned i = tid; i < CAP; i += THREADS) { tab[i] = EMPTY; cc[i] = 0; }
    for (unsigned i = tid; i < MAXK / 32 + 2; i += THREADS) bv32[i] = 0;
    for (unsigned i = tid; i < TILE * FP_TS + 8; i += THREADS) tile[i] = 0;
    for (unsigned i = tid; i < 104; i += THREADS) lhist[i] = 0;
    if (tid < 16) misc[tid] = 0;
    if (DEDUP) for (unsigned i = tid; i < C::DAREA; i += THREADS) dtab[i] = 0;
    if (tid == 0) {
        const uint32_t t0 = atomicAdd(queue, 3u), nbk = b_hi - b_lo;
        bq[0] = t0 < nbk ? b_lo + t0 : NONE32; bq[1] = t0 + 1 < nbk ? b_lo + t0 + 1 : NONE32; bq[2] = t0 + 2 < nbk ? b_lo + t0 + 2 : NONE32; bq[3] = NONE32;
    }
    __syncthreads();
    if (wv == 0) {
        uint64_t r0; uint32_t cnt;
        seg_load(bq[0], r0, cnt); seg_store(0, r0, cnt);
        seg_load(bq[1], r0, cnt); seg_store(1, r0, cnt);
    }
    __syncthreads();
    uint32_t pf[NPF];
    tile_load(0, pf);
    unsigned long long my_distinct = 0;
    unsigned qn = 0;
    uint32_t tick4 = 0;

    // ---- finish the top `cnt` (<= 64) parked instances of this wave: the full probe sequence; returns the new keys
    auto drain = [&](unsigned cnt) -> unsigned {
        wave_lds_fence();
        const bool live = lane < cnt;
        const uint32_t qv = live ? qref[qn - cnt + lane] : 0u;         // DEDUP: the record's weight rides above the reference
        const unsigned ref = qv & 0xFFFFu, rec = ref >> 6, idx = ref & 63u;
        const FpInst x = fp_fetch(tile, rec, idx);
        const FpKey k = fp_key(x);
        const uint32_t ctx24 = ctx24_of(x, k.rc, tile[rec * FP_TS], idx);
        const uint32_t h1 = fp_hash(k), tag = (h1 >> 5) & 0xFFFFu;
        unsigned s = (h1 >> (33 - C::LOG_CAP)) << 1;                  // the probe sequence starts at an EVEN slot: the window loop looks at a pair
        bool isnew = false;
        if (live) {
            bool ok = false;
            int budget = (int)CAP;
            for (;;) {
                uint32_t a = ld32(&tab[s]);
                if (a == EMPTY) {
                    a = atomicCAS(&tab[s], EMPTY, (tag << 16) | ref);
                    if (a == EMPTY) { isnew = true; ok = true; break; }
                }
                if ((a >> 16) == tag && fp_same(tile, a & 0xFFFFu, x, k)) { ok = true; break; }
                s = (s + 1) & (CAP - 1);
                if (--budget <= 0) break;
            }
            if (ok) { atomicAdd(&cc[s], DEDUP ? qv >> 16 : 1u); atomicOr(&cc[s], ctx24); }
            else st32(&misc[FP_OVF], 1u);
        }
        qn -= cnt;
        wave_lds_fence();
        return (unsigned)__builtin_popcountll(__ballot(isnew));
    };

    for (uint32_t it = 0;; ++it) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&bq[it & 3]));
        if (b >= b_hi) break;
        const unsigned q = it % 3;
        const uint32_t nrec = (uint32_t)__builtin_amdgcn_readfirstlane((int)segdpre[q * (MAXSEG + 1) + nseg]) / REC_DWORDS;
        bool skip = nrec > TILE;                                      // block-uniform
        // ---- stage in this bucket's records; start the look-ahead loads (consumed before barrier A)
        tile_store(pf);
        if (!skip) tile_rest(q);
        uint32_t la_b = 0;
        if (tid == 0) {
            // Tickets FP_TICKETS at a time: an atomic on ONE address costs ~24 ns at its L2 channel whoever waits for it, and ~940 k buckets per
            // step each take a ticket here and an output range below -- 58 % of one channel's atomic unit for the kernel's duration.  Four at a
            // time: k_count_fp 38.9 -> 37.9 ms, the step -0.8 ms (three alternating runs each, profiles/r05_tickets_ab.txt).
            if ((it & (FP_TICKETS - 1u)) == 0) tick4 = atomicAdd(queue, FP_TICKETS);
            const uint32_t t = tick4 + (it & (FP_TICKETS - 1u));
            la_b = t < b_hi - b_lo ? b_lo + t : NONE32;
        }
        uint64_t la_r0 = 0; uint32_t la_cnt = 0;
        if (wv == 0) seg_load(ld32(&bq[(it + 2) & 3]), la_r0, la_cnt);
        tile_load((it + 1) % 3, pf);
        __syncthreads();                                             // S1
        // ---- flatten: record rec occupies positions [e, e + nk) of the bucket-wide k-mer numbering (see k_count_buckets)
        //      DEDUP: a record equal to one met before adds to that one's copies and takes no positions; the scans carry the number of
        //      distinct records above bit 16 (k-mers below: TILE * 64 < 2^16), which numbers them j = 0, 1, .. in record order
        unsigned nkr[ROUNDS], inclr[ROUNDS];
#pragma unroll
        for (unsigned r = 0; r < ROUNDS; ++r) {
            const unsigned rec = r * THREADS + tid;
            bool dup = false;
            if (DEDUP && !skip && r * THREADS + (tid & ~63u) < nrec)             // (wave-uniform: waves without a record pass)
                if (rec < nrec) dup = fp_dedup<C::DT, C::LOG_DT>(tile, dtab, dmul, rec, dedup_tag_mask << 10);
            nkr[r] = (!skip && rec < nrec && !dup) ? (tile[rec * FP_TS] & 63u) + 1u : 0u;
            inclr[r] = wave_scan64(DEDUP ? nkr[r] | (nkr[r] ? 1u << 16 : 0u) : nkr[r]);
            if (lane == 63) wtot[r * NW + wv] = inclr[r];
        }
        if (tid == 0) { misc[FP_WIN] = 2 * NW; stk[0] = 0; stk[1] = 1; misc[FP_DEPTH] = 1; }
        __syncthreads();                                             // X1
        const unsigned wsum = lane < ROUNDS * NW ? wtot[lane] : 0u, wsc = row_scan16(wsum);
        const int wvu = __builtin_amdgcn_readfirstlane((int)wv);
        const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)wsc, ROUNDS * NW - 1) & (DEDUP ? 0xFFFFu : ~0u);
        skip |= total > MAXK;
#pragma unroll
        for (unsigned r = 0; r < ROUNDS; ++r) {
            const unsigned base = (unsigned)__builtin_amdgcn_readlane((int)wsc, r * NW + wvu) - (unsigned)__builtin_amdgcn_readlane((int)wsum, r * NW + wvu);
            if (nkr[r] && !skip) {
                const unsigned pe = base + inclr[r], rec = r * THREADS + tid;
                const unsigned e = (DEDUP ? pe & 0xFFFFu : pe) - nkr[r], j = DEDUP ? (pe >> 16) - 1u : rec;
                atomicOr(&bv32[e >> 5], 1u << (e & 31));
                const unsigned w1 = (e + 63) >> 6;
                if (64 * w1 < e + nkr[r]) Bw[w1] = (j << 16) | e;
                if (DEDUP) rinfo[j] = rec | ((1u + ((dmul[rec >> 1] >> (16u * (rec & 1u))) & 0xFFFFu)) << 16);     // (every copy was added before X1)
            }
        }
        __syncthreads();                                             // X2
        const unsigned nwin = skip ? 0u : (total + 63) / 64;
        bool first_pass = true;
        // A bucket whose distinct set does not fit the table (or whose solid set does not fit the staging area) is counted in hash classes:
        // (class, P) work stack as in k_count_buckets (= MapReduceEngine.h:288-291); the records stay where they are.  Normally one pass.
        for (;;) {
        const unsigned sp = (unsigned)__builtin_amdgcn_readfirstlane((int)ld32(&misc[FP_DEPTH])) - 1u;
        const uint32_t cls = (uint32_t)__builtin_amdgcn_readfirstlane((int)stk[2 * sp]), P = (uint32_t)__builtin_amdgcn_readfirstlane((int)stk[2 * sp + 1]);
        {
            // ---- the windows of this wave (dealt out on demand); straight-line, predicated code as in k_count_buckets
            uint32_t fill_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&misc[FP_FILL])),
                     ovf_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ld32(&misc[FP_OVF]));
            const unsigned wv_s = (unsigned)wvu;
            uint32_t nM0 = 0, nM1 = 0, nB = 0;
            { const unsigned w0 = wv_s < nwin ? wv_s : 0u; nM0 = bv32[2 * w0]; nM1 = bv32[2 * w0 + 1]; nB = Bw[w0]; }
            const uint64_t lane_le = ~0ull >> (63 - lane);
            const uint32_t lane_lt_lo = lane < 32 ? (1u << lane) - 1u : 0xFFFFFFFFu, lane_lt_hi = lane < 32 ? 0u : (1u << (lane - 32)) - 1u;
            unsigned wnext = wv_s + NW;
            for (unsigned w = wv_s; w < nwin;) {
                if (ovf_seen) break;
                if (fill_seen >= fill_limit) { if (lane == 0) st32(&misc[FP_OVF], 1u); break; }
                const uint32_t fill_ld = ld32(&misc[FP_FILL]), ovf_ld = ld32(&misc[FP_OVF]);
                uint32_t wdraw = 0;
                if (lane == 0) wdraw = atomicAdd(&misc[FP_WIN], 1u);
                // ---- A: locate every lane's k-mer (record, index)
                const uint32_t M0 = nM0, M1 = nM1, Bv = nB;
                { const unsigned wn = wnext < nwin ? wnext : w; nM0 = bv32[2 * wn]; nM1 = bv32[2 * wn + 1]; nB = Bw[wn]; }
                const unsigned g = w * 64 + lane;
                const bool active = g < total;
                const uint32_t mle0 = M0 & (uint32_t)lane_le, mle1 = M1 & (uint32_t)(lane_le >> 32);
                const unsigned c = (unsigned)__builtin_popcount(mle0 & ~1u) + (unsigned)__builtin_popcount(mle1);
                const unsigned top = mle1 ? 63u - (unsigned)__builtin_clz(mle1) : 31u - (unsigned)__builtin_clz(mle0 | 1u);
                const unsigned idx = active ? lane - (c ? top : (Bv & 0xFFFFu) - w * 64) : 0u;
                const unsigned rj = active ? (Bv >> 16) + c : 0u;              // the rj-th record that is flattened ...
                const uint32_t inf = DEDUP ? rinfo[rj] : rj;                   // ... is record `rec`, which stands for `inf >> 16` equal ones
                const unsigned rec = inf & 0xFFFFu;
                const uint32_t hdr = tile[rec * FP_TS];
                // ---- B: cut out the k-mer, canonicalise, hash, look at its home slot
                const FpInst x = fp_fetch(tile, rec, idx);
                const FpKey k = fp_key(x);
                const uint32_t ctx24 = ctx24_of(x, k.rc, hdr, idx);
                const uint32_t h1 = fp_hash(k), tag = (h1 >> 5) & 0xFFFFu;
                const unsigned s0 = (h1 >> (33 - C::LOG_CAP)) << 1;
                const unsigned myref = (rec << 6) | idx;
                // ---- C: ONE 8-byte look at the first TWO slots of the k-mer's probe sequence.  A tag match is verified against the instance it
                //      refers to (lanes without one compare with themselves); no match and a free slot among the two -> claim the first free one;
                //      anything else (two other keys there, a lost claim, a tag match that is another k-mer) is parked and finished by drain().
                const uint64_t ab = ld64(reinterpret_cast<const uint64_t*>(tab + s0));
                const uint32_t a0 = (uint32_t)ab, a1 = (uint32_t)(ab >> 32);
                const bool m0 = ((a0 >> 16) == tag) & (a0 != EMPTY), m1 = ((a1 >> 16) == tag) & (a1 != EMPTY);
                const bool second = !m0 & (m1 | ((a0 != EMPTY) & (a1 == EMPTY)));        // act on the second slot: it matches, or it is the first free one
                const uint32_t a = second ? a1 : a0;
                const unsigned s = s0 + (second ? 1u : 0u);
                bool mine = active;
                if (P != 1u) {                                                             // (a bucket counted in hash classes: this pass's class only)
                    asm volatile("; hash-class pass");                                     // P is wave-uniform: a scalar branch, not three predicated VALU instructions
                    mine &= ((h1 >> 2) & (P - 1)) == cls;
                }
                const bool tagm = mine & (m0 | m1);
                const bool hit = tagm & fp_same(tile, tagm ? (a & 0xFFFFu) : myref, x, k);
                const bool want = mine & !tagm & (a == EMPTY);
                const uint32_t old = atomicCAS(&tab[s], EMPTY, want ? ((tag << 16) | myref) : EMPTY);
                const bool won = want & (old == EMPTY);
                const bool done = hit | won;
                atomicAdd(&cc[s], done ? (DEDUP ? inf >> 16 : 1u) : 0u);
                atomicOr(&cc[s], done ? ctx24 : 0u);
                const bool parked = mine & !done;
                unsigned nnew = (unsigned)__builtin_popcountll(__ballot(won));
                {
                    const unsigned long long pm = __ballot(parked);
                    const unsigned below = (unsigned)__builtin_popcount((uint32_t)pm & lane_lt_lo) + (unsigned)__builtin_popcount((uint32_t)(pm >> 32) & lane_lt_hi);
                    const unsigned npark = (unsigned)__builtin_popcountll(pm);
                    // parked lanes take qn .. qn+npark-1, the others the (unused) entries behind them: qn + 63 <= 126 < QCAP
                    qref[qn + (parked ? below : npark + lane - below)] = DEDUP ? myref | (inf & 0xFFFF0000u) : myref;
                    qn += npark;
                    if (qn >= 64) nnew += drain(64);
                }
                if (nnew && lane == 0) atomicAdd(&misc[FP_FILL], nnew);
                fill_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)fill_ld); ovf_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)ovf_ld);
                w = wnext; wnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)wdraw);
            }
            unsigned nnew = 0;
            while (qn) nnew += drain(qn < 64 ? qn : 64);
            if (nnew && lane == 0) atomicAdd(&misc[FP_FILL], nnew);
        }
        // ---- publish the look-ahead results
        if (first_pass) {
            if (wv == 0) seg_store((it + 2) % 3, la_r0, la_cnt);
            if (tid == 0) st32(&bq[(it + 3) & 3], la_b);
            first_pass = false;
        }
        if (tid == 0) {
            misc[FP_CNT] = 0;
            if (skip) misc[FP_OVF] = 1;
        }
        __syncthreads();                                             // A: all inserts done
        bool deferred = ld32(&misc[FP_OVF]) != 0;
        // ---- emit, pass 0: every thread looks at PER neighbouring slots (16-byte LDS reads): which are occupied, how many are solid
        static_assert(PER % 4 == 0, "PER");
        uint32_t occm = 0, nsol = 0;
        if (!deferred) {
            const u32x4* c4 = reinterpret_cast<const u32x4*>(cc + tid * PER);
#pragma unroll
            for (unsigned j4 = 0; j4 < PER / 4; ++j4) {
                const u32x4 v4 = c4[j4];
#pragma unroll
                for (unsigned j = 0; j < 4; ++j) {
                    const uint32_t cnt = v4[j] & 0xFFFFFFu;
                    occm |= (cnt != 0 ? 1u : 0u) << (4 * j4 + j);
                    nsol += (cnt != 0 && cnt >= min_freq) ? 1u : 0u;
                }
            }
        }
        const unsigned nocc = (unsigned)__builtin_popcount(occm);
        const unsigned i_occ = wave_scan64(nocc), i_sol = wave_scan64(nsol);
        if (lane == 63) { wtot[wv] = i_occ; wtot[16 + wv] = i_sol; }
        __syncthreads();                                             // P0
        const unsigned ws_o = lane < NW ? wtot[lane] : 0u, wc_o = row_scan16(ws_o), ws_s = lane < NW ? wtot[16 + lane] : 0u, wc_s = row_scan16(ws_s);
        const unsigned tot_occ = (unsigned)__builtin_amdgcn_readlane((int)wc_o, NW - 1), tot = (unsigned)__builtin_amdgcn_readlane((int)wc_s, NW - 1);
        deferred |= tot > solid_limit;                               // (nothing has been written yet)
        if (deferred) {
            // the table or the staging area is too small for this class: refine it and count again; a bucket that is not this kernel's shape
            // at all (more records than the tile, more k-mers than the start bits) goes to the list kernel, which counts it from scratch
            for (unsigned i = tid; i < CAP; i += THREADS) { tab[i] = EMPTY; cc[i] = 0; }
            if (tid == 0) {
                if (skip) {
                    const uint32_t at = atomicAdd(&defer[0], 1u);
                    if (at < defer_cap) defer[2 + at] = b; else counters[3] = 3;
                    misc[FP_DEPTH] = sp;
                } else if (P >= (1u << 16)) { counters[3] = 1; misc[FP_DEPTH] = sp; }
                else { atomicAdd(&counters[2], 1ull); stk[2 * sp] = cls + P; stk[2 * sp + 1] = 2 * P; stk[2 * sp + 2] = cls; stk[2 * sp + 3] = 2 * P; misc[FP_DEPTH] = sp + 2; }
                misc[FP_FILL] = 0; misc[FP_OVF] = 0; misc[FP_WIN] = 2 * NW;
            }
            __syncthreads();
            if (ld32(&misc[FP_DEPTH]) == 0) break;
            continue;
        }
        {
            unsigned at = (unsigned)__builtin_amdgcn_readlane((int)wc_o, wvu) - (unsigned)__builtin_amdgcn_readlane((int)ws_o, wvu) + i_occ - nocc;
            for (uint32_t m = occm; m; m &= m - 1) olist[at++] = (uint16_t)(tid * PER + (unsigned)__builtin_ctz(m));
        }
        if (tid == 0) {
            // the bucket's output range and chunk number: ONE global atomic (count in bits 39:0, chunks above); its result is needed behind
            // barrier B2 only -- this lane waits for it there while the block runs pass 1, and the CU's other block does not wait at all
            misc[FP_FILL] = 0; misc[FP_DEPTH] = sp; misc[FP_WIN] = 2 * NW;
            const unsigned long long pk = tot ? atomicAdd(&counters[0], (1ull << 40) | tot) : 0ull;
            misc[FP_BASELO] = (uint32_t)pk; misc[FP_BASEHI] = (uint32_t)(pk >> 32);
            if (tot && chunk_start && (pk >> 40) < chunk_cap) { chunk_start[pk >> 40] = pk & SMASK; chunk_cnt[pk >> 40] = tot; }
        }
        __syncthreads();                                             // P1: the list of occupied slots is complete
        // ---- pass 1, dense over the occupied slots: histogram over ALL distinct k-mers (:1097), reset; the solid ones (:1098-1100) go to the
        //      staging area -- as references first, as keys after one dense extraction round
        for (unsigned i0 = 0; i0 < tot_occ; i0 += THREADS) {
            const unsigned i = i0 + tid;
            const bool live = i < tot_occ;
            const unsigned slot = live ? olist[i] : 0u;
            const uint32_t v = cc[slot];
            uint32_t cnt = v & 0xFFFFFFu; if (cnt > 255) cnt = 255;                  // :943-949 saturating u8
            const unsigned long long m1 = __ballot(live && cnt == 1);                  // singletons (sequencing errors) dominate
            if (m1 && lane == (unsigned)__builtin_ctzll(m1)) atomicAdd(&lhist[1], (uint32_t)__builtin_popcountll(m1));
            if (live && cnt != 1) atomicAdd(&lhist[cnt > 100 ? 100 : cnt], 1u);
            if (live) ++my_distinct;
            const bool solid = live && cnt >= min_freq;
            const unsigned long long sb = __ballot(solid);
            if (sb) {
                uint32_t base = 0;
                if (lane == (unsigned)__builtin_ctzll(sb)) base = atomicAdd(&misc[FP_CNT], (uint32_t)__builtin_popcountll(sb));
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(sb));
                if (solid) {
                    const unsigned pos = base + (unsigned)__builtin_popcountll(sb & ((1ull << lane) - 1));
                    stref[pos] = tab[slot] & 0xFFFFu; stcc[pos] = cnt | ((v >> 24) << 8);
                    if (sctx) cc[slot] = 0x80000000u | pos;                             // (fused prune: a solid k-mer's slot names its place in the chunk ...
                }
            }
            if (live && sctx && !solid) cc[slot] = 0x40000000u;                         //  ... any other occupied slot says "not solid"; the table is reset behind the probes)
            if (live && !sctx) { cc[slot] = 0; tab[slot] = EMPTY; }
        }
        __syncthreads();                                             // B2: the references are in place, the output range is known
        {   // the keys of the solid k-mers, one dense extraction round, straight to their places (coalesced 8-B / 4-B stores)
            const unsigned long long gb = ((unsigned long long)misc[FP_BASELO] | ((unsigned long long)misc[FP_BASEHI] << 32)) & SMASK;
            for (unsigned i0 = 0; i0 < tot; i0 += THREADS) {
                const unsigned i = i0 + tid;
                const bool have = i < tot;
                const uint32_t ref = have ? stref[i] : 0u;
                const FpKey k = fp_key(fp_fetch(tile, ref >> 6, ref & 63u));
                const uint32_t ccv = have ? stcc[i] : 0u;
                if (have && gb + i < solid_cap) { shi[gb + i] = k.hi; slo[gb + i] = k.lo; scc[gb + i] = ccv; }
                if (sctx) {
                    // KmerDict::recomputeAdjacencies (ReadPather.h:317-346) as far as this bucket can tell: a neighbour k-mer shares the minimizer
                    // with probability 45/47 and then lies in THIS table with its whole count -- solid: the bit stays and the neighbour's node id
                    // is kept for the unipath links; present but not solid: the bit goes; absent: the bit stays open for k_prune's global probe
                    constexpr uint32_t NONE = 0xFFFFFFFFu, PAL = 0xFFFFFFFEu;
                    unsigned c = (ccv >> 8) & 0xFFu, un = 0;
                    uint32_t ns = NONE, np_ = NONE;
                    const Kmer kk{k.hi, k.lo};
                    for (unsigned rest = have ? c : 0u; __any(rest != 0);) {
                        if (rest) {
                            const unsigned t = (unsigned)__builtin_ctz(rest);
                            rest &= rest - 1;
                            Kmer nk = t < 4 ? kmer_succ(kk, t & 3) : kmer_pred(kk, t & 3);
                            const bool r = kmer_canon(nk);
                            FpInst nx; FpKey nkk;
                            const uint64_t lh = rev2_64(nk.hi) >> 4, ll = rev2_64(nk.lo) >> 4;     // LSB-first halves (base 0 at bits 1:0)
                            nx.s[0] = (uint32_t)lh; nx.s[1] = (uint32_t)(lh >> 32); nx.s[2] = (uint32_t)ll; nx.s[3] = (uint32_t)(ll >> 32); nx.e0 = 0; nx.e3 = 0;
                            nkk.hi = nk.hi; nkk.lo = nk.lo; nkk.rc = false;
                            nkk.f[0] = (uint32_t)(nk.hi >> 32); nkk.f[1] = (uint32_t)nk.hi; nkk.f[2] = (uint32_t)(nk.lo >> 32); nkk.f[3] = (uint32_t)nk.lo;
                            const uint32_t h1 = fp_hash(nkk), tag = (h1 >> 5) & 0xFFFFu;
                            unsigned s = (h1 >> (33 - C::LOG_CAP)) << 1;
                            int found = -1;
                            for (int budget = (int)CAP; budget > 0; --budget) {
                                const uint32_t a = tab[s];
                                if (a == EMPTY) break;
                                if ((a >> 16) == tag && fp_same(tile, a & 0xFFFFu, nx, nkk)) { found = (int)s; break; }
                                s = (s + 1) & (CAP - 1);
                            }
                            if (found < 0) un |= 1u << t;
                            else {
                                const uint32_t v = cc[found];
                                if (v & 0x80000000u) {
                                    const uint32_t id = kmer_is_pal(nk) ? PAL : (uint32_t)(2 * (gb + (v & 0xFFFFu)) + (r ? 1u : 0u));
                                    if (t < 4) ns = id; else np_ = id;
                                } else c &= ~(1u << t);
                            }
                        }
                    }
                    if (have && gb + i < solid_cap) {
                        const unsigned long long gi = gb + i;
                        sctx[gi] = (uint8_t)c; unres[gi] = (uint8_t)un;
                        // only meaningful when exactly one successor / predecessor survives (then it is the last one found): as k_prune_local
                        nbr[2 * gi] = (!(un & 15u) && popc4(c & 15) != 1) ? NONE : ns;
                        nbr[2 * gi + 1] = (!(un >> 4) && popc4(c >> 4) != 1) ? NONE : np_;
                    }
                }
            }
        }
        __syncthreads();                                             // C: the tile is free for the next bucket (or the next class starts)
        if (sctx) {                                                  // fused prune: the table was kept for the probes; reset it now
            for (unsigned i = tid; i < tot_occ; i += THREADS) { const unsigned slot = olist[i]; cc[slot] = 0; tab[slot] = EMPTY; }
            if (sp != 0) __syncthreads();                            // (the next class starts at once; the next bucket has barriers of its own)
        }
        if (sp == 0) break;
        }
        for (unsigned i = tid; i < 2 * nwin + 2; i += THREADS) bv32[i] = 0;            // the next bucket's start bits (behind its barriers S1 and X1)
        // the next bucket's record table and copy counts: the emit wrote over them, and its last reads of stcc / stref lie before barrier C
        if (DEDUP) for (unsigned i = tid; i < C::DAREA; i += THREADS) dtab[i] = 0;
    }
    // ---- histogram, distinct count
    __syncthreads();
    for (unsigned i = tid; i < 101; i += THREADS) if (lhist[i]) atomicAdd(&ghist[i], (unsigned long long)lhist[i]);
    for (int o = 32; o > 0; o >>= 1) my_distinct += __shfl_down(my_distinct, o);
    if (lane == 0 && my_distinct) atomicAdd(&counters[1], my_distinct);
}
template <unsigned THREADS, unsigned MINW, unsigned TILE_, unsigned SC_>
__global__ void __launch_bounds__(THREADS, MINW) k_count_fp(W2_FP_PARAMS) { count_fp_body<THREADS, TILE_, SC_, false>(W2_FP_ARGS); }
// k_count_fp with the record dedup stage behind barrier S1 (fp_dedup: a table of tagged record ids, a record read as two 16-byte words, the
// eight-dword compare only where the tags are equal) in front of the same window loop, whose lanes then stand for `copies` equal records.
// The window loop, per window of 64 k-mers and wavefront, is 176 VALU / 70 SALU / 19 LDS instructions in the ISA of <512, 4, 512, 1024> while
// no bucket is counted in hash classes (NOTES.md section 20: the class test behind a scalar branch, the reversal in fp_key, the context bits
// by one bit reverse, the strand compare without selects).
// The dedup stage must not take the kernel past 120 VGPRs: a wavefront is given registers in steps of 8, and k_table_insert finds room beside
// two resident 512-thread blocks of this kernel only while 4 x its allocation stays below the SIMD's 512 (round 4: at 128 it ran in the gaps,
// 16 -> 33 ms).  Left alone the scheduler uses whatever occupancy 4 allows (124); the body needs 116.  (The attribute counts registers in
// halves of the unified file: 60 = 120 VGPRs.  The 1024-thread shape with eight waves per SIMD keeps its bound of 64.)  As it stands:
// 120 VGPRs, nothing spilled, no scratch; k_count_fp 117 / 0 / 0.
template <unsigned THREADS, unsigned MINW, unsigned TILE_, unsigned SC_>
__global__ void __attribute__((amdgpu_num_vgpr(60))) __launch_bounds__(THREADS, MINW) k_count_fp_dedup(W2_FP_PARAMS) { count_fp_body<THREADS, TILE_, SC_, true>(W2_FP_ARGS); }
#undef W2_FP_PARAMS
#undef W2_FP_ARGS

// =============================================================================== K4
__global__ void __launch_bounds__(256) k_table_insert(uint64_t i0, uint64_t S, const uint64_t* __restrict__ shi, const uint64_t* __restrict__ slo,
                                                       Slot* __restrict__ table, uint64_t mask) {
    uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const uint64_t h = kmer_hash(Kmer{shi[i], slo[i]});
    const Slot v = slot_make(h, i);                                  // fingerprint | index: the whole entry is the claim
    uint64_t s = h & mask;
    while (atomicCAS(&table[s], SLOT_EMPTY, v) != SLOT_EMPTY) s = (s + 1) & mask;
}

// =============================================================================== K5
// KmerDict::recomputeAdjacencies (ReadPather.h:317-346): clear every context bit whose
// neighbour k-mer is not in the solid set.  Membership only, so it is order-free.
//
// Two steps.  k_prune_local works on one K3 emit chunk (the solid k-mers of one minimizer bucket) at a time: their keys
// go into an LDS hash table and every neighbour is looked for THERE first -- consecutive k-mers share their minimizer
// with probability ~45/47, so most surviving neighbours are found without touching HBM.  A bit whose neighbour is not in
// the chunk (another bucket, or not solid at all) stays set and is recorded in unres[i]; k_prune then probes the global
// table for exactly those bits.  Without chunks (multi-GPU: the gathered dictionary is renumbered) k_prune does it all.
// A chunk holds the solid k-mers of one bucket: ~4500 k-mer INSTANCES' worth, i.e. ~250 k-mers at 30x coverage, ~420 at 17x (the per-GPU share of
// BASELINE configs[4]), more below that.  A thread takes U of them (U = 2, 4, 8: chunks of up to 512, 1024, 2048 k-mers in a table of twice
// as many slots); the launcher picks U from the mean chunk size (PL_LAUNCH).  An oversized chunk is still exact -- its bits stay open for the
// global step -- but at U = 2 a 17x data set left a third of its chunks to it: 0.87 routed queries per k-mer instead of 0.26 in the sharded phase.
template <unsigned U> struct PlCfg { static constexpr unsigned CAP = 256 * U, SLOTS = 512 * U, BITS = U == 2 ? 10 : U == 4 ? 11 : 12; };
template <unsigned BITS>
__device__ inline unsigned pl_hash(Kmer k) {
    const uint32_t fa = (uint32_t)k.hi ^ (uint32_t)(k.lo >> 32), fb = (uint32_t)(k.hi >> 32) ^ (uint32_t)k.lo;
    return ((fa + ((fb << 16) | (fb >> 16))) * 0x9E3779B1u) >> (32 - BITS);
}
template <class Id, unsigned U = 2>
__global__ void __launch_bounds__(256) k_prune_local(uint64_t nchunks, const uint64_t* __restrict__ cstart, const uint32_t* __restrict__ ccnt,
                                                      const uint64_t* __restrict__ shi, const uint64_t* __restrict__ slo,
                                                      const uint32_t* __restrict__ scc, uint8_t* __restrict__ sctx,
                                                      Id* __restrict__ nbr, uint8_t* __restrict__ unres) {
    constexpr Id NONE = NodeId<Id>::NONE, PAL = NodeId<Id>::PAL;
    constexpr unsigned PL_CAP = PlCfg<U>::CAP, PL_SLOTS = PlCfg<U>::SLOTS, PL_BITS = PlCfg<U>::BITS;
    __shared__ uint64_t khi[PL_SLOTS], klo[PL_SLOTS];
    __shared__ uint16_t kix[PL_SLOTS];
    const unsigned tid = threadIdx.x;
    // software pipeline over this block's chunks: the descriptor of the chunk after next and the keys of the next chunk are
    // loaded while the current one is worked on in LDS
    auto load_desc = [&](uint64_t ch, uint64_t& st_, uint32_t& cn_) {
        st_ = 0; cn_ = 0;
        if (ch < nchunks) { st_ = cstart[ch]; cn_ = ccnt[ch]; if (cn_ > PL_CAP) cn_ = 0; }   // oversized chunk: its k-mers stay fully unresolved
    };
    auto load_keys = [&](uint64_t st_, uint32_t cn_, Kmer (&k_)[U], unsigned (&c_)[U]) {
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const unsigned j = tid + 256 * u;
            k_[u] = Kmer{0, 0}; c_[u] = 0;
            if (j < cn_) { k_[u] = Kmer{shi[st_ + j], slo[st_ + j]}; c_[u] = (scc[st_ + j] >> 8) & 0xFF; }
        }
    };
    uint64_t st_c, st_n; uint32_t cn_c, cn_n;
    Kmer nx[U]; unsigned ncx[U];
    load_desc(blockIdx.x, st_c, cn_c);
    load_keys(st_c, cn_c, nx, ncx);
    load_desc((uint64_t)blockIdx.x + gridDim.x, st_n, cn_n);
    for (uint64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const uint64_t start = st_c;
        const uint32_t cnt = cn_c;
        Kmer mine[U]; unsigned cm[U];
#pragma unroll
        for (unsigned u = 0; u < U; ++u) { mine[u] = nx[u]; cm[u] = ncx[u]; }
        st_c = st_n; cn_c = cn_n;
        load_keys(st_c, cn_c, nx, ncx);                           // next chunk's keys
        load_desc(ch + 2 * (uint64_t)gridDim.x, st_n, cn_n);      // the one after's descriptor
        if (cnt == 0) continue;
        __syncthreads();
        for (unsigned s = tid; s < PL_SLOTS; s += 256) khi[s] = EMPTY_HI;
        __syncthreads();
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            const unsigned j = tid + 256 * u;
            if (j < cnt) {
                unsigned s = pl_hash<PL_BITS>(mine[u]);
                for (;;) {                                        // the keys of a chunk are distinct
                    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&khi[s]), (unsigned long long)EMPTY_HI,
                                                             (unsigned long long)mine[u].hi);
                    if (old == EMPTY_HI) { klo[s] = mine[u].lo; kix[s] = (uint16_t)j; break; }
                    s = (s + 1) & (PL_SLOTS - 1);
                }
            }
        }
        __syncthreads();
        auto find = [&](Kmer nk) -> int {
            unsigned s = pl_hash<PL_BITS>(nk);
            for (;;) {
                const uint64_t h = khi[s];
                if (h == EMPTY_HI) return -1;
                if (h == nk.hi && klo[s] == nk.lo) return (int)kix[s];
                s = (s + 1) & (PL_SLOTS - 1);
            }
        };
#pragma unroll
        for (unsigned u = 0; u < U; ++u) {
            if (256 * u + (tid & ~63u) >= cnt) continue;          // this wavefront has no k-mer in this part of the chunk (wave-uniform)
            const unsigned j = tid + 256 * u;
            const Kmer k = mine[u];
            const unsigned c = j < cnt ? cm[u] : 0;
            unsigned un = 0;
            Id ns = NONE, np = NONE;
            // The reverse complement of a neighbour is a neighbour of the reverse complement: rc(k + b) = (3-b) + rc(k) without its last base,
            // rc(b + k) = rc(k) without its first base + (3-b).  One 120-bit reversal per k-mer instead of two per context bit.
            const Kmer rk = kmer_rc(k);
            // one set bit per trip (3-4 trips for a wave instead of eight branches): bits 0..3 successors, 4..7 predecessors
            for (unsigned rest = c; __any(rest != 0);) {
                if (rest) {
                    const unsigned t = (unsigned)__builtin_ctz(rest);
                    rest &= rest - 1;
                    const unsigned b = t & 3;
                    const Kmer fw = t < 4 ? kmer_succ(k, b) : kmer_pred(k, b);
                    const Kmer rv = t < 4 ? kmer_pred(rk, 3u - b) : kmer_succ(rk, 3u - b);
                    const bool r = kmer_lt(rv, fw);                          // kmer_canon: the reverse complement only if it is smaller
                    const Kmer nk = r ? rv : fw;
                    const int f = find(nk);
                    if (f < 0) un |= 1u << t;
                    else {
                        const Id id = kmer_eq(rv, fw) ? PAL : (Id)(2 * (start + (unsigned)f) + (r ? 1u : 0u));
                        if (t < 4) ns = id; else np = id;
                    }
                }
            }
            if (j < cnt) {
                const uint64_t i = start + j;
                sctx[i] = (uint8_t)c; unres[i] = (uint8_t)un;
                // only meaningful when exactly one successor / predecessor survives (then it is the last one found)
                nbr[2 * i] = (!(un & 15u) && popc4(c & 15) != 1) ? NONE : ns;
                nbr[2 * i + 1] = (!(un >> 4) && popc4(c >> 4) != 1) ? NONE : np;
            }
        }
    }
}
// the launcher: k-mers per thread from the mean chunk size (W2RAP_PL_U forces 2, 4 or 8: the parity tests run all three)
#define PL_LAUNCH(c, IdT, gl, S_, nch_, ...)                                                                                          \
    do {                                                                                                                              \
        unsigned u__ = (nch_) ? ((S_) / (nch_) > 600 ? 8u : (S_) / (nch_) > 300 ? 4u : 2u) : 2u;                                       \
        if (const char* v__ = getenv("W2RAP_PL_U")) { const int x__ = atoi(v__); if (x__ == 2 || x__ == 4 || x__ == 8) u__ = (unsigned)x__; }  \
        if (u__ == 8) LAUNCH(c, "k_prune_local", (k_prune_local<IdT, 8>), dim3(gl), dim3(256), 0, nch_, __VA_ARGS__);                  \
        else if (u__ == 4) LAUNCH(c, "k_prune_local", (k_prune_local<IdT, 4>), dim3(gl), dim3(256), 0, nch_, __VA_ARGS__);             \
        else LAUNCH(c, "k_prune_local", (k_prune_local<IdT, 2>), dim3(gl), dim3(256), 0, nch_, __VA_ARGS__);                           \
    } while (0)
// the global step: every context bit recorded in unres[i] (all set bits when unres == nullptr) is looked up in the table
template <class Id>
__global__ void __launch_bounds__(256) k_prune(uint64_t i0, uint64_t S /* k-mers [i0, S) */, const uint64_t* __restrict__ shi, const uint64_t* __restrict__ slo,
                                                const uint32_t* __restrict__ scc, const Slot* __restrict__ table, uint64_t mask,
                                                uint8_t* __restrict__ sctx, Id* __restrict__ nbr, const uint8_t* __restrict__ unres) {
    constexpr Id NONE = NodeId<Id>::NONE, PAL = NodeId<Id>::PAL;
    uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    unsigned c, todo;
    // the neighbour found for each context bit is remembered (oriented node id 2*idx + reversed) so that the
    // unipath linking step does not have to probe the dictionary again
    Id ns = NONE, np = NONE;
    if (unres) {
        todo = unres[i];
        if (!todo) return;                                        // settled by k_prune_local
        if (todo == 0xFFu && sctx[i] == 0xFFu) { c = (scc[i] >> 8) & 0xFF; todo = c; }        // never visited (oversized chunk)
        else { c = sctx[i]; ns = nbr[2 * i]; np = nbr[2 * i + 1]; }
    } else { c = (scc[i] >> 8) & 0xFF; todo = c; }
    const Kmer k{shi[i], slo[i]}, rk = kmer_rc(k);                // (the reverse complement of a neighbour is a neighbour of rk: see k_prune_local)
    // one open bit per trip: a wave makes as many dependent table probes as its busiest lane has open bits (2-3), not eight
    for (unsigned rest = todo; rest;) {
        const unsigned t = (unsigned)__builtin_ctz(rest);
        rest &= rest - 1;
        const unsigned b = t & 3;
        const Kmer fw = t < 4 ? kmer_succ(k, b) : kmer_pred(k, b);
        const Kmer rv = t < 4 ? kmer_pred(rk, 3u - b) : kmer_succ(rk, 3u - b);
        const bool r = kmer_lt(rv, fw);
        const Kmer nk = r ? rv : fw;
        const int64_t s = table_find(table, mask, shi, slo, nk);
        if (s < 0) c &= ~(1u << t);
        else {
            const Id id = kmer_eq(rv, fw) ? PAL : (Id)(2 * (uint64_t)s + (r ? 1u : 0u));
            if (t < 4) ns = id; else np = id;
        }
    }
    sctx[i] = (uint8_t)c;
    // only meaningful when exactly one successor / predecessor survives (then it is the last one found)
    nbr[2 * i] = popc4(c & 15) == 1 ? ns : NONE;
    nbr[2 * i + 1] = popc4(c >> 4) == 1 ? np : NONE;
}

// =============================================================================== driver
static constexpr unsigned COUNT_CAP = 4096, COUNT_THREADS = 1024;
static constexpr unsigned KMERS_PER_BUCKET = 4500;      // (round 4: 5000 -> 4500 with k_count_fp: fewer buckets beyond its resident tile; 4000 .. 5500 are within 1 %)

// ---- K0: quality windows; sets c.M (k-mer instances of this rank's reads) and c.max_len
int count_quality(Ctx& c, uint32_t min_qual) {
    c.min_qual = min_qual;
    c.counted = false;
    hipStream_t st = c.stream;
    const uint64_t n = c.n;
    if (c.d_good) c.release(c.d_good);
    W2_ALLOC(c.d_good, uint16_t, n);
    unsigned long long* d_cnt = nullptr;                 // [0..QSLOTS) partial M  [QSLOTS..) partial max_len (as u32)
    W2_ALLOC(d_cnt, unsigned long long, 2 * QSLOTS);
    W2_HIP(hipMemsetAsync(d_cnt, 0, 2 * QSLOTS * sizeof(unsigned long long), st));
    const bool masked = c.d_qmask && c.qmask_min_qual == (int)std::min<uint32_t>(min_qual, 255u);
    if (!masked && c.quals_absent) { c.err = "quality windows: the reads were installed by a graph-only call for another min_qual, their raw qualities were not uploaded"; return W2RAP_E_STATE; }
    if (!masked) W2_TRY(quals_wait(c));                  // (another threshold than the mask was made for: the raw qualities, once they are up)
    if (n) {
        if (masked) LAUNCH(c, "k_good_len", k_good_len<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, n, c.d_quals, c.d_qmask, c.d_qoff, c.d_len, min_qual,
                           c.d_good, d_cnt, reinterpret_cast<uint32_t*>(d_cnt + QSLOTS));
        else LAUNCH(c, "k_good_len", k_good_len<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, n, c.d_quals, (const uint32_t*)nullptr, c.d_qoff, c.d_len, min_qual,
                    c.d_good, d_cnt, reinterpret_cast<uint32_t*>(d_cnt + QSLOTS));
        W2_HIP(hipGetLastError());
    }
    unsigned long long h_cnt[2 * QSLOTS];
    W2_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    W2_HIP(hipStreamSynchronize(st));
    c.M = 0; c.max_len = 0;
    for (unsigned i = 0; i < QSLOTS; ++i) {
        c.M += h_cnt[i];
        const uint32_t* mx = reinterpret_cast<const uint32_t*>(h_cnt + QSLOTS);
        c.max_len = std::max(c.max_len, mx[i]);
    }
    c.release(d_cnt);
    // (device arrays are not swept on the host: the longest read shows here; its good length would not fit the 16-bit words written above)
    if (c.max_len > 65535u) { c.err = "a read of more than 65,535 bases: good lengths are 16-bit words"; return W2RAP_E_LIMIT; }
    c.quality_done = true;
    return 0;
}

uint32_t default_buckets(uint64_t total_kmers, uint32_t multiple_of) {
    const char* v = getenv("W2RAP_KPB");               // tuning knob: k-mers per bucket
    uint64_t kpb = v ? (uint64_t)atoll(v) : KMERS_PER_BUCKET;
    uint64_t nb64 = total_kmers / kpb + 1;
    if (nb64 > (1u << 24)) nb64 = 1u << 24;
    if (multiple_of > 1) nb64 = (nb64 + multiple_of - 1) / multiple_of * multiple_of;
    return (uint32_t)nb64;
}

// ---- K3: count `nbl` buckets whose records arrive in `nseg` segments (one per source rank), each
// segment grouped by bucket; d_counts[s*nbl + b] = records of bucket b in segment s, d_recs = the
// segments back to back.  total_kmers bounds the solid set (S <= kmers / min_freq).
// lookup-table geometry for S solid k-mers: 4 slots per k-mer (load <= 0.25: ~1.3 probes per miss instead of ~2.3)
static void table_geometry(uint64_t S, uint64_t& tcap) {
    const char* lf = getenv("W2RAP_TABLE_X");
    // beyond 2^30 k-mers the table is kept at 1.3 slots per k-mer at least (a power of two: load 0.38 .. 0.77) -- at 2.5 G solid
    // k-mers (BASELINE configs[2] replicated, capacity estimate + 15 %) that is 34 GB instead of 137
    const uint64_t mult10 = lf ? 10 * (uint64_t)atoll(lf) : (S < (1ull << 30) ? 40 : 13);
    tcap = 1024;
    while (10 * tcap < mult10 * S) tcap <<= 1;
    // (there is no per-k-mer absence filter in front of it any more -- a second atomic per k-mer in K4: read pathing proves
    // absence through the 31-mer filter built with the graph, step2_graph.hip k_filter32)
}

// The buckets are counted in NS launches (slices of the bucket range); after each one the running totals (solid k-mers,
// chunks) are copied to pinned memory and an event is recorded, so that a caller can consume slice k -- insert its solid
// k-mers into the lookup table on the side stream (single GPU), or exchange them with the other ranks (multi-GPU) -- while
// slice k+1 is being counted: the insert kernel is bound by device atomics and leaves the SIMDs idle, the counting kernel is
// bound by instruction issue and leaves the memory system idle.
int count_buckets_launch(Ctx& c, uint32_t min_freq, uint32_t nbl, uint32_t nseg, const uint32_t* d_recs, const uint32_t* d_counts,
                         uint64_t total_kmers, unsigned NS, bool deferred) {
    hipStream_t st = c.stream;
    if (c.cs_planned) { c.err = "count_records_begin: a sliced count is already pending"; return W2RAP_E_STATE; }
    c.min_freq = min_freq;
    if (!c.pass) c.table_built = false;                  // (a later pass goes on filling the owner's own dictionary of the earlier ones: local_dict_slice)
    if (NS < 1) NS = 1; if (NS > 16) NS = 16;
    if (nbl < 4096) NS = 1;
    if (nseg > 64) { c.err = "count_records: more than 64 segments"; return W2RAP_E_LIMIT; }
    const uint64_t nflat = (uint64_t)nbl * nseg;
    uint64_t* d_off = nullptr;
    W2_ALLOC(d_off, uint64_t, nflat + 1);
    c.cs_packed = c.slab_cap != 0;
    if (c.cs_packed) {                                   // bucket slabs + overflow segment: (start | count) words, count_partition_slabs
        if (nseg != 2 || d_counts != c.d_bcount || !c.d_bbase) { c.err = "count_records: the slab layout has two segments"; return W2RAP_E_STATE; }
        W2_TRY(slab_segments(c, nbl, d_counts, d_off));
    } else
    W2_TRY(exclusive_scan_u32_to_u64(c, d_counts, d_off, nflat));
    // A later pass of a multi-pass count (c.pass > 0) appends to the solid arrays, the chunk list, the counters and the histogram of
    // the passes before it; everything else is this pass's own.
    unsigned long long* d_cnt = c.pass ? c.pass_cnt : nullptr;   // [4..7] counters  [8..108] hist  [144] queue (a line of its own)
    uint32_t chunk_cap = c.pass ? c.cs_chunk_cap : 0;
    if (!c.pass) {
        W2_ALLOC(d_cnt, unsigned long long, 160);
        W2_HIP(hipMemsetAsync(d_cnt, 0, 160 * sizeof(unsigned long long), st));
        c.solid_cap = total_kmers / (min_freq ? min_freq : 1) + 1;
        for (void* p : {(void*)c.d_shi, (void*)c.d_slo, (void*)c.d_scc}) if (p) c.release(p);
        W2_ALLOC(c.d_shi, uint64_t, c.solid_cap);
        W2_ALLOC(c.d_slo, uint64_t, c.solid_cap);
        W2_ALLOC(c.d_scc, uint32_t, c.solid_cap);
        // chunk list for the bucket-local prune and the chunk-local list ranking (multi-GPU: exchanged with the solid k-mers)
        if (c.d_chunk_start) { c.release(c.d_chunk_start); c.release(c.d_chunk_cnt); c.d_chunk_start = nullptr; c.d_chunk_cnt = nullptr; }
        c.nchunks = 0;
        if (!getenv("W2RAP_NO_LOCAL_PRUNE")) {
            const uint64_t nb_all = c.npass > 1 ? c.NB : nbl;                      // all passes share the list
            chunk_cap = (uint32_t)std::min<uint64_t>(nb_all * 2 + 4096, 1u << 24);
            W2_ALLOC(c.d_chunk_start, uint64_t, chunk_cap);
            W2_ALLOC(c.d_chunk_cnt, uint32_t, chunk_cap);
            W2_HIP(hipMemsetAsync(c.d_chunk_cnt, 0, (size_t)chunk_cap * 4, st));
        }
    }
    c.cs_cnt = d_cnt; c.cs_off = d_off; c.cs_chunk_cap = chunk_cap;
    W2_ALLOC(c.cs_defer, uint32_t, (uint64_t)nbl + 2);
    c.cs_planned = NS; c.cs_ns = 0; c.cs_nbl = nbl; c.cs_nseg = nseg; c.cs_recs = d_recs;
    c.cs_short_first = deferred && NS >= 3;        // deferred: slice 0's records are exchanged before anything can be counted -- keep it short
    if (!deferred) for (unsigned k = 0; k < NS; ++k) W2_TRY(count_buckets_launch_slice(c, k));
    return 0;
}

// bucket range of slice k: equal slices, or (cs_short_first) a first slice of half the size of the others
void count_slice_bounds(const Ctx& c, unsigned k, uint32_t* b_lo, uint32_t* b_hi) {
    const uint64_t NS = c.cs_planned, nbl = c.cs_nbl;
    auto cut = [&](uint64_t j) -> uint32_t {
        if (!c.cs_short_first) return (uint32_t)(nbl * j / NS);
        return (uint32_t)(j == 0 ? 0 : nbl * (2 * j - 1) / (2 * NS - 1));       // weights 1, 2, 2, ..
    };
    *b_lo = cut(k); *b_hi = cut(k + 1);
}

// launches bucket slice k of a prepared count (slices go in order; deferred mode: the caller launches slice k once its
// records have arrived)
int count_buckets_launch_slice(Ctx& c, unsigned k) {
    hipStream_t st = c.stream;
    if (!c.cs_planned || k != c.cs_ns || k >= c.cs_planned) { c.err = "count_records_launch: slices are launched once each, in order"; return W2RAP_E_STATE; }
    const unsigned NS = c.cs_planned;
    const uint32_t nbl = c.cs_nbl, nseg = c.cs_nseg;
    const uint32_t nb_arg = nbl | (c.cs_packed ? SEG_PACKED : 0u);     // the kernels' segment-table stride, with the table's form
    unsigned long long* d_cnt = c.cs_cnt;
    // (the bucket queue in a 128-byte line of its own: the counters behind d_cnt + 4 take one same-address atomic per bucket too -- its output range --,
    //  and two hot words in one line share one L2 channel's atomic unit)
#ifndef W2RAP_QUEUE_AT
#define W2RAP_QUEUE_AT 144
#endif
    uint32_t* d_queue = reinterpret_cast<uint32_t*>(d_cnt + W2RAP_QUEUE_AT);
    uint32_t b_lo, b_hi;
    count_slice_bounds(c, k, &b_lo, &b_hi);
    auto slice_done = [&]() -> int {
        W2_HIP(hipMemcpyAsync(c.h_pinned + k, d_cnt + 4, 8, hipMemcpyDeviceToHost, st));
        W2_HIP(hipEventCreateWithFlags(&c.cs_ev[k], hipEventDisableTiming));
        W2_HIP(hipEventRecord(c.cs_ev[k], st));
        c.cs_ns = k + 1;
        return 0;
    };
    auto launch = [&](auto kern, unsigned lds, unsigned threads, unsigned blocks_per_cu) -> int {
        W2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        unsigned grid = (unsigned)std::min<uint64_t>(b_hi - b_lo, (uint64_t)c.sm_count * blocks_per_cu);
        if (k || c.pass) W2_HIP(hipMemsetAsync(d_queue, 0, 4, st));
        LAUNCH(c, "k_count_buckets", kern, dim3(grid ? grid : 1), dim3(threads), lds, nb_arg, b_lo, b_hi, nseg, c.cs_off, c.cs_recs, c.min_freq, d_queue,
               c.d_shi, c.d_slo, c.d_scc, c.solid_cap, d_cnt + 4, d_cnt + 8, c.d_chunk_start, c.d_chunk_cnt, c.cs_chunk_cap, (const uint32_t*)nullptr, 0u);
        W2_HIP(hipGetLastError());
        return slice_done();
    };
    // the round-4 shape: fingerprint + reference slots over the bucket's resident records, two (or more) blocks per CU; what it defers
    // (a bucket beyond its tile or table) is counted behind it by the round-1..3 kernel in list mode
    auto launch_fp = [&](auto kern, unsigned lds, unsigned threads, unsigned blocks_per_cu, uint32_t fp_limit, uint32_t fp_sc) -> int {
        W2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        auto list_kern = k_count_buckets<COUNT_CAP, COUNT_THREADS>;
        W2_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(list_kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)K3Cfg<COUNT_CAP, COUNT_THREADS>::LDS));
        const unsigned grid = (unsigned)std::min<uint64_t>(b_hi - b_lo, (uint64_t)c.sm_count * blocks_per_cu);
        if (k || c.pass) W2_HIP(hipMemsetAsync(d_queue, 0, 4, st));
        if (k == 0) W2_HIP(hipMemsetAsync(c.cs_defer, 0, 8, st));                 // the deferred buckets of ALL slices collect in one list ...
        // (test hooks: a tiny table / staging area sends nearly every bucket through the hash-class path)
        uint32_t fill_limit = fp_limit, solid_limit = fp_sc;
        if (const char* t = getenv("W2RAP_TEST_FP_LIMIT")) { if (test_hook("W2RAP_TEST_FP_LIMIT")) fill_limit = std::min<uint32_t>(fill_limit, (uint32_t)std::max(1, atoi(t))); }
        if (const char* t = getenv("W2RAP_TEST_FP_SC")) { if (test_hook("W2RAP_TEST_FP_SC")) solid_limit = std::min<uint32_t>(solid_limit, (uint32_t)std::max(1, atoi(t))); }
        // (test hook: 0 makes every held slot of the record table a tag match, 1 half of them -- the content compare has to tell the records apart)
        uint32_t dedup_tag_mask = 0xFFFFFFFFu;
        if (const char* t = getenv("W2RAP_TEST_DEDUP_TAG_MASK")) { if (test_hook("W2RAP_TEST_DEDUP_TAG_MASK")) dedup_tag_mask = (uint32_t)strtoul(t, nullptr, 0); }
        LAUNCH(c, "k_count_fp", kern, dim3(grid ? grid : 1), dim3(threads), lds, nb_arg, b_lo, b_hi, nseg, c.cs_off, c.cs_recs, c.min_freq, d_queue,
               c.d_shi, c.d_slo, c.d_scc, c.solid_cap, d_cnt + 4, d_cnt + 8, c.d_chunk_start, c.d_chunk_cnt, c.cs_chunk_cap, c.cs_defer, nbl, fill_limit, solid_limit,
               c.fused_prune ? c.d_sctx : (uint8_t*)nullptr, c.fused_prune ? c.d_unres : (uint8_t*)nullptr, c.fused_prune ? (uint32_t*)c.d_nbr : (uint32_t*)nullptr,
               dedup_tag_mask);
        W2_HIP(hipGetLastError());
        if (k + 1 == NS && c.fused_prune) W2_HIP(hipMemcpyAsync(c.h_pinned + 20, d_cnt + 4, 8, hipMemcpyDeviceToHost, st));      // chunks so far: the list kernel's come behind
        if (k + 1 == NS) {
            // ... which the list kernel counts behind the last slice: one launch with every block busy instead of one thin launch per slice
            // (its buckets are the heavy ones: several tiles, hash classes -- 50-80 us each)
            const unsigned lgrid = (unsigned)std::min<uint64_t>(nbl, (uint64_t)c.sm_count);
            constexpr unsigned list_lds = K3Cfg<COUNT_CAP, COUNT_THREADS>::LDS;
            LAUNCH(c, "k_count_buckets", list_kern, dim3(lgrid ? lgrid : 1), dim3(COUNT_THREADS), list_lds, nb_arg, 0u, nbl, nseg, c.cs_off,
                   c.cs_recs, c.min_freq, c.cs_defer + 1, c.d_shi, c.d_slo, c.d_scc, c.solid_cap, d_cnt + 4, d_cnt + 8, c.d_chunk_start, c.d_chunk_cnt, c.cs_chunk_cap,
                   (const uint32_t*)c.cs_defer, nbl);
            W2_HIP(hipGetLastError());
        }
        return slice_done();
    };
    const char* v = getenv("W2RAP_K3");            // tuning knob: table/block shape
    int cfg = v ? atoi(v) : 22;
    if (cfg >= 20 && nseg > FpCfg<512, 512, 1024>::MAXSEG) cfg = 0;
    // (threads, min waves per SIMD, resident records, solid k-mers per bucket): two 512-thread blocks per CU is the shipped shape.  Default
    // 22 since K1 cuts 17 % fewer records (a 4500-k-mer bucket holds ~240): 512 resident records are enough -- 0.2 % of the buckets go to
    // the list kernel instead of 0.004 % -- and k_count_fp is 0.7 ms faster than with shape 20's 640 (three alternating runs, and the
    // planted workload within 0.2 ms: profiles/r04_sched_ab.txt)
    // Record dedup (NOTES.md section 18): byte-identical records of a bucket are counted once, with their multiplicity as the weight.  W2RAP_FP_DEDUP=0
    // launches the form without it (the A/B, and the parity tests run both).
    const char* ddv = getenv("W2RAP_FP_DEDUP");
    const bool dedup = !(ddv && atoi(ddv) == 0);
#define W2_FP_SHAPE(T, W, TL, S, BPC)                                                                                                                  \
    W2_TRY(dedup ? launch_fp(k_count_fp_dedup<T, W, TL, S>, FpCfg<T, TL, S>::LDS_DEDUP, T, BPC, FpCfg<T, TL, S>::LIMIT, S)                             \
                 : launch_fp(k_count_fp<T, W, TL, S>, FpCfg<T, TL, S>::LDS, T, BPC, FpCfg<T, TL, S>::LIMIT, S))
    if (cfg == 20) W2_FP_SHAPE(512, 4, 640, 768, 2);
    else if (cfg == 21) W2_FP_SHAPE(1024, 8, 576, 512, 2);
    else if (cfg == 22) W2_FP_SHAPE(512, 4, 512, 1024, 2);
    else if (cfg == 23) W2_FP_SHAPE(1024, 4, 576, 1024, 1);
    else if (cfg == 24) W2_FP_SHAPE(512, 4, 576, 1024, 2);
#undef W2_FP_SHAPE
    else if (cfg == 1) W2_TRY(launch(k_count_buckets<2048, 512>, K3Cfg<2048, 512>::LDS, 512, 2));
    else if (cfg == 2) W2_TRY(launch(k_count_buckets<4096, 512>, K3Cfg<4096, 512>::LDS, 512, 1));
    else if (cfg == 3) W2_TRY(launch(k_count_buckets<1024, 256>, K3Cfg<1024, 256>::LDS, 256, 4));
    // round-3 experiments (profiles/r03_k3_variants.txt; results identical, times at 50 M reads against 50.3 ms for the shipped form):
    //   5: no parking queue, 2048 slots, 256-record tiles -> 62 KB of LDS, 64 VGPRs (39 spilled): TWO blocks per CU, eight waves per SIMD: 69.2 ms
    //   8: the shipped shape without the parking queue (collisions probed at once): 61.9 ms
    else if (cfg == 5) W2_TRY(launch(k_count_buckets<2048, 1024, false, false, 8>, K3Cfg<2048, 1024, false>::LDS, 1024, 2));
    else if (cfg == 8) W2_TRY(launch(k_count_buckets<4096, 1024, false, false, 1>, K3Cfg<4096, 1024, false>::LDS, 1024, 1));
    else if (cfg == 9) W2_TRY(launch(k_count_buckets<COUNT_CAP, COUNT_THREADS, true>, K3Cfg<COUNT_CAP, COUNT_THREADS>::LDS, COUNT_THREADS, 1));
    else W2_TRY(launch(k_count_buckets<COUNT_CAP, COUNT_THREADS>, K3Cfg<COUNT_CAP, COUNT_THREADS>::LDS, COUNT_THREADS, 1));
    return 0;
}

// waits for slice k; -> solid k-mers / chunks emitted by slices 0..k (all of them written)
int count_buckets_slice(Ctx& c, unsigned k, uint64_t* n_solid, uint64_t* n_chunks) {
    if (k >= c.cs_ns) { c.err = "count_records_slice: slice not launched"; return W2RAP_E_ARG; }
    W2_HIP(hipEventSynchronize(c.cs_ev[k]));
    const uint64_t w = c.h_pinned[k];
    if (n_solid) *n_solid = std::min<uint64_t>(w & ((1ull << 40) - 1), c.solid_cap);
    if (n_chunks) *n_chunks = std::min<uint64_t>(w >> 40, c.cs_chunk_cap);
    return 0;
}

int count_buckets_finish(Ctx& c) {
    hipStream_t st = c.stream;
    if (!c.cs_planned || c.cs_ns != c.cs_planned) { c.err = "count_records_end: not every slice has been launched"; return W2RAP_E_STATE; }
    unsigned long long h_all[160];
    W2_HIP(hipMemcpyAsync(h_all, c.cs_cnt, sizeof(h_all), hipMemcpyDeviceToHost, st));
    W2_HIP(hipStreamSynchronize(st));
    for (unsigned k = 0; k < c.cs_ns; ++k) (void)hipEventDestroy(c.cs_ev[k]);
    c.cs_ns = 0; c.cs_planned = 0;
    if (c.pass + 1 < c.npass) c.pass_cnt = c.cs_cnt;                     // the next pass goes on counting into these
    else { c.release(c.cs_cnt); c.pass_cnt = nullptr; c.pass = 0; c.npass = 1; }
    c.release(c.cs_off); c.cs_cnt = nullptr; c.cs_off = nullptr;
    if (getenv("W2RAP_TRACE") && c.cs_defer) {
        uint32_t nd = 0;
        (void)hipMemcpy(&nd, c.cs_defer, 4, hipMemcpyDeviceToHost);
        fprintf(stderr, "[w2rap] k_count_fp deferred %u buckets (all slices) to k_count_buckets\n", nd);
    }
    if (c.cs_defer) { c.release(c.cs_defer); c.cs_defer = nullptr; }
    if (getenv("W2RAP_TRACE") && h_all[111])
        fprintf(stderr, "[w2rap] k_count_buckets wave-0 clocks per block: stage-in %.0f, count %.0f, barrier A %.0f, flush+scan %.0f, barrier B %.0f, staging %.0f; slowest wave's count %.0f (x%u blocks, %u buckets)\n",
                (double)h_all[110] / c.sm_count, (double)h_all[111] / c.sm_count, (double)h_all[112] / c.sm_count, (double)h_all[113] / c.sm_count,
                (double)h_all[114] / c.sm_count, (double)h_all[115] / c.sm_count, (double)h_all[116] / c.sm_count, (unsigned)c.sm_count, 0u);
    if (getenv("W2RAP_TRACE") && h_all[128]) {
        fprintf(stderr, "[w2rap] k_count_buckets count-phase clocks per block, by wave:");
        for (int w = 0; w < 16; ++w) fprintf(stderr, " %.1fM", (double)h_all[128 + w] / c.sm_count / 1e6);
        fprintf(stderr, "\n");
    }
    if (getenv("W2RAP_TRACE") && h_all[121])
        fprintf(stderr, "[w2rap] k_count_buckets wave-0 clocks per window: loads %.0f, extract+hash %.0f, probe %.0f, atomics %.0f (%.0f windows per block)\n",
                (double)h_all[117] / h_all[121], (double)h_all[118] / h_all[121], (double)h_all[119] / h_all[121], (double)h_all[120] / h_all[121],
                (double)h_all[121] / c.sm_count);
    if (h_all[7]) { c.err = "k_count_buckets: a bucket did not fit the LDS table after 2^16-way splitting"; return W2RAP_E_LIMIT; }
    c.S = h_all[4] & ((1ull << 40) - 1); c.D = h_all[5];
    c.nchunks = c.cs_chunk_cap ? std::min<uint64_t>(h_all[4] >> 40, c.cs_chunk_cap) : 0;
    for (int i = 0; i < 101; ++i) c.hist[i] = h_all[8 + i];
    if (c.S > c.solid_cap) { c.err = "solid k-mer count exceeds its bound"; return W2RAP_E_LIMIT; }
    return 0;
}

// lookup-table + absence-filter storage for `S` solid k-mers, cleared on stream `on`
static int table_alloc(Ctx& c, uint64_t S, hipStream_t on) {
    uint64_t tcap;
    table_geometry(S, tcap);
    c.tcap = tcap;
    W2_ALLOC(c.d_table, Slot, tcap);
    W2_HIP(hipMemsetAsync(c.d_table, 0xFF, tcap * sizeof(Slot), on));
    return 0;
}

// single-GPU counting: all buckets of this GPU; with build_table the solid k-mers of a finished slice are inserted into the
// lookup table on the side stream while the next slice counts.  The table is sized from the first slice (buckets are
// hash-uniform, so S ~ NS * S_1); if the guess turns out too small the table is rebuilt the plain way.
int count_buckets(Ctx& c, uint32_t min_freq, uint32_t nbl, uint32_t nseg, const uint32_t* d_recs, const uint32_t* d_counts,
                  uint64_t total_kmers, bool build_table) {
    hipStream_t st2 = c.stream2;
    const char* nsv = getenv("W2RAP_SLICES");
    unsigned NS = (build_table && !getenv("W2RAP_NO_OVERLAP") && nbl >= 4096 && st2) ? (nsv ? (unsigned)atoi(nsv) : 4) : 1;
    // The chunk-local adjacency prune inside k_count_fp's emit (W2RAP_FUSED_PRUNE=1): only where the k-mer numbering of this count is final
    // (one GPU, one pass: build_table), node ids are 32-bit words, and the round-4 kernel counts (its deferred buckets, which the list kernel
    // counts, keep k_prune_local).  The prune's arrays exist before the first launch then, sized by the bound of the solid set.
    {
        const char* fv = getenv("W2RAP_FUSED_PRUNE"); const char* kv = getenv("W2RAP_K3"); const char* wv = getenv("W2RAP_WIDE_IDS");
        const uint64_t cap = total_kmers / (min_freq ? min_freq : 1) + 1;
        c.fused_prune = build_table && fv && atoi(fv) == 1 && !(kv && atoi(kv) < 20) && !(wv && atoi(wv) != 0) && cap < (1ull << 31) - 1 && c.npass == 1 &&
                        nseg <= 16 && !getenv("W2RAP_NO_LOCAL_PRUNE");
        c.unfused_chunks.clear();
        if (c.fused_prune) {
            for (void* p : {(void*)c.d_sctx, (void*)c.d_nbr, (void*)c.d_unres}) if (p) c.release(p);
            W2_ALLOC(c.d_sctx, uint8_t, cap); W2_ALLOC(c.d_unres, uint8_t, cap);
            uint32_t* nb32 = nullptr; W2_ALLOC(nb32, uint32_t, 2 * cap); c.d_nbr = nb32;
            W2_HIP(hipMemsetAsync(c.d_sctx, 0xFF, cap, c.stream));      // unvisited k-mers (the list kernel's chunks until k_prune_local): every bit open
            W2_HIP(hipMemsetAsync(c.d_unres, 0xFF, cap, c.stream));
        }
    }
    // (Round 5, measured and removed: the bucket-local prune slice by slice on the side stream, under the counting of the next slice --
    //  count phase 70.2 -> 77.7 ms: like the table inserts, it takes from k_count_fp more than it saves behind it.)
    W2_TRY(count_buckets_launch(c, min_freq, nbl, nseg, d_recs, d_counts, total_kmers, NS, false));
    NS = c.cs_ns;
    uint64_t s_cap = 0;
    if (NS > 1) {
        uint64_t s_prev = 0;
        for (unsigned k = 0; k < NS; ++k) {
            uint64_t s_k = 0;
            W2_TRY(count_buckets_slice(c, k, &s_k, nullptr));
            if (k == 0) {
                s_cap = s_k * NS + s_k / 2 + 1024;          // 12 % head room over the extrapolation
                if (test_hook("W2RAP_TEST_SMALL_SCAP")) s_cap = s_k + 1;   // test hook: make the extrapolation fail
                W2_TRY(table_alloc(c, s_k * NS, st2));      // the table itself is laid out for the extrapolation (a power of two)
            }
            const uint64_t s_hi = s_k < s_cap ? s_k : s_cap;
            if (s_hi > s_prev) {
                LAUNCH_ON(c, st2, "k_table_insert", k_table_insert, dim3((unsigned)((s_hi - s_prev + 255) / 256)), dim3(256), 0, s_prev, s_hi,
                          c.d_shi, c.d_slo, c.d_table, c.tcap - 1);
                W2_HIP(hipGetLastError());
                s_prev = s_hi;
            }
        }
    }
    // the last slice's insert is still running on the side stream: the bucket-local prune does not need the table and
    // runs beside it (count_table waits for the side stream before the first global probe)
    W2_TRY(count_buckets_finish(c));
    if (c.fused_prune) c.unfused_chunks.emplace_back(std::min<uint64_t>(c.h_pinned[20] >> 40, c.nchunks), c.nchunks);
    if (NS > 1) {
        if (c.S <= s_cap && 10 * c.tcap >= 13 * c.S) c.table_built = true;  // load <= 0.77 at worst; normally the intended 0.25
        else {                                                            // the extrapolation was too small: build it the plain way
            W2_HIP(hipStreamSynchronize(st2));
            c.release(c.d_table);
            c.d_table = nullptr;
        }
    }
    return 0;
}

// ---- dictionary built incrementally from gathered solid k-mers (multi-GPU): every append is copied behind the ones
// before it and inserted into the table on the side stream, while the main stream keeps counting the next bucket slice.
__global__ void __launch_bounds__(256) k_shift_u64(uint64_t n, const uint64_t* __restrict__ in, uint64_t add, uint64_t* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + add;
}
void dict_abort(Ctx& c) {
    if (!c.g_open) return;
    if (c.stream2) (void)hipStreamSynchronize(c.stream2);
    for (void* p : {(void*)c.g_hi, (void*)c.g_lo, (void*)c.g_cc, (void*)c.g_cstart, (void*)c.g_ccnt, (void*)c.d_table}) if (p) c.release(p);
    c.g_hi = c.g_lo = nullptr; c.g_cc = nullptr; c.g_cstart = nullptr; c.g_ccnt = nullptr; c.d_table = nullptr;
    c.g_open = false; c.g_n = c.g_nc = 0;
}
int dict_begin(Ctx& c, uint64_t kmer_cap, uint64_t chunk_cap) {
    if (c.g_open) dict_abort(c);
    if (!c.stream2) { c.err = "dict_begin: no side stream"; return W2RAP_E_STATE; }
    if (kmer_cap >= MAX_SOLID_KMERS) { c.err = "more than 2^32 solid k-mers on one GPU"; return W2RAP_E_LIMIT; }
    if (c.d_table) c.release(c.d_table);
    c.d_table = nullptr;
    W2_ALLOC(c.g_hi, uint64_t, kmer_cap); W2_ALLOC(c.g_lo, uint64_t, kmer_cap); W2_ALLOC(c.g_cc, uint32_t, kmer_cap);
    c.g_cstart = nullptr; c.g_ccnt = nullptr;
    if (chunk_cap) { W2_ALLOC(c.g_cstart, uint64_t, chunk_cap); W2_ALLOC(c.g_ccnt, uint32_t, chunk_cap); }
    c.g_cap = kmer_cap; c.g_ccap = chunk_cap; c.g_n = 0; c.g_nc = 0;
    W2_TRY(table_alloc(c, kmer_cap, c.stream2));
    c.g_open = true;
    return 0;
}
// (chunk_bias: the chunk starts handed over count from that k-mer of the source array on -- a slice of an owner's arrays, given in place)
int dict_append(Ctx& c, const uint64_t* d_hi, const uint64_t* d_lo, const uint32_t* d_cc, uint64_t n, const uint64_t* d_cstart, const uint32_t* d_ccnt,
                uint64_t nc, uint64_t chunk_bias) {
    hipStream_t st2 = c.stream2;
    if (!c.g_open) { c.err = "dict_append before dict_begin"; return W2RAP_E_STATE; }
    if (c.g_n + n > c.g_cap || (nc && c.g_nc + nc > c.g_ccap)) { c.err = "dict_append: capacity of dict_begin exceeded"; return W2RAP_E_LIMIT; }
    // first everything that is COPIED (k-mers, chunk list), then an event, then the insert kernel: dict_end lets the main stream
    // wait for the last append's copies only -- the bucket-local prune reads the k-mers and the chunk list but not the table, and
    // runs beside the last insert
    if (n) {
        W2_HIP(hipMemcpyAsync(c.g_hi + c.g_n, d_hi, n * 8, hipMemcpyDeviceToDevice, st2));
        W2_HIP(hipMemcpyAsync(c.g_lo + c.g_n, d_lo, n * 8, hipMemcpyDeviceToDevice, st2));
        W2_HIP(hipMemcpyAsync(c.g_cc + c.g_n, d_cc, n * 4, hipMemcpyDeviceToDevice, st2));
    }
    if (nc) {
        hipLaunchKernelGGL(k_shift_u64, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st2, nc, d_cstart, c.g_n - chunk_bias, c.g_cstart + c.g_nc);
        W2_HIP(hipMemcpyAsync(c.g_ccnt + c.g_nc, d_ccnt, nc * 4, hipMemcpyDeviceToDevice, st2));
    }
    if (!c.g_copied) W2_HIP(hipEventCreateWithFlags(&c.g_copied, hipEventDisableTiming));
    W2_HIP(hipEventRecord(c.g_copied, st2));
    if (n) {
        LAUNCH_ON(c, st2, "k_table_insert", k_table_insert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.g_n, c.g_n + n,
                  c.g_hi, c.g_lo, c.d_table, c.tcap - 1);
        W2_HIP(hipGetLastError());
    }
    c.g_n += n; c.g_nc += nc;
    return 0;
}
// the gathered dictionary becomes the context's solid set; adjacency prune (count_table)
int dict_end(Ctx& c) {
    if (!c.g_open) { c.err = "dict_end before dict_begin"; return W2RAP_E_STATE; }
    if (c.cs_planned) { c.err = "dict_end while a sliced count is pending (count_records_end first)"; return W2RAP_E_STATE; }
    for (void* p : {(void*)c.d_shi, (void*)c.d_slo, (void*)c.d_scc, (void*)c.d_recs, (void*)c.d_sctx, (void*)c.d_nbr, (void*)c.d_chunk_start, (void*)c.d_chunk_cnt})
        if (p) c.release(p);
    c.d_recs = nullptr; c.d_sctx = nullptr; c.d_nbr = nullptr;
    c.d_shi = c.g_hi; c.d_slo = c.g_lo; c.d_scc = c.g_cc; c.S = c.g_n; c.solid_cap = c.g_cap;
    c.d_chunk_start = c.g_cstart; c.d_chunk_cnt = c.g_ccnt; c.nchunks = c.g_nc;
    c.g_hi = c.g_lo = nullptr; c.g_cc = nullptr; c.g_cstart = nullptr; c.g_ccnt = nullptr; c.g_open = false;
    bool wait_copies = true;
#ifdef W2RAP_TESTING
    if (test_hook("W2RAP_TEST_NO_APPEND_WAIT")) wait_copies = false;     // re-opens the race of commit b0ca512 (testing builds only)
#endif
    if (c.g_copied && wait_copies) W2_HIP(hipStreamWaitEvent(c.stream, c.g_copied, 0));       // the appended k-mers and chunks are in place (the last insert may still run)
    if (10 * c.tcap >= 13 * c.S) c.table_built = true;
    else {                                               // capacity guess far too small for the load factor: plain rebuild
        W2_HIP(hipStreamSynchronize(c.stream2));
        c.release(c.d_table);
        c.d_table = nullptr; c.table_built = false;
    }
    return count_table(c);
}

// ---- pieces of K4 + K5 for the sharded dictionary (step2_shard.hip): the table over this owner's k-mers, built in one go; the
// bucket-local step of the prune over its chunk list with 64-bit node numbers (LOCAL ones: 2 * index + orientation)
int table_build_plain(Ctx& c) {
    if (c.d_table) { c.release(c.d_table); c.d_table = nullptr; }
    W2_TRY(table_alloc(c, c.S, c.stream));
    if (c.S) {
        LAUNCH(c, "k_table_insert", k_table_insert, dim3((unsigned)((c.S + 255) / 256)), dim3(256), 0, (uint64_t)0, c.S, c.d_shi, c.d_slo, c.d_table, c.tcap - 1);
        W2_HIP(hipGetLastError());
    }
    c.table_built = false;
    return 0;
}
// The owner's OWN dictionary built under its counting (sharded dictionary, row e-3): after bucket slice k the solid k-mers [done, n_solid) of
// c.d_shi are inserted on the side stream while slice k+1 counts (what count_buckets does on one GPU).  The first call lays the table out
// for `expected_total` (the caller's extrapolation from the first slice); a table that turns out too small is rebuilt by shard_begin.
int local_dict_slice(Ctx& c, uint64_t n_solid, uint64_t expected_total) {
    if (!c.stream2) return 0;
    if (!c.table_built) {
        if (c.d_table) { c.release(c.d_table); c.d_table = nullptr; }
        W2_TRY(table_alloc(c, std::max<uint64_t>(expected_total, n_solid), c.stream2));
        c.table_built = true; c.ld_done = 0;
    }
    if (n_solid > c.solid_cap) n_solid = c.solid_cap;
    if (n_solid > c.ld_done && 10 * c.tcap >= 13 * n_solid) {          // (beyond its load limit the table is abandoned: nothing more goes in, shard_begin rebuilds)
        LAUNCH_ON(c, c.stream2, "k_table_insert", k_table_insert, dim3((unsigned)((n_solid - c.ld_done + 255) / 256)), dim3(256), 0, c.ld_done, n_solid,
                  c.d_shi, c.d_slo, c.d_table, c.tcap - 1);
        W2_HIP(hipGetLastError());
        c.ld_done = n_solid;
    }
    return 0;
}
int prune_local_chunks64(Ctx& c, uint8_t* sctx, uint64_t* nbr, uint8_t* unres) {
    hipStream_t st = c.stream;
    W2_HIP(hipMemsetAsync(unres, 0xFF, c.S, st));       // unvisited k-mers (oversized or unlisted chunks): every bit open
    W2_HIP(hipMemsetAsync(sctx, 0xFF, c.S, st));
    if (!c.nchunks || getenv("W2RAP_NO_LOCAL_PRUNE")) return 0;
    const unsigned gl = (unsigned)std::min<uint64_t>(c.nchunks, (uint64_t)c.sm_count * 64);
    PL_LAUNCH(c, uint64_t, gl, c.S, c.nchunks, c.d_chunk_start, c.d_chunk_cnt, c.d_shi, c.d_slo, c.d_scc, sctx, nbr, unres);
    W2_HIP(hipGetLastError());
    return 0;
}
int prune_local_chunks32(Ctx& c, uint8_t* sctx, uint32_t* nbr, uint8_t* unres) {
    hipStream_t st = c.stream;
    W2_HIP(hipMemsetAsync(unres, 0xFF, c.S, st));       // unvisited k-mers (oversized or unlisted chunks): every bit open
    W2_HIP(hipMemsetAsync(sctx, 0xFF, c.S, st));
    if (!c.nchunks || getenv("W2RAP_NO_LOCAL_PRUNE")) return 0;
    const unsigned gl = (unsigned)std::min<uint64_t>(c.nchunks, (uint64_t)c.sm_count * 64);
    PL_LAUNCH(c, uint32_t, gl, c.S, c.nchunks, c.d_chunk_start, c.d_chunk_cnt, c.d_shi, c.d_slo, c.d_scc, sctx, nbr, unres);
    W2_HIP(hipGetLastError());
    return 0;
}

// ---- K4+K5: lookup table over c.d_shi/d_slo/d_scc[0..S) and adjacency prune
template <class Id>
static int count_table_t(Ctx& c) {
    hipStream_t st = c.stream;
    if (!c.table_built) W2_TRY(table_alloc(c, c.S, st));
    const bool fused = c.fused_prune && sizeof(Id) == 4 && c.d_sctx && c.d_nbr && c.d_unres;      // most chunks are pruned already (inside k_count_fp's emit, or slice by slice on the side stream)
    Id* nbr = nullptr;
    if (fused) nbr = reinterpret_cast<Id*>(c.d_nbr);
    else {
        for (void* p : {(void*)c.d_sctx, (void*)c.d_nbr, (void*)c.d_unres}) if (p) c.release(p);
        c.d_unres = nullptr;
        W2_ALLOC(c.d_sctx, uint8_t, c.S);
        W2_ALLOC(nbr, Id, 2 * c.S);
        c.d_nbr = nbr;
    }
    c.fused_prune = false;
    if (c.S) {
        unsigned g = (unsigned)((c.S + 255) / 256);
        if (!c.table_built) {
            LAUNCH(c, "k_table_insert", k_table_insert, dim3(g), dim3(256), 0, (uint64_t)0, c.S, c.d_shi, c.d_slo, c.d_table, c.tcap - 1);
            W2_HIP(hipGetLastError());
        }
        uint8_t* d_unres = nullptr;
        if (fused) {
            d_unres = c.d_unres; c.d_unres = nullptr;
            for (auto& rg : c.unfused_chunks) {                  // the list kernel's chunks: the bucket-local prune as before
                const uint64_t nch = rg.second - rg.first;
                if (!nch) continue;
                const unsigned gl = (unsigned)std::min<uint64_t>(nch, (uint64_t)c.sm_count * 64);
                PL_LAUNCH(c, Id, gl, c.S, nch, c.d_chunk_start + rg.first, c.d_chunk_cnt + rg.first, c.d_shi, c.d_slo, c.d_scc, c.d_sctx, nbr, d_unres);
                W2_HIP(hipGetLastError());
            }
        } else if (c.nchunks) {
            W2_ALLOC(d_unres, uint8_t, c.S);
            W2_HIP(hipMemsetAsync(d_unres, 0xFF, c.S, st));       // unvisited k-mers (oversized or unlisted chunks): every bit open
            W2_HIP(hipMemsetAsync(c.d_sctx, 0xFF, c.S, st));
            // (the two steps as a pipeline over four groups of chunks on two streams -- bucket-local step of group j+1 beside the global probes of
            //  group j -- was measured in round 4: 12.8-13.8 ms against 11.9 ms back to back: both wait for the same random sectors.  Removed.)
            const unsigned gl = (unsigned)std::min<uint64_t>(c.nchunks, (uint64_t)c.sm_count * 64);
            PL_LAUNCH(c, Id, gl, c.S, c.nchunks, c.d_chunk_start, c.d_chunk_cnt, c.d_shi, c.d_slo, c.d_scc, c.d_sctx, nbr, d_unres);
            W2_HIP(hipGetLastError());
        }
        if (c.table_built && c.stream2) {            // dictionary built on the side stream: complete before the first probe
            hipEvent_t ev;
            W2_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            W2_HIP(hipEventRecord(ev, c.stream2));
            W2_HIP(hipStreamWaitEvent(st, ev, 0));
            (void)hipEventDestroy(ev);
        }
        LAUNCH(c, "k_prune", k_prune<Id>, dim3(g), dim3(256), 0, (uint64_t)0, c.S, c.d_shi, c.d_slo, c.d_scc, c.d_table, c.tcap - 1, c.d_sctx, nbr,
               (const uint8_t*)d_unres);
        W2_HIP(hipGetLastError());
        W2_HIP(hipStreamSynchronize(st));
        if (d_unres) c.release(d_unres);
    }
    W2_HIP(hipStreamSynchronize(st));
    if (c.stream2) W2_HIP(hipStreamSynchronize(c.stream2));
    c.table_built = false;
    c.counted = true;
    return 0;
}
// ---- K4+K5: lookup table over c.d_shi/d_slo/d_scc[0..S) and adjacency prune.  Node ids are 32-bit words while S < 2^31 and 64-bit
// words beyond (W2RAP_WIDE_IDS=1 forces the wide path on any input: the parity tests run both).
int count_table(Ctx& c) {
    if (c.S >= MAX_SOLID_KMERS) { c.err = "more than 2^32 solid k-mers on one GPU"; return W2RAP_E_LIMIT; }
    const char* wv = getenv("W2RAP_WIDE_IDS");
    c.wide_ids = c.S >= (1ull << 31) - 1 || (wv && atoi(wv) != 0);
    return c.wide_ids ? count_table_t<uint64_t>(c) : count_table_t<uint32_t>(c);
}

// number of hash-range passes of the counting phase when the caller leaves the choice to the library: the super-k-mer records (32 B
// per ~15..23 k-mer instances) and the two descriptor buffers should take no more than a quarter of the free HBM
static unsigned auto_passes(uint64_t M) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !free_b) return 1;
    const double need = (double)M / 15.0 * REC_BYTES * 1.25;
    unsigned p = (unsigned)(need / ((double)free_b / 4.0)) + 1;
    return std::min(p, 64u);
}

int phase_count(Ctx& c, uint32_t min_qual, uint32_t min_freq) {
    const bool trace = getenv("W2RAP_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    W2_TRY(count_quality(c, min_qual));
    double t1 = now();
    const char* bv = getenv("W2RAP_BATCHES");
    const char* pv = getenv("W2RAP_PASSES");
    unsigned P = pv ? (unsigned)atoi(pv) : c.n_passes;
    if (!P) P = auto_passes(c.M);
    const uint32_t NB = default_buckets(c.M, 1);
    if (P > NB) P = NB;
    if (P < 1) P = 1;
    c.npass = P;
    double t_part = 0, t_cnt = 0;
    for (unsigned p = 0; p < P; ++p) {
        // pass p: the reads are cut again, only the records of buckets [NB p / P, NB (p+1) / P) are kept (MapReduceEngine.h:288-299)
        const uint32_t lo = (uint32_t)((uint64_t)NB * p / P), hi = (uint32_t)((uint64_t)NB * (p + 1) / P);
        unsigned nseg = 1;
        c.pass = p;
        double a = now();
        // (one GPU, one pass, the lane kernel, room for the slabs: the cutter stores the records itself; W2RAP_K1_SLABS=0: the scatter pass)
        uint32_t slabs = slab_route(c, NB, P);
        uint64_t ask_from = 1ull << 20;                  // (W2RAP_TEST_SLAB_SAMPLE_MIN: a test hook, so that a small input is asked too)
        if (const char* t = getenv("W2RAP_TEST_SLAB_SAMPLE_MIN")) { if (test_hook("W2RAP_TEST_SLAB_SAMPLE_MIN")) ask_from = (uint64_t)std::max(64ll, atoll(t)); }
        if (slabs && c.n >= ask_from) {                  // (an input whose buckets pass their slabs by much is faster on the scatter pass)
            uint64_t est = 0, limit = 0;
            W2_TRY(slab_excess_estimate(c, NB, slabs, &est, &limit));
            if (trace) fprintf(stderr, "[w2rap] partition: ~%llu records beyond slabs of %u (limit %llu)\n", (unsigned long long)est, slabs, (unsigned long long)limit);
            if (est > limit) slabs = 0;
        }
        if (slabs) {                                     // (an asked input whose list overflows after all is not cut a second time into slabs)
            bool refused = false;
            W2_TRY(count_partition_slabs(c, NB, slabs, ask_from, &refused));
            if (refused) slabs = 0; else nseg = 2;
        }
        if (!slabs) W2_TRY(count_partition_batched(c, NB, bv ? (unsigned)atoi(bv) : 4, &nseg, lo, hi));
        double b = now();
        W2_TRY(count_buckets(c, min_freq, hi - lo, nseg, c.d_recs, c.d_bcount, c.M, P == 1));
        c.release(c.d_recs); c.d_recs = nullptr;         // the records are no longer needed
        c.slab_cap = 0;
        t_part += b - a; t_cnt += now() - b;
    }
    c.pass = 0; c.npass = 1;
    double t3 = now();
    W2_TRY(count_table(c));
    double t4 = now();
    if (trace) fprintf(stderr, "[w2rap] count: quality %.1f ms, partition %.1f ms, buckets %.1f ms, table %.1f ms (%u pass%s)\n",
                       (t1 - t0) * 1e3, t_part * 1e3, t_cnt * 1e3, (t4 - t3) * 1e3, P, P == 1 ? "" : "es");
    return 0;
}

}  // namespace w2
