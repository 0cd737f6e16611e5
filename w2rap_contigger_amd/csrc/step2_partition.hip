// step2_partition.hip -- the partition of Step 2's counting phase: the reads' k-mers as super-k-mer records grouped by bucket.
//   K1  k_superkmers_lane, canonical-minimizer super-k-mers: bucket histogram + one descriptor per record
//       k_superkmers
//   K2  k_scatter_records descriptor -> 32-B record in its bucket  (K1+K2 replace the leaf loop BuildReadQGraph.cc:1062-1080 and
//                                                                   std::sort's partitioning :1081)
//       (one GPU, one pass, reads of up to 315 good bases: K1 stores the records itself, into a slab per bucket -- count_partition_slabs)
// Host side: every route -- the scatter pass in batches or with owner parts, the slab route, its 1/32 sample -- is a few lines of policy
// around ONE cut attempt (K1Cut, cut_attempt) into ONE kind of overflow list (OvList); K3..K5 and phase_count are step2_count.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "ctx.h"

namespace w2 {

// =============================================================================== K1+K2
// (mmer_key, bucket_of, wave_lds_fence: common.h -- the sharded graph phase and the pathing index use the same minimizers)

// One wavefront per read; a pass covers 128 k-mer positions (two per lane), i.e. a whole PE150 read.
// The canonical-minimizer of every k-mer is a sliding-window minimum over 46 m-mer keys; the window
// minimum is computed by doubling (2,4,8,16,32, then 32+16) entirely in registers with ds_bpermute
// lane shifts, so a pass is six cross-lane round trips deep and needs no barrier.  The m-mer key is
// mix32(canonical 15-mer): mix32 is a bijection, so distinct m-mers never tie and the choice depends
// only on the SET of canonical m-mers in the window (strand-symmetric, as it must be for a k-mer
// and its reverse complement to land in the same bucket).
__device__ inline uint32_t lane_shift(uint32_t lo, uint32_t hi, unsigned lane, unsigned d) {
    // value at position (lane + d) of the concatenation lo[0..63] ++ hi[0..63]
    const int idx = (int)(((lane + d) & 63u) << 2);
    const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute(idx, (int)lo);
    const uint32_t b = (uint32_t)__builtin_amdgcn_ds_bpermute(idx, (int)hi);
    return lane + d < 64 ? a : b;
}

// Output of K1: the number of records per bucket (fire-and-forget atomics) and one 8-B descriptor per record
// (bucket; start | nk-1 << 16 | hasL << 22 | hasR << 23).  Descriptors live at FIXED positions -- `spp` slots per
// (read, pass of 128 k-mer positions), unused slots keep the 0xFFFFFFFF the array was filled with -- so the wave
// neither reserves anything nor waits for memory; the rare pass with more than `spp` records appends the surplus
// to a small overflow list.  K2 turns every descriptor into a 32-B record with one thread per slot, so the slot
// reservations of a whole wavefront are in flight together instead of one read's at a time.
template <unsigned MINW>
__global__ void __launch_bounds__(256, MINW) k_superkmers(uint64_t n, uint32_t chunk, const uint8_t* __restrict__ bases,
                                                    const uint64_t* __restrict__ boff, const uint16_t* __restrict__ good,
                                                    uint32_t nb, uint32_t pb_lo, uint32_t pb_hi /* this pass keeps buckets [pb_lo, pb_hi) */,
                                                    uint32_t* __restrict__ bcount /* [pb_hi - pb_lo] */,
                                                    uint32_t nbl_part, uint32_t inv_nbl, unsigned long long* __restrict__ part_kmers,
                                                    uint2* __restrict__ s_desc, uint32_t spp, uint32_t npass,
                                                    const uint64_t* __restrict__ pass_off /* [n + 1]: read r's passes start at pass_off[r] */,
                                                    uint32_t* __restrict__ o_read, uint32_t* __restrict__ o_bkt, uint32_t* __restrict__ o_meta,
                                                    uint32_t* __restrict__ o_rank,
                                                    uint64_t ov_cap, unsigned long long* __restrict__ ov_cursor /*[0] entries*/) {
    // four independent wavefronts per block (a CU holds more 256-thread blocks than 64-thread ones); no block barriers
    __shared__ uint2 dbuf_[4][128];       // the descriptors of one pass, in record order
    __shared__ uint32_t spart_[4][64];    // multi-GPU: k-mers this wave sends to each owner rank (owner = bucket / nbl_part)
    const unsigned lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    if (part_kmers) { spart_[wv_][lane] = 0; wave_lds_fence(); }
    uint2* dbuf = dbuf_[wv_];
    // The window of a read that a pass needs (<= 206 bases = 52 bytes) lives in REGISTERS: lanes 0..15 hold the sixteen aligned dwords from
    // the dword that contains the window's first byte (an aligned word that holds a valid byte never leaves the allocation), and a lane
    // fetches the two dwords of its 15-mer from them with ds_bpermute.  (Rounds 1-3 staged the bytes in LDS: three fences, a clearing
    // store, a byte store -- 60 of the pass's 300 VALU instructions.)
    auto win_load = [&](uint64_t first_byte, unsigned nbytes) -> uint32_t {          // nbytes: valid bytes from first_byte on
        const uintptr_t a = reinterpret_cast<uintptr_t>(bases) + first_byte;         // (aligned by ADDRESS: the array itself may start anywhere)
        const unsigned sb = (unsigned)(a & 3);
        return 4 * lane < sb + nbytes ? reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3))[lane & 15u] : 0u;
    };
    // A wave takes `chunk` CONSECUTIVE reads and the grid has one wave per chunk: blocks are dispatched in order, so the reads
    // -- and with them the ranks the histogram atomic hands out inside a bucket -- advance roughly in read order, the order in
    // which the scatter pass writes the records (neighbouring slots of a bucket are then written close in time and meet in L2).
    const uint64_t stride = 1;
    uint64_t r = ((uint64_t)blockIdx.x * 4 + wv_) * chunk;
    const uint64_t r_end = r + chunk < n ? r + chunk : n;
    // Software pipeline over this wave's reads: the quality window and byte offset of the read after next and the
    // first 60 packed bytes of the next read are loaded while the current read is cut, so no read waits for HBM.
    unsigned gl_c = 0, gl_n = 0; uint64_t off_c = 0, off_n = 0; uint32_t win_c = 0;
    if (r < r_end) { gl_c = good[r]; off_c = boff[r]; }
    if (r + stride < r_end) { gl_n = good[r + stride]; off_n = boff[r + stride]; }
    if (r < r_end && lane < 16 && gl_c > K) win_c = win_load(off_c, (gl_c + 3) >> 2);
    for (; r < r_end; r += stride) {
        const unsigned gl = gl_c;
        const uint64_t off_cur = off_c;
        const uint32_t win0 = win_c;
        // look ahead
        unsigned gl_nn = 0; uint64_t off_nn = 0;
        if (r + 2 * stride < r_end) { gl_nn = good[r + 2 * stride]; off_nn = boff[r + 2 * stride]; }
        win_c = 0;
        if (r + stride < r_end && lane < 16 && gl_n > K) win_c = win_load(off_n, (gl_n + 3) >> 2);
        gl_c = gl_n; off_c = off_n; gl_n = gl_nn; off_n = off_nn;
        if (gl <= K) continue;                                   // strict, BuildReadQGraph.cc:1064: no records, no passes, no slots
        const unsigned nk_total = gl - (K - 1);
        const unsigned nbytes_read = (gl + 3) >> 2;
        for (unsigned c0 = 0; c0 < nk_total; c0 += 128) {
            // ---- stage the window of the read this pass needs: bases [c0-1, c0+189) ----
            const unsigned first_base = c0 ? c0 - 1 : 0;
            const unsigned b0a = (first_base >> 2) & ~3u;        // window start byte, dword aligned in the read
            // this pass's window: the prefetched dwords (first pass) or sixteen dwords from byte b0a of the read on
            uint32_t wdw = win0;
            if (c0) wdw = lane < 16 ? win_load(off_cur + b0a, nbytes_read - b0a) : 0u;
            const unsigned sbit = 8u * (unsigned)((reinterpret_cast<uintptr_t>(bases) + off_cur) & 3);   // the window's first byte inside its first dword (b0a is a multiple of 4)
            const unsigned sbase = 4 * b0a;                      // read base of the window's first byte
            // ---- canonical m-mer keys at m-mer positions c0+lane, c0+64+lane, c0+128+lane ----
            uint32_t k0, k1, k2;
            {
                uint32_t kk[3];
#pragma unroll
                for (int h = 0; h < 3; ++h) {
                    const unsigned j = c0 + h * 64 + lane;
                    uint32_t key = 0xFFFFFFFFu;
                    // (every lane takes part in the two cross-lane fetches; lanes without an m-mer read dword 0)
                    const bool has = j + MMER <= gl && (h < 2 || lane < WIN - 1);
                    const unsigned o = has ? sbit + 2 * (j - sbase) : 0u, wi = o >> 5, sh = o & 31;
                    const uint32_t w0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(wi << 2), (int)wdw);
                    const uint32_t w1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((wi + 1) << 2), (int)wdw);
                    if (has) {
                        const uint32_t f = __funnelshift_r(w0, w1, sh) & 0x3FFFFFFFu;                 // 15 bases, LSB first
                        // reverse complement in 32-bit ops: complement, reverse the 16 two-bit groups, drop the padding group
                        uint32_t rc = __brev(~f & 0x3FFFFFFFu);
                        rc = (((rc & 0x55555555u) << 1) | ((rc >> 1) & 0x55555555u)) >> 2;
                        key = mmer_key(f < rc ? f : rc);
                    }
                    kk[h] = key;
                }
                k0 = kk[0]; k1 = kk[1]; k2 = kk[2];
            }
            // ---- sliding-window minimum over WIN=46 keys, by 16-lane rows: the window [p, p+45] is the suffix of p's
            //      row from p, the prefix of (p+45)'s row up to p+45, and the one or two whole rows in between.
            //      Suffix/prefix minima inside rows are DPP scans (VALU only), row minima travel through SGPRs
            //      (v_readlane), and only the prefix at p+45 is a cross-lane fetch: 2 ds_bpermute per half-pass.
            constexpr uint32_t INF = 0xFFFFFFFFu;
            auto row_pref = [](uint32_t x) {
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x111, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x112, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x114, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x118, 0xF, 0xF, false));
                return x;
            };
            auto row_suff = [](uint32_t x) {
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x101, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x102, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x104, 0xF, 0xF, false));
                x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)x, 0x108, 0xF, 0xF, false));
                return x;
            };
            const uint32_t P0 = row_pref(k0), P1 = row_pref(k1), P2 = row_pref(k2), S0 = row_suff(k0), S1 = row_suff(k1);
            uint32_t F[12];                                          // row minima, rows 0..11 of the 192 keys (wave-uniform)
#pragma unroll
            for (int R = 0; R < 4; ++R) {
                F[R] = (uint32_t)__builtin_amdgcn_readlane((int)P0, 16 * R + 15);
                F[4 + R] = (uint32_t)__builtin_amdgcn_readlane((int)P1, 16 * R + 15);
                F[8 + R] = (uint32_t)__builtin_amdgcn_readlane((int)P2, 16 * R + 15);
            }
            const unsigned rowi = lane >> 4;
            const bool two = (lane & 15u) >= 3;                      // (p+45) lies three rows after p's row: two whole rows between
            uint32_t mkh[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t g1a = F[4 * h + 1], g1b = F[4 * h + 2], g1c = F[4 * h + 3], g1d = F[4 * h + 4];
                const uint32_t g2a = min(g1a, F[4 * h + 2]), g2b = min(g1b, F[4 * h + 3]), g2c = min(g1c, F[4 * h + 4]), g2d = min(g1d, F[4 * h + 5]);
                const uint32_t one_row = rowi == 0 ? g1a : rowi == 1 ? g1b : rowi == 2 ? g1c : g1d;
                const uint32_t two_rows = rowi == 0 ? g2a : rowi == 1 ? g2b : rowi == 2 ? g2c : g2d;
                const uint32_t pend = h ? lane_shift(P1, P2, lane, WIN - 1) : lane_shift(P0, P1, lane, WIN - 1);
                mkh[h] = min(min(h ? S1 : S0, pend), two ? two_rows : one_row);
            }
            const uint32_t mk0 = mkh[0], mk1 = mkh[1];
            // ---- two half-passes of 64 k-mer positions.  All global traffic of both halves (slot
            //      reservation, bucket base) is issued before any of it is consumed, so a read pays
            //      one atomic round trip, not two. ----
            unsigned nkh[2] = {0, 0}; uint32_t bkh[2] = {0, 0}; bool sth[2] = {false, false};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned cc0 = c0 + 64 * h;
                const unsigned p = cc0 + lane;
                const bool valid = p < nk_total;
                const uint32_t bkt = valid ? bucket_of(h ? mk1 : mk0, nb) : 0xFFFFFFFFu;
                const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bkt, 0x138, 0xF, 0xF, false);   // wave_shr:1 (lane 0 unused)
                bool start = valid && (lane == 0 || prev != bkt);
                unsigned long long smask = __ballot(start);
                unsigned nvalid = cc0 < nk_total ? nk_total - cc0 : 0; if (nvalid > 64) nvalid = 64;
                // a record holds at most 63 k-mers (32 B): a half-pass that is ONE run of 64 is cut before its last k-mer
                if (REC_MAXK < 64 && smask == 1ull && nvalid == 64) { start |= lane == 63; smask |= 1ull << 63; }
                unsigned long long rest = lane < 63 ? (smask >> (lane + 1)) : 0ull;
                unsigned nxt = rest ? lane + 1 + __builtin_ctzll(rest) : nvalid;
                // multi-pass counting (MapReduceEngine.h:288-291): records of buckets outside this pass's range are dropped here and
                // cut again in their own pass; bucket numbers are relative to the range
                const bool mine = bkt - pb_lo < pb_hi - pb_lo;
                sth[h] = start && mine; bkh[h] = bkt - pb_lo; nkh[h] = start ? nxt - lane : 0;
            }
            unsigned cnt = 0;
            const uint64_t slot0 = (pass_off[r] + c0 / 128) * spp;
            // the histogram atomic RETURNS the record's rank inside its bucket: it travels in the descriptor (16 bits; the rare
            // bucket that gets more than 65535 records from these reads sends the surplus through the overflow list), so the
            // scatter pass needs no atomic of its own.  Both halves' atomics are in flight before either result is used.
            uint32_t rk[2] = {0, 0};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (sth[h]) {
                    rk[h] = atomicAdd(&bcount[bkh[h]], 1u);
                    if (part_kmers) {                                        // bucket / nbl_part by reciprocal (+1 correction)
                        uint32_t pt = nbl_part > 1 ? __umulhi(bkh[h], inv_nbl) : bkh[h];
                        if ((pt + 1) * nbl_part <= bkh[h]) ++pt;
                        atomicAdd(&spart_[wv_][pt & 63], nkh[h]);
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned long long m = __ballot(sth[h]);
                if (sth[h]) {
                    const unsigned p = c0 + 64 * h + lane, nk = nkh[h];
                    const uint32_t meta = p | ((nk - 1) << 16) | (p > 0 ? 1u << 22 : 0u) | ((p + nk - 1) < (nk_total - 1) ? 1u << 23 : 0u);
                    const unsigned j = cnt + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1));
                    if (j < spp && rk[h] < 65536u) dbuf[j] = make_uint2(bkh[h] | (rk[h] << 24), meta | ((rk[h] >> 8) << 24));
                    else {
                        if (j < spp) dbuf[j] = make_uint2(0u, NONE32);
                        const unsigned long long o = atomicAdd(ov_cursor, 1ull);
                        if (o < ov_cap) { o_read[o] = (uint32_t)r; o_bkt[o] = bkh[h]; o_meta[o] = meta; o_rank[o] = rk[h]; }
                    }
                }
                cnt += (unsigned)__builtin_popcountll(m);
            }
            // the pass's slots as whole, coalesced 8-B stores (unused ones marked empty)
            wave_lds_fence();
            for (unsigned i = lane; i < spp; i += 64) s_desc[slot0 + i] = i < cnt ? dbuf[i] : make_uint2(0u, NONE32);
            wave_lds_fence();
        }
    }
    if (part_kmers) {
        wave_lds_fence();
        const uint32_t v = spart_[wv_][lane];
        // 64 copies of the 64 totals: millions of waves adding to ONE address would serialise at ~11 ns each
        if (v) atomicAdd(&part_kmers[(blockIdx.x & 63u) * 64u + lane], (unsigned long long)v);
    }
}


// ------------------------------------------------------------------------------- K1, one LANE per read (round 4)
// The wavefront-per-read kernel above spends ~300 VALU instructions of a whole wavefront on the 136 m-mers of a PE150 read (cross-lane
// scans for the window minimum, wave-wide control flow per record) -- measured in round 4: with its atomics AND its descriptor stores
// removed it still takes 19.2 of its 22.9 ms (profiles/r04_k1_diag.txt), it is bound by its own instruction stream.  Here a lane walks
// ITS read base by base: the forward and the reverse-complement 15-mer roll (five operations), the sliding-window minimum over 46 keys is
// the block decomposition of van Herk / Gil-Werman with blocks of 16 keys held in registers -- a window is the suffix of its first block,
// one or two whole blocks and the running prefix of the current one: one v_min3 per position --, and a run of equal buckets ends with ~10 instructions of the few
// lanes it concerns.  Descriptors (bucket, meta) are staged in LDS at the lane's S slots; when the 64 reads are done the wave turns the
// staged descriptors into final ones 64 at a time -- the histogram atomic returns the rank -- and stores them coalesced: the 64 reads'
// slots are one contiguous piece of s_desc.  Runs are cut at bucket changes and when a record is full (REC_MAXK = 63 k-mers);
// the kernel above also cuts at every multiple of 64 (its half-passes).
// SLABS (NOTES.md section 19): every bucket owns records [b * C, (b + 1) * C) of `recs`, so the rank the histogram atomic returns IS the
// record's place: the tail builds the 32-B record itself (rec_build, K2's code; the wave's reads are 2.4 KB it loaded a moment ago) and
// stores it as K2 does -- through LDS, two lanes per record, 16 B each -- and no descriptor is written.  Ranks >= C go to the overflow list
// like a read's records beyond its S slots; K2's list branch places both.  The LDS it needs is the part of the staging area whose
// descriptors the lanes hold in registers by then.
template <unsigned SMAX, bool ALIGN64, bool SLABS = false, unsigned MINW = 4>
__global__ void __launch_bounds__(256, MINW) k_superkmers_lane(uint64_t n, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ boff,
                                                            const uint16_t* __restrict__ good, uint32_t nb, uint32_t pb_lo, uint32_t pb_hi,
                                                            uint32_t* __restrict__ bcount, uint32_t nbl_part, uint32_t inv_nbl,
                                                            unsigned long long* __restrict__ part_kmers, uint2* __restrict__ s_desc, uint32_t S,
                                                            uint32_t* __restrict__ o_read, uint32_t* __restrict__ o_bkt, uint32_t* __restrict__ o_meta,
                                                            uint32_t* __restrict__ o_rank, uint64_t ov_cap, unsigned long long* __restrict__ ov_cursor,
                                                            uint32_t* __restrict__ recs, uint32_t slab_cap, uint64_t bases_bytes) {
    __shared__ __attribute__((aligned(16))) uint2 stage_[4][64 * SMAX];
    __shared__ uint32_t spart_[4][64];
    const unsigned lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wv_) * 64;
    if (r0 >= n) return;                                     // (the whole wavefront; the kernel has no block barrier)
    uint2* stage = stage_[wv_];
    if (part_kmers) spart_[wv_][lane] = 0;
    for (unsigned u = 0; u < S; ++u) stage[lane + 64 * u] = make_uint2(0u, NONE32);
    wave_lds_fence();
    constexpr uint32_t INF = 0xFFFFFFFFu;
    const uint64_t r = r0 + lane;
    unsigned gl = r < n ? good[r] : 0;
    if (gl <= K) gl = 0;                                     // strict, BuildReadQGraph.cc:1064
    const unsigned nk = gl ? gl - (K - 1) : 0;
    unsigned maxgl = gl;
#pragma unroll
    for (int d = 32; d; d >>= 1) maxgl = max(maxgl, (unsigned)__shfl_xor((int)maxgl, d));
    maxgl = (unsigned)__builtin_amdgcn_readfirstlane((int)maxgl);
    if (maxgl) {
        // the read as ALIGNED dwords (an aligned word that holds a valid byte never leaves the allocation), sixteen bases per refill, one
        // refill ahead; words past the read's last one are not loaded (the last one again: bases past the good length are never used)
        const uint64_t off = gl ? boff[r] : 0;
        const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(bases) + off) & 3);
        const unsigned sb8 = 8u * mis;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(bases + ((int64_t)off - (int64_t)mis));
        const unsigned ulast = gl ? (mis + ((gl + 3) >> 2) - 1) >> 2 : 0;
        uint32_t dA, dB, W; unsigned un = 3;
        { const uint32_t d0 = q[0]; dA = q[min(1u, ulast)]; dB = q[min(2u, ulast)]; W = __funnelshift_r(d0, dA, sb8); }
        uint32_t f = 0, rc = 0;
        auto roll = [&]() {                                  // takes the next base into the two 15-mers
            const uint32_t b = W & 3u; W >>= 2;
            f = (f >> 2) | (b << 28);
            rc = ((rc << 2) & 0x3FFFFFFFu) | (b ^ 3u);
        };
#pragma unroll
        for (unsigned s = 0; s < MMER - 1; ++s) roll();
        // Sliding-window minimum over WIN = 46 keys, blocks of 16 m-mers: at m-mer 16c + i the window of k-mer 16c + i - 45 is the suffix of
        // block c-3 from i+3, the blocks c-2 and c-1 and the prefix of block c (i <= 12), or the suffix of block c-2 from i-13, block c-1
        // and the prefix of block c (i >= 13): one v_min3 per position.  X3, X2, X1: suffix minima of the three blocks before the current one.
        uint32_t X3[16], X2[16], X1[16], C[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) { X3[t] = INF; X2[t] = INF; X1[t] = INF; C[t] = INF; }
        uint32_t cur = 0;
        unsigned p0 = 0, jrec = 0;
        // one block of 16 m-mers from m-mer jb on (base jb + 14 + i is taken at step i: the refill of sixteen bases falls on step 2 of every
        // block).  FIRST: its first step that has a k-mer position -- blocks 0 and 1 have none, block 2 has k-mer 0 at step 13.  Steps past
        // the longest read of the wave do nothing (no key, no k-mer), so the block needs no guard -- a guard makes every array a phi of
        // the branch and costs a register move per element and step.
        auto block = [&](auto first, unsigned jb) {
            constexpr int FIRST = decltype(first)::value;
            // stage 1, branch-free: the sixteen keys of the block and the buckets of its k-mer positions -- sixteen independent chains
            // (three multiplications each) in one basic block, so that a wavefront alone keeps its SIMD issuing
            uint32_t pref = INF;
            const uint32_t w21 = min(X2[0], X1[0]);
            uint32_t bk[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const unsigned s = jb + (MMER - 1) + i;      // base taken in this step; m-mer s-14 is complete, k-mer s-59 gets its window
                if (i == 2) { W = __funnelshift_r(dA, dB, sb8); dA = dB; dB = q[min(un, ulast)]; ++un; }
                roll();
                const uint32_t key = s < gl ? mmer_key(f < rc ? f : rc) : INF;
                C[i] = key; pref = min(pref, key);
                bk[i] = 0;
                if (i >= FIRST) {
                    const uint32_t mk = i <= 12 ? min(min(X3[i <= 12 ? i + 3 : 0], w21), pref) : min(min(X2[i >= 13 ? i - 13 : 0], X1[0]), pref);
                    bk[i] = bucket_of(mk, nb);
                }
            }
            // stage 2: where runs end (the few lanes it concerns; nearly every step has some)
#pragma unroll
            for (int i = FIRST; i < 16; ++i) {
                const unsigned p = jb + i - (WIN - 1);       // (= s - 59)
                const bool isk = p < nk;
                const uint32_t bkt = bk[i];
                // a run ends where the bucket changes and when the record is full (ALIGN64: at every multiple of 64 instead, the cuts
                // of the wavefront-per-read kernel -- 17 % more records; the parity test of the two kernels asks for it)
                const bool brk = isk && (!p || bkt != cur || (ALIGN64 ? !(p & 63u) || (REC_MAXK < 64 && p - p0 == REC_MAXK) : p - p0 == REC_MAXK));
                if ((brk && p) || (p == nk && nk)) {                                  // the run [p0, p) ends here
                    const uint32_t rb = cur - pb_lo;
                    if (rb < pb_hi - pb_lo) {                // multi-pass counting: other ranges' records are cut again in their own pass
                        const uint32_t meta = p0 | ((p - p0 - 1) << 16) | (p0 ? 1u << 22 : 0u) | (isk ? 1u << 23 : 0u);
                        if (jrec < S) stage[lane * S + jrec] = make_uint2(rb, meta);
                        else {                               // more records than slots: the overflow list, with its rank
                            const uint32_t rk = atomicAdd(&bcount[rb], 1u);
                            if (part_kmers) {
                                uint32_t pt = nbl_part > 1 ? __umulhi(rb, inv_nbl) : rb;
                                if ((pt + 1) * nbl_part <= rb) ++pt;
                                atomicAdd(&spart_[wv_][pt & 63], p - p0);
                            }
                            const unsigned long long o = atomicAdd(ov_cursor, 1ull);
                            if (o < ov_cap) { o_read[o] = (uint32_t)r; o_bkt[o] = rb; o_meta[o] = meta; o_rank[o] = rk; }
                        }
                        ++jrec;
                    }
                }
                if (brk) { p0 = p; cur = bkt; }
            }
#pragma unroll
            for (int t = 14; t >= 0; --t) C[t] = min(C[t], C[t + 1]);                     // suffix minima of the block just filled
#pragma unroll
            for (int t = 0; t < 16; ++t) { X3[t] = X2[t]; X2[t] = X1[t]; X1[t] = C[t]; }
        };
        block(std::integral_constant<int, 16>{}, 0);
        block(std::integral_constant<int, 16>{}, 16);
        block(std::integral_constant<int, 13>{}, 32);
        for (unsigned jb = 48; jb + (MMER - 1) <= maxgl; jb += 16) block(std::integral_constant<int, 0>{}, jb);
    }
    wave_lds_fence();
    // ---- staged descriptors -> final ones, 64 at a time in slot order (conflict-free LDS reads, coalesced stores): the histogram atomic
    //      RETURNS the record's rank inside its bucket (16 bits in the descriptor; beyond that the overflow list); eight atomics are in
    //      flight per lane before the first result is used
    const uint64_t nflat = (uint64_t)((n - r0 < 64 ? n - r0 : 64)) * S;
    for (unsigned u0 = 0; u0 < S; u0 += 8) {
        uint2 d[8]; uint32_t rk[8];
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const unsigned i = lane + 64 * (u0 + k);
            d[k] = u0 + k < S ? stage[i] : make_uint2(0u, NONE32);
            rk[k] = 0;
            if (d[k].y != NONE32) {
                rk[k] = atomicAdd(&bcount[d[k].x], 1u);
                if (part_kmers) {                            // bucket / nbl_part by reciprocal (+1 correction)
                    uint32_t pt = nbl_part > 1 ? __umulhi(d[k].x, inv_nbl) : d[k].x;
                    if ((pt + 1) * nbl_part <= d[k].x) ++pt;
                    atomicAdd(&spart_[wv_][pt & 63], ((d[k].y >> 16) & 63u) + 1u);
                }
            }
        }
        if constexpr (SLABS && REC_DWORDS == 8) {
            // the 512 staged descriptors of this group are in registers: their 4 KB hold the 64 records of a round (2 KB) and their places
            static_assert(SMAX >= 8, "a group of eight slots per lane is the tail's record buffer");
            uint4* s_rec = reinterpret_cast<uint4*>(stage + 64 * u0);                       // [128]
            uint64_t* s_dst = reinterpret_cast<uint64_t*>(stage + 64 * u0 + 256);           // [64]
#pragma unroll 1
            for (unsigned k = 0; k < 8 && u0 + k < S; ++k) {                                 // (one copy of the builder: d[] and rk[] rotate through element 0)
                const unsigned i = lane + 64 * (u0 + k);
                const uint2 dk = d[0]; const uint32_t rkk = rk[0];
#pragma unroll
                for (unsigned t = 0; t < 7; ++t) { d[t] = d[t + 1]; rk[t] = rk[t + 1]; }
                uint64_t dst = ~0ull;
                uint32_t out[REC_DWORDS] = {};
                const uint32_t rd = (uint32_t)(r0 + i / S);
                const bool listed = dk.y != NONE32 && rkk >= slab_cap;
                if (dk.y != NONE32 && !listed) {
                    rec_build(bases, bases_bytes, boff[rd], dk.y, out);
                    dst = slab_place(dk.x, rkk, slab_cap, 0, 0) * REC_DWORDS;
                }
                // beyond the slab: the list, its cursor taken ONCE for the wave's lanes (every wave's atomics on that one word queue up behind each other)
                const unsigned long long lm = __ballot(listed);
                if (lm) {
                    unsigned long long o0 = 0;
                    if (lane == (unsigned)__ffsll((long long)lm) - 1u) o0 = atomicAdd(ov_cursor, (unsigned long long)__popcll(lm));
                    o0 = ((unsigned long long)(unsigned)__shfl((int)(o0 >> 32), __ffsll((long long)lm) - 1) << 32) | (unsigned)__shfl((int)o0, __ffsll((long long)lm) - 1);
                    const unsigned long long o = o0 + __popcll(lm & ((1ull << lane) - 1ull));
                    if (listed && o < ov_cap) { o_read[o] = rd; o_bkt[o] = dk.x; o_meta[o] = dk.y; o_rank[o] = rkk; }
                }
                wave_lds_fence();                                                            // (the round before has left the buffer)
                s_rec[2 * lane] = make_uint4(out[0], out[1], out[2], out[3]);
                s_rec[2 * lane + 1] = make_uint4(out[4], out[5], out[6], out[7]);
                s_dst[lane] = dst;
                wave_lds_fence();
#pragma unroll
                for (unsigned j = 0; j < 2; ++j) {
                    const unsigned idx = j * 64 + lane;
                    const uint64_t t = s_dst[idx >> 1];
                    if (t != ~0ull) reinterpret_cast<uint4*>(recs + t)[idx & 1u] = s_rec[idx];
                }
            }
            wave_lds_fence();
            continue;
        }
#pragma unroll
        for (unsigned k = 0; k < 8; ++k) {
            const unsigned i = lane + 64 * (u0 + k);
            if (u0 + k < S && i < nflat) {
                uint2 out = make_uint2(0u, NONE32);
                if (d[k].y != NONE32) {
                    if (rk[k] < 65536u) out = make_uint2(d[k].x | (rk[k] << 24), d[k].y | ((rk[k] >> 8) << 24));
                    else {
                        const unsigned long long o = atomicAdd(ov_cursor, 1ull);
                        if (o < ov_cap) { o_read[o] = (uint32_t)(r0 + i / S); o_bkt[o] = d[k].x; o_meta[o] = d[k].y; o_rank[o] = rk[k]; }
                    }
                }
                s_desc[r0 * S + i] = out;
            }
        }
    }
    if (part_kmers) {
        wave_lds_fence();
        const uint32_t v = spart_[wv_][lane];
        if (v) atomicAdd(&part_kmers[(blockIdx.x & 63u) * 64u + lane], (unsigned long long)v);
    }
}

// =============================================================================== K2
// One thread per descriptor slot (then per overflow entry): the record's place is its bucket's base + the rank K1's
// histogram atomic returned; cut the 2*(nk+61) stream bits [left flank][k-mers' bases][right flank] out of the read
// (unaligned 8-byte loads), store the 32-B record.  No atomics.
// (PASS_OFF: the wavefront kernel's layout, spp slots per pass a read has -- slots_per_read is spp, pass_off[nreads + 1] the reads' first passes)
// (its binary search costs ~log2(nreads) dependent loads per slot; it runs only where the longest read passes 315 bases or W2RAP_K1=wave,
// never on the PE150 lane route, and its cost on long-read inputs has not been measured)
template <bool PASS_OFF>
__global__ void __launch_bounds__(256) k_scatter_records(uint64_t nslots, uint32_t slots_per_read, const uint64_t* __restrict__ pass_off, uint64_t nreads,
                                                          const uint2* __restrict__ s_desc,
                                                          uint64_t nov, const uint32_t* __restrict__ o_read,
                                                          const uint32_t* __restrict__ o_bkt, const uint32_t* __restrict__ o_meta,
                                                          const uint32_t* __restrict__ o_rank,
                                                          const uint8_t* __restrict__ bases,
                                                          const uint64_t* __restrict__ boff, uint64_t bases_bytes,
                                                          const uint64_t* __restrict__ bbase,
                                                          uint32_t* __restrict__ recs, uint32_t slab_cap, uint64_t slab_nb) {
    // A wavefront's 64 records leave through LDS: built one per lane, stored REC_DWORDS lanes per record, so that every store
    // instruction carries eight whole 32-B records (seven of 36 B in a W2RAP_REC36 build) as contiguous bursts instead of 64 scattered dwords.
    __shared__ __attribute__((aligned(16))) uint32_t s_rec[4][64 * REC_DWORDS];
    __shared__ uint64_t s_dst[4][64];
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r = 0, b = 0, meta = NONE32, slot = 0;
    if (i < nslots) {
        const uint2 d = s_desc[i];
        if (d.y != NONE32) { meta = d.y & 0xFFFFFFu; b = d.x & 0xFFFFFFu; slot = (d.x >> 24) | ((d.y >> 24) << 8); }
        if (PASS_OFF) {                                          // the read whose passes hold pass i / spp: pass_off[lo] <= pass < pass_off[hi]
            const uint64_t ps = i / slots_per_read;
            uint64_t lo = 0, hi = nreads;
            while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (pass_off[mid] <= ps) lo = mid; else hi = mid; }
            r = (uint32_t)lo;
        } else r = (uint32_t)(i / slots_per_read);
    } else if (i - nslots < nov) { r = o_read[i - nslots]; b = o_bkt[i - nslots]; meta = o_meta[i - nslots]; slot = o_rank[i - nslots]; }
    const bool valid = meta != NONE32;
    uint64_t dst = ~0ull;
    uint32_t out[REC_DWORDS] = {};
    if (valid) {
        // (slab route, nslots == 0: the listed records only -- into the bucket's slab, or beyond it into the overflow segment, bbase its scan)
        const uint64_t place = slab_cap ? slab_place(b, slot, slab_cap, slab_nb, slot < slab_cap ? 0 : bbase[b]) : bbase[b] + slot;
        rec_build(bases, bases_bytes, boff[r], meta, out);
        dst = place * REC_DWORDS;
    }
    if constexpr (REC_DWORDS == 8) {
        reinterpret_cast<uint4*>(s_rec[wv])[2 * lane] = make_uint4(out[0], out[1], out[2], out[3]);
        reinterpret_cast<uint4*>(s_rec[wv])[2 * lane + 1] = make_uint4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (unsigned j = 0; j < REC_DWORDS; ++j) s_rec[wv][lane * REC_DWORDS + j] = out[j];
    }
    s_dst[wv][lane] = dst;
    wave_lds_fence();
    if constexpr (REC_DWORDS == 8) {                               // 32-B records, 32-B aligned: two lanes per record, 16 B each
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            const unsigned idx = j * 64 + lane, rec = idx >> 1;
            const uint64_t d = s_dst[wv][rec];
            if (d != ~0ull) reinterpret_cast<uint4*>(recs + d)[idx & 1u] = reinterpret_cast<const uint4*>(s_rec[wv])[idx];
        }
    } else {
#pragma unroll
        for (unsigned j = 0; j < REC_DWORDS; ++j) {
            const unsigned idx = j * 64 + lane, rec = idx / REC_DWORDS, qd = idx - rec * REC_DWORDS;
            const uint64_t d = s_dst[wv][rec];
            if (d != ~0ull) recs[d + qd] = s_rec[wv][idx];
        }
    }
}

static uint32_t k1_chunk_reads() {                      // consecutive reads per wavefront of K1
    const char* v = getenv("W2RAP_K1_CHUNK");
    const int x = v ? atoi(v) : 16;
    return x > 0 ? (uint32_t)x : 16;
}

// K1 on reads [0, nr) of (boff, good): the lane-per-read kernel when a read's slots fit its LDS staging (spp * npass <= 16: reads up to
// ~315 good bases at the default 8 slots per pass), the wavefront-per-read kernel otherwise or with W2RAP_K1=wave
// (W2RAP_K1_MINW: 6 or 7 waves per SIMD instead of 8 for the latter -- 80 / 72 VGPRs, no spills -- an A/B knob)
static bool k1_wave(uint32_t spp, uint32_t npass) {
    const char* k1v = getenv("W2RAP_K1");
    return (k1v && !strcmp(k1v, "wave")) || spp * npass > 16;
}
// descriptor slots per pass of 128 k-mer positions (W2RAP_SPP, default 8) and passes of the longest read: the one place they are derived
static void k1_slots(const Ctx& c, uint32_t* spp, uint32_t* npass) {
    const char* sv = getenv("W2RAP_SPP");
    *spp = sv ? (uint32_t)atoi(sv) : 8;
    *npass = c.max_len > K + 127 ? (c.max_len - (K - 1) + 127) / 128 : 1;
}

__global__ void __launch_bounds__(256) k_k1_passes(uint64_t n, const uint16_t* __restrict__ good, uint32_t* __restrict__ np) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t g = good[r];
    np[r] = g > K ? (g - (K - 1) + 127) / 128 : 0;
}

// The wavefront kernel's descriptor slots: spp per pass of 128 k-mer positions that read r HAS, from slot pass_off[r] * spp on -- sized by
// the reads' own lengths, not n times the longest read's passes (one read of 65,535 bases among 600 k PE150 reads: 20 GB of slots).
// pass_off: [nr + 1] (the caller's); *total: the passes of all nr reads.
static int k1_pass_offsets(Ctx& c, uint64_t nr, const uint16_t* good, uint64_t* pass_off, uint64_t* total) {
    *total = 0;
    if (!nr) return 0;
    uint32_t* np = nullptr;
    W2_ALLOC(np, uint32_t, nr);
    LAUNCH(c, "k_k1_passes", k_k1_passes, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, nr, good, np);
    W2_HIP(hipGetLastError());
    W2_TRY(exclusive_scan_u32_to_u64(c, np, pass_off, nr));
    W2_HIP(hipMemcpyAsync(total, pass_off + nr, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    c.release(np);
    return 0;
}

// ---- the slab layout's two helpers: what every bucket holds beyond C records (its scan lays out the overflow segment), and the (start,
// count) words of a bucket's two segments for the counting kernels
__global__ void __launch_bounds__(256) k_slab_excess(uint32_t nb, const uint32_t* __restrict__ bcount, uint32_t C, uint32_t* __restrict__ excess) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) excess[b] = bcount[b] > C ? bcount[b] - C : 0u;
}
__global__ void __launch_bounds__(256) k_slab_segments(uint32_t nb, const uint32_t* __restrict__ bcount, uint32_t C, const uint64_t* __restrict__ ovbase,
                                                        uint64_t* __restrict__ seg /* [2][nb] */) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t n = bcount[b];
    seg[b] = seg_pack((uint64_t)b * C, n < C ? n : C);
    seg[(uint64_t)nb + b] = seg_pack((uint64_t)nb * C + ovbase[b], n > C ? n - C : 0u);
}
int slab_segments(Ctx& c, uint32_t nb, const uint32_t* d_counts, uint64_t* d_seg) {
    LAUNCH(c, "k_slab_segments", k_slab_segments, dim3((nb + 255) / 256), dim3(256), 0, nb, d_counts, c.slab_cap, c.d_bbase, d_seg);
    W2_HIP(hipGetLastError());
    return 0;
}

// =============================================================================== one cut attempt
namespace {
// a block of the context's pool that goes back when its owner leaves the scope, whichever way
template <class T>
struct Pooled {
    Ctx& c;
    T* p = nullptr;
    explicit Pooled(Ctx& c_) : c(c_) {}
    ~Pooled() { c.release(p); }
    Pooled(const Pooled&) = delete; Pooled& operator=(const Pooled&) = delete;
    int size(uint64_t count) { c.release(p); p = c.alloc<T>(count); return p ? 0 : W2RAP_E_HIP; }   // (a new block: the contents are not kept)
    T* take() { T* q = p; p = nullptr; return q; }                                                  // the caller's from now on
};

// The overflow list of a cut: (read, bucket, meta, rank) of every record that found no descriptor slot, no 16-bit rank or no place in its
// slab.  The cursor counts them all, stored or not, so a list that was too small tells its exact need.
struct OvList {
    Ctx& c;
    uint32_t *read = nullptr, *bkt = nullptr, *meta = nullptr, *rank = nullptr;
    unsigned long long* cursor = nullptr;                // [2]
    uint64_t cap = 0;
    explicit OvList(Ctx& c_) : c(c_) {}
    ~OvList() { drop(); c.release(cursor); }
    OvList(const OvList&) = delete; OvList& operator=(const OvList&) = delete;
    void drop() { for (uint32_t** q : {&read, &bkt, &meta, &rank}) { c.release(*q); *q = nullptr; } cap = 0; }
    int alloc(uint64_t entries) {
        drop();
        if (!cursor) W2_ALLOC(cursor, unsigned long long, 2);
        W2_ALLOC(read, uint32_t, entries); W2_ALLOC(bkt, uint32_t, entries); W2_ALLOC(meta, uint32_t, entries); W2_ALLOC(rank, uint32_t, entries);
        cap = entries;
        return 0;
    }
    int grow_to(uint64_t nov) { return alloc(nov + nov / 8 + 1024); }     // nov: the cursor of the attempt that did not fit
};

// One cut of reads [0, nr) of (boff, good): what goes in, where it goes, what came of it
struct K1Cut {
    uint64_t nr = 0;                                     // the reads (a batch: from its first read on)
    const uint64_t* boff = nullptr; const uint16_t* good = nullptr;
    uint64_t bases_bytes = 0;                            // extent of c.d_bases: the record builder reads no byte beyond it
    uint32_t pb_lo = 0, pb_hi = 0;                       // the records of buckets [pb_lo, pb_hi) of c.NB are kept, numbered from pb_lo
    uint32_t n_parts = 0;                                // multi-GPU: the owners that divide the range, and
    unsigned long long* d_part = nullptr;                // [64][64] partial sums of the k-mer instances sent to each -> c.part_kmers
    // descriptor geometry: spp slots per pass of 128 k-mer positions, npass passes of the longest read -- per read (lane kernel) or, with
    // k1_wave(spp, npass), per pass a read has, from slot pass_off[r] * spp on (k1_pass_offsets)
    uint32_t spp = 0, npass = 0;
    const uint64_t* pass_off = nullptr;
    uint2* s_desc = nullptr;                             // [nslots] (the slab route has none)
    uint64_t nslots = 0;
    OvList* ov = nullptr;
    uint32_t* bcount = nullptr;                          // [pb_hi - pb_lo] records per bucket
    uint64_t* bbase = nullptr;                           // [pb_hi - pb_lo + 1] the scan of the counts -- with excess_over: of what each bucket holds beyond it
    uint32_t excess_over = 0; uint32_t* excess = nullptr;   // ([pb_hi - pb_lo] words for it)
    uint32_t* recs = nullptr;                            // K2's target; with slab_cap the slabs, which K1 fills itself
    uint32_t slab_cap = 0;
    // <- cut_attempt
    uint64_t total = 0;                                  // bbase's last word: the records, or those beyond excess_over
    uint64_t nov = 0;                                    // listed records (the cursor)
};
}  // namespace

// K1: the lane-per-read kernel when a read's slots fit its LDS staging, the wavefront-per-read kernel otherwise (k1_wave)
static int launch_k1(Ctx& c, const K1Cut& k) {
    const bool wave = k1_wave(k.spp, k.npass);
    const OvList& o = *k.ov;
    if (getenv("W2RAP_TRACE"))                           // the route (tests assert it: a moved threshold must not go unnoticed)
        fprintf(stderr, "[w2rap] K1 route: %s, npass %u, spp %u, %llu reads, longest %u, records %s %u\n", wave ? "wave" : "lane",
                k.npass, k.spp, (unsigned long long)k.nr, c.max_len, k.slab_cap ? "to slabs of" : "by scatter pass", k.slab_cap);
    if (k.slab_cap && (wave || REC_DWORDS != 8)) { c.err = "partition: the slab route is the lane kernel's"; return W2RAP_E_STATE; }
    const uint32_t nbl_part = k.n_parts ? (k.pb_hi - k.pb_lo) / k.n_parts : 0, inv_nbl = nbl_part > 1 ? (uint32_t)((1ull << 32) / nbl_part) : 0;
#define W2_K1L(SMAX, A64, SLABS, MINW) LAUNCH(c, "k_superkmers_lane", (k_superkmers_lane<SMAX, A64, SLABS, MINW>), dim3((unsigned)((k.nr + 255) / 256)), dim3(256), 0, \
                                              k.nr, c.d_bases, k.boff, k.good, c.NB, k.pb_lo, k.pb_hi, k.bcount, nbl_part, inv_nbl, k.d_part, k.s_desc, k.spp * k.npass,       \
                                              o.read, o.bkt, o.meta, o.rank, o.cap, o.cursor, k.recs, k.slab_cap, k.bases_bytes)
    if (k.slab_cap) {
        // (eight slots per read -- PE150 -- need half the staging area, so more than four blocks fit a CU, and the tail is a chain of round
        // trips that only other waves hide: K1 14.5 / 13.6 / 11.9 ms at 4 / 5 / 6 waves per SIMD -- the last with 15 VGPRs spilled --, 16.5 at
        // 7 and 8, whose instantiations are not kept (NOTES.md section 19).  The six-wave figure rests on WHERE the allocator puts those
        // spills: two small edits of the tail moved them and lost the whole gain.  After any edit of the kernel, measure 4 / 5 / 6 again
        // (W2RAP_TEST_K1_SLAB_WAVES = 4, 5: a test hook, announced like the others))
        int waves = 6;
        if (const char* wv = getenv("W2RAP_TEST_K1_SLAB_WAVES")) { if (test_hook("W2RAP_TEST_K1_SLAB_WAVES")) waves = atoi(wv); }
        if (k.spp * k.npass > 8 || waves == 4) W2_K1L(16, false, true, 4);
        else if (waves == 5) W2_K1L(8, false, true, 5);
        else W2_K1L(8, false, true, 6);
    } else if (!wave) {
        // (four waves per SIMD: with five -- the staging area of 8 slots per read would leave room -- the scatter pass beside it loses more
        // than this kernel gains, partition 20.6 -> 23.8 ms; W2RAP_K1_ALIGN64: the cuts of the wavefront-per-read kernel, for the test that
        // compares the two)
        if (getenv("W2RAP_K1_ALIGN64")) W2_K1L(16, true, false, 4); else W2_K1L(16, false, false, 4);
    } else {
        // many more blocks than fit at once (8 resident per CU with __launch_bounds__(256, 8)): the dispatcher refills freed slots,
        // so no CU waits for a straggler block (a grid of exactly "8 per CU" ran 25 ms instead of 20 -- the occupancy API answers 7,
        // the hardware admits 6, and the surplus blocks start when the others are done)
        const uint32_t k1_chunk = k1_chunk_reads();
        const unsigned grid = (unsigned)((k.nr + 4ull * k1_chunk - 1) / (4ull * k1_chunk) + 1);
        static const int k1_minw = getenv("W2RAP_K1_MINW") ? atoi(getenv("W2RAP_K1_MINW")) : 8;
#define W2_K1W(MINW) LAUNCH(c, "k_superkmers", k_superkmers<MINW>, dim3(grid), dim3(256), 0, k.nr, k1_chunk, c.d_bases, k.boff, k.good, c.NB, k.pb_lo, k.pb_hi, k.bcount, \
                            nbl_part, inv_nbl, k.d_part, k.s_desc, k.spp, k.npass, k.pass_off, o.read, o.bkt, o.meta, o.rank, o.cap, o.cursor)
        if (k1_minw == 6) W2_K1W(6); else if (k1_minw == 7) W2_K1W(7); else W2_K1W(8);
#undef W2_K1W
    }
#undef W2_K1L
    W2_HIP(hipGetLastError());
    return 0;
}

// What every route does around the cutter: clear the counts, the cursor and the owners' sums, cut, scan the counts (or the excess) into
// k.bbase, and learn the totals with one host wait.  *fits: the list held every listed record -- if not, k.nov is its exact need (the cut
// does not depend on the list, only on spp), and what to do about it is the route's own business.
static int cut_attempt(Ctx& c, K1Cut& k, bool* fits) {
    hipStream_t st = c.stream;
    const uint32_t nbr = k.pb_hi - k.pb_lo;
    W2_HIP(hipMemsetAsync(k.bcount, 0, (size_t)nbr * 4, st));
    W2_HIP(hipMemsetAsync(k.ov->cursor, 0, 16, st));
    if (k.d_part) W2_HIP(hipMemsetAsync(k.d_part, 0, 64 * 64 * 8, st));
    if (k.nr) W2_TRY(launch_k1(c, k));
    if (k.excess_over) {
        LAUNCH(c, "k_slab_excess", k_slab_excess, dim3((nbr + 255) / 256), dim3(256), 0, nbr, k.bcount, k.excess_over, k.excess);
        W2_HIP(hipGetLastError());
    }
    W2_TRY(exclusive_scan_u32_to_u64(c, k.excess_over ? k.excess : k.bcount, k.bbase, nbr));
    unsigned long long h_ov = 0, h_part[64 * 64];
    W2_HIP(hipMemcpyAsync(&k.total, k.bbase + nbr, 8, hipMemcpyDeviceToHost, st));
    W2_HIP(hipMemcpyAsync(&h_ov, k.ov->cursor, 8, hipMemcpyDeviceToHost, st));
    if (k.d_part) W2_HIP(hipMemcpyAsync(h_part, k.d_part, sizeof(h_part), hipMemcpyDeviceToHost, st));
    W2_HIP(hipStreamSynchronize(st));
    if (k.d_part) for (unsigned g = 0; g < 64; ++g) { c.part_kmers[g] = 0; for (unsigned j = 0; j < 64; ++j) c.part_kmers[g] += h_part[j * 64 + g]; }
    k.nov = h_ov;
    *fits = k.nov <= k.ov->cap;
    return 0;
}

// K2 on stream sk: the cut's descriptor slots and its list -> k.recs at k.bbase (the slab route, no slots: the listed records only, into
// their slabs or the overflow segment)
static int launch_scatter(Ctx& c, const K1Cut& k, hipStream_t sk) {
    const bool wave = k1_wave(k.spp, k.npass);
    const OvList& o = *k.ov;
    const dim3 grid((unsigned)((k.nslots + k.nov + 255) / 256));
    const uint32_t slots_per_read = wave ? k.spp : k.npass * k.spp;
    const uint64_t nreads = wave ? k.nr : 0, slab_nb = k.slab_cap ? k.pb_hi - k.pb_lo : 0;
#define W2_K2(PASS_OFF) LAUNCH_ON(c, sk, "k_scatter_records", k_scatter_records<PASS_OFF>, grid, dim3(256), 0, k.nslots, slots_per_read, k.pass_off, nreads, k.s_desc, \
                                  k.nov, o.read, o.bkt, o.meta, o.rank, c.d_bases, k.boff, k.bases_bytes, k.bbase, k.recs, k.slab_cap, slab_nb)
    if (wave) W2_K2(true); else W2_K2(false);
#undef W2_K2
    W2_HIP(hipGetLastError());
    return 0;
}

// what every route asks and clears before it cuts; -> the extent of the packed bases
static int partition_begin(Ctx& c, uint32_t nb, uint64_t* bases_bytes) {
    if (!c.quality_done) { c.err = "partition before quality_windows"; return W2RAP_E_STATE; }
    if (c.n >= (1ull << 32)) { c.err = "more than 2^32 reads on one GPU (32-bit read ids in the record descriptors)"; return W2RAP_E_LIMIT; }
    c.NB = nb; c.slab_cap = 0;
    c.release(c.d_bcount); c.release(c.d_bbase); c.release(c.d_recs);
    c.d_bcount = nullptr; c.d_bbase = nullptr; c.d_recs = nullptr;
    *bases_bytes = 0;
    if (c.n) W2_HIP(hipMemcpy(bases_bytes, c.d_boff + c.n, 8, hipMemcpyDeviceToHost));
    return 0;
}

// =============================================================================== the scatter routes
// ---- K1/K2 in batches of reads.  K1 is bound by instruction issue, K2 by device atomics and scattered stores: batch k's records are
// scattered on the side stream while batch k+1 is being cut.  Every batch becomes one SEGMENT of records (grouped by bucket, segments back
// to back) -- the layout K3 already consumes for the records of several source ranks -- so nothing is merged: c.d_bcount is
// [n_batches][pb_hi - pb_lo], c.d_recs the segments, *n_seg the number of batches.
// Descriptor slots: spp per (read, pass of 128 k-mer positions).  A pass of a PE150 read cuts into ~4 records, 8 slots hold all but ~1 %
// of them; the surplus goes to the overflow list.  If even that list is too small the batch is cut again into a list of the exact size --
// records beyond rank 65535 of a heavy bucket do not depend on spp --, with twice the slots where it had many more entries than reads
// (128 cannot overflow; this and the later batches, earlier ones keep their slots).
// n_seg == nullptr: the multi-GPU call -- one batch, the k-mer instances per owner counted, the record buffer of the exact size and the
// scan kept as c.d_bbase (w2rap_step2_partition_range reads the owners' shares from it).
namespace {
struct Batch {                                           // what a batch's cut writes and its scatter pass reads: two of them take turns
    OvList ov;
    Pooled<uint64_t> bbase, pass_off;
    Pooled<uint2> s_desc;
    uint64_t slots = 0, pass_k = ~0ull, npass_tot = 0;   // slots allocated; (k1_wave) the batch whose passes pass_off holds, and their number
    explicit Batch(Ctx& c) : ov(c), bbase(c), pass_off(c), s_desc(c) {}
};
struct ScatterEvents {                                   // one per batch, behind its scatter pass; waited for before anything it reads goes back
    hipEvent_t e[16] = {};
    ~ScatterEvents() { for (hipEvent_t x : e) if (x) { (void)hipEventSynchronize(x); (void)hipEventDestroy(x); } }
};
}  // namespace

static int partition_by_scatter(Ctx& c, uint32_t nb, uint32_t pb_lo, uint32_t pb_hi, unsigned n_batches, uint32_t n_parts, unsigned* n_seg) {
    const uint32_t nbl = pb_hi - pb_lo;                  // buckets of this pass
    uint64_t bases_bytes = 0;
    W2_TRY(partition_begin(c, nb, &bases_bytes));
    if (n_parts > 64 || (n_parts && nbl % n_parts)) { c.err = "partition: at most 64 parts, dividing the bucket count"; return W2RAP_E_LIMIT; }
    hipStream_t sk = n_batches > 1 ? c.stream2 : c.stream;           // K2's stream
    const uint64_t n = c.n;
    W2_ALLOC(c.d_bcount, uint32_t, (uint64_t)n_batches * nbl);
    Pooled<unsigned long long> d_part(c);
    if (n_parts) W2_TRY(d_part.size(64 * 64));
    // equal batches (W2RAP_LAST_BATCH < 1: a shorter last one, whose scatter pass is the one nothing hides -- measured in round 4: no difference)
    const double last_frac = getenv("W2RAP_LAST_BATCH") ? std::min(1.0, std::max(0.1, atof(getenv("W2RAP_LAST_BATCH")))) : 1.0;
    const uint64_t per_batch = n_batches > 1 ? (((uint64_t)((double)n / ((double)n_batches - 1.0 + last_frac)) + 2) & ~1ull) : ((n + 1) & ~1ull);
    Batch batch[2] = {Batch(c), Batch(c)};
    ScatterEvents ev;
    for (unsigned b = 0; b < std::min(n_batches, 2u); ++b) {
        W2_TRY(batch[b].bbase.size((uint64_t)nbl + 1));
        W2_TRY(batch[b].ov.alloc((n_seg ? per_batch : n) / 8 + 1024));
    }
    uint32_t spp, npass;
    k1_slots(c, &spp, &npass);
    uint64_t rec_cap = 0, seg_base = 0;
    for (unsigned k = 0; k < n_batches; ++k) {
        const uint64_t r0 = std::min<uint64_t>(n, k * per_batch), r1 = std::min<uint64_t>(n, r0 + per_batch), nr = r1 - r0;
        Batch& B = batch[k & 1];
        if (k >= 2) W2_HIP(hipEventSynchronize(ev.e[k - 2]));              // the scatter that read these double buffers is done
        K1Cut cut;
        cut.nr = nr; cut.boff = c.d_boff + r0; cut.good = c.d_good + r0; cut.bases_bytes = bases_bytes;
        cut.pb_lo = pb_lo; cut.pb_hi = pb_hi; cut.n_parts = n_parts; cut.d_part = d_part.p;
        cut.bcount = c.d_bcount + (uint64_t)k * nbl; cut.bbase = B.bbase.p; cut.ov = &B.ov;
        for (;;) {
            const bool wave = k1_wave(spp, npass);
            if (wave && B.pass_k != k) {
                if (!B.pass_off.p) W2_TRY(B.pass_off.size(per_batch + 1));
                W2_TRY(k1_pass_offsets(c, nr, cut.good, B.pass_off.p, &B.npass_tot));
                B.pass_k = k;
            }
            cut.spp = spp; cut.npass = npass; cut.pass_off = wave ? B.pass_off.p : nullptr;
            cut.nslots = wave ? B.npass_tot * spp : nr * npass * spp;
            if (B.slots < cut.nslots) { W2_TRY(B.s_desc.size(cut.nslots)); B.slots = cut.nslots; }
            cut.s_desc = B.s_desc.p;
            bool fits = false;
            W2_TRY(cut_attempt(c, cut, &fits));
            if (fits) break;
            if (cut.nov > nr && spp < 128) spp *= 2;
            W2_TRY(B.ov.grow_to(cut.nov));
        }
        // room for this segment: the first batch predicts the total (batches are equal samples of the reads)
        if (!n_seg) W2_ALLOC(c.d_recs, uint32_t, cut.total * REC_DWORDS);
        else if (seg_base + cut.total > rec_cap) {
            const uint64_t want = k == 0 ? (uint64_t)((double)cut.total * ((double)n / (double)std::max<uint64_t>(nr, 1))) + cut.total / 16 + (1u << 20) : (seg_base + cut.total) * 2;
            uint32_t* bigger = c.alloc<uint32_t>(want * REC_DWORDS);
            if (!bigger) return W2RAP_E_HIP;
            if (c.d_recs) {
                W2_HIP(hipStreamSynchronize(sk));
                W2_HIP(hipMemcpyAsync(bigger, c.d_recs, seg_base * REC_BYTES, hipMemcpyDeviceToDevice, sk));
                W2_HIP(hipStreamSynchronize(sk));
                c.release(c.d_recs);
            }
            c.d_recs = bigger; rec_cap = want;
        }
        cut.recs = c.d_recs + seg_base * REC_DWORDS;
        if (cut.total) W2_TRY(launch_scatter(c, cut, sk));
        W2_HIP(hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
        W2_HIP(hipEventRecord(ev.e[k], sk));
        seg_base += cut.total;
    }
    for (unsigned k = 0; k < n_batches; ++k) W2_HIP(hipEventSynchronize(ev.e[k]));
    c.nrec = seg_base;
    if (!n_seg) c.d_bbase = batch[0].bbase.take();
    else {
        if (!c.d_recs) W2_ALLOC(c.d_recs, uint32_t, REC_DWORDS);
        *n_seg = n_batches;
    }
    return 0;
}

// ---- the multi-GPU call: the super-k-mer records of this rank's reads, grouped by bucket.  (pb_lo, pb_hi): this hash-range pass keeps the
// records of buckets [pb_lo, pb_hi) of nb only (MapReduceEngine.h:288-299); bucket numbers in the outputs are relative to pb_lo, the
// n_parts owners divide the RANGE
int count_partition(Ctx& c, uint32_t nb, uint32_t n_parts, uint32_t pb_lo, uint32_t pb_hi) {
    if (pb_hi > nb || pb_lo >= pb_hi) { c.err = "partition: bad bucket range"; return W2RAP_E_ARG; }
    return partition_by_scatter(c, nb, pb_lo, pb_hi, 1, n_parts, nullptr);
}
// ---- single GPU, the scatter pass
int count_partition_batched(Ctx& c, uint32_t nb, unsigned n_batches, unsigned* n_seg, uint32_t pb_lo, uint32_t pb_hi) {
    n_batches = std::min(std::max(n_batches, 1u), 16u);
    if (c.n < (1u << 20) || !c.stream2) n_batches = 1;
    return partition_by_scatter(c, nb, pb_lo, pb_hi, n_batches, 0, n_seg);
}

// =============================================================================== the slab route
// records per slab: the resident tile of the shipped k_count_fp shape -- the buckets that overflow are the ones it defers anyway
static constexpr uint32_t SLAB_CAP = 512;

// whether this count takes the slab route, and its C (0: the scatter pass)
uint32_t slab_route(const Ctx& c, uint32_t nb, unsigned npass_hash) {
    const char* sv = getenv("W2RAP_K1_SLABS");
    if (sv && atoi(sv) == 0) return 0;
    if (REC_DWORDS != 8 || npass_hash != 1 || !c.n || getenv("W2RAP_K1_ALIGN64")) return 0;
    uint32_t spp, npass;
    k1_slots(c, &spp, &npass);
    if (!spp || k1_wave(spp, npass)) return 0;
    uint32_t C = SLAB_CAP;
    if (const char* t = getenv("W2RAP_TEST_SLAB_CAP")) { if (test_hook("W2RAP_TEST_SLAB_CAP")) C = (uint32_t)std::max(1, atoi(t)); }
    // the slabs take no more than a quarter of the free HBM (the rule of auto_passes), and a segment word holds every record's number
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !free_b) return 0;
    const double need = (double)nb * C * REC_BYTES + (double)c.M / 15.0 * REC_BYTES * 0.25;
    if (need > (double)free_b / 4.0 || (double)nb * C + (double)c.M >= (double)(1ull << SEG_START_BITS)) return 0;
    return C;
}

// The slab route pays for every record beyond its slab: the overflow list has ONE cursor word, and its atomics queue up behind each other
// (~2 ns a listed record: 8.7 M of them -- 50 M reads of a genome with repeat families -- make K1 29 ms instead of 11.5, against 17.5 ms for
// the scatter pass; the routes break even near reads / 18 such records).  So inputs of 2^20 reads and more are asked first: the old lane
// kernel cuts the first 1/32 of the reads (0.4 ms at 50 M), and the records its buckets hold beyond C / 32, times 32, estimate the records
// beyond the slabs.  The estimate runs high by about reads / 25 -- ordinary buckets near C, whose sampled counts scatter above C / 32 --, so
// the limit is reads / 10 (SLAB_EXCESS_DIV): above it the scatter pass.  -> *est, *limit
static constexpr uint32_t SLAB_EXCESS_DIV = 10;
static constexpr uint32_t SLAB_SAMPLE = 32;
int slab_excess_estimate(Ctx& c, uint32_t nb, uint32_t C, uint64_t* est, uint64_t* limit) {
    c.NB = nb;
    K1Cut cut;
    k1_slots(c, &cut.spp, &cut.npass);
    cut.nr = c.n / SLAB_SAMPLE; cut.boff = c.d_boff; cut.good = c.d_good;
    cut.pb_hi = nb; cut.nslots = cut.nr * cut.spp * cut.npass; cut.excess_over = std::max(1u, C / SLAB_SAMPLE);
    Pooled<uint32_t> cnt(c), exc(c);
    Pooled<uint64_t> scan(c);
    Pooled<uint2> s_desc(c);
    OvList ov(c);
    W2_TRY(cnt.size(nb)); W2_TRY(exc.size(nb)); W2_TRY(scan.size((uint64_t)nb + 1)); W2_TRY(s_desc.size(cut.nslots));
    W2_TRY(ov.alloc(cut.nr / 8 + 1024));
    cut.bcount = cnt.p; cut.excess = exc.p; cut.bbase = scan.p; cut.s_desc = s_desc.p; cut.ov = &ov;
    bool fits = false;                                   // (a list too small loses entries, not counts)
    W2_TRY(cut_attempt(c, cut, &fits));
    *est = cut.total * SLAB_SAMPLE;
    *limit = c.n / SLAB_EXCESS_DIV;
    return 0;
}

// ---- K1 alone, records into bucket slabs (single GPU, one hash-range pass, lane route; NOTES.md section 19): bucket b owns records
// [b * C, (b + 1) * C) of c.d_recs -- not zeroed, the counts bound every read --, the cutter stores a record where its rank atomic says, and
// what it cannot store from its tail (a read's records beyond its staged slots, ranks >= C) goes through the overflow list: K2's list
// branch puts the former into their slabs and the latter into an overflow segment behind the slabs (c.d_bbase: the scan of the buckets'
// excess).  One launch over all reads, one host wait.  c.d_bcount: [nb]; the count reads two (start, count) segments per bucket.
// *refused: the overflow list of an input of refuse_from reads and more -- the inputs that were asked first, 2^20 reads unless a test hook
// lowers it -- was too small after all (the estimate's sample was not like the rest): nothing is kept, the caller takes the scatter pass -- a
// second cut of all reads costs more than that.  Smaller inputs are cut again into a list of the exact size.
int count_partition_slabs(Ctx& c, uint32_t nb, uint32_t C, uint64_t refuse_from, bool* refused) {
    *refused = false;
    K1Cut cut;
    W2_TRY(partition_begin(c, nb, &cut.bases_bytes));
    const uint64_t n = c.n;
    W2_ALLOC(c.d_bcount, uint32_t, nb);
    W2_ALLOC(c.d_bbase, uint64_t, (uint64_t)nb + 1);
    Pooled<uint32_t> excess(c);
    OvList ov(c);
    W2_TRY(excess.size(nb));
    k1_slots(c, &cut.spp, &cut.npass);
    cut.nr = n; cut.boff = c.d_boff; cut.good = c.d_good; cut.pb_hi = nb;
    cut.bcount = c.d_bcount; cut.bbase = c.d_bbase; cut.excess = excess.p; cut.ov = &ov;
    cut.slab_cap = cut.excess_over = C;
    // every record of the overflow segment is a listed one: a list that held them all bounds the segment
    W2_TRY(ov.alloc(n / 8 + 1024));
    for (;;) {
        W2_ALLOC(c.d_recs, uint32_t, ((uint64_t)nb * C + ov.cap) * REC_DWORDS);
        cut.recs = c.d_recs;
        bool fits = false;
        W2_TRY(cut_attempt(c, cut, &fits));
        if (fits) break;
        c.release(c.d_recs); c.d_recs = nullptr;
        if (n >= refuse_from) { *refused = true; return 0; }
        W2_TRY(ov.grow_to(cut.nov));
    }
    if (cut.total > cut.nov) { c.err = "partition: more records beyond the slabs than the overflow list holds"; return W2RAP_E_STATE; }
    if (cut.nov) W2_TRY(launch_scatter(c, cut, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    if (getenv("W2RAP_TRACE"))
        fprintf(stderr, "[w2rap] partition slabs: %u buckets x %u records, %llu listed records, %llu beyond their slab\n", nb, C, (unsigned long long)cut.nov,
                (unsigned long long)cut.total);
    c.slab_cap = C;
    c.nrec = (uint64_t)nb * C + cut.total;               // (the extent of c.d_recs in use)
    return 0;
}

}  // namespace w2
