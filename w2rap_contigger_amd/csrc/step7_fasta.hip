// step7_fasta.hip -- DumpLineFiles (src/paths/long/large/Lines.cc:680-798): the texts of a.lines.fasta, a.lines.efasta and a.lines.src.
//
//   host    line_shape                                   :694-707  the skip rule, the circular kinds, what every cell is (line-sized)
//   device  k7f_path_len                                 :770-775  a thread per cell: the bases of every path behind the cut
//   device  paths_index (step5_runs.h) / k7f_vote        :713-762  invert(); a wavefront per voted cell, lanes over the index entries of e and
//                                                                  of inv[e]; the cov row in LDS (VOTE_ROW paths), in global memory beyond
//   host    pick_best                                    :763-765  ReverseSortSync = std::sort on the index vector (see w2rap_step7.h)
//   device  k7f_share                                    efasta/EfastaTools.cc:44-61  a wavefront per cell of several paths, lanes over positions
//   device  k7f_cell_size / scans / k7f_pieces / k7f_line_size / scan
//                                                        the layout: a text is a row of PIECES (bases of one edge, or one repeated
//                                                        character) in one coordinate, the bodies of all printed lines end to end
//   device  k7f_write                                    efasta::Print (EfastaTools.cc:1303-1316): 16 output bytes per thread, its line and its
//                                                        piece by binary search, 2-bit bases decoded into one aligned 16-byte store
//   host    src_text                                     :786-798
// Integer arithmetic throughout; nothing on the device depends on the order in which cells, reads or pieces are processed.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include "ctx.h"
#include "step5_runs.h"
#include "../../include/w2rap_step7.h"

namespace w2 {
namespace {

constexpr unsigned VOTE_ROW = W2RAP_STEP7_VOTE_ROW, GAP_N = W2RAP_STEP7_GAP_N;
constexpr unsigned CELL_WAVES = 4;                            // cells per block of k7f_vote and k7f_share
enum : uint32_t { CF_WRITTEN = 1, CF_GAP = 2, CF_LAST = 4, CF_VOTED = 8, CF_MULTI = 16 };     // CF_LAST: the line's last cell, no cut
enum : uint32_t { LF_PRINTED = 1, LF_CIRCULAR = 2 };
constexpr uint64_t LITERAL = 1ull << 63;                      // a piece's source: LITERAL | character, or the base's place in the edge stream

#define LAUNCH_N(n, ...) do { if (n) LAUNCH(__VA_ARGS__); } while (0)

// 32 bases from base position pos of a 2-bit stream (base p at bits 2(p&3) of byte p>>2); the buffer is padded by 32 readable bytes
__device__ inline uint64_t stream64(const uint8_t* __restrict__ s, uint64_t pos) {
    const uint64_t b = pos >> 2; const unsigned sh = 2 * (unsigned)(pos & 3);
    uint64_t x = reinterpret_cast<const U64u*>(s + b)->v;
    if (sh) x = (x >> sh) | ((uint64_t)s[b + 8] << (64 - sh));
    return x;
}
__device__ inline unsigned stream1(const uint8_t* __restrict__ s, uint64_t pos) { return (s[pos >> 2] >> (2 * (pos & 3))) & 3u; }
__device__ inline uint32_t base_char(unsigned b) { return (0x54474341u >> (8 * b)) & 0xFFu; }       // "ACGT"
template <class T>
__device__ inline uint64_t upper_index(const T* __restrict__ a, uint64_t n, T x) {       // largest i in [0, n) with a[i] <= x
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t m = (lo + hi) >> 1; if (a[m] <= x) lo = m; else hi = m; }
    return lo;
}
template <class T>
__device__ inline uint64_t upper_index_in(const T* __restrict__ a, uint64_t lo, uint64_t hi, T x) {       // the same in [lo, hi), lo < hi
    while (hi - lo > 1) { const uint64_t m = (lo + hi) >> 1; if (a[m] <= x) lo = m; else hi = m; }
    return lo;
}
__host__ __device__ inline unsigned ndigits(uint64_t v) { unsigned d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

// the lines and the edges as the kernels read them
struct Lines {
    const uint64_t* line_off; const uint64_t* cell_off; const uint64_t* lpath_off; const int32_t* ledges;
    const uint8_t* bits; const uint64_t* base0; const uint32_t* elen; int32_t K;
    __device__ uint64_t n_edges(uint64_t p) const { return lpath_off[p + 1] - lpath_off[p]; }
    // the bases edge number i of a path adds to its Cat: the first edge whole, each further one from base K - 1
    __device__ uint32_t first(uint64_t i) const { return i ? (uint32_t)(K - 1) : 0u; }
    // base r of the Cat of path p (r below its length)
    __device__ unsigned base(uint64_t p, uint32_t r) const {
        for (uint64_t i = 0, n = n_edges(p); i < n; ++i) {
            const int32_t e = ledges[lpath_off[p] + i];
            const uint32_t f = first(i), cnt = elen[e] - f;
            if (r < cnt) return stream1(bits, base0[e] + f + r);
            r -= cnt;
        }
        return 0;                                              // (not reached)
    }
};

// ---- the bases of every path behind the cut (Lines.cc:770-775); lp_cell[p] = the cell of path p -------------------------------------
__global__ __launch_bounds__(256) void k7f_path_len(uint64_t NC, Lines L, const uint32_t* __restrict__ cflag, uint32_t* __restrict__ plen, uint32_t* __restrict__ lp_cell) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= NC) return;
    const uint32_t cut = cflag[c] & CF_LAST ? 0u : (uint32_t)(L.K - 1);
    for (uint64_t p = L.cell_off[c]; p < L.cell_off[c + 1]; ++p) {
        uint32_t sum = 0;                                      // (the argument checks bound a whole line below 2^31 K-mers)
        for (uint64_t i = 0, n = L.n_edges(p); i < n; ++i) sum += L.elen[L.ledges[L.lpath_off[p] + i]] - L.first(i);
        plen[p] = sum > cut ? sum - cut : 0u;                  // (a gap's empty path: 0)
        lp_cell[p] = (uint32_t)c;
    }
}

// ---- the vote (Lines.cc:713-762) ------------------------------------------------------------------------------------------------------
enum { V_ENTRIES, V_OCC, V_ONE, V_NONE, V_SEVERAL, N_VOTE_CNT };
// One wavefront per cell, CELL_WAVES cells per block; a cell that takes no vote only keeps the block's barriers company.  cov is zero
// before: a cell of up to VOTE_ROW paths counts in its LDS row and writes it out once, a wider one counts in cov itself.
__global__ __launch_bounds__(64 * CELL_WAVES) void k7f_vote(uint64_t NC, Lines L, const uint32_t* __restrict__ cflag, const int32_t* __restrict__ cell_e,
                                                             const uint64_t* __restrict__ ioff, const uint32_t* __restrict__ iread, const uint64_t* __restrict__ poff,
                                                             const int32_t* __restrict__ pe, const int32_t* __restrict__ inv, uint32_t* __restrict__ cov,
                                                             unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t row[CELL_WAVES][VOTE_ROW];
    __shared__ unsigned bsum[N_VOTE_CNT];
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (unsigned r = lane; r < VOTE_ROW; r += 64) row[w][r] = 0;
    if (threadIdx.x < N_VOTE_CNT) bsum[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * CELL_WAVES + w;
    const bool live = c < NC && (cflag[c] & CF_VOTED);         // (wave-uniform)
    uint64_t p0 = 0, np = 0;
    bool lds = false;
    if (live) {
        p0 = L.cell_off[c]; np = L.cell_off[c + 1] - p0; lds = np <= VOTE_ROW;
        const int32_t e = cell_e[c], re = inv[e];
        const uint64_t a1 = ioff[e], n1 = ioff[e + 1] - a1, a2 = ioff[re], n2 = ioff[re + 1] - a2;
        unsigned occ = 0, one = 0, none = 0, several = 0;
        for (uint64_t i = lane; i < n1 + n2; i += 64) {
            const bool rev = i >= n1;                          // the read reversed and mapped through inv
            const uint32_t rd = iread[rev ? a2 + (i - n1) : a1 + i];
            const uint64_t a = poff[rd];
            const int64_t len = (int64_t)(poff[rd + 1] - a);
            auto at = [&](int64_t m) { return rev ? inv[pe[a + (uint64_t)(len - 1 - m)]] : pe[a + (uint64_t)m]; };
            for (int64_t m = 0; m < len; ++m) {                // every occurrence, for every entry: a read through e twice counts four times
                if (at(m) != e) continue;
                ++occ;
                uint64_t matches = 0, which = 0;
                for (uint64_t r = 0; r < np; ++r) {
                    const uint64_t x0 = L.lpath_off[p0 + r], xn = L.lpath_off[p0 + r + 1] - x0;
                    bool match = true;
                    for (uint64_t s = 0; s < xn && m + 1 + (int64_t)s < len; ++s) if (at(m + 1 + (int64_t)s) != L.ledges[x0 + s]) { match = false; break; }
                    if (match) { if (!matches) which = r; ++matches; }
                }
                if (matches == 1) { ++one; if (lds) atomicAdd(&row[w][which], 1u); else atomicAdd(&cov[p0 + which], 1u); }
                else if (!matches) ++none; else ++several;
            }
        }
        if (lane == 0 && n1 + n2) atomicAdd(&cnt[V_ENTRIES], (unsigned long long)(n1 + n2));
        if (occ) atomicAdd(&bsum[V_OCC], occ);
        if (one) atomicAdd(&bsum[V_ONE], one);
        if (none) atomicAdd(&bsum[V_NONE], none);
        if (several) atomicAdd(&bsum[V_SEVERAL], several);
    }
    __syncthreads();
    if (live && lds) for (uint64_t r = lane; r < np; r += 64) cov[p0 + r] = row[w][r];
    if (threadIdx.x < N_VOTE_CNT && bsum[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)bsum[threadIdx.x]);
}

// ---- the shares (EfastaTools.cc:44-61) ----------------------------------------------------------------------------------------------
// One wavefront per written cell of two or more paths: 64 positions at a time from the left, then from the right, the first position
// at which some path ends or differs from path 0
__global__ __launch_bounds__(64 * CELL_WAVES) void k7f_share(uint64_t NC, Lines L, const uint32_t* __restrict__ cflag, const uint32_t* __restrict__ plen,
                                                              uint32_t* __restrict__ left_share, uint32_t* __restrict__ right_share) {
    const unsigned lane = threadIdx.x & 63;
    const uint64_t c = (uint64_t)blockIdx.x * CELL_WAVES + (threadIdx.x >> 6);
    if (c >= NC || (cflag[c] & (CF_WRITTEN | CF_MULTI)) != (CF_WRITTEN | CF_MULTI)) return;      // (wave-uniform)
    const uint64_t p0 = L.cell_off[c], np = L.cell_off[c + 1] - p0;
    const uint32_t len0 = plen[p0];
    uint32_t ls = len0;
    for (uint32_t b = 0; b < len0; b += 64) {
        const uint32_t r = b + lane;
        bool differ = false;
        if (r < len0) {
            const unsigned x = L.base(p0, r);
            for (uint64_t j = 1; j < np && !differ; ++j) differ = plen[p0 + j] <= r || L.base(p0 + j, r) != x;
        }
        const unsigned long long m = __ballot(differ);
        if (m) { ls = b + (uint32_t)__builtin_ctzll(m); break; }
    }
    const uint32_t lim = len0 - ls;
    uint32_t rs = lim;
    for (uint32_t b = 0; b < lim; b += 64) {
        const uint32_t r = b + lane;
        bool differ = false;
        if (r < lim) {
            const unsigned x = L.base(p0, len0 - 1 - r);
            for (uint64_t j = 1; j < np && !differ; ++j) { const uint32_t lj = plen[p0 + j]; differ = lj - ls <= r || L.base(p0 + j, lj - 1 - r) != x; }
        }
        const unsigned long long m = __ballot(differ);
        if (m) { rs = b + (uint32_t)__builtin_ctzll(m); break; }
    }
    if (lane == 0) { left_share[c] = ls; right_share[c] = rs; }
}

// ---- the layout ---------------------------------------------------------------------------------------------------------------------
// EF false: the flattened text (path best[c] of every cell); true: efasta.  A cell's pieces: a gap one (N x 100); a path one per edge;
// a cell of several paths in efasta: left share (the edges of path 0), '{', per path its middle (its edges) and ',' or '}', right share
// (the edges of path 0 again).  Pieces of no characters stay in the list.
template <bool EF>
__global__ __launch_bounds__(256) void k7f_cell_size(uint64_t NC, Lines L, const uint32_t* __restrict__ cflag, const uint32_t* __restrict__ plen, const int32_t* __restrict__ best,
                                                     const uint32_t* __restrict__ left_share, const uint32_t* __restrict__ right_share,
                                                     uint64_t* __restrict__ npieces, uint64_t* __restrict__ nbytes) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= NC) return;
    const uint32_t f = cflag[c];
    const uint64_t p0 = L.cell_off[c], np = L.cell_off[c + 1] - p0;
    uint64_t pieces = 0, bytes = 0;
    if (!(f & CF_WRITTEN)) {}
    else if (f & CF_GAP) { pieces = 1; bytes = GAP_N; }
    else if (!EF || !(f & CF_MULTI)) { const uint64_t p = p0 + (EF ? 0 : (uint64_t)best[c]); pieces = L.n_edges(p); bytes = plen[p]; }
    else {
        const uint32_t ls = left_share[c], rs = right_share[c];
        pieces = 2 * L.n_edges(p0) + np + 1; bytes = (uint64_t)ls + rs + np + 1;
        for (uint64_t r = 0; r < np; ++r) { pieces += L.n_edges(p0 + r); bytes += plen[p0 + r] - ls - rs; }
    }
    npieces[c] = pieces; nbytes[c] = bytes;
}

// bases [a, b) of the Cat of path p as one piece per edge from piece `k` on, the first character at `at` of the body coordinate
__device__ inline void emit_clipped(const Lines& L, uint64_t p, uint32_t a, uint32_t b, uint64_t k, uint64_t at, uint64_t* __restrict__ piece_off, uint64_t* __restrict__ piece_src) {
    uint32_t start = 0;
    for (uint64_t i = 0, n = L.n_edges(p); i < n; ++i) {
        const int32_t e = L.ledges[L.lpath_off[p] + i];
        const uint32_t f = L.first(i), cnt = L.elen[e] - f;
        const uint32_t lo = start > a ? start : a, hi = start + cnt < b ? start + cnt : b;
        piece_off[k + i] = at; piece_src[k + i] = L.base0[e] + f + (lo > start ? lo - start : 0);
        if (hi > lo) at += hi - lo;
        start += cnt;
    }
}
__device__ inline void emit_literal(char ch, uint64_t k, uint64_t at, uint64_t* __restrict__ piece_off, uint64_t* __restrict__ piece_src) {
    piece_off[k] = at; piece_src[k] = LITERAL | (uint8_t)ch;
}
// a thread per path of a cell; pc[c] / bo[c] = the first piece / the first character of cell c (the scans of k7f_cell_size)
template <bool EF>
__global__ __launch_bounds__(256) void k7f_pieces(uint64_t NLP, Lines L, const uint32_t* __restrict__ lp_cell, const uint32_t* __restrict__ cflag, const uint32_t* __restrict__ plen,
                                                  const int32_t* __restrict__ best, const uint32_t* __restrict__ left_share, const uint32_t* __restrict__ right_share,
                                                  const uint64_t* __restrict__ pc, const uint64_t* __restrict__ bo, uint64_t* __restrict__ piece_off, uint64_t* __restrict__ piece_src) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= NLP) return;
    const uint64_t c = lp_cell[p], p0 = L.cell_off[c], np = L.cell_off[c + 1] - p0, r = p - p0;
    const uint32_t f = cflag[c];
    if (!(f & CF_WRITTEN)) return;
    if (f & CF_GAP) { emit_literal('N', pc[c], bo[c], piece_off, piece_src); return; }
    if (!EF || !(f & CF_MULTI)) {
        if (r == (EF ? 0 : (uint64_t)best[c])) emit_clipped(L, p, 0, plen[p], pc[c], bo[c], piece_off, piece_src);
        return;
    }
    const uint32_t ls = left_share[c], rs = right_share[c];
    const uint64_t ne0 = L.n_edges(p0);
    uint64_t k = pc[c] + ne0 + 1, at = bo[c] + ls + 1;         // behind the left share and '{'
    for (uint64_t q = 0; q < r; ++q) { k += L.n_edges(p0 + q) + 1; at += plen[p0 + q] - ls - rs + 1; }
    emit_clipped(L, p, ls, plen[p] - rs, k, at, piece_off, piece_src);
    emit_literal(r + 1 < np ? ',' : '}', k + L.n_edges(p), at + (plen[p] - ls - rs), piece_off, piece_src);
    if (r == 0) {
        emit_clipped(L, p0, 0, ls, pc[c], bo[c], piece_off, piece_src);
        emit_literal('{', pc[c] + ne0, bo[c] + ls, piece_off, piece_src);
        for (uint64_t q = 0; q < np; ++q) { k += L.n_edges(p0 + q) + 1; at += plen[p0 + q] - ls - rs + 1; }
        emit_clipped(L, p0, plen[p0] - rs, plen[p0], k, at, piece_off, piece_src);
    }
}

// ">line_<l>[ circular]\n" / ">flattened_line_<l>[ circular]\n"
template <bool EF> __host__ __device__ inline unsigned header_len(uint64_t l, uint32_t lflag) { return 1 + (EF ? 0 : 10) + 5 + ndigits(l) + (lflag & LF_CIRCULAR ? 9 : 0) + 1; }
template <bool EF> __device__ inline uint32_t header_char(uint64_t l, uint32_t lflag, unsigned at) {
    const char name[] = ">flattened_line_", circ[] = " circular";
    const unsigned skip = EF ? 10 : 0, nn = 16 - skip, nd = ndigits(l);
    if (at < nn) return (uint8_t)(at ? name[at + skip] : '>');
    at -= nn;
    if (at < nd) { uint64_t v = l; for (unsigned d = nd - 1 - at; d; --d) v /= 10; return '0' + (uint32_t)(v % 10); }
    at -= nd;
    if ((lflag & LF_CIRCULAR) && at < 9) return (uint8_t)circ[at];
    return '\n';
}
// a thread per line: the characters of its body and of its text (efasta::Print: the header, rows of 80, no empty last row)
template <bool EF>
__global__ __launch_bounds__(256) void k7f_line_size(uint64_t NL, const uint64_t* __restrict__ line_off, const uint32_t* __restrict__ lflag, const uint64_t* __restrict__ bo,
                                                     uint64_t* __restrict__ lbody, uint64_t* __restrict__ lbytes) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= NL) return;
    const uint64_t body = bo[line_off[l + 1]] - bo[line_off[l]];
    lbody[l] = body;
    lbytes[l] = lflag[l] & LF_PRINTED ? header_len<EF>(l, lflag[l]) + body + (body + 79) / 80 : 0;
}

// ---- the writer -----------------------------------------------------------------------------------------------------------------------
// 16 output bytes per thread.  Its line: the last one that starts at or before its first byte (a skipped line has no bytes and is never
// that one); a body character b of line l is character bo[line_off[l]] + b of the body coordinate, its piece the last one that starts
// at or before it (piece_off[NPC] = the end).  16 bytes inside one piece -- 16 bases, or 15 and the end of a row -- are one 32-bit read of
// the edge stream: every fifth thread meets a row end, and a byte-by-byte path for those would be paid by its whole wavefront
template <bool EF>
__global__ __launch_bounds__(256) void k7f_write(uint64_t total, uint64_t NL, const uint64_t* __restrict__ ltext, const uint64_t* __restrict__ line_off, const uint32_t* __restrict__ lflag,
                                                 const uint64_t* __restrict__ bo, const uint64_t* __restrict__ pc, uint64_t NPC, const uint64_t* __restrict__ piece_off,
                                                 const uint64_t* __restrict__ piece_src, const uint8_t* __restrict__ bits, uint8_t* __restrict__ text) {
    const uint64_t t0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (t0 >= total) return;
    const unsigned nb = total - t0 < 16 ? (unsigned)(total - t0) : 16u;
    uint64_t l = upper_index(ltext, NL, t0);
    uint64_t within = t0 - ltext[l], g0 = bo[line_off[l]], body = bo[line_off[l + 1]] - g0;
    uint64_t k0 = pc[line_off[l]], k1 = pc[line_off[l + 1]];   // the line's own pieces: a handful, so that their search is a step or two
    unsigned hdr = header_len<EF>(l, lflag[l]);
    uint32_t w[4] = {0, 0, 0, 0};
    bool done = false;
    // the place in the body: row and column of Print's rows of 80 + '\n', b = the body character at or behind this byte
    uint64_t col = 0, b = 0;
    if (within >= hdr) {
        const uint64_t q = within - hdr, row = q >> 32 ? q / 81 : (uint32_t)q / 81u;      // (a 64-bit division is a long routine)
        col = q - row * 81; b = row * 80 + col;
    }
    if (nb == 16 && within >= hdr) {
        // at most one row end falls into the 16 bytes, at byte nl (16: none); the other bytes are consecutive bases
        const unsigned nl = col >= 65 ? (unsigned)(80 - col) : 16u, nbases = nl < 16 ? 15u : 16u;
        if (b + nbases <= body) {
            const uint64_t g = g0 + b, k = upper_index_in(piece_off, k0, k1, g), src = piece_src[k];
            if (!(src & LITERAL) && g + nbases <= piece_off[k + 1]) {
                const uint32_t x = (uint32_t)stream64(bits, src + (g - piece_off[k]));
#pragma unroll
                for (unsigned t = 0; t < 16; ++t) {
                    const uint32_t ch = t == nl ? (uint32_t)'\n' : base_char((x >> (2 * (t - (t > nl ? 1u : 0u)))) & 3u);
                    w[t >> 2] |= ch << (8 * (t & 3));
                }
                done = true;
            }
        }
    }
    if (!done) {                                               // headers, line ends, piece borders, literals: byte by byte
        uint64_t k = NPC;                                      // the piece of the last body character written, NPC: none yet
        for (unsigned t = 0; t < nb; ++t) {
            if (within == ltext[l + 1] - ltext[l]) {           // the next line that has bytes
                do ++l; while (ltext[l + 1] == ltext[l]);
                within = 0; g0 = bo[line_off[l]]; body = bo[line_off[l + 1]] - g0; hdr = header_len<EF>(l, lflag[l]);
                k0 = pc[line_off[l]]; k1 = pc[line_off[l + 1]];
            }
            uint32_t ch;
            if (within < hdr) { ch = header_char<EF>(l, lflag[l], (unsigned)within); col = 0; b = 0; }
            else if (col == 80) { ch = '\n'; col = 0; }
            else if (b == body) ch = '\n';                     // (the end of a last row that is not full; the line ends here)
            else {
                const uint64_t g = g0 + b;
                if (k == NPC || g < piece_off[k] || g >= piece_off[k + 1]) k = upper_index_in(piece_off, k0, k1, g);
                const uint64_t src = piece_src[k];
                ch = src & LITERAL ? (uint32_t)(src & 0xFF) : base_char(stream1(bits, src + (g - piece_off[k])));
                ++b; ++col;
            }
            w[t >> 2] |= ch << (8 * (t & 3));
            ++within;
        }
    }
    if (nb == 16) *reinterpret_cast<uint4*>(text + t0) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (unsigned t = 0; t < nb; ++t) text[t0 + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
std::string g_profile7f;
void save_profile7f(Ctx& c) { g_profile7f = profile_text(c); }

template <class T> int host_copy(Ctx& c, T** p, const T* v, uint64_t n) {
    W2_TRY(host_zeros(c, p, n));
    if (n) std::memcpy(*p, v, n * sizeof(T));
    return 0;
}

// Lines.cc:694-707 on the host: which lines are printed, which are circular, and what every cell is
struct Shape { std::vector<uint8_t> printed; std::vector<uint32_t> lflag, cflag; std::vector<int32_t> cell_e; };
void line_shape(const w2rap_step7_fasta_in& in, w2rap_step7_fasta_out& out, Shape& S) {
    const uint64_t NL = in.n_lines, NC = NL ? in.line_off[NL] : 0;
    std::vector<int32_t> vleft, vright;
    args::edge_ends(in, vleft, vright);
    S.printed.assign(NL, 0); S.lflag.assign(NL, 0); S.cflag.assign(NC, 0); S.cell_e.assign(NC, 0);
    auto first_edge = [&](uint64_t cell) { return in.line_edges[in.lpath_off[in.cell_off[cell]]]; };
    for (uint64_t l = 0; l < NL; ++l) {
        const uint64_t c0 = in.line_off[l], c1 = in.line_off[l + 1];
        const int32_t F = first_edge(c0), B = first_edge(c1 - 1);
        const bool skip = l > 0 && first_edge(in.line_off[l - 1]) == in.inv[B];
        if (skip) { ++out.n_skipped; continue; }
        const bool circular1 = c1 - c0 > 1 && F == B, circular2 = c1 - c0 == 1 && vleft[F] == vright[F];
        S.printed[l] = 1; S.lflag[l] = LF_PRINTED | (circular1 || circular2 ? LF_CIRCULAR : 0);
        ++out.n_printed; out.n_circular1 += circular1; out.n_circular2 += circular2;
        for (uint64_t cl = c0; cl < c1; ++cl) {
            if (circular1 && cl == c1 - 1) break;
            const uint64_t p0 = in.cell_off[cl], np = in.cell_off[cl + 1] - p0;
            const bool gap = np == 1 && in.lpath_off[p0 + 1] == in.lpath_off[p0], odd = (cl - c0) & 1;
            uint32_t f = CF_WRITTEN | (gap ? CF_GAP : 0) | (cl == c1 - 1 ? CF_LAST : 0) | (np > 1 ? CF_MULTI : 0);
            if (odd && !gap) { f |= CF_VOTED; S.cell_e[cl] = first_edge(cl - 1); }
            S.cflag[cl] = f;
            out.n_gap_cells += gap;
        }
    }
}

// Lines.cc:786-798
std::string src_text(const w2rap_step7_fasta_in& in) {
    std::string s;
    for (uint64_t l = 0; l < in.n_lines; ++l) {
        for (uint64_t cl = in.line_off[l]; cl < in.line_off[l + 1]; ++cl) {
            if (cl > in.line_off[l]) s += ',';
            const uint64_t p0 = in.cell_off[cl], p1 = in.cell_off[cl + 1];
            if (((cl - in.line_off[l]) & 1) == 0) { s += std::to_string(in.line_edges[in.lpath_off[p0]]); continue; }
            s += '{';
            for (uint64_t p = p0; p < p1; ++p) {
                if (p > p0) s += ',';
                s += '{';
                for (uint64_t i = in.lpath_off[p]; i < in.lpath_off[p + 1]; ++i) { if (i > in.lpath_off[p]) s += ','; s += std::to_string(in.line_edges[i]); }
                s += '}';
            }
            s += '}';
        }
        s += '\n';
    }
    return s;
}

// Lines.cc:763-765: ReverseSortSync(cov, ids); best = ids[0] -- std::sort on the index vector with cov[i] > cov[j], as WhatPermutation
// (VecUtilities.h:349-371) calls it: the tie order is the C++ library's (see w2rap_step7.h)
void pick_best(const w2rap_step7_fasta_in& in, const Shape& S, const uint32_t* cov, int32_t* best, w2rap_step7_fasta_out& out) {
    std::vector<unsigned> perm;
    for (uint64_t c = 0; c < S.cflag.size(); ++c) {
        if (!(S.cflag[c] & CF_VOTED)) continue;
        const uint64_t p0 = in.cell_off[c], np = in.cell_off[c + 1] - p0;
        const uint32_t* v = cov + p0;
        perm.resize(np);
        std::iota(perm.begin(), perm.end(), 0u);
        std::sort(perm.begin(), perm.end(), [v](size_t i, size_t j) { return v[i] > v[j]; });
        best[c] = (int32_t)perm[0];
        const uint32_t top = v[perm[0]];
        out.n_cells_tied += std::count(v, v + np, top) > 1;
        out.n_cells_wide += np > VOTE_ROW;
        ++out.n_cells_voted;
    }
}

struct Dev {
    Lines L{}; uint64_t NL = 0, NC = 0, NLP = 0;
    uint32_t *cflag = nullptr, *lflag = nullptr, *plen = nullptr, *lp_cell = nullptr, *ls = nullptr, *rs = nullptr; int32_t* best = nullptr;
};

// one text: the layout, the limit of efasta::Print, the writer, the text on the host
template <bool EF>
int write_text(Ctx& c, const Dev& d, char** text_out, uint64_t* len_out, uint64_t* n_pieces, w2rap_step7_fasta_out& out) {
    const uint64_t NL = d.NL, NC = d.NC, NLP = d.NLP;
    uint64_t *npc = nullptr, *nby = nullptr, *pc = nullptr, *bo = nullptr, *lbody = nullptr, *lbytes = nullptr, *ltext = nullptr, *piece_off = nullptr, *piece_src = nullptr;
    uint8_t* text = nullptr;
    uint64_t NPC = 0, total = 0;
    W2_ALLOC(npc, uint64_t, NC + 1); W2_ALLOC(nby, uint64_t, NC + 1); W2_ALLOC(pc, uint64_t, NC + 2); W2_ALLOC(bo, uint64_t, NC + 2);
    W2_ALLOC(lbody, uint64_t, NL + 1); W2_ALLOC(lbytes, uint64_t, NL + 1); W2_ALLOC(ltext, uint64_t, NL + 2);
    {
        Timer t(c.stream);
        LAUNCH(c, EF ? "k7f_cell_size_efasta" : "k7f_cell_size_fasta", k7f_cell_size<EF>, dim3(grid5(NC)), dim3(256), 0, NC, d.L, (const uint32_t*)d.cflag, (const uint32_t*)d.plen,
               (const int32_t*)d.best, (const uint32_t*)d.ls, (const uint32_t*)d.rs, npc, nby);
        W2_TRY(exclusive_scan_u64(c, npc, pc, NC)); W2_TRY(exclusive_scan_u64(c, nby, bo, NC));
        W2_HIP(hipMemcpyAsync(&NPC, pc + NC, 8, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        W2_ALLOC(piece_off, uint64_t, NPC + 1); W2_ALLOC(piece_src, uint64_t, NPC + 1);
        W2_HIP(hipMemcpyAsync(piece_off + NPC, bo + NC, 8, hipMemcpyDeviceToDevice, c.stream));
        LAUNCH_N(NPC, c, EF ? "k7f_pieces_efasta" : "k7f_pieces_fasta", k7f_pieces<EF>, dim3(grid5(NLP)), dim3(256), 0, NLP, d.L, (const uint32_t*)d.lp_cell, (const uint32_t*)d.cflag,
                 (const uint32_t*)d.plen, (const int32_t*)d.best, (const uint32_t*)d.ls, (const uint32_t*)d.rs, (const uint64_t*)pc, (const uint64_t*)bo, piece_off, piece_src);
        LAUNCH(c, EF ? "k7f_line_size_efasta" : "k7f_line_size_fasta", k7f_line_size<EF>, dim3(grid5(NL)), dim3(256), 0, NL, d.L.line_off, (const uint32_t*)d.lflag, (const uint64_t*)bo, lbody, lbytes);
        W2_TRY(exclusive_scan_u64(c, lbytes, ltext, NL));
        W2_HIP(hipMemcpyAsync(&total, ltext + NL, 8, hipMemcpyDeviceToHost, c.stream));
        out.ms_layout += t.stop();
    }
    std::vector<uint64_t> body(NL);
    W2_HIP(hipMemcpyAsync(body.data(), lbody, NL * 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    for (uint64_t l = 0; l < NL; ++l) if (body[l] >= (1ull << 32)) { c.err = "a line body of 2^32 characters or more"; return W2RAP_E_LIMIT; }
    W2_ALLOC(text, uint8_t, total + 32);
    {
        Timer t(c.stream);
        LAUNCH_N(total, c, EF ? "k7f_write_efasta" : "k7f_write_fasta", k7f_write<EF>, dim3(grid5((total + 15) / 16)), dim3(256), 0, total, NL, (const uint64_t*)ltext, d.L.line_off,
                 (const uint32_t*)d.lflag, (const uint64_t*)bo, (const uint64_t*)pc, NPC, (const uint64_t*)piece_off, (const uint64_t*)piece_src, d.L.bits, text);
        out.ms_write += t.stop();
    }
    uint8_t* h = nullptr;
    W2_TRY(dl(c, &h, (const uint8_t*)text, total));
    W2_HIP(hipStreamSynchronize(c.stream));
    *text_out = (char*)h; *len_out = total; *n_pieces = NPC;
    for (void* p : {(void*)npc, (void*)nby, (void*)pc, (void*)bo, (void*)lbody, (void*)lbytes, (void*)ltext, (void*)piece_off, (void*)piece_src, (void*)text}) c.release(p);
    return 0;
}

int line_files(Ctx& c, const w2rap_step7_fasta_in& in, uint32_t parts, w2rap_step7_fasta_out& out) {
    const uint64_t E = in.n_edge_objs, n = in.n_paths, npe = n ? in.path_off[n] : 0, NL = in.n_lines;
    const uint64_t NC = NL ? in.line_off[NL] : 0, NLP = NL ? in.cell_off[NC] : 0, NLE = NL ? in.lpath_off[NLP] : 0;
    static const uint64_t zero = 0;
    Shape S;
    line_shape(in, out, S);
    W2_TRY(host_copy(c, &out.printed, (const uint8_t*)S.printed.data(), NL));
    if (parts & W2RAP_STEP7_SRC) {
        const std::string s = src_text(in);
        W2_TRY(host_copy(c, &out.src, s.data(), s.size()));
        out.src_len = s.size();
    }
    const bool fasta = parts & W2RAP_STEP7_FASTA, efasta = parts & W2RAP_STEP7_EFASTA;
    if (!fasta && !efasta) return 0;
    if (!NC) {                                                 // no line: two empty texts, nothing to launch
        if (fasta) { W2_TRY(host_zeros(c, &out.fasta, 0)); W2_TRY(host_zeros(c, &out.best, 0)); W2_TRY(host_zeros(c, &out.cov, 0)); }
        if (efasta) { W2_TRY(host_zeros(c, &out.efasta, 0)); W2_TRY(host_zeros(c, &out.left_share, 0)); W2_TRY(host_zeros(c, &out.right_share, 0)); }
        return 0;
    }

    // ---- uploads: the lines, the edges as one 2-bit stream (every object starts a byte: base0 = 4 x its byte offset)
    Dev d; d.NL = NL; d.NC = NC; d.NLP = NLP;
    uint64_t *d_line_off = nullptr, *d_cell_off = nullptr, *d_lpath_off = nullptr, *d_base0 = nullptr; int32_t* d_ledges = nullptr; uint32_t* d_elen = nullptr; uint8_t* d_bits = nullptr;
    std::vector<uint64_t> base0(E);
    for (uint64_t e = 0; e < E; ++e) base0[e] = in.edge_byte_off[e] * 4;
    W2_TRY(up_pooled(c, &d_line_off, in.line_off, NL + 1)); W2_TRY(up_pooled(c, &d_cell_off, in.cell_off, NC + 1)); W2_TRY(up_pooled(c, &d_lpath_off, in.lpath_off, NLP + 1));
    W2_TRY(up_pooled(c, &d_ledges, in.line_edges, NLE)); W2_TRY(up_pooled(c, &d_elen, in.edge_len, E)); W2_TRY(up_pooled(c, &d_base0, (const uint64_t*)base0.data(), E));
    W2_TRY(up_pooled(c, &d_bits, in.edge_packed, E ? in.edge_byte_off[E] : 0, 32));
    W2_TRY(up_pooled(c, &d.cflag, (const uint32_t*)S.cflag.data(), NC)); W2_TRY(up_pooled(c, &d.lflag, (const uint32_t*)S.lflag.data(), NL));
    d.L = Lines{d_line_off, d_cell_off, d_lpath_off, d_ledges, d_bits, d_base0, d_elen, in.K};
    W2_ALLOC(d.plen, uint32_t, NLP); W2_ALLOC(d.lp_cell, uint32_t, NLP);
    W2_ALLOC(d.best, int32_t, NC); W2_ALLOC(d.ls, uint32_t, NC); W2_ALLOC(d.rs, uint32_t, NC);
    W2_HIP(hipMemsetAsync(d.best, 0, NC * 4, c.stream)); W2_HIP(hipMemsetAsync(d.ls, 0, NC * 4, c.stream)); W2_HIP(hipMemsetAsync(d.rs, 0, NC * 4, c.stream));
    LAUNCH(c, "k7f_path_len", k7f_path_len, dim3(grid5(NC)), dim3(256), 0, NC, d.L, (const uint32_t*)d.cflag, d.plen, d.lp_cell);
    W2_HIP(hipStreamSynchronize(c.stream));                    // (the host vectors above have been read)

    // ---- the vote and best (FASTA)
    if (fasta) {
        uint64_t *d_poff = nullptr, *d_keys = nullptr, *d_ioff = nullptr; int32_t *d_pe = nullptr, *d_inv = nullptr, *d_cell_e = nullptr; uint32_t *d_iread = nullptr, *d_cov = nullptr;
        unsigned long long* d_cnt = nullptr;
        W2_TRY(up_pooled(c, &d_poff, n ? in.path_off : &zero, n + 1)); W2_TRY(up_pooled(c, &d_pe, in.path_edges, npe)); W2_TRY(up_pooled(c, &d_inv, in.inv, E));
        W2_TRY(up_pooled(c, &d_cell_e, (const int32_t*)S.cell_e.data(), NC));
        W2_ALLOC(d_cov, uint32_t, NLP); W2_ALLOC(d_cnt, unsigned long long, 8);
        {
            Timer t(c.stream);
            W2_HIP(hipMemsetAsync(d_cov, 0, (NLP ? NLP : 1) * 4, c.stream)); W2_HIP(hipMemsetAsync(d_cnt, 0, 8 * 8, c.stream));
            if (npe) W2_TRY(paths_index(c, d_poff, d_pe, n, npe, E, &d_keys, &d_iread, &d_ioff));
            else { W2_ALLOC(d_ioff, uint64_t, E + 2); W2_ALLOC(d_iread, uint32_t, 1); W2_HIP(hipMemsetAsync(d_ioff, 0, (E + 2) * 8, c.stream)); }     // no path entry: every list empty
            LAUNCH(c, "k7f_vote", k7f_vote, dim3(grid5(NC, CELL_WAVES)), dim3(64 * CELL_WAVES), 0, NC, d.L, (const uint32_t*)d.cflag, (const int32_t*)d_cell_e, (const uint64_t*)d_ioff,
                   (const uint32_t*)d_iread, (const uint64_t*)d_poff, (const int32_t*)d_pe, (const int32_t*)d_inv, d_cov, d_cnt);
            out.ms_vote = t.stop();
        }
        unsigned long long cnt[N_VOTE_CNT] = {0};
        W2_TRY(dl(c, &out.cov, (const uint32_t*)d_cov, NLP));
        W2_HIP(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        out.n_entries = cnt[V_ENTRIES]; out.n_occurrences = cnt[V_OCC]; out.n_match_one = cnt[V_ONE]; out.n_match_none = cnt[V_NONE]; out.n_match_several = cnt[V_SEVERAL];
        W2_TRY(host_zeros(c, &out.best, NC));
        pick_best(in, S, out.cov, out.best, out);
        W2_HIP(hipMemcpyAsync(d.best, out.best, NC * 4, hipMemcpyHostToDevice, c.stream));
        W2_HIP(hipStreamSynchronize(c.stream));
        for (void* p : {(void*)d_poff, (void*)d_keys, (void*)d_ioff, (void*)d_pe, (void*)d_inv, (void*)d_cell_e, (void*)d_iread, (void*)d_cov, (void*)d_cnt}) c.release(p);
        W2_TRY(write_text<false>(c, d, &out.fasta, &out.fasta_len, &out.n_pieces_fasta, out));
    }

    // ---- the shares (EFASTA)
    if (efasta) {
        {
            Timer t(c.stream);
            LAUNCH(c, "k7f_share", k7f_share, dim3(grid5(NC, CELL_WAVES)), dim3(64 * CELL_WAVES), 0, NC, d.L, (const uint32_t*)d.cflag, (const uint32_t*)d.plen, d.ls, d.rs);
            out.ms_share = t.stop();
        }
        W2_TRY(dl(c, &out.left_share, (const uint32_t*)d.ls, NC)); W2_TRY(dl(c, &out.right_share, (const uint32_t*)d.rs, NC));
        W2_HIP(hipStreamSynchronize(c.stream));
        W2_TRY(write_text<true>(c, d, &out.efasta, &out.efasta_len, &out.n_pieces_efasta, out));
    }
    W2_HIP(hipStreamSynchronize(c.stream));
    for (void* p : {(void*)d_line_off, (void*)d_cell_off, (void*)d_lpath_off, (void*)d_base0, (void*)d_ledges, (void*)d_elen, (void*)d_bits, (void*)d.cflag, (void*)d.lflag, (void*)d.plen,
                    (void*)d.lp_cell, (void*)d.best, (void*)d.ls, (void*)d.rs}) c.release(p);
    return 0;
}

constexpr uint32_t ALL_PARTS = W2RAP_STEP7_FASTA | W2RAP_STEP7_EFASTA | W2RAP_STEP7_SRC;

// The argument checks: 0, or the code with the message in `err`.  Everything a kernel or the host code uses as an index is looked at here
int fasta_check(const w2rap_step7_fasta_in* in, const w2rap_step7_fasta_params* P, char* err, size_t errlen) {
    auto fail = [&](int code, const char* m) { if (err && errlen) std::snprintf(err, errlen, "%s", m); return code; };
    if (!in || !P) return fail(W2RAP_E_ARG, "null argument");
    if (P->flags & ~ALL_PARTS) return fail(W2RAP_E_ARG, "unknown flag");
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640]");
    if (args::too_large(*in, args::READS_END)) return fail(W2RAP_E_ARG, args::TOO_LARGE);
    W2_ARGS(args::null_arrays(*in, !in->inv));
    W2_ARGS(args::edge_off_start(*in));
    W2_ARGS(args::edge_lens(*in, 1ull << 31));
    W2_ARGS(args::adjacency(*in));
    W2_ARGS(args::from_v_agrees(*in));
    W2_ARGS(args::involution(*in));
    W2_ARGS(args::reads_and_paths(*in));
    W2_ARGS(args::lines(*in));
    W2_ARGS(args::line_lengths(*in));
    for (uint64_t l = 0; l < in->n_lines; ++l)
        for (uint64_t cl = in->line_off[l]; cl < in->line_off[l + 1]; ++cl) {
            const uint64_t p0 = in->cell_off[cl], np = in->cell_off[cl + 1] - p0;
            const bool even = ((cl - in->line_off[l]) & 1) == 0, last = cl + 1 == in->line_off[l + 1];
            if (even && in->lpath_off[p0 + 1] == in->lpath_off[p0]) return fail(W2RAP_E_ARG, "an even cell whose first path is empty");
            for (uint64_t p = p0; p < p0 + np; ++p) {
                const uint64_t ne = in->lpath_off[p + 1] - in->lpath_off[p];
                if (!ne) { if (np > 1) return fail(W2RAP_E_ARG, "an empty path in a cell of two or more paths"); continue; }
                uint64_t bases = 0;
                for (uint64_t i = in->lpath_off[p]; i < in->lpath_off[p + 1]; ++i) bases += in->edge_len[in->line_edges[i]] - (i > in->lpath_off[p] ? (uint64_t)in->K - 1 : 0);
                if (!last && bases < (uint64_t)in->K - 1) return fail(W2RAP_E_ARG, "a path shorter than the K-1 bases cut from it");
            }
        }
    return 0;
}

}  // namespace
}  // namespace w2

using namespace w2;

extern "C" int w2rap_step7_line_files(const w2rap_step7_fasta_in* in, const w2rap_step7_fasta_params* P, w2rap_step7_fasta_out* out, char* err, size_t errlen) {
    auto fail = [&](int code, const std::string& m) { if (err && errlen) std::snprintf(err, errlen, "%s", m.c_str()); return code; };
    if (!out) return fail(W2RAP_E_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (const int rc = fasta_check(in, P, err, errlen)) return rc;
    const uint32_t parts = P->flags ? P->flags : ALL_PARTS;
    return one_shot(P->device, err, errlen, [&](Ctx& c) { return line_files(c, *in, parts, *out); }, save_profile7f, [&] { w2rap_step7_line_files_free(out); });
}

extern "C" void w2rap_step7_line_files_free(w2rap_step7_fasta_out* o) {
    if (!o) return;
    for (void* p : {(void*)o->fasta, (void*)o->efasta, (void*)o->src, (void*)o->printed, (void*)o->best, (void*)o->cov, (void*)o->left_share, (void*)o->right_share}) std::free(p);
    std::memset(o, 0, sizeof(*o));
}

extern "C" size_t w2rap_step7_line_files_profile(char* buf, size_t len) {
    if (buf && len) std::snprintf(buf, len, "%s", g_profile7f.c_str());
    return g_profile7f.size() + 1;
}
