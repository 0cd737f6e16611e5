// step5_runs.h -- what the Step-5 files share (step5_partners.hip, step5_open.hip, step5_add.hip): the argument checks (args.h), the
// profile of the last Step-5 call, and the heads of the runs of equal keys in a sorted array, their ranks, their number, and the paths index (step7_fasta.hip builds it too).  Each file
// that includes it gets its own copy of the kernel.
#pragma once
#include "args.h"
#include "ctx.h"

namespace w2 {
void save_profile5(Ctx& c);             // step5_partners.hip: keeps the context's per-kernel sums for w2rap_step5_profile
namespace {

inline unsigned grid5(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }
inline unsigned bits_for(uint64_t count) {                     // bits that hold every value below `count`
    unsigned b = 1;
    while (b < 64 && (count - 1) >> b) ++b;
    return b;
}

__global__ __launch_bounds__(256) void k5_heads(uint64_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ head) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n) head[j] = j == 0 || keys[j] != keys[j - 1];
}

// head[j] = keys[j] opens a run, hpos[j] = the runs before j (hpos[n] = their number, also returned).  `name` is the profile line
int run_heads(Ctx& c, const char* name, const uint64_t* keys, uint64_t n, uint32_t** head, uint64_t** hpos, uint64_t* n_runs) {
    W2_ALLOC(*head, uint32_t, n + 1); W2_ALLOC(*hpos, uint64_t, n + 2);
    LAUNCH(c, name, k5_heads, dim3(grid5(n)), dim3(256), 0, n, keys, *head);
    W2_TRY(exclusive_scan_u32_to_u64(c, *head, *hpos, n));
    W2_HIP(hipMemcpyAsync(n_runs, *hpos + n, 8, hipMemcpyDeviceToHost, c.stream));
    W2_HIP(hipStreamSynchronize(c.stream));
    return 0;
}

// off[e] = the first j with keys[j] >> shift >= e, for e in [0, E]: the CSR offsets of a sorted key array whose edge sits above `shift`
__global__ __launch_bounds__(256) void k5o_lower_bound(uint64_t E, const uint64_t* __restrict__ keys, uint64_t n, unsigned shift, uint64_t* __restrict__ off) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > E) return;
    uint64_t lo = 0, hi = n;                                   // the answer lies in [lo, hi]
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if ((keys[mid] >> shift) < e) lo = mid + 1; else hi = mid; }
    off[e] = lo;
}

// the paths index (INDEX of step5_open.hip, the vote of step7_fasta.hip)
__global__ __launch_bounds__(256) void k5o_index_emit(uint64_t n, const uint64_t* __restrict__ poff, const int32_t* __restrict__ pe,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    for (uint64_t k = poff[r]; k < poff[r + 1]; ++k) { keys[k] = (uint32_t)pe[k]; vals[k] = (uint32_t)r; }
}

// invert(paths, index, E) (src/VecUtilities.h:693): *vals = the read of every path entry, ordered by edge, the reads of an edge in read
// order and once per occurrence (the stable sort keeps the emission order); *off[e .. e + 1] = the entries of edge e.  N = path_off[n] > 0
int paths_index(Ctx& c, const uint64_t* poff, const int32_t* pe, uint64_t n, uint64_t N, uint64_t E, uint64_t** keys, uint32_t** vals, uint64_t** off) {
    W2_ALLOC(*keys, uint64_t, N + 1); W2_ALLOC(*vals, uint32_t, N + 1); W2_ALLOC(*off, uint64_t, E + 2);
    LAUNCH(c, "k5o_index_emit", k5o_index_emit, dim3(grid5(n)), dim3(256), 0, n, poff, pe, *keys, *vals);
    W2_TRY(sort_pairs_u64(c, *keys, *vals, N, 0, (int)bits_for(E)));
    LAUNCH(c, "k5o_lower_bound", k5o_lower_bound, dim3(grid5(E + 1)), dim3(256), 0, E, (const uint64_t*)*keys, N, 0u, *off);
    return 0;
}

}  // namespace
}  // namespace w2
