// step5_runs.h -- what the Step-5 files share (step5_partners.hip, step5_open.hip, step5_add.hip): the argument checks (args.h), the
// profile of the last Step-5 call, and the heads of the runs of equal keys in a sorted array, their ranks, their number.  Each file
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

}  // namespace
}  // namespace w2
