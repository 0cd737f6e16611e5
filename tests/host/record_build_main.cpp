// Host check of the super-k-mer record builder and the slab arithmetic of common.h (rec_build, slab_place, seg_pack), meant to be
// compiled with -fsanitize=address,undefined: every record cut out of heap buffers of EXACTLY the reads' size (the builder's loads at
// the end of the allocation must stay inside it) is compared with a base-by-base restatement of the format.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../w2rap_contigger_amd/csrc/common.h"

using namespace w2;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static unsigned base_at(const uint8_t* bases, uint64_t ro, unsigned i) { return (bases[ro + (i >> 2)] >> (2 * (i & 3))) & 3u; }

// the format, base by base: header byte, then from bit REC_HB the 2-bit stream [left flank][nk + 59 bases][right flank]
static void rec_naive(const uint8_t* bases, uint64_t ro, unsigned p, unsigned nk, bool hasL, bool hasR, uint32_t (&out)[REC_DWORDS]) {
    memset(out, 0, sizeof(out));
    auto put = [&](unsigned bit, unsigned v) { out[bit >> 5] |= v << (bit & 31); };
    out[0] = (nk - 1) | (hasL ? 64u : 0u) | (hasR ? 128u : 0u);
    if (hasL) put(REC_HB, base_at(bases, ro, p - 1));
    for (unsigned t = 0; t < nk + 59; ++t) put(REC_HB + 2 * (t + 1), base_at(bases, ro, p + t));
    if (hasR) put(REC_HB + 2 * (nk + 60), base_at(bases, ro, p + nk + 59));
}

int main() {
    static_assert(REC_DWORDS == 8, "the 32-byte record");
    unsigned long checked = 0;
    for (unsigned trial = 0; trial < 400; ++trial) {
        // a few reads of 61 .. 315 bases, packed four to a byte, each starting on a byte; the buffer ends with the last read's last byte
        const unsigned nreads = 1 + (unsigned)(rnd() % 4);
        std::vector<unsigned> len(nreads); std::vector<uint64_t> off(nreads + 1, 0);
        for (unsigned r = 0; r < nreads; ++r) { len[r] = 61 + (unsigned)(rnd() % 255); off[r + 1] = off[r] + (len[r] + 3) / 4; }
        const uint64_t bytes = off[nreads];
        uint8_t* bases = (uint8_t*)malloc(bytes);
        for (uint64_t i = 0; i < bytes; ++i) bases[i] = (uint8_t)rnd();
        for (unsigned r = 0; r < nreads; ++r) {
            const unsigned nkr = len[r] - 59;                  // k-mers of the read
            for (unsigned rep = 0; rep < 60; ++rep) {
                // a run [p, p + nk) of the read's k-mers, as the cutter describes it; now and then the read's first or last run
                unsigned p = (unsigned)(rnd() % nkr), nk = 1 + (unsigned)(rnd() % REC_MAXK);
                if (rep % 5 == 0) p = 0;
                if (p + nk > nkr) nk = nkr - p;
                if (rep % 7 == 0) { nk = nk < nkr ? nk : nkr; p = nkr - nk; }
                const bool hasL = p != 0, hasR = p + nk < nkr;
                const uint32_t meta = p | ((nk - 1) << 16) | (hasL ? 1u << 22 : 0u) | (hasR ? 1u << 23 : 0u);
                uint32_t a[REC_DWORDS], b[REC_DWORDS];
                rec_build(bases, bytes, off[r], meta, a);
                rec_naive(bases, off[r], p, nk, hasL, hasR, b);
                if (memcmp(a, b, sizeof(a))) { fprintf(stderr, "record differs: trial %u read %u p %u nk %u\n", trial, r, p, nk); return 1; }
                ++checked;
            }
        }
        free(bases);
    }
    // slabs: places inside the slab, the first place of the overflow segment, and beyond 2^32 dwords (940 k buckets x 512 records x 8)
    const uint32_t C = 512; const uint64_t nb = 940000;
    if (slab_place(0, 0, C, nb, 0) != 0 || slab_place(7, 511, C, nb, 99) != 7ull * 512 + 511) return 2;
    if (slab_place(7, 512, C, nb, 99) != nb * 512 + 99 || slab_place(939999, 20000, C, nb, 1000) != nb * 512 + 1000 + 20000 - 512) return 2;
    if (slab_place(939999, 511, C, nb, 0) * REC_DWORDS != 3850239992ull || slab_place(939999, 511, C, nb, 0) * REC_DWORDS <= (1ull << 31)) return 2;
    if (slab_place(5, 0, 1, 6, 0) != 5 || slab_place(5, 1, 1, 6, 3) != 6 + 3) return 2;
    // segment words: start and count come back; 2^26 records and more are what the counting kernels refuse
    const uint64_t starts[] = {0, 1, nb * C, (1ull << SEG_START_BITS) - 1};
    const uint64_t counts[] = {0, 1, 512, (1ull << 26) - 1, 1ull << 26, 1ull << 40};
    for (uint64_t s : starts) for (uint64_t n : counts) {
        const uint64_t w = seg_pack(s, n);
        if ((w & ((1ull << SEG_START_BITS) - 1)) != s || (w >> SEG_START_BITS) != (n < (1ull << 26) ? n : 1ull << 26)) return 3;
    }
    if (SEG_PACKED & ((1u << 24) | ((1u << 24) - 1))) return 3;      // the flag lies above every bucket count
    printf("record builder: %lu records equal the base-by-base form; slab places and segment words exact\n", checked);
    return 0;
}
