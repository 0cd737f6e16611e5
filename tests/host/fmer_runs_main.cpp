// Host figures for the absence filter's key (fmer_key, common.h) per window stride, meant to be compiled with
// -fsanitize=address,undefined: the runs of equal words along a random stream (the atomics the builder issues), the filter's efficacy
// against 31-mers with one substituted base, and the key's symmetries (reverse complement, ignored top bits).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../w2rap_contigger_amd/csrc/common.h"

using namespace w2;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

constexpr uint64_t M62 = (1ull << 62) - 1;
// reverse complement of 31 bases (base t at bits 2t+1:2t), base by base
static uint64_t rc31(uint64_t x) {
    uint64_t r = 0;
    for (unsigned t = 0; t < FMER; ++t) r |= (3 - ((x >> (2 * t)) & 3)) << (2 * (FMER - 1 - t));
    return r;
}
static bool same(const FmerKey& a, const FmerKey& b) { return a.word == b.word && a.mask == b.mask; }

template <unsigned S>
static int symmetries() {
    auto check = [](uint64_t x) -> bool {
        const FmerKey k = fmer_key<S>(x);
        if (__builtin_popcountll(k.mask) < 1 || __builtin_popcountll(k.mask) > 2) return false;
        return same(k, fmer_key<S>(rc31(x & M62))) && same(k, fmer_key<S>(x | (3ull << 62))) && same(k, fmer_key<S>(x & M62));
    };
    for (unsigned i = 0; i < 20000; ++i) if (!check(rnd())) { fprintf(stderr, "stride %u: a random 31-mer and its reverse complement differ\n", S); return 1; }
    for (unsigned period : {1u, 2u, 3u, 4u, 15u, 17u})
        for (unsigned rep = 0; rep < 64; ++rep) {
            unsigned pat[17];
            for (unsigned t = 0; t < period; ++t) pat[t] = (unsigned)(rnd() & 3);
            uint64_t x = 0;
            for (unsigned t = 0; t < FMER; ++t) x |= (uint64_t)pat[t % period] << (2 * t);
            if (!check(x) || !check(~x & M62)) { fprintf(stderr, "stride %u: period %u differs from its reverse complement\n", S, period); return 1; }
        }
    return 0;
}

static std::vector<uint8_t> g_bits;            // the stream, four bases a byte, 16 bytes of slack
static uint64_t mer_at(uint64_t g) {
    const uint64_t b0 = g >> 2; const unsigned sh = 2 * (unsigned)(g & 3);
    uint64_t v; std::memcpy(&v, &g_bits[b0], 8);
    v >>= sh;
    if (sh) v |= (uint64_t)g_bits[b0 + 8] << (64 - sh);
    return v;
}

// -> the count of maximal runs along the stride's chains (what the line's first figure is)
template <unsigned S>
static unsigned long stride_figures(uint64_t nbases) {
    uint64_t fw = 1024;
    while (fw * 4 < nbases) fw <<= 1;                                  // filter32_words_for (step2_graph.hip)
    const uint32_t fmask = (uint32_t)(fw - 1);
    const uint64_t npos = nbases - (FMER - 1);
    std::vector<uint32_t> word(npos);
    std::vector<uint64_t> filter(fw, 0);
    for (uint64_t g = 0; g < npos; ++g) { const FmerKey k = fmer_key<S>(mer_at(g)); word[g] = k.word & fmask; filter[word[g]] |= k.mask; }
    unsigned long runs = 0, cut64 = 0, cut256 = 0;
    for (uint64_t g = 0; g < npos; ++g) {
        const bool differs = g < S || word[g - S] != word[g];
        runs += differs; cut64 += differs || (g & 63) < S; cut256 += differs || (g & 255) < S;
    }
    // one substituted base in every 31-mer of a sample: does the filter prove it absent?  (a few of them do occur elsewhere in the stream)
    unsigned long tried = 0, absent = 0;
    for (uint64_t g = 0; g < npos; g += 5) {
        const unsigned t = (unsigned)(rnd() % FMER); const uint64_t flip = (1 + rnd() % 3) << (2 * t);
        const FmerKey k = fmer_key<S>(mer_at(g) ^ flip);
        ++tried; absent += (filter[k.word & fmask] & k.mask) != k.mask;
    }
    unsigned long bits = 0;
    for (uint64_t w : filter) bits += (unsigned long)__builtin_popcountll(w);
    printf("stride %u: positions %lu runs %lu cut64 %lu cut256 %lu absent %lu of %lu (%.4f) filter_words %lu bits_set %.4f\n", S, (unsigned long)npos, runs, cut64,
           cut256, absent, tried, (double)absent / (double)tried, (unsigned long)fw, (double)bits / (64.0 * (double)fw));
    return runs;
}

int main(int argc, char** argv) {
    const uint64_t nbases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000;
    if (nbases < 1000 || nbases > (1ull << 28)) return 2;
    if (symmetries<1>() || symmetries<2>() || symmetries<4>() || symmetries<8>() || symmetries<16>()) return 1;
    printf("keys equal their reverse complements' and ignore the bits above 62\n");
    g_bits.assign((nbases + 3) / 4 + 16, 0);
    for (uint64_t g = 0; g < nbases; ++g) g_bits[g >> 2] |= (uint8_t)(((rnd() >> 33) & 3) << (2 * (g & 3)));
    const unsigned long r4 = stride_figures<4>(nbases), r2 = stride_figures<2>(nbases), r1 = stride_figures<1>(nbases);
    if (!(r1 < r2 && r2 < r4)) { fprintf(stderr, "run counts are not in the order stride 1 < 2 < 4\n"); return 3; }
    printf("run counts in the order stride 1 < 2 < 4\n");
    return 0;
}
