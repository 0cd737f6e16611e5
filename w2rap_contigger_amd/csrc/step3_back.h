// step3_back.h -- the back half of Step 3 (step3_repath.hip): buildBigKHBVFromReads behind its input, on a stream of 2-bit sequences that
// is already on the device.  RepathInMemory (w2rap_step3_run) feeds it the unique places, AddNewStuff (step5_add.hip) feeds it `allx`.
// Internal: not part of the C ABI.
#ifndef W2RAP_STEP3_BACK_H_
#define W2RAP_STEP3_BACK_H_
#include "ctx.h"

namespace w2 {

// U sequences in one stream of 64-bit words, 32 bases a word, base t of sequence u at stream position 32 woff[u] + t.  Sequence u owns
// ceil(nbases[u] / 32) + 1 words (the last one zero: 64-bit reads past its end stay inside its own zeros); 4 zeroed words follow the
// last sequence.  koff[u] = the number of K2-mers of the sequences before u (nbases - K2 + 1 each, 0 for a shorter one); N2 = koff[U].
// kblk = block_index over koff (where every block of 256 occurrences starts among the sequences).
struct Stream3 { uint64_t U, N2; const uint64_t* all; const uint64_t* woff; const uint32_t* nbases; const uint64_t* koff; const uint32_t* kblk; };
// W2RAP_STEP3_UNIQUE_KMERS only: the places as edge vectors of a graph whose K-mers are unique (k3_mid_edges, k3_lone_places)
struct Lone3 { uint64_t NO; const uint64_t* voff; const int32_t* pvec; const int32_t* inv; };

struct Back3 {
    // step3_back: the dictionary ...
    uint64_t D = 0, E = 0, NO2 = 0, NV = 0;          // distinct K2-mers, unipaths, edge objects, vertices
    uint32_t* id_of = nullptr; uint16_t* meta = nullptr;                         // [N2] per occurrence
    uint32_t *k_edge = nullptr, *k_off = nullptr;                               // [D] unipath (bit 31: against its orientation) and offset of a K2-mer
    uint32_t* edge_nk = nullptr; uint64_t* edge_off = nullptr; uint8_t* codes = nullptr;   // [E] K2-mers, base offsets; the unipaths a base a byte
    int32_t *fwdX = nullptr, *revX = nullptr;                                   // [E] the objects of a unipath and of its reverse complement
    // ... and the graph
    uint32_t* obj_edge = nullptr; int32_t *inv2 = nullptr, *left = nullptr, *right = nullptr;      // [NO2]
    uint64_t *from_off = nullptr, *to_off = nullptr; int32_t *from_v = nullptr, *from_e = nullptr, *to_v = nullptr, *to_e = nullptr;
    float ms_dict = 0, ms_graph = 0;
    // step3_through
    uint64_t nip = 0; uint64_t* oex = nullptr; int32_t* ipath = nullptr; uint64_t* ioff = nullptr; int32_t *starts = nullptr, *stops = nullptr;
    // step3_pack
    uint32_t* olen = nullptr; uint64_t* byoff = nullptr; uint8_t* packed = nullptr; uint64_t total_bytes = 0;
};

// d_flags: 8 zeroed words ([1] = error bits, read by step3_check); d_cnt: 112 zeroed counters ([101..103] are used here)
// out[b] = the last i with a[i] <= 256 b, for the blocks of 256 over `total` elements (Stream3::kblk over koff)
int step3_block_index(Ctx& c, const uint64_t* a, uint64_t n, uint64_t total, uint32_t** out);
int step3_check(Ctx& c, const uint32_t* d_flags, uint32_t h_flags[4]);
int step3_back(Ctx& c, unsigned K2, const Stream3& S, const Lone3* lone, const w2rap_edge_hint* hint, uint32_t* d_flags, unsigned long long* d_cnt, Back3& B);
int step3_through(Ctx& c, const Stream3& S, Back3& B);
int step3_pack(Ctx& c, unsigned K2, Back3& B);

}  // namespace w2
#endif
