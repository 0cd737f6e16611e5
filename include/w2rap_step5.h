/* w2rap_step5.h -- C ABI of the MI355X-native replacement for the LAST line of w2rap-contigger's Step 5: PartnersToEnds.
 * Exported by the same shared library as Steps 1-4 (w2rap_contigger_amd/libw2rap_step2.so).
 *
 * Drop-in boundary.  w2rap_step5_partners_to_ends replaces exactly this call of the reference's main (src/modules/w2rap-contigger.cc:448):
 *     PartnersToEnds(hbvr, pathsr, bases, quals);                         // src/paths/long/large/GapToyTools5.cc:1150-1517
 * A read that has no path, whose mate (read id ^ 1) is placed and ends on an edge within 500 K-mers of a dead end of the graph, has its
 * 28-mers looked up against every edge object; every (edge, offset) hit is checked with a quality-aware sliding window, and the read is
 * placed -- path [edge], offset -- when exactly ONE candidate is good.  The graph is not edited; the output is the read paths.
 * Everything before it in Step 5 (the local assemblies, AddNewStuff, Unsat) and Steps 6-7 stay the reference's.
 *
 * What runs where.  Everything runs in HIP kernels for gfx950 (the k5_* kernels of step5_partners.hip, the library's scans and radix sort);
 * there is no CPU fallback (W2RAP_E_NO_DEVICE).  The host checks the arguments and derives each edge's two vertices from the adjacency
 * lists before the upload.
 *
 * Plain pointers and sizes; never throws; returns 0 or a W2RAP_E_* code (w2rap_step2.h) with a message in `err`.  Integer arithmetic
 * throughout: the result does not depend on the order in which anything is processed.
 */
#ifndef W2RAP_STEP5_H_
#define W2RAP_STEP5_H_

#include "w2rap_step2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- inputs (host memory): the graph, paths, reads and unpacked-qualities fields of w2rap_step4_in, same meaning; no inv ---- */
typedef struct w2rap_step5_in {
    int32_t  K;                      /* hbvr.K(); 16 <= K <= 640 */
    uint64_t n_edge_objs;
    const uint8_t*  edge_packed;     /* each object ceil(len/4) bytes, base i at bits 2*(i%4) of byte i/4 */
    const uint64_t* edge_byte_off;   /* [n_edge_objs+1] */
    const uint32_t* edge_len;        /* [n_edge_objs] bases, >= K */
    uint64_t n_vertices;
    const uint64_t* from_off;        /* [n_vertices+1] */
    const int32_t*  from_v;          /* [n_edge_objs] */
    const int32_t*  from_e;          /* [n_edge_objs] */
    const uint64_t* to_off;          /* [n_vertices+1] */
    const int32_t*  to_e;            /* [n_edge_objs] */
    /* pathsr */
    uint64_t n_paths;                /* even: read r and read r ^ 1 are mates */
    const int32_t*  path_offset;     /* [n_paths] */
    const uint64_t* path_off;        /* [n_paths+1] */
    const int32_t*  path_edges;
    /* the reads and the UNPACKED .qualp values, one byte per base */
    uint64_t n_reads;                /* == n_paths */
    const uint8_t*  read_packed;
    const uint64_t* read_byte_off;   /* [n_reads+1] */
    const uint32_t* read_len;        /* [n_reads] */
    const uint8_t*  quals;
    const uint64_t* qual_off;        /* [n_reads+1]; qual_off[r+1] - qual_off[r] == read_len[r] */
} w2rap_step5_in;

typedef struct w2rap_step5_params {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t flags;                  /* none defined: must be 0 */
} w2rap_step5_params;

/* ---- outputs (library-allocated HOST memory; free with w2rap_step5_free) ---------------------------------------------------- */
typedef struct w2rap_step5_out {
    /* ALL read paths: a read the call did not touch keeps its path and offset */
    uint64_t n_paths;
    int32_t*  path_offset;           /* [n_paths] */
    uint64_t* path_off;              /* [n_paths+1] */
    int32_t*  path_edges;
    uint64_t n_interesting;          /* reads looked up (findInterestingReadIds) */
    uint64_t n_read_kmers;           /* their 28-mers: the nKmers the reference's findInterestingReadIds returns */
    uint64_t n_dict_kmers;           /* distinct 28-mers left in the dictionary after both multiplicity filters */
    uint64_t n_candidates;           /* distinct (read, edge, offset) triples */
    uint64_t n_good;                 /* of those: passed the window check */
    uint64_t n_placed;               /* reads with exactly one good candidate */
    uint64_t n_ambiguous;            /* reads with two or more */
    /* device time per phase, milliseconds */
    float ms_ends, ms_select, ms_dict, ms_edges, ms_candidates, ms_verify, ms_paths;
} w2rap_step5_out;

int  w2rap_step5_partners_to_ends(const w2rap_step5_in* in, const w2rap_step5_params* params, w2rap_step5_out* out, char* err, size_t errlen);
void w2rap_step5_free(w2rap_step5_out* out);

/* per-kernel device time of the last w2rap_step5_partners_to_ends in this process: "kernel_name total_ms launches\n" lines; returns the
 * bytes needed */
size_t w2rap_step5_profile(char* buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* W2RAP_STEP5_H_ */
