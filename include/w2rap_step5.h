/* w2rap_step5.h -- C ABI of the MI355X-native replacements for the read-sized parts of w2rap-contigger's Step 5: its LAST line,
 * PartnersToEnds (below), its opening, the paths index, Unsat's links and LayoutReads (w2rap_step5_open, further down), and AddNewStuff,
 * which rebuilds the graph with the patches in front of PartnersToEnds (w2rap_step5_add_new_stuff, at the end).
 * Exported by the same shared library as Steps 1-4 (w2rap_contigger_amd/libw2rap_step2.so).
 *
 * Drop-in boundary.  w2rap_step5_partners_to_ends replaces exactly this call of the reference's main (src/modules/w2rap-contigger.cc:448):
 *     PartnersToEnds(hbvr, pathsr, bases, quals);                         // src/paths/long/large/GapToyTools5.cc:1150-1517
 * A read that has no path, whose mate (read id ^ 1) is placed and ends on an edge within 500 K-mers of a dead end of the graph, has its
 * 28-mers looked up against every edge object; every (edge, offset) hit is checked with a quality-aware sliding window, and the read is
 * placed -- path [edge], offset -- when exactly ONE candidate is good.  The graph is not edited; the output is the read paths.
 * AddNewStuff, the call in front of it, is w2rap_step5_add_new_stuff (at the end of this header).  The local assemblies, the clustering
 * half of Unsat and Step 6 stay the reference's (Step 7's read-sized passes: w2rap_step7.h).
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

/* ==== the OPENING of Step 5: the three read-sized passes the reference runs before its first cluster exists =====================
 * w2rap_step5_open computes, from the clean graph, its involution and the read paths (no bases, no qualities):
 *   INDEX   invert(pathsr, paths_inv, E)              src/modules/w2rap-contigger.cc:427, src/VecUtilities.h:693
 *   LINKS   Phase 1 of Unsat: unsats[e] and mult      src/paths/long/large/Unsat.cc:142-207
 *   LAYOUT  LayoutReads                               src/paths/long/large/GapToyTools2.cc:550-588
 * Each result is one CSR over the edge objects.  The clustering half of Unsat, the local assemblies and AddNewStuff stay the reference's.
 * All kernels are HIP for gfx950 (k5o_* of step5_open.hip, the library's scan and radix sort); there is no CPU fallback
 * (W2RAP_E_NO_DEVICE).  Integer arithmetic throughout; the result does not depend on the order in which reads or pairs are processed.
 *
 * Limits (32-bit ids, as elsewhere in the library; beyond them the call answers W2RAP_E_ARG): n_edge_objs and n_vertices below 2^31,
 * n_paths below 2^30 (a read has up to four layout entries, and the layout's sort carries an entry's number as its 32-bit value).
 * The number of path entries is not limited: keys and offsets are 64-bit.
 *
 * INDEX.   index_read[index_off[e] .. index_off[e+1]) = the ids of the reads whose path holds e, ascending, a read once per occurrence.
 * LINKS.   A pair (reads 2p, 2p+1; pid = p) with both paths non-empty is examined: x1 = the edges of p1, x2 = inv of the edges of p2,
 *          reversed.  It is dropped when x1 and x2 share an edge (Meet2), or when v = to_right[x1.back] equals w = to_left[x2.front].
 *          Otherwise w is searched from v over from_v, level by level for 15 levels, the frontier a MULTISET (no visited set): a level
 *          that holds w satisfies the pair, however large the level; otherwise a level of more than 50 entries ends the search.  A
 *          pair that is not satisfied and has p1.back != p2.back gives the links (p1.back, inv[p2.back], pid) and
 *          (p2.back, inv[p1.back], pid).  link_to / link_pid[link_off[e] .. link_off[e+1]) = unsats[e] after the reference's Sort and
 *          de-duplication, ordered by (link_to, pid).  kind_from / kind_to / kind_mult [n_kinds] = the map `mult`: one entry per distinct
 *          (e, link_to) in that order, kind_mult its number of links.
 * LAYOUT.  layout_pos / layout_id / layout_fw [layout_off[e] .. layout_off[e+1]) = layout_pos[e], layout_id[e], layout_or[e].  Per read
 *          with a path x of n > 0 edges, kmers(e) = edge_len[e] - K + 1: forward (x[0], offset) and, if n > 1, (x[n-1], offset - kmers(x[0]))
 *          -- the reference skips the interior edges BEFORE it subtracts their length, so only the first edge's K-mers come off, which
 *          is reproduced; reverse, with y = inv of x reversed, len = edge_len[y[0]] + the sum of kmers(y[j]) over j >= 1 and
 *          pos = len - (offset + read_len): (y[0], pos) and, if n > 1, (y[n-1], pos - kmers(y[0])).  Each edge's entries ascend by pos as
 *          a SIGNED value.  Ties: the reference's SortSync leaves them in an unspecified order and its only consumer (FindPidsST) reads
 *          the lists as sets; THIS LIBRARY orders ties by read id, then forward before reverse -- its own choice, not the reference's.
 */
#define W2RAP_STEP5_OPEN_INDEX  1u
#define W2RAP_STEP5_OPEN_LINKS  2u
#define W2RAP_STEP5_OPEN_LAYOUT 4u

typedef struct w2rap_step5_open_in {
    int32_t  K;                      /* hbv.K(); 16 <= K <= 640 (only LAYOUT reads it) */
    uint64_t n_edge_objs;
    const uint32_t* edge_len;        /* [n_edge_objs] bases, >= K */
    uint64_t n_vertices;
    const uint64_t* from_off;        /* [n_vertices+1] */
    const int32_t*  from_v;          /* [n_edge_objs] */
    const int32_t*  from_e;          /* [n_edge_objs] */
    const uint64_t* to_off;          /* [n_vertices+1] */
    const int32_t*  to_e;            /* [n_edge_objs] */
    const int32_t*  inv;             /* [n_edge_objs]; inv[inv[e]] == e */
    uint64_t n_paths;                /* even: read r and read r ^ 1 are mates */
    const int32_t*  path_offset;     /* [n_paths] */
    const uint64_t* path_off;        /* [n_paths+1] */
    const int32_t*  path_edges;
    const uint32_t* read_len;        /* [n_paths] bases[i].size() */
} w2rap_step5_open_in;

/* params: w2rap_step5_params; flags = any of W2RAP_STEP5_OPEN_*, 0 = all three.  A part that is not asked for launches no kernel and
 * leaves its pointers null, its counters and its time zero */
typedef struct w2rap_step5_open_out {
    uint64_t* index_off;  uint32_t* index_read;                                  /* [E+1], [n_index] */
    uint64_t* link_off;   int32_t* link_to;  uint32_t* link_pid;                 /* [E+1], [n_links] */
    int32_t*  kind_from;  int32_t* kind_to;  uint32_t* kind_mult;                /* [n_kinds] */
    uint64_t* layout_off; int32_t* layout_pos; uint32_t* layout_id; uint8_t* layout_fw;   /* [E+1], [n_layout]; fw 1 = forward */
    /* LINKS: pairs with both paths non-empty, and what became of them (placed = meet + same_vertex + reached + unsat_depth + unsat_overflow) */
    uint64_t n_pairs_placed, n_meet, n_same_vertex, n_reached;
    uint64_t n_unsat_depth;          /* fell out of the 15 levels */
    uint64_t n_unsat_overflow;       /* stopped by a level of more than 50 */
    uint64_t n_unsat_same_end;       /* of the unsatisfied: p1.back == p2.back, no link */
    uint64_t n_links, n_kinds, n_index, n_layout;
    float ms_index, ms_links, ms_layout;       /* device time per part, milliseconds */
} w2rap_step5_open_out;

int  w2rap_step5_open(const w2rap_step5_open_in* in, const w2rap_step5_params* params, w2rap_step5_open_out* out, char* err, size_t errlen);
void w2rap_step5_open_free(w2rap_step5_open_out* out);

/* ==== the CLOSE of Step 5: AddNewStuff, the call in front of PartnersToEnds and the only place in Step 5 where the graph changes ====
 *     AddNewStuff(new_stuff, hbr, inv2, pathsr, bases, quals, MIN_GAIN, TRACE_PATHS, work_dir, EXT_MODE);
 *                                                  src/modules/w2rap-contigger.cc:447, src/paths/long/large/GapToyTools4.cc:133-368
 * w2rap_step5_add_new_stuff takes the clean large-K graph, the read paths, the reads with their qualities and the patch sequences
 * `new_stuff` (what the local assemblies of AssembleGaps2 found), and does what the reference does:
 *   ALL        allx = the edge objects in id order, then one (K+1)-mer per vertex crossing in BuildAll's order (vertex, i1 over To, i2
 *              over From: the last K bases of e1 followed by base K-1 of e2), then new_stuff                          (:131-161, :238-241)
 *   GRAPH      buildBigKHBVFromReads(K, allx): the SAME builder RepathInMemory calls -- the back half of this library's Step 3, shared
 *              (csrc/step3_back.h).  W2RAP_STEP3_UNIQUE_KMERS' shortcut is off here: new_stuff repeats the graph's K-mers.  to3[e] /
 *              left3[e] = the path and first skip of sequence e of allx, e an old edge object                         (:250-262)
 *   TRANSLATE  TranslatePaths: every read path moves onto the new graph and is cut to ONE edge.  A path the reference clear()s keeps its
 *              OLD offset (ReadPath::clear is std::vector's: mOffset is not touched), and so it does here             (:164-197)
 *   EXTEND     ExtendPath, mode 1: a read that runs past the end of its edge is extended over the branches behind it when exactly one
 *              extension covering the read beats the runner-up by min_gain in summed quality at mismatches           (:289-356)
 * The new graph comes back laid out exactly as w2rap_step3_out lays one out; edge numbering as in Step 3 (canonical, or edge_order_hint).
 * All kernels are HIP for gfx950 (k5a_* of step5_add.hip and the k3_* of the shared back half); there is no CPU fallback.
 *
 * W2RAP_E_ARG before any kernel runs: K odd or outside [16, 640] (what the Step-3 stage builds); ext_mode != 1 -- the reference's mode 2
 * is NOT built; min_gain < 1 -- at 1 and above a tie for the best extension never extends, so the order the reference's SortSync leaves
 * ties in cannot matter, below 1 it would; an unknown flag; and every check of w2rap_step5_in.  new_stuff entries may have any length,
 * 0 and below K included (they hold no K-mer), and n_new may be 0.
 */
#define W2RAP_STEP5_ADD_KEEP_MAP 1u  /* return to3 / left3 */

typedef struct w2rap_step5_add_params {
    int32_t  device;                 /* HIP device ordinal */
    int32_t  min_gain;               /* MIN_GAIN: the reference passes 5; >= 1 */
    int32_t  ext_mode;               /* EXT_MODE: the reference passes 1; only 1 is built */
    const w2rap_edge_hint* edge_order_hint;   /* as in Step 3; NULL = canonical (lexicographic) order of the new graph's unipaths */
    uint32_t flags;                  /* W2RAP_STEP5_ADD_KEEP_MAP */
} w2rap_step5_add_params;

typedef struct w2rap_step5_add_out {
    /* the new graph, as w2rap_step3_out lays it out */
    int32_t  K;
    uint64_t n_vertices;
    uint64_t n_edge_objs;
    uint8_t*  edge_packed;
    uint64_t* edge_byte_off;         /* [n_edge_objs+1] */
    uint32_t* edge_len;              /* [n_edge_objs] */
    int32_t*  vleft;                 /* [n_edge_objs] */
    int32_t*  vright;                /* [n_edge_objs] */
    uint64_t* from_off;              /* [n_vertices+1] */
    int32_t*  from_v;
    int32_t*  from_e;
    uint64_t* to_off;                /* [n_vertices+1] */
    int32_t*  to_v;
    int32_t*  to_e;
    int32_t*  inv2;                  /* [n_edge_objs] the new graph's involution */
    /* ALL read paths on the new graph */
    uint64_t n_paths;
    int32_t*  path_offset;           /* [n_paths] */
    uint64_t* path_off;              /* [n_paths+1] */
    int32_t*  path_edges;
    /* W2RAP_STEP5_ADD_KEEP_MAP: a CSR over the OLD edge objects, and left3 */
    uint64_t n_old_edge_objs;
    uint64_t* to3_off;               /* [n_old_edge_objs+1] */
    int32_t*  to3;
    int32_t*  left3;                 /* [n_old_edge_objs] */
    /* counters */
    uint64_t n_all, n_junctions, n_all_bases;               /* sequences of allx; of those, vertex crossings; the sum of their lengths */
    uint64_t n_kmer_instances, n_kmers_distinct, n_unipaths;
    uint64_t n_tr_empty, n_tr_first, n_tr_walked, n_tr_cleared;   /* TranslatePaths: sum = n_paths */
    uint64_t n_ext_tried;            /* reads past ExtendPath's early returns = too_many + no_cover + ambiguous + extended */
    uint64_t n_ext_too_many, n_ext_no_cover, n_ext_ambiguous, n_ext_extended;
    float ms_all, ms_dict, ms_graph, ms_translate, ms_extend;     /* device time per phase, milliseconds */
} w2rap_step5_add_out;

/* in: w2rap_step5_in (n_paths need not be even here: no mates are looked at); new_stuff in the packing of the edges */
int  w2rap_step5_add_new_stuff(const w2rap_step5_in* in, uint64_t n_new, const uint8_t* new_packed, const uint64_t* new_byte_off, const uint32_t* new_len,
                               const w2rap_step5_add_params* params, w2rap_step5_add_out* out, char* err, size_t errlen);
void w2rap_step5_add_free(w2rap_step5_add_out* out);

/* per-kernel device time of the last w2rap_step5_partners_to_ends, w2rap_step5_open or w2rap_step5_add_new_stuff in this process: "kernel_name total_ms launches\n"
 * lines; returns the bytes needed */
size_t w2rap_step5_profile(char* buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* W2RAP_STEP5_H_ */
