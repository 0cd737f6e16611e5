/* w2rap_step4.h -- C ABI of the MI355X-native replacement for w2rap-contigger's Step 4, "Cleaning graph" (Clean200x).
 * Exported by the same shared library as Steps 1-3 (w2rap_contigger_amd/libw2rap_step2.so).
 *
 * Drop-in boundary.  w2rap_step4_run replaces exactly this block of the reference's main (src/modules/w2rap-contigger.cc:395-399):
 *     inv.clear();
 *     hbvr.Involution(inv);                                              // src/paths/HyperBasevector.cc:648-660
 *     Clean200x(hbvr, inv, pathsr, bases, quals, 0, 3, min_size);        // src/paths/long/large/Clean200.cc:202-389
 * Inputs are what BinaryReader::readFile(<prefix>.large_K.hbv), LoadReadPathVec(<prefix>.large_K.paths) and the loads of
 * frag_reads_orig.fastb / .qualp hold (:322-328, :388-389); outputs are what BinaryWriter::writeFile(<prefix>.large_K.clean.hbv, hbvr)
 * and WriteReadPathVec(pathsr, <prefix>.large_K.clean.paths) serialise (:404-405).
 *
 * What runs where.  Everything runs in HIP kernels for gfx950; there is no CPU fallback (W2RAP_E_NO_DEVICE).  The reads' side: the paths
 * index (invert(), VecUtilities.h:693-719), the placements of reads on branch vertices, the quality-weighted vote, the verdict
 * (AnalyzeScores) and the rewrite of the read paths.  The graph's side: min_size, DeleteEdges, RemoveUnneededVertices2 and CleanupCore
 * (the k4e_* kernels), which reproduce the numbering the reference's two stacks define, and the branch-vertex and task lists of each
 * pass.  The graph is uploaded once and downloaded once; between the two nothing of it crosses PCIe (the per-pass deleted lists, which
 * are results, and a handful of counts come down).  Only the involution for in.inv == NULL is computed on the host, before the upload.
 * The same edit exists on the host inside the library: W2RAP_STEP4_EDIT_ON_HOST forces it (the cross-check), and a call whose graph does
 * not meet a precondition of the device edit -- adjacency lists sorted by neighbour vertex, as AddEdge keeps them; every merged run's
 * mirror image is itself a run with the mirrored ends -- or has no edges falls back to it silently, with the same result.
 * w2rap_step4_profile tells which one ran.
 *
 * Behind Step 3 in one process.  w2rap_step2_run_step4_after_step3 replaces the same block of main in the reference's default flow, where hbvr,
 * pathsr, bases and quals are the objects Steps 1-3 left in memory: its inputs are a Step-2 context's reads and qualities and the large-K
 * result that w2rap_step3_run_after_step2 left in that context's HBM (W2RAP_STEP3_KEEP_DEVICE, w2rap_step3.h); inv is Step 3's inv2.
 * Nothing is uploaded, validated on the host or rebuilt there; the vote and edit kernels are the same, and the clean graph and paths
 * come down once.  The reads never come down.
 *
 * Plain pointers and sizes; never throws; returns 0 or a W2RAP_E_* code (w2rap_step2.h) with a message in `err`.  Integer arithmetic
 * throughout: results are exact, byte for byte the reference's.
 */
#ifndef W2RAP_STEP4_H_
#define W2RAP_STEP4_H_

#include "w2rap_step2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- inputs (host memory) ------------------------------------------------------------------------------------------------- */
typedef struct w2rap_step4_in {
    int32_t  K;                      /* hbvr.K(): the large K, 200 by default; 16 <= K <= 640 */
    uint64_t n_edge_objs;            /* hbvr.EdgeObjectCount() */
    const uint8_t*  edge_packed;     /* each object ceil(len/4) bytes, base i at bits 2*(i%4) of byte i/4 (.hbv edges_ section) */
    const uint64_t* edge_byte_off;   /* [n_edge_objs+1] */
    const uint32_t* edge_len;        /* [n_edge_objs] bases, >= K */
    /* the adjacency LISTS as the .hbv file holds them: their order is From(v) / To(v), which IFrom(v, j) and the stacks of
       RemoveUnneededVertices2 depend on.  Every edge object appears once in from_e and once in to_e */
    uint64_t n_vertices;             /* hbvr.N() */
    const uint64_t* from_off;        /* [n_vertices+1] */
    const int32_t*  from_v;          /* [n_edge_objs] From(v) */
    const int32_t*  from_e;          /* [n_edge_objs] from_edge_obj_ */
    const uint64_t* to_off;          /* [n_vertices+1] */
    const int32_t*  to_e;            /* [n_edge_objs] to_edge_obj_ */
    const int32_t*  inv;             /* [n_edge_objs] hbvr.Involution (w2rap_step3_out.inv2), or NULL: computed here from the sequences */
                                     /* (checked: an involution of edges of equal length.  If it does not mirror a merged run onto a run,
                                      *  the call returns W2RAP_E_GRAPH where the reference's walk would leave the graph) */
    /* pathsr */
    uint64_t n_paths;
    const int32_t*  path_offset;     /* [n_paths] */
    const uint64_t* path_off;        /* [n_paths+1] */
    const int32_t*  path_edges;
    /* the reads: frag_reads_orig.fastb and the UNPACKED .qualp values, one byte per base */
    uint64_t n_reads;                /* == n_paths */
    const uint8_t*  read_packed;
    const uint64_t* read_byte_off;   /* [n_reads+1] */
    const uint32_t* read_len;        /* [n_reads] */
    const uint8_t*  quals;
    const uint64_t* qual_off;        /* [n_reads+1]; qual_off[r+1] - qual_off[r] == read_len[r] */
} w2rap_step4_in;

typedef struct w2rap_step4_params {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t min_size;               /* -s / --min_size: a component that is one edge of at most min_size K-mers is deleted; default 0 (off) */
    uint32_t flags;
} w2rap_step4_params;
#define W2RAP_STEP4_VOTE_ONLY 1u     /* run pass 1's vote (and min_size), return its deleted list, edit nothing: the outputs hold the input graph and paths */
#define W2RAP_STEP4_EDIT_ON_HOST 2u  /* edit the graph on the host (one pack, CSR and upload per pass, as before the device edit existed) */

/* ---- outputs (library-allocated HOST memory; free with w2rap_step4_free) ---------------------------------------------------- */
typedef struct w2rap_step4_out {
    int32_t  K;
    /* the clean graph, field layout of w2rap_step3_out */
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
    int32_t*  inv;                   /* [n_edge_objs] the involution of the clean graph */
    /* the read paths on it */
    uint64_t n_paths;
    int32_t*  path_offset;           /* [n_paths] */
    uint64_t* path_off;              /* [n_paths+1] */
    int32_t*  path_edges;
    /* per pass: the sorted unique edge ids handed to hb.DeleteEdges (Clean200.cc:384), ids of THAT pass's input graph */
    uint64_t n_deleted[2];
    int32_t*  deleted[2];
    uint64_t n_runs_merged[2];       /* edges RemoveUnneededVertices2 added (a run and its mirror count as two) */
    uint64_t n_branch_vertices;      /* vertices with an edge in and two or more out, both passes */
    uint64_t n_skipped_too_many_exts;/* of those: more than 10 walks (Clean200.cc:246) */
    uint64_t n_placements;           /* (read, start) placements scored, both passes */
    float ms_index[2], ms_vote[2], ms_paths[2];      /* device time per pass, milliseconds */
    float ms_graph_edit_host[2];                     /* HOST clock spent in the graph edit phase per pass, milliseconds: the edit itself and the
                                                        upload of the next pass's graph with EDIT_ON_HOST (HostEditor4::pass); launching the
                                                        k4e_* kernels and waiting for their counts without (DeviceEditor4::pass) */
    void* _owner;                    /* internal */
} w2rap_step4_out;

int  w2rap_step4_run(const w2rap_step4_in* in, const w2rap_step4_params* params, w2rap_step4_out* out, char* err, size_t errlen);
void w2rap_step4_free(w2rap_step4_out* out);

/* Step 4 straight behind Step 3, a call on the Step-2 context like w2rap_step2_fetch (hence its prefix: the w2rap_step4_* names are the
 * three of the one-shot interface, and stay those three): `ctx` has run w2rap_step3_run_after_step2 with W2RAP_STEP3_KEEP_DEVICE and nothing since that gives the
 * kept result up (w2rap_step3.h).  params->device must be the context's device (W2RAP_E_ARG).  W2RAP_E_STATE, with a message that names
 * the missing step, when the context holds no kept result or its reads' raw qualities were never uploaded (a graph-only Step 2).
 * A full run consumes the kept result -- pass 1's inputs go back to the context's pool as soon as pass 1 is through -- so a second call
 * answers W2RAP_E_STATE; W2RAP_STEP4_VOTE_ONLY edits nothing and leaves it valid, so a vote can be followed by the full run.  With
 * W2RAP_STEP4_EDIT_ON_HOST, VOTE_ONLY, or a graph that misses a precondition of the device edit (then from the pass that found it on),
 * the host editor works on one download of the graph as it lies on the device.  On any failure the kept result is given up and every
 * device block of the call goes back to the pool.  Whatever happens, the context's Step-2 state is not touched (w2rap_step2_fetch and
 * another Step 3 work afterwards) and its live device bytes return to what they were before Step 3 kept anything. */
int  w2rap_step2_run_step4_after_step3(w2rap_step2_ctx* ctx, const w2rap_step4_params* params, w2rap_step4_out* out, char* err, size_t errlen);

/* per-kernel device time of the last w2rap_step4_run or w2rap_step2_run_step4_after_step3 in this process: "kernel_name total_ms launches\n" lines; returns the bytes needed.
 * The device edit's time is the sum of the k4e_* lines.  The last line, in the same format, is "edit_path_device <0|1> <passes>": 1 and
 * the number of passes edited on the device, or 0 0 when the host edit ran (EDIT_ON_HOST, the fallback -- also one that the chained call
 * took in pass 2 only) or nothing was edited (VOTE_ONLY) */
size_t w2rap_step4_profile(char* buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* W2RAP_STEP4_H_ */
