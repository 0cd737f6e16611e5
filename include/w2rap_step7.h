/* w2rap_step7.h -- C ABI of the MI355X-native replacement for the read-sized passes of w2rap-contigger's Step 7 (PE scaffolding):
 * the pairs of every line (GetLineNpairs, which Step 6 writes to .fin.lines.npairs and Step 7 reads back) and everything MakeGaps
 * does up to its list of accepted gaps.  Exported by the same shared library as Steps 1-5 (w2rap_contigger_amd/libw2rap_step2.so).
 *
 *   LINES   GetTol, GetLineLengths, GetLineNpairs        src/paths/long/large/Lines.cc:329-355, Lines.h:74-117
 *   LINKS   MakeGaps up to the accepted gaps             src/paths/long/large/MakeGaps.cc:25-427
 *   FILES   DumpLineFiles: a.lines.fasta, .efasta, .src   src/paths/long/large/Lines.cc:680-798 (w2rap_step7_line_files, below)
 *   COVER   ComputeCoverage, CNIntegerFraction: .covs, .lines.stats  src/paths/long/large/Lines.cc:442-624 (w2rap_step7_coverage, below)
 * What stays the reference's: the graph edit and the truncation of the paths behind the accepted gaps (MakeGaps.cc:429-493),
 * GAP_CLEANUP, the edge report and the GFA of FinalFiles, and FindLines -- the lines come in as data (the .fin.lines file, formats.read_lines).
 *
 * One call on host arrays; plain pointers and sizes; never throws; returns 0 or a W2RAP_E_* code (w2rap_step2.h) with a message in
 * `err`.  There is no CPU fallback (W2RAP_E_NO_DEVICE).
 *
 * What runs where.  HIP kernels for gfx950 (the k7_* kernels of csrc/step7_links.hip, the library's scans and radix sort):
 *   tol, llens and each line's end edges (a thread per line), npairs (a thread per pair), the nears (a thread per pair and pass:
 *   count, 64-bit scan, fill, one radix sort of the packed (e1, e2) keys), their runs and the per-edge maxima, the bounded search
 *   (a wavefront per distinct near), the links (compaction, sort by (first, second)) and the per-link filters (a thread per link).
 * On the HOST, because they are E-sized or smaller, integer, and ORDER-DEPENDENT or tiny:
 *   the edge groups tom / sink_like / source_like / dist_to_end (MakeGaps.cc:56-120) -- the two loops run in edge order, an edge reads
 *   what an earlier edge of the same sweep has just written, and three passes do not converge that away, so a parallel sweep is wrong;
 *   the set rules on the accepted links (MakeGaps.cc:353-427: one-to-one, bubble advance, UniqueSort, forced symmetry, overlinked) --
 *   the list is no longer than the number of line ends.
 *
 * LINES.  tol[e] = the LAST line that names e (GetTol writes in line order).  llens[l] = the sum over the line's cells of: the one
 *   path's K-mers; the mean of two paths ((a + b) / 2, integer); the median of three or more (for an even number the integer mean
 *   of the two middle ones), kmers(e) = edge_len[e] - K + 1, an empty path 0.  npairs[l]: per pair (reads 2p, 2p+1) the SET of
 *   tol[e] and tol[inv[e]] over both mates' edges; each line of the set counts once.  A pair counts even when one mate has no path.
 *   The distinct-line step keeps a sorted list of up to W2RAP_STEP7_PAIR_LINES (16) lines per thread; a pair that names more lines
 *   takes the spill path (every value is counted where it occurs first, found by rescanning; no storage) -- any number of lines, any
 *   path length.  n_pairs_listed / n_pairs_spilled say which path the pairs took.
 *
 * LINKS.  Parameters min_line and min_link_count (the reference's main passes 5000 and 3); the other heuristics are the reference's
 *   constants: max_hang 800, max_depth 2, max_int 1500, passes 3, max_cov_pc_off 20.0, max_line_to_ignore 500.
 *   1. Edge groups (host): zpass 1 works on the REVERSED graph, zpass 2 on the graph as given (hb.Reverse() at the top of each,
 *      six in all).  digraphE::Reverse swaps from_ with to_ and from_edge_obj_ with to_edge_obj_ per vertex, so the order inside an
 *      adjacency list is kept: EdgeObjectIndexByIndexFrom(v, i) of the reversed graph is to_e[to_off[v] + i] of the graph as given.
 *   2. Nears: per pair with both paths non-empty and per pass (pass 1: x = p1, y = inv of p2 reversed; pass 2: x = p2,
 *      y = inv of p1 reversed): tom applied, consecutive duplicates compressed, edges on lines of llens <= 500 dropped, then
 *      (x[j1], y[j2]) for every x[j1] that is not in y.  The per-thread list of y holds W2RAP_STEP7_NEAR_LIST (16) edges; a longer y
 *      is rescanned from the path (any length).  nears1 / nears2 are only read as run lengths: near_max1[e] = the largest count of
 *      any (e, .), near_max2[e] of any (., e), from the runs of the sorted nears.
 *   3. Links: one candidate per distinct near, count = its run length.  close = e2 is met on a walk of at most 3 steps from e1 or
 *      from e1's only predecessor (when to_left[e1] has exactly one in-edge); a step goes to an out-edge of the right vertex or an
 *      in-edge of the left vertex; a node is stepped from only while its accumulated K-mers (the start not counted) are <= 1500.
 *      The last step is not enumerated (e2 leaves v exactly when to_left[e2] == v).  Candidates that are not close are the links
 *      (tom[e1], tom[e2], count) -- tom a second time, as the reference does -- sorted by (first, second); links equal after tom
 *      stay separate entries, in the order of their nears.
 *   4. Filters, in the reference's order; link_reason[i] = the first that rejects link i (W2RAP_STEP7_R_*), 0 = accepted.
 *      The coverage test is IEEE double: cov = 100.0 * npairs / llens, c1 >= c2, rejected when c1 / c2 - 1.0 > 0.2: no pairs on one
 *      side give inf and reject, none on both give NaN and pass.
 *   5. Set rules (host) -> gap_from / gap_to sorted by (from, to), gap_inv[i] = the index of (inv[gap_to[i]], inv[gap_from[i]]), or
 *      -1 where the overlinked rule has removed it (the reference asserts there).
 *
 * W2RAP_E_ARG before the device is touched: K outside [16, 640]; an unknown flag; min_line or min_link_count < 0; sizes beyond
 * 32-bit ids (n_edge_objs, n_vertices, n_lines >= 2^31, n_paths >= 2^32 - 2); an odd n_paths; null arrays; edge_len < K; adjacency
 * lists or inv that are not what they claim; path_off / path_edges faults; line offsets that do not start at 0, descend or do not end
 * where the next level says; a line with an even number of cells (a line without cells included); a cell without a path (GetSegmentLength
 * asserts there), so also an empty first or last cell; an empty first path in the first or last cell (MakeGaps reads
 * lines[l].front()[0][0] and .back()[0][0]); a line edge outside [0, n_edge_objs); an edge object that belongs to no line (the
 * reference indexes llens[-1] there); npairs given with n_npairs != n_lines, or LINKS asked without LINES and without npairs.
 * W2RAP_E_LIMIT: a line whose paths, every path of every cell counted in full, hold 2^31 K-mers or more (llens is the reference's int).
 */
#ifndef W2RAP_STEP7_H_
#define W2RAP_STEP7_H_

#include "w2rap_step2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define W2RAP_STEP7_LINES 1u
#define W2RAP_STEP7_LINKS 2u

#define W2RAP_STEP7_PAIR_LINES 16    /* LINES: distinct lines a pair's sorted list holds before the spill path takes over */
#define W2RAP_STEP7_NEAR_LIST  16    /* LINKS: edges of y a thread keeps before it rescans the path instead */

/* link_reason */
#define W2RAP_STEP7_R_ACCEPTED   0
#define W2RAP_STEP7_R_COUNT      1   /* count < min_link_count */
#define W2RAP_STEP7_R_LINE       2   /* llens of either side < min_line */
#define W2RAP_STEP7_R_COVERAGE   3   /* c1 / c2 - 1.0 > 0.2 */
#define W2RAP_STEP7_R_ALT        4   /* max_alt > count */
#define W2RAP_STEP7_R_LEFT_END   5   /* e1 (advanced past bubbles) is not the last edge of its line */
#define W2RAP_STEP7_R_RIGHT_END  6   /* e2 (advanced) is not the first edge of its line */

typedef struct w2rap_step7_in {
    int32_t  K;                      /* hb.K(); 16 <= K <= 640 */
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
    const uint64_t* path_off;        /* [n_paths+1] */
    const int32_t*  path_edges;
    /* the lines, vec<vec<vec<vec<int>>>> flattened: line -> cell -> path -> edge */
    uint64_t n_lines;
    const uint64_t* line_off;        /* [n_lines+1] into the cells */
    const uint64_t* cell_off;        /* [n_cells+1] into the paths, n_cells = line_off[n_lines] */
    const uint64_t* lpath_off;       /* [n_lpaths+1] into line_edges, n_lpaths = cell_off[n_cells] */
    const int32_t*  line_edges;      /* [lpath_off[n_lpaths]] */
    /* .fin.lines.npairs for LINKS without LINES; NULL: LINKS reads what LINES of this call counts.  With LINES and npairs both,
       LINKS reads the GIVEN values */
    uint64_t n_npairs;               /* == n_lines when npairs is given */
    const int32_t*  npairs;
} w2rap_step7_in;

typedef struct w2rap_step7_params {
    int32_t  device;                 /* HIP device ordinal */
    uint32_t flags;                  /* any of W2RAP_STEP7_*, 0 = both */
    int32_t  min_line;               /* MIN_LINE: the reference's main passes 5000 */
    int32_t  min_link_count;         /* MIN_LINK_COUNT: the reference's main passes 3 */
} w2rap_step7_params;

/* outputs: library-allocated HOST memory, free with w2rap_step7_free.  A part that is not asked for launches no kernel of its own and
 * leaves its pointers null, its counters and its time zero; tol and llens come back with either part */
typedef struct w2rap_step7_out {
    int32_t* tol;                    /* [n_edge_objs] */
    int32_t* llens;                  /* [n_lines] */
    int32_t* npairs;                 /* [n_lines]  LINES */
    /* LINKS 1 */
    int32_t* tom;                    /* [n_edge_objs] */
    uint8_t* sink_like;              /* [n_edge_objs] */
    uint8_t* source_like;            /* [n_edge_objs] */
    int32_t* dist_to_end;            /* [n_edge_objs] */
    /* LINKS 2 */
    int32_t* near_max1;              /* [n_edge_objs] */
    int32_t* near_max2;              /* [n_edge_objs] */
    /* LINKS 3-4: every link, sorted by (from, to) */
    int32_t* link_from;              /* [n_links] */
    int32_t* link_to;
    int32_t* link_count;
    uint8_t* link_reason;            /* W2RAP_STEP7_R_* */
    /* LINKS 5 */
    int32_t* gap_from;               /* [n_gaps] */
    int32_t* gap_to;
    int32_t* gap_inv;
    /* LINES counters: n_pairs = n_pairs_listed + n_pairs_spilled */
    uint64_t n_pairs, n_pairs_listed, n_pairs_spilled;
    uint64_t n_pairs_no_path;        /* of the listed: neither mate has a path (no line counted) */
    uint64_t n_line_hits;            /* the sum of npairs */
    /* LINKS counters */
    uint64_t n_group_sink, n_group_source;     /* sink-like / source-like edges behind step 1 (dead ends and sources included) */
    uint64_t n_group_loop1, n_group_loop2;     /* times the first / the second loop fired, over all six sweeps */
    uint64_t n_pass_placed;          /* (pair, pass) with both paths non-empty = 2 x such pairs */
    uint64_t n_pass_y_long;          /* of those: y longer than the per-thread list */
    uint64_t n_pass_none;            /* of those: no near emitted */
    uint64_t n_nears, n_near_kinds;  /* nears; distinct (e1, e2) = candidates */
    uint64_t n_pred_start;           /* candidates whose search also starts from e1's only predecessor */
    uint64_t n_close[4];             /* candidates found close, by the fewest steps: [0] e2 is that predecessor, [1..3] steps */
    uint64_t n_links;                /* candidates that are not close */
    uint64_t n_reason[7];            /* links per W2RAP_STEP7_R_* */
    uint64_t n_not_one_to_one;       /* accepted links the one-to-one rule deleted */
    uint64_t n_advanced;             /* of the remaining: moved past a bubble on either side */
    uint64_t n_unique;               /* after UniqueSort (the reference's na) */
    uint64_t n_sym_deleted;          /* "deleting N gaps ... */
    int64_t  n_sym_added;            /* ... and adding M gaps to force symmetry": size after - na, as the reference prints it */
    uint64_t n_overlinked;           /* gaps the overlinked rule deleted */
    uint64_t n_gaps;
    float ms_lines, ms_nears, ms_search, ms_filter;   /* device time per part, milliseconds (ms_lines: tol, llens, npairs) */
} w2rap_step7_out;

int  w2rap_step7_links(const w2rap_step7_in* in, const w2rap_step7_params* params, w2rap_step7_out* out, char* err, size_t errlen);
void w2rap_step7_free(w2rap_step7_out* out);

/* per-kernel device time of the last w2rap_step7_links in this process: "kernel_name total_ms launches\n" lines; returns the bytes needed */
size_t w2rap_step7_profile(char* buf, size_t len);

/* ---- FILES: DumpLineFiles (Lines.cc:680-798), the texts of a.lines.fasta, a.lines.efasta and a.lines.src -------------------------------
 *
 * One call on host arrays, as above.  HIP kernels for gfx950 (the k7f_* kernels of csrc/step7_fasta.hip, the library's scans and sort):
 *   the paths index (`invert`, the kernels Step 5's opening builds it with), the vote (k7f_vote: a wavefront per voted cell, lanes over
 *   the index entries of e and of inv[e], the cov row in LDS up to W2RAP_STEP7_VOTE_ROW paths per cell and in global memory beyond),
 *   the shares (k7f_share: a wavefront per cell of two or more paths), the layout (k7f_path_len, k7f_cell_size, k7f_pieces: a thread
 *   per path of a cell turns it into pieces, scans place every piece and line) and the writer (k7f_write: 16 output bytes per thread).
 * On the HOST: the skip rule and the circular kinds (line-sized), `best` of every voted cell, a.lines.src, and the last argument checks.
 *
 * DEPENDENCY ON THE C++ LIBRARY.  best = the first id after ReverseSortSync(cov, ids) (VecUtilities.h:349-405), which is std::sort on the
 *   index vector 0 .. n-1 with cov[i] > cov[j].  std::sort is not stable: among tied maxima the lowest index wins up to 16 paths
 *   (insertion sort) and need not from 17 (introsort's partition).  The host code of this call makes the same std::sort call on the same
 *   vector, so it gives the reference's tie order exactly when it is linked against the libstdc++ the reference was built with; the
 *   recorded runs (tests/golden/refruns/step7_ff_*) were made with the one this library is built against.  The votes themselves (cov)
 *   are counted on the device and do not depend on it.
 *
 * Semantics, in the reference's order.
 *   1. Line i is printed unless i > 0 and first_edge(line i-1) == inv[last_edge(line i)], first_edge = front()[0][0], last_edge =
 *      back()[0][0]: the rule reads the order AS GIVEN (after SortLines a line is followed by its mirror image).
 *   2. circular kind 1: more than one cell and first_edge == last_edge, the last cell is not written; kind 2: one cell and the edge's two
 *      vertices are one.  Either adds " circular" to both headers.
 *   3. A cell of ONE EMPTY path is a gap: 100 N in both texts.  Every other path is the Cat of its edges (the first whole, each further
 *      one from base K-1), shortened by K-1 bases unless the cell is the line's last; the cut may run back over several edges.
 *   4. The vote, odd cells only (best = 0 elsewhere), e = the first edge of the cell in front.  For every entry of the paths index of e
 *      and every position m of that read with p[m] == e, path r matches when p[m+1+s] == x[r][s] for every s still inside the read; the
 *      occurrence counts for r when it is the ONLY match.  The index lists a read once per occurrence and every entry visits every
 *      occurrence: a read through e twice counts four times.  The same over the index of inv[e], each read reversed and mapped by inv.
 *   5. efasta of a cell: one path its bases; several: left_share { middles joined by , } right_share, both shares against path 0 after
 *      the cut, right_share <= len(path 0) - left_share (efasta/EfastaTools.cc:35-71).
 *   6. Text: ">line_<i>[ circular]\n" / ">flattened_line_<i>[ circular]\n", i the index in the input, then rows of 80 characters, no empty
 *      last row, a body of 0 characters the header alone (efasta::Print).
 *   7. a.lines.src: every line, skipped ones too: cells joined by ",", an even cell its first edge, an odd one {{path},{path}}.
 *
 * W2RAP_E_ARG before the device is touched: K outside [16, 640]; an unknown flag; sizes beyond 32-bit ids; null arrays; edge_byte_off that
 * does not start at 0 or does not match edge_len (packed edges shorter than edge_len says); edge_len < K; adjacency, inv and path faults
 * as above; the line checks of w2rap_step7_links (w2rap_step7_in) but for "belongs to no line" (no tol is read here); an EVEN cell whose
 * first path is empty (the reference reads [0] of it); an empty path in a cell of two or more (the reference reads e[0] of an empty
 * vector); a path shorter than K-1 bases where the cut applies -- behind edge_len >= K no path with an edge is, so this guards the
 * kernels only.  These three are refused in every line, printed or not.
 * W2RAP_E_LIMIT: a line of 2^31 K-mers or more; a line body of 2^32 characters or more in either text (Print counts in unsigned).
 */
#define W2RAP_STEP7_FASTA   1u
#define W2RAP_STEP7_EFASTA  2u
#define W2RAP_STEP7_SRC     4u
#define W2RAP_STEP7_VOTE_ROW 64      /* paths of a cell whose votes a wavefront keeps in LDS; larger cells count in global memory */
#define W2RAP_STEP7_GAP_N    100     /* N per gap cell */

typedef struct w2rap_step7_fasta_in {
    int32_t  K;
    uint64_t n_edge_objs;
    const uint8_t*  edge_packed;     /* as w2rap_gfa_in: each object ceil(len/4) bytes, base i at bits 2*(i%4) of byte i/4 */
    const uint64_t* edge_byte_off;   /* [n_edge_objs+1] */
    const uint32_t* edge_len;        /* [n_edge_objs] bases, >= K */
    uint64_t n_vertices;
    const uint64_t* from_off;        /* the adjacency, inv and the read paths as w2rap_step7_in (n_paths may be odd: no mates here) */
    const int32_t*  from_v;
    const int32_t*  from_e;
    const uint64_t* to_off;
    const int32_t*  to_e;
    const int32_t*  inv;
    uint64_t n_paths;
    const uint64_t* path_off;
    const int32_t*  path_edges;
    uint64_t n_lines;                /* the lines as w2rap_step7_in */
    const uint64_t* line_off;
    const uint64_t* cell_off;
    const uint64_t* lpath_off;
    const int32_t*  line_edges;
} w2rap_step7_fasta_in;

typedef struct w2rap_step7_fasta_params {
    int32_t  device;
    uint32_t flags;                  /* any of W2RAP_STEP7_FASTA / EFASTA / SRC, 0 = all three */
} w2rap_step7_fasta_params;

/* library-allocated HOST memory, free with w2rap_step7_line_files_free.  A part that is not asked for launches no kernel of its own and
 * leaves its pointers null, its counters and its time zero: the vote runs for FASTA, the shares for EFASTA; printed and the line
 * counters come back with any part */
typedef struct w2rap_step7_fasta_out {
    char*    fasta;  uint64_t fasta_len;         /* a.lines.fasta */
    char*    efasta; uint64_t efasta_len;        /* a.lines.efasta */
    char*    src;    uint64_t src_len;           /* a.lines.src */
    uint8_t*  printed;               /* [n_lines] */
    int32_t*  best;                  /* [n_cells]  FASTA: the path flattened, 0 where no vote is taken */
    uint32_t* cov;                   /* [n_lpaths] FASTA: the votes of every path of every voted cell (cell_off is its CSR), 0 elsewhere */
    uint32_t* left_share;            /* [n_cells]  EFASTA: of the written cells of two or more paths, 0 elsewhere */
    uint32_t* right_share;           /* [n_cells] */
    uint64_t n_printed, n_skipped, n_circular1, n_circular2;     /* lines (circular: of the printed) */
    uint64_t n_gap_cells;            /* written cells of one empty path */
    uint64_t n_cells_voted;          /* written odd cells that are no gap (cells of one path included) */
    uint64_t n_entries;              /* index entries visited, of e and of inv[e] over all voted cells */
    uint64_t n_occurrences;          /* positions with p[m] == e */
    uint64_t n_match_one, n_match_none, n_match_several;         /* of those: exactly one path matches (a vote), none, several */
    uint64_t n_cells_tied;           /* voted cells whose largest vote is shared by two or more paths */
    uint64_t n_cells_wide;           /* voted cells of more than W2RAP_STEP7_VOTE_ROW paths (no LDS row) */
    uint64_t n_pieces_fasta, n_pieces_efasta;                    /* pieces of the layout (those of no characters included) */
    float ms_vote, ms_share, ms_layout, ms_write;                /* device time per part, milliseconds (ms_vote: the index included) */
} w2rap_step7_fasta_out;

int  w2rap_step7_line_files(const w2rap_step7_fasta_in* in, const w2rap_step7_fasta_params* params, w2rap_step7_fasta_out* out, char* err, size_t errlen);
void w2rap_step7_line_files_free(w2rap_step7_fasta_out* out);
/* per-kernel device time of the last w2rap_step7_line_files in this process, as w2rap_step7_profile */
size_t w2rap_step7_line_files_profile(char* buf, size_t len);

/* ---- COVERAGE: ComputeCoverage (Lines.cc:442-624), what .covs, .lines.npairs and .lines.stats hang on, and CNIntegerFraction -------------
 *
 * FinalFiles.cc:40-50 calls it in Step 7 and w2rap-contigger.cc:528-536 in Step 6, where CNIntegerFraction (GapToyTools5.cc:1520-1538) turns
 * it into the `CN fraction good = ...` line.  ONE sample (subsam_starts = {0}): the reference's main never has more than one.
 *
 * What runs where.  HIP kernels for gfx950:
 *   npairs, llens          the LINES kernels of w2rap_step7_links (k7_path_len, k7_line_stats, k7_pair_lines), unchanged, where they lie
 *   the paths index        k5o_index_emit, the radix sort, k5o_lower_bound (step5_runs.h); built only when a group or a long edge needs it
 *   distinct pairs         of a GROUP of edges = the distinct read / 2 over the index rows of every e of the group and of every inv[e] (Pids,
 *                          Lines.cc:390-404): k7c_row_len (a thread per (group edge, pass)), a scan, k7c_emit (a thread per index entry: key
 *                          group << pbits | pid), ONE stable radix sort on bits_for(groups) + bits_for(pairs) bits, head flags and their scan
 *                          (k5_heads), k5o_lower_bound for the groups' first keys, k7c_group_count (differences of the scanned flags).  No
 *                          atomic on a shared address.  The cell groups (one per (in, out) class, Lines.cc:591-604) go through it first, the long
 *                          edges (one edge each, :619-624) in a second round, because the long-edge rule reads what the cell rule left; they take the
 *                          sort-free form described at the end of this text unless the sorted one is asked for.
 *   the E-sized rules      k7c_line_pos (a thread per line: the loop position of the last even cell that names an edge as its first, atomicMax
 *                          per edge), k7c_cell_pos (a thread per edge of a z: the last group), k7c_edge_cov (a thread per edge: line rule, then
 *                          cell rule, and whether the long-edge rule is due), k7c_edge_long (the long-edge rule, the counts of CNIntegerFraction)
 * On the HOST (csrc/step7_peak.h, plain C++): covl, the candidates, their sort, mass, PeakFinder::FindPeaks and CN1PeakFinder::FindPeak,
 *   and the grouping of every cell's paths (io, ins, outs, pi, the upper median, z): line- or cell-sized and sequential in meaning.
 *
 * Semantics, in the reference's order.
 *   1. npairs, llens as part LINES.  covl[l] = double(npairs[l]) / double(llens[l]).
 *   2. Candidates: llens >= min(10000, max_len / 2) and covl > 0, sorted by covl (equal coverages by line id here, in no stated order in the
 *      reference: mass, and so base_cov, do not depend on it).  mass[i] = the llens of the contiguous window around i whose ends are found with
 *      covx[i] - covx[j] > 0.08 * covx[i] going down and covx[j] - covx[i] > 0.08 * covx[i] going up, in double, as written.
 *   3. base_cov = CN1PeakFinder::FindPeak(covx, mass): peaks are the first maximum of their 21 neighbours (so none below 21 candidates),
 *      not below max / 10000 (integer), with upper_bound windows of +-5% that do not touch either end of the data and hold 10 points on
 *      each side, the maximum of their window, and 1.2 x the deeper of the two troughs not above them; plateaus are centred; peaks above
 *      5 x the largest-mass peak go; one peak: it; none: the candidate of the largest mass (the first of equals); several: every peak is
 *      scored as CN1 (the half step for all but the first, then 2x .. 5x, each within 10%), the best score that uses the largest peak wins, a
 *      tie only for a diploid half-step peak of under a tenth of the mass.  At the end the larger of the first two chosen peaks decides: the
 *      second, halved, when it is larger.  No candidate: base_cov = 0, and every later quotient is what IEEE gives (inf or NaN).
 *   4. Line rule: for every line of llens >= 1000, every even cell j: cov[lines[l][j][0][0]] = float(covl[l] / base_cov).
 *   5. Cell rule: every odd cell with a non-empty first path, whose paths' (first, last) pairs, firsts and lasts are equally many and at
 *      least 2: per class of (first, last), len = the UPPER median of its paths' K-mers (v[n / 2]); len >= 1000: c = double(distinct pairs of
 *      the class's edges) / double(len), and cov[z] = float(c / base_cov) for every edge z that every path of the class holds.
 *   6. Long-edge rule: every edge with !(cov >= 0) (NaN is undefined: Def() is cov_ >= 0) and Kmers >= 1000:
 *      cov = float(double(distinct pairs of e) / double(Kmers(e)) / base_cov).
 *   Later writes win: a later cell over an earlier one, the cell rule over the line rule; rule[e] = the rule that wrote last
 *   (W2RAP_STEP7_RULE_*).  There is ONE rounding to float, at Set.
 *   7. CNIntegerFraction(frac, min_edge_size): over the edges of min_edge_size BASES or more with cov >= 0: int_cov = int(double(cov) + 0.5)
 *      (a cov of 2^31 or more -- inf with base_cov 0 -- is the reference's undefined behaviour; here int_cov saturates), good when
 *      |int_cov - cov| <= frac in double.  cn_fraction = double(good) / double(counted): NaN when nothing is counted.
 *
 * W2RAP_E_ARG before the device is touched: K outside [16, 640]; an unknown flag; negative or NaN frac, negative min_edge_size; sizes beyond
 * 32-bit ids; an odd n_paths; null arrays; NO LINES (the reference dereferences the end of an empty vector); edge_len < K; inv that is no
 * involution; path and line faults as w2rap_step7_links (an edge out of range, an even number of cells, an edge object in no line, ...); an
 * even cell whose first path is empty.  W2RAP_E_LIMIT: a line of 2^31 K-mers or more.
 * A cell that holds an empty path behind its first one (the reference reads front() of it) forms no group and counts as n_cells_empty.
 *
 * WHAT IS PINNED BY WHAT.  Recorded runs of the reference's own main (tests/golden/refruns/step7_cov_*, `--from_step 7`, at 1 thread and at 4):
 *   .covs bit for bit, .lines.stats byte for byte and .lines.npairs for lone contigs below 21 candidates (the largest mass), 20 and 22
 *   candidates, one peak of 80 lines (a single peak), two peaks of 120 lines with and without a far outlier (scored, the second halved), a line
 *   below min_len, no pairs at all and pairs on a short line only (base_cov 0: NaN and inf), bubbles of 999 / 1,000 / 1,001 K-mers (the cell rule
 *   on either side of 1000), classes of two and of four parallel paths (the upper median), a shared first edge of 1,000 and of 999 K-mers (the
 *   long-edge rule on either side), reads with both mates on one edge, on e and inv[e], through e twice, with an unplaced mate.  Step-6 runs
 *   (step7_cn_*) of the three Step-4 fixtures and of a hand-staged input of eight isolated contigs: the `CN fraction good` line, a `-nan` among them.
 *   On the MODEL only (tests/step7_cov_model.py, a loop-for-loop restatement, and literal outcomes derived by hand): the overwrite order of
 *   hand-written lines, a cell named twice, e and inv[e] in one group, an edge that is its own inverse (and the odd candidate count it gives:
 *   21), index rows of 0 .. 257 entries, 1 .. 257 groups, a group of 20 edges, gap cells, the prefilter at 5x (no record reaches it), frac and
 *   min_edge_size other than the defaults.  The diploid tie of the scoring is reached by no case: it rests on the text.
 * WHICH FORMS OF THE ARITHMETIC THE RECORDS CHOSE (the reference is built with -Ofast):
 *   - `x / base_cov` is a DIVISION in all three rules, not x * (1.0 / base_cov): the record `reciprocal` holds a line found by search
 *     (2,839 pairs on 1,024 K-mers over base_cov 512 / 9,907: 53.64603805541992 as written, 53.646034240722656 by the reciprocal) under the
 *     line rule, the cell rule and the long-edge rule, and the recorded .covs has the first value six times.
 *   - abs(int_cov - frac_cov) in CNIntegerFraction is the FLOATING function: the integer one truncates every difference to 0 and would print 1
 *     where the record of repeats_snps prints 0.8 (16 of 20) and the hand-staged input with copy numbers of 1.3, 2.3 and 0.7 (step7_cn_hand) 0.625 (10 of 16).
 *   - Median(lens) is the upper median (the record parallel_4: 1,140 of 1,100, 1,110, 1,140, 1,150).
 *   - A NaN is stored in .covs as ffc00000 (x86-64's default NaN, sign bit set), and the library stores that pattern whatever the device gives;
 *     a NaN of 0 / 0 in cn_fraction prints as `-nan`.
 *   - In .lines.stats a NaN prints as ` cov=?x`: under -Ofast the first `covs[ss][e].Def()` of WriteLineStats holds for a NaN and the second
 *     does not (record no_pairs); -1 prints nothing and inf prints `cov=infx` (step7.line_stats_text).
 * THE TWO FORMS OF THE LONG EDGES' COUNT.  A group of one edge needs no sort: an index row ascends in read id, so its distinct pairs are the
 *   entries that open a pair, and the group's count is those of row e, plus those of row inv[e], minus the pairs in both (k7c_single_flag: a
 *   thread per entry, a binary search into the other row; then a scan and k7c_single_count).  Measured against the sorted form on the 2,000
 *   long edges (198,440 index entries) of tools/step7_time.py --coverage, both forms in turn in one process, two processes on an MI355X
 *   (profiles/step7_coverage_generated_4M.json, _process2.json): sorted 0.295-0.312 ms, sort-free 0.132-0.137 ms of device time for that
 *   round; the two processes differ by 0.016 ms at most.  The sort-free form is ahead by ten times that and is the default
 *   (W2RAP_STEP7_LONG_DEFAULT); the cell groups, of several edges, keep the one radix sort.  tests/test_gpu_step7_cov.py holds the two forms
 *   to each other and to Pids.
 */
#define W2RAP_STEP7_COV_NPAIRS 1u    /* npairs, llens */
#define W2RAP_STEP7_COV_PEAK   2u    /* + covl, the candidates, base_cov */
#define W2RAP_STEP7_COV_EDGES  4u    /* + cov, rule, the cell groups, the CN counts (the paths index only here) */

#define W2RAP_STEP7_LONG_DEFAULT   0u  /* the library's choice: the sort-free form (the measurement is in the text above) */
#define W2RAP_STEP7_LONG_SORTED    1u  /* keys and the radix sort, as the cell groups */
#define W2RAP_STEP7_LONG_SORT_FREE 2u  /* k7c_single_flag: pairs of row e + pairs of row inv[e] - pairs in both, by binary search */

#define W2RAP_STEP7_RULE_NONE 0
#define W2RAP_STEP7_RULE_LINE 1
#define W2RAP_STEP7_RULE_CELL 2
#define W2RAP_STEP7_RULE_LONG 3

#define W2RAP_STEP7_PEAK_NO_DATA      0   /* no candidate: base_cov 0 */
#define W2RAP_STEP7_PEAK_SINGLE       1
#define W2RAP_STEP7_PEAK_LARGEST_MASS 2   /* no peak (always below 21 candidates) */
#define W2RAP_STEP7_PEAK_SCORED       3

typedef struct w2rap_step7_cov_in {
    int32_t  K;
    uint64_t n_edge_objs;
    const uint32_t* edge_len;        /* [n_edge_objs] bases, >= K; Kmers(e) = edge_len[e] - K + 1 */
    const int32_t*  inv;             /* [n_edge_objs] */
    uint64_t n_paths;                /* even */
    const uint64_t* path_off;        /* [n_paths+1] */
    const int32_t*  path_edges;
    uint64_t n_lines;                /* the lines as w2rap_step7_in; at least one */
    const uint64_t* line_off;
    const uint64_t* cell_off;
    const uint64_t* lpath_off;
    const int32_t*  line_edges;
} w2rap_step7_cov_in;

typedef struct w2rap_step7_cov_params {
    int32_t  device;
    uint32_t flags;                  /* the highest W2RAP_STEP7_COV_* asked for decides (a part needs those before it); 0 = everything */
    double   frac;                   /* CNIntegerFraction: the reference's default 0.1 */
    int32_t  min_edge_size;          /* bases; the reference's default 2000 */
    uint32_t long_form;              /* how the long edges' pairs are counted: W2RAP_STEP7_LONG_* (both give the same counts) */
} w2rap_step7_cov_params;

/* library-allocated HOST memory, free with w2rap_step7_coverage_free; a part that is not asked for leaves its pointers null and its counters zero */
typedef struct w2rap_step7_cov_out {
    int32_t* npairs;                 /* [n_lines] */
    int32_t* llens;                  /* [n_lines] */
    double*  covl;                   /* [n_lines]  PEAK */
    double*  covx;                   /* [n_candidates] sorted */
    int64_t* mass;                   /* [n_candidates] */
    int32_t* ids;                    /* [n_candidates] */
    float*   cov;                    /* [n_edge_objs] EDGES: -1 undefined; what .covs holds */
    uint8_t* rule;                   /* [n_edge_objs] W2RAP_STEP7_RULE_* */
    int32_t* group_line;             /* [n_groups] one record per qualifying class of a cell, in the reference's loop order */
    int32_t* group_cell;             /* the cell's position in its line */
    int32_t* group_len;              /* the upper median */
    int64_t* group_pairs;            /* distinct pairs */
    uint64_t* group_z_off;           /* [n_groups+1] into group_z */
    int32_t* group_z;
    int32_t* long_edge;              /* [n_long_asked] the edges the long-edge rule counted pairs for, ascending */
    int64_t* long_pairs;             /* [n_long_asked] their distinct pairs */
    double   base_cov;
    double   cn_fraction;            /* double(n_cn_good) / double(n_cn_edges) */
    int32_t  max_len, min_len;
    uint64_t n_candidates, n_groups;
    uint64_t n_cn_edges, n_cn_good;
    /* the peak finder's branches (csrc/step7_peak.h) */
    uint64_t n_simple, n_noise, n_edge, n_sparse, n_not_window_max, n_shallow, n_centred, n_prefiltered, n_peaks, peak_way, n_score_ties_taken, halved;
    /* the cell rule's branches */
    uint64_t n_cells, n_cells_empty, n_cells_sizes, n_cells_one_in, n_classes, n_classes_short;
    /* the edge rules */
    uint64_t n_line_lines;           /* lines of llens >= 1000 */
    uint64_t n_rule[4];              /* edges per W2RAP_STEP7_RULE_* */
    uint64_t n_long_asked;           /* edges the long-edge rule counted pairs for */
    uint64_t n_undefined;            /* edges with !(cov >= 0) at the end (NaN included) */
    uint64_t n_group_entries[2];     /* index entries sorted for the cell groups / for the long edges */
    uint64_t index_built;
    float ms_lines, ms_index, ms_groups, ms_rules;   /* device time per part, milliseconds */
    float ms_long;                   /* of ms_groups: the long edges' round */
} w2rap_step7_cov_out;

int  w2rap_step7_coverage(const w2rap_step7_cov_in* in, const w2rap_step7_cov_params* params, w2rap_step7_cov_out* out, char* err, size_t errlen);
void w2rap_step7_coverage_free(w2rap_step7_cov_out* out);
/* the per-kernel device time of the last w2rap_step7_coverage comes from w2rap_step7_profile (the LINES kernels are in it) */

#ifdef __cplusplus
}
#endif
#endif /* W2RAP_STEP7_H_ */
