// oracle/ref_step7_driver.cc -- TEST INFRASTRUCTURE, not product code.
//
// Runs the read-sized passes of the UNMODIFIED reference's Step 7 on hand-made inputs, each through the reference's own public function.
// Both modes read <dir>/t.contig.hbv, t.contig.paths, t.fin.lines, t.fin.lines.npairs (MakeGaps reads the last two itself, as
// <dir>/t.fin.lines and <dir>/t.fin.lines.npairs) and t.inv: text, one integer per edge object -- the case's own involution;
// hbv.Involution is NOT called (the cases' edges hold no real sequence).
//
//   ref_step7 lines <dir> [threads=1]
//       calls  GetTol(hb, lines, tol), GetLineLengths(hb, lines, llens), GetLineNpairs(hb, inv, paths, lines, npairs)
//                                                                                     (paths/long/large/Lines.h)
//       writes <dir>/t.lines.txt: three lines of integers, blank separated -- tol (one per edge object), llens and npairs (one per line)
//
//   ref_step7 gaps <dir> [threads=1] [min_line=5000] [min_link_count=3] [verbose=1]
//       calls  invert(paths, paths_inv, hb.EdgeObjectCount())                          (VecUtilities.h)
//              MakeGaps(hb, inv, paths, paths_inv, min_line, min_link_count, dir, "t", verbose, False)
//                                                                                     (paths/long/large/MakeGaps.h)
//       With GAP_CLEANUP False MakeGaps leaves the graph with one empty edge per accepted gap appended behind the old edges, in the
//       order of its final list: gap i is the edge nold + i between two NEW vertices; its left vertex has one in-edge, the gap's e1, its
//       right vertex one out-edge, the gap's e2, and inv[nold + i] - nold is the index of the gap's mirror image.
//       writes <dir>/t.gaps.txt: one line "e1 e2 mirror_index" per appended edge, read from the edited graph;
//              stdout is MakeGaps' own (with verbose: every accepted link, its lines, nears and edge groups, the one-to-one deletions)
//       refuses (exit 3, nothing written) when an appended edge's left vertex does not have exactly one in-edge or its right vertex
//       exactly one out-edge
//
// No reference source is copied; this file only includes and calls the reference's public functions.  Built by oracle/Makefile into
// oracle/_ref/ref_step7 (gitignored).
#include <omp.h>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "Basevector.h"
#include "VecUtilities.h"
#include "feudal/BinaryStream.h"
#include "Intvector.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "paths/long/large/Lines.h"
#include "paths/long/large/MakeGaps.h"
#include "system/SysConf.h"

static void write_row(std::ofstream& f, const vec<int>& v) {
    for (int i = 0; i < v.isize(); i++) f << (i ? " " : "") << v[i];
    f << "\n";
}

int main(int argc, char** argv) {
    if (argc < 3) { std::cerr << "usage: ref_step7 lines|gaps dir [threads] [min_line] [min_link_count] [verbose]\n"; return 2; }
    const std::string mode = argv[1], dir = argv[2];
    if (mode != "lines" && mode != "gaps") { std::cerr << "ref_step7: unknown mode " << mode << "\n"; return 2; }
    const int threads = argc > 3 ? atoi(argv[3]) : 1;
    configNumThreads(threads);                       // the thread pools of MapReduceEngine (SetThreads, DiscovarTools.cc:480-481)
    omp_set_num_threads(threads);
    HyperBasevector hb; ReadPathVec paths; vec<int> inv; vec<vec<vec<vec<int>>>> lines;
    BinaryReader::readFile(dir + "/t.contig.hbv", &hb);
    LoadReadPathVec(paths, (dir + "/t.contig.paths").c_str());
    BinaryReader::readFile(dir + "/t.fin.lines", &lines);
    {   std::ifstream in((dir + "/t.inv").c_str());
        int x;
        while (in >> x) inv.push_back(x); }
    if (inv.isize() != hb.EdgeObjectCount()) { std::cerr << "ref_step7: t.inv does not have one integer per edge object\n"; return 2; }
    if (mode == "lines") {
        vec<int> tol, llens, npairs;
        GetTol(hb, lines, tol);
        GetLineLengths(hb, lines, llens);
        GetLineNpairs(hb, inv, paths, lines, npairs);
        std::ofstream f((dir + "/t.lines.txt").c_str());
        write_row(f, tol); write_row(f, llens); write_row(f, npairs);
        std::cout << "REF_STEP7 lines edges " << hb.EdgeObjectCount() << " lines " << lines.size() << " paths " << paths.size() << std::endl;
        return 0;
    }
    const int min_line = argc > 4 ? atoi(argv[4]) : 5000, min_link_count = argc > 5 ? atoi(argv[5]) : 3;
    const Bool verbose = argc > 6 ? (atoi(argv[6]) ? True : False) : True;
    VecULongVec paths_inv;
    invert(paths, paths_inv, hb.EdgeObjectCount());
    const int nold = hb.EdgeObjectCount();
    MakeGaps(hb, inv, paths, paths_inv, min_line, min_link_count, String(dir), String("t"), verbose, False);
    vec<int> to_left, to_right;
    hb.ToLeft(to_left); hb.ToRight(to_right);
    std::ostringstream out;
    for (int g = nold; g < hb.EdgeObjectCount(); g++) {
        const int v = to_left[g], w = to_right[g];
        if (hb.To(v).size() != 1 || hb.From(w).size() != 1) {
            std::cerr << "ref_step7: the appended edge " << g << " lies between a left vertex with " << hb.To(v).size() << " in-edges and a right vertex with "
                      << hb.From(w).size() << " out-edges: not one gap edge between two new vertices\n";
            return 3;
        }
        out << hb.ITo(v, 0) << " " << hb.IFrom(w, 0) << " " << inv[g] - nold << "\n";
    }
    std::ofstream f((dir + "/t.gaps.txt").c_str());
    f << out.str();
    return 0;
}
