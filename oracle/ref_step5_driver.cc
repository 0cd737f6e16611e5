// oracle/ref_step5_driver.cc -- TEST INFRASTRUCTURE, not product code.
//
// Runs two pieces of the UNMODIFIED reference's Step 5 on hand-made inputs, each through the reference's own public function, with the
// files read and written as its main() reads and writes them (src/modules/w2rap-contigger.cc:415-455):
//
//   ref_step5 partners <dir> [threads=1]
//       reads  <dir>/t.hbv, t.paths, frag_reads_orig.fastb, frag_reads_orig.qualp
//       calls  PartnersToEnds(hbv, paths, bases, quals)                              (paths/long/large/GapToyTools.h)
//       writes <dir>/t.out.paths with WriteReadPathVec
//
//   ref_step5 open <dir> [threads=1]
//       reads  <dir>/t.hbv, t.paths, frag_reads_orig.fastb (only the read sizes are used) and t.inv: text, one integer per edge
//              object -- the case's own involution; hbv.Involution is NOT called (the cases' edges hold no real sequence)
//       calls  invert(paths, paths_inv, hbv.EdgeObjectCount())                       (VecUtilities.h)
//              LayoutReads(hbv, inv, bases, paths, layout_pos, layout_id, layout_or) (paths/long/large/GapToyTools.h)
//       writes <dir>/t.index.txt   one line per edge object: the read ids of paths_inv[e], blank separated
//              <dir>/t.layout.txt  one line per edge object: "pos id or" triples, blank separated, in the order LayoutReads left them
//
// No reference source is copied; this file only includes and calls the reference's public functions.  Built by oracle/Makefile into
// oracle/_ref/ref_step5 (gitignored).
#include <omp.h>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "Basevector.h"
#include "VecUtilities.h"
#include "feudal/BinaryStream.h"
#include "Intvector.h"
#include "feudal/PQVec.h"
#include "paths/HyperBasevector.h"
#include "paths/long/ReadPath.h"
#include "paths/long/large/GapToyTools.h"
#include "system/SysConf.h"

int main(int argc, char** argv) {
    if (argc < 3) { std::cerr << "usage: ref_step5 partners|open dir [threads]\n"; return 2; }
    std::string mode = argv[1], dir = argv[2];
    int threads = argc > 3 ? atoi(argv[3]) : 1;
    configNumThreads(threads);                       // the thread pools of MapReduceEngine (SetThreads, DiscovarTools.cc:480-481)
    omp_set_num_threads(threads);
    HyperBasevector hbv; ReadPathVec paths; vecbvec bases;
    BinaryReader::readFile(dir + "/t.hbv", &hbv);
    LoadReadPathVec(paths, (dir + "/t.paths").c_str());
    bases.ReadAll(dir + "/frag_reads_orig.fastb");
    if (mode == "partners") {
        VecPQVec quals;
        quals.ReadAll(dir + "/frag_reads_orig.qualp");
        PartnersToEnds(hbv, paths, bases, quals);
        WriteReadPathVec(paths, (dir + "/t.out.paths").c_str());
        std::cout << "REF_STEP5 partners edges " << hbv.EdgeObjectCount() << " paths " << paths.size() << std::endl;
        return 0;
    }
    if (mode == "open") {
        vec<int> inv;
        {   std::ifstream in((dir + "/t.inv").c_str());
            int x;
            while (in >> x) inv.push_back(x); }
        if (inv.isize() != hbv.EdgeObjectCount()) { std::cerr << "ref_step5: t.inv does not have one integer per edge object\n"; return 2; }
        VecULongVec paths_inv;
        invert(paths, paths_inv, hbv.EdgeObjectCount());
        std::vector<std::vector<int>> pos; std::vector<std::vector<int64_t>> id; std::vector<std::vector<bool>> orient;
        LayoutReads(hbv, inv, bases, paths, pos, id, orient);
        std::ofstream fi((dir + "/t.index.txt").c_str()), fl((dir + "/t.layout.txt").c_str());
        for (int e = 0; e < hbv.EdgeObjectCount(); e++) {
            for (size_t j = 0; j < paths_inv[e].size(); j++) fi << (j ? " " : "") << paths_inv[e][j];
            fi << "\n";
            for (size_t j = 0; j < pos[e].size(); j++) fl << (j ? " " : "") << pos[e][j] << " " << id[e][j] << " " << (orient[e][j] ? 1 : 0);
            fl << "\n";
        }
        std::cout << "REF_STEP5 open edges " << hbv.EdgeObjectCount() << " paths " << paths.size() << std::endl;
        return 0;
    }
    std::cerr << "ref_step5: unknown mode " << mode << "\n";
    return 2;
}
