// oracle/ref_step5_driver.cc -- TEST INFRASTRUCTURE, not product code.
//
// Runs pieces of the UNMODIFIED reference's Step 5 on hand-made inputs, each through the reference's own public function, with the
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
//   ref_step5 add <dir> [threads=1] [min_gain=5]
//       reads  <dir>/t.hbv, t.inv (text, as above), t.paths, frag_reads_orig.fastb, frag_reads_orig.qualp and new_stuff.fastb -- the
//              patches as the case has them: no encoding, no added reverse complements, repeats and entries below K kept
//       calls  AddNewStuff(new_stuff, hbv, inv, paths, bases, quals, min_gain, {}, dir, 1)  (paths/long/large/GapToyTools.h)
//       writes <dir>/t.out.hbv, t.out.paths and t.out.inv (text, one integer per line)
//
//   ref_step5 tail <dir> [threads=1] [min_gain=5]
//       for inputs AddNewStuff's own Validate refuses (two consecutive path edges that share no vertex): the second half of the call
//       reads  <dir>/t.hbv -- here the NEW graph --, t.map.txt: one line per old edge object, left3 and then the entries of to3,
//              t.paths (in old ids), frag_reads_orig.fastb, frag_reads_orig.qualp
//       calls  TranslatePaths(paths, hb3, to3, left3), then per read what AddNewStuff does: resize(1) if not empty and
//              ExtendPath(paths[i], i, hb3, to_right, bases[i], quals.begin()[i], min_gain, False, 1), to_right from hb3.ToRight
//       writes <dir>/t.out.paths
//
// No reference source is copied; this file only includes and calls the reference's public functions.  Built by oracle/Makefile into
// oracle/_ref/ref_step5 (gitignored).
#include <omp.h>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
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
    if (argc < 3) { std::cerr << "usage: ref_step5 partners|open|add|tail dir [threads] [min_gain]\n"; return 2; }
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
    const int min_gain = argc > 4 ? atoi(argv[4]) : 5;
    if (mode == "add") {
        VecPQVec quals; vecbvec new_stuff; vec<int> inv;
        quals.ReadAll(dir + "/frag_reads_orig.qualp");
        new_stuff.ReadAll(dir + "/new_stuff.fastb");
        {   std::ifstream in((dir + "/t.inv").c_str());
            int x;
            while (in >> x) inv.push_back(x); }
        if (inv.isize() != hbv.EdgeObjectCount()) { std::cerr << "ref_step5: t.inv does not have one integer per edge object\n"; return 2; }
        const int n_old = hbv.EdgeObjectCount();
        AddNewStuff(new_stuff, hbv, inv, paths, bases, quals, min_gain, vec<int>(), String(dir), 1);
        BinaryWriter::writeFile(dir + "/t.out.hbv", hbv);
        WriteReadPathVec(paths, (dir + "/t.out.paths").c_str());
        {   std::ofstream fo((dir + "/t.out.inv").c_str());
            for (int e = 0; e < inv.isize(); e++) fo << inv[e] << "\n"; }
        std::cout << "REF_STEP5 add old edges " << n_old << " new edges " << hbv.EdgeObjectCount() << " paths " << paths.size() << std::endl;
        return 0;
    }
    if (mode == "tail") {
        VecPQVec quals;
        quals.ReadAll(dir + "/frag_reads_orig.qualp");
        vec<vec<int>> to3; vec<int> left3;
        {   std::ifstream in((dir + "/t.map.txt").c_str());
            std::string line;
            while (std::getline(in, line)) {
                std::istringstream ls(line);
                int x;
                if (!(ls >> x)) { std::cerr << "ref_step5: a line of t.map.txt without left3\n"; return 2; }
                left3.push_back(x);
                to3.push_back(vec<int>());
                while (ls >> x) to3.back().push_back(x); } }
        for (size_t i = 0; i < paths.size(); i++)
            for (size_t j = 0; j < paths[i].size(); j++)
                if (paths[i][j] < 0 || paths[i][j] >= to3.isize()) { std::cerr << "ref_step5: a path names an edge t.map.txt does not hold\n"; return 2; }
        for (int e = 0; e < to3.isize(); e++)
            for (int j = 0; j < to3[e].isize(); j++)
                if (to3[e][j] < 0 || to3[e][j] >= hbv.EdgeObjectCount()) { std::cerr << "ref_step5: t.map.txt names an edge t.hbv does not hold\n"; return 2; }
        TranslatePaths(paths, hbv, to3, left3);
        vec<int> to_right;
        hbv.ToRight(to_right);
        #pragma omp parallel for
        for (int64_t i = 0; i < (int64_t)paths.size(); i++) {
            if (paths[i].size() > 0) paths[i].resize(1);
            ExtendPath(paths[i], i, hbv, to_right, bases[i], quals.begin()[i], min_gain, False, 1);
        }
        WriteReadPathVec(paths, (dir + "/t.out.paths").c_str());
        std::cout << "REF_STEP5 tail old edges " << to3.size() << " new edges " << hbv.EdgeObjectCount() << " paths " << paths.size() << std::endl;
        return 0;
    }
    std::cerr << "ref_step5: unknown mode " << mode << "\n";
    return 2;
}
