// w2rap-step4 -- standalone Step 4 with the reference's file names and flags.
//
// Drop-in for `w2rap-contigger --from_step 4 --to_step 4` (src/modules/w2rap-contigger.cc:386-409): reads
// <out_dir>/<prefix>.large_K.{hbv,paths} written by Step 3 and <out_dir>/frag_reads_orig.{fastb,qualp} written by Step 1, writes
// <out_dir>/<prefix>.large_K.clean.{hbv,paths} that Step 5 (`--from_step 5`) loads.  The vote, the graph edit and the path rewrite
// run in libw2rap_step2.so (HIP); --host_edit runs the library's host edit instead (include/w2rap_step4.h).
//
//   w2rap-step4 -o <out_dir> -p <prefix> [-s min_size] [--device 0] [--host_edit]
//
// File layouts: include/w2rap_step4.h and w2rap_contigger_amd/formats.py.  Every count in the inputs is checked against the bytes
// that are there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "w2rap_step4.h"

namespace {

bool slurp(const std::string& path, std::vector<uint8_t>& buf) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    std::streamsize n = f.tellg();
    f.seekg(0);
    buf.resize((size_t)n);
    return n == 0 || (bool)f.read((char*)buf.data(), n);
}

// a BINWRITE .hbv (HyperBasevector::writeBinary, paths/HyperBasevector.cc:121-125): K, from_, from_edge_obj_, to_edge_obj_, edges_
struct Hbv {
    int32_t K = 0;
    uint64_t n_vertices = 0;
    std::vector<uint64_t> off[3]; std::vector<int32_t> val[3];          // from_, from_edge_obj_, to_edge_obj_ as CSR
    std::vector<uint8_t> packed; std::vector<uint64_t> byte_off{0}; std::vector<uint32_t> len;
    bool load(const std::string& path, std::string& err) {
        std::vector<uint8_t> hb;
        if (!slurp(path, hb) || hb.size() < 12 || std::memcmp(hb.data(), "BINWRITE", 8)) { err = "cannot read " + path + " (not a BINWRITE .hbv)"; return false; }
        std::memcpy(&K, &hb[8], 4);
        size_t p = 12;
        auto need = [&](uint64_t bytes) { return bytes <= hb.size() - p; };
        for (int t = 0; t < 3; ++t) {
            if (!need(8)) goto bad;
            { uint64_t nv; std::memcpy(&nv, &hb[p], 8); p += 8;
              if (t == 0) n_vertices = nv; else if (nv != n_vertices) goto bad;
              off[t].assign(1, 0);
              for (uint64_t v = 0; v < nv; ++v) {
                  if (!need(8)) goto bad;
                  uint64_t d; std::memcpy(&d, &hb[p], 8); p += 8;
                  if (d > (hb.size() - p) / 4) goto bad;
                  const size_t at = val[t].size(); val[t].resize(at + d); if (d) std::memcpy(&val[t][at], &hb[p], 4 * d);
                  p += 4 * d; off[t].push_back(val[t].size());
              } }
        }
        if (off[0] != off[1]) goto bad;
        if (!need(8)) goto bad;
        { uint64_t E; std::memcpy(&E, &hb[p], 8); p += 8;
          for (uint64_t e = 0; e < E; ++e) {
              if (!need(4)) goto bad;
              uint32_t nb; std::memcpy(&nb, &hb[p], 4); p += 4;
              const size_t nby = ((size_t)nb + 3) / 4;
              if (!need(nby)) goto bad;
              packed.insert(packed.end(), hb.begin() + p, hb.begin() + p + nby); p += nby;
              byte_off.push_back(packed.size()); len.push_back(nb);
          } }
        if (p != hb.size()) goto bad;
        return true;
    bad:
        err = "cannot read " + path + ": truncated or not a .hbv file";
        return false;
    }
};

// a single-file feudal container (feudal/FeudalControlBlock.h:157-166): -> element offsets into `var`, the fixed section
bool load_feudal(const std::string& path, std::vector<uint8_t>& buf, uint64_t& n, uint64_t& var_off, uint64_t& fixed_off, std::string& err) {
    if (!slurp(path, buf) || buf.size() < 24) { err = "cannot read " + path; return false; }
    uint32_t n32; std::memcpy(&n32, &buf[0], 4);
    std::memcpy(&var_off, &buf[8], 8); std::memcpy(&fixed_off, &buf[16], 8);
    if ((buf[4] & 3) != 1 || var_off < 24 || var_off > buf.size() || fixed_off < var_off || fixed_off > buf.size() || (fixed_off - var_off) % 8 || fixed_off - var_off < 8) {
        err = "cannot read " + path + ": not a single-file feudal file, or truncated"; return false;
    }
    n = (fixed_off - var_off) / 8 - 1;
    if ((uint32_t)n != n32) { err = "cannot read " + path + ": element count mismatch"; return false; }
    uint64_t prev = 24;
    for (uint64_t i = 0; i <= n; ++i) {
        uint64_t o; std::memcpy(&o, &buf[var_off + 8 * i], 8);
        if (o < prev || o > var_off) { err = "cannot read " + path + ": element offsets out of range"; return false; }
        prev = o;
    }
    return true;
}

void put(std::vector<uint8_t>& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
template <class T> void put(std::vector<uint8_t>& b, T v) { put(b, &v, sizeof(T)); }
void put_csr(std::vector<uint8_t>& b, uint64_t nv, const uint64_t* off, const int32_t* vals) {
    put<uint64_t>(b, nv);
    for (uint64_t v = 0; v < nv; ++v) { put<uint64_t>(b, off[v + 1] - off[v]); put(b, vals + off[v], (off[v + 1] - off[v]) * 4); }
}

}  // namespace

int main(int argc, char** argv) {
    std::string out_dir, prefix;
    w2rap_step4_params P{};
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-o" || a == "--out_dir") out_dir = next();
        else if (a == "-p" || a == "--prefix") prefix = next();
        else if (a == "-s" || a == "--min_size") P.min_size = (uint32_t)std::atoi(next());
        else if (a == "--device") P.device = std::atoi(next());
        else if (a == "--host_edit") P.flags |= W2RAP_STEP4_EDIT_ON_HOST;
        else if (a == "-t" || a == "-m" || a == "-d" || a == "--disk_batches" || a == "--tmp_dir" || a == "-r" || a == "-K" || a == "--large_k") next();   // accepted, unused
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (out_dir.empty() || prefix.empty()) { std::fprintf(stderr, "usage: w2rap-step4 -o out_dir -p prefix [-s min_size] [--device d] [--host_edit]\n"); return 2; }
    std::string err;
    Hbv hb;
    if (!hb.load(out_dir + "/" + prefix + ".large_K.hbv", err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    std::vector<uint8_t> pb;
    const std::string ppath = out_dir + "/" + prefix + ".large_K.paths";
    if (!slurp(ppath, pb) || pb.size() < 8) { std::fprintf(stderr, "cannot read %s\n", ppath.c_str()); return 1; }
    uint64_t n; std::memcpy(&n, pb.data(), 8);
    std::vector<int32_t> p_offset; std::vector<uint64_t> p_off{0}; std::vector<int32_t> p_edges;
    {
        size_t p = 8;
        for (uint64_t r = 0; r < n; ++r) {
            if (pb.size() - p < 6) { std::fprintf(stderr, "cannot read %s: truncated\n", ppath.c_str()); return 1; }
            int32_t o; uint16_t l; std::memcpy(&o, &pb[p], 4); std::memcpy(&l, &pb[p + 4], 2); p += 6;
            if ((pb.size() - p) / 4 < l) { std::fprintf(stderr, "cannot read %s: truncated\n", ppath.c_str()); return 1; }
            p_offset.push_back(o);
            for (unsigned j = 0; j < l; ++j) { int32_t e; std::memcpy(&e, &pb[p + 4 * j], 4); p_edges.push_back(e); }
            p += 4 * (size_t)l; p_off.push_back(p_edges.size());
        }
        if (p != pb.size()) { std::fprintf(stderr, "cannot read %s: trailing bytes\n", ppath.c_str()); return 1; }
    }
    // frag_reads_orig.fastb: ceil(len/4) bytes per read, n u32 lengths in the fixed section
    std::vector<uint8_t> fb; uint64_t nr = 0, vo = 0, fo = 0;
    const std::string bpath = out_dir + "/frag_reads_orig.fastb", qpath = out_dir + "/frag_reads_orig.qualp";
    if (!load_feudal(bpath, fb, nr, vo, fo, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    if (fb.size() - fo != 4 * nr) { std::fprintf(stderr, "cannot read %s: the fixed section is not one u32 per read\n", bpath.c_str()); return 1; }
    std::vector<uint64_t> r_boff(nr + 1); std::vector<uint32_t> r_len(nr);
    for (uint64_t i = 0; i <= nr; ++i) { uint64_t o; std::memcpy(&o, &fb[vo + 8 * i], 8); r_boff[i] = o - 24; }
    for (uint64_t i = 0; i < nr; ++i) {
        std::memcpy(&r_len[i], &fb[fo + 4 * i], 4);
        if (r_boff[i + 1] - r_boff[i] != ((uint64_t)r_len[i] + 3) / 4) { std::fprintf(stderr, "cannot read %s: read %llu: bytes do not match its length\n", bpath.c_str(), (unsigned long long)i); return 1; }
    }
    // frag_reads_orig.qualp: a PQVec byte string per read (feudal/PQVec.cc:129-188), unpacked here to a byte per base
    std::vector<uint8_t> qb; uint64_t nq = 0, qvo = 0, qfo = 0;
    if (!load_feudal(qpath, qb, nq, qvo, qfo, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    if (nq != nr) { std::fprintf(stderr, "%s holds %llu reads, %s %llu\n", qpath.c_str(), (unsigned long long)nq, bpath.c_str(), (unsigned long long)nr); return 1; }
    if (nr != n) { std::fprintf(stderr, "%s holds %llu paths, %s %llu reads\n", ppath.c_str(), (unsigned long long)n, bpath.c_str(), (unsigned long long)nr); return 1; }
    std::vector<uint8_t> quals; std::vector<uint64_t> q_off(nr + 1, 0);
    for (uint64_t i = 0; i < nr; ++i) {
        uint64_t a, b; std::memcpy(&a, &qb[qvo + 8 * i], 8); std::memcpy(&b, &qb[qvo + 8 * (i + 1)], 8);
        size_t p = a; bool ended = false;
        while (p < b) {
            const unsigned nqs = qb[p++];
            if (!nqs) { ended = true; break; }
            if (p >= b) break;
            const unsigned nbits = qb[p] & 7;
            const size_t nbytes = ((size_t)nqs * nbits + 9 + 7) / 8;
            if (nbytes > b - p) break;
            uint64_t acc = 0; unsigned have = 0; size_t q = p;
            auto take = [&](unsigned k) { while (have < k) { acc |= (uint64_t)(q < p + nbytes ? qb[q] : 0) << have; ++q; have += 8; } const uint64_t v = acc & ((1ull << k) - 1); acc >>= k; have -= k; return (unsigned)v; };
            take(3); const unsigned mn = take(6);
            for (unsigned k = 0; k < nqs; ++k) quals.push_back((uint8_t)(mn + (nbits ? take(nbits) : 0)));
            p += nbytes;
        }
        q_off[i + 1] = quals.size();
        if (!ended || q_off[i + 1] - q_off[i] != r_len[i]) { std::fprintf(stderr, "cannot read %s: read %llu: qualities truncated or not one per base\n", qpath.c_str(), (unsigned long long)i); return 1; }
    }
    std::printf("--== Step 4: Cleaning graph ==--\n");
    w2rap_step4_in I{};
    I.K = hb.K; I.n_edge_objs = hb.len.size(); I.edge_packed = hb.packed.data(); I.edge_byte_off = hb.byte_off.data(); I.edge_len = hb.len.data();
    I.n_vertices = hb.n_vertices; I.from_off = hb.off[0].data(); I.from_v = hb.val[0].data(); I.from_e = hb.val[1].data(); I.to_off = hb.off[2].data(); I.to_e = hb.val[2].data();
    I.n_paths = n; I.path_offset = p_offset.data(); I.path_off = p_off.data(); I.path_edges = p_edges.data();
    I.n_reads = nr; I.read_packed = fb.data() + 24; I.read_byte_off = r_boff.data(); I.read_len = r_len.data(); I.quals = quals.data(); I.qual_off = q_off.data();
    w2rap_step4_out O{};
    char ebuf[1024] = {0};
    int rc = w2rap_step4_run(&I, &P, &O, ebuf, sizeof ebuf);
    if (rc) { std::fprintf(stderr, "w2rap_step4_run failed (%d): %s\n", rc, ebuf); return 1; }
    for (int k = 0; k < 2; ++k)
        std::printf("pass %d: %llu edges deleted, %llu runs merged; GPU ms: index %.2f vote %.2f paths %.2f; host ms in the graph edit: %.2f\n", k + 1, (unsigned long long)O.n_deleted[k],
                    (unsigned long long)O.n_runs_merged[k], O.ms_index[k], O.ms_vote[k], O.ms_paths[k], O.ms_graph_edit_host[k]);
    std::printf("%llu branch vertices, %llu skipped (too many walks), %llu placements\n", (unsigned long long)O.n_branch_vertices, (unsigned long long)O.n_skipped_too_many_exts,
                (unsigned long long)O.n_placements);
    std::vector<uint8_t> b;
    put(b, "BINWRITE", 8); put<int32_t>(b, O.K);
    put_csr(b, O.n_vertices, O.from_off, O.from_v);
    put_csr(b, O.n_vertices, O.from_off, O.from_e);
    put_csr(b, O.n_vertices, O.to_off, O.to_e);
    put<uint64_t>(b, O.n_edge_objs);
    for (uint64_t e = 0; e < O.n_edge_objs; ++e) { put<uint32_t>(b, O.edge_len[e]); put(b, O.edge_packed + O.edge_byte_off[e], O.edge_byte_off[e + 1] - O.edge_byte_off[e]); }
    { std::ofstream f(out_dir + "/" + prefix + ".large_K.clean.hbv", std::ios::binary); f.write((const char*)b.data(), (std::streamsize)b.size()); if (!f) { std::fprintf(stderr, "cannot write .hbv\n"); return 1; } }
    b.clear();
    put<uint64_t>(b, O.n_paths);
    for (uint64_t r = 0; r < O.n_paths; ++r) {
        const uint64_t m = O.path_off[r + 1] - O.path_off[r];
        put<int32_t>(b, O.path_offset[r]); put<uint16_t>(b, (uint16_t)m); put(b, O.path_edges + O.path_off[r], m * 4);
    }
    { std::ofstream f(out_dir + "/" + prefix + ".large_K.clean.paths", std::ios::binary); f.write((const char*)b.data(), (std::streamsize)b.size()); if (!f) { std::fprintf(stderr, "cannot write .paths\n"); return 1; } }
    std::printf("Cleaning graph DONE!\n");
    w2rap_step4_free(&O);
    return 0;
}
