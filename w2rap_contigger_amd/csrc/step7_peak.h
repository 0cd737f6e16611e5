// step7_peak.h -- the line- and cell-sized parts of ComputeCoverage (src/paths/long/large/Lines.cc:442-624), restated in plain C++:
// host-only (no HIP header: a plain C++ compiler reads it, and it runs under a host sanitizer in tests/step7_cov_main.cc).
//
//   check            the argument checks of w2rap_step7_coverage (everything a kernel or a loop below uses as an index)
//   candidates       covl, min_len, the candidate lines, their sort and `mass`                      Lines.cc:483-536
//   find_peaks       PeakFinder<double, int64_t>::FindPeaks                                          util/PeakFinder.h
//   find_peak        CN1PeakFinder::FindPeak, PrefilterHighCNPeaks, MatchPeak, MaxPeak               paths/long/large/CN1PeakFinder.cc
//   cell_groups      the (in, out) classes of every odd cell, their upper median, e and z            Lines.cc:561-615
//
// Arithmetic: double wherever the reference has it; the expressions are written as the reference writes them and the library is built
// with -ffp-contract=off and without fast-math.  What -Ofast made of them in the recorded build is said in w2rap_step7.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <utility>
#include <vector>
#include "args.h"
#include "../../include/w2rap_step7.h"

namespace w2 {
namespace cov {

constexpr int MIN_LINE = 1000;                                // Lines.cc:448 (line rule, cell rule and long-edge rule alike)
constexpr double RADIUS = 0.08;                               // :504
constexpr size_t MIN_SHOULDER = 10;                           // PeakFinder.h:20
constexpr double WINDOW = 0.05;                               // :19
constexpr int64_t MIN_PEAK_RATIO = 10000;                     // :21
constexpr double MIN_PEAK_HEIGHT_RATIO = 1.2;                 // :22
constexpr uint64_t HIGH_CN_PREFILTER = 5;                     // CN1PeakFinder.h:27
constexpr double MAX_PEAK_TOLERANCE = 0.1;                    // :28
// `x / base_cov` in the loops of the three rules: true where the recorded build of the reference (-Ofast) multiplies by 1.0 / base_cov,
// computed once (tests/step7_cov_cases.py: the reciprocal search and the records that hold its lines)
constexpr bool RECIP_LINE = false, RECIP_CELL = false, RECIP_LONG = false;
// abs(int_cov - frac_cov) of CNIntegerFraction: the floating-point function (true) or the integer one, which truncates the difference to 0
constexpr bool ABS_FLOATING = true;

// ---- the argument checks: 0, or the code with the message in `err`
inline int check(const w2rap_step7_cov_in* in, const w2rap_step7_cov_params* P, char* err, size_t errlen) {
    auto fail = [&](int code, const char* m) { if (err && errlen) std::snprintf(err, errlen, "%s", m); return code; };
    if (!in || !P) return fail(W2RAP_E_ARG, "null argument");
    if (P->flags & ~(W2RAP_STEP7_COV_NPAIRS | W2RAP_STEP7_COV_PEAK | W2RAP_STEP7_COV_EDGES)) return fail(W2RAP_E_ARG, "unknown flag");
    if (in->K < 16 || in->K > 640) return fail(W2RAP_E_ARG, "K must be in [16, 640]");
    if (P->long_form > W2RAP_STEP7_LONG_SORT_FREE) return fail(W2RAP_E_ARG, "unknown long_form");
    if (!(P->frac >= 0) || P->min_edge_size < 0) return fail(W2RAP_E_ARG, "frac and min_edge_size must not be negative");
    if (in->n_edge_objs >= (1ull << 31) || in->n_paths >= args::READS_END) return fail(W2RAP_E_ARG, args::TOO_LARGE);
    if (in->n_paths & 1) return fail(W2RAP_E_ARG, args::ODD_PATHS);
    if (in->n_edge_objs && (!in->edge_len || !in->inv)) return fail(W2RAP_E_ARG, "null graph array");
    if (in->n_paths && !in->path_off) return fail(W2RAP_E_ARG, "null input array");
    if (!in->n_lines) return fail(W2RAP_E_ARG, "no lines: the reference takes the largest of no lengths");
    W2_ARGS(args::edge_lens(*in, 1ull << 31));
    W2_ARGS(args::involution(*in));
    W2_ARGS(args::reads_and_paths(*in));
    W2_ARGS(args::lines(*in));
    W2_ARGS(args::lines_cover(*in));
    W2_ARGS(args::line_lengths(*in));
    for (uint64_t l = 0; l < in->n_lines; ++l)                 // lines[l][j][0][0] of every even cell (Lines.cc:555)
        for (uint64_t cl = in->line_off[l]; cl < in->line_off[l + 1]; cl += 2) {
            const uint64_t p0 = in->cell_off[cl];
            if (in->lpath_off[p0 + 1] == in->lpath_off[p0]) return fail(W2RAP_E_ARG, "an even cell whose first path is empty");
        }
    return 0;
}

// ---- Lines.cc:483-536: the candidates as the peak finder sees them
struct Candidates {
    std::vector<double> covl;                                  // [NL]
    std::vector<double> covx; std::vector<int64_t> mass; std::vector<int32_t> ids;
    int32_t max_len = 0, min_len = 0;
};
inline void candidates(const int32_t* llens, const int32_t* npairs, uint64_t NL, Candidates& C) {
    C.covl.resize(NL);
    for (uint64_t l = 0; l < NL; ++l) C.covl[l] = double(npairs[l]) / double(llens[l]);
    C.max_len = *std::max_element(llens, llens + NL);
    C.min_len = std::min(10000, C.max_len / 2);
    std::vector<std::pair<double, int32_t>> v;
    for (uint64_t l = 0; l < NL; ++l) if (llens[l] >= C.min_len && C.covl[l] > 0) v.push_back(std::make_pair(C.covl[l], (int32_t)l));
    std::sort(v.begin(), v.end());                             // SortSync(covx, ids); equal coverages by id (the reference: in no stated order)
    const int64_t n = (int64_t)v.size();
    C.covx.resize(n); C.ids.resize(n); C.mass.resize(n);
    for (int64_t i = 0; i < n; ++i) { C.covx[i] = v[i].first; C.ids[i] = v[i].second; }
    const std::vector<double>& covx = C.covx;
    for (int64_t i = 0; i < n; ++i) {
        int64_t m = llens[C.ids[i]];
        for (int64_t j = i - 1; j >= 0; --j) { if (covx[i] - covx[j] > RADIUS * covx[i]) break; m += llens[C.ids[j]]; }
        for (int64_t j = i + 1; j < n; ++j) { if (covx[j] - covx[i] > RADIUS * covx[i]) break; m += llens[C.ids[j]]; }
        C.mass[i] = m;
    }
}

// ---- the peak finder.  The counters say which way a call went
struct PeakCounters {
    uint64_t n_simple = 0, n_noise = 0;                        // FindPeaks(y): peaks of the shoulder of 10; those below global_peak / 10000
    uint64_t n_edge = 0, n_sparse = 0, n_not_window_max = 0;   // FindPeaks(x, y): dropped at the edge of the data, for a thin window, for a larger point inside the window
    uint64_t n_shallow = 0, n_centred = 0;                     // the trough filter; plateaus whose peak moved
    uint64_t n_prefiltered = 0;                                // peaks above 5x the largest one
    uint64_t n_peaks = 0;                                      // what the scoring sees
    uint64_t way = 0;                                          // W2RAP_STEP7_PEAK_*
    uint64_t n_score_ties_taken = 0;                           // the diploid preference fired
    uint64_t halved = 0;                                       // the larger of the first two peaks was the second
};

inline std::vector<size_t> find_peaks_y(const std::vector<int64_t>& y, PeakCounters& n) {
    const int64_t global_peak = *std::max_element(y.begin(), y.end());
    std::vector<size_t> cand;
    if (y.size() > MIN_SHOULDER * 2)
        for (size_t it = MIN_SHOULDER; it < y.size() - MIN_SHOULDER; ++it) {
            const size_t peak = std::max_element(y.begin() + (it - MIN_SHOULDER), y.begin() + (it + MIN_SHOULDER + 1)) - y.begin();
            if (peak != it) continue;
            if (y[it] < global_peak / MIN_PEAK_RATIO) { ++n.n_noise; continue; }
            cand.push_back(it);
        }
    n.n_simple = cand.size();
    return cand;
}

inline std::vector<size_t> find_peaks(const std::vector<double>& x, const std::vector<int64_t>& y, PeakCounters& n) {
    std::vector<size_t> cand;
    if (x.empty()) return cand;
    for (const size_t i : find_peaks_y(y, n)) {
        const double center_x = x[i];
        const size_t left = std::upper_bound(x.begin(), x.end(), center_x * (1.0 - WINDOW)) - x.begin();      // inclusive
        const size_t right = std::upper_bound(x.begin(), x.end(), center_x * (1.0 + WINDOW)) - x.begin();     // exclusive
        if (left == 0 || right == x.size()) { ++n.n_edge; continue; }
        if (i - left < MIN_SHOULDER || right - i - 1 < MIN_SHOULDER) { ++n.n_sparse; continue; }
        const size_t peak = std::max_element(y.begin() + left, y.begin() + right) - y.begin();
        if (peak == i) cand.push_back(i); else ++n.n_not_window_max;
    }
    const size_t count = cand.size();
    std::vector<size_t> kept;
    for (size_t i = 0; i < count; ++i) {
        const size_t left_peak = i == 0 ? 0 : cand[i - 1], this_peak = cand[i], right_peak = i == count - 1 ? x.size() : cand[i + 1];
        const int64_t left_min = *std::min_element(y.begin() + left_peak, y.begin() + this_peak);     // (an empty range gives y[this_peak]: a peak sits at 10 or beyond, so it never is)
        const int64_t right_min = *std::min_element(y.begin() + this_peak, y.begin() + right_peak);
        if (std::max(left_min, right_min) * MIN_PEAK_HEIGHT_RATIO > y[this_peak]) ++n.n_shallow; else kept.push_back(this_peak);
    }
    for (size_t& p : kept) {
        size_t end = p + 1;
        while (end < y.size() && y[end] == y[p]) ++end;
        const size_t centre = p + (end - p - 1) / 2;
        n.n_centred += centre != p;
        p = centre;
    }
    return kept;
}

inline size_t max_peak(const std::vector<size_t>& cand, const std::vector<int64_t>& mass) {
    size_t m = 0;
    for (size_t i = 0; i < cand.size(); ++i) if (mass[cand[i]] > mass[cand[m]]) m = i;
    return m;
}

inline bool match_peak(const std::vector<size_t>& cand, const std::vector<double>& coverage, std::vector<int>& used, double base, double multiplier) {
    const double target = base * multiplier;
    for (size_t i = 0; i < used.size(); ++i)
        if (used[i] == 0 && std::fabs(target - coverage[cand[i]]) < MAX_PEAK_TOLERANCE * target) {
            used[i] = (int)(multiplier >= 1 ? multiplier : -1.0 / multiplier);
            return true;
        }
    return false;
}

// -> cn1_coverage; 0 for no data
inline double find_peak(const std::vector<double>& coverage, const std::vector<int64_t>& mass, PeakCounters& n) {
    if (mass.empty()) { n.way = W2RAP_STEP7_PEAK_NO_DATA; return 0; }
    std::vector<size_t> cand = find_peaks(coverage, mass, n);
    if (cand.size() >= 2) {                                    // PrefilterHighCNPeaks
        const double max_coverage = coverage[cand[max_peak(cand, mass)]];
        size_t keep = 0;
        while (keep < cand.size() && coverage[cand[keep]] <= HIGH_CN_PREFILTER * max_coverage) ++keep;
        n.n_prefiltered = cand.size() - keep;
        cand.resize(keep);
    }
    const size_t count = cand.size();
    n.n_peaks = count;
    std::vector<size_t> cn_peaks;
    if (count == 1) { n.way = W2RAP_STEP7_PEAK_SINGLE; cn_peaks.push_back(cand[0]); }
    else if (count == 0) { n.way = W2RAP_STEP7_PEAK_LARGEST_MASS; cn_peaks.push_back(std::max_element(mass.begin(), mass.end()) - mass.begin()); }
    else {
        n.way = W2RAP_STEP7_PEAK_SCORED;
        const size_t top = max_peak(cand, mass);
        int best_score = 0;
        std::vector<int> best_used;
        for (size_t i = 0; i < count; ++i) {
            const double base_cov = coverage[cand[i]];
            std::vector<int> used(count, 0);
            used[i] = 1;
            if (i > 0) match_peak(cand, coverage, used, base_cov, 0.5);
            for (size_t m = 2; m <= HIGH_CN_PREFILTER; ++m) match_peak(cand, coverage, used, base_cov, (double)m);
            const int score = (int)std::count_if(used.begin(), used.end(), [](int v) { return v != 0; });
            if (used[top] == 0) continue;
            if (score == best_score) {
                const size_t dip = std::find(used.begin(), used.end(), -2) - used.begin();
                if (dip != used.size() && mass[cand[dip]] * 10 < mass[cand[i]]) { best_score = score; best_used = used; ++n.n_score_ties_taken; }
            } else if (score > best_score) { best_score = score; best_used = used; }
        }
        for (size_t i = 0; i < best_used.size(); ++i) if (best_used[i] != 0) cn_peaks.push_back(cand[i]);     // (the pass of i == top always scores: never empty)
    }
    if (cn_peaks.size() > 1 && mass[cn_peaks[0]] < mass[cn_peaks[1]]) { n.halved = 1; return coverage[cn_peaks[1]] / 2.0; }
    return coverage[cn_peaks[0]];
}

// ---- Lines.cc:561-615: the groups of the cell rule, in the reference's loop order
struct CellGroups {
    std::vector<int32_t> line, cell, len;                      // per group: the line, the cell's position in it, the class's upper median
    std::vector<uint64_t> e_off, z_off;                        // [G + 1]
    std::vector<int32_t> e, z;                                 // the class's edges (UniqueSort), the edges every path of the class holds
    uint64_t n_cells = 0, n_cells_empty = 0, n_cells_sizes = 0, n_cells_one_in = 0, n_classes = 0, n_classes_short = 0;
};
template <class In> void cell_groups(const In& in, CellGroups& G) {
    G.e_off.assign(1, 0); G.z_off.assign(1, 0);
    auto kmers = [&](int32_t e) { return (int32_t)in.edge_len[e] - in.K + 1; };
    for (uint64_t l = 0; l < in.n_lines; ++l)
        for (uint64_t cl = in.line_off[l] + 1; cl < in.line_off[l + 1]; cl += 2) {
            const uint64_t p0 = in.cell_off[cl], np = in.cell_off[cl + 1] - p0;
            auto path = [&](uint64_t i) { return std::make_pair(in.line_edges + in.lpath_off[p0 + i], in.line_edges + in.lpath_off[p0 + i + 1]); };
            ++G.n_cells;
            if (np == 0 || path(0).first == path(0).second) { ++G.n_cells_empty; continue; }
            // (the reference reads front() and back() of every path: an empty path behind the first is its undefined behaviour; such a cell is skipped here)
            bool hole = false;
            for (uint64_t i = 0; i < np; ++i) hole = hole || path(i).first == path(i).second;
            if (hole) { ++G.n_cells_empty; continue; }
            std::vector<std::pair<int, int>> io;
            std::vector<int> ins, outs;
            for (uint64_t i = 0; i < np; ++i) { const auto p = path(i); io.emplace_back(p.first[0], p.second[-1]); ins.push_back(p.first[0]); outs.push_back(p.second[-1]); }
            auto unique_sort = [](auto& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
            unique_sort(io); unique_sort(ins); unique_sort(outs);
            if (ins.size() != outs.size() || ins.size() != io.size()) { ++G.n_cells_sizes; continue; }
            if (ins.size() < 2) { ++G.n_cells_one_in; continue; }
            std::vector<std::vector<uint64_t>> pi(io.size());
            for (uint64_t i = 0; i < np; ++i) { const auto p = path(i); pi[std::lower_bound(io.begin(), io.end(), std::make_pair((int)p.first[0], (int)p.second[-1])) - io.begin()].push_back(i); }
            for (size_t c = 0; c < io.size(); ++c) {
                ++G.n_classes;
                std::vector<int> lens;
                for (const uint64_t p : pi[c]) { int len = 0; for (const int32_t* q = path(p).first; q != path(p).second; ++q) len += kmers(*q); lens.push_back(len); }
                std::sort(lens.begin(), lens.end());
                const int len = lens[lens.size() / 2];          // Median of math/Functions.h: the upper median
                if (len < MIN_LINE) { ++G.n_classes_short; continue; }
                std::vector<int32_t> e, z;
                for (const uint64_t p : pi[c]) e.insert(e.end(), path(p).first, path(p).second);
                unique_sort(e);
                for (size_t k = 0; k < pi[c].size(); ++k) {     // Intersection of the paths' edge sets
                    std::vector<int32_t> y(path(pi[c][k]).first, path(pi[c][k]).second), t;
                    unique_sort(y);
                    if (k == 0) z = y;
                    else { std::set_intersection(z.begin(), z.end(), y.begin(), y.end(), std::back_inserter(t)); z.swap(t); }
                }
                G.line.push_back((int32_t)l); G.cell.push_back((int32_t)(cl - in.line_off[l])); G.len.push_back(len);
                G.e.insert(G.e.end(), e.begin(), e.end()); G.e_off.push_back(G.e.size());
                G.z.insert(G.z.end(), z.begin(), z.end()); G.z_off.push_back(G.z.size());
            }
        }
}

}  // namespace cov
}  // namespace w2
