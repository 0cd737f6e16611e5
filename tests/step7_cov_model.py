"""A naive restatement of ComputeCoverage (src/paths/long/large/Lines.cc:442-624), PeakFinder::FindPeaks (util/PeakFinder.h),
CN1PeakFinder::FindPeak (paths/long/large/CN1PeakFinder.cc), CNIntegerFraction (paths/long/large/GapToyTools5.cc:1520-1538) and
WriteLineStats (Lines.cc:357-379) for one sample, loop for loop, with Python lists: the model the library (w2rap_step7_coverage) and the
recorded runs of the reference are held to.  Python floats are IEEE doubles; the one rounding to float is numpy.float32 at Set.

RECIP and ABS_FLOATING say which machine form the recorded build of the reference (-Ofast) takes where the text leaves two: `x /
base_cov` inside a loop as written or as x * (1.0 / base_cov), and abs(int - double) as the floating or the integer function.  The
records of tests/step7_cov_cases.py decide them (test_step7_cov_model.py holds the model to every record)."""
import bisect
import math

import numpy as np

MIN_LINE = 1000
RECIP = dict(line=False, cell=False, long=False)
ABS_FLOATING = True
RULES = ("none", "line", "cell", "long")
WAYS = ("no_data", "single", "largest_mass", "scored")


NAN = -math.nan                                               # what an invalid operation gives on x86-64: the default NaN has its sign bit set ("-nan" in text, ffc00000 as a float)


def _div(x, b):
    """IEEE x / b where Python raises"""
    if b == 0:
        return x if math.isnan(x) else NAN if x == 0 else math.copysign(math.inf, x)
    return x / b


def _over_base(x, base, recip):
    if not recip:
        return _div(x, base)
    r = _div(1.0, base)
    if math.isinf(r) and x == 0:
        return NAN
    return x * r


def kmers(hbv, e):
    return int(hbv.edge_len[e]) - hbv.K + 1


def line_lengths(hbv, nested):
    """GetLineLengths (Lines.h:84-117)"""
    out = []
    for line in nested:
        total = 0
        for cell in line:
            lens = sorted(sum(kmers(hbv, e) for e in p) for p in cell)
            n = len(lens)
            if n == 1:
                total += lens[0]
            elif n == 2:
                total += (lens[0] + lens[1]) // 2
            elif n % 2:
                total += lens[n // 2]
            elif n:
                total += (lens[n // 2 - 1] + lens[n // 2]) // 2
        out.append(total)
    return out


def line_npairs(inv, paths, nested, E):
    tol = [-1] * E
    for i, line in enumerate(nested):
        for cell in line:
            for p in cell:
                for e in p:
                    tol[e] = i
    po, pe = [int(x) for x in paths[1]], [int(x) for x in paths[2]]
    npairs = [0] * len(nested)
    for pid in range((len(po) - 1) // 2):
        s = set()
        for e in pe[po[2 * pid]:po[2 * pid + 2]]:
            s.add(tol[e]); s.add(tol[int(inv[e])])
        for l in s:
            npairs[l] += 1
    return npairs


def find_peaks_y(y, n):
    cand = []
    if len(y) > 20:
        top = max(y)
        for it in range(10, len(y) - 10):
            w = y[it - 10:it + 11]
            if w.index(max(w)) != 10:
                continue
            if y[it] < top // 10000:
                n["n_noise"] += 1
                continue
            cand.append(it)
    n["n_simple"] = len(cand)
    return cand


def find_peaks(x, y, n):
    if not x:
        return []
    cand = []
    for i in find_peaks_y(y, n):
        left = bisect.bisect_right(x, x[i] * (1.0 - 0.05))
        right = bisect.bisect_right(x, x[i] * (1.0 + 0.05))
        if left == 0 or right == len(x):
            n["n_edge"] += 1
            continue
        if i - left < 10 or right - i - 1 < 10:
            n["n_sparse"] += 1
            continue
        w = y[left:right]
        if left + w.index(max(w)) == i:
            cand.append(i)
        else:
            n["n_not_window_max"] += 1
    kept = []
    for k, p in enumerate(cand):
        lp = 0 if k == 0 else cand[k - 1]
        rp = len(x) if k == len(cand) - 1 else cand[k + 1]
        left_min = min(y[lp:p]) if lp < p else y[p]
        right_min = min(y[p:rp])
        if max(left_min, right_min) * 1.2 > y[p]:
            n["n_shallow"] += 1
        else:
            kept.append(p)
    out = []
    for p in kept:
        end = p + 1
        while end < len(y) and y[end] == y[p]:
            end += 1
        c = p + (end - p - 1) // 2
        n["n_centred"] += c != p
        out.append(c)
    return out


def _max_peak(cand, mass):
    m = 0
    for i in range(len(cand)):
        if mass[cand[i]] > mass[cand[m]]:
            m = i
    return m


def _match(cand, cov, used, base, mult):
    target = base * mult
    for i in range(len(used)):
        if used[i] == 0 and abs(target - cov[cand[i]]) < 0.1 * target:
            used[i] = int(mult) if mult >= 1 else int(-1.0 / mult)
            return True
    return False


def find_peak(cov, mass, n):
    if not mass:
        n["peak_way"] = 0
        return 0.0
    cand = find_peaks(cov, mass, n)
    if len(cand) >= 2:
        mc = cov[cand[_max_peak(cand, mass)]]
        keep = 0
        while keep < len(cand) and cov[cand[keep]] <= 5 * mc:
            keep += 1
        n["n_prefiltered"] = len(cand) - keep
        cand = cand[:keep]
    n["n_peaks"] = len(cand)
    if len(cand) == 1:
        n["peak_way"] = 1
        peaks = [cand[0]]
    elif not cand:
        n["peak_way"] = 2
        peaks = [mass.index(max(mass))]
    else:
        n["peak_way"] = 3
        top = _max_peak(cand, mass)
        best_score, best_used = 0, []
        for i in range(len(cand)):
            used = [0] * len(cand)
            used[i] = 1
            if i > 0:
                _match(cand, cov, used, cov[cand[i]], 0.5)
            for m in range(2, 6):
                _match(cand, cov, used, cov[cand[i]], float(m))
            score = sum(1 for u in used if u != 0)
            if used[top] != 0:
                if score == best_score:
                    if -2 in used and mass[cand[used.index(-2)]] * 10 < mass[cand[i]]:
                        best_score, best_used = score, used
                        n["n_score_ties_taken"] += 1
                elif score > best_score:
                    best_score, best_used = score, used
        peaks = [cand[i] for i in range(len(best_used)) if best_used[i] != 0]
    if len(peaks) > 1 and mass[peaks[0]] < mass[peaks[1]]:
        n["halved"] = 1
        return cov[peaks[1]] / 2.0
    return cov[peaks[0]]


def pids(e, inv, index):
    return sorted(set(r // 2 for d in (e, int(inv[e])) for r in index[d]))


def run(hbv, inv, paths, nested, frac=0.1, min_edge_size=2000, recip=None, abs_floating=None):
    recip = RECIP if recip is None else recip
    abs_floating = ABS_FLOATING if abs_floating is None else abs_floating
    E, NL = len(hbv.edge_len), len(nested)
    assert NL, "no lines: the reference dereferences the end of an empty vector"
    n = dict.fromkeys(("n_simple", "n_noise", "n_edge", "n_sparse", "n_not_window_max", "n_shallow", "n_centred", "n_prefiltered", "n_peaks", "peak_way", "n_score_ties_taken", "halved",
                       "n_cells", "n_cells_empty", "n_cells_sizes", "n_cells_one_in", "n_classes", "n_classes_short", "n_line_lines", "n_long_asked", "n_undefined"), 0)
    po, pe = [int(x) for x in paths[1]], [int(x) for x in paths[2]]
    index = [[] for _ in range(E)]                             # invert
    for r in range(len(po) - 1):
        for e in pe[po[r]:po[r + 1]]:
            index[e].append(r)
    npairs = line_npairs(inv, paths, nested, E)
    lens = line_lengths(hbv, nested)
    covl = [_div(float(npairs[l]), float(lens[l])) for l in range(NL)]
    max_len = max(lens)
    min_len = min(10000, max_len // 2)
    c = sorted((covl[i], i) for i in range(NL) if lens[i] >= min_len and covl[i] > 0)
    covx, ids = [a for a, _ in c], [b for _, b in c]
    mass = []
    for i in range(len(covx)):
        m = lens[ids[i]]
        for j in range(i - 1, -1, -1):
            if covx[i] - covx[j] > 0.08 * covx[i]:
                break
            m += lens[ids[j]]
        for j in range(i + 1, len(covx)):
            if covx[j] - covx[i] > 0.08 * covx[i]:
                break
            m += lens[ids[j]]
        mass.append(m)
    base = find_peak(covx, mass, n)
    cov = [np.float32(-1)] * E
    rule = [0] * E
    for l in range(NL):                                        # the line rule
        if lens[l] >= MIN_LINE:
            n["n_line_lines"] += 1
            for j in range(0, len(nested[l]), 2):
                e = nested[l][j][0][0]
                cov[e] = np.float32(_over_base(covl[l], base, recip["line"])); rule[e] = 1
    groups = []
    for l in range(NL):                                        # the cell rule
        for j in range(1, len(nested[l]), 2):
            x = nested[l][j]
            n["n_cells"] += 1
            if not x or not x[0] or any(not p for p in x):     # (an empty path behind the first: the reference's undefined behaviour, the library skips the cell)
                n["n_cells_empty"] += 1
                continue
            io = sorted(set((p[0], p[-1]) for p in x))
            ins, outs = sorted(set(p[0] for p in x)), sorted(set(p[-1] for p in x))
            if len(ins) != len(outs) or len(ins) != len(io):
                n["n_cells_sizes"] += 1
                continue
            if len(ins) < 2:
                n["n_cells_one_in"] += 1
                continue
            pi = [[i for i in range(len(x)) if (x[i][0], x[i][-1]) == k] for k in io]
            for cls in pi:
                n["n_classes"] += 1
                ls = sorted(sum(kmers(hbv, e) for e in x[p]) for p in cls)
                ln = ls[len(ls) // 2]
                if ln < MIN_LINE:
                    n["n_classes_short"] += 1
                    continue
                es = sorted(set(e for p in cls for e in x[p]))
                pp = sorted(set(q for e in es for q in pids(e, inv, index)))
                cc = _div(float(len(pp)), float(ln))
                z = sorted(set.intersection(*[set(x[p]) for p in cls]))
                for e in z:
                    cov[e] = np.float32(_over_base(cc, base, recip["cell"])); rule[e] = 2
                groups.append(dict(line=l, cell=j, len=ln, pairs=len(pp), z=z))
    for e in range(E):                                         # the long-edge rule
        if not cov[e] >= 0 and kmers(hbv, e) >= MIN_LINE:
            n["n_long_asked"] += 1
            cc = _div(float(len(pids(e, inv, index))), float(kmers(hbv, e)))
            cov[e] = np.float32(_over_base(cc, base, recip["long"])); rule[e] = 3
    n["n_undefined"] = sum(1 for e in range(E) if not cov[e] >= 0)
    edges = good = 0
    for e in range(E):                                         # CNIntegerFraction
        if int(hbv.edge_len[e]) >= min_edge_size and cov[e] >= 0:
            edges += 1
            fc = float(cov[e])
            ic = 2147483647 if fc + 0.5 >= 2147483648.0 else int(fc + 0.5)
            d = abs(ic - fc) if abs_floating else float(abs(int(ic - fc)))
            good += d <= frac
    n["n_rule"] = [rule.count(r) for r in range(4)]
    return dict(npairs=npairs, llens=lens, covl=covl, covx=covx, mass=mass, ids=ids, base_cov=base, max_len=max_len, min_len=min_len, cov=np.array(cov, np.float32), rule=rule,
                groups=groups, n_cn_edges=edges, n_cn_good=good, cn_fraction=_div(float(good), float(edges)), counters=n)


def fixed2(x):
    """ToString(float, 2): a fixed stream of precision 2"""
    x = float(np.float32(x))
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return "%.2f" % x


def line_stats_text(res, nested):
    """WriteLineStats for one sample"""
    out = []
    for i, line in enumerate(nested):
        e1, e2 = line[0][0][0], line[-1][0][0]
        row = f"line[{i}] {e1}..{e2} len={res['llens'][i]} npairs={res['npairs'][i]}"
        if res["cov"][e1] >= 0:
            row += f" cov={fixed2(res['cov'][e1])}x"
        elif res["cov"][e1] != res["cov"][e1]:                  # a NaN: the recorded build (-Ofast) takes `defined` one way and the test inside the other (step7_cov_no_pairs)
            row += " cov=?x"
        out.append(row + "\n")
    return "".join(out)


def cn_line(x):
    """`std::cout << "CN fraction good = " << double`"""
    if math.isnan(x):
        return "CN fraction good = " + ("-nan" if math.copysign(1.0, x) < 0 else "nan")
    return "CN fraction good = %g" % x
