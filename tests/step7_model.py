"""A naive Python restatement of the reference text of Step 7's read-sized passes, counting every branch:
GetTol / GetLineLengths / GetLineNpairs (src/paths/long/large/Lines.cc:319-355, Lines.h:74-117) and MakeGaps up to its accepted gaps
(src/paths/long/large/MakeGaps.cc:25-427).  Lists and loops as the reference has them: the nears are built as lists and sorted, nears1 and
nears2 are real lists whose runs are walked, the search is the reference's queue.  Names of results and counters are those of
include/w2rap_step7.h."""
import numpy as np

MAX_HANG, MAX_DEPTH, MAX_INT, PASSES, MAX_COV_PC_OFF, MAX_LINE_TO_IGNORE = 800, 2, 1500, 3, 20.0, 500
PAIR_LINES = NEAR_LIST = 16
R_ACCEPTED, R_COUNT, R_LINE, R_COVERAGE, R_ALT, R_LEFT_END, R_RIGHT_END = range(7)


class Graph:
    """the digraphE as the reference holds it: per vertex From (vertices) / FromE (edge objects) and To / ToE, orders as in the file"""

    def __init__(self, hbv):
        self.K = int(hbv.K)
        self.kmers = [int(l) - self.K + 1 for l in hbv.edge_len]
        self.E, self.N = len(self.kmers), hbv.n_vertices
        fo, to = np.asarray(hbv.from_off, np.int64), np.asarray(hbv.to_off, np.int64)
        self.From = [[int(x) for x in hbv.from_v[fo[v]:fo[v + 1]]] for v in range(self.N)]
        self.FromE = [[int(x) for x in hbv.from_e[fo[v]:fo[v + 1]]] for v in range(self.N)]
        self.ToE = [[int(x) for x in hbv.to_e[to[v]:to[v + 1]]] for v in range(self.N)]
        self.to_left, self.to_right = [-1] * self.E, [-1] * self.E
        for v in range(self.N):
            for e in self.FromE[v]:
                self.to_left[e] = v
            for e in self.ToE[v]:
                self.to_right[e] = v
        self.To = [[self.to_left[e] for e in self.ToE[v]] for v in range(self.N)]

    def reverse(self):
        """digraphE::Reverse (graph/DigraphTemplate.h:439-442): the lists are swapped per vertex, their inner order stays"""
        self.From, self.To = self.To, self.From
        self.FromE, self.ToE = self.ToE, self.FromE
        self.to_left, self.to_right = self.to_right, self.to_left


def get_tol(E, lines):
    tol = [-1] * E
    for i, line in enumerate(lines):
        for cell in line:
            for path in cell:
                for e in path:
                    tol[e] = i
    return tol


def line_lengths(g, lines):
    def segment(cell):
        lens = [sum(g.kmers[e] for e in path) for path in cell]
        assert lens, "GetSegmentLength asserts nPaths > 0"
        if len(lens) == 1:
            return lens[0]
        if len(lens) == 2:
            return (lens[0] + lens[1]) // 2
        lens.sort()
        n = len(lens)
        return lens[n // 2] if n & 1 else (lens[n // 2] + lens[n // 2 - 1]) // 2
    return [sum(segment(cell) for cell in line) for line in lines]


def read_paths(paths):
    po = np.asarray(paths[1], np.int64)
    ed = np.asarray(paths[2]).tolist()
    return [ed[po[r]:po[r + 1]] for r in range(len(po) - 1)]


def line_npairs(tol, inv, rp, n_lines, cnt):
    npairs = [0] * n_lines
    cnt.update(n_pairs=len(rp) // 2, n_pairs_listed=0, n_pairs_spilled=0, n_pairs_no_path=0)
    for pid in range(len(rp) // 2):
        e = []
        for r in (2 * pid, 2 * pid + 1):
            for x in rp[r]:
                e += [tol[x], tol[inv[x]]]
        s = sorted(set(e))
        for l in s:
            npairs[l] += 1
        cnt["n_pairs_spilled" if len(s) > PAIR_LINES else "n_pairs_listed"] += 1
        cnt["n_pairs_no_path"] += not e
    cnt["n_line_hits"] = sum(npairs)
    return npairs


def edge_groups(g, cnt):
    nobj = g.E
    tom = list(range(nobj))
    sink_like, source_like, dist_to_end = [False] * nobj, [False] * nobj, [0] * nobj
    for e in range(nobj):
        if not g.From[g.to_right[e]]:
            sink_like[e] = True
        if not g.To[g.to_left[e]]:
            source_like[e] = True
    cnt.update(n_group_loop1=0, n_group_loop2=0)
    for _ in range(PASSES):
        for zpass in (1, 2):
            g.reverse()
            to_right = g.to_right
            like = sink_like if zpass == 2 else source_like
            for e in range(nobj):
                v = to_right[e]
                if len(g.From[v]) != 2 or len(g.To[v]) != 1:
                    continue
                e1, e2 = g.FromE[v][0], g.FromE[v][1]
                w1, w2 = to_right[e1], to_right[e2]
                if not like[e1] or not like[e2]:
                    continue
                if w1 == w2 and len(g.To[w1]) != 2:
                    continue
                if w1 != w2 and (len(g.To[w1]) != 1 or len(g.To[w2]) != 1):
                    continue
                d1, d2 = g.kmers[e1] + dist_to_end[e1], g.kmers[e2] + dist_to_end[e2]
                if d1 > MAX_HANG or d2 > MAX_HANG:
                    continue
                like[e] = True
                dist_to_end[e] = max(d1, d2)
                tom[e1] = tom[e]
                tom[e2] = tom[e]
                cnt["n_group_loop1"] += 1
            for e in range(nobj):
                v = to_right[e]
                if len(g.From[v]) != 2 or len(g.To[v]) != 1:
                    continue
                e1, e2 = g.FromE[v][0], g.FromE[v][1]
                w1, w2 = to_right[e1], to_right[e2]
                if w1 != w2:
                    continue
                if len(g.To[w1]) != 2 or len(g.From[w1]) != 1:
                    continue
                z = g.From[w1][0]
                if len(g.To[z]) != 1:
                    continue
                e3 = g.FromE[w1][0]
                if not like[e3]:
                    continue
                d1 = g.kmers[e1] + g.kmers[e3] + dist_to_end[e3]
                d2 = g.kmers[e2] + g.kmers[e3] + dist_to_end[e3]
                if d1 > MAX_HANG or d2 > MAX_HANG:
                    continue
                like[e] = True
                dist_to_end[e] = max(d1, d2)
                tom[e1] = tom[e]
                tom[e2] = tom[e]
                tom[e3] = tom[e]
                cnt["n_group_loop2"] += 1
    cnt.update(n_group_sink=sum(sink_like), n_group_source=sum(source_like))
    return tom, sink_like, source_like, dist_to_end


def make_nears(rp, inv, tom, tol, llens, cnt):
    nears = []
    cnt.update(n_pass_placed=0, n_pass_y_long=0, n_pass_none=0)
    for pid in range(len(rp) // 2):
        for ps in (1, 2):
            p1, p2 = rp[2 * pid], rp[2 * pid + 1]
            if not p1 or not p2:
                continue
            x = list(p1)
            y = [inv[e] for e in reversed(p2)]
            if ps == 2:
                x, y = y, x
                x = [inv[e] for e in reversed(x)]
                y = [inv[e] for e in reversed(y)]
            x = [tom[e] for e in x]
            y = [tom[e] for e in y]

            def compress(s):
                t = 0
                for j in range(1, len(s)):
                    if s[j] != s[t]:
                        t += 1
                        s[t] = s[j]
                return s[:t + 1]
            x, y = compress(x), compress(y)
            x = [e for e in x if llens[tol[e]] > MAX_LINE_TO_IGNORE]
            y = [e for e in y if llens[tol[e]] > MAX_LINE_TO_IGNORE]
            ys = set(y)
            n = 0
            for e1 in x:
                if e1 in ys:
                    continue
                for e2 in y:
                    if e1 == e2:
                        continue
                    nears.append((e1, e2))
                    n += 1
            cnt["n_pass_placed"] += 1
            cnt["n_pass_y_long"] += len(y) > NEAR_LIST
            cnt["n_pass_none"] += n == 0
    nears.sort()
    cnt["n_nears"] = len(nears)
    return nears


def is_close(g, e1, e2, shortcut_last=False):
    """the reference's queue (MakeGaps.cc:233-252) -> (steps at which e2 is met or None, the predecessor root exists).
    shortcut_last: the children of a node of depth 1 are not queued but asked for e2 (for hubs, where the queue has degree^3 entries)"""
    x, d, k = [e1], [-1], [0]
    pred = len(g.To[g.to_left[e1]]) == 1
    if pred:
        x.append(g.ToE[g.to_left[e1]][0]); d.append(-1); k.append(0)
    j = 0
    found = None
    while j < len(x):
        e = x[j]
        if e == e2:
            found = d[j] + 1
            break
        if not (k[j] > MAX_INT or d[j] == MAX_DEPTH):
            v, w = g.to_right[e], g.to_left[e]
            if shortcut_last and d[j] == MAX_DEPTH - 1:
                if e2 in g.FromE[v] or e2 in g.ToE[w]:
                    x.append(e2); d.append(d[j] + 1); k.append(k[j] + g.kmers[e2])
            else:
                for c in g.FromE[v] + g.ToE[w]:
                    x.append(c); d.append(d[j] + 1); k.append(k[j] + g.kmers[c])
        j += 1
    return found, pred


def advance(g, e1, e2):
    for _ in range(PASSES):
        v = g.to_right[e1]
        if len(g.To[v]) != 1 or len(g.From[v]) != 2:
            break
        if g.From[v][0] != g.From[v][1]:
            break
        w = g.From[v][0]
        if len(g.To[w]) != 2 or len(g.From[w]) != 1:
            break
        e1 = g.FromE[w][0]
    for _ in range(PASSES):
        v = g.to_left[e2]
        if len(g.From[v]) != 1 or len(g.To[v]) != 2:
            break
        if g.To[v][0] != g.To[v][1]:
            break
        w = g.To[v][0]
        if len(g.From[w]) != 2 or len(g.To[w]) != 1:
            break
        e2 = g.ToE[w][0]
    return e1, e2


def runs(s):
    """the lengths of the runs of equal values in a sorted list"""
    out, i = [], 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] == s[i]:
            j += 1
        out.append(j - i)
        i = j
    return out


def cover(np_, ll):
    """100.0 * double(npairs) / double(llens) in IEEE double, a zero divisor as the hardware answers it"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(100.0) * np.float64(np_) / np.float64(ll)


def run(hbv, inv, paths, lines, npairs=None, min_line=5000, min_link_count=3, parts=("lines", "links"), shortcut_last=False):
    """-> dict: the arrays and counters of w2rap_step7_out.  lines: nested lists; npairs None: LINKS reads what LINES counts"""
    g = Graph(hbv)
    inv = [int(x) for x in inv]
    rp = read_paths(paths)
    cnt, out = {}, {}
    tol = get_tol(g.E, lines)
    llens = line_lengths(g, lines)
    out.update(tol=tol, llens=llens)
    if "lines" in parts:
        out["npairs"] = line_npairs(tol, inv, rp, len(lines), cnt)
    if "links" not in parts:
        out["counters"] = cnt
        return out
    npairs = [int(x) for x in npairs] if npairs is not None else out["npairs"]
    cov = [cover(npairs[i], llens[i]) for i in range(len(lines))]
    tom, sink_like, source_like, dist_to_end = edge_groups(g, cnt)
    out.update(tom=tom, sink_like=sink_like, source_like=source_like, dist_to_end=dist_to_end)
    nears = make_nears(rp, inv, tom, tol, llens, cnt)
    nears1, nears2 = [[] for _ in range(g.E)], [[] for _ in range(g.E)]
    for e1, e2 in nears:
        nears1[e1].append(e2)
        nears2[e2].append(e1)
    for l in nears1 + nears2:
        l.sort()
    out["near_max1"] = [max(runs(l), default=0) for l in nears1]
    out["near_max2"] = [max(runs(l), default=0) for l in nears2]
    # links
    links = []
    cnt.update(n_near_kinds=0, n_pred_start=0, n_close=[0, 0, 0, 0])
    i = 0
    while i < len(nears):
        j = i
        while j < len(nears) and nears[j] == nears[i]:
            j += 1
        e1, e2 = nears[i]
        cnt["n_near_kinds"] += 1
        found, pred = is_close(g, e1, e2, shortcut_last)
        cnt["n_pred_start"] += pred
        if found is None:
            links.append((tom[e1], tom[e2], j - i))
        else:
            cnt["n_close"][found] += 1
        i = j
    links.sort(key=lambda l: (l[0], l[1]))                 # (stable: links equal after tom stay in the order of their nears)
    cnt["n_links"] = len(links)
    out.update(link_from=[l[0] for l in links], link_to=[l[1] for l in links], link_count=[l[2] for l in links])
    # the filters
    reason, accepted = [], []
    for e1, e2, count in links:
        r = R_ACCEPTED
        if count < min_link_count:
            r = R_COUNT
        elif llens[tol[e1]] < min_line or llens[tol[e2]] < min_line:
            r = R_LINE
        else:
            c1, c2 = cov[tol[e1]], cov[tol[e2]]
            if c1 < c2:
                c1, c2 = c2, c1
            with np.errstate(divide="ignore", invalid="ignore"):
                off = c1 / c2 - np.float64(1.0) > np.float64(MAX_COV_PC_OFF) / np.float64(100.0)
            max_alt = max(runs(nears1[e1]) + runs(nears2[e2]) + [0])
            if off:
                r = R_COVERAGE
            elif max_alt > count:
                r = R_ALT
            else:
                e1x, e2x = advance(g, e1, e2)
                if lines[tol[e1x]][-1][0][0] != e1x:
                    r = R_LEFT_END
                elif lines[tol[e2x]][0][0][0] != e2x:
                    r = R_RIGHT_END
        reason.append(r)
        if r == R_ACCEPTED:
            accepted.append((e1, e2))
    out["link_reason"] = reason
    cnt["n_reason"] = [reason.count(r) for r in range(7)]
    # the set rules
    a1, a2 = sorted(a[0] for a in accepted), sorted(a[1] for a in accepted)
    kept = [a for a in accepted if a1.count(a[0]) == 1 and a2.count(a[1]) == 1]
    cnt["n_not_one_to_one"] = len(accepted) - len(kept)
    moved = [advance(g, *a) for a in kept]
    cnt["n_advanced"] = sum(a != b for a, b in zip(kept, moved))
    accepted = sorted(set(moved))
    na = len(accepted)
    cnt["n_unique"] = na
    xa1, xa2 = {a[0] for a in accepted}, {a[1] for a in accepted}
    accepted2, acdel = [], []
    for e1, e2 in accepted:
        re1, re2 = inv[e1], inv[e2]
        d = False
        if (re2, re1) not in accepted:
            if re2 not in xa1 and re1 not in xa2:
                accepted2.append((re2, re1))
            else:
                d = True
        acdel.append(d)
    accepted = sorted(set([a for a, d in zip(accepted, acdel) if not d] + accepted2))
    cnt["n_sym_deleted"] = sum(acdel)
    cnt["n_sym_added"] = len(accepted) - na
    cleft, cright = [0] * g.E, [0] * g.E
    for e1, e2 in accepted:
        cleft[e1] += 1
        cright[e2] += 1
    over = [cleft[e] > 1 or cright[e] > 1 for e in range(g.E)]
    gaps = [a for a in accepted if not over[a[0]] and not over[a[1]]]
    cnt["n_overlinked"] = len(accepted) - len(gaps)
    cnt["n_gaps"] = len(gaps)
    out.update(gap_from=[a[0] for a in gaps], gap_to=[a[1] for a in gaps],
               gap_inv=[gaps.index((inv[b], inv[a])) if (inv[b], inv[a]) in gaps else -1 for a, b in gaps])
    out["counters"] = cnt
    return out
