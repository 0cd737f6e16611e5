"""A plain Python restatement of the reference's DumpLineFiles (src/paths/long/large/Lines.cc:680-798), efasta of a cell
(efasta/EfastaTools.cc:35-71), efasta::Print (:1303-1316), SortLines (Lines.cc:664-678) and the `stats` file of FinalFiles
(FinalFiles.cc:73-104), written from the reference text, with a counter on every branch -- the names of w2rap_step7_fasta_out.

What the model does NOT restate is std::sort: `best` of a voted cell is the first id after ReverseSortSync(cov, ids), std::sort on the
index vector with cov[i] > cov[j].  Up to 16 paths that is an insertion sort, which keeps tied ids in order: the lowest tied index wins,
and the model says so.  From 17 paths up the partition decides, and for a cell of 17 paths or more whose largest vote is tied the model
TAKES THE ANSWER FROM THE RECORD: the tied path whose bases stand at that place of the recorded a.lines.fasta (`recorded_fasta`); without
a record it refuses such a cell."""
import numpy as np

GAP_N = 100
VOTE_ROW = 64
COUNTERS = ("n_printed", "n_skipped", "n_circular1", "n_circular2", "n_gap_cells", "n_cells_voted", "n_entries", "n_occurrences", "n_match_one", "n_match_none",
            "n_match_several", "n_cells_tied", "n_cells_wide", "n_pieces_fasta", "n_pieces_efasta")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def edge_texts(hbv):
    codes, off = hbv.edge_codes()
    text = _ACGT[codes].tobytes()
    return [text[int(off[e]):int(off[e + 1])] for e in range(hbv.n_edges)]


def cat(texts, K, path):
    """HyperBasevector::Cat: the first edge whole, each further one from base K - 1"""
    return texts[path[0]] + b"".join(texts[e][K - 1:] for e in path[1:])


def read_list(paths):
    off, ed = np.asarray(paths[1], np.int64), np.asarray(paths[2]).tolist()
    return [ed[off[r]:off[r + 1]] for r in range(len(off) - 1)]


def invert(reads, E):
    """invert(paths, paths_index, E): a read once per occurrence of the edge, in read order"""
    index = [[] for _ in range(E)]
    for r, p in enumerate(reads):
        for e in p:
            index[e].append(r)
    return index


def efasta_of(bs, cnt=None):
    """efasta::efasta(const vec<basevector>&) -> (text, left_share, right_share)"""
    if len(bs) == 1:
        return bs[0], 0, 0
    x0 = bs[0]
    left = 0
    for r in range(len(x0)):
        if not all(len(x) > r and x[r] == x0[r] for x in bs):
            break
        left += 1
    right = 0
    for r in range(len(x0) - left):
        if not all(len(x) - left > r and x[len(x) - r - 1] == x0[len(x0) - r - 1] for x in bs):
            break
        right += 1
    mids = [x[left:len(x) - right] for x in bs]
    return x0[:left] + b"{" + b",".join(mids) + b"}" + x0[len(x0) - right:], left, right


def print_record(header, body):
    """efasta::Print: the header, rows of 80, no empty last row"""
    return b">" + header + b"\n" + b"".join(body[i:i + 80] + b"\n" for i in range(0, len(body), 80))


def fasta_bodies(text):
    """a recorded fasta text -> {header: body}"""
    out, name = {}, None
    for row in text.split(b"\n"):
        if row.startswith(b">"):
            name = row[1:]; out[name] = b""
        elif row:
            out[name] += row
    return out


def vote(x, e, inv, reads, index, cnt):
    """Lines.cc:715-762 -> cov"""
    cov = [0] * len(x)

    def scan(p):
        for m in range(len(p)):
            if p[m] != e:
                continue
            cnt["n_occurrences"] += 1
            match = [True] * len(x)
            for r in range(len(x)):
                for s in range(len(x[r])):
                    if m + 1 + s >= len(p):
                        break
                    if p[m + 1 + s] != x[r][s]:
                        match[r] = False
                        break
            if sum(match) == 1:
                cnt["n_match_one"] += 1
                cov[match.index(True)] += 1
            elif sum(match) == 0:
                cnt["n_match_none"] += 1
            else:
                cnt["n_match_several"] += 1
    for rd in index[e]:
        cnt["n_entries"] += 1
        scan(reads[rd])
    for rd in index[inv[e]]:
        cnt["n_entries"] += 1
        scan([inv[q] for q in reversed(reads[rd])])
    return cov


def run(hbv, inv, paths, nested, parts=("fasta", "efasta", "src"), recorded_fasta=None):
    """-> dict(fasta, efasta, src: bytes or None; printed, best, cov, left_share, right_share: lists as the library lays them out
    (per line, per cell, per path of a cell) or None; counters)"""
    K, E = hbv.K, hbv.n_edges
    inv = [int(v) for v in inv]
    texts = edge_texts(hbv)
    to_left, to_right = hbv.to_left_right()
    want_f, want_e = "fasta" in parts, "efasta" in parts
    reads = read_list(paths) if want_f else []
    index = invert(reads, E) if want_f else []
    rec = fasta_bodies(recorded_fasta) if recorded_fasta is not None else None
    cnt = dict.fromkeys(COUNTERS, 0)
    printed, best_all, cov_all, ls_all, rs_all = [], [], [], [], []
    out1, out2 = [], []
    for i, L in enumerate(nested):
        cells = [(0, [0] * len(x), 0, 0) for x in L]               # best, cov, left, right of every cell: 0 where nothing is computed
        skip = i > 0 and nested[i - 1][0][0][0] == inv[L[-1][0][0]]
        printed.append(0 if skip else 1)
        if skip:
            cnt["n_skipped"] += 1
        else:
            cnt["n_printed"] += 1
            circular1 = len(L) > 1 and L[0][0][0] == L[-1][0][0]
            circular2 = len(L) == 1 and to_left[L[0][0][0]] == to_right[L[0][0][0]]
            cnt["n_circular1"] += circular1; cnt["n_circular2"] += circular2
            header = b"line_%d" % i + (b" circular" if circular1 or circular2 else b"")
            b1, b2 = b"", b""
            for j, x in enumerate(L):
                if circular1 and j == len(L) - 1:
                    break
                if len(x) == 1 and not x[0]:
                    cnt["n_gap_cells"] += 1
                    b1 += b"N" * GAP_N; b2 += b"N" * GAP_N
                    cnt["n_pieces_fasta"] += want_f; cnt["n_pieces_efasta"] += want_e
                    continue
                bs = [cat(texts, K, p) for p in x]
                if j < len(L) - 1:
                    assert all(len(b) >= K - 1 for b in bs)
                    bs = [b[:len(b) - (K - 1)] for b in bs]
                best, cov = 0, [0] * len(x)
                if j % 2 == 1 and want_f:
                    cnt["n_cells_voted"] += 1; cnt["n_cells_wide"] += len(x) > VOTE_ROW
                    cov = vote(x, L[j - 1][0][0], inv, reads, index, cnt)
                    tied = [r for r in range(len(x)) if cov[r] == max(cov)]
                    cnt["n_cells_tied"] += len(tied) > 1
                    if len(tied) == 1 or len(x) <= 16:
                        best = tied[0]                              # an insertion sort up to 16: the lowest tied index stays in front
                    else:                                           # std::sort's partition decides: the answer is taken from the record
                        assert rec is not None, "a tied cell of 17 paths or more: std::sort decides, and there is no record to ask"
                        body = rec[b"flattened_" + header]
                        fit = [r for r in tied if body[len(b2):len(b2) + len(bs[r])] == bs[r]]
                        assert len(fit) == 1, "the record does not name one of the tied paths"
                        best = fit[0]
                ef, left, right = efasta_of(bs) if want_e else (b"", 0, 0)
                b1 += ef; b2 += bs[best]
                cells[j] = (best, cov, left, right)
                cnt["n_pieces_fasta"] += want_f * len(x[best])
                cnt["n_pieces_efasta"] += want_e * (len(x[0]) if len(x) == 1 else 2 * len(x[0]) + sum(len(p) for p in x) + len(x) + 1)
            out1.append(print_record(header, b1)); out2.append(print_record(b"flattened_" + header, b2))
        for b, cov, l, r in cells:
            best_all.append(b); cov_all += cov; ls_all.append(l); rs_all.append(r)
    src = None
    if "src" in parts:
        rows = []
        for L in nested:
            rows.append(",".join(str(x[0][0]) if j % 2 == 0 else "{" + ",".join("{" + ",".join(map(str, p)) + "}" for p in x) + "}" for j, x in enumerate(L)) + "\n")
        src = "".join(rows).encode()
    return dict(fasta=b"".join(out2) if want_f else None, efasta=b"".join(out1) if want_e else None, src=src, printed=printed, best=best_all if want_f else None,
                cov=cov_all if want_f else None, left_share=ls_all if want_e else None, right_share=rs_all if want_e else None, counters=cnt)


def line_lengths(hbv, nested):
    """GetLineLengths (Lines.h:74-117): one path its K-mers, two their integer mean, more the median (an even number: the integer mean
    of the two middle ones)"""
    kmers = [int(n) - hbv.K + 1 for n in hbv.edge_len]
    out = []
    for L in nested:
        total = 0
        for x in L:
            lens = sorted(sum(kmers[e] for e in p) for p in x)
            n = len(lens)
            total += lens[0] if n == 1 else (lens[0] + lens[1]) // 2 if n == 2 else lens[n // 2] if n % 2 else (lens[n // 2] + lens[n // 2 - 1]) // 2
        out.append(total)
    return out


def sort_lines(hbv, inv, nested):
    """SortLines: by (-llens, min(F, inv[B]), F)"""
    llens = line_lengths(hbv, nested)
    key = lambda i: (-llens[i], min(nested[i][0][0][0], int(inv[nested[i][-1][0][0]])), nested[i][0][0][0])
    return [nested[i] for i in sorted(range(len(nested)), key=key)]


def stats_text(llens, K, prefix):
    """FinalFiles.cc:73-104 with LineN50 (Lines.cc:381-388) and N50 (math/Functions.cc:300-342)"""
    lens = sorted(x + K - 1 for x in llens if x >= 1000)
    n50, total, half = 0, sum(lens), 0
    for i, x in enumerate(lens):
        half += x
        if 2 * half == total and i < len(lens) - 1:
            n50 = (x + lens[i + 1]) // 2
            break
        if 2 * half >= total:
            n50 = x
            break
    rows = [f"# {prefix} assembly statistics", "", f"N50: {n50:,}"]
    for name, m in (("1", 1000), ("10", 10000), ("100", 100000)):
        rows.append(f"total bases in {name} kb+ sequences: {sum(x for x in llens if x >= m) // 2:,}")
    return "\n".join(rows) + "\n"
