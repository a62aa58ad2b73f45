"""What the canonical minimizer calls state (include/pwalign.h, "Canonical minimizers: one sketch, both strands"), in plain Python: the
canonical hash with its strand bit, the sketch, the index, and the two anchor lists per read.  Codes, mix, the windows and the leftmost
tie are minimizer_oracle.py's.  The keyword switches are deliberate mistakes: test_canonical_oracle.py shows that each changes a built
case, so a kernel that made it would be caught by the cases the GPU tests use."""
import minimizer_oracle as MO

INF, CODE = MO.INF, MO.CODE


def values(seq, k):
    """(f, r) of every start, None where the k-mer holds a byte that is not ACGT: f the k-mer's value, the first symbol most
    significant, r that of its reverse complement"""
    out = []
    for p in range(len(seq) - k + 1):
        f = r = 0
        for i, c in enumerate(seq[p:p + k]):
            if c not in CODE:
                f = None
                break
            f = f << 2 | CODE[c]
            r |= (3 - CODE[c]) << 2 * i
        out.append(None if f is None else (f, r))
    return out


def hashes(seq, k, palindrome_valid=False):
    """(h, s) of every start: the hash of the smaller of f and r and the strand bit, 1 where that is r; INF where the k-mer is
    invalid or its own reverse complement"""
    mask = (1 << 2 * k) - 1
    hs, ss = [], []
    for v in values(seq, k):
        if v is None or (v[0] == v[1] and not palindrome_valid):
            hs.append(INF)
            ss.append(0)
        else:
            hs.append(MO.mix(min(v), mask))
            ss.append(1 if v[1] < v[0] else 0)
    return hs, ss


def sketch(seq, k, w, hashed=None, **mistake):
    """[(pos, hash, strand)] of one sequence, ascending pos (hashed: its hashes(seq, k), where the caller has them)"""
    hs, ss = hashed or hashes(seq, k, **mistake)
    return [(p, hs[p], ss[p]) for p in MO.select_windows(hs, w)]


def index(text, k, w, **mistake):
    """the text's canonical sketch as (hash, t, strand) in ascending (hash, t)"""
    return sorted((h, t, s) for t, h, s in sketch(text, k, w, **mistake))


def swap_pairs_in_runs(rv):
    """the mistake of turning a run of equal t round by swapping its neighbouring pairs: right for runs of one and two hits, wrong
    from three on.  rv: one reverse list's (t, q', k, q) as they arrive, in ascending (t, q)"""
    out, i = list(rv), 0
    while i < len(out):
        j = i
        while j < len(out) and out[j][0] == out[i][0]:
            j += 1
        for p in range(i, j - 1, 2):
            out[p], out[p + 1] = out[p + 1], out[p]
        i = j
    return out


def seed(text, reads, k, w, max_occ=64, entries=None, strand_from_read=False, no_mirror=False, reverse_by_q=False, occ_per_strand=False,
         palindrome_valid=False, reverse_pairs_only=False, probe_at_end_dropped=False):
    """-> (lists, read minimizers looked up): lists[2 r] = read r's forward anchors (t, q, k), lists[2 r + 1] its reverse anchors
    (t, L - k - q, k), each in ascending (t, q); none looked up in an empty index, whose calls do no device work"""
    entries = index(text, k, w, palindrome_valid=palindrome_valid) if entries is None else entries
    by_hash = {}
    for h, t, s in entries:
        by_hash.setdefault(h, []).append((t, s))
    out, looked = [], 0
    for r in reads:
        fw, rv = [], []
        for q, h, sq in sketch(r, k, w, palindrome_valid=palindrome_valid):
            looked += 1 if entries else 0
            hits = by_hash.get(h, [])
            if probe_at_end_dropped and hits and len(hits) == max_occ and h == entries[-1][0]:
                continue    # the probe at lo + max_occ read one past the index's last entry, and taken for one more of the same hash
            for t, st in hits:
                flip = sq if strand_from_read else sq ^ st
                if occ_per_strand:
                    if sum(1 for _, s2 in hits if s2 == st) > max_occ:
                        continue
                elif len(hits) > max_occ:
                    continue
                if flip:
                    rv.append((t, q if no_mirror else len(r) - k - q, k, q))
                else:
                    fw.append((t, q, k, q))
        out.append(sorted(a[:3] for a in fw))
        if reverse_by_q or reverse_pairs_only:
            arrived = sorted(rv, key=lambda a: (a[0], a[3]))
            out.append([a[:3] for a in (swap_pairs_in_runs(arrived) if reverse_pairs_only else arrived)])
        else:
            out.append(sorted(a[:3] for a in rv))
    return out, looked


def by_strand(lists):
    """the call's order (2 r, 2 r + 1) -> MinimizerIndex.seed_strands' (all forward lists, then all reverse lists)"""
    return lists[0::2] + lists[1::2]
