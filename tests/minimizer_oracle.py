"""What the minimizer calls state (include/pwalign.h, "Minimizer sketches, a minimizer index, seeding against it"), in plain Python:
the hash, the sketch in its window form and in its local form, the index, the anchors, and the plan (seed_oracle's, for a text that
has n_min k-mers).  The keyword switches of sketch() and sketch_local() are deliberate mistakes: test_minimizer_oracle.py shows that
each changes a built case, so a kernel that made it would be caught by the cases the GPU tests use."""
import seed_oracle as SO

INVALID, CAPACITY = SO.INVALID, SO.CAPACITY
INF = (1 << 64) - 1            # an invalid k-mer: above every hash
CODE = {65: 0, 67: 1, 71: 2, 84: 3}
MAX_K, MAX_W = 31, 128


def mix(key, mask):
    key = (~key + (key << 21)) & mask
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & mask
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & mask
    key ^= key >> 28
    key = (key + (key << 31)) & mask
    return key


def hashes(seq, k, invalid_zero=False):
    """h(p) of every start p = 0 .. len - k, INF where the k-mer holds a byte that is not ACGT"""
    mask = (1 << 2 * k) - 1
    out = []
    for p in range(len(seq) - k + 1):
        v = 0
        for c in seq[p:p + k]:
            if c not in CODE:
                v = None
                break
            v = v << 2 | CODE[c]
        out.append((0 if invalid_zero else INF) if v is None else mix(v, mask))
    return out


def select_windows(hs, w, tie_right=False, short_empty=False):
    """the window form over a list of hashes -> the selected starts, ascending"""
    n = len(hs)
    if n == 0 or (short_empty and n < w):
        return []
    wins = [(s, s + w) for s in range(n - w + 1)] if n >= w else [(0, n)]
    chosen = set()
    for a, b in wins:
        low = min(hs[a:b])
        if low == INF:
            continue
        at = [j for j in range(a, b) if hs[j] == low]
        chosen.add(at[-1] if tie_right else at[0])
    return sorted(chosen)


def select_local(hs, w, left_ge=False):
    """the local form: p is selected iff it is valid and some window that holds it has only larger hashes before p and none smaller after"""
    n = len(hs)
    wins = [(s, s + w) for s in range(n - w + 1)] if n >= w else ([(0, n)] if n else [])
    out = []
    for p in range(n):
        if hs[p] == INF:
            continue
        for a, b in wins:
            if a <= p < b and all((hs[j] >= hs[p]) if left_ge else (hs[j] > hs[p]) for j in range(a, p)) and all(hs[j] >= hs[p] for j in range(p + 1, b)):
                out.append(p)
                break
    return out


def sketch(seq, k, w, **mistake):
    """[(pos, hash)] of one sequence, ascending pos"""
    hs = hashes(seq, k, mistake.pop("invalid_zero", False))
    return [(p, hs[p]) for p in select_windows(hs, w, **mistake)]


def sketch_local(seq, k, w, **mistake):
    hs = hashes(seq, k)
    return [(p, hs[p]) for p in select_local(hs, w, **mistake)]


def sketch_joined(seqs, k, w):
    """the mistake of comparing hashes across a sequence boundary: the list's k-mers as one run of hashes -> per sequence [(pos, hash)]"""
    per = [hashes(s, k) for s in seqs]
    flat = [h for hs in per for h in hs]
    picked = set(select_windows(flat, w))
    out, base = [], 0
    for hs in per:
        out.append([(p, hs[p]) for p in range(len(hs)) if base + p in picked])
        base += len(hs)
    return out


def index(text, k, w):
    """the text's sketch as (hash, t) in ascending (hash, t)"""
    return sorted((h, t) for t, h in sketch(text, k, w))


def seed(text, reads, k, w, max_occ=64, entries=None, probe_at_end_dropped=False):
    """per read its anchors (t, q, k) in ascending (t, q); -> (anchors, read minimizers looked up: none in an empty index, whose
    calls do no device work).  probe_at_end_dropped is a deliberate mistake: the probe at lo + max_occ read one past the index's last
    entry and taken for one more of the same hash, so a minimizer whose exactly max_occ occurrences end the index is dropped"""
    entries = index(text, k, w) if entries is None else entries
    by_hash = {}
    for h, t in entries:
        by_hash.setdefault(h, []).append(t)
    out, looked = [], 0
    for r in reads:
        anchors = []
        for q, h in sketch(r, k, w):
            looked += 1 if entries else 0
            ts = by_hash.get(h, [])
            if probe_at_end_dropped and ts and len(ts) == max_occ and h == entries[-1][0]:
                continue
            if len(ts) <= max_occ:
                anchors += [(t, q, k) for t in ts]
        out.append(sorted(anchors))
    return out, looked


def validate(n_min, offsets, k, max_occ):
    """(code, first offending read or None, k-mers) as pwa_mm_plan answers: pwa_seed_plan's rule with step 1 for a text of n_min k-mers"""
    if not 1 <= k <= MAX_K:
        return INVALID, None, 0
    return SO.validate(n_min + k - 1, offsets, k, 1, max_occ)


def worst_hits(length, n_min, k, max_occ):
    return SO.slots(length, k, 1) * min(max_occ, n_min)


def ranges(n_min, lengths, k, max_occ, budget=0):
    return SO.ranges(n_min + k - 1, lengths, k, 1, max_occ, budget)
