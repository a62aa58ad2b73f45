"""What pwa_seed_plan and pwa_sa_seed state, in plain Python: the slots of a read, the validation order with its first offending
read, the greedy cut of a read list into ranges under a budget of worst-case hits, and the anchors themselves -- those come from
chain_oracle's k-mer dictionary (kmer_index / seed), which is what Context.seed has been tested against since it exists."""
import chain_oracle as CO

INVALID, CAPACITY = CO.INVALID, CO.CAPACITY
DEFAULT_BUDGET = 1 << 27   # the suffix-array unit's budget of hits per chunk, where PWA_OCC_CHUNK_HITS is unset


def slots(length, k, step):
    """the k-mers of a read of `length` bytes: q = 0, step, 2 step, ... while q + k <= length"""
    return 0 if length < k else (length - k) // step + 1


def worst_hits(length, n, k, step, max_occ):
    """no slot can keep more hits than max_occ, nor than the text has k-mers"""
    return slots(length, k, step) * min(max_occ, max(n - k + 1, 0))


def validate(n, offsets, k, step, max_occ):
    """(code, first offending read or None, slots) as pwa_seed_plan answers for read offsets (len(offsets) = reads + 1, or empty for
    no reads): parameters first, then the reads in order -- offsets decreasing, a read of 2^31 bytes or more, worst-case hits of 2^32
    or more -- then the total of the slots; slots is 0 with an error"""
    if k == 0 or step == 0 or max_occ == 0:
        return INVALID, None, 0
    total = 0
    for r in range(max(len(offsets) - 1, 0)):
        length = offsets[r + 1] - offsets[r]
        if length < 0:
            return INVALID, r, 0
        if length >= 1 << 31:
            return CAPACITY, r, 0
        if worst_hits(length, n, k, step, max_occ) >= 1 << 32:
            return CAPACITY, r, 0
        total += slots(length, k, step)
    if total >= 1 << 32:
        return CAPACITY, None, 0
    return 0, None, total


def ranges(n, lengths, k, step, max_occ, budget=0):
    """the greedy cut: consecutive reads as long as their worst-case hits fit the budget (0: the library's; never more than 2^32 - 1),
    or one read that alone exceeds it -> [(first read, end read)] of the ranges that hold a slot that can hit"""
    budget = min(budget or DEFAULT_BUDGET, (1 << 32) - 1)
    w = [worst_hits(ln, n, k, step, max_occ) for ln in lengths]
    out, k0 = [], 0
    while k0 < len(w):
        k1, tot = k0 + 1, w[k0]
        while k1 < len(w) and tot + w[k1] <= budget:
            tot += w[k1]
            k1 += 1
        if tot:
            out.append((k0, k1))
        k0 = k1
    return out


def seed(text, reads, k, step=1, max_occ=64, index=None):
    """per read its anchors (t, q, k) in ascending (t, q): chain_oracle.seed over chain_oracle.kmer_index of the text as given"""
    index = CO.kmer_index(text, k) if index is None else index
    return [CO.seed(index, r, k, step, max_occ) for r in reads]


def brute(text, read, k, step=1, max_occ=64):
    """the same anchors from the definition alone: every t compared byte for byte"""
    out = []
    for q in range(0, len(read) - k + 1, step):
        hits = [t for t in range(len(text) - k + 1) if text[t:t + k] == read[q:q + k]]
        if len(hits) <= max_occ:
            out += [(t, q, k) for t in hits]
    return sorted(out)
