"""Inputs that put the stages BEHIND the minimizer sketch on their edges, built without a GPU: the hash lookup with its max_occ probe,
the scan of the hit counts, the two gathers, the list cuts taken from the sorted keys, and the split that turns the reverse lists'
tied runs round (minim.hip.h, mm_seed_range / mm_create in sufarr_kernels.hip).  Every builder asserts the shape it promises -- with
the oracles where a hash or a count is claimed -- so a test that runs its case cannot pass on an input that lost its edge.
test_gpu_seed_stages.py runs them; test_canonical_oracle.py and test_minimizer_oracle.py show which deliberate mistakes they catch.

The idiom is test_gpu_minimizer.py::test_order_is_t_then_q's and test_canonical_oracle.py::order_trap's: X, a 15-mer, between invalid
bytes is the one valid k-mer of every window it is in, for any w <= 16; k is odd, so there are no reverse palindromes."""
import random

import canonical_oracle as KO
import chain_oracle as CO
import minimizer_oracle as MO

X = b"GATTACAGATTACCA"
K = len(X)                # 15: the tied runs and the list shapes
RUNS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097]
EDGE_K = 13               # the exact counts (w = 1)
PROBE_K = 5               # the probes (w = 1): mix is a bijection on 1024 values
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def runs_of(lists):
    """(list, t, start, end) of every maximal run of equal (list, t) in the flattened order of the lists: the order of the sorted keys"""
    out, at = [], 0
    for i, lst in enumerate(lists):
        j = 0
        while j < len(lst):
            e = j
            while e < len(lst) and lst[e][0] == lst[j][0]:
                e += 1
            out.append((i, lst[j][0], at + j, at + e))
            j = e
        at += len(lst)
    return out


# ---- 1. tied runs: run_edge / split_strands_kernel, and the sort's stability on the forward paths

def tied_runs(variant, runs=None, sep=b"N"):
    """Read i is its unit, X or revcomp(X), R[i] times, joined by `sep`; the text holds two units, at t1 < t2, between N inside
    random fill.  Every list that is not empty is runs of R[i] hits of one t, at q = 0, 16, 32, ...: in the mirrored coordinates
    too, since L - k - 16 j = 16 (R - 1 - j).
      "reverse": X in the reads, revcomp(X) twice in the text: list 2 i + 1 = the run at t1, then the run at t2, back to back
      "swapped": revcomp(X) in the reads, X twice in the text: the same lists from the other value of the read's strand bit
      "both":    X at t1 and revcomp(X) at t2; even reads repeat X, odd reads revcomp(X): every read has a forward and a reverse
                 run, and all four pairings of the read k-mer's and the text entry's strand bits occur.  Its reads begin with
                 five bases and a separator more, so the forward runs are at q = 6 + 16 j and the reverse runs at q' = 16 j: in
                 the other variants the mirror maps a read's starts onto themselves, and a missing mirror would not show
      "forward": X in the reads and twice in the text: the plain calls (MinimizerIndex.seed; TextIndex.seed with sep=b"R", a byte
                 the text has not, so that no k-mer that only overlaps X can hit), whose q order within a run is the sort's stability
    -> dict(text, reads, runs, t, lists): lists are the promised anchors in the call's order (2 r, 2 r + 1; r for "forward")."""
    runs = RUNS if runs is None else runs
    rng = random.Random(51)
    fill = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    rx = CO.revcomp(X)
    first, second = {"reverse": (rx, rx), "swapped": (X, X), "both": (X, rx), "forward": (X, X)}[variant]
    text = fill(300) + b"N" + first + b"N" + fill(410) + b"N" + second + b"N" + fill(200)
    t1, t2 = 301, 301 + 16 + 411
    assert text[t1:t1 + K] == first and text[t2:t2 + K] == second and text.count(X) + text.count(rx) == 2
    flipped = lambda i: variant == "swapped" or (variant == "both" and i % 2 == 1)
    head = [b"ACGTA"] if variant == "both" else []        # no k-mer of its own; it takes the mirror's symmetry away (below)
    reads = [sep.join(head + [rx if flipped(i) else X] * r) for i, r in enumerate(runs)]
    run = lambda t, r, q0=0: [(t, q0 + 16 * j, K) for j in range(r)]
    lists = []
    for i, r in enumerate(runs):
        if variant == "forward":
            lists.append(run(t1, r) + run(t2, r))
        elif variant == "both":
            lists += [run(t2, r, 6), run(t1, r)] if flipped(i) else [run(t1, r, 6), run(t2, r)]
        else:
            lists += [[], run(t1, r) + run(t2, r)]
    # the runs whose order the split (canonical) or the sort's stability (plain) decides: where they lie in the sorted keys
    tied = [x for x in runs_of(lists) if variant == "forward" or x[0] % 2 == 1]
    assert sorted(e - s for _, _, s, e in tied) == sorted(list(runs) * (1 if variant == "both" else 2))
    if runs is RUNS:
        assert sum(len(lst) for lst in lists) == 29642
        for edge in (64, 256, 4096):
            assert any(s // edge < (e - 1) // edge for _, _, s, e in tied), edge     # a multiple of it strictly inside a run
        assert len({s % 256 for _, _, s, _ in tied}) > 20
    return dict(text=text, reads=reads, runs=list(runs), t=(t1, t2), lists=lists)


def four_pairings(case):
    """the (read strand bit, text strand bit) pairs of the hits of a tied_runs case, over all its anchors"""
    st = {t: s for _, t, s in KO.index(case["text"], K, 1) if t in case["t"]}
    pairs = set()
    for read in case["reads"][:4]:
        sq = {s for _, _, s in KO.sketch(read, K, 1)}
        assert len(sq) == 1
        pairs |= {(s, b) for s in sq for b in st.values()}
    return pairs


def single_hit_read(case, canonical):
    """a read with one valid k-mer that occurs once in the case's text, selected there at w = 1 and at w = 8; on a canonical index
    it is reversed, so the call's one hit (total = 1: the sort runs no pass) is in a reverse list -> (read, t)"""
    text = case["text"]
    entries = KO.index(text, K, 8) if canonical else MO.index(text, K, 8)
    count = {}
    for e in entries:
        count[e[0]] = count.get(e[0], 0) + 1
    t = next(e[1] for e in entries if count[e[0]] == 1 and 50 < e[1] < 250)
    kmer = text[t:t + K]
    return b"N" + (CO.revcomp(kmer) if canonical else kmer) + b"N", t


# ---- 2. the max_occ probe of lookup_kernel: ix_hash[lo + max_occ] inside the index, on n_min, past it; lo = 0 and lo = n_min

def all_kmers(k):
    return [bytes(b"ACGT"[(v >> 2 * (k - 1 - i)) & 3] for i in range(k)) for v in range(4 ** k)]


def probe_cases(canonical, k=PROBE_K, c=3):
    """A text at w = 1 whose index lacks the k-mer of the smallest hash there is and the k-mer of the largest, and whose own largest
    hash and own smallest hash occur exactly c times each (planted between N; on a canonical index one of the plantings is the
    reverse complement, so the count is over both strands): the top k-mer's entries END the index (lo = n_min - c) and the bottom
    k-mer's START it (lo = 0).  Reads, one k-mer each: "below" (hash below every entry: lo = 0, nothing there), "above" (lo = n_min),
    "between" (absent, strictly between two neighbouring entries), "top", "bottom".
    -> dict(text, entries, reads, names, c, max_occs, hits): hits[max_occ] = the anchors each read must have in all."""
    hash_of = (lambda m: KO.hashes(m, k)[0][0]) if canonical else (lambda m: MO.hashes(m, k)[0])
    every = {m: hash_of(m) for m in all_kmers(k)}
    lowest, highest = min(every.values()), max(every.values())
    index = KO.index if canonical else MO.index
    for seed in range(60, 200):
        rng = random.Random(seed)
        body = CO.random_text(rng, 400)
        here = [every[body[p:p + k]] for p in range(len(body) - k + 1)]
        if lowest in here or highest in here:
            continue
        top, bottom = max(here), min(here)
        if here.count(top) >= c or here.count(bottom) >= c:
            continue
        top_kmer, bottom_kmer = (body[here.index(h):here.index(h) + k] for h in (top, bottom))
        text = body
        for kmer, h in ((top_kmer, top), (bottom_kmer, bottom)):
            for j in range(c - here.count(h)):
                text += b"N" + (CO.revcomp(kmer) if canonical and j == 0 else kmer)
        break
    else:
        raise AssertionError("no such text")
    entries = index(text, k, 1)
    hashes = [e[0] for e in entries]
    n_min = len(entries)
    between = next(m for m in sorted(every, key=every.get) if bottom < every[m] < top and every[m] not in hashes)
    names = ["below", "above", "between", "top", "bottom"]
    reads = [next(m for m in every if every[m] == lowest), next(m for m in every if every[m] == highest), between, top_kmer, bottom_kmer]
    # the hash relations claimed
    assert every[reads[0]] == lowest < hashes[0] and every[reads[1]] == highest > hashes[-1]
    at = next(i for i in range(n_min) if hashes[i] > every[between])
    assert 0 < at < n_min and hashes[at - 1] < every[between] < hashes[at]
    assert hashes[-c:] == [top] * c and hashes[-c - 1] < top and hashes[:c] == [bottom] * c and hashes[c] > bottom
    assert every[top_kmer] == top and every[bottom_kmer] == bottom
    if canonical:
        assert {s for _, _, s in entries[-c:]} == {0, 1} and {s for _, _, s in entries[:c]} == {0, 1}
    # the probe index lo + max_occ of the top k-mer: inside the index, on n_min, past it
    lo = n_min - c
    assert lo + (c - 1) == n_min - 1 and lo + c == n_min and lo + (c + 1) > n_min and lo + 1 < n_min
    max_occs = [c - 1, c, c + 1, 1, 0xffffffff]
    hits = {m: [0, 0, 0, c if m >= c else 0, c if m >= c else 0] for m in max_occs}
    return dict(text=text, entries=entries, reads=reads, names=names, c=c, max_occs=max_occs, hits=hits, k=k)


# ---- 3. exact counts on the block and tile edges: minimizers looked up, hits, index entries

def edge_text():
    """30 kb with a 400-base unit in five copies, at 0, 7400, 14800, 22200 and 29600, the second and the fourth reverse-complemented:
    on a canonical index (k = 13, w = 1) a k-mer of the unit hits five times, three forward and two reverse; on a plain one three times"""
    def make():
        text = bytearray(CO.random_text(random.Random(53), 30000, repeat=400, copies=5))
        unit = bytes(text[:400])
        for at in (7400, 22200):
            assert bytes(text[at:at + 400]) == unit
            text[at:at + 400] = CO.revcomp(unit)
        assert bytes(text[14800:15200]) == unit == bytes(text[29600:30000])
        return bytes(text)
    return cached("edge_text", make)


def edge_entries(canonical):
    return cached(("edge_entries", canonical), lambda: (KO.index if canonical else MO.index)(edge_text(), EDGE_K, 1))


def edge_counts(target, canonical):
    """Reads against edge_text() at k = 13, w = 1 whose calls have exactly `target` minimizers looked up, or exactly `target` hits;
    and a text whose index has exactly `target` entries.
    -> dict(one, spread: reads of `target` valid k-mers in all -- one read; three reads and an empty one;
            walk, walk_occ: a read that leaves the unit's third copy into text that hits once, cut where its hits reach `target`
            under max_occ = walk_occ (on a canonical index both of its lists fill);
            small: a text of `target` k-mers, all valid)"""
    text, k = edge_text(), EDGE_K
    one = text[3000:3000 + target + k - 1]
    a, b = target // 3, target // 2
    spread = [text[3000:3000 + a + k - 1], b"", text[9000:9000 + (b - a) + k - 1], text[16000:16000 + (target - b) + k - 1]]
    assert sum(max(len(r) - k + 1, 0) for r in spread) == target == len(one) - k + 1
    count = {}
    for e in edge_entries(canonical):
        count[e[0]] = count.get(e[0], 0) + 1
    start = 14800 + 400 - k - 40
    hs = KO.hashes(text[start:start + target + 400], k)[0] if canonical else MO.hashes(text[start:start + target + 400], k)
    total, end = 0, None
    for q, h in enumerate(hs):
        total += count[h] if count[h] <= 5 else 0
        if total >= target:
            end = start + q + k
            break
    assert total == target and end is not None and count[hs[0]] == (5 if canonical else 3)
    small = CO.random_text(random.Random(540 + target), target + k - 1)
    return dict(one=one, spread=spread, walk=text[start:end], walk_occ=5, small=small, k=k)


# ---- 4. / 5. degenerate lists for list_offsets_kernel, and the mirror of gather_strands_kernel at q = 0 and q = L - k

def list_shapes(canonical, n):
    """n reads at k = 15, w = 8 against a text that holds revcomp(X) (canonical) or X (plain) between N.  Kinds of read:
      f  50 bases of the text: forward hits only        r  their reverse complement: reverse hits only (none on a plain index)
      0  no hit: random bases, empty, or shorter than k
      A  X + N + junk: X is its first k-mer.  Canonical: its only hit is reverse, at q' = L - k.  Plain: forward, at q = 0
      B  junk + N + X: X is its last k-mer.  Canonical: its only hit is reverse, at q' = 0.  Plain: forward, at q = L - k
    -> dict(text, t, k, w, shapes): shapes[name] = (reads, kinds); filled(kinds) is the pattern of lists that are not empty."""
    rng, other = random.Random(55), random.Random(56)
    fill = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))
    junk = lambda m: bytes(other.choice(b"ACGT") for _ in range(m))
    text = fill(1500) + b"N" + (CO.revcomp(X) if canonical else X) + b"N" + fill(300)
    t = 1501

    def read(kind, i):
        at = 20 + (37 * i) % 1400
        if kind == "f":
            return text[at:at + 50]
        if kind == "r":
            return CO.revcomp(text[at:at + 50])
        if kind == "A":
            return X + b"N" + junk(30)
        if kind == "B":
            return junk(30) + b"N" + X
        return (junk(50), b"", b"ACGTACGT", junk(K))[i % 4]

    mixed = "frA0Bf0r"
    kinds = {
        "first": "f" + "0" * (n - 1),                                        # every hit in the first list
        "last": "0" * (n - 1) + ("r" if canonical else "f"),                  # every hit in the last list
        "ends_empty": "000" + "".join(mixed[i % 8] for i in range(n - 6)) + "000",
        "alternate": "".join("fr"[i % 2] for i in range(n)),
        "forward_only": "".join("f0ff"[i % 4] for i in range(n)),           # canonical: only even lists filled
        "reverse_only": "".join("rA0B"[i % 4] for i in range(n)),           # canonical: only odd lists filled
    }
    shapes = {name: ([read(c, i) for i, c in enumerate(ks)], ks) for name, ks in kinds.items()}
    assert all(len(ks) == n for ks in kinds.values())
    return dict(text=text, t=t, k=K, w=8, shapes=shapes, canonical=canonical)


def filled(kinds, canonical):
    """which lists of the call are promised not empty, in the call's order (canonical: 2 r forward, 2 r + 1 reverse)"""
    if not canonical:
        return [c in "fAB" for c in kinds]
    return [x for c in kinds for x in (c == "f", c in "rAB")]


def end_anchors(case, reads, kinds):
    """the promised lists of the A and B reads, whole: {list index in the call's order: anchors}"""
    t, k, out = case["t"], case["k"], {}
    for i, (r, c) in enumerate(zip(reads, kinds)):
        if c in "AB":
            first = c == "A"
            if case["canonical"]:
                out[2 * i] = []
                out[2 * i + 1] = [(t, len(r) - k if first else 0, k)]
            else:
                out[i] = [(t, 0 if first else len(r) - k, k)]
    return out
