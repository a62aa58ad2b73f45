"""canonical_oracle.py held to the definitions it restates, without a GPU: anchors are byte-for-byte matches on their strand, the hash
ignores direction, reverse palindromes are invalid, a shared stretch on either strand shares a selected k-mer, each deliberate mistake
changes a built case (those of the stages behind the sketch change a case of seed_stage_cases.py), the planted reads of
test_gpu_map_reads.py chain to their strand and place from one sketch each, and the both-strand text of test_gpu_map_secondary.py
gives its two chains."""
import random

import canonical_oracle as KO
import chain_oracle as CO
import minimizer_oracle as MO


def has_palindrome(seq, k):
    return any(v is not None and v[0] == v[1] for v in KO.values(seq, k))


def test_every_anchor_is_a_byte_for_byte_match_on_its_strand():
    rng = random.Random(21)
    total = [0, 0]
    for alphabet, extra in [(b"ACGT", b"ACGT"), (b"ACGTN", b"ACGTNa")]:
        text = bytes(rng.choice(alphabet) for _ in range(4000))
        reads = []
        for i, a in enumerate(range(0, 3600, 300)):
            r = CO.mutate(rng, text[a:a + 300], 0.03, alphabet=extra)
            reads.append(CO.revcomp(r) if i % 2 else r)
        for k, w in [(5, 4), (11, 10), (4, 1), (6, 3)]:
            lists, looked = KO.seed(text, reads, k, w, max_occ=1000)
            assert len(lists) == 2 * len(reads) and looked == sum(len(KO.sketch(r, k, w)) for r in reads)
            for i, anchors in enumerate(lists):
                seq = reads[i // 2] if i % 2 == 0 else CO.revcomp(reads[i // 2])
                assert anchors == sorted(anchors) and CO.validate([anchors]) == (0, None)
                assert all(ln == k and text[t:t + k] == seq[q:q + k] and set(seq[q:q + k]) <= set(b"ACGT") for t, q, ln in anchors), (i, k, w)
                total[i % 2] += len(anchors)
    assert total[0] > 300 and total[1] > 300


def test_the_hash_ignores_direction_and_the_strand_bits_are_opposite():
    rng = random.Random(22)
    for case in range(300):
        k = rng.randint(1, 12)
        x = bytes(rng.choice((b"ACGT", b"ACGTN")[case % 2]) for _ in range(rng.randint(k, 50)))
        (h, s), (hr, sr) = KO.hashes(x, k), KO.hashes(CO.revcomp(x), k)
        n = len(x) - k
        for p in range(n + 1):
            assert h[p] == hr[n - p], (x, k, p)
            assert h[p] == KO.INF or s[p] + sr[n - p] == 1, (x, k, p)
    # the value pair itself: r of x is f of revcomp(x)
    assert KO.values(b"GATTACA", 7) == [tuple(reversed(KO.values(CO.revcomp(b"GATTACA"), 7)[0]))]
    assert KO.values(b"AAC", 3) == [(1, 0b101111)] and KO.hashes(b"AAC", 3)[1] == [0] and KO.hashes(b"GTT", 3)[1] == [1]


def test_reverse_palindromes_are_invalid_and_exist_only_for_even_k():
    assert KO.hashes(b"AT", 2)[0] == [KO.INF] and KO.hashes(b"ACGT", 4)[0] == [KO.INF] and KO.hashes(b"ACGTTAACGTAC"[:12], 12)[0][0] != KO.INF
    pal12 = b"ACGGTCGACCGT"
    assert CO.revcomp(pal12) == pal12 and KO.hashes(pal12, 12)[0] == [KO.INF] and KO.sketch(b"GG" + pal12 + b"TT", 12, 1) == KO.sketch(b"GG" + pal12 + b"TT", 12, 1)
    assert [p for p, _, _ in KO.sketch(b"GG" + pal12 + b"TT", 12, 1)] == [0, 1, 3, 4]
    assert KO.sketch(b"AT" * 40, 2, 5) == [] and KO.sketch(b"CG" * 40, 2, 1) == []            # AT, TA; CG, GC: every k-mer a palindrome
    # of ACGT repeated, ACGT and GTAC are palindromes, CGTA and TACG are each other's reverse complement: the odd starts alone are valid
    assert [p for p, _, _ in KO.sketch(b"ACGT" * 40, 4, 1)] == list(range(1, 157, 2)) and {s for _, _, s in KO.sketch(b"ACGT" * 40, 4, 1)} == {0, 1}
    for k in (2, 4):
        count = sum(1 for v in range(4 ** k) if KO.hashes(bytes(b"ACGT"[(v >> 2 * i) & 3] for i in range(k)), k)[0] == [KO.INF])
        assert count == 4 ** (k // 2), k
    for k in (1, 3, 5):
        assert all(KO.hashes(bytes(b"ACGT"[(v >> 2 * i) & 3] for i in range(k)), k)[0] != [KO.INF] for v in range(4 ** k)), k
    # a palindrome is skipped like a k-mer over N: its window selects the next valid one
    seq = b"TTGACGTCAAG"
    assert [p for p, _, _ in KO.sketch(seq, 4, 1)] == [p for p in range(8) if seq[p:p + 4] != CO.revcomp(seq[p:p + 4])] and has_palindrome(seq, 4)


def test_a_shared_stretch_on_either_strand_shares_a_selected_kmer():
    rng = random.Random(23)
    seen = [0, 0]
    while min(seen) < 150:
        k, w = rng.randint(2, 9), rng.randint(1, 12)
        core = bytes(rng.choice(b"ACGT") for _ in range(w + k - 1))
        if has_palindrome(core, k):
            continue
        flank = lambda: bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(0, 30)))
        flip = rng.random() < 0.5
        a, b = flank(), flank()
        s1, s2 = a + core + flank(), b + (CO.revcomp(core) if flip else core) + flank()
        in1 = {(p - len(a), h, s) for p, h, s in KO.sketch(s1, k, w) if len(a) <= p <= len(a) + w - 1}
        in2 = {(p - len(b), h, s) for p, h, s in KO.sketch(s2, k, w) if len(b) <= p <= len(b) + w - 1}
        if flip:   # the same canonical k-mer, not always the same start: among equal hashes (the k-mer twice, or it and its
            in1, in2 = {h for _, h, _ in in1}, {h for _, h, _ in in2}   # reverse complement) each strand selects its own leftmost
        assert in1 & in2, (s1, s2, k, w, flip)
        seen[flip] += 1


def order_trap():
    """a read that holds one k-mer selected at two starts, and a text that holds its reverse complement selected once: two reverse
    anchors with the same t, whose mirrored starts descend where the starts ascend.  Between invalid bytes x is the one valid k-mer
    of every window it is in.  -> text, read, x (k = 15), w, t, (q1, q2)"""
    rng = random.Random(24)
    x = b"GATTACAGATTACCA"
    fill = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    text = fill(300) + b"N" + CO.revcomp(x) + b"N" + fill(200)
    read = fill(40) + b"N" + x + b"N" + fill(25) + b"N" + x + b"N" + fill(33)
    return text, read, x, 8, 301, (41, 41 + 16 + 26)


def test_each_mistake_changes_a_built_case():
    text, read, x, w, t, (q1, q2) = order_trap()
    n, k = len(read), len(x)
    want, _ = KO.seed(text, [read], k, w)
    assert [a for a in want[1] if a[0] == t] == [(t, n - k - q2, k), (t, n - k - q1, k)] and CO.validate(want) == (0, None)
    assert all(text[a:a + k] == CO.revcomp(read)[b:b + k] for a, b, _ in want[1])
    # the reverse list left in ascending q: its mirrored starts descend, and chain()'s order rule refuses the list
    wrong, _ = KO.seed(text, [read], k, w, reverse_by_q=True)
    assert wrong != want and sorted(wrong[1]) == want[1] and CO.validate(wrong)[0] != 0
    # q not mirrored
    wrong, _ = KO.seed(text, [read], k, w, no_mirror=True)
    assert wrong[0] == want[0] and wrong[1] != want[1] and (t, q1, k) in wrong[1]
    # strand taken from the read only: x has s = 1 here or its reverse complement has, and the text holds both of them forward
    both = text + b"N" + x + b"N"
    want, _ = KO.seed(both, [read, CO.revcomp(read)], k, w)
    wrong, _ = KO.seed(both, [read, CO.revcomp(read)], k, w, strand_from_read=True)
    assert all(len([a for a in lst if a[0] in (t, len(text) + 1)]) == 2 for lst in want) and wrong != want
    assert [len(lst) for lst in wrong].count(0) >= 2
    # a palindrome kept as valid: a text of nothing but palindromes then seeds, and elsewhere they displace other minimizers
    assert KO.seed(b"AT" * 20, [b"AT" * 5], 2, 3)[0] == [[], []] and KO.seed(b"AT" * 20, [b"AT" * 5], 2, 3, palindrome_valid=True)[0] != [[], []]
    assert KO.seed(b"ACGT" * 10, [b"ACGT" * 5], 4, 3)[0] != KO.seed(b"ACGT" * 10, [b"ACGT" * 5], 4, 3, palindrome_valid=True)[0]
    # max_occ counted per strand: three forward copies and two reverse ones are five hits, dropped at max_occ 4, kept at 5
    rng = random.Random(25)
    fill = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))
    rep = b"N".join([fill(50), x, fill(60), x, fill(70), CO.revcomp(x), fill(40), x, fill(30), CO.revcomp(x), fill(20)])
    sizes = {m: [len(lst) for lst in KO.seed(rep, [b"N" + x + b"N"], k, w, max_occ=m)[0]] for m in (2, 3, 4, 5, 6)}
    assert sizes[4] == [0, 0] and sizes[5] == sizes[6] == [3, 2]
    assert [len(lst) for lst in KO.seed(rep, [b"N" + x + b"N"], k, w, max_occ=4, occ_per_strand=True)[0]] == [3, 2]
    assert [len(lst) for lst in KO.seed(rep, [b"N" + x + b"N"], k, w, max_occ=2, occ_per_strand=True)[0]] == [0, 2] and sizes[2] == [0, 0]


def several_t_per_q(seed=25):
    """order_trap()'s x at three places forward and two reverse, each between N: a minimizer of five hits over both strands"""
    rng = random.Random(seed)
    x = order_trap()[2]
    fill = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))
    return b"N".join([fill(50), x, fill(60), x, fill(70), CO.revcomp(x), fill(40), x, fill(30), CO.revcomp(x), fill(20)])


def test_the_stage_cases_catch_what_the_older_cases_let_through():
    """seed_stage_cases.py: each mistake of the stages behind the sketch changes a built case there -- and the two new ones change
    nothing in the cases test_gpu_canonical.py had before, which is why they are there"""
    import seed_stage_cases as SC
    text, read, x, w, t, _ = order_trap()
    k = len(x)
    older = [(text, [read, CO.revcomp(read), x], 64), (several_t_per_q(), [read, b"N" + x + b"N"], 64)]
    older += [(several_t_per_q(), [b"N" + x + b"N"], m) for m in (4, 5, 6)]
    assert max(e - s for tx, reads, m in older for _, _, s, e in SC.runs_of(KO.seed(tx, reads, k, w, m)[0])) == 2   # no run beyond two hits
    for tx, reads, m in older:
        want = KO.seed(tx, reads, k, w, m)
        assert KO.seed(tx, reads, k, w, m, reverse_pairs_only=True) == want
        assert KO.seed(tx, reads, k, w, m, probe_at_end_dropped=True) == want
    # runs turned round by swapping pairs: right up to two hits, wrong from three on, and chain()'s order rule refuses the list
    for variant, runs in [("reverse", None), ("swapped", [1, 2, 3, 4, 5]), ("both", [1, 2, 3, 4, 5, 6])]:
        case = SC.tied_runs(variant, runs)
        want, looked = KO.seed(case["text"], case["reads"], SC.K, 8)
        assert want == case["lists"] and looked == sum(case["runs"]) and CO.validate(want) == (0, None)
        wrong, _ = KO.seed(case["text"], case["reads"], SC.K, 8, reverse_pairs_only=True)
        assert [i for i in range(len(want)) if wrong[i] != want[i]] == [2 * i + 1 for i, r in enumerate(case["runs"]) if r >= 3]
        assert all(sorted(a) == b for a, b in zip(wrong, want)) and CO.validate(wrong)[0] != 0
    # the four pairings of the strand bits, and the mirror: each mistake changes the variant that has them all
    case = SC.tied_runs("both", [1, 2, 3, 4, 5, 6])
    assert SC.four_pairings(case) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert SC.four_pairings(SC.tied_runs("reverse", [1, 2])) | SC.four_pairings(SC.tied_runs("swapped", [1, 2])) == {(0, 1), (1, 0)}
    want, _ = KO.seed(case["text"], case["reads"], SC.K, 8)
    for mistake in ("no_mirror", "strand_from_read"):
        wrong, _ = KO.seed(case["text"], case["reads"], SC.K, 8, **{mistake: True})
        assert wrong != want and (mistake == "strand_from_read" or wrong[0::2] == want[0::2])
    sym = SC.tied_runs("reverse", [1, 2, 3])         # (where a read is nothing but its units the mirror maps its starts onto themselves)
    assert KO.seed(sym["text"], sym["reads"], SC.K, 8, no_mirror=True) == KO.seed(sym["text"], sym["reads"], SC.K, 8)
    # ... and the reads whose one reverse hit is their first k-mer (q' = L - k) and their last (q' = 0)
    shapes = SC.list_shapes(True, 127)
    reads, kinds = shapes["shapes"]["reverse_only"]
    ends = SC.end_anchors(shapes, reads, kinds)
    want, _ = KO.seed(shapes["text"], reads, shapes["k"], shapes["w"])
    assert [bool(lst) for lst in want] == SC.filled(kinds, True) and all(want[i] == a for i, a in ends.items())
    assert {a[0][1] for a in ends.values() if a} == {0, 31}                    # q' = 0, and q' = L - k of L = 15 + 1 + 30
    for mistake in ("no_mirror", "strand_from_read"):
        wrong, _ = KO.seed(shapes["text"], reads, shapes["k"], shapes["w"], **{mistake: True})
        assert all(wrong[i] != want[i] for i, a in ends.items() if a), mistake
    # the probe one past the index's last entry: a minimizer whose exactly max_occ occurrences end the index
    p = SC.probe_cases(True)
    for m in p["max_occs"]:
        want, _ = KO.seed(p["text"], p["reads"], p["k"], 1, m, entries=p["entries"])
        assert [len(want[2 * i]) + len(want[2 * i + 1]) for i in range(len(p["reads"]))] == p["hits"][m], m
        wrong, _ = KO.seed(p["text"], p["reads"], p["k"], 1, m, entries=p["entries"], probe_at_end_dropped=True)
        assert (wrong != want) == (m == p["c"]), m
    top = p["names"].index("top")
    assert want[2 * top] and want[2 * top + 1]                                 # counted over both strands


def test_the_two_lists_are_not_two_plain_seedings():
    """what the header does not promise: the sketch of revcomp(x) is not always the mirror of the sketch of x"""
    rng = random.Random(26)
    differ = 0
    for _ in range(300):
        x = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(10, 40)))
        k, w = rng.randint(2, 5), rng.randint(2, 8)
        mirror = sorted((len(x) - k - p, h, 1 - s) for p, h, s in KO.sketch(CO.revcomp(x), k, w))
        differ += mirror != KO.sketch(x, k, w)
    assert 0 < differ < 150


def test_planted_reads_chain_to_their_strand_and_place_from_one_sketch_each():
    """the condition test_gpu_map_canonical.py relies on: K = 13, w = 10, the n reads as given"""
    import test_gpu_map_reads as MR
    text, planted = MR.planted()
    entries = KO.index(text, MR.K, 10)
    fw = [r for r, _, _ in planted]
    lists, looked = KO.seed(text, fw, MR.K, 10, entries=entries)
    anchors = KO.by_strand(lists)
    plain, plain_looked = MO.seed(text, fw + [CO.revcomp(r) for r in fw], MR.K, 10)
    print("read minimizers looked up: canonical %d, plain on 2n reads %d, ratio %.3f; anchors %d and %d" %
          (looked, plain_looked, looked / plain_looked, sum(map(len, anchors)), sum(map(len, plain))))
    assert looked <= 0.55 * plain_looked
    for i, (read, at, strand) in enumerate(planted):
        c = [CO.chain(anchors[s * len(fw) + i], want_dp=False) for s in (0, 1)]
        s = 1 if c[1]["score"] > c[0]["score"] else 0
        assert "+-"[s] == strand, i
        assert abs(c[s]["t_begin"] - c[s]["q_begin"] - at) <= 100, i
        assert CO.window_and_band(c[s], len(read), len(text), MR.W) is not None, i


def test_the_both_strand_text_gives_a_forward_and_a_reverse_chain():
    from test_gpu_map_secondary import three_copies
    _, unit, _, both = three_copies()
    lists, _ = KO.seed(both, [unit], 12, 5)
    fw, rv = (CO.chain(lst, want_dp=False) for lst in lists)
    print("chain scores: forward %d, reverse %d" % (fw["score"], rv["score"]))
    assert fw["count"] and abs(fw["t_begin"] - fw["q_begin"] - 2000) <= 5
    assert rv["count"] and abs(rv["t_begin"] - rv["q_begin"] - 12000) <= 5
    assert (fw["score"], rv["score"]) == (595, 531)
