"""minimizer_oracle.py held to the definitions it restates, without a GPU: the mix is a bijection, the window form equals the local
form, w = 1 is plain k-mer seeding, anchors are byte-for-byte matches, a shared stretch of w + k - 1 symbols shares a selected k-mer,
each deliberate mistake changes a built case, and the planted reads of test_gpu_map_reads.py still chain to their places at w = 10."""
import random

import chain_oracle as CO
import minimizer_oracle as MO
import seed_oracle as SO


def test_mix_is_a_bijection_of_the_kmer_values():
    for k in range(1, 9):
        mask = (1 << 2 * k) - 1
        assert sorted(MO.mix(v, mask) for v in range(mask + 1)) == list(range(mask + 1)), k
    assert MO.mix(0, (1 << 62) - 1) < 1 << 62 and MO.mix((1 << 62) - 1, (1 << 62) - 1) < 1 << 62


def test_window_form_equals_local_form():
    rng = random.Random(11)
    seen_short = seen_invalid = 0
    for case in range(400):
        alphabet = (b"ACGT", b"ACGTN", b"AC")[case % 3]
        k, w = rng.randint(1, 8), rng.randint(1, 20)
        seq = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 60)))
        got = MO.sketch(seq, k, w)
        assert got == MO.sketch_local(seq, k, w), (seq, k, w)
        assert [p for p, _ in got] == sorted(set(p for p, _ in got)) and all(h == MO.hashes(seq, k)[p] != MO.INF for p, h in got)
        seen_short += 0 < len(seq) - k + 1 < w
        seen_invalid += b"N" in seq
    assert seen_short > 30 and seen_invalid > 30


def test_w_1_is_every_valid_kmer_and_seeds_like_the_kmer_dictionary():
    rng = random.Random(12)
    text = CO.random_text(rng, 3000, repeat=200, copies=3)
    reads = [CO.mutate(rng, text[a:a + 150], 0.05) for a in (0, 500, 1400, 2800)] + [b"", b"ACG", text[:9]]
    for k, max_occ in [(9, 64), (9, 2), (3, 64), (1, 1000)]:
        assert [p for p, _ in MO.sketch(text, k, 1)] == list(range(len(text) - k + 1))
        got, looked = MO.seed(text, reads, k, 1, max_occ)
        assert got == SO.seed(text, reads, k, 1, max_occ) and looked == sum(SO.slots(len(r), k, 1) for r in reads)
    assert [p for p, _ in MO.sketch(b"ACNNGTAC", 2, 1)] == [0, 4, 5, 6]


def test_every_anchor_is_a_byte_for_byte_match():
    rng = random.Random(13)
    text = bytes(rng.choice(b"ACGTNacgt") for _ in range(4000))
    reads = [CO.mutate(rng, text[a:a + 300], 0.03, alphabet=b"ACGTNa") for a in range(0, 3600, 400)]
    total = 0
    for k, w in [(5, 4), (11, 10), (4, 1)]:
        got, _ = MO.seed(text, reads, k, w, max_occ=1000)
        for r, anchors in zip(reads, got):
            assert anchors == sorted(anchors)
            assert all(ln == k and text[t:t + k] == r[q:q + k] and set(r[q:q + k]) <= set(b"ACGT") for t, q, ln in anchors)
            total += len(anchors)
    assert total > 100      # (five of the nine byte values are invalid, so valid k-mers are few; the loop is not empty)


def test_a_shared_stretch_of_w_plus_k_minus_1_shares_a_selected_kmer():
    rng = random.Random(14)
    for _ in range(200):
        k, w = rng.randint(2, 9), rng.randint(1, 12)
        core = bytes(rng.choice(b"ACGT") for _ in range(w + k - 1))
        flank = lambda: bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(0, 30)))
        a, b = flank(), flank()
        s1, s2 = a + core + flank(), b + core + flank()
        in1 = {p - len(a) for p, _ in MO.sketch(s1, k, w) if len(a) <= p <= len(a) + w - 1}
        in2 = {p - len(b) for p, _ in MO.sketch(s2, k, w) if len(b) <= p <= len(b) + w - 1}
        assert in1 & in2, (s1, s2, k, w)


def test_each_mistake_changes_a_built_case():
    ones = b"A" * 30                                       # ties everywhere: K = 28 at k = 3
    assert [p for p, _ in MO.sketch(ones, 3, 5)] == list(range(0, 28 - 5 + 1))
    assert [p for p, _ in MO.sketch(ones, 3, 5, tie_right=True)] == list(range(4, 28))
    assert [p for p, _ in MO.sketch_local(ones, 3, 5, left_ge=True)] == list(range(28))
    withn = b"ACGTACNACGTTGCA"
    assert MO.sketch(withn, 3, 4) != MO.sketch(withn, 3, 4, invalid_zero=True)
    short = b"GATTACA"                                     # K = 3 < w
    assert len(MO.sketch(short, 5, 8)) == 1 and MO.sketch(short, 5, 8, short_empty=True) == []
    rng = random.Random(15)
    differ = 0
    for _ in range(20):
        seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(6, 14))) for _ in range(6)]
        differ += MO.sketch_joined(seqs, 4, 6) != [MO.sketch(s, 4, 6) for s in seqs]
    assert differ >= 15


def test_the_probe_case_catches_what_the_max_occ_test_lets_through():
    """seed_stage_cases.probe_cases: the lookup's probe at lo + max_occ, read one past the index's last entry, changes the built case
    at max_occ = c alone -- and nothing in the inputs of test_gpu_minimizer.py's max_occ test, which never looks up the index's top"""
    import seed_stage_cases as SC
    from test_gpu_minimizer import K, W, max_occ_inputs
    text, entries, reads = max_occ_inputs()
    for m in (1, 4, 5, 6, 64, 0xffffffff):
        assert MO.seed(text, reads, K, W, m, entries=entries, probe_at_end_dropped=True) == MO.seed(text, reads, K, W, m, entries=entries)
    p = SC.probe_cases(False)
    assert p["entries"] == MO.index(p["text"], p["k"], 1)
    for m in p["max_occs"]:
        want, looked = MO.seed(p["text"], p["reads"], p["k"], 1, m, entries=p["entries"])
        assert [len(a) for a in want] == p["hits"][m] and looked == len(p["reads"]), m
        wrong, _ = MO.seed(p["text"], p["reads"], p["k"], 1, m, entries=p["entries"], probe_at_end_dropped=True)
        assert (wrong != want) == (m == p["c"]), m
    # the tied runs in their forward form: the plain calls' q order within 4097 equal (read, t) keys
    case = SC.tied_runs("forward")
    assert MO.seed(case["text"], case["reads"], SC.K, 8)[0] == case["lists"]
    sa = SC.tied_runs("forward", sep=b"R")
    assert SO.seed(sa["text"], sa["reads"], SC.K) == sa["lists"] == case["lists"]


def test_the_plan_is_the_seed_plan_of_a_text_with_n_min_kmers():
    assert MO.validate(100, [0, 50], 0, 64)[0] == MO.INVALID and MO.validate(100, [0, 50], 32, 64)[0] == MO.INVALID
    assert MO.validate(100, [0, 50], 31, 64) == (0, None, 20) and MO.validate(0, [0, 50, 40], 5, 64) == (MO.INVALID, 1, 0)
    assert MO.worst_hits(50, 7, 5, 64) == 46 * 7 and MO.worst_hits(50, 700, 5, 64) == 46 * 64 and MO.worst_hits(4, 700, 5, 64) == 0
    assert MO.ranges(0, [50, 60], 5, 64) == [] and MO.ranges(9, [50, 3, 60], 5, 64, budget=1) == [(0, 1), (2, 3)]


def test_planted_reads_still_chain_to_their_places_at_w_10():
    """the condition test_gpu_map_minimizer.py relies on: K = 13, w = 10, both strands"""
    import test_gpu_map_reads as MR
    text, planted = MR.planted()
    entries = MO.index(text, MR.K, 10)
    assert 4000 < len(entries) < 8000                       # about 2 / (w + 1) of the text's 29 988 k-mers
    fw = [r for r, _, _ in planted]
    anchors, _ = MO.seed(text, fw + [CO.revcomp(r) for r in fw], MR.K, 10, entries=entries)
    assert sum(len(a) for a in anchors) < 10000
    for i, (read, at, strand) in enumerate(planted):
        c = [CO.chain(anchors[s * len(fw) + i], want_dp=False) for s in (0, 1)]
        s = 1 if c[1]["score"] > c[0]["score"] else 0
        assert "+-"[s] == strand, i
        assert abs(c[s]["t_begin"] - c[s]["q_begin"] - at) <= MR.W, i
        assert CO.window_and_band(c[s], len(read), len(text), MR.W) is not None, i
