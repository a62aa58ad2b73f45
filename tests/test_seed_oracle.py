"""seed_oracle.py against the definition: the slot counts, the anchors of chain_oracle's k-mer dictionary against a byte-for-byte scan of
the text (raw bytes, the text's end, max_occ at and past a slot's count), the validation order and the greedy cut on small lists."""
import random

import chain_oracle as CO
import seed_oracle as SO


def test_slots_are_the_positions_the_definition_lists():
    for k in (1, 2, 5):
        for step in (1, 2, 3, 7):
            for length in range(0, 30):
                want = len([q for q in range(0, length, step) if q + k <= length])
                assert SO.slots(length, k, step) == want, (length, k, step)


def test_anchors_against_a_byte_for_byte_scan():
    rng = random.Random(5)
    text = bytes(rng.choice(b"\x00\x7f\x80\xffA") for _ in range(400))
    reads = [text[10:60], text[-9:], text[-9:] + b"A", b"", b"\x80", bytes(rng.choice(b"\x00\x80A") for _ in range(40))]
    for k, step, max_occ in [(1, 1, 200), (1, 1, 64), (3, 1, 64), (3, 2, 2), (4, 5, 1), (9, 1, 64)]:
        got = SO.seed(text, reads, k, step, max_occ)
        assert got == [SO.brute(text, r, k, step, max_occ) for r in reads], (k, step, max_occ)
        assert CO.validate(got) == (0, None)
    assert SO.seed(b"ACGT", [b"ACGTA"], 5) == [[]] and SO.seed(b"ACGTA", [b"ACGTA"], 5) == [[(0, 0, 5)]]
    assert SO.seed(b"AAAA", [b"AA"], 2, max_occ=2) == [[]] and SO.seed(b"AAAA", [b"AA"], 2, max_occ=3) == [[(0, 0, 2), (1, 0, 2), (2, 0, 2)]]


def test_validation_order():
    assert SO.validate(100, [0, 10], 0, 1, 1) == (SO.INVALID, None, 0)
    assert SO.validate(100, [0, 10, 5, 1 << 40], 3, 1, 1) == (SO.INVALID, 1, 0)          # the decrease comes before the long read
    assert SO.validate(100, [0, 1 << 31, 5], 3, 1, 1) == (SO.CAPACITY, 0, 0)
    assert SO.validate(100, [0, 10, 12, 20], 3, 2, 64) == (0, None, 4 + 0 + 3)
    assert SO.validate(100, [], 3, 2, 64) == (0, None, 0)
    assert SO.validate(1 << 20, [0, 1 << 30], 1, 1, 4) == (SO.CAPACITY, 0, 0)             # 2^30 slots of 4 hits
    assert SO.validate(1 << 20, [0, (1 << 30) - 1], 1, 1, 4)[0] == 0
    assert SO.validate(2, [0, 1 << 30], 1, 1, 4)[0] == 0                                   # ... a text of two k-mers caps a slot at 2


def test_greedy_cut():
    n, k = 1000, 4
    lens = [0, 3, 4, 5, 0, 20, 2, 9, 9]                       # slots 0 0 1 2 0 17 0 6 6
    cut = lambda budget, max_occ=10: SO.ranges(n, lens, k, 1, max_occ, budget)
    assert cut(0) == [(0, 9)]
    assert cut(320) == [(0, 9)] and cut(319) == [(0, 8), (8, 9)]
    assert cut(30) == [(0, 5), (5, 6), (7, 8), (8, 9)]        # the read of 170 alone exceeds it; the slot-less read after it is left out
    assert cut(1) == [(2, 3), (3, 4), (5, 6), (7, 8), (8, 9)]
    assert SO.ranges(3, lens, k, 1, 10, 1) == [] and SO.ranges(n, [0, 3, 2], k, 1, 10, 1) == []
    assert SO.ranges(4, lens, k, 1, 10, 3) == [(0, 5), (5, 6), (7, 8), (8, 9)]   # one k-mer in the text: a slot's worst case is 1 hit
