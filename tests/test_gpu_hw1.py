"""hw1 on the device: the suffix array (prefix doubling over the device radix sort), the pattern search and occurrence
lists of include/pwalign.h (pwa_sa_*), and hw1_amd against every fixture of the unmodified reference, byte for byte."""
import hashlib
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hw1_gen as G
from conftest import B, load_golden, switched_context
from test_hw1_host import mismatches, needs_device, run_cli, signed_sa

GOLD = load_golden("hw1")


def fib_word(n):
    a, b = b"A", b"AB"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


@pytest.mark.gpu
def test_suffix_array_small_texts(ctx):
    rng = random.Random(11)
    texts = [b"", b"A", b"AA", b"AAA", b"BA", b"ACGT$", bytes(range(256)), bytes(range(255, -1, -1)), b"\x00\x80\x7f\xff\x00\x80"]
    texts += [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (2, 3, 15, 16, 17, 63, 64, 65, 100, 1000, 4095, 4096, 4097, 5000)]
    texts += [bytes(rng.randrange(256) for _ in range(n)) for n in (300, 3000)]
    texts += [b"AC" * k for k in (1, 2, 8, 9, 100, 1000)] + [fib_word(n) for n in (10, 100, 987, 2000)]
    texts += [bytes(rng.choice(b"ACGT") for _ in range(500)) + b"$" + bytes(rng.choice(b"ACGTN") for _ in range(500)) + b"#"]
    for t in texts:
        assert ctx.suffix_array(t) == signed_sa(t), (len(t), t[:20])


@pytest.mark.gpu
def test_suffix_array_runs_and_repeats(ctx):
    """poly-A (one suffix after the other: the most rounds) and long tandem repeats"""
    for n in (1, 2, 3, (1 << 16) + 1):
        assert ctx.suffix_array(b"A" * n) == list(range(n - 1, -1, -1))
    k = 1 << 15
    t = b"AC" * k   # suffixes AC..., then C...: by length within each
    want = [2 * k - 2 - 2 * i for i in range(k)] + [2 * k - 1 - 2 * i for i in range(k)]
    assert ctx.suffix_array(t) == want
    f = fib_word(5000)
    assert ctx.suffix_array(f) == signed_sa(f)


@pytest.mark.gpu
def test_suffix_array_16m_random(ctx):
    """2^24 random bases: a permutation whose neighbours are in order (24-byte prefixes vectorised, ties by slices)"""
    n = 1 << 24
    t = G.dna(99, n)
    sa = np.array(ctx.suffix_array(t), dtype=np.int64)
    assert ctx.sa_stats["rounds"] >= 2
    assert sa.size == n and np.bincount(sa, minlength=n).max() == 1
    pad = np.frombuffer(t + b"\x00" * 24, dtype=np.uint8)
    ties = np.ones(n - 1, dtype=bool)
    for w in range(3):
        word = np.zeros(n, dtype=np.uint64)
        for j in range(8 * w, 8 * w + 8):
            word = (word << np.uint64(8)) | pad[sa + j].astype(np.uint64)
        a, b = word[:-1], word[1:]
        assert not np.any(ties & (a > b))
        ties &= a == b
    for j in np.nonzero(ties)[0]:
        assert t[sa[j]:] < t[sa[j + 1]:]


def brute_count(t, p):
    if not p:
        return len(t)
    c, i = 0, t.find(p)
    while i >= 0:
        c += 1
        i = t.find(p, i + 1)
    return c


@pytest.mark.gpu
def test_find_counts_brute_force(ctx):
    rng = random.Random(5)
    for it in range(12):
        alpha = [b"ACGT", b"AC", b"ACGT$#", bytes(range(256))][it % 4]
        t = bytes(rng.choice(alpha) for _ in range(rng.choice([0, 1, 7, 200, 3000])))
        pats = [b"", b"Z", b"\xff\x00", t, t + b"A", t[:1]]
        for _ in range(200):
            m = rng.randint(1, 12)
            if t and rng.random() < 0.6:
                a = rng.randrange(len(t))
                pats.append(t[a:a + m])
            else:
                pats.append(bytes(rng.choice(alpha) for _ in range(m)))
        assert ctx.find(t, pats) == [brute_count(t, p) for p in pats], it


def brute_occ(t, starts, ranks, p):
    out = []
    for r in range(len(starts) - 1):
        for q in range(starts[r], starts[r + 1] - 1):
            if t.startswith(p, q):
                out.append((ranks[r], q - starts[r]))
    return sorted(out)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "1", "37"])
def test_occurrences_brute_force(chunk):
    rng = random.Random(7)
    with switched_context(**({"PWA_OCC_CHUNK_HITS": chunk} if chunk else {})) as ctx:
        for it in range(6):
            n_ref = rng.randint(1, 12)
            seqs = [bytes(rng.choice(b"ACG") for _ in range(rng.choice([0, 1, 5, 40, 300]))) for _ in range(n_ref)]
            t, starts = b"", []
            for i, s in enumerate(seqs):
                starts.append(len(t))
                t += s + b"$"
            starts.append(len(t))
            ranks = [rng.randrange(4) for _ in range(n_ref)]
            pats = [b"", b"$", b"A$", b"T"] + [bytes(rng.choice(b"ACG$") for _ in range(rng.randint(1, 4))) for _ in range(150)]
            got = ctx.find(t, pats, (starts, ranks))
            assert got == [brute_occ(t, starts, ranks, p) for p in pats], it


def check_case(pkg, case, tmp_path, env=None):
    return [(case["name"], k) for k in mismatches(case, run_cli(pkg, case, tmp_path, env))]


@pytest.mark.gpu
def test_cli_fixtures_byte_for_byte(pkg, tmp_path):
    """every fixture, the ones that need the device included; eight at a time, each in its own process"""
    with ThreadPoolExecutor(8) as ex:
        bad = sum(ex.map(lambda c: check_case(pkg, c, tmp_path), GOLD["cases"]), [])
    assert not bad
    assert sum(needs_device(c) for c in GOLD["cases"]) >= 70


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "4096"])
def test_cli_16mb_genome_100k_reads(pkg, tmp_path, chunk):
    """16 Mb in 24 references, 100k reads: sha256 of the reference's .txt (tests/hw1_gen.py regenerates the input)"""
    g = GOLD["large"]
    refs = G.genome(g["ref_seed"], g["total"], g["n_refs"])
    (tmp_path / "ref.fa").write_bytes(G.fasta(refs))
    (tmp_path / "pat.fa").write_bytes(G.fasta(G.reads(g["read_seed"], refs, g["n_reads"])))
    env = dict(os.environ)
    if chunk:
        env["PWA_OCC_CHUNK_HITS"] = chunk
    pr = subprocess.run([pkg.HW1_CLI_PATH, "-r", "ref.fa", "-p", "pat.fa", "-o", "out"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=600, env=env)
    assert pr.returncode == g["rc"], pr.stderr
    assert pr.stderr.decode("latin-1") == g["stderr"]
    txt = (tmp_path / "out.txt").read_bytes()
    assert len(txt) == g["txt_bytes"] and hashlib.sha256(txt).hexdigest() == g["txt_sha256"]
