#!/usr/bin/env python3
"""Fixtures for hw1 (multiple_pattern_matching.cpp) from the UNMODIFIED reference program, compiled by hand outside the
repository (its Makefile names a hw1.cpp that does not exist):

    g++ -std=c++17 -O2 -o /some/dir/hw1 multiple_pattern_matching/multiple_pattern_matching.cpp
    python3 tests/golden/make_golden_hw1.py --ref-bin /some/dir/hw1 --ref-dir .../multiple_pattern_matching

writes hw1.json (rc, stderr, .txt and .dot bytes per CLI case; outputs over 2 KiB as sha256 + length) and copies the reference's bundled inputs to
hw1_reference.fasta, hw1_reference_graph.fasta, hw1_patterns.fasta.  The large case is stored as the sha256 of the
.txt and the seeds of tests/hw1_gen.py, so that any machine regenerates its input.  Every case whose sequences do
not contain a terminator byte is also checked here against a brute force of "exact occurrences in T"."""
import argparse
import hashlib
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hw1_gen as G  # noqa: E402

FEW = b"$#@%^&!"
MANY = bytes(c for c in range(33, 127) if c not in b"ACGT")


MAX_INLINE = 2048


def L(b):
    return b.decode("latin-1")


def B(s):
    return s.encode("latin-1")


def brute(ref_data, pat_data):
    refs, pats = G.read_sequences(ref_data), G.read_sequences(pat_data)
    terms = FEW if len(refs) <= 7 else MANY
    text, bounds = b"", []
    for i, (h, s) in enumerate(refs):
        bounds.append((len(text), len(text) + len(s), h))
        text += s + terms[i:i + 1]
    if any(t in s for _, s in refs for t in terms[:len(refs)]):
        return None   # terminator collision: the reference's tree is malformed (unpinned)
    lines = []
    for name, p in pats:
        occ = {}
        for a, e, h in bounds:
            for q in range(a, e):
                if text[q:q + len(p)] == p and q + len(p) <= len(text):
                    occ.setdefault(h, []).append(q - a)
        body = ", ".join(L(h) + ":" + ",".join(str(x) for x in sorted(v)) for h, v in sorted(occ.items()))
        lines.append("(" + L(name) + ") - " + body + "\n")
    return "".join(lines)


def run(ref_bin, td, args):
    pr = subprocess.run([ref_bin] + args, cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return pr.returncode, L(pr.stderr.replace(ref_bin.encode(), b"hw1"))


def cli_case(ref_bin, name, ref, pat, dot=False, args=None, check=True):
    with tempfile.TemporaryDirectory() as td:
        if ref is not None:
            open(os.path.join(td, "ref.fa"), "wb").write(ref)
        if pat is not None:
            open(os.path.join(td, "pat.fa"), "wb").write(pat)
        a = args if args is not None else ["-r", "ref.fa", "-p", "pat.fa", "-o", "out"] + (["-d"] if dot else [])
        rc, err = run(ref_bin, td, a)
        rec = dict(name=name, args=a, rc=rc, stderr=err)
        if ref is not None:
            rec["ref"] = L(ref)
        if pat is not None:
            rec["pat"] = L(pat)
        for ext in ("txt", "dot"):
            p = os.path.join(td, "out." + ext)
            if os.path.exists(p):
                rec[ext] = L(open(p, "rb").read())
        if check and "txt" in rec and ref is not None and pat is not None:
            want = brute(ref, pat)
            if want is not None:
                assert rec["txt"] == want, name
        for ext in ("txt", "dot"):   # large outputs (the -d dumps are quadratic) are kept as their sha256 and length
            if len(rec.get(ext, "")) > MAX_INLINE:
                data = B(rec.pop(ext))
                rec[ext + "_sha256"], rec[ext + "_bytes"] = hashlib.sha256(data).hexdigest(), len(data)
        return rec


def rand_case(rng, k):
    alpha = rng.choice([b"ACGT", b"ACGT", b"ACGTN", b"AC"])
    n_ref = rng.choice([1, 2, 3, 5, 7, 8, 12])
    heads = [b"r%d" % i for i in range(n_ref)]
    if rng.random() < 0.3:
        heads = [rng.choice([b"b", b"a", b"\xe9x", b"Z", b"b"]) for _ in range(n_ref)]
    refs = []
    for i in range(n_ref):
        m = 0 if rng.random() < 0.1 else rng.randint(1, 40 if k % 2 else 12)
        refs.append((heads[i], bytes(rng.choice(alpha) for _ in range(m))))
    terms = FEW if n_ref <= 7 else MANY
    text = b"".join(s + terms[i:i + 1] for i, (_, s) in enumerate(refs))
    pats = []
    for j in range(rng.randint(1, 8)):
        r = rng.random()
        if r < 0.1:
            p = b""
        elif r < 0.3 and text:
            a = rng.randrange(len(text))
            p = text[a:a + rng.randint(1, 6)]   # may run across a terminator
        elif r < 0.7 and text:
            a = rng.randrange(len(text))
            p = text[a:a + rng.randint(1, 4)].rstrip(terms)
        else:
            p = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 5)))
        pats.append((b"p%d" % j, p))
    return G.fasta(refs, width=rng.choice([5, 80])), G.fasta(pats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-bin", required=True)
    ap.add_argument("--ref-dir", required=True, help="the reference's multiple_pattern_matching directory (bundled inputs)")
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    ref_bin = os.path.abspath(a.ref_bin)
    for src, dst in (("reference.fasta", "hw1_reference.fasta"), ("reference_graph.fasta", "hw1_reference_graph.fasta"),
                     ("patterns.fasta", "hw1_patterns.fasta")):
        shutil.copyfile(os.path.join(a.ref_dir, src), os.path.join(HERE, dst))
    rd = lambda f: open(os.path.join(HERE, f), "rb").read()  # noqa: E731
    cases = []
    for dot in (False, True):
        cases.append(cli_case(ref_bin, "bundled%s" % ("_d" if dot else ""), rd("hw1_reference.fasta"), rd("hw1_patterns.fasta"), dot))
        cases.append(cli_case(ref_bin, "bundled_graph%s" % ("_d" if dot else ""), rd("hw1_reference_graph.fasta"), rd("hw1_patterns.fasta"), dot))
    # readSequences quirks
    q = [
        ("crlf", b">a\r\nACGT\r\nGGA\r\n>b\r\nTTAC\r\n", b">p\r\nAC\r\n>q\r\nGA\r\n"),
        ("blank_stops", b">a\nACGT\n\n>b\nACGT\n", b">p\nAC\n"),
        ("cr_only_line_does_not_stop", b">a\nACGT\n\r\n>b\nCGTA\n", b">p\nGT\n"),
        ("spaces_line_does_not_stop", b">a\nAC GT\n   \n>b\n\tCGTA  \n", b">p\nCG\n>q\nC GT\n"),
        ("before_first_header", b"GGGG\nCC\n>a\nACGT\n>b\nTTT\n", b"AC\n>p\nGGGGCC\n>q\nGA\n"),
        ("bare_header", b">a\nACGT\n>\nCCCC\n>b\nGGGG\n", b">p\nCCCCGG\n>\nA\n>q\nCCCC\n"),
        ("trim_header", b">  a b \t\nACGT\n> c\nACG\n", b">  p x\nAC\n"),
        ("no_trailing_newline", b">a\nACGTACGT", b">p\nCGTA"),
        ("header_only_last", b">a\nACGT\n>b", b">p\nA\n>q"),
        ("leading_empty_line", b"\n>a\nACGT\n", b">p\nA\n"),
    ]
    for name, r, p in q:
        cases.append(cli_case(ref_bin, name, r, p, dot=True))
    rng = random.Random(481)
    for n_ref in (8, 40):
        refs = [(b"s%02d" % i, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 30)))) for i in range(n_ref)]
        text = b"".join(s + MANY[i:i + 1] for i, (_, s) in enumerate(refs))
        pats = [(b"x%d" % j, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3)))) for j in range(10)]
        pats += [(b"cross%d" % j, text[a:a + 5]) for j, a in enumerate(rng.sample(range(len(text) - 5), 5))]
        cases.append(cli_case(ref_bin, "refs%d" % n_ref, G.fasta(refs), G.fasta(pats), dot=True))
    cases.append(cli_case(ref_bin, "dup_nonascii_headers", b">b\nACAC\n>a\nCACA\n>b\nACAC\n>\xc3\xa9\nAAC\n>B\nCA\n>\x7f\nAC\n",
                          b">p\xc3\xa9\nAC\n>q\nCA\n>r\nA\n", dot=True))
    cases.append(cli_case(ref_bin, "empty_refs_and_patterns", b">a\n>b\nACG\n>c\n>d\nGGA\n", b">e\n>p\nG\n>f\n\n", dot=True))
    cases.append(cli_case(ref_bin, "cross_boundary", b">a\nACGT\n>b\nGTAC\n>c\nTT\n", b">p\nGT$GT\n>q\nT#T\n>r\nAC@\n>s\n$\n>t\nT$G\n", dot=True))
    cases.append(cli_case(ref_bin, "longer_than_text", b">a\nAC\n", b">p\nACACACAC\n>q\nAC$\n>r\nAC$X\n", dot=True))
    for k in range(60):
        r, p = rand_case(rng, k)
        cases.append(cli_case(ref_bin, "random%d" % k, r, p, dot=k % 3 == 0))
    # no references / missing inputs / unwritable output / missing flags
    cases.append(cli_case(ref_bin, "no_references", b"", b">p\nACGT\n>q\n\n", dot=True))
    cases.append(cli_case(ref_bin, "missing_ref", None, b">p\nACGT\n", args=["-r", "missing.fa", "-p", "pat.fa", "-o", "out", "-d"]))
    cases.append(cli_case(ref_bin, "missing_both", None, None, args=["-r", "nope_r.fa", "-p", "nope_p.fa", "-o", "out"]))
    cases.append(cli_case(ref_bin, "unwritable_prefix", b">a\nACGT\n", b">p\nAC\n", args=["-r", "ref.fa", "-p", "pat.fa", "-o", "no/such/dir/out"]))
    cases.append(cli_case(ref_bin, "unknown_args_ignored", b">a\nACGT\n", b">p\nCG\n", args=["-x", "-r", "ref.fa", "--y", "-p", "pat.fa", "-o", "out", "z"]))
    for args in (["-r", "ref.fa", "-p", "pat.fa"], ["-p", "pat.fa", "-o", "out"], [], ["-r", "ref.fa", "-p", "pat.fa", "-o"], ["-d"]):
        cases.append(cli_case(ref_bin, "usage_" + "_".join(x.strip("-.") for x in args), b">a\nAC\n", b">p\nA\n", args=args))
    out = dict(cases=cases)
    if not a.no_large:
        large = dict(total=16_000_000, n_refs=24, ref_seed=16, n_reads=100_000, read_seed=17)
        refs = G.genome(large["ref_seed"], large["total"], large["n_refs"])
        rds = G.reads(large["read_seed"], refs, large["n_reads"])
        with tempfile.TemporaryDirectory() as td:
            open(os.path.join(td, "ref.fa"), "wb").write(G.fasta(refs))
            open(os.path.join(td, "pat.fa"), "wb").write(G.fasta(rds))
            t0 = time.time()
            rc, err = run(ref_bin, td, ["-r", "ref.fa", "-p", "pat.fa", "-o", "out"])
            large["ref_seconds"] = round(time.time() - t0, 2)
            txt = open(os.path.join(td, "out.txt"), "rb").read()
            large.update(rc=rc, stderr=err, txt_sha256=hashlib.sha256(txt).hexdigest(), txt_bytes=len(txt))
        out["large"] = large
    with open(os.path.join(HERE, "hw1.json"), "w") as f:   # one case per line
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]")
        if "large" in out:
            f.write(',\n"large": ' + json.dumps(out["large"]))
        f.write("}\n")
    print("hw1.json", os.path.getsize(os.path.join(HERE, "hw1.json")), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
