"""hw1's host pieces without a GPU: readSequences and the DOT writer of libhw1_host.so against the reference's fixtures
(tests/golden/hw1.json, made by make_golden_hw1.py from the unmodified reference), and every hw1_amd case that ends
before the device is needed (usage, unwritable output, no references, missing inputs)."""
import hashlib
import os
import subprocess

import pytest

from conftest import B, load_golden, load_pkg
from hw1_gen import read_sequences as py_read_sequences

CASES = load_golden("hw1")["cases"]


def signed_sa(text):
    """suffixes in signed-char order (a prefix before the longer suffix)"""
    return sorted(range(len(text)), key=lambda i: bytes(b ^ 0x80 for b in text[i:]))


def needs_device(case):
    """hw1_amd opens the GPU only for a non-empty text with patterns or -d"""
    if case["rc"] != 0:
        return False
    args = case["args"]
    refs = py_read_sequences(B(case.get("ref", ""))) if "ref" in case else []
    pats = py_read_sequences(B(case.get("pat", ""))) if "pat" in case else []
    return bool(refs) and (bool(pats) or "-d" in args)


def run_cli(pkg, case, tmp_path, env=None):
    d = tmp_path / case["name"]
    d.mkdir()
    if "ref" in case:
        (d / "ref.fa").write_bytes(B(case["ref"]))
    if "pat" in case:
        (d / "pat.fa").write_bytes(B(case["pat"]))
    pr = subprocess.run([pkg.HW1_CLI_PATH] + case["args"], cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                        env=env)
    got = dict(rc=pr.returncode, stderr=pr.stderr.replace(pkg.HW1_CLI_PATH.encode(), b"hw1").decode("latin-1"))
    for ext in ("txt", "dot"):
        p = d / ("out." + ext)
        if p.exists():
            got[ext] = p.read_bytes()
    return got


def same_output(case, ext, data):
    """an output kept inline, or (over 2 KiB) as sha256 + length"""
    if ext + "_sha256" in case:
        return data is not None and len(data) == case[ext + "_bytes"] and hashlib.sha256(data).hexdigest() == case[ext + "_sha256"]
    return data == (B(case[ext]) if ext in case else None)


def mismatches(case, got):
    bad = [k for k in ("rc", "stderr") if got[k] != case[k]]
    return bad + [ext for ext in ("txt", "dot") if not same_output(case, ext, got.get(ext))]


def test_reader_matches_restatement_and_fixtures(tmp_path):
    pkg = load_pkg()
    n = 0
    for case in CASES:
        for key in ("ref", "pat"):
            if key not in case:
                continue
            p = tmp_path / ("%s.%s" % (case["name"], key))
            p.write_bytes(B(case[key]))
            recs, opened = pkg.hw1_read_sequences(str(p))
            assert opened
            assert recs == py_read_sequences(B(case[key])), (case["name"], key)
            n += 1
    assert n > 150
    recs, opened = pkg.hw1_read_sequences(str(tmp_path / "does_not_exist.fa"))
    assert recs == [] and not opened


def test_reader_quirks():
    """the cases the reference's reader handles unlike hw2's readFasta"""
    want = {
        "blank_stops": [(b"a", b"ACGT")],
        "cr_only_line_does_not_stop": [(b"a", b"ACGT"), (b"b", b"CGTA")],
        "before_first_header": [(b"a", b"GGGGCCACGT"), (b"b", b"TTT")],
        "bare_header": [(b"a", b"ACGT"), (b"b", b"CCCCGGGG")],
        "trim_header": [(b"  a b", b"ACGT"), (b" c", b"ACG")],   # trimmed before the ">" is dropped
        "leading_empty_line": [],
    }
    by_name = {c["name"]: c for c in CASES}
    for name, recs in want.items():
        assert py_read_sequences(B(by_name[name]["ref"])) == recs, name


def test_terminators():
    H = load_pkg().hw1_host()
    assert bytes(H.hw1_terminator(7, i) for i in range(7)) == b"$#@%^&!"
    many = bytes(H.hw1_terminator(90, i) for i in range(90))
    assert many == bytes(c for c in range(33, 127) if c not in b"ACGT")
    assert H.hw1_terminator(8, 0) == 33 and H.hw1_terminator(200, 90) == 33 and H.hw1_terminator(200, 95) == many[5]


def test_dot_writer_matches_reference_fixtures(tmp_path):
    """every -d fixture: the DOT text rebuilt from (SA, LCP) of T equals the reference's Ukkonen tree dump, byte for byte"""
    pkg = load_pkg()
    n = 0
    for case in CASES:
        if not ("dot" in case or "dot_sha256" in case) or "ref" not in case:
            continue
        p = tmp_path / (case["name"] + ".fa")
        p.write_bytes(B(case["ref"]))
        refs, _ = pkg.hw1_read_sequences(str(p))
        text, starts, heads = pkg.hw1_text(refs)
        out = tmp_path / (case["name"] + ".dot")
        assert pkg.hw1_write_dot(str(out), text, signed_sa(text), starts, heads) == 0
        assert same_output(case, "dot", out.read_bytes()), case["name"]
        n += 1
    assert n >= 25


def test_dot_writer_unwritable_path(tmp_path):
    pkg = load_pkg()
    assert pkg.hw1_write_dot(str(tmp_path / "no" / "dir" / "x.dot"), b"A$", [1, 0], [0, 2], [b"a"]) == -1


def test_cli_cases_without_device(tmp_path):
    """usage, unwritable prefix, missing inputs, no references: hw1_amd answers these before any HIP call"""
    pkg = load_pkg()
    done = 0
    for case in CASES:
        if needs_device(case):
            continue
        assert not mismatches(case, run_cli(pkg, case, tmp_path)), case["name"]
        done += 1
    assert done >= 10
