"""The codes form of the wavefront-alignment calls at the C boundary, without a GPU: exported, listed, declared with the parameter
lists of the offsets calls, refusing what those refuse (a null context first), and chosen in Python by form="codes"."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT, load_pkg

PAIRS = [("pwa_align_wfa_batch", "pwa_align_wfa_codes_batch"), ("pwa_align_wfa_batch_cigar", "pwa_align_wfa_codes_batch_cigar")]
INVALID = -1


def declaration(hdr, name):
    """the parameter list of `name` in the header, comments and white space removed"""
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_symbols_are_exported_listed_and_declared_like_the_offsets_calls():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwalign.h")).read(), flags=re.S)
    for old, new in PAIRS:
        assert hasattr(L, new), new
        assert new in pkg.EXPORTS, new
        assert declaration(hdr, new) == declaration(hdr, old)
        assert getattr(L, new).argtypes == getattr(L, old).argtypes


def test_the_header_describes_the_form():
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    block = hdr[hdr.index("Wavefront alignments"):hdr.index("#define PWA_WFA_NONE")]
    for word in ("codes form", "bits 0-1", "bit 2", "bit 3", "Pass A", "Pass B", "ring + cells"):
        assert word in block, word


def calls(L, name, ctx):
    """the call with every argument in place but `ctx`, then with each required pointer null in turn -> the return codes"""
    off, pa, pb = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc = (C.c_int32 * 1)()
    fn = getattr(L, name)
    if name.endswith("_cigar"):
        cg, md, co, mo = C.create_string_buffer(64), C.create_string_buffer(64), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        full = [ctx, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, cg, 64, co, md, 64, mo, None, None]
        nullable = [5, 6, 8, 9, 11, 12, 14, 15, 17]
    else:
        ops, ooff, nops = C.create_string_buffer(4), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)()
        full = [ctx, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, ops, ooff, nops, None]
        nullable = [5, 6, 8, 9, 11, 12, 13, 14]
    out = [fn(*full)]
    for at in nullable:
        args = list(full)
        args[at] = None
        out.append(fn(*args))
    bad = list(full)
    bad[1:5] = [1, 1, -1, -1]   # a scoring without a penalty form: still the null context's answer
    out.append(fn(*bad))
    return out


@pytest.mark.parametrize("old,new", PAIRS)
def test_a_null_context_is_refused_before_anything_else(old, new):
    L = load_pkg().lib()
    got, want = calls(L, new, None), calls(L, old, None)
    assert got == want and set(got) == {INVALID}


def test_python_chooses_the_call_by_form():
    pkg = load_pkg()
    f = pkg.Context._wfa_form
    assert f("offsets", "pwa_align_wfa_batch") == "pwa_align_wfa_batch"
    assert f("codes", "pwa_align_wfa_batch") == "pwa_align_wfa_codes_batch"
    assert f("codes", "pwa_align_wfa_batch_cigar") == "pwa_align_wfa_codes_batch_cigar"
    for bad in ("", "ring", "CODES", None, 1):
        with pytest.raises(ValueError):
            f(bad, "pwa_align_wfa_batch")
    for method in (pkg.Context.align_wfa_batch, pkg.Context.align_wfa_batch_cigar):
        assert inspect.signature(method).parameters["form"].default == "offsets"
