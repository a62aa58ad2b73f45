"""The canonical minimizer calls at the C boundary, without a GPU: exported, listed, declared with the header's definitions, refusing
null pointers and k and w out of range before they touch a context, and the Python layer's pairing of calls and index kinds.  An
index needs a device, so the pairings at the C boundary and the 2 n + 1 offsets are test_gpu_canonical.py's."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, load_pkg

NAMES = ["pwa_mm_create_canonical", "pwa_mm_fetch_canonical", "pwa_mm_sketch_canonical", "pwa_mm_seed_strands"]
INVALID = -1


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert hdr.index("Minimizer sketches, a minimizer index, seeding against it") < hdr.index("Canonical minimizers: one sketch, both strands")
    block = hdr[hdr.index("Canonical minimizers: one sketch, both strands"):hdr.index("int pwa_mm_create_canonical")]
    for word in ("f(p) = sum of c_i * 4^(k - 1 - i)", "r(p) = sum of (3 - c_i) * 4^i", "If f < r the", "strand bit s(p) = 0 and h(p) = mix(f)",
                 "s(p) = 1 and h(p) = mix(r)", "a reverse palindrome, possible only for", "+infinity, never selected", "in ascending (hash, t)",
                 "the count being over both strands together", "goes to list 2r", "text[t .. t + k) == read[q .. q + k)", "goes to list 2r + 1",
                 "(t, L - k - q)", "revcomp(read)[q' .. q' + k)", "in ascending (t, q)", "pwa_chain_anchors requires", "Not promised",
                 "anc_off_out[2 n_reads + 1]", "minimizers counting each read", "On a plain index PWA_E_INVALID", "2^31 - 1", "PWA_E_CAPACITY",
                 "is the plan of pwa_mm_seed_strands as it stands", "summed over the two lists", "bit 31 of the position word",
                 "nothing per text position is kept"):
        assert word in block, word
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert re.search(r"pwa_mm_fetch_canonical\s*\([^)]*uint8_t\s*\*\s*strand_out", hdr) and re.search(r"pwa_mm_sketch_canonical\s*\([^)]*uint8_t\s*\*\s*strand_out", hdr)
    for method in ("seed", "seed_strands", "entries"):
        assert callable(getattr(pkg.MinimizerIndex, method)), method


def test_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, out = (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 3)()
    t, h, s = (C.c_uint32 * 4)(), (C.c_uint64 * 4)(), (C.c_uint8 * 4)()
    ix = C.c_void_p()
    assert L.pwa_mm_create_canonical(None, b"ACGT", 4, 2, 2, C.byref(ix)) == INVALID and not ix
    assert L.pwa_mm_sketch_canonical(None, b"ACGT", off, 1, 2, 2, out, t, h, s, 4, None) == INVALID
    assert L.pwa_mm_fetch_canonical(None, h, t, s, 4) == INVALID and L.pwa_mm_fetch_canonical(None, None, None, None, 0) == INVALID
    assert L.pwa_mm_seed_strands(None, b"ACGT", off, 1, 64, out) == INVALID and L.pwa_mm_seed_strands(None, None, None, 0, 64, None) == INVALID


def test_k_and_w_at_and_past_their_limits():
    pkg = load_pkg()
    # the calls with a context check k and w before they touch it -- but after a null context; the Python layer checks them itself
    for k, w in [(0, 5), (32, 5), (5, 0), (5, 129)]:
        with pytest.raises(ValueError):
            pkg.Context.sketch(None, [b"ACGT"], k, w, canonical=True)
        with pytest.raises(ValueError):
            pkg.MinimizerIndex(None, b"ACGT", k, w, canonical=True)
    for k, w in [(1, 1), (31, 128)]:                      # at the limits the Python layer goes on to the context it was not given
        with pytest.raises(AttributeError):
            pkg.MinimizerIndex(None, b"ACGT", k, w, canonical=True)
    with pytest.raises(ValueError):
        pkg.Context.index(None, b"ACGT", canonical=True)  # canonical is a property of a minimizer index


def test_the_python_layer_pairs_calls_and_index_kinds():
    pkg = load_pkg()
    for canonical, refused, message in [(True, "seed", "seed_strands"), (False, "seed_strands", "seed()")]:
        ix = object.__new__(pkg.MinimizerIndex)           # no device: the kind is checked before anything else
        ix.canonical, ix.k, ix._ix = canonical, 5, None
        with pytest.raises(ValueError, match=re.escape(message)):
            getattr(ix, refused)([b"ACGTACGT"])
        with pytest.raises(pkg.PwaError):                 # ... and the right call gets as far as the closed index
            getattr(ix, "seed_strands" if canonical else "seed")([b"ACGTACGT"])
