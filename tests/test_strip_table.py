"""pwa_strip_table (host only, no GPU): the listing of the instantiated register-strip kernels, and that tests/test_gpu_strip_table.py has
a recipe for every kernel it lists.  An instantiation added to a strip_kernels_*.hip without a recipe fails here, on any machine."""
import ctypes as C
import os
import re

import oracle_lib as O
from conftest import ROOT, load_pkg
from test_gpu_strip_form_limits import DIST_SCORINGS, DIST_SHAPES, packed_ok, shape_list
from test_gpu_strip_table import BASE, PROFILE_FORMS, RECIPES


def listed_pairs(table):
    return {(e["R"], e["mode"], e["score"], v) for e in table for v in (BASE,) + e["variants"]}


def test_listing_is_well_formed():
    pkg = load_pkg()
    table = pkg.strip_table()
    assert len(table) >= 56
    keys = [(e["R"], e["mode"], e["score"]) for e in table]
    assert len(set(keys)) == len(keys)
    for e in table:
        assert "R=%d," % e["R"] in e["name"] and e["name"].endswith(">"), e
        assert e["R"] % 4 == 0 and e["mode"] in range(11) and e["score"] in (0, 1), e
        assert set(e["variants"]) <= set(pkg.STRIP_VARIANTS)
        # a single-strip form goes with every multi-strip one of the LANES and CELL16 kernels, and the profile forms hang on CELL16 entries
        assert ("lanes" in e["variants"]) == ("lanes_single" in e["variants"]) and ("cell16" in e["variants"]) == ("cell16_single" in e["variants"]), e
        assert "cell16" in e["variants"] or not {"prof16", "prof16_int"} & set(e["variants"]), e


def test_every_listed_kernel_has_a_recipe():
    table = load_pkg().strip_table()
    listed = listed_pairs(table)
    assert PROFILE_FORMS <= listed and not PROFILE_FORMS & set(RECIPES)
    missing = listed - set(RECIPES) - PROFILE_FORMS
    assert not missing, "strip kernels without a recipe in tests/test_gpu_strip_table.py: %s" % sorted(missing)
    stale = set(RECIPES) - listed
    assert not stale, "recipes for kernels the table does not hold: %s" % sorted(stale)
    names = {(e["R"], e["mode"], e["score"]): e["name"] for e in table}
    for key, r in RECIPES.items():
        assert r.name == names[key[:3]], (key, r.name, names[key[:3]])   # the GPU case asserts the name the library reports


def test_packed_key_bounds_are_reached_on_the_oracle():
    """the lists of tests/test_gpu_strip_form_limits.py for hw4's packed (H, dist) key, on the oracle: over the five AC-against-GT
    pairs with n + m == 4000 and the seven scorings the rule's products stay inside (and 4001 is outside), dist reaches 4000
    exactly, and H reaches +64 000 (4000 gap columns at +16) and -63 984 (3999 x 1 at 16 / -16 / -16: one mismatch and 3998 gaps)
    -- the widest values the key has to hold"""
    dists, hs = [], []
    for n, m in DIST_SHAPES:
        seqs, pa, pb = shape_list(n, m, b"ACGT", 4000)
        assert n + m == 4000 and set(seqs[pa[0]]) <= set(b"AC") and set(seqs[pb[0]]) <= set(b"GT")
        for sc in DIST_SCORINGS:
            assert packed_ok(n, m, sc) and not packed_ok(n + 1, m, sc) and (n + m + 2) * max(abs(s) for s in sc) < 65536
            d, h = O.nw_distance(seqs[pa[0]], seqs[pb[0]], *sc)
            dists.append(d)
            hs.append(h)
    assert max(dists) == 4000 and max(hs) == 64000 and min(hs) == -63984


def test_listing_call_abi():
    pkg = load_pkg()
    L = pkg.lib()
    count, name, rows = C.c_uint32(0), C.c_char_p(), C.c_int(-1)
    assert L.pwa_strip_table(0xffffffff, None, None, None, None, None, C.byref(count)) == -1   # PWA_E_INVALID past the end, the count all the same
    n = count.value
    assert n == len(pkg.strip_table())
    assert L.pwa_strip_table(n, C.byref(name), C.byref(rows), None, None, None, None) == -1 and name.value is None and rows.value == -1
    assert L.pwa_strip_table(n - 1, C.byref(name), C.byref(rows), None, None, None, None) == 0 and name.value and rows.value > 0
    assert L.pwa_strip_table(0, None, None, None, None, None, None) == 0   # every output is optional
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert "pwa_strip_table" in pkg.EXPORTS and re.search(r"\bint\s+pwa_strip_table\s*\(\s*uint32_t\s+index", hdr)
    for k, v in enumerate(pkg.STRIP_VARIANTS):   # the wrapper's names are the header's bits, in order
        assert re.search(r"#define\s+PWA_STRIP_%s\s+%du\b" % (v.upper(), 1 << k), hdr), v
