"""pwa_pair_form_table, pwa_pair_forms, pwa_pair_forms_reset (host side, no GPU): the listing of the pair-engine forms the library's
call sites can build, its distinctness checks behind pwa_selftest_host, and that tests/test_gpu_pair_forms.py has exactly one recipe
for every form it lists.  A form added to the generator without a recipe -- or a recipe for a form the library does not list -- fails
here, on any machine; there is no exclusion list."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg
from test_gpu_pair_forms import MINI_RL, RECIPES, WIDE

NAME = re.compile(r"^(stripe_fill|stripe_dist|stripe_affine|stripe_affine_tb|mini_fill|mini_gotoh|mini_subst)/(NW|SW|SG)/(none|tb|tb\+scores)/"
                  r"(none|ops|overlap)/(plain|keyed|coded|gap0)/rl(\d+)/(w|ln)(\d+)$")


def test_exports_and_declarations():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    for sym, args in (("pwa_pair_form_table", r"uint32_t\s+index"), ("pwa_pair_forms", r"const\s+pwa_ctx\s*\*\s*ctx"), ("pwa_pair_forms_reset", r"pwa_ctx\s*\*\s*ctx")):
        assert sym in pkg.EXPORTS and getattr(L, sym)
        assert re.search(r"\bint\s+%s\s*\(\s*%s" % (sym, args), hdr), sym


def test_listing_is_well_formed():
    table = load_pkg().pair_form_table()
    assert len(set(table)) == len(table) and len(table) >= 400
    for name in table:
        m = NAME.match(name)
        assert m, name
        family, mode, band, walk, cells, rl, unit, w = m.groups()
        rl, w = int(rl), int(w)
        assert (unit == "ln") == family.startswith("mini"), name
        if unit == "w":
            assert rl in (2, 4) and w in (1, 4), name
        else:
            assert (w == 16 and rl in MINI_RL) or (w == 64 and rl in WIDE), name
        assert (band == "none") <= (walk == "none"), name          # no walk without a band
        assert cells != "gap0" or (mode == "NW" and band != "tb+scores"), name


def test_listing_call_abi():
    pkg = load_pkg()
    L = pkg.lib()
    count, name = C.c_uint32(0), C.c_char_p()
    assert L.pwa_pair_form_table(0xffffffff, None, C.byref(count)) == -1   # PWA_E_INVALID past the end, the count all the same
    n = count.value
    assert n == len(pkg.pair_form_table())
    assert L.pwa_pair_form_table(n, C.byref(name), None) == -1 and name.value is None
    assert L.pwa_pair_form_table(n - 1, C.byref(name), None) == 0 and NAME.match(name.value.decode())
    assert L.pwa_pair_form_table(0, None, None) == 0   # every output is optional
    need = C.c_uint64(7)
    assert L.pwa_pair_forms(None, None, 0, C.byref(need)) == -1 and L.pwa_pair_forms_reset(None) == -1 and need.value == 7   # no context


def test_selftest_covers_the_listing():
    """pwa_selftest_host ends with the listing's checks: every form resolves, no name twice, a fill of its own wherever anything but
    the walk differs, a walk that follows from (engine class, rl, lanes, mode, walk) alone and differs with each of them"""
    L = load_pkg().lib()
    L.pwa_selftest_host.argtypes = [C.c_uint32]
    L.pwa_selftest_host.restype = C.c_int
    assert L.pwa_selftest_host(11) == 0


def test_every_listed_form_has_one_recipe():
    listed = load_pkg().pair_form_table()
    missing = sorted(set(listed) - set(RECIPES))
    assert not missing, "pair forms without a recipe in tests/test_gpu_pair_forms.py: %s" % missing
    stale = sorted(set(RECIPES) - set(listed))
    assert not stale, "recipes for forms the library does not list: %s" % stale
    assert all(name == r.name for name, r in RECIPES.items())   # (one recipe per name: the dict's keys; a second add() asserts)
    assert len({r.env for r in RECIPES.values()}) <= 16           # the switch sets stay in the tens
