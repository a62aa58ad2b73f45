"""The host-side view of the packed profile form's integer row (pwalign.hip, batch_scores.hip.h), without a device, through
pwa_profile_plan: how many leading 8-column blocks of a task prefetch their texts with plain loads.  There is one instantiation
of the integer kernel (the one that tests each pair of rows for the pattern's end), so a task list selects nothing else.  The
block bound is checked against a restatement of the kernel's two kinds of load: below the bound the clamped, masked word() of
every lane equals the plain word, and at the bound it does not for the task's shortest text."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, load_pkg

PAD = 12
LENGTHS = [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 256, 257]


def plan(min_len, max_len):
    L = load_pkg().lib()
    interior, blocks = C.c_uint32(99), C.c_uint32(99)
    rc = L.pwa_profile_plan(min_len, max_len, C.byref(interior), C.byref(blocks))
    assert rc == 0, rc
    return interior.value, blocks.value


def word(text, w):
    """the kernel's word(): 4 columns from column 4w of a text, the word index clamped into the text, codes past its end the pad"""
    ml = len(text)
    wi = min(w, max((ml - 1) >> 2, 0))
    raw = list(text[4 * wi:4 * wi + 4]) + [0xEE] * 4        # (the arena's slack: anything)
    valid = ml - 4 * w
    return [raw[k] if k < valid else PAD for k in range(4)]


def plain(text, w):
    """the interior blocks' load: the 4 bytes at 4w, whatever they are"""
    raw = list(text[4 * w:4 * w + 4])
    return raw + [0xEE] * (4 - len(raw))


def prefetch_is_plain(lens, jb):
    """block jb prefetches words 2 jb + 2 and 2 jb + 3 of every text: True when the plain load gives word()'s value in every lane"""
    texts = [bytes((i + 3 * k) & 3 for k in range(m)) for i, m in enumerate(lens)]
    return all(word(t, w) == plain(t, w) for t in texts for w in (2 * jb + 2, 2 * jb + 3))


@pytest.mark.parametrize("min_len", LENGTHS + [40, 57, 137])
def test_interior_block_count_is_the_exact_bound(min_len):
    """lanes whose texts differ by 0, 1, 7, 8, 9 columns and by several blocks: the bound goes by the shortest, the length by the longest"""
    for diff in (0, 1, 7, 8, 9, 40, 200):
        max_len = min_len + diff
        lens = sorted({min_len, max_len, min_len + diff // 2, max(min_len, max_len - 1)})
        interior, blocks = plan(min_len, max_len)
        assert blocks == (max_len + 7) // 8
        assert interior == max(min_len // 8 - 1, 0) and interior <= blocks
        for jb in range(interior):
            assert prefetch_is_plain(lens, jb), (lens, jb)
        if interior < blocks:   # the first block past the bound needs the mask (or the clamp) in the shortest text's lane
            assert not prefetch_is_plain(lens, interior), (lens, interior)


def test_no_interior_block_and_no_masked_column():
    assert plan(7, 7) == (0, 1)            # every text shorter than a block
    assert plan(1, 15) == (0, 2)
    assert plan(15, 15) == (0, 2)
    assert plan(16, 16) == (1, 2)          # block 0 prefetches bytes 8..15: whole
    assert plan(64, 64) == (7, 8)          # all equal, a multiple of 8: only the last block's prefetch (of nothing) is masked
    assert plan(57, 257) == (6, 33)
    assert plan(10000, 10000) == (1249, 1250)   # the benchmark's task


def test_plan_rejects_bad_arguments():
    L = load_pkg().lib()
    a, b = C.c_uint32(), C.c_uint32()
    assert L.pwa_profile_plan(9, 8, C.byref(a), C.byref(b)) == -1     # PWA_E_INVALID: shortest > longest
    assert L.pwa_profile_plan(8, 8, None, C.byref(b)) == -1
    assert L.pwa_profile_plan(8, 8, C.byref(a), None) == -1
    assert L.pwa_profile_plan(0, 0, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)


def test_entry_point_is_exported_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pwalign.h")).read(), flags=re.S)
    assert hasattr(L, "pwa_profile_plan") and "pwa_profile_plan" in pkg.EXPORTS
    assert re.search(r"\bint\s+pwa_profile_plan\s*\(\s*uint32_t", hdr)
