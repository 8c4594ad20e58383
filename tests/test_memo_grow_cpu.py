"""The expansion memo's grown extension, host side (include/mzh.h mzh_set_memo_grow): the stats struct's layout,
the setter's refusals (decided before the engine is looked at, so no device is needed) and the sizes the header
and the documents state."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_abi_cpu import _c_offsets, lib  # noqa: F401  (the module's library fixture)

CSRC = os.path.join(ROOT, "muzero-hanoi_amd", "csrc")


def test_grow_info_layout_matches_header(lib, tmp_path):
    """ctypes MemoGrowInfo == struct mzh_memo_grow_info as the C compiler lays it out; mzh_memo_info is untouched"""
    fields = [f[0] for f in lib.MemoGrowInfo._fields_]
    want = [getattr(lib.MemoGrowInfo, f).offset for f in fields] + [ctypes.sizeof(lib.MemoGrowInfo)]
    assert _c_offsets("mzh_memo_grow_info", fields, tmp_path) == want
    assert want[-1] == 40
    fields = [f[0] for f in lib.MemoInfo._fields_]
    want = [getattr(lib.MemoInfo, f).offset for f in fields] + [ctypes.sizeof(lib.MemoInfo)]
    assert _c_offsets("mzh_memo_info", fields, tmp_path) == want and want[-1] == 56


@pytest.mark.parametrize("budget,log,what", [
    (-2, -1, "memo growth budget"), ((1 << 26) * 288 + 1, -1, "memo growth budget"),
    (-1, 0, "memo miss log entries"), (-1, -2, "memo miss log entries"), (-1, 1025, "memo miss log entries"),
    (0, 16, "engine NULL"), (-1, -1, "engine NULL"), ((1 << 26) * 288, 1024, "engine NULL"),
])
def test_set_memo_grow_refusals(lib, budget, log, what):
    """a value out of range is refused whatever the engine; in-range values reach the engine check"""
    L = lib.lib()
    st = L.mzh_set_memo_grow(None, budget, log)
    assert st != 0
    assert what in L.mzh_last_error().decode(), L.mzh_last_error()
    with pytest.raises(ValueError, match=what):
        lib.check(st, "mzh_set_memo_grow")


def test_stats_and_debug_refuse_null(lib):
    L = lib.lib()
    assert L.mzh_memo_grow_stats(None, None) != 0
    assert L.mzh_memo_debug_grow(None, None, None, None, None, None, None) != 0


def test_constants_are_the_documented_ones():
    """the default budget (64 MiB), the default and largest log, and the tree block's spare word the rows ride in"""
    h = open(os.path.join(CSRC, "mzh_internal.h")).read()
    assert re.search(r"#define MZH_MEMO_GROW_BUDGET_BYTES \(64ll << 20\)", h)
    assert re.search(r"#define MZH_MEMO_LOG_CAP 16\b", h) and re.search(r"#define MZH_MEMO_LOG_CAP_MAX 1024\b", h)
    assert re.search(r"#define MZH_LINK_NONE 0\b", h) and re.search(r"#define MZH_LINK_CLAIM \(-1\)", h)
    w = open(os.path.join(CSRC, "mzh_wave.hip")).read()
    blk = w[w.index("struct __align__(128) MzwBlock"):w.index('static_assert(sizeof(MzwBlock) == 128')]
    assert "uint32_t pad[2];" in blk  # 24 + 24 + 24 + 48 bytes of fields, then pad[0] at byte 120
    hdr = open(os.path.join(ROOT, "include", "mzh.h")).read()
    assert "-1 the default (64 MiB)" in hdr and "-1 the default (16)" in hdr
