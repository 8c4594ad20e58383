"""The wave kernels' tree block (csrc/mzh_wave.hip MzwBlock) as the compiler lays selection's loads out.

The layout's gain rests on a selection level being exactly four aligned 16-byte loads per lane.  The compiler,
left alone, loads the first child unit's W a second time as a dwordx2 beside the dwordx4 (five loads, 18 dwords),
and the layout then measures slower than the one it replaced; an empty asm on that unit's
words prevents it.  That depends on the compiler, so this test compiles the file for the device (no GPU needed)
and looks at the instructions: in every one of the eight instantiations, every group of loads off one block
half's address is four `global_load_dwordx4` at byte offsets 0, 16, 32, 48 and nothing else.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

LOAD = re.compile(r"\b(global_load_\w+)\s+v\[?[\d:]+\]?,\s*(v\[\d+:\d+\]),\s*off(?:\s+offset:(\d+))?")


def level_groups(asm):
    """per kernel name: the loads sharing the address register pair of each `dwordx4 ... offset:48`, as sorted
    (instruction, offset) lists; the loads of one level stand within a few lines of each other"""
    out, name, lines = {}, None, asm.splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"^(\w+):", ln)  # a function's label (block labels start with a dot)
        if m:
            name = m.group(1) if "mzh_wave_kernel" in m.group(1) else None
            if name:
                out[name] = []
        ld = LOAD.search(ln)
        if name is None or not ld or ld.group(1) != "global_load_dwordx4" or ld.group(3) != "48":
            continue
        base, grp = ld.group(2), []
        for other in lines[max(0, i - 8): i + 9]:
            o = LOAD.search(other)
            if o and o.group(2) == base:
                grp.append((o.group(1), int(o.group(3) or 0)))
        out[name].append(sorted(grp))
    return out


@pytest.fixture(scope="module")
def wave_asm(tmp_path_factory):
    from muzero_hanoi_amd import build as b

    if not os.path.exists(b.HIPCC):
        pytest.fail(f"{b.HIPCC}: the device compiler the library is built with is missing")
    dst = tmp_path_factory.mktemp("wave") / "mzh_wave.s"
    cmd = [b.HIPCC, *b.FLAGS, *b.SOURCE_FLAGS.get("mzh_wave.hip", []), "--cuda-device-only", "-S",
           os.path.join(b.CSRC, "mzh_wave.hip"), "-o", str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return dst.read_text()


def test_a_selection_level_is_four_aligned_16_byte_loads(wave_asm):
    groups = level_groups(wave_asm)
    assert len(groups) == 8, sorted(groups)  # NT = 1, 2 x REPLAY x SUP33
    want = [("global_load_dwordx4", o) for o in (0, 16, 32, 48)]
    for name, gs in groups.items():
        # the walk is instantiated twice per kernel (the exact and the Markstein normaliser)
        assert len(gs) >= 2, (name, gs)
        for g in gs:
            assert g == want, (name, g)


def test_the_grouping_sees_a_split_load():
    """the form the compiler gave the first build: the first unit's W again as a dwordx2 off the same address"""
    bad = """_Z15mzh_wave_kernelILi2ELb0ELb1EEv7MzhWNet15MzhSearchParams:
\tglobal_load_dwordx4 v[58:61], v[80:81], off offset:48
\tglobal_load_dwordx4 v[34:37], v[80:81], off offset:32
\tglobal_load_dwordx4 v[62:65], v[80:81], off offset:16
\tglobal_load_dwordx4 v[66:69], v[80:81], off
\tglobal_load_dwordx2 v[66:67], v[80:81], off
"""
    (g,) = level_groups(bad)["_Z15mzh_wave_kernelILi2ELb0ELb1EEv7MzhWNet15MzhSearchParams"]
    assert ("global_load_dwordx2", 0) in g and len(g) == 5


def test_block_struct_is_the_documented_layout():
    """two 64-byte halves, each three 16-byte units, three priors and the row word (source text; the sizes and
    offsets themselves are static_asserts of the file, checked by every build)"""
    w = open(os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_wave.hip")).read()
    blk = w[w.index("struct MzwUnit"):w.index('static_assert(sizeof(MzwBlock) == 128')]
    assert "uint32_t row1;" in blk and "MzwHalf h[2];" in blk and "sizeof(MzwHalf) == 64" in blk
    assert "__builtin_offsetof(MzwHalf, row1) == 60" in blk
    assert not re.search(r"^\s*uint32_t pad\[2\];", blk, re.M)  # no spare word: only a comment still names it
