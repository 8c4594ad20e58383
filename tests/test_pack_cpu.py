"""CPU check of the weight packers (csrc/mzh_pack.cpp): tests/pack_check.cpp, built with the host
sanitizers as a stand-alone program and run as a child process (nothing is loaded into Python).  The
program maps every canonical element to the blob positions the layout comments give it, checks the
padding, the alignment and how often each layout holds an element, and compares the blob's FNV-1a hash."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

# (n_disks, support): in_dim 3, 12, 18, 33, 48 -> 1, 1, 2, 3, 3 first-layer k-blocks, both head kinds, ragged
# in_dim.  The hashes are those of the blob the packers produced while they were still part of the C ABI's
# host code (now split: the loaders that upload the blob are in csrc/mzh_api_weights.hip), recorded from that
# code with canonical weight i = i + 1: the device blob is byte-identical.
CASES = [(1, 1, "b7827b302f6215ec"), (4, 33, "0ab989dc40ac5b9d"), (6, 1, "d5adb99db29eb745"),
         (11, 33, "de9ba4f6e5d06fe5"), (16, 33, "991661f028a0f789")]


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("pack_check") / "pack_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "pack_check.cpp"),
                    os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_pack.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("n_disks,support,fnv", CASES, ids=[f"N{n}-S{s}" for n, s, _ in CASES])
def test_packed_blob_element_by_element(pack_check, n_disks, support, fnv):
    r = subprocess.run([pack_check, str(n_disks), str(support), fnv], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
