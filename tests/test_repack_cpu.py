"""The device repack (mzh_load_weights_device, csrc/mzh_repack.hip), the checks that need no GPU: the pack maps
the gather kernel applies (tests/pack_map_check.cpp, built with the host sanitizers as a stand-alone program and
run as a child process; nothing is loaded into Python under a sanitizer), and the C boundary -- the symbols, the
host-only mzh_pack_map, and the argument errors, which are refused before any device work."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_pack_cpu import CASES

HEADER = os.path.join(ROOT, "include", "mzh.h")
SYMBOLS = ("mzh_load_weights_device", "mzh_load_weight_set_device", "mzh_pack_map", "mzh_weights_debug_blob")
FAKE = 0x1000  # a non-NULL pointer the argument checks must not dereference


@pytest.fixture(scope="module")
def pack_map_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("pack_map_check") / "pack_map_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "pack_map_check.cpp"),
                    os.path.join(ROOT, "muzero-hanoi_amd", "csrc", "mzh_pack.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def lib():
    from muzero_hanoi_amd import build

    build.build()
    from muzero_hanoi_amd import _lib

    return _lib


def _pack_map(lib, n_disks, support, which):
    """mzh_pack_map -> (map int32 [n], scalar sources [2])"""
    L = lib.lib()
    n, scal = ctypes.c_size_t(), (ctypes.c_int64 * 2)()
    assert L.mzh_pack_map(n_disks, support, which, None, ctypes.byref(n), None) == lib.MZH_OK, lib.last_error()
    m = np.empty(n.value, np.int32)
    n2 = ctypes.c_size_t()
    assert L.mzh_pack_map(n_disks, support, which, m.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n2), scal) == lib.MZH_OK
    assert n2.value == n.value
    return m, [scal[0], scal[1]]


@pytest.mark.parametrize("n_disks,support,fnv", CASES, ids=[f"N{n}-S{s}" for n, s, _ in CASES])
def test_pack_maps_reproduce_the_packers(pack_map_check, lib, n_disks, support, fnv):
    r = subprocess.run([pack_map_check, str(n_disks), str(support), fnv], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n_main, n_trans = (int(x) for x in r.stdout.split())
    # the host-only ABI call needs no device and agrees with the program
    total = ctypes.c_size_t()
    assert lib.lib().mzh_weights_size(n_disks, support, ctypes.byref(total)) == lib.MZH_OK
    main, scal = _pack_map(lib, n_disks, support, 0)
    trans, scal_t = _pack_map(lib, n_disks, support, 1)
    assert (main.size, trans.size) == (n_main, n_trans) and scal == scal_t
    assert main.size % 4 == 0 and trans.size % 4 == 0  # a thread of the gather owns one float4
    for m in (main, trans):
        assert m.min() >= -1 and m.max() < total.value
    assert np.array_equal(np.unique(main[main >= 0]), np.arange(total.value))  # every weight reaches the main blob
    if support == 33:  # bias bin 32 of the reward and the value head: the last element of layers 5 and 9
        sizes = [256 * 3 * n_disks + 256, 64 * 256 + 64, 256 * 70 + 256, 64 * 256 + 64, 256 * 64 + 256, 33 * 256 + 33,
                 256 * 64 + 256, 6 * 256 + 6, 256 * 64 + 256, 33 * 256 + 33]
        assert scal == [sum(sizes[:6]) - 1, sum(sizes) - 1] and sum(sizes) == total.value
    else:
        assert scal == [-1, -1]


def test_symbols_declared_exported_and_abi_version_unchanged(lib):
    L = lib.lib()
    hdr = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.SIGNATURES, name
    assert "int mzh_load_weights_device(mzh_engine* eng, const float* const* param, mzh_stream stream);" in hdr
    assert "int mzh_load_weight_set_device(mzh_engine* eng, const float* const* param, int M, mzh_stream stream);" in hdr
    assert "int mzh_pack_map(int n_disks, int support, int which, int32_t* map" in hdr
    assert "int mzh_weights_debug_blob(mzh_engine* eng, int which, float* dst" in hdr
    assert "#define MZH_ABI_VERSION 6" in hdr and L.mzh_abi_version() == lib.ABI_VERSION == 6


def test_pack_map_argument_errors(lib):
    L = lib.lib()
    n = ctypes.c_size_t()
    for n_disks, support in ((0, 33), (17, 33), (-1, 1), (3, 2), (3, 0), (3, 32)):  # what mzh_weights_size refuses
        assert L.mzh_weights_size(n_disks, support, ctypes.byref(n)) == lib.MZH_ERR_ARG
        assert L.mzh_pack_map(n_disks, support, 0, None, ctypes.byref(n), None) == lib.MZH_ERR_ARG == -1
        assert f"n_disks={n_disks}" in lib.last_error() and f"support={support}" in lib.last_error()
    for which in (-1, 2, 7):
        assert L.mzh_pack_map(3, 33, which, None, ctypes.byref(n), None) == lib.MZH_ERR_ARG
        assert f"got {which}" in lib.last_error()
    assert L.mzh_pack_map(3, 33, 1, None, None, None) == lib.MZH_OK  # every output is optional


def test_device_load_argument_errors_without_device(lib):
    """refused before any device work: no engine exists here, and a fake one is never dereferenced"""
    L = lib.lib()
    ptrs = (ctypes.c_void_p * 60)(*([FAKE] * 60))
    holed = (ctypes.c_void_p * 60)(*([FAKE] * 60))
    holed[13] = None
    assert L.mzh_load_weights_device(None, ptrs, None) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    assert L.mzh_load_weights_device(FAKE, None, None) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    assert L.mzh_load_weights_device(FAKE, holed, None) == lib.MZH_ERR_ARG and "param[13] is NULL" in lib.last_error()
    assert L.mzh_load_weight_set_device(None, ptrs, 3, None) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    assert L.mzh_load_weight_set_device(FAKE, None, 3, None) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    holed[13], holed[47] = FAKE, None
    assert L.mzh_load_weight_set_device(FAKE, holed, 3, None) == lib.MZH_ERR_ARG
    assert "param[2][7] is NULL" in lib.last_error()
    for M in (0, -1, 257, 100000):
        assert L.mzh_load_weight_set_device(FAKE, ptrs, M, None) == lib.MZH_ERR_ARG
        assert f"got {M}" in lib.last_error() and "[1,256]" in lib.last_error()


def test_debug_blob_argument_errors_without_device(lib):
    L = lib.lib()
    n = ctypes.c_size_t()
    assert L.mzh_weights_debug_blob(None, 0, None, ctypes.byref(n)) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    assert L.mzh_weights_debug_blob(FAKE, 0, None, None) == lib.MZH_ERR_ARG and "NULL" in lib.last_error()
    for which in (-1, 4):
        assert L.mzh_weights_debug_blob(FAKE, which, None, ctypes.byref(n)) == lib.MZH_ERR_ARG
        assert f"got {which}" in lib.last_error()


def test_weight_shapes_are_the_canonical_layer_table(lib):
    """engine.weight_shapes (what load_weights_from validates against) sums to mzh_weights_size"""
    from muzero_hanoi_amd import engine

    for n_disks, support, _ in CASES:
        shapes = engine.weight_shapes(n_disks, support)
        n = ctypes.c_size_t()
        assert lib.lib().mzh_weights_size(n_disks, support, ctypes.byref(n)) == lib.MZH_OK
        assert len(shapes) == len(engine.WEIGHT_KEYS) == 20
        assert sum(int(np.prod(s)) for s in shapes) == n.value
