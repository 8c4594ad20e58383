"""The search kernel divides with y = RN(1/b) and one fma correction step (csrc/mzh_mcts.h
mzh_div, Markstein's theorem) instead of the long IEEE division sequence; the reference divides
with Python floats (node.py:98-121, utils_mcts.py:12-16).  The two must agree bit for bit on the
operand domains the search produces.  The fp32 form (csrc/mzh_device.h mzh_fdiv) serves the latent
normalisation and the replay draw's P_i = p_i / np.sum(p); it is exact only while y is a normal float."""
import ctypes

import numpy as np


def test_markstein_division_is_ieee(oracle):
    assert oracle.lib().orc_markstein_mismatches(20_000_000, 12345) == 0


# a / s with 1/s subnormal, found by emulating mzh_fdiv's three operations in exact rational arithmetic
FIX_A, FIX_S, FIX_IEEE = 0x7E8316A4, 0x7F6937D4, 1049617618


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def test_markstein_f32_is_ieee_up_to_2_126_and_not_above(oracle):
    """mzh_fdiv over the replay draw's domain, 0 <= a <= b: equal to IEEE division wherever `slow` is clear for
    every normal b up to 2^126 (the largest b with a normal reciprocal), and NOT above it: there y = RN(1/b) is
    subnormal, its relative error reaches 2^-22, and a quotient within ~2^-20 ulp of a rounding boundary comes
    out one ulp off -- about 1 result in 10^7 (seeds 1..6 of this sweep find 1, 0, 1, 0, 3, 2 in 20,000,000
    each), so the replay kernel divides in IEEE there.  The fixture pair is asserted by itself too, so that the
    second half does not hinge on the seed."""
    L = oracle.lib()
    assert L.orc_markstein_f32_mismatches(20_000_000, 12345, 0) == 0
    a, s = _f32(FIX_A), _f32(FIX_S)
    slow = ctypes.c_int(-1)
    got = np.float32(L.orc_markstein_f32(float(a), float(s), ctypes.byref(slow)))
    assert (a / s).view(np.uint32) == FIX_IEEE
    assert slow.value == 0 and got.view(np.uint32) == FIX_IEEE - 1  # one ulp low, and not flagged
    assert L.orc_markstein_f32_mismatches(20_000_000, 5, 1) > 0
