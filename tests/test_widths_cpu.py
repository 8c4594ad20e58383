"""What tests/test_widths_gpu.py rests on, checked without a GPU at every width of widths.WIDTHS (in_dim 3, 6, 15,
18, 33, 48):

  a. the C oracle is a valid reference: its initial and recurrent inference stay within the project's bars
     (latents and logits 1e-5, transformed value and reward 2e-3) of this repository's MuZeroNet in float64;
  b. the inputs reach every column: zeroing one column of representation_net.0.weight in the oracle's weights
     changes the bits of h (every column) and of a search's root_q (every k-block boundary column), so a kernel
     that ignores or misplaces a boundary column cannot pass the bit comparisons;
  c. the saliency and parameter-gradient cases are well-conditioned by the rules of saliency_ref / pgrad_ref.
     (The training cases' condition is tests/test_train_grad.py::test_baseline_inputs_are_well_conditioned.)

Measured (the oracle against float64, max |d| over the case's 37 rows; initial / recurrent call):

    width     h                    policy logits        value logits         value                reward logits  reward
    n1_s33    2.76e-07 / 4.57e-07  6.98e-08 / 1.05e-07  1.61e-07 / 2.52e-07  1.93e-04 / 1.99e-04  4.67e-08       1.22e-04
    n2_s1     3.58e-07 / 4.43e-07  1.32e-07 / 1.02e-07  6.32e-08 / 4.91e-08  6.32e-08 / 4.91e-08  3.84e-08       3.84e-08
    n5_s33    4.25e-07 / 3.58e-07  9.06e-08 / 1.08e-07  1.70e-07 / 2.70e-07  1.57e-04 / 2.10e-04  6.43e-08       1.49e-04
    n6_s1     3.45e-07 / 3.67e-07  1.67e-07 / 2.26e-07  9.34e-08 / 7.07e-08  9.34e-08 / 7.07e-08  2.71e-08       2.71e-08
    n11_s33   3.19e-07 / 3.83e-07  9.84e-08 / 1.35e-07  1.81e-07 / 2.59e-07  1.42e-04 / 1.58e-04  6.65e-08       1.56e-04
    n16_s33   2.90e-07 / 3.85e-07  1.12e-07 / 1.14e-07  1.78e-07 / 2.18e-07  1.28e-04 / 1.69e-04  5.44e-08       1.28e-04
    n16_s1    2.90e-07 / 3.85e-07  1.04e-07 / 1.22e-07  1.11e-07 / 1.32e-07  1.11e-07 / 1.32e-07  4.03e-08       4.03e-08

Zeroing one boundary column moves root_q of 11 to 20 of the search case's 40 roots; every column moves h of every
float row.  The pgrad cases pass over 0 to 6 candidates of their pools.
"""
import numpy as np
import pytest

import widths as wd

CASES = pytest.mark.parametrize("n,support", wd.WIDTHS, ids=wd.IDS)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


# ------------------------------------------------------------------------------------ a. the oracle
@CASES
def test_oracle_inference_agrees_with_float64(oracle, n, support):
    net, flat = wd.net(n, support), wd.flat(wd.net(n, support))
    x = wd.rows(n, 100 + n, 32, 5)
    h_in, a_in = wd.recurrent_case(n)
    ei = wd.float64_errors(oracle.initial_inference(flat, 3 * n, support, x), wd.initial64(net, x))
    er = wd.float64_errors(oracle.recurrent_inference(flat, 3 * n, support, h_in, a_in), wd.recurrent64(net, h_in, a_in))
    print(f"\nn{n}_s{support} initial   " + " ".join(f"{k} {e:.2e}" for k, e in ei.items()))
    print(f"n{n}_s{support} recurrent " + " ".join(f"{k} {e:.2e}" for k, e in er.items()))
    assert set(ei) == {"h", "policy_logits", "value_logits", "value"} and set(er) == set(wd.BARS)
    for what, errs in (("initial", ei), ("recurrent", er)):
        for k, e in errs.items():
            assert e <= wd.BARS[k], (what, k, e)


# ------------------------------------------------------------------------------------ b. every column counts
@CASES
def test_every_column_reaches_the_latent(oracle, n, support):
    flat = wd.flat(wd.net(n, support))
    x = wd.rows(n, 100 + n, 32, 5)
    h = oracle.initial_inference(flat, 3 * n, support, x)["h"]
    for k in range(3 * n):
        hk = oracle.initial_inference(wd.zero_column(flat, 3 * n, k), 3 * n, support, x)["h"]
        changed = (_bits(h) != _bits(hk)).any(axis=1)
        assert changed.any(), f"column {k} does not reach h"
        assert changed[32:].all(), f"column {k}: a float row's h did not move"


@CASES
def test_boundary_columns_reach_the_search(oracle, n, support):
    flat = wd.flat(wd.net(n, support))
    obs, noise, tie, u = wd.search_case(n)
    kw = dict(support=support, noise=noise, tie_idx=tie, action_u=u, temperature=1.0)
    q = oracle.search(n, 20, obs, flat=flat, **kw)["rootQ"]
    cols = wd.boundary_columns(3 * n)
    assert cols[0] == 0 and cols[-1] == 3 * n - 1
    for k in cols:
        qk = oracle.search(n, 20, obs, flat=wd.zero_column(flat, 3 * n, k), **kw)["rootQ"]
        moved = _bits(q) != _bits(qk)
        print(f"n{n}_s{support} column {k}: root_q of {int(moved.sum())} / {len(q)} roots moved")
        assert moved.any(), f"column {k} does not reach root_q"


# ------------------------------------------------------------------------------------ c. conditioning
@CASES
def test_saliency_case_is_well_conditioned(n, support):
    ref = wd.saliency_reference(n, support)
    ref.report(f"n{n}_s{support}")
    assert len(ref.obs) == wd.NROWS and ref.bad.size == 0


@CASES
def test_pgrad_case_is_well_conditioned(n, support):
    ref = wd.pgrad_reference(n, support)
    ref.report(f"n{n}_s{support} (rejected {ref.rejected})")
    assert len(ref.obs) == wd.NROWS and ref.bad.size == 0 and ref.near0_rows.size == 0
    assert ref.forced.any() and (~ref.forced).any()  # both policy objectives
    assert (np.abs(ref.obs[:32]).sum(axis=1) == n).all() and (ref.obs[32:] != 0).all()  # 32 states, 5 float rows
