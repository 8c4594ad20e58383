"""The fused training update's gradients (csrc/mzh_train.hip) against a float64 reference.

tests/test_training.py sees the fused update only through Adam's first steps, which move every
parameter by ~lr * sign(g) whatever the size of g.  Here the gradient itself is read out of
mzh_train_update: with beta1 = beta2 = 0, step_size = 0, bc2_sqrt = 1, eps = 1 and zeroed moments,
adam() computes m = 0 + 1 * (g - 0), so afterwards

    exp_avg[i]     the kernel's fp32 gradient of parameter i, bit for bit
    exp_avg_sq[i]  g * g
    param[i]       unchanged (p + (-0) * x), asserted bit for bit

for i = 0..19 in state_dict order (representation, dynamics, reward, policy, value net; layer 1
weight, bias, layer 2 weight, bias), each in torch's own shape ([out][in] weights, [out] biases).

The reference is the project's torch path (muzero.unrolled_losses, importance weights, mean, the
1/U hook, backward) on a float64 copy of the net (train_ref.torch_grads).  The same function in
float32 is the baseline: for every compared tensor the kernel's errors

    e_max = max|x - x64| / max|x64|        e_fro = ||x - x64||_2 / ||x64||_2

must stay within max(4 x the fp32 torch baseline's error of that tensor, floor).  The factor 4
covers other summation orders and a ReLU or arg-min / arg-max of the latent normalisation flipping
at rounding noise in one implementation only; the floor is the largest baseline error over all
cases and tensors, because such a flip can hit the kernel alone.  A case whose baseline passes
1e-2 in any tensor has a near-tie in a min / max normalisation and is a bad input: the test asserts
that instead of letting the bound grow (pick another seed).

Measured (torch-CPU fp32 baseline against fp64, this module's generator, seed 0 everywhere):
FLOOR_MAX = 7.59e-5 and FLOOR_FRO = 6.36e-5 are the largest e_max / e_fro of that baseline.  Worst
tensor per case, baseline and kernel (MI355X; rows = 1 and rows = 2 gave the same figures), and
whether rows = 1 and rows = 2 gave the same bits:

    case                     baseline e_max  e_fro      kernel e_max  e_fro      rows 1 == rows 2
    n3_s33_B24_U5            4.77e-05        4.97e-05   4.47e-05      3.95e-05   bit-identical
    n3_s33_B103_U5           3.02e-05        2.90e-05   5.02e-05      4.06e-05   bit-identical
    n3_s33_B515_U5           6.60e-05        4.64e-05   3.27e-05      3.13e-05   bit-identical
    n4_s1_B515_U5_uniform    1.16e-06        6.91e-07   4.93e-07      4.60e-07   bit-identical
    n4_s1_B24_U5             3.82e-07        3.38e-07   5.25e-07      5.24e-07   bit-identical
    n7_s33_B129_U5           7.59e-05        6.36e-05   6.33e-05      5.41e-05   bit-identical
    n3_s33_B33_U7            2.35e-05        2.34e-05   2.76e-05      2.26e-05   bit-identical
    n4_s33_B7_U1             6.87e-05        5.51e-05   6.67e-05      5.51e-05   bit-identical
    n7_s1_B2_U5              4.68e-07        3.65e-07   4.41e-07      4.22e-07   bit-identical
    n1_s33_B24_U5            6.70e-05        5.81e-05   6.99e-05      6.01e-05   bit-identical
    n1_s1_B7_U1              6.91e-07        3.47e-07   4.93e-07      4.62e-07   bit-identical
    n5_s33_B24_U5            5.39e-05        4.33e-05   5.80e-05      4.50e-05   bit-identical
    n6_s1_B24_U5             8.76e-07        6.15e-07   6.46e-07      6.13e-07   bit-identical
    n10_s33_B33_U5           2.00e-04        1.82e-04   2.13e-04      1.94e-04   bit-identical
    n10_s1_B24_U5            5.57e-07        3.22e-07   4.80e-07      3.61e-07   bit-identical

The last six rows cover the observation widths the update accepts beyond 9 to 21: in_dim 3, 15, 18 and 30 (the
widest; the rows kernel stages the observation as [R][32] and train_check refuses in_dim > 32).  The floors are
those of the first nine cases and stay there: n10_s33_B33_U5's baseline is larger than both, and its bound is
4 x its own baseline like any other case's.

The baseline moves with the host's torch build and thread count (a second host gave 7.02e-05 / 5.98e-05 for
n7_s33_B129_U5, 2.92e-04 / 2.57e-04 for n1_s33_B24_U5 and 1.11e-04 / 1.02e-04 for n10_s33_B33_U5); the floors are
the larger figures of the first nine.  With support 33 both
torch fp32 and the kernel are dominated by the cancellation in the signed parabolic transform
(sqrt(.) / 2 / eps - 1 / 2 / eps), which the kernel evaluates op by op as torch does.
"""
import functools
import math

import numpy as np
import pytest
import torch

import train_ref as tr

FLOOR_MAX = 7.59e-5  # largest baseline e_max seen (n7_s33_B129_U5)
FLOOR_FRO = 6.36e-5  # largest baseline e_fro seen (n7_s33_B129_U5)
BAD_INPUT = 1e-2

# name: (N, support, B, U, importance weights given, seed)
CASES = {
    "n3_s33_B24_U5": (3, 33, 24, 5, True, 0),     # the fixture's shape, with real weights
    "n3_s33_B103_U5": (3, 33, 103, 5, True, 0),   # M = 515 = 512 + 3: second row pass, tail not a multiple of 4, odd B
    "n3_s33_B515_U5": (3, 33, 515, 5, True, 0),   # M = B = 515 on the representation layers, 2575 on the step layers
    "n4_s1_B515_U5_uniform": (4, 1, 515, 5, False, 0),  # support 1 (LD_GS = 16), weights and new_prio NULL
    "n4_s1_B24_U5": (4, 1, 24, 5, True, 0),       # support 1 with importance weights
    "n7_s33_B129_U5": (7, 33, 129, 5, True, 0),   # in_dim 21: partial second k-block of rep1
    "n3_s33_B33_U7": (3, 33, 33, 7, True, 0),     # U != 5: the LDS per-step plan, acts indexing
    "n4_s33_B7_U1": (4, 33, 7, 1, True, 0),       # U = 1, one tail workgroup at rows = 2
    "n7_s1_B2_U5": (7, 1, 2, 5, True, 0),         # the smallest batch the reference supports
    "n1_s33_B24_U5": (1, 33, 24, 5, True, 0),     # in_dim 3: the narrowest observation, 29 unused stage columns
    "n1_s1_B7_U1": (1, 1, 7, 1, True, 0),         # in_dim 3 with support 1, U = 1
    "n5_s33_B24_U5": (5, 33, 24, 5, True, 0),     # in_dim 15: one column short of a 16-column block
    "n6_s1_B24_U5": (6, 1, 24, 5, True, 0),       # in_dim 18: two columns into the second block
    "n10_s33_B33_U5": (10, 33, 33, 5, True, 0),   # in_dim 30: the widest accepted, two columns from the stage's end
    "n10_s1_B24_U5": (10, 1, 24, 5, True, 0),     # in_dim 30 with support 1
}


@functools.lru_cache(maxsize=None)
def reference(case):
    """net, batch, names, the fp64 reference and the fp32 torch baseline's errors against it"""
    n, support, B, U, use_w, seed = CASES[case]
    net = tr.make_net(n, support, seed)
    batch = tr.make_batch(n, B, U, seed)
    if not use_w:
        batch = batch[:5] + (None,)
    names = list(net.state_dict().keys())
    ref = tr.torch_grads(net, batch, U, torch.float64)
    base = tr.compare(names, tr.torch_grads(net, batch, U, torch.float32), ref)
    return net, batch, names, ref, base


def bounds(base):
    return {k: (max(4 * e[0], FLOOR_MAX), max(4 * e[1], FLOOR_FRO)) for k, e in base.items()}


def report(title, errs, base, bnd):
    print(f"\n{title}\n{'tensor':34s} {'e_max':>9s} {'base':>9s} {'bound':>9s}   {'e_fro':>9s} {'base':>9s} {'bound':>9s}")
    for k, e in errs.items():
        print(f"{k:34s} {e[0]:9.2e} {base[k][0]:9.2e} {bnd[k][0]:9.2e}   {e[1]:9.2e} {base[k][1]:9.2e} {bnd[k][1]:9.2e}")
    print(f"worst: kernel e_max {max(e[0] for e in errs.values()):.2e} e_fro {max(e[1] for e in errs.values()):.2e}; "
          f"baseline e_max {max(e[0] for e in base.values()):.2e} e_fro {max(e[1] for e in base.values()):.2e}")


# ---------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", list(CASES))
def test_baseline_inputs_are_well_conditioned(case):
    """the condition the bound rests on: the fp32 torch baseline of every case stays under 1e-2 in
    every tensor (else the input has a near-tie in a min / max normalisation: another seed)"""
    base = reference(case)[4]
    print(f"\n{case}: baseline e_max {max(e[0] for e in base.values()):.2e} e_fro {max(e[1] for e in base.values()):.2e}")
    bad = {k: e for k, e in base.items() if max(e) >= BAD_INPUT}
    assert not bad, bad


def test_written_out_losses_equal_unrolled_losses():
    """the op-by-op copy the deliberate errors are switched into is muzero.unrolled_losses"""
    net, batch, names, ref, _ = reference("n3_s33_B24_U5")
    n, support, B, U, use_w, seed = CASES["n3_s33_B24_U5"]
    out = tr.torch_grads(net, batch, U, torch.float64, written_out=True)
    assert all(torch.equal(a, b) for a, b in zip(out[0], ref[0]))
    assert torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])


@pytest.mark.parametrize("variant", tr.VARIANTS)
def test_bound_discriminates(variant):
    """One deliberate error at a time in the fp64 reference -- (a) the 0.5 latent hook removed, (b) w
    ignored, (c) the 1/U factor dropped, (d) the policy backward assuming sum(pi) = 1 -- moves at
    least one tensor's e_fro to 10 x the bound the GPU test applies to that tensor or further."""
    case = "n3_s33_B24_U5"
    net, batch, names, ref, base = reference(case)
    U = CASES[case][3]
    errs = tr.compare(names, tr.torch_grads(net, batch, U, torch.float64, variant=variant), ref)
    bnd = bounds(base)
    ratio = {k: errs[k][1] / bnd[k][1] for k in errs}
    k = max(ratio, key=ratio.get)
    print(f"\n{variant}: e_fro {min(e[1] for e in errs.values()):.3g} .. {max(e[1] for e in errs.values()):.3g}; "
          f"largest e_fro / bound = {ratio[k]:.3g} at {k}")
    assert ratio[k] >= 10, (k, errs[k], bnd[k])


def lds_bytes_rows1(U):
    """RowLds<1>::bytes(U) of csrc/mzh_train.hip"""
    F, H, RNT = 256, 64, 512
    per_step = ((4 * F + H + 8 + 48 + 48) + 2 + 3) & ~3
    fixed = (32 + F + 4 * H + 8 + 48 + 48 + 4 * F + 12 * RNT) + 8 + 64
    return 4 * (fixed + U * per_step)


U_LDS = 28  # the smallest U whose rows = 1 LDS plan passes 160 KB


def _refusal_call(U=5, rows=1, **kw):
    dev = "cuda" if torch.cuda.is_available() else "cpu"  # nothing may be launched: host memory will do
    return tr.TrainCall(tr.make_net(3, 33, 0), tr.make_batch(3, 4, U, 0), U, rows, dev, **kw)


REFUSALS = {
    "rows2_U40": (dict(U=40, rows=2), None, "rows * U"),
    "rows3": (dict(rows=3), None, "rows must be"),
    "in_dim33": (dict(), lambda a: setattr(a, "in_dim", 33), "in_dim=33"),
    "support2": (dict(), lambda a: setattr(a, "support", 2), "support=2"),
    "scratch_one_byte_short": (dict(scratch_short=1), None, "too small"),
    "null_exp_avg7": (dict(), lambda a: a.exp_avg.__setitem__(7, None), "pointer 7"),
    "lds_U28_rows1": (dict(U=U_LDS, rows=1), None, "LDS"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    """train_check refuses before any launch: MZH_ERR_ARG, the reason named, every output untouched"""
    assert lds_bytes_rows1(U_LDS) > 160 * 1024 >= lds_bytes_rows1(U_LDS - 1) and U_LDS <= 64
    kw, poke, msg = REFUSALS[what]
    tc = _refusal_call(**kw)
    if poke:
        poke(tc.a)
    assert tc.update() == tc.L.MZH_ERR_ARG
    assert msg in tc.L.last_error(), tc.L.last_error()
    assert tc.outputs_untouched()


# ---------------------------------------------------------------------------------------- GPU
_KERNEL = {}  # (case, rows) -> the kernel's raw fp32 outputs, for the rows 1 / rows 2 bit comparison


def kernel_grads(case, rows):
    """one gradient-extraction call: (grads, row_loss, new_prio or None) as the kernel wrote them"""
    net, batch, names, ref, base = reference(case)
    n, support, B, U, use_w, seed = CASES[case]
    tc = tr.TrainCall(net, batch, U, rows, "cuda", use_w=use_w, want_prio=use_w)
    assert tc.transpose() == tc.L.MZH_OK, tc.L.last_error()
    assert tc.wt_matches_params()
    assert tc.update() == tc.L.MZH_OK, tc.L.last_error()
    for p, q in zip(tc.param, tc.param_in):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), "parameters moved in a gradient-extraction call"
    assert tc.wt_matches_params()
    for m, v in zip(tc.exp_avg, tc.exp_avg_sq):
        assert torch.equal(v, m * m)
    out = ([m.cpu() for m in tc.exp_avg], tc.row_loss.cpu().clone(), tc.new_prio.cpu().clone() if use_w else None)
    _KERNEL[(case, rows)] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_gradient_vs_fp64(case, rows):
    """every parameter gradient, row_loss column and new_prio of the fused update within
    max(4 x fp32 torch baseline, floor) of the fp64 reference, at rows = 1 and rows = 2"""
    net, batch, names, ref, base = reference(case)
    assert max(max(e) for e in base.values()) < BAD_INPUT, "bad input: near-tie in a normalisation, pick another seed"
    got = kernel_grads(case, rows)
    errs = tr.compare(names, got, ref)
    bnd = bounds(base)
    report(f"{case} rows={rows}", errs, base, bnd)
    other = _KERNEL.get((case, 3 - rows))
    if other is not None:
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[0], other[0]))
        same = same and torch.equal(got[1].view(torch.int32), other[1].view(torch.int32))
        print(f"rows=1 and rows=2 bit-identical: {same}")
    bad = {k: (errs[k], bnd[k]) for k in errs if errs[k][0] > bnd[k][0] or errs[k][1] > bnd[k][1]}
    assert not bad, bad


@pytest.mark.gpu
def test_adam_moments_and_transposed_copies():
    """A real Adam step (step 4 of lr 0.002, betas 0.9 / 0.999, eps 1e-8) from random moments, against
    float64 in adam()'s order, with g taken from a gradient-extraction call on the same inputs (the
    kernels sum in a fixed order without atomics; two extraction calls are asserted bit-identical).
    The float64 side uses the fp32-rounded constants the kernel receives; 1 - beta is exact in fp32.
    u = 2^-24 = eps32 / 2, roundings counted along the longest chain (the build has no FMA contraction):
      m' = m + c1 (g - m)         3 roundings: |dm| <= 3u (|m| + |c1 (g - m)|)   (no cancellation-free form)
      v' = v b2 + c2 (g g)        3 roundings, all terms >= 0: |dv| <= 3u v' (+ 2^-125 where g g is denormal)
      denom = sqrt(v')/bc2 + eps  1.5u + 3 roundings = 4.5u relative
      p' = p - ss (m'/denom)      the term: 3u (from m') + 4.5u + 2 roundings = 9.5u of ss (|m| + |c1 (g - m)|)/denom,
                                  the sum one more rounding of |p'| <= |p| + |term|:
                                  |dp| <= 10.5u (|p| + ss (|m| + |c1 (g - m)|)/denom)  -> k = 5.5 eps32
    Then wt[l] == param[2l].T bit for bit with zero pad columns, after the update and after a
    mzh_train_transpose that follows a weight written from torch."""
    case = "n3_s33_B24_U5"
    net, batch, names, ref, base = reference(case)
    U = CASES[case][3]
    g1 = kernel_grads(case, 1)[0]
    g2 = kernel_grads(case, 1)[0]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g1, g2))
    f32 = lambda x: float(np.float32(x))
    lr, beta1, beta2, eps, step = 0.002, 0.9, 0.999, 1e-8, 4
    hyper = dict(step_size=lr / (1 - beta1 ** step), bc2_sqrt=math.sqrt(1 - beta2 ** step), beta1=beta1, beta2=beta2,
                 eps=eps)
    ss, bc2, b2, e = f32(hyper["step_size"]), f32(hyper["bc2_sqrt"]), f32(beta2), f32(eps)
    c1, c2 = float(np.float32(1) - np.float32(beta1)), float(np.float32(1) - np.float32(beta2))
    tc = tr.TrainCall(net, batch, U, 1, "cuda")
    gen = torch.Generator().manual_seed(1)
    for g, m, v in zip(g1, tc.exp_avg, tc.exp_avg_sq):
        rms = float(g.double().pow(2).mean().sqrt())
        m.copy_(torch.randn(g.shape, generator=gen) * rms)
        v.copy_(torch.rand(g.shape, generator=gen) * rms * rms)
    m0 = [m.cpu().double() for m in tc.exp_avg]
    v0 = [v.cpu().double() for v in tc.exp_avg_sq]
    tc.set_adam(**hyper)
    assert tc.transpose() == tc.L.MZH_OK
    assert tc.update() == tc.L.MZH_OK, tc.L.last_error()
    u = 2.0 ** -24
    for k, g, m, v, p, mk, vk, pk in zip(names, g1, m0, v0, tc.param_in, tc.exp_avg, tc.exp_avg_sq, tc.param):
        g, p = g.double(), p.cpu().double()
        inc = c1 * (g - m)
        m1 = m + inc
        v1 = v * b2 + c2 * (g * g)
        denom = v1.sqrt() / bc2 + e
        p1 = p + (-ss) * (m1 / denom)
        mag = m.abs() + inc.abs()
        dm = (mk.cpu().double() - m1).abs()
        dv = (vk.cpu().double() - v1).abs()
        dp = (pk.cpu().double() - p1).abs()
        assert bool((dm <= 1.001 * 3 * u * mag).all()), (k, float((dm / mag).max() / u))
        assert bool((dv <= 1.001 * 3 * u * v1 + 2.0 ** -125).all()), (k, float((dv / v1).max() / u))
        lim = 1.001 * 10.5 * u * (p.abs() + ss * mag / denom)
        assert bool((dp <= lim).all()), (k, float((dp / lim).max()))
        assert float((pk.cpu().double() - p).abs().max()) > 0, k  # it was a real step
    assert tc.wt_matches_params()
    with torch.no_grad():
        tc.param[4][3, 5] += 1.0  # a weight written from torch (dynamics layer 1)
        tc.param[18][32, 255] -= 2.0  # ... and the last element of the value head
    torch.cuda.synchronize()
    assert not tc.wt_matches_params()
    assert tc.transpose() == tc.L.MZH_OK
    assert tc.wt_matches_params()
