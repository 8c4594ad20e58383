"""Shared by tests/test_pgrad_cpu.py and tests/test_pgrad_gpu.py: the float64 reference of the five sub-networks'
parameter gradients (this repository's MuZeroNet torch path on the CPU, gradient_analysis.py get_results'
objectives), the fp32 torch baseline, the cases, the conditioning rules and the bound.

Outputs are the rank-one factors per row and net (representation, dynamic, reward, policy, value): delta2 =
d objective / d Linear2 output, act = relu(Linear0(in)), delta1 = d objective / d Linear0 output; the dense
gradients are delta1 (x) in and delta2 (x) act (dense_from_factors; test_pgrad_cpu checks that against
autograd.grad on the parameters themselves).

The rule is tests/saliency_ref.py's: per case and tensor kind (delta1 / delta2 / act / objective of each net, and
each of the 20 dense tensors) e = max|x - x64| / max|x64| over the case's tensor, and the bound is
max(4 x the fp32 torch path's e on that tensor, FLOOR), FLOOR the largest fp32-torch e over all cases.  The five
objective scalars have a floor of their own, FLOOR_OBJECTIVE, the largest fp32-torch e of a scalar: torch's fp32
signed parabolic transform cancels (sqrt(.) / 2 / eps - 1 / 2 / eps) and is off by up to 1.8e-3 on the reward and
value scalars themselves, thirty times its error on their gradients, and one shared floor would loosen every
factor's bound to that.  FLOOR covers delta1 / delta2 / act and the dense tensors.
Measured on the CPU (torch fp32 against fp64, the cases below; test_pgrad_cpu.test_conditioning_report prints all):

    case               rows  fp32-torch e delta1 rep / dyn / rwd / pol / val, objective rwd / val   smallest latent gap
    weights_N3_s0      37    3.45e-07 / 4.52e-07 / 4.22e-05 / 0 / 4.91e-05   objective 3.35e-04 / 3.63e-04   5.41e-04
    weights_N4_s0      37    4.11e-07 / 6.23e-07 / 5.44e-05 / 0 / 6.41e-05   objective 6.82e-04 / 9.84e-04   3.44e-04
    weights_N7_s0      37    5.41e-07 / 4.23e-07 / 5.60e-05 / 0 / 3.71e-05   objective 3.67e-04 / 1.17e-04   1.59e-04
    weights_N3_s0_mc   37    3.45e-07 / 4.52e-07 / 0 / 0 / 0                 objective 5.02e-07 / 3.89e-07   5.41e-04
    fixture, base      162   3.02e-07 / 4.86e-07 / 6.11e-05 / 0 / 2.86e-05   objective 1.82e-03 / 6.45e-05   2.69e-04
    fixture, policy-   162   3.02e-07 / 4.86e-07 / 6.11e-05 / 0 / 2.86e-05   objective 1.82e-03 / 6.45e-05   2.69e-04
    fixture, value-    162   3.02e-07 / 4.86e-07 / 6.11e-05 / 0 / 4.08e-05   objective 1.82e-03 / 1.60e-04   2.69e-04

With support 33 the reward and value nets' fp32 torch path is dominated by the cancellation in the signed
parabolic transform, as in saliency; support 1 has none.  The policy net's deltas (rows with a forced logit: a
one-hot seed and a row of W2, no arithmetic) are exact in fp32.  The largest delta2 error is 6.48e-05
(weights_N4_s0, value), the closest hidden unit to the kink in a weight case 1.02e-05; the atlas holds such a unit
in 6 / 12 / 6 rows (base / policy- / value-ablated; the closest 1.98e-06).  The baseline moves a little with the host's torch build.

Rows whose policy objective is the reference's softmax(lp).mean() have a true policy gradient of 0 (the objective
is constant), so the policy net's delta1 / delta2 of those rows are held to absolute bounds instead:
|delta2| <= 2^-21 (p_i |g - sum_j p_j g| with a handful of ulps of 1/6) and |delta1[k]| <= 2^-21 sum_n |W2[n][k]|.

A row is ill-conditioned when, in float64, the two smallest or the two largest elements of z0 or of z1 are within
GAP, its top two policy logits are within GAP where policy_logit is not forced, or the fp32 torch path is off by
more than BAD_INPUT on it.  A hidden unit whose float64 pre-activation lies within NEAR0 of zero may get either
ReLU mask in fp32: for such a unit delta1 and act must match the masked value (0) or the unmasked float64 value,
each within the bound.  The weight cases' rows are the first candidates of a seeded stream that are neither
ill-conditioned nor hold such a unit; the checkpoint atlas may hold such a unit in at most NEAR0_ROWS_CAP rows
per network.
"""
import copy
import functools

import numpy as np
import torch

from saliency_ref import WEIGHTS, all_states, fixture_nets, npz_net, state_obs  # noqa: F401

FLOOR = 6.48e-5  # the largest fp32-torch error of any case, net and factor, measured (weights_N4_s0, value delta2)
FLOOR_OBJECTIVE = 1.82e-3  # and of any objective scalar (the fixture's networks, reward)
GAP = 1e-4
BAD_INPUT = 1e-2
NEAR0 = 1e-5
NEAR0_ROWS_CAP = 16
ABS_POLICY = 2.0 ** -21
NETS = ("representation", "dynamic", "reward", "policy", "value")
MODULES = ("representation_net", "dynamic_net", "rwd_net", "policy_net", "value_net")
KINDS = ("delta1", "delta2", "act", "objective")
NROWS = 37


def torch_factors(net, obs, action, policy_logit, dtype):
    """the factors of every row by autograd on the torch path in `dtype`; policy_logit [n]: -1 the reference's
    objective, k the logit k.  Returns numpy arrays: delta1 / act / pre / d1_open [n][5][256] (pre: Linear0's output
    before the ReLU; d1_open: delta2 . W2 without the mask), delta2 [n][5][64] (zero beyond the net's outputs),
    objective [n][5], ins (the five first-layer inputs), h0, z0, z1, h1, pi0, value0, reward, lp."""
    net = copy.deepcopy(net).to(dtype)
    n = len(obs)
    x = torch.as_tensor(np.asarray(obs), dtype=dtype)
    a = torch.zeros(n, 6, dtype=dtype)
    a[torch.arange(n), torch.as_tensor(np.asarray(action), dtype=torch.int64)] = 1.0
    pl = torch.as_tensor(np.asarray(policy_logit), dtype=torch.int64)
    out = {k: np.zeros((n, 5, 256), np.dtype(str(dtype).split(".")[1])) for k in ("delta1", "act", "pre", "d1_open")}
    out["delta2"] = np.zeros((n, 5, 64), out["act"].dtype)
    out["objective"] = np.zeros((n, 5), out["act"].dtype)
    ins = []

    def run(i, inp, objective):
        seq = getattr(net, MODULES[i])
        inp = inp.detach()
        pre = seq[0](inp)
        act = torch.relu(pre)
        o2 = seq[2](act)
        obj, extra = objective(o2)
        d1, d2 = torch.autograd.grad(obj.sum(), [pre, o2])
        out["delta1"][:, i], out["act"][:, i], out["pre"][:, i] = d1.numpy(), act.detach().numpy(), pre.detach().numpy()
        out["delta2"][:, i, :d2.shape[1]] = d2.numpy()
        out["d1_open"][:, i] = (d2 @ seq[2].weight.detach()).numpy()
        out["objective"][:, i] = obj.detach().numpy()
        ins.append(inp.numpy())
        return o2.detach(), extra

    def norm_mean(z):
        h = net.normalize_h_state(z)
        return h.mean(dim=1), h.detach()

    def scalar(l):
        v = net.logits_to_transformed_expected_value(l) if net.TD_return else l
        return v[:, 0], v[:, 0].detach()

    def policy(lp):
        ref = torch.softmax(lp, dim=-1).mean(dim=1)
        forced = lp.gather(1, pl.clamp(min=0)[:, None])[:, 0]
        return torch.where(pl >= 0, forced, ref), torch.softmax(lp, dim=-1).detach()

    z0, h0 = run(0, x, norm_mean)
    z1, h1 = run(1, torch.cat([h0, a], dim=1), norm_mean)
    _, reward = run(2, z1, scalar)
    lp, pi0 = run(3, h0, policy)
    _, value0 = run(4, h0, scalar)
    out.update(ins=ins, h0=h0.numpy(), z0=z0.numpy(), z1=z1.numpy(), h1=h1.numpy(), pi0=pi0.numpy(),
               value0=value0.numpy(), reward=reward.numpy(), lp=lp.numpy())
    return out


def dense_from_factors(delta1, delta2, act, ins, support):
    """[n][n_floats] in the flat layout of load_weights (weight then bias of Linear0 and Linear2 of the five nets):
    every weight element the single product delta[i] * in[j] in the arrays' dtype, every bias a copy"""
    n = delta1.shape[0]
    outs = (64, 64, support, 6, support)
    parts = []
    for i in range(5):
        d2 = delta2[:, i, :outs[i]]
        parts += [(delta1[:, i, :, None] * ins[i][:, None, :]).reshape(n, -1), delta1[:, i],
                  (d2[:, :, None] * act[:, i][:, None, :]).reshape(n, -1), d2]
    return np.concatenate(parts, axis=1)


def dense_slices(in_dim, support):
    """[(state_dict key, lo, hi)] of the 20 tensors in the flat vector"""
    ins = (in_dim, 70, 64, 64, 64)
    outs = (64, 64, support, 6, support)
    sl, lo = [], 0
    for i, m in enumerate(MODULES):
        for key, size in ((f"{m}.0.weight", 256 * ins[i]), (f"{m}.0.bias", 256), (f"{m}.2.weight", outs[i] * 256),
                          (f"{m}.2.bias", outs[i])):
            sl.append((key, lo, lo + size))
            lo += size
    return sl


def _gap2(z):
    s = np.sort(z, axis=1)
    return np.minimum(s[:, 1] - s[:, 0], s[:, -1] - s[:, -2])


def rel(x, x64):
    d = np.abs(x64).max()
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / d) if d > 0 else float(np.abs(x).max())


class Reference:
    """the float64 factors of a case, the fp32 torch baseline's error against them, the bounds, the bad rows and
    the rows with a hidden unit within NEAR0 of the ReLU's kink"""

    def __init__(self, net, obs, action, policy_logit):
        self.obs = np.asarray(obs, np.float32)
        self.action = np.asarray(action, np.int32)
        self.policy_logit = np.asarray(policy_logit, np.int32)
        self.support = net.support_size if net.TD_return else 1
        self.r64 = torch_factors(net, self.obs, self.action, self.policy_logit, torch.float64)
        self.r32 = torch_factors(net, self.obs, self.action, self.policy_logit, torch.float32)
        self.w2abs = [np.abs(getattr(net, m)[2].weight.detach().numpy().astype(np.float64)).sum(axis=0) for m in MODULES]
        self.forced = self.policy_logit >= 0
        self.near0 = np.abs(self.r64["pre"]) < NEAR0  # [n][5][256]
        self.near0_rows = np.nonzero(self.near0.any(axis=(1, 2)))[0]
        self.base, self.bound = {}, {}
        row32 = np.zeros(len(self.obs))
        for kind in KINDS:
            for i in range(5):
                e, rows = self._err(kind, i, self.r32[kind], per_row=True)
                self.base[kind, i] = e
                self.bound[kind, i] = max(4 * e, FLOOR_OBJECTIVE if kind == "objective" else FLOOR)
                row32 = np.maximum(row32, rows)
        g = self.r64
        top = np.sort(g["lp"], axis=1)
        self.gaps = dict(z0=_gap2(g["z0"]), z1=_gap2(g["z1"]), logit=top[:, -1] - top[:, -2])
        self.bad = np.nonzero((self.gaps["z0"] < GAP) | (self.gaps["z1"] < GAP) | ((self.gaps["logit"] < GAP) & ~self.forced)
                              | (row32 > BAD_INPUT))[0]
        self.compared = 0

    def _rows(self, kind, i):
        """the rows a relative comparison covers: all, but for the policy net's deltas only the forced rows"""
        if i == 3 and kind in ("delta1", "delta2"):
            return np.nonzero(self.forced)[0]
        return np.arange(len(self.obs))

    def _err(self, kind, i, x, per_row=False):
        rows = self._rows(kind, i)
        x64 = self.r64[kind][:, i].astype(np.float64)
        x = np.asarray(x)[:, i].astype(np.float64)
        d = np.abs(x - x64)
        if kind in ("delta1", "act"):  # a unit at the kink: the masked value or the unmasked float64 one
            open64 = (self.r64["d1_open"] if kind == "delta1" else self.r64["pre"])[:, i].astype(np.float64)
            either = np.minimum(np.abs(x), np.abs(x - open64))
            d = np.where(self.near0[:, i], np.minimum(d, either), d)
        d = d.reshape(len(x), -1)
        scale = np.abs(x64[rows]).max() if len(rows) else 1.0
        per = np.zeros(len(x))
        per[rows] = d[rows].max(axis=1) / scale
        self.compared = len(rows)
        return (float(per.max()), per) if per_row else float(per.max())

    def errors(self, got):
        """{(kind, net): e} of the arrays got[kind]"""
        return {(kind, i): self._err(kind, i, got[kind]) for kind in KINDS for i in range(5)}

    def policy_abs(self, got):
        """the largest |delta2| and the largest |delta1[k]| / sum_n |W2[n][k]| of the policy net over the rows with
        the reference's objective (true value 0), both to be <= ABS_POLICY; and how many rows that is"""
        rows = np.nonzero(~self.forced)[0]
        if not len(rows):
            return 0.0, 0.0, 0
        d2 = float(np.abs(got["delta2"][rows, 3]).max())
        d1 = float((np.abs(got["delta1"][rows, 3].astype(np.float64)) / self.w2abs[3][None, :]).max())
        return d2, d1, len(rows)

    def dense64(self):
        g = self.r64
        return dense_from_factors(g["delta1"], g["delta2"], g["act"], g["ins"], self.support)

    def dense_errors(self, grad, grad32=None):
        """{key: (e, bound)} of a dense [n][n_floats] array per state_dict tensor, the bound from the fp32 torch
        path's dense gradients; the policy net's tensors over the forced rows only"""
        g32 = self.r32
        d64 = self.dense64()
        d32 = dense_from_factors(g32["delta1"], g32["delta2"], g32["act"], g32["ins"], self.support) if grad32 is None else grad32
        res = {}
        for key, lo, hi in dense_slices(self.obs.shape[1], self.support):
            rows = np.nonzero(self.forced)[0] if key.startswith("policy_net") else np.arange(len(self.obs))
            ref = d64[rows, lo:hi]
            res[key] = (rel(grad[rows, lo:hi], ref), max(4 * rel(d32[rows, lo:hi], ref), FLOOR))
        return res

    def report(self, title, errs=None):
        b = self.base
        line = (f"{title}: rows {len(self.obs)} fp32-torch e delta1 " + " / ".join(f"{b['delta1', i]:.2e}" for i in range(5))
                + " delta2 " + " / ".join(f"{b['delta2', i]:.2e}" for i in range(5))
                + " act " + " / ".join(f"{b['act', i]:.2e}" for i in range(5))
                + " objective " + " / ".join(f"{b['objective', i]:.2e}" for i in range(5))
                + f"; min gaps z0 {self.gaps['z0'].min():.2e} z1 {self.gaps['z1'].min():.2e}"
                + f" logit (unforced) {self.gaps['logit'][~self.forced].min() if (~self.forced).any() else float('nan'):.2e}"
                + f"; bad rows {self.bad.tolist()}; rows with a unit within {NEAR0:g} of the kink {self.near0_rows.tolist()}"
                + f" (closest {np.abs(self.r64['pre']).min():.2e}); forced rows {int(self.forced.sum())}")
        if errs is not None:
            line += "; compared e " + " ".join(f"{k}{i}={errs[k, i]:.2e}" for k in KINDS for i in range(5))
        print("\n" + line)


def case_rows(net, n, seed=0, pool=512, obs_pool=None):
    """the case's 37 rows: the first 32 well-conditioned state rows and the first 5 well-conditioned arbitrary-float
    rows of a seeded stream that draws observation, action and policy_logit per candidate; well-conditioned: not
    in Reference.bad and without a hidden unit within NEAR0 of the kink.  Returns obs, action, policy_logit and
    how many candidates were rejected.  obs_pool: the candidates' observations, `pool` state rows and then the float
    rows, where the caller draws them itself (all_states enumerates 3^n states: not beyond a dozen discs); the
    stream then draws action and policy_logit only."""
    rs = np.random.RandomState(7000 * n + seed)
    if obs_pool is None:
        st = state_obs(all_states(n)[rs.randint(0, 3 ** n, size=pool)])
        fl = rs.uniform(-1.0, 2.0, size=(pool // 8, 3 * n)).astype(np.float32)
        obs = np.concatenate([st, fl])
    else:
        obs = np.asarray(obs_pool, np.float32)
        assert obs.shape[1] == 3 * n and len(obs) > pool
    action = rs.randint(0, 6, size=len(obs)).astype(np.int32)
    pl = np.maximum(rs.randint(-3, 6, size=len(obs)), -1).astype(np.int32)
    ref = Reference(net, obs, action, pl)
    ok = np.ones(len(obs), bool)
    ok[ref.bad] = False
    ok[ref.near0_rows] = False
    a = np.nonzero(ok[:pool])[0][:32]
    b = pool + np.nonzero(ok[pool:])[0][:5]
    assert len(a) == 32 and len(b) == 5, "the candidate pool is too small"
    rows = np.concatenate([a, b])
    rejected = int((~ok[:a[-1] + 1]).sum() + (~ok[pool:b[-1] + 1]).sum())
    return obs[rows], action[rows], pl[rows], rejected


@functools.lru_cache(maxsize=None)
def weights_reference(name):
    net = npz_net(name)
    obs, action, pl, rejected = case_rows(net, net.representation_net[0].in_features // 3)
    ref = Reference(net, obs, action, pl)
    ref.rejected = rejected
    return ref


def atlas_rows():
    """the N = 3 atlas: 27 states x 6 actions, state-major, the reference's policy objective"""
    obs = np.repeat(state_obs(all_states(3)), 6, axis=0)
    return obs, np.tile(np.arange(6, dtype=np.int32), 27), np.full(162, -1, np.int32)


@functools.lru_cache(maxsize=None)
def fixture_reference():
    """per fixture network the Reference on the 162 (state, action) pairs"""
    return tuple(Reference(net, *atlas_rows()) for net in fixture_nets())
