"""Shared by tests/test_widths_cpu.py and tests/test_widths_gpu.py: the observation widths the engine accepts
beyond those the other GPU tests run (n_disks 3, 4 and 7), their seeded networks and input rows, and the canaried
device buffers every observation of a GPU test goes in through.

    n_disks  support  in_dim  kin  k-blocks of rep0   what the width is for
    1        33       3       16   1                  the narrowest: 13 padding columns
    2        1        6       16   1                  scalar heads on one block
    5        33       15      16   1                  one column short of a block
    6        1        18      32   2                  two columns into the second block
    11       33       33      48   3                  one column into the third block
    16       33       48      48   3                  the widest: no padding at all
    16       1        48      48   3                  ... with scalar heads
"""
import functools

import numpy as np
import torch

import train_ref as tr

WIDTHS = [(1, 33), (2, 1), (5, 33), (6, 1), (11, 33), (16, 33), (16, 1)]  # (n_disks, support)
IDS = [f"n{n}_s{s}" for n, s in WIDTHS]
NROWS = 37  # 32 state rows + 5 float rows: two 16-row tiles and a ragged third
BOUNDARY_COLUMNS = (0, 15, 16, 31, 32)  # and in_dim - 1: the first and last column of every 16-column k-block


@functools.lru_cache(maxsize=None)
def net(n, support, seed=0):
    """this repository's MuZeroNet for n discs, seeded"""
    return tr.make_net(n, support, seed).eval()


def flat(network):
    """the canonical fp32 vector of the oracle and of Engine.load_weights"""
    from muzero_hanoi_amd import engine

    return engine.flat_weights(network.state_dict())


def rows(n, seed, states, floats):
    """[states + floats][3n] float32: `states` one-hot rows with a peg drawn per disc, then `floats` rows of
    arbitrary floats in [-1, 2) -- a non-zero value in every column, so a dropped or doubled column changes bits"""
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 3, (states, n))
    obs = np.zeros((states, 3 * n), np.float32)
    obs[np.arange(states)[:, None], np.arange(n) * 3 + st] = 1
    fl = rs.uniform(-1.0, 2.0, size=(floats, 3 * n)).astype(np.float32)
    return np.concatenate([obs, fl])


def boundary_columns(in_dim):
    return sorted({k for k in BOUNDARY_COLUMNS + (in_dim - 1,) if 0 <= k < in_dim})


def zero_column(flat_weights, in_dim, k):
    """a copy of the canonical vector with representation_net.0.weight[:, k] zeroed (the vector starts with that
    [256][in_dim] tensor)"""
    out = np.array(flat_weights, np.float32, copy=True)
    out[:256 * in_dim].reshape(256, in_dim)[:, k] = 0
    return out


def canaried(x, device="cuda"):
    """(the whole allocation as int32, a device copy of x that is a contiguous view inside it): PAD words of
    train_ref.CANARY -- an fp32 NaN -- on either side, so a read past a row's end poisons the result"""
    x = torch.as_tensor(np.asarray(x))
    assert x.element_size() in (4, 8)
    words = x.numel() * x.element_size() // 4
    big, view = tr._canaried(words, device)
    view = view.view(x.dtype).view(x.shape)
    view.copy_(x)
    return big, view


def canaried_like(t):
    """(the whole allocation, a view of t's shape and dtype inside it) holding the canary's bytes everywhere"""
    words = t.numel() * t.element_size() // 4
    assert words * 4 == t.numel() * t.element_size()
    big, view = tr._canaried(words, t.device)
    return big, view.view(t.dtype).view(t.shape)


intact = tr._intact


def search_case(n, B=40):
    """the search case of every width: 37 state roots and 3 float roots (these never use the memo), Dirichlet
    noise, tie and action draws seeded by n"""
    from muzero_hanoi_amd import rng

    obs = rows(n, 5, B - 3, 3)
    noise, tie, u = rng.synthetic_draws(B, deterministic=False, alpha=0.25, seed=n)
    return obs, noise, tie, u


def pgrad_pool(n):
    """the candidate pool of a width's parameter-gradient case: 512 state rows, then 64 float rows"""
    return rows(n, 7000 * n, 512, 64)


@functools.lru_cache(maxsize=None)
def saliency_reference(n, support):
    """saliency_ref.Reference of the width's 37 rows (float64, the fp32-torch baseline, the bound, the bad rows)"""
    import saliency_ref as sr

    return sr.Reference(net(n, support), rows(n, 1000 * n, 32, 5))


@functools.lru_cache(maxsize=None)
def pgrad_reference(n, support):
    """pgrad_ref.Reference of the width's 37 rows, chosen by pgrad_ref.case_rows' rule from pgrad_pool(n); .rejected
    counts the candidates passed over on the way"""
    import pgrad_ref as pr

    network, pool = net(n, support), pgrad_pool(n)
    obs, action, pl, rejected = pr.case_rows(network, n, pool=512, obs_pool=pool)
    ref = pr.Reference(network, obs, action, pl)
    ref.rejected = rejected
    return ref


# ------------------------------------------------------------------------------------ float64 inference
BAR_LOGIT = 1e-5   # latents and every logit against float64, absolute (tests/test_gpu_parity.py, "north_star")
BAR_SCALAR = 2e-3  # transformed value and reward
BARS = dict(h=BAR_LOGIT, policy_logits=BAR_LOGIT, value_logits=BAR_LOGIT, reward_logits=BAR_LOGIT, value=BAR_SCALAR,
            reward=BAR_SCALAR)


def _heads64(net64, h, out):
    logits, vl = net64.policy_net(h), net64.value_net(h)
    out.update(h=h, policy_logits=logits, value_logits=vl,
               value=(net64.logits_to_transformed_expected_value(vl) if net64.TD_return else vl)[:, 0])
    return {k: v.detach().numpy() for k, v in out.items()}


def initial64(network, x):
    """initial_inference by the torch path in float64 on the CPU"""
    import copy

    net64 = copy.deepcopy(network).double()
    with torch.no_grad():
        return _heads64(net64, net64.represent(torch.as_tensor(np.asarray(x), dtype=torch.float64)), {})


def recurrent64(network, h_in, action):
    """recurrent_inference by the torch path in float64 on the CPU"""
    import copy

    net64 = copy.deepcopy(network).double()
    with torch.no_grad():
        a = torch.zeros(len(action), 6, dtype=torch.float64)
        a[torch.arange(len(action)), torch.as_tensor(np.asarray(action), dtype=torch.int64)] = 1
        z = net64.dynamic_net(torch.cat([torch.as_tensor(np.asarray(h_in), dtype=torch.float64), a], dim=1))
        rl = net64.rwd_net(z)
        out = dict(reward_logits=rl,
                   reward=(net64.logits_to_transformed_expected_value(rl) if net64.TD_return else rl)[:, 0])
        return _heads64(net64, net64.normalize_h_state(z), out)


def float64_errors(got, want):
    """{key: max |got - want|} over the keys of BARS that both hold"""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(want[k].shape) - want[k]).max())
            for k in BARS if k in got and k in want}


def recurrent_case(n):
    """the 37 latents in [0, 1) and actions of the width's recurrent call"""
    rs = np.random.RandomState(200 + n)
    return rs.uniform(0, 1, (NROWS, 64)).astype(np.float32), rs.randint(0, 6, NROWS).astype(np.int32)
