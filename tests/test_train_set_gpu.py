"""One update round of a network set in four launches (mzh_train_set_update) against the lone calls.

Every case builds M networks twice from the same bytes: parameters, random Adam moments, a replay ring filled from
train_ref.make_batch with priorities of tests/test_replay.py's kinds, and every output and workspace (the sampled
batch, indx, cdf, scratch, row_loss, new_prio) inside a canary-filled allocation.  One copy runs the set call; the
other runs mzh_replay_sample + mzh_train_update + mzh_replay_set_priorities network by network with the same
uniforms and Adam scalars, and skips an inactive network altogether.  Then the WHOLE allocations are compared bit
for bit, canaries and unwritten rows included -- parameters, both moments, wt, scratch, row_loss, new_prio, indx,
the five sampled arrays, cdf, the whole prio array -- and the status rows.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_replay import _prios
from train_ref import CANARY, PAD, make_batch, make_net

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATUS_CANARY = -7
STEP = np.dtype([("active", np.int32), ("n", np.int32), ("step_size", np.float32), ("bc2_sqrt", np.float32)])
BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-8, 0.002


def canaried(shape, dtype):
    """(the whole allocation as int32, its payload viewed as dtype and shape): CANARY everywhere"""
    n32 = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() // 4
    big = torch.full((PAD + n32 + PAD,), CANARY, dtype=torch.int32, device=DEV)
    return big, big[PAD:PAD + n32].view(dtype).view(shape)


def pinned(shape, dtype, fill=0):
    from muzero_hanoi_amd import _lib

    t = torch.full(shape, fill, dtype=dtype).pin_memory()
    return t, _lib.host_device_pointer(t.data_ptr())


class Network:
    """one network of a case on the device: its tensors and the two argument blocks over them"""

    def __init__(self, spec, case, m):
        from muzero_hanoi_amd import _lib

        self.L = _lib
        B, U, rows = case["B"], case["U"], case["rows"]
        self.B, self.size = B, spec["prio"].shape[0]
        self.whole = {}  # name -> allocations compared as wholes
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.param = [to(p) for p in spec["param"]]
        self.exp_avg = [to(p) for p in spec["exp_avg"]]
        self.exp_avg_sq = [to(p) for p in spec["exp_avg_sq"]]
        self.wt = [torch.full((p.shape[1], (p.shape[0] + 3) // 4 * 4), float("nan"), dtype=torch.float32, device=DEV)
                   for p in self.param[0::2]]
        self.ring = [to(x) for x in spec["ring"]]  # states, rwds, actions, pi, returns
        self.prio = to(spec["prio"])
        self.w = to(spec["w"])
        in_dim, support = self.param[0].shape[1], self.param[18].shape[0]
        nb = ctypes.c_size_t()
        assert _lib.lib().mzh_train_scratch_bytes(B, U, in_dim, support, nb) == _lib.MZH_OK
        outs = {"out_states": ((B, in_dim), torch.float32), "out_rwds": ((B, U), torch.float32),
                "out_actions": ((B, U), torch.int64), "out_pi": ((B, U, 6), torch.float32),
                "out_returns": ((B, U), torch.float32), "indx": ((B,), torch.int64),
                "cdf": ((self.size,), torch.float64), "scratch": ((nb.value // 4,), torch.float32),
                "row_loss": ((B, 3), torch.float32), "new_prio": ((B,), torch.float32)}
        v = {}
        for k, (shape, dt) in outs.items():
            self.whole[k], v[k] = canaried(shape, dt)
        self.view = v
        for k in ("param", "exp_avg", "exp_avg_sq", "wt"):
            self.whole[k] = getattr(self, k)
        self.whole["prio"] = self.prio
        t = _lib.TrainArgs()
        t.B, t.U, t.in_dim, t.support, t.rows = B, U, in_dim, support, rows
        t.beta1, t.beta2, t.eps = BETA1, BETA2, EPS
        for i in range(20):
            t.param[i], t.exp_avg[i] = self.param[i].data_ptr(), self.exp_avg[i].data_ptr()
            t.exp_avg_sq[i] = self.exp_avg_sq[i].data_ptr()
        for i, x in enumerate(self.wt):
            t.wt[i] = x.data_ptr()
        t.obs, t.rwds, t.actions, t.pi, t.returns = (v[k].data_ptr() for k in ("out_states", "out_rwds", "out_actions",
                                                                               "out_pi", "out_returns"))
        t.weights, t.scratch, t.scratch_bytes = self.w.data_ptr(), v["scratch"].data_ptr(), nb.value
        t.row_loss, t.new_prio = v["row_loss"].data_ptr(), v["new_prio"].data_ptr()
        self.train = t
        d = _lib.ReplayArgs()
        d.n, d.m, d.d_state, d.U, d.A = self.size, B, in_dim, U, 6
        d.prio, d.cdf = self.prio.data_ptr(), v["cdf"].data_ptr()
        d.states, d.rwds, d.actions, d.pi, d.returns = (x.data_ptr() for x in self.ring)
        d.indx = v["indx"].data_ptr()
        d.out_states, d.out_rwds, d.out_actions, d.out_pi, d.out_returns = t.obs, t.rwds, t.actions, t.pi, t.returns
        self.draw = d
        stream = torch.cuda.current_stream().cuda_stream
        assert _lib.lib().mzh_train_transpose(ctypes.byref(t), stream) == _lib.MZH_OK, _lib.last_error()
        torch.cuda.synchronize()

    def lone_round(self, n, u_dev, step_size, bc2_sqrt, status, status_dev):
        """the three lone calls; status: this network's pinned row [4] at device address status_dev"""
        L, stream = self.L, torch.cuda.current_stream().cuda_stream
        d, t = self.draw, self.train
        d.n, d.u, d.status = n, u_dev, status_dev
        L.check(L.lib().mzh_replay_sample(ctypes.byref(d), stream), "mzh_replay_sample")
        t.step_size, t.bc2_sqrt = step_size, bc2_sqrt
        L.check(L.lib().mzh_train_update(ctypes.byref(t), stream), "mzh_train_update")
        L.check(L.lib().mzh_replay_set_priorities(self.prio.data_ptr(), self.size, d.indx, t.new_prio, self.B,
                                                  status_dev + 8, stream), "mzh_replay_set_priorities")
        torch.cuda.synchronize()
        status[3] = 0
        d.n = self.size  # what the set's creation reads here: the ring's size


def specs(case):
    """the bytes of the case's M networks, built once for both copies"""
    g = np.random.default_rng(case["seed"])
    out = []
    for m, fill in enumerate(case["fills"]):
        net = make_net(case["n_disks"], case["support"], 100 * case["seed"] + m)
        param = [p.detach().numpy().copy() for p in net.parameters()]
        size = fill + 5  # rows behind the filled part: their priorities are compared too
        obs, rwds, actions, pi, returns, w = (x.numpy() for x in make_batch(case["n_disks"], max(size, 6), case["U"],
                                                                            case["seed"] + m))
        ring = [x[:size].copy() for x in (obs, rwds, actions, pi, returns)]
        prio = _prios(g, size, case["kinds"][m])
        if case.get("nan_prio") == m:
            prio[min(3, fill - 1)] = np.nan
        if case.get("zero_prio") == m:  # the value head answers 0.5 whatever it sees, and every return_0 is 0.5
            param[18][...] = 0
            param[19][...] = 0.5
            ring[4][:, 0] = 0.5
        out.append(dict(param=param, exp_avg=[(0.01 * g.standard_normal(p.shape)).astype(np.float32) for p in param],
                        exp_avg_sq=[(1e-4 * g.random(p.shape)).astype(np.float32) for p in param],
                        ring=ring, prio=prio, w=w[:case["B"]].copy()))
    return out


def run_case(case):
    """both copies through case['rounds'] rounds; returns (set copy, lone copy, set status, lone status, handle-free)"""
    from muzero_hanoi_amd import _lib

    L = _lib.lib()
    M, B, R = len(case["fills"]), case["B"], case["rounds"]
    active = case.get("active", [1] * M)
    sp = specs(case)
    sets, lones = [Network(s, case, m) for m, s in enumerate(sp)], [Network(s, case, m) for m, s in enumerate(sp)]
    g = np.random.default_rng(case["seed"] + 1)
    u, u_dev = pinned((R, M, B), torch.float64)
    u.numpy()[...] = g.random((R, M, B))
    step, step_dev = pinned((R, M, 4), torch.int32)
    assert step_dev == step.data_ptr()
    rec = step.numpy().view(STEP).reshape(R, M)
    for r in range(R):
        for m in range(M):
            k = 1 + 3 * m + r  # every network at another Adam step
            rec[r, m] = (active[m], case["fills"][m], LR / (1 - BETA1 ** k), math.sqrt(1 - BETA2 ** k))
    st_set, st_set_dev = pinned((R, M, 4), torch.int32, STATUS_CANARY)
    st_lone, st_lone_dev = pinned((R, M, 4), torch.int32, STATUS_CANARY)
    train, draw = (_lib.TrainArgs * M)(), (_lib.ReplayArgs * M)()
    for m in range(M):
        train[m], draw[m] = sets[m].train, sets[m].draw
    h = ctypes.c_void_p()
    _lib.check(L.mzh_train_set_create(train, draw, M, ctypes.byref(h)), "mzh_train_set_create")
    try:
        stream = torch.cuda.current_stream().cuda_stream
        for r in range(R):
            _lib.check(L.mzh_train_set_update(h, step_dev + r * M * 16, u_dev + r * M * B * 8,
                                              st_set_dev + r * M * 16, stream), "mzh_train_set_update")
        torch.cuda.synchronize()
    finally:
        L.mzh_train_set_destroy(h)
    for r in range(R):
        for m in range(M):
            if active[m]:
                lones[m].lone_round(case["fills"][m], u_dev + (r * M + m) * B * 8, float(rec[r, m]["step_size"]),
                                    float(rec[r, m]["bc2_sqrt"]), st_lone.numpy()[r, m],
                                    st_lone_dev + (r * M + m) * 16)
    return sets, lones, st_set.numpy().copy(), st_lone.numpy().copy(), sp


def raw(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous().view(torch.int64)


def assert_same(sets, lones, st_set, st_lone):
    for m, (a, b) in enumerate(zip(sets, lones)):
        for k in a.whole:
            xs, ys = a.whole[k], b.whole[k]
            for i, (x, y) in enumerate(zip(xs, ys) if isinstance(xs, list) else [(xs, ys)]):
                assert torch.equal(raw(x), raw(y)), (m, k, i)
    assert np.array_equal(st_set, st_lone), (st_set, st_lone)


def untouched(net, spec):
    """every tensor of the network as created (wt: as mzh_train_transpose left it, which the copies share)"""
    for k in ("out_states", "out_rwds", "out_actions", "out_pi", "out_returns", "indx", "cdf", "scratch", "row_loss",
              "new_prio"):
        if not bool((net.whole[k] == CANARY).all()):
            return False
    same = lambda ts, arrs: all(np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
                                for t, a in zip(ts, arrs))
    return same(net.param, spec["param"]) and same(net.exp_avg, spec["exp_avg"]) \
        and same(net.exp_avg_sq, spec["exp_avg_sq"]) and same([net.prio], [spec["prio"]])


def case(**kw):
    base = dict(n_disks=3, support=33, B=5, U=5, rows=1, fills=(1, 37, 515), kinds=("uniform",) * 3, rounds=1, seed=7)
    base.update(kw)
    return base


MAIN = case(rounds=2, kinds=("uniform", "heavy", "zeros"))


def test_main_case_two_rounds():
    """three networks at rings of 1, 37 and 515 rows, each at its own Adam step, two rounds in a row: round 2 draws
    from the priorities round 1 wrote"""
    sets, lones, st_set, st_lone, sp = run_case(MAIN)
    assert_same(sets, lones, st_set, st_lone)
    assert (st_set[:, :, 0] == 0).all() and (st_set[:, :, 1] == 1).all() and (st_set[:, :, 2:] == 0).all(), st_set
    for m, net in enumerate(sets):  # the case is a real step: the rounds moved parameters and priorities
        assert not untouched(net, sp[m]), m
        assert not np.array_equal(net.prio.cpu().numpy()[:MAIN["fills"][m]], sp[m]["prio"][:MAIN["fills"][m]]), m


def test_an_inactive_network_is_left_alone():
    c = case(active=[1, 0, 1], kinds=("uniform", "heavy", "zeros"))
    sets, lones, st_set, st_lone, sp = run_case(c)
    assert_same(sets, lones, st_set, st_lone)
    assert untouched(sets[1], sp[1]) and (st_set[:, 1] == STATUS_CANARY).all(), st_set
    assert not untouched(sets[0], sp[0]) and not untouched(sets[2], sp[2])


def test_all_inactive_writes_nothing():
    c = case(active=[0, 0, 0])
    sets, lones, st_set, st_lone, sp = run_case(c)
    assert all(untouched(n, s) for n, s in zip(sets, sp))
    assert (st_set == STATUS_CANARY).all()


VARIANTS = {
    "rows 2 with a tail workgroup": case(rows=2),
    "support 1, in_dim 12": case(n_disks=4, support=1, fills=(37, 515), kinds=("uniform", "heavy")),
    "in_dim 21": case(n_disks=7, fills=(37, 515), kinds=("heavy", "uniform")),
    "one network": case(fills=(37,), kinds=("heavy",), rounds=2),
    # the widest and the narrowest observation the training update accepts: the [R][32] stage filled to two columns
    # from its end, and 3 columns of it
    "in_dim 30": case(n_disks=10, fills=(37, 515), kinds=("heavy", "uniform")),
    "in_dim 3": case(n_disks=1, fills=(37, 515), kinds=("uniform", "heavy")),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants(name):
    sets, lones, st_set, st_lone, _ = run_case(VARIANTS[name])
    assert_same(sets, lones, st_set, st_lone)
    assert (st_set[:, :, 0] == 0).all() and (st_set[:, :, 2] == 0).all(), st_set


def test_a_refused_draw_stays_with_its_network():
    """a NaN priority in network 1's ring: its draw reports 1 and gives the lone call's outputs (row 0), the others
    draw as ever"""
    c = case(nan_prio=1)
    sets, lones, st_set, st_lone, _ = run_case(c)
    assert_same(sets, lones, st_set, st_lone)
    assert st_set[0, :, 0].tolist() == [0, 1, 0], st_set
    assert bool((sets[1].view["indx"] == 0).all())


def test_a_refused_write_back_stays_with_its_network():
    """network 0's new priorities are all zero: its write-back reports 1 and leaves prio alone"""
    c = case(n_disks=4, support=1, fills=(37, 64), kinds=("uniform", "uniform"), zero_prio=0)
    sets, lones, st_set, st_lone, sp = run_case(c)
    assert_same(sets, lones, st_set, st_lone)
    assert bool((sets[0].view["new_prio"] == 0).all()), "the case must produce all-zero priorities"
    assert st_set[0, :, 2].tolist() == [1, 0], st_set
    assert np.array_equal(sets[0].prio.cpu().numpy().view(np.uint32), sp[0]["prio"].view(np.uint32))
    assert not np.array_equal(sets[1].prio.cpu().numpy().view(np.uint32), sp[1]["prio"].view(np.uint32))


def test_sequential_chain_draw_beside_an_exact_one():
    """priorities below 2^-28 of the total force the draw's sequential chain (status[1] = 0) in network 0"""
    c = case(fills=(515, 515), kinds=("tiny", "uniform"), rounds=2)
    sets, lones, st_set, st_lone, _ = run_case(c)
    assert_same(sets, lones, st_set, st_lone)
    assert st_set[0, :, 1].tolist() == [0, 1], st_set
    assert (st_set[:, :, 0] == 0).all()
