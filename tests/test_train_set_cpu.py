"""Host side of the set update (mzh_train_set_create / _update, MuzeroPopulation(update=...)): the boundary agrees
between include/mzh.h and the ctypes mirror, and every refusal comes before a device is needed, with a message that
names the field.  The argument blocks here hold made-up non-NULL addresses: a refusal never dereferences them."""
import ctypes
import re

import pytest

from test_abi_cpu import HEADER, _c_offsets, declared_symbols, lib  # noqa: F401  (lib: the built library's fixture)

B, U, IN_DIM, SUPPORT, RING = 5, 5, 9, 33, 64
FAKE = 0x10000  # 16-byte aligned, never dereferenced


def blocks(lib, M):
    """M consistent (mzh_train_args, mzh_replay_args) pairs as mzh_train_set_create accepts them"""
    nb = ctypes.c_size_t()
    assert lib.lib().mzh_train_scratch_bytes(B, U, IN_DIM, SUPPORT, nb) == lib.MZH_OK
    train, draw = (lib.TrainArgs * M)(), (lib.ReplayArgs * M)()
    for m in range(M):
        t, d = train[m], draw[m]
        base = FAKE * (m + 1) * 64
        t.B, t.U, t.in_dim, t.support, t.rows = B, U, IN_DIM, SUPPORT, 1
        t.beta1, t.beta2, t.eps = 0.9, 0.999, 1e-8
        for i in range(20):
            t.param[i], t.exp_avg[i], t.exp_avg_sq[i] = base + 16 * i, base + 0x1000 + 16 * i, base + 0x2000 + 16 * i
        for i in range(10):
            t.wt[i] = base + 0x3000 + 16 * i
        t.obs, t.rwds, t.actions, t.pi, t.returns = (base + 0x4000 + 16 * i for i in range(5))
        t.weights, t.scratch, t.scratch_bytes = base + 0x5000, base + 0x6000, nb.value
        t.row_loss, t.new_prio = base + 0x7000, base + 0x7100
        d.n, d.m, d.d_state, d.U, d.A = RING, B, IN_DIM, U, 6
        d.prio, d.cdf = base + 0x8000, base + 0x8100
        d.states, d.rwds, d.actions, d.pi, d.returns = (base + 0x9000 + 16 * i for i in range(5))
        d.indx = base + 0xA000
        d.out_states, d.out_rwds, d.out_actions, d.out_pi, d.out_returns = t.obs, t.rwds, t.actions, t.pi, t.returns
    return train, draw


def create(lib, train, draw, M):
    h = ctypes.c_void_p()
    st = lib.lib().mzh_train_set_create(train, draw, M, ctypes.byref(h))
    if st == lib.MZH_OK:  # only on a machine with a device
        lib.lib().mzh_train_set_destroy(h)
    else:
        assert not h.value
    return st, lib.last_error()


def test_symbols_and_struct_sizes_agree(lib, tmp_path):
    syms = declared_symbols()
    for name in ("mzh_train_set_create", "mzh_train_set_destroy", "mzh_train_set_update"):
        assert name in syms and name in lib.SIGNATURES and hasattr(lib.lib(), name), name
    fields = [f[0] for f in lib.TrainSetStep._fields_]
    want = [getattr(lib.TrainSetStep, f).offset for f in fields] + [ctypes.sizeof(lib.TrainSetStep)]
    assert _c_offsets("mzh_train_set_step", fields, tmp_path) == want
    assert ctypes.sizeof(lib.TrainSetStep) == 16
    cap = int(re.search(r"#define MZH_TRAIN_SET_MAX (\d+)", open(HEADER).read()).group(1))
    assert cap == lib.TRAIN_SET_MAX
    assert lib.lib().mzh_abi_version() == 6


def test_a_consistent_set_passes_the_host_checks(lib):
    """the blocks the refusals below start from are refused for nothing but a missing device (creation uploads the
    argument table and dereferences none of its addresses)"""
    import torch

    train, draw = blocks(lib, 3)
    st, msg = create(lib, train, draw, 3)
    assert st == (lib.MZH_OK if torch.cuda.is_available() else lib.MZH_ERR_HIP), msg


def edit(which, net, **fields):
    def go(train, draw):
        blk = (train if which == "train" else draw)[net]
        for k, v in fields.items():
            setattr(blk, k, v)
    return go


REFUSALS = [
    ("B differs", edit("train", 1, B=B + 1, scratch_bytes=1 << 40), r"network 1: B=6 differs"),
    ("U differs", edit("train", 2, U=4), r"network 2: U=4 differs"),
    ("in_dim differs", edit("train", 1, in_dim=12), r"network 1: in_dim=12 differs"),
    ("support differs", edit("train", 1, support=1), r"network 1: support=1 differs"),
    ("rows differ", edit("train", 2, rows=2), r"network 2: rows=2 differs"),
    ("draw.m", edit("draw", 1, m=B + 1), r"network 1: draw\.m=6 != train\.B=5"),
    ("draw.d_state", edit("draw", 0, d_state=12), r"network 0: draw\.d_state=12 != train\.in_dim=9"),
    ("draw.U", edit("draw", 0, U=4), r"network 0: draw\.U=4 != train\.U=5"),
    ("draw.A", edit("draw", 2, A=5), r"network 2: draw\.A=5 != 6"),
    ("out_states", edit("draw", 1, out_states=FAKE), r"network 1: draw\.out_states is not train\.obs"),
    ("out_rwds", edit("draw", 1, out_rwds=FAKE), r"network 1: draw\.out_rwds is not train\.rwds"),
    ("out_actions", edit("draw", 1, out_actions=FAKE), r"network 1: draw\.out_actions is not train\.actions"),
    ("out_pi", edit("draw", 1, out_pi=FAKE), r"network 1: draw\.out_pi is not train\.pi"),
    ("out_returns", edit("draw", 1, out_returns=FAKE), r"network 1: draw\.out_returns is not train\.returns"),
    ("new_prio", edit("train", 2, new_prio=None), r"network 2: new_prio is NULL"),
    # what train_check refuses
    ("train shape", edit("train", 0, support=7), r"network 0: train: bad B=5 U=5 in_dim=9 support=7"),
    ("null parameter", lambda t, d: t[1].param.__setitem__(3, None), r"network 1: train: null parameter .* 3"),
    ("null wt", lambda t, d: t[1].wt.__setitem__(4, None), r"network 1: train: null transposed weight 4"),
    ("null scratch", edit("train", 1, scratch=None), r"network 1: train: null batch / output / scratch"),
    ("short scratch", edit("train", 2, scratch_bytes=64), r"network 2: train: scratch of 64 bytes is too small"),
    ("bad rows", lambda t, d: [setattr(x, "rows", 3) for x in t], r"network 0: train: rows must be 1 or 2 \(got 3\)"),
    # what mzh_replay_sample refuses
    ("ring size", edit("draw", 1, n=0), r"network 1: replay_sample: bad n=0"),
    ("batch above the cap", lambda t, d: (setattr(t[0], "B", 4097), setattr(t[0], "scratch_bytes", 1 << 40),
                                          setattr(d[0], "m", 4097)),
     r"network 0: replay_sample: bad n=64 m=4097"),
    ("null ring array", edit("draw", 2, pi=None), r"network 2: replay_sample: null pointer"),
    ("unaligned prio", edit("draw", 1, prio=FAKE + 4), r"network 1: replay_sample: prio must be 16-byte aligned"),
]


@pytest.mark.parametrize("what,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_create_refuses_before_the_device(lib, what, change, message):
    train, draw = blocks(lib, 3)
    change(train, draw)
    st, msg = create(lib, train, draw, 3)
    assert st == lib.MZH_ERR_ARG, (what, st, msg)
    assert re.search(message, msg), (what, msg)


def test_create_refuses_bad_m_and_null_arguments(lib):
    L = lib.lib()
    train, draw = blocks(lib, 1)
    for M in (0, -1, lib.TRAIN_SET_MAX + 1):
        st, msg = create(lib, train, draw, M)
        assert st == lib.MZH_ERR_ARG and f"M={M} outside [1, {lib.TRAIN_SET_MAX}]" in msg, msg
    h = ctypes.c_void_p()
    assert L.mzh_train_set_create(None, draw, 1, ctypes.byref(h)) == lib.MZH_ERR_ARG and "train is NULL" in lib.last_error()
    assert L.mzh_train_set_create(train, None, 1, ctypes.byref(h)) == lib.MZH_ERR_ARG and "draw is NULL" in lib.last_error()
    assert L.mzh_train_set_create(train, draw, 1, None) == lib.MZH_ERR_ARG and "out is NULL" in lib.last_error()
    assert L.mzh_train_set_destroy(None) == lib.MZH_OK


def test_update_refuses_null_pointers(lib):
    L = lib.lib()
    step = (lib.TrainSetStep * 2)()
    u = (ctypes.c_double * (2 * B))()
    status = (ctypes.c_int32 * 8)()
    ptr = lambda x: ctypes.cast(x, ctypes.c_void_p)
    for args, name in (((None, ptr(u), ptr(status)), "step"), ((ptr(step), None, ptr(status)), "u"),
                       ((ptr(step), ptr(u), None), "status")):
        assert L.mzh_train_set_update(None, *args, None) == lib.MZH_ERR_ARG
        assert f"{name} is NULL" in lib.last_error()
    assert L.mzh_train_set_update(None, ptr(step), ptr(u), ptr(status), None) == lib.MZH_ERR_ARG
    assert "set is NULL" in lib.last_error()


def test_population_update_keyword_is_validated_first():
    """before any agent is built: no device, not even Muzero's own arguments are needed"""
    from muzero_hanoi_amd.muzero import MuzeroPopulation

    with pytest.raises(ValueError, match="update must be 'each' or 'set', not 'bogus'"):
        MuzeroPopulation([1, 2], update="bogus")
    with pytest.raises(ValueError, match="update_impl='fused' with device sampling"):
        MuzeroPopulation([1, 2], update="set", update_impl="torch")
    with pytest.raises(ValueError, match="update_impl='fused' with device sampling"):
        MuzeroPopulation([1, 2], update="set")
