"""The replay draw (csrc/mzh_replay.hip) at its structural edges, on chosen uniforms, against NumPy itself.

mzh_replay_sample is called directly (one workgroup, the caller's own uniforms); after each launch the
indices, the status, the cdf workspace and the five row outputs are read back.  The oracle everywhere is what
RandomState.choice computes:

    P = p / np.sum(p)                     # float32
    cdf = P.astype(np.float64).cumsum()
    c = cdf / cdf[-1]
    want = c.searchsorted(u, 'right')

* the cdf workspace holds the kernel's prefix sums before normalisation, cdf_ws[g] == cdf[min(4g + 3, n - 1)]
  bit for bit: a one-ulp error in np.sum's restatement, in a quotient or in a prefix fails here at once, where
  an index would change with probability ~1e-8 per draw;
* the sizes sit on the seams of np.sum's order (blocks of 8 / 128, buffers of 8,192), of the cdf pass (tiles of
  16,384), of the cdf sample (4,096 entries: its stride changes at n4 = 4,096 k + 1) and of the block passes
  (32 full buffers);
* the uniforms sit on cdf values and next to them (searchsorted's tie rule, the `> uk` comparisons of the LDS
  search, the binary steps in HBM, the 16-entry window and the replay inside a group), with runs of zero
  priorities for exact ties.
Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from test_replay import _prios

pytestmark = pytest.mark.gpu

NC, LIN = 4096, 16  # the kernel's cdf sample and search window (mzh_replay.hip)
N_MAX = 270337
TWO_M28 = np.float32(2.0 ** -28)


def _L():
    from muzero_hanoi_amd import _lib

    return _lib


class _Src:
    """five transition arrays whose every word identifies its row and column: floats distinct and non-zero,
    actions with both 32-bit halves non-zero, negative at odd positions and above 2^32 elsewhere"""

    def __init__(self, rows, d_state, U, A):
        def ar(w, mul):
            return (torch.arange(1, rows * w + 1, dtype=torch.float64, device="cuda") * mul).float().reshape(rows, w)

        self.d_state, self.U, self.A, self.rows = d_state, U, A, rows
        k = torch.arange(1, rows * U + 1, dtype=torch.int64, device="cuda")
        act = k * (2 ** 32 + 1) + (7 << 32)
        act = torch.where(k % 2 == 1, -act, act).reshape(rows, U)
        self.t = [ar(d_state, 1.0), ar(U, -3.0), act, ar(U * A, 0.5).reshape(rows, U, A), ar(U, 5.0)]


@pytest.fixture(scope="module")
def big_src():
    return _Src(N_MAX, 9, 5, 6)


def _launch(p, u, src):
    """one mzh_replay_sample over priorities p (float32, len n <= src.rows) and uniforms u (float64, len m)"""
    L = _L()
    n, m = len(p), len(u)
    assert 1 <= n <= src.rows and p.dtype == np.float32 and u.dtype == np.float64
    prio = torch.from_numpy(p).cuda()
    ud = torch.from_numpy(u).cuda()
    cdf = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    out = [torch.full((m,) + tuple(t.shape[1:]), 77, dtype=t.dtype, device="cuda") for t in src.t]
    indx = torch.full((m,), -5, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    r = L.ReplayArgs(n=n, m=m, d_state=src.d_state, U=src.U, A=src.A)
    r.prio, r.u, r.cdf, r.indx, r.status = prio.data_ptr(), ud.data_ptr(), cdf.data_ptr(), indx.data_ptr(), status.data_ptr()
    r.states, r.rwds, r.actions, r.pi, r.returns = (t.data_ptr() for t in src.t)
    r.out_states, r.out_rwds, r.out_actions, r.out_pi, r.out_returns = (t.data_ptr() for t in out)
    L.check(L.lib().mzh_replay_sample(ctypes.byref(r), L.stream_handle()), "mzh_replay_sample")
    torch.cuda.synchronize()
    return indx, status.cpu().numpy(), cdf.cpu().numpy(), out


def _numpy_cdf(p):
    with np.errstate(all="ignore"):
        P = p / np.sum(p)
        cdf = P.astype(np.float64).cumsum()
        return P, cdf, cdf / cdf[-1]


def _exact_path(P, cdf):
    """the kernel's stated condition for its parallel scan (mzh.h status[1]): every non-zero P_i >= 2^-28 and
    the total below 4"""
    return bool(np.all((P == 0) | (P >= TWO_M28)) and cdf[-1] < 4.0)


def _check(p, u, src, path=None):
    """launch and hold everything to NumPy: status, the cdf workspace (a), the indices and the rows"""
    n = len(p)
    P, cdf, c = _numpy_cdf(p)
    want = c.searchsorted(u, "right")
    assert want.max() < n
    exact = _exact_path(P, cdf)
    if path is not None:
        assert exact == path  # the case is on the path it was built for
    indx, status, ws, out = _launch(p, u, src)
    assert status.tolist() == [0, int(exact)]
    g = np.arange((n + 3) // 4)
    assert np.array_equal(ws[: len(g)].view(np.uint64), cdf[np.minimum(4 * g + 3, n - 1)].view(np.uint64))
    assert np.array_equal(indx.cpu().numpy(), want)
    wd = torch.from_numpy(want).cuda()
    for o, t in zip(out, src.t):
        assert torch.equal(o, t[wd])
    return want


def _window_ends(g, e):
    """the groups at which the kernel's binary steps in HBM can leave the window [g, e] of one cdf sample"""
    if e - g < LIN:
        return {g, e}
    mid = (g + e) >> 1
    return _window_ends(g, mid) | _window_ends(mid + 1, e)


def _edge_elements(n, rng, extra=()):
    n4 = (n + 3) // 4
    stride = (n4 + NC - 1) // NC
    nc = (n4 + stride - 1) // stride
    groups = {0, 1}
    for j in sorted({0, 1, nc // 2, nc - 2, nc - 1}):
        if j < 0:
            continue
        b = (j + 1) * stride
        groups |= {b - 1, b, b + 1}
        if stride >= LIN:
            groups |= _window_ends(j * stride, min(n4, b) - 1)
    el = {0, 1, n - 2, n - 1} | set(extra)
    for g in groups:
        el |= {4 * g - 1, 4 * g, 4 * g + 3}
    el |= set(rng.integers(0, n, 64).tolist())
    return np.array(sorted(i for i in el if 0 <= i < n), np.int64)


def _chosen_uniforms(p, m, rng, extra=()):
    """uniforms on NumPy's own normalised cdf values and their neighbours, 0.0, 1 - 2^-53, then random ones"""
    _, _, c = _numpy_cdf(p)
    ci = c[_edge_elements(len(p), rng, extra)]
    u = np.concatenate([ci, np.nextafter(ci, 0.0), np.nextafter(ci, 1.0), [0.0, 1.0 - 2.0 ** -53]])
    u = np.unique(u[(u >= 0.0) & (u < 1.0)])
    assert len(u) <= m
    u = np.concatenate([u, rng.random(m - len(u))])
    return np.ascontiguousarray(rng.permutation(u))


SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 8199, 8200, 8192 + 129,
         8192 + 4097, 16383, 16384, 16385, 16388, 65536, 65540, 262144, 262145, 262148, 270336, 270337]
M_EDGE = 1024


def _zero_run(n, kind):
    """[start, end) of the run of zero priorities of this kind, or None where n has no room for it"""
    n4 = (n + 3) // 4
    if kind == "lead0":
        return (0, min(9, n - 1)) if n >= 2 else None
    if kind == "trail0":
        return (n - min(9, n - 1), n) if n >= 2 else None
    if kind == "groups0":  # whole groups 1..3 and a part of group 4
        return (4, 18) if n >= 24 else None
    if kind == "stride0":  # more than one whole stride of the cdf sample, from the middle of a sample
        stride = (n4 + NC - 1) // NC
        s0 = 4 * (stride * (NC // 2) + 1)
        return (s0, s0 + 4 * (2 * stride + 3) + 2) if stride >= 2 and s0 + 12 * stride + 32 < n else None
    raise ValueError(kind)


_CASES = [(n, k) for n in SIZES for k in ("uniform", "heavy")]
_CASES += [(n, k) for n in SIZES for k in ("lead0", "trail0", "groups0") if _zero_run(n, k)]
_CASES += [(n, "stride0") for n in (65540, 270337)]


@pytest.mark.parametrize("n,kind", _CASES)
def test_draw_at_size_and_tie_edges(n, kind, big_src):
    """(a) the cdf workspace, (b) the sizes, (c) the chosen uniforms, with and without runs of zero priorities:
    indices, rows, cdf words and status equal NumPy's"""
    rng = np.random.default_rng(7 * n + len(kind))
    extra = ()
    if kind in ("uniform", "heavy"):
        p = _prios(rng, n, kind)
    else:
        p = _prios(rng, n, "uniform")
        z0, z1 = _zero_run(n, kind)
        p[z0:z1] = 0
        assert (p > 0).any()
        extra = (z0 - 1, z0, z0 + 1, z1 - 2, z1 - 1, z1)
    u = _chosen_uniforms(p, M_EDGE, rng, extra)
    want = _check(p, u, big_src)
    if kind == "lead0":
        assert want[u == 0.0].tolist() == [_zero_run(n, kind)[1]]  # u = 0.0 skips the leading zeros


# ---------------------------------------------------------------------------------------- (d) the row gather
@pytest.mark.parametrize("dims", [(3, 5, 6), (9, 5, 6), (48, 5, 6), (9, 1, 1), (5, 3, 7)])
def test_row_gather_lane_counts(dims):
    """every lanes-per-sample count of the gather (16, 8, 4, 2, 1) and both sides of each threshold, at the
    narrowest, the default and the widest observation rows and at odd row widths"""
    n = 200
    src = _Src(n, *dims)
    rng = np.random.default_rng(dims[0])
    p = _prios(rng, n, "uniform")
    for m in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096):
        _check(p, rng.random(m), src, path=True)


# ------------------------------------------------------------------------- (e) the sequential-chain path
@pytest.mark.parametrize("where", ["first", "last", "both"])
@pytest.mark.parametrize("n", [2, 5, 2047, 2048, 2049, 4099, 16385])
def test_chain_path_at_tile_edges(n, where, big_src):
    """probabilities below 2^-28 next to O(1) ones: NumPy's sequential chain through 2,048-element LDS tiles"""
    rng = np.random.default_rng(31 * n + len(where))
    p = (rng.random(n) + 0.5).astype(np.float32)
    tiny = set(rng.integers(0, n, n // 500).tolist()) if n > 5 else set()
    tiny |= {"first": {0}, "last": {n - 1}, "both": {0, n - 1}}[where]
    if len(tiny) == n:  # n = 2, both: one O(1) entry has to stay
        tiny = {0}
    p[sorted(tiny)] = np.float32(1e-9)
    _check(p, _chosen_uniforms(p, 512, rng, tuple(tiny)), big_src, path=False)


def test_exact_path_threshold(big_src):
    """P = 2^-28 is the last probability the parallel scan takes; the float below it goes to the chain"""
    rng = np.random.default_rng(5)
    for p1, path in ((TWO_M28, True), (np.nextafter(TWO_M28, np.float32(0)), False)):
        p = np.array([1.0, p1], np.float32)
        assert np.sum(p) == np.float32(1.0)
        _check(p, _chosen_uniforms(p, 64, rng), big_src, path=path)


@pytest.mark.parametrize("value,zeros", [(1e-42, 0), (1e-42, 3), (1e-40, 3)])
def test_all_subnormal_priorities(value, zeros, big_src):
    """a subnormal np.sum: NumPy forms P ~ 0.01 each and draws.  100 x 1e-42 sums to ~1.0005e-40, whose float32
    reciprocal is inf (0 * inf = NaN in the Markstein quotient of every zero priority, and of the elements past
    n); 100 x 1e-40 sums to ~1e-38, subnormal with a finite reciprocal"""
    p = np.full(100, np.float32(value), np.float32)
    p[10:10 + zeros] = 0
    s = np.sum(p)
    assert 0 < s < np.finfo(np.float32).tiny
    if zeros == 0:
        assert np.all(p / s == np.float32(0.01))
    rng = np.random.default_rng(6)
    _check(p, _chosen_uniforms(p, 512, rng, (9, 10, 12, 13)), big_src, path=True)


# --------------------------------------------------------------------------------------- (f) the refusals
def _refused(n, at, bad):
    p = (np.random.default_rng(n + at).random(n) + 0.05).astype(np.float32)
    p[at] = bad
    return p


_REFUSED = {
    "nan_n2": np.array([1, np.nan], np.float32), "inf_n2": np.array([1, np.inf], np.float32),
    "sum_overflows": np.array([3e38, 3e38], np.float32), "all_zero": np.array([0, 0], np.float32),
    "all_zero_16385": np.zeros(16385, np.float32),
}
for _at, _n in ((0, 10), (0, 16385), (8198, 8199), (16384, 16385)):  # first; the scalar tail load; the second tile
    for _name, _bad in (("neg", -0.5), ("nan", np.nan), ("inf", np.inf)):
        _REFUSED[f"{_name}_at_{_at}_of_{_n}"] = _refused(_n, _at, _bad)


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_refuses_what_numpy_refuses(case, big_src):
    p = _REFUSED[case]
    n, m = len(p), 300
    with np.errstate(all="ignore"):
        P = p / np.sum(p)
    with pytest.raises(ValueError):
        np.random.choice(np.arange(n), size=m, replace=True, p=P)
    indx, status, _, out = _launch(p, np.random.default_rng(1).random(m), big_src)
    assert status[0] == 1
    assert torch.equal(indx, torch.zeros(m, dtype=torch.int64, device="cuda"))
    for o, t in zip(out, big_src.t):
        assert torch.equal(o, t[:1].expand_as(o))


def test_accepts_negative_zero(big_src):
    p = np.array([-0.0, 1.0], np.float32)
    assert np.signbit(p[0])
    np.random.choice(np.arange(2), size=4, replace=True, p=p / np.sum(p))  # NumPy accepts it
    rng = np.random.default_rng(8)
    want = _check(p, _chosen_uniforms(p, 64, rng), big_src, path=True)
    assert (want == 1).all()


# ------------------------------------------------------------------------------ (g) sums above 2^126
# Above np.sum(p) = 2^126 the reciprocal RN(1/s) is subnormal and the Markstein quotient of mzh_fdiv can be one
# ulp off (tests/test_markstein.py); the draw takes IEEE quotients there.  Both fixtures were found on the CPU
# by emulating mzh_fdiv's three float32 operations exactly (oracle/mzh_oracle.c orc_markstein_f32, and in
# rational arithmetic): the pair (a, s) with p = [a, float32(s - a)], and, for n = 4,100 with the other 4,098
# priorities at 2e30 (P ~ 7e-9, still on the exact path), a walk of (a + k ulp, b - k ulp) that evaluated np.sum
# and the emulation at every k until P_0 was a mismatch (k = 3,402,574).  Bit patterns of float32:
G2_P, G2_SUM, G2_P0 = (0x7E8316A4, 0x7F27AC82), 0x7F6937D4, 1049617618
G4100_P, G4100_REST, G4100_SUM, G4100_P0 = (0x7EB701F2, 0x7EF3C134), 0x71C9F2CA, 0x7F556323, 1054576059


@pytest.mark.parametrize("n,head,rest,total,p0", [(2, G2_P, 0, G2_SUM, G2_P0),
                                                   (4100, G4100_P, G4100_REST, G4100_SUM, G4100_P0)])
def test_sum_above_2_126(n, head, rest, total, p0, big_src):
    """the cdf words and the indices around element 0 where 1/np.sum(p) is subnormal"""
    bits = np.full(n, rest, np.uint32)
    bits[:2] = head
    p = bits.view(np.float32)
    s = np.sum(p)
    assert s.view(np.uint32) == total and s > np.float32(2.0 ** 126)  # NumPy still sums to the fixture's s
    assert (p[0] / s).view(np.uint32) == p0
    rng = np.random.default_rng(9)
    _check(p, _chosen_uniforms(p, 512, rng), big_src, path=True)


# ------------------------------------------------------------------------------------- (h) the write-back
def _set_priorities(prio, idx, val):
    L = _L()
    pd, idd, vd = torch.from_numpy(prio).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda()
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    L.check(L.lib().mzh_replay_set_priorities(pd.data_ptr(), len(prio), idd.data_ptr(), vd.data_ptr(), len(idx),
                                              status.data_ptr(), L.stream_handle()), "mzh_replay_set_priorities")
    torch.cuda.synchronize()
    return pd.cpu().numpy(), int(status.item())


SIZE = 5000


def _repeats(m, rng):
    """distinct indices, then repeats whose later copy sits inside the first 8-wide chunk a thread compares,
    in its scalar tail, and in the k the same thread owns on its second trip (k + 1024); index size - 1"""
    idx = rng.permutation(SIZE - 1)[:m].astype(np.int64)
    idx[m // 2] = SIZE - 1
    pairs = []
    if m >= 9:
        pairs.append((0, 3))  # k = 0 compares [1, 9) unrolled
    if m >= 2:
        k = 1 if m >= 3 and (m - 2) % 8 else 0
        k2 = m - 1 if m <= 1024 else m - 2  # one of the last (m - k - 1) % 8 entries: k's scalar tail
        if (m - k - 1) % 8 >= m - k2:
            pairs.append((k, k2))
    if m > 1024:  # thread t owns k = t and t + 1024
        pairs += [(m - 1025, m - 1), (1000, 1022)]
    if m > 2048:
        pairs += [(5, 5 + 1024), (1030, 1030 + 7), (1100, 3 * 1024 + 1)]
    for k, k2 in pairs:
        assert k < k2 < m
        idx[k2] = idx[k]
    assert len({k2 for _, k2 in pairs}) == len(pairs) and not {k2 for _, k2 in pairs} & {k for k, _ in pairs}
    return idx, pairs


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("m", [1, 8, 9, 10, 17, 1025, 4096])
def test_set_priorities_last_repeat_wins(m, dense):
    rng = np.random.default_rng(m + dense)
    prio = (rng.random(SIZE) + 0.05).astype(np.float32)
    if dense:  # every index repeated ~4 times anywhere in the batch
        idx = rng.integers(SIZE - 1 - max(1, m // 4), SIZE, m).astype(np.int64)
    else:
        idx, pairs = _repeats(m, rng)
        assert m < 17 or len(pairs) >= 2
    val = rng.normal(size=m).astype(np.float32)  # negatives are allowed next to one positive
    val[rng.integers(0, m)] = 0.75
    want = prio.copy()
    want[idx] = val
    got, status = _set_priorities(prio, idx, val)
    assert status == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("m", [1, 9, 1025, 4096])
def test_set_priorities_refusals_write_nothing(m):
    rng = np.random.default_rng(m)
    prio = (rng.random(SIZE) + 0.05).astype(np.float32)
    idx = rng.integers(0, SIZE, m).astype(np.int64)
    good = (rng.random(m) + 0.01).astype(np.float32)
    last = m - 1  # for m > 1024 a k of a thread's second trip

    def put(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    cases = [(idx, -np.abs(good), 1), (idx, np.zeros(m, np.float32), 1), (idx, put(good, last, -np.inf), 1),
             (idx, put(good, last, np.nan), 1), (idx, put(good, 0, np.inf), 1),
             (put(idx, last, -1), good, 2), (put(idx, last, SIZE), good, 2), (put(idx, 0, SIZE), good, 2)]
    for i, v, code in cases:
        got, status = _set_priorities(prio, i, v)
        assert status == code
        assert np.array_equal(got, prio)
    got, status = _set_priorities(prio, idx, good)  # and the same batch unspoilt is written
    want = prio.copy()
    want[idx] = good
    assert status == 0 and np.array_equal(got, want)
