"""Engine: one libmzh engine (device workspace + packed weights) driven with torch tensors.

All tensors are device tensors on the engine's GPU; calls are asynchronous on torch's current
stream.  This is the layer the drop-in classes (env.py, networks.py, mcts.py) and bench.py use.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

WEIGHT_KEYS = [
    f"{net}.{layer}.{kind}"
    for net in ("representation_net", "dynamic_net", "rwd_net", "policy_net", "value_net")
    for layer in (0, 2)
    for kind in ("weight", "bias")
]

ACTIONS = 6
LATENT = 64
HIDDEN = 256


def flat_weights(state_dict):
    """MuZeroNet.state_dict() (or a dict of arrays) -> canonical flat fp32 numpy vector."""
    parts = []
    for k in WEIGHT_KEYS:
        v = state_dict[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().to("cpu", torch.float32).numpy()
        parts.append(np.asarray(v, np.float32).reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


def weight_shapes(n_disks, support):
    """the shapes of the 20 tensors of WEIGHT_KEYS for a Hanoi MuZeroNet of n_disks discs and a `support`-bin
    reward / value head (networks.py:39-67; the layer table of csrc/mzh_pack.cpp)"""
    mlps = ((3 * n_disks, LATENT), (LATENT + ACTIONS, LATENT), (LATENT, support), (LATENT, ACTIONS), (LATENT, support))
    shapes = []
    for i, o in mlps:
        shapes += [(HIDDEN, i), (HIDDEN,), (o, HIDDEN), (o,)]
    return shapes


def require_device():
    if not torch.cuda.is_available() or _lib.device_count() == 0:
        raise RuntimeError("muzero_hanoi_amd needs a HIP device (MI355X); there is no CPU fallback")


class Engine:
    def __init__(self, n_disks, max_sims, max_roots, support=33, device=None):
        require_device()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.n_disks = int(n_disks)
        self.max_sims = int(max_sims)
        self.max_roots = int(max_roots)
        self.support = int(support)
        h = ctypes.c_void_p()
        check(_lib.lib().mzh_create(self.device.index, self.n_disks, self.max_sims, self.max_roots,
                                     self.support, ctypes.byref(h)), "mzh_create")
        self._h = h
        self.weights_loaded = False

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            _lib.lib().mzh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _lib.stream_handle(self.device)

    # ---------------------------------------------------------------- weights
    def load_weights(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        n = ctypes.c_size_t()
        check(_lib.lib().mzh_weights_size(self.n_disks, self.support, ctypes.byref(n)), "mzh_weights_size")
        if flat.size != n.value:
            raise ValueError(f"expected {n.value} weights, got {flat.size}")
        torch.cuda.synchronize(self.device)
        check(_lib.lib().mzh_load_weights(self._h, flat.ctypes.data_as(ctypes.c_void_p), flat.size),
              "mzh_load_weights")
        self.weights_loaded = True

    def load_weight_set(self, flats):
        """a set of networks for search_multi (mzh_load_weight_set): a sequence of canonical flat vectors of this
        engine's shape.  The engine's own network (load_weights) is a separate allocation and stays as it is."""
        n = ctypes.c_size_t()
        check(_lib.lib().mzh_weights_size(self.n_disks, self.support, ctypes.byref(n)), "mzh_weights_size")
        flats = [np.ascontiguousarray(f, np.float32).reshape(-1) for f in flats]
        if not flats or any(f.size != n.value for f in flats):
            raise ValueError(f"expected a non-empty sequence of vectors of {n.value} weights, got sizes "
                             f"{[f.size for f in flats]}")
        flat = np.ascontiguousarray(np.stack(flats))
        torch.cuda.synchronize(self.device)
        check(_lib.lib().mzh_load_weight_set(self._h, flat.ctypes.data_as(ctypes.c_void_p), n.value, len(flats)),
              "mzh_load_weight_set")
        self.set_size = len(flats)

    def _param_pointers(self, params, what):
        """the 20 device pointers of one network's parameters for the device repack, validated: `params` is a
        mapping with the state_dict keys or a sequence in state_dict order (WEIGHT_KEYS).  ValueError on
        anything the gather could not read as it stands; nothing has been launched then."""
        if hasattr(params, "keys"):
            missing = [k for k in WEIGHT_KEYS if k not in params]
            if missing:
                raise ValueError(f"{what}: parameters {missing} are missing")
            params = [params[k] for k in WEIGHT_KEYS]
        params = list(params)
        if len(params) != len(WEIGHT_KEYS):
            raise ValueError(f"{what}: expected {len(WEIGHT_KEYS)} tensors in state_dict order, got {len(params)}")
        shapes = weight_shapes(self.n_disks, self.support)
        for k, t, shp in zip(WEIGHT_KEYS, params, shapes):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}: {k} is a {type(t).__name__}, not a tensor")
            if tuple(t.shape) != shp:
                raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, this engine's is {shp}")
            if t.dtype != torch.float32:
                raise ValueError(f"{what}: {k} is {t.dtype}, not torch.float32")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {k} is not contiguous")
            if t.device != self.device:
                raise ValueError(f"{what}: {k} is on {t.device}, the engine on {self.device}")
        return params

    def load_weights_from(self, params):
        """mzh_load_weights_device: load_weights(flat_weights(...)) without the host round trip -- the blobs are
        gathered on the device from the 20 parameter tensors as they are when the current stream reaches the
        call (contiguous fp32 tensors of this engine's shape on its device; a state_dict or a sequence in
        WEIGHT_KEYS order).  Same blob bytes, bit-identical results afterwards.  No torch.cuda.synchronize; a
        33-bin engine waits for the current stream once (two scalars the kernels take by value)."""
        params = self._param_pointers(params, "load_weights_from")
        arr = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        check(_lib.lib().mzh_load_weights_device(self._h, arr, self._stream()), "mzh_load_weights_device")
        self._weight_src = params  # the gather reads them at stream time
        self.weights_loaded = True

    def load_weight_set_from(self, param_sets):
        """mzh_load_weight_set_device: load_weight_set from the members' live parameter tensors (a sequence of
        what load_weights_from takes).  Never waits."""
        param_sets = list(param_sets)
        if not 1 <= len(param_sets) <= 256:
            raise ValueError(f"load_weight_set_from: a set has 1 to 256 networks, got {len(param_sets)}")
        sets = [self._param_pointers(p, f"load_weight_set_from: network {m}") for m, p in enumerate(param_sets)]
        flat = [t.data_ptr() for ps in sets for t in ps]
        arr = (ctypes.c_void_p * len(flat))(*flat)
        check(_lib.lib().mzh_load_weight_set_device(self._h, arr, len(sets), self._stream()),
              "mzh_load_weight_set_device")
        self._weight_set_src = sets
        self.set_size = len(sets)

    def debug_blob(self, which):
        """mzh_weights_debug_blob: a copy of a weight buffer as the kernels read it ([n] float32 on the device).
        which = 0 / 1 the engine's main / transposed blob, 2 / 3 the loaded set's (2 with its scalar tail)."""
        n = ctypes.c_size_t()
        fn = _lib.lib().mzh_weights_debug_blob
        check(fn(self._h, int(which), None, ctypes.byref(n)), "mzh_weights_debug_blob")
        out = self._f32(n.value)
        check(fn(self._h, int(which), ptr(out), ctypes.byref(n)), "mzh_weights_debug_blob")
        return out

    def debug_counters(self):
        """mzh_weights_debug_counters as a dict: allocations / frees of weight buffers and device-wide waits"""
        c = (ctypes.c_uint64 * 3)()
        check(_lib.lib().mzh_weights_debug_counters(self._h, c), "mzh_weights_debug_counters")
        return {"allocs": c[0], "frees": c[1], "device_waits": c[2]}

    # ---------------------------------------------------------------- inference
    def _f32(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def initial_inference(self, obs):
        obs = obs.to(self.device, torch.float32).contiguous()
        B = obs.shape[0]
        out = dict(h=self._f32(B, LATENT), reward=self._f32(B), pi=self._f32(B, ACTIONS), value=self._f32(B),
                   policy_logits=self._f32(B, ACTIONS), value_logits=self._f32(B, self.support))
        check(_lib.lib().mzh_initial_inference(self._h, B, ptr(obs), ptr(out["h"]), ptr(out["reward"]),
                                               ptr(out["pi"]), ptr(out["value"]), ptr(out["policy_logits"]),
                                               ptr(out["value_logits"]), self._stream()), "mzh_initial_inference")
        return out

    def recurrent_inference(self, h, action):
        h = h.to(self.device, torch.float32).contiguous()
        a = action.to(self.device, torch.int32).contiguous()
        B = h.shape[0]
        out = dict(h=self._f32(B, LATENT), reward=self._f32(B), pi=self._f32(B, ACTIONS), value=self._f32(B),
                   policy_logits=self._f32(B, ACTIONS), value_logits=self._f32(B, self.support),
                   reward_logits=self._f32(B, self.support))
        check(_lib.lib().mzh_recurrent_inference(self._h, B, ptr(h), ptr(a), ptr(out["h"]), ptr(out["reward"]),
                                                 ptr(out["pi"]), ptr(out["value"]), ptr(out["policy_logits"]),
                                                 ptr(out["value_logits"]), ptr(out["reward_logits"]),
                                                 self._stream()), "mzh_recurrent_inference")
        return out

    def _rows_call(self, who, args, inputs, outputs, tile, err, net_index, out):
        """what probe_actions, saliency and param_grads share.  args: the call's _lib structure.  inputs: (field,
        tensor or None, dtype, shape) in the order checked, "obs" first; outputs: (key of `out`, field, dtype, shape,
        allocate when missing).  A shape's "B" is obs's rows, its "n" env_index's (B without it).  Checks every given
        tensor, allocates, fills args (and with net_index a MultiArgs and out["_status"]) and calls mzh_<who>."""
        dev = self.device
        given = {f: t for f, t, _, _ in inputs}
        dims = {"B": int(given["obs"].shape[0])}
        dims["n"] = dims["B"] if given.get("env_index") is None else int(given["env_index"].shape[0])
        inputs = list(inputs) + [("net_index", net_index, torch.int32, ("n",))]
        checks = [(f, t, dt, shp) for f, t, dt, shp in inputs if t is not None]
        out = dict(out) if out is not None else {}
        for k, _, dt, shp, allocate in outputs:
            if k not in out and allocate:
                out[k] = torch.empty(tuple(dims.get(d, d) for d in shp), dtype=dt, device=dev)
            if k in out:
                checks.append((k, out[k], dt, shp))
        for name, t, dt, shp in checks:
            shp = tuple(dims.get(d, d) for d in shp)
            if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{who}: {name} must be a contiguous {dt} {shp} tensor on {dev}")
        args.B, args.n, args.flags, args.err_count = dims["B"], dims["n"], search_flags(None, tile), ptr(err)
        for f, t, _, _ in inputs[:-1]:
            setattr(args, f, ptr(t))
        for k, f, _, _, _ in outputs:
            setattr(args, f, ptr(out.get(k)))
        m = None
        if net_index is not None:
            if getattr(self, "set_size", 0) < 1:
                raise RuntimeError(f"{who}: no weight set loaded (load_weight_set)")
            out["_status"] = torch.zeros(2, dtype=torch.int32, device=dev)
            m = _lib.MultiArgs()
            m.n_networks, m.net_index, m.status = self.set_size, ptr(net_index), ptr(out["_status"])
        check(getattr(_lib.lib(), "mzh_" + who)(self._h, ctypes.byref(args), None if m is None else ctypes.byref(m),
                                                self._stream()), "mzh_" + who)
        return out

    def probe_actions(self, obs, *, env_index=None, state=None, net_index=None, out=None, full=False, tile=None,
                      err=None):
        """mzh_probe_actions: for every row the six one-step lookaheads recurrent_inference(represent(obs), a),
        a = 0..5, in one launch (legal_illegal_preds.py:39-57).  obs [B, 3N] float32 is the full batch's; row j of
        the call is env env_index[j] ([n] int32, distinct; None: every env, n = B); every output is indexed by env
        and rows outside the call are left as they are.  state [B, N] uint8 adds legal [B] (mzh_legal_mask's
        bits); net_index [n] int32 probes row j under network net_index[j] of the loaded weight set (non-decreasing).
        out: a dict of output tensors to write into (reward / value [B, 6] float32, legal [B] uint8, and with
        them any of h0 [B, 64], pi0 [B, 6], value0 [B], h1 [B, 6, 64], pi1 [B, 6, 6]); missing reward / value
        (and legal with state) are allocated, the others only with full=True.  tile = None | 16 | 32.
        Returns the dict; with net_index, "_status" is the device's [2] int32 verdict as in search_multi."""
        f32, N = torch.float32, self.n_disks
        return self._rows_call(
            "probe_actions", _lib.ProbeArgs(),
            [("obs", obs, f32, ("B", 3 * N)), ("env_index", env_index, torch.int32, ("n",)),
             ("state", state, torch.uint8, ("B", N))],
            [("reward", "reward", f32, ("B", ACTIONS), True), ("value", "value", f32, ("B", ACTIONS), True),
             ("h0", "h0", f32, ("B", LATENT), full), ("pi0", "pi0", f32, ("B", ACTIONS), full),
             ("value0", "value0", f32, ("B",), full), ("h1", "h1", f32, ("B", ACTIONS, LATENT), full),
             ("pi1", "pi1", f32, ("B", ACTIONS, ACTIONS), full),
             ("legal", "legal", torch.uint8, ("B",), state is not None)],
            tile, err, net_index, out)

    def saliency(self, obs, *, env_index=None, net_index=None, logit_index=None, out=None, full=False, tile=None,
                 err=None):
        """mzh_saliency: for every row d(policy logit k)/d(obs) and d(value)/d(obs) through represent + prediction
        in one launch (gradient_analysis.py:354-391).  obs [B, 3N] float32 is the full batch's; row j of the call is
        env env_index[j] ([n] int32, distinct; None: every env, n = B); every output is indexed by env and rows
        outside the call are left as they are.  logit_index [B] int32 names the logit differentiated (-1, or no
        logit_index: the row's largest); net_index [n] int32 runs row j under network net_index[j] of the loaded
        weight set (non-decreasing).  out: a dict of output tensors to write into (policy / value [B, 3N] float32,
        and with them any of picked [B] int32, disc_policy / disc_value [B, N], h0 [B, 64], pi0 [B, 6],
        value0 [B]); missing policy / value are allocated, the others only with full=True.  tile = None | 16 | 32.
        err: [1] int32, += 1 per skipped row.  Returns the dict; with net_index, "_status" is the device's [2]
        int32 verdict as in search_multi."""
        f32, N = torch.float32, self.n_disks
        return self._rows_call(
            "saliency", _lib.SaliencyArgs(),
            [("obs", obs, f32, ("B", 3 * N)), ("env_index", env_index, torch.int32, ("n",)),
             ("logit_index", logit_index, torch.int32, ("B",))],
            [("policy", "sal_policy", f32, ("B", 3 * N), True), ("value", "sal_value", f32, ("B", 3 * N), True),
             ("disc_policy", "disc_policy", f32, ("B", N), full), ("disc_value", "disc_value", f32, ("B", N), full),
             ("h0", "h0", f32, ("B", LATENT), full), ("pi0", "pi0", f32, ("B", ACTIONS), full),
             ("value0", "value0", f32, ("B",), full), ("picked", "picked", torch.int32, ("B",), full)],
            tile, err, net_index, out)

    def param_grads(self, obs, action, *, env_index=None, net_index=None, policy_logit=None, out=None, full=False,
                    tile=None, dense=False, err=None):
        """mzh_param_grads: for every row the parameter gradients of the five sub-networks (representation, dynamic,
        reward, policy, value; gradient_analysis.py:274-338) as rank-one factors, in one launch.  obs [B, 3N]
        float32 and action [B] int32 are the full batch's; row j of the call is env env_index[j] ([n] int32,
        distinct; None: every env, n = B); every output but grad is indexed by env and rows outside the call are
        left as they are.  policy_logit [B] int32: -1 (or None) the reference's mean(softmax) objective of the
        policy net, k its logit k; net_index [n] int32 runs row j under network net_index[j] of the loaded weight
        set (non-decreasing).  out: a dict of output tensors to write into (delta1 / act [B, 5, 256], delta2
        [B, 5, 64], h0 / z1 [B, 64] float32, and with them any of h1 [B, 64], pi0 [B, 6], value0 / reward [B],
        objective [B, 5], grad [n, n_floats]); the first five are allocated where missing, the others only with
        full=True, grad with dense=True (row j of the CALL: the dense gradients in load_weights' flat layout).
        tile = None | 16 | 32.  err: [1] int32, += 1 per skipped row.  Returns the dict; with net_index, "_status"
        is the device's [2] int32 verdict as in search_multi."""
        f32, N = torch.float32, self.n_disks
        n_floats = sum(int(np.prod(s)) for s in weight_shapes(N, self.support))
        shapes = dict(delta1=("B", 5, HIDDEN), delta2=("B", 5, LATENT), act=("B", 5, HIDDEN), h0=("B", LATENT),
                      z1=("B", LATENT), h1=("B", LATENT), pi0=("B", ACTIONS), value0=("B",), reward=("B",),
                      objective=("B", 5), grad=("n", n_floats))
        required = ("delta1", "delta2", "act", "h0", "z1")
        return self._rows_call(
            "param_grads", _lib.PgradArgs(),
            [("obs", obs, f32, ("B", 3 * N)), ("action", action, torch.int32, ("B",)),
             ("env_index", env_index, torch.int32, ("n",)), ("policy_logit", policy_logit, torch.int32, ("B",))],
            [(k, k, f32, shp, k in required or (dense if k == "grad" else full)) for k, shp in shapes.items()],
            tile, err, net_index, out)

    # ---------------------------------------------------------------- expansion memo (wave kernel)
    def set_memo_depth(self, depth):
        """mzh_set_memo_depth: -1 automatic (default), 0 off, d > 0 forced; takes effect with the next search"""
        check(_lib.lib().mzh_set_memo_depth(self._h, int(depth)), "mzh_set_memo_depth")

    def memo_stats(self):
        """mzh_memo_stats as a dict: depth, built, rows, table_bytes, build_ms and the cumulative
        pairs_skipped / pairs_packed / pairs_full of the wave searches (waits for the device); and, of the grown
        extension (mzh_memo_grow_stats): grow_budget_bytes, grow_capacity, grow_rows (in use), grow_rows_last
        (inserted by the last harvest), grow_log_entries"""
        info = _lib.MemoInfo()
        check(_lib.lib().mzh_memo_stats(self._h, ctypes.byref(info)), "mzh_memo_stats")
        g = _lib.MemoGrowInfo()
        check(_lib.lib().mzh_memo_grow_stats(self._h, ctypes.byref(g)), "mzh_memo_grow_stats")
        return dict(info.as_dict(), grow_budget_bytes=g.budget_bytes, grow_capacity=g.capacity_rows,
                    grow_rows=g.rows_used, grow_rows_last=g.rows_last_harvest, grow_log_entries=g.log_entries)

    def set_memo_grow(self, budget_bytes=-1, log_entries=-1):
        """mzh_set_memo_grow: the byte budget of the memo's grown extension (-1 the default, 0 off) and the per-root
        miss log's entries (-1 the default); takes effect with the next search"""
        check(_lib.lib().mzh_set_memo_grow(self._h, int(budget_bytes), int(log_entries)), "mzh_set_memo_grow")

    def memo_grow_table(self):
        """debug: the grown extension as (latent [used, 64] in natural unit order, record [used, 8], link
        [dense_rows + capacity, 6] of table rows (0: none), dense_rows); None without one.  Extension row i is
        table row dense_rows + i."""
        used, base, cap = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fn = _lib.lib().mzh_memo_debug_grow
        refs = (ctypes.byref(used), ctypes.byref(base), ctypes.byref(cap))
        check(fn(self._h, None, None, None, *refs), "mzh_memo_debug_grow")
        if cap.value == 0:
            return None
        n = cap.value
        h, rec = self._f32(n, LATENT), self._f32(n, 8)
        link = torch.empty((base.value + n, 6), dtype=torch.int32, device=self.device)
        check(fn(self._h, ptr(h), ptr(rec), ptr(link), *refs), "mzh_memo_debug_grow")
        u = used.value
        h = h[:u].view(u, 4, 4, 4).transpose(2, 3).reshape(u, LATENT).contiguous()
        return h, rec[:u].contiguous(), link, base.value

    def memo_table(self):
        """debug: copies of the built table as (latent [rows, 64] in natural unit order, record [rows, 8], depth);
        None before the first wave search built it.  Row = state * K(depth) + memo_node_id(path)."""
        rows, depth = ctypes.c_int64(), ctypes.c_int32()
        fn = _lib.lib().mzh_memo_debug_table
        check(fn(self._h, None, None, ctypes.byref(rows), ctypes.byref(depth)), "mzh_memo_debug_table")
        n = rows.value
        if n == 0:
            return None
        h, rec = self._f32(n, LATENT), self._f32(n, 8)
        check(fn(self._h, ptr(h), ptr(rec), ctypes.byref(rows), ctypes.byref(depth)), "mzh_memo_debug_table")
        # the wave kernel's order: position 16kb + 4g + t holds unit 16kb + 4t + g
        h = h.view(n, 4, 4, 4).transpose(2, 3).reshape(n, LATENT).contiguous()
        return h, rec, depth.value

    # ---------------------------------------------------------------- search
    def alloc_search_outputs(self, B, n_sims, lockstep=False):
        """lockstep=True adds lockstep_levels (zeroed, one entry per group of roots that advance together: at most
        one per root -- the latency kernel's groups are single roots)"""
        d = self.device
        extra = {"lockstep_levels": torch.zeros(B + 1, dtype=torch.int32, device=d)} if lockstep else {}
        return dict(**extra,
            visits=torch.empty((B, ACTIONS), dtype=torch.int32, device=d),
            root_q=torch.empty(B, dtype=torch.float64, device=d),
            minmax=torch.empty((B, 2), dtype=torch.float64, device=d),
            extra_ties=torch.empty(B, dtype=torch.int32, device=d),
            action=torch.empty(B, dtype=torch.int32, device=d),
            pi=torch.empty((B, ACTIONS), dtype=torch.float64, device=d),
            latent=torch.empty((B, n_sims + 1), dtype=torch.int32, device=d),
            latent_len=torch.empty(B, dtype=torch.int32, device=d),
            sel_steps=torch.empty(B, dtype=torch.int32, device=d),
        )

    def pow_table(self, n_sims, temperature):
        """play-policy power table for a non-integer exponent (None otherwise): np.power over
        arange(n_sims + 1) as int64 with the Python-float exponent, exactly the call
        generate_play_policy makes on the visit counts (MCTS/mcts.py:168-174), on the device"""
        if not 0.0 < temperature <= 1.0:
            return None
        e = max(1.0, min(5.0, 1.0 / temperature))
        if e == int(e):
            return None
        cache = self.__dict__.setdefault("_pow_tables", {})
        key = (int(n_sims), float(temperature))
        if key not in cache:
            tab = np.power(np.arange(n_sims + 1, dtype=np.int64), e)
            cache[key] = torch.from_numpy(tab).to(self.device)
        return cache[key]

    def search(self, n_sims, *, obs=None, replay=None, tie_idx, noise=None, action_u=None, minmax_in=None,
               temperature=1.0, deterministic=False, discount=0.8, eps=0.25, np1_ucb=False, out=None,
               kernel=None, tile=None):
        """Batched search. Tensors must already be on the device (bench: inputs resident in HBM).
        replay = dict(root_pi, pi, reward, value) -> tree-only mode (mzh_search_replay).
        kernel = None (automatic by batch size) | "coop" | "occ2" | "wave" | "wave16" | "one" (all give identical
        results; "one" = the latency kernel, MLP searches only);
        tile = None | 16 | 32: the cooperative kernel's roots per workgroup (default by batch size)."""
        a, out = self._search_args(n_sims, obs=obs, replay=replay, tie_idx=tie_idx, noise=noise, action_u=action_u,
                                   minmax_in=minmax_in, temperature=temperature, deterministic=deterministic,
                                   discount=discount, eps=eps, out=out, flags=search_flags(kernel, tile, np1_ucb))
        fn = _lib.lib().mzh_search_replay if replay is not None else _lib.lib().mzh_search
        check(fn(self._h, ctypes.byref(a), self._stream()), "mzh_search")
        out["_plan"] = out.pop("_plan_struct").as_dict()  # the instantiation the library launched
        return out

    def search_multi(self, n_sims, *, net_index, obs, tie_idx, noise=None, action_u=None, minmax_in=None,
                     temperature=1.0, deterministic=False, discount=0.8, eps=0.25, np1_ucb=False, out=None, tile=None,
                     sims=None, max_runs=None):
        """Batched search over the loaded weight set (load_weight_set): root b under network net_index[b], the
        roots of one network consecutive (net_index [B] non-decreasing, each in [0, set size)).  The other
        arguments and the result are search's; only the cooperative kernel has this form (tile = None | 16 | 32).
        sims: an int32 device tensor [B], root b runs sims[b] simulations (mzh_search_multi_budget) and gets what a
        search_multi of sims[b] simulations gives it; n_sims is then the maximum (every entry in [0, n_sims]; it
        sizes latent's rows and the power table).  Inside a network the budgets may come in any order.  max_runs:
        an upper bound on the runs of equal (net_index, sims) among consecutive roots, which sizes the grid
        (default: as many as the engine's tile workspace allows at 16-root tiles, at most B; never below 256).
        out["_status"] is the device's [2] int32 verdict: [0] = 1 where it refused net_index or sims (nothing
        was searched, no output written), [1] the tiles searched."""
        if getattr(self, "set_size", 0) < 1:
            raise RuntimeError("search_multi: no weight set loaded (load_weight_set)")
        if sims is not None:
            B = int(tie_idx.shape[0])
            if not isinstance(sims, torch.Tensor) or sims.dtype != torch.int32 or sims.dim() != 1 or sims.shape[0] != B:
                raise ValueError(f"search_multi: sims must be an int32 tensor with one entry per root ({B}), got "
                                 f"{getattr(sims, 'dtype', type(sims).__name__)} {tuple(getattr(sims, 'shape', ()))}")
            if max_runs is not None and int(max_runs) < 1:
                raise ValueError(f"search_multi: max_runs must be >= 1, got {max_runs}")
        elif max_runs is not None:
            raise ValueError("search_multi: max_runs goes with sims")
        a, out = self._search_args(n_sims, obs=obs, replay=None, tie_idx=tie_idx, noise=noise, action_u=action_u,
                                   minmax_in=minmax_in, temperature=temperature, deterministic=deterministic,
                                   discount=discount, eps=eps, out=out, flags=search_flags(None, tile, np1_ucb))
        ni = net_index.to(self.device, torch.int32).contiguous()
        if ni.dim() != 1 or ni.shape[0] != a.B:
            raise ValueError(f"search_multi: net_index must have one entry per root ({a.B}), got {tuple(ni.shape)}")
        status = torch.zeros(2, dtype=torch.int32, device=self.device)
        out["_keep"].append(ni)
        m = _lib.MultiArgs()
        m.n_networks = self.set_size
        m.net_index = ptr(ni)
        m.status = ptr(status)
        if sims is None:
            check(_lib.lib().mzh_search_multi(self._h, ctypes.byref(a), ctypes.byref(m), self._stream()), "mzh_search_multi")
        else:
            sd = sims.to(self.device).contiguous()
            out["_keep"].append(sd)
            b = _lib.BudgetArgs()
            b.n_sims = ptr(sd)
            # the workspace holds ceil(max_roots / 16) + 255 tiles; the grid is ceil(B / tile) + min(max_runs, B) - 1
            room = -(-self.max_roots // 16) + 256 - -(-a.B // 16)
            b.max_runs = max(1, min(a.B, room)) if max_runs is None else int(max_runs)
            check(_lib.lib().mzh_search_multi_budget(self._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(b),
                                                     self._stream()), "mzh_search_multi_budget")
        out["_plan"] = out.pop("_plan_struct").as_dict()
        out["_status"] = status
        return out

    def play_episodes(self, n_sims, state, max_steps, *, tie_idx, noise=None, action_u=None, minmax_in=None,
                      goal_peg=2, temperature=1.0, deterministic=False, discount=0.8, eps=0.25, np1_ucb=False,
                      record_obs=False, visits=False, out=None, err=None, net_index=None, sims=None, discounts=None):
        """Whole episodes in one launch (mzh_play_episodes): env b starts from state[b] ([B, n_disks] uint8) and
        plays until it is done; move t of env b searches with row [t, b] of tie_idx [T, B] int32, noise [T, B, 6]
        float64 (None: no root noise) and action_u [T, B] float64 (None when deterministic), its MinMaxStats
        starting from minmax_in[b] ([B, 2]; None: fresh) and carried on the device.  T >= max_steps.  All tensors
        on the engine's device.
        Returns the record -- pi [T, B, 6], root_q [T, B], action [T, B] int32, reward [T, B] int8 codes (0 -> 0,
        1 -> 100, -1 -> -0.1), with record_obs the observations searched obs [T, B, 3 n_disks], with visits=True
        visits [T, B, 6] -- whose rows t >= steps[b] the kernel leaves as they are (allocated here: action -1,
        everything else 0; or the caller's tensors of the same names in `out`), and per env steps, illegal
        (int32), solved (uint8), final_state [B, n_disks] and minmax [B, 2].  err [1] int32 counts the envs
        refused on the device (a start state with a peg outside 0..2; such an env plays nothing).
        net_index [B] (non-decreasing, each in [0, set size)): env b plays under network net_index[b] of the loaded
        weight set instead of the engine's network (mzh_play_episodes_multi), with the result a lone engine of
        that network gives; the dict then has "_status", the device's [2] int32 verdict: [0] = 1 where it refused
        net_index (nothing played, nothing written), [1] the networks that had envs.
        sims [B] int32 / discounts [B] float64 (device tensors; with net_index only): env b searches sims[b]
        simulations per move under discounts[b] (mzh_play_episodes_sweep) and plays as a lone engine of its network
        plays it with that budget and discount.  n_sims is then the launch's maximum (every entry in [0, n_sims]; a
        budget outside is refused on the device as a bad net_index is); discounts alone goes with sims = n_sims for
        every env, sims alone with `discount` for every env.  Both None: the calls and launches above."""
        d = self.device
        sweep = sims is not None or discounts is not None
        if sweep and net_index is None:
            raise ValueError("play_episodes: sims / discounts [B] need net_index: only the episodes of a weight set "
                             "take a budget and a discount per env")
        if net_index is not None and getattr(self, "set_size", 0) < 1:
            raise RuntimeError("play_episodes: no weight set loaded (load_weight_set)")
        if tie_idx.dim() != 2:
            raise ValueError(f"play_episodes: tie_idx must be [T, B], got {tuple(tie_idx.shape)}")
        T, B = (int(x) for x in tie_idx.shape)
        keep = []

        def dev(name, t, dtype, shape):
            if t is None:
                return None
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"play_episodes: {name} must be {dtype} {shape}, got {t.dtype} {tuple(t.shape)}")
            t = t.to(d).contiguous()
            keep.append(t)
            return t

        res = dict(out or {})
        for k, shape, dt, fill in (("pi", (T, B, ACTIONS), torch.float64, 0), ("root_q", (T, B), torch.float64, 0),
                                   ("action", (T, B), torch.int32, -1), ("reward", (T, B), torch.int8, 0),
                                   ("obs", (T, B, 3 * self.n_disks), torch.float32, 0),
                                   ("visits", (T, B, ACTIONS), torch.int32, 0)):
            if k in res:
                if not res[k].is_contiguous() or res[k].device != d:  # written in place: no silent copy
                    raise ValueError(f"play_episodes: out[{k!r}] must be contiguous on {d}")
                res[k] = dev(k, res[k], dt, shape)
            elif k not in ("obs", "visits") or (record_obs if k == "obs" else visits):
                res[k] = torch.full(shape, fill, dtype=dt, device=d)
        res.update(steps=torch.empty(B, dtype=torch.int32, device=d), illegal=torch.empty(B, dtype=torch.int32, device=d),
                   solved=torch.empty(B, dtype=torch.uint8, device=d),
                   final_state=torch.empty((B, self.n_disks), dtype=torch.uint8, device=d),
                   minmax=torch.empty((B, 2), dtype=torch.float64, device=d),
                   err=torch.zeros(1, dtype=torch.int32, device=d) if err is None else err)
        a = _lib.EpisodeArgs()
        a.B, a.T, a.n_sims, a.goal_peg, a.max_steps = B, T, int(n_sims), int(goal_peg), int(max_steps)
        a.deterministic, a.flags = (1 if deterministic else 0), search_flags(None, None, np1_ucb)
        a.discount, a.eps, a.temperature = float(discount), float(eps), float(temperature)
        a.state = ptr(dev("state", state, torch.uint8, (B, self.n_disks)))
        a.noise = ptr(dev("noise", noise, torch.float64, (T, B, ACTIONS)))
        a.tie_idx = ptr(dev("tie_idx", tie_idx, torch.int32, (T, B)))
        a.action_u = ptr(dev("action_u", action_u, torch.float64, (T, B)))
        a.minmax_in = ptr(dev("minmax_in", minmax_in, torch.float64, (B, 2)))
        pt = self.pow_table(n_sims, float(temperature))
        a.pow_table = ptr(pt)
        for k, f in (("pi", "pi"), ("root_q", "root_q"), ("action", "action"), ("reward", "reward"), ("visits", "visits"),
                     ("obs", "obs"), ("steps", "steps"), ("illegal", "illegal"), ("solved", "solved"),
                     ("final_state", "final_state"), ("minmax_out", "minmax"), ("err_count", "err")):
            setattr(a, k, ptr(res.get(f)))
        if net_index is None:
            check(_lib.lib().mzh_play_episodes(self._h, ctypes.byref(a), self._stream()), "mzh_play_episodes")
        else:
            ni = net_index.to(d, torch.int32).contiguous()
            if tuple(ni.shape) != (B,):
                raise ValueError(f"play_episodes: net_index must have one entry per env ({B}), got {tuple(ni.shape)}")
            res["_status"] = torch.zeros(2, dtype=torch.int32, device=d)
            keep.append(ni)
            m = _lib.MultiArgs()
            m.n_networks, m.net_index, m.status = self.set_size, ptr(ni), ptr(res["_status"])
            if sweep:
                for name, t, dt in (("sims", sims, torch.int32), ("discounts", discounts, torch.float64)):
                    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B,)):
                        got = f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}"
                        raise ValueError(f"play_episodes: {name} must be a {dt} tensor with one entry per env ({B}), "
                                         f"got {got}")
                sd = torch.full((B,), int(n_sims), dtype=torch.int32, device=d) if sims is None else dev(
                    "sims", sims, torch.int32, (B,))
                w = _lib.EpisodeSweepArgs()
                w.n_sims, w.discount = ptr(sd), ptr(dev("discounts", discounts, torch.float64, (B,)))
                keep.append(sd)
                check(_lib.lib().mzh_play_episodes_sweep(self._h, ctypes.byref(a), ctypes.byref(m), ctypes.byref(w),
                                                         self._stream()), "mzh_play_episodes_sweep")
            else:
                check(_lib.lib().mzh_play_episodes_multi(self._h, ctypes.byref(a), ctypes.byref(m), self._stream()),
                      "mzh_play_episodes_multi")
        res["_keep"] = keep + [pt]
        return res

    def _search_args(self, n_sims, *, obs, replay, tie_idx, noise, action_u, minmax_in, temperature, deterministic,
                     discount, eps, out, flags):
        """the mzh_search_args of a search / search_multi call and its result dict (outputs allocated unless given;
        "_keep": the inputs, alive until the caller is done with the asynchronous call)"""
        B = int(tie_idx.shape[0])
        if out is None:
            out = self.alloc_search_outputs(B, n_sims)
        keep = []

        def dev(t, dtype):
            if t is None:
                return None
            t = t.to(self.device, dtype).contiguous()
            keep.append(t)
            return t

        a = _lib.SearchArgs()
        a.B = B
        a.n_sims = int(n_sims)
        a.discount = float(discount)
        a.eps = float(eps)
        a.temperature = float(temperature)
        a.deterministic = 1 if deterministic else 0
        a.flags = flags
        a.obs = ptr(dev(obs, torch.float32))
        a.noise = ptr(dev(noise, torch.float64))
        a.tie_idx = ptr(dev(tie_idx, torch.int32))
        a.action_u = ptr(dev(action_u, torch.float64))
        a.minmax_in = ptr(dev(minmax_in, torch.float64))
        if replay is not None:
            a.rp_root_pi = ptr(dev(replay["root_pi"], torch.float32))
            a.rp_sim = ptr(dev(replay["sim"] if "sim" in replay else pack_replay(replay), torch.float32))
        for k, f in _lib.SEARCH_OUTPUTS:  # visits is required, the others optional
            setattr(a, k, ptr(out[f] if f == "visits" else out.get(f)))
        pt = self.pow_table(n_sims, float(temperature)) if (out.get("pi") is not None or
                                                              out.get("action") is not None) else None
        if pt is not None:
            keep.append(pt)
        a.pow_table = ptr(pt)
        a.lockstep_levels = ptr(out.get("lockstep_levels"))
        plan = _lib.SearchPlan()
        a.plan_out = ctypes.pointer(plan)
        out["_keep"] = keep
        out["_plan_struct"] = plan
        return a, out


def memo_node_id(path):
    """the expansion memo's node id of an action path: id(()) = 0, id(path + (a,)) = 6 id(path) + a + 1"""
    i = 0
    for a in path:
        if not 0 <= int(a) < ACTIONS:
            raise ValueError(f"action {a} outside [0, {ACTIONS})")
        i = 6 * i + int(a) + 1
    return i


def memo_nodes(depth):
    """nodes per state of a depth-D memo: K(D) = 1 + 6 + ... + 6^D"""
    return (6 ** (depth + 1) - 1) // 5


def memo_state_index(pegs):
    """a state's index in the memo: sum of peg(disc i) 3^i"""
    return sum(int(p) * 3 ** i for i, p in enumerate(pegs))


def search_flags(kernel=None, tile=None, np1_ucb=False):
    """mzh_search_args.flags for a kernel choice (None | "coop" | "occ2" | "wave" | "wave16" | "one") and coop
    tile ("occ2": the cooperative kernel's two-workgroups-per-CU 16-root form; "one": the latency kernel)"""
    f = _lib.MZH_FLAG_NP1_UCB if np1_ucb else 0
    f |= {None: 0, "auto": 0, "coop": _lib.MZH_FLAG_KERNEL_COOP, "wave": _lib.MZH_FLAG_KERNEL_WAVE,
          "wave16": _lib.MZH_FLAG_KERNEL_WAVE16,
          "occ2": _lib.MZH_FLAG_KERNEL_COOP | _lib.MZH_FLAG_COOP_OCC2, "one": _lib.MZH_FLAG_KERNEL_ONE}[kernel]
    return f | {None: 0, 16: _lib.MZH_FLAG_COOP_TILE16, 32: _lib.MZH_FLAG_COOP_TILE32}[tile]


def pack_replay(replay):
    """recorded network outputs pi [B,S,6], reward [B,S], value [B,S] -> the kernel's replay records
    [S,B,8] (6 priors, reward, value per simulation and root; simulation-major, mzh_search_args.rp_sim)"""
    pi = torch.as_tensor(replay["pi"], dtype=torch.float32)
    rw = torch.as_tensor(replay["reward"], dtype=torch.float32).to(pi.device)
    va = torch.as_tensor(replay["value"], dtype=torch.float32).to(pi.device)
    return torch.cat([pi, rw[..., None], va[..., None]], -1).transpose(0, 1).contiguous()


# ---------------------------------------------------------------- environment (no engine needed)
def env_step(n_disks, max_steps, state, action, step_ctr, active, goal_peg=2, moved=None, obs=None, err=None,
             reward=None, done=None, illegal=None):
    """Batched TowersOfHanoi.step on device tensors (state/step_ctr/active updated in place;
    reward codes / done / illegal written to the given tensors or fresh ones)."""
    B = state.shape[0]
    dev = state.device
    reward = torch.empty(B, dtype=torch.int8, device=dev) if reward is None else reward
    done = torch.empty(B, dtype=torch.uint8, device=dev) if done is None else done
    illegal = torch.empty(B, dtype=torch.uint8, device=dev) if illegal is None else illegal
    check(_lib.lib().mzh_env_step(n_disks, goal_peg, max_steps, B, ptr(state), ptr(action), ptr(moved), ptr(obs),
                                  ptr(reward), ptr(done), ptr(illegal), ptr(step_ctr), ptr(active), ptr(err),
                                  _lib.stream_handle(dev)), "mzh_env_step")
    return reward, done, illegal


def env_run_plan(n_disks, max_steps, state, step_ctr, active, obs, plan, plan_len, max_plan_len, steps_total,
                 illegal_total, *, env_index=None, goal_peg=2, err=None, record=False):
    """mzh_env_run_plan on device tensors: row j (env env_index[j], or j) executes plan[j, :min(plan_len[j],
    max_plan_len)] while its env is active.  state / step_ctr / active / obs / steps_total / illegal_total are the
    full batch's, updated in place; plan [n, stride] int32 and plan_len [n] int32 are read where the search left
    them.  Returns (executed [n], rec_action [L, n] | None, rec_reward [L, n] | None)."""
    dev = state.device
    n, L = int(plan_len.shape[0]), int(max_plan_len)
    if plan.dtype != torch.int32 or plan_len.dtype != torch.int32 or plan.dim() != 2 or plan.stride(1) != 1:
        raise ValueError("env_run_plan: plan [n, stride] and plan_len [n] must be int32 with unit inner stride")
    if env_index is not None and (env_index.dtype != torch.int32 or not env_index.is_contiguous()
                                  or env_index.shape[0] != n):
        raise ValueError("env_run_plan: env_index must be a contiguous int32 [n]")
    a = _lib.PlanArgs()
    a.n_disks, a.goal_peg, a.max_steps = int(n_disks), int(goal_peg), int(max_steps)
    a.B, a.n, a.max_plan_len, a.plan_stride = int(state.shape[0]), n, L, int(plan.stride(0))
    executed = torch.empty(n, dtype=torch.int32, device=dev)
    rec_a = torch.empty((L, n), dtype=torch.int32, device=dev) if record and L > 0 else None
    rec_r = torch.empty((L, n), dtype=torch.int8, device=dev) if record and L > 0 else None
    for k, t in (("env_index", env_index), ("plan", plan), ("plan_len", plan_len), ("state", state),
                 ("step_ctr", step_ctr), ("active", active), ("obs", obs), ("executed", executed),
                 ("steps_total", steps_total), ("illegal_total", illegal_total), ("rec_action", rec_a),
                 ("rec_reward", rec_r), ("err_count", err)):
        setattr(a, k, ptr(t))
    check(_lib.lib().mzh_env_run_plan(ctypes.byref(a), _lib.stream_handle(dev)), "mzh_env_run_plan")
    return executed, rec_a, rec_r


def env_step_observe(n_disks, max_steps, state, step_ctr, active, obs, steps_total, illegal_total, solved, *,
                     action=None, env_index=None, perm_disc=None, perm_peg=None, noise=None, goal_peg=2, err=None,
                     reward=None, done=None):
    """mzh_env_step_observe on device tensors: row j (env env_index[j], or j) takes action[j] on its true env
    (action None: no step) and, while the env is still active, its row of obs becomes the observation the model
    is to see: disc perm_disc[env]'s peg replaced by perm_peg[j], one-hot, plus noise[j] (float64, pre-scaled).
    state / step_ctr / active / obs / steps_total / illegal_total / solved (and perm_disc) are the full batch's,
    updated in place; action, perm_peg, noise are per row.  Returns (reward codes [n] int8, done [n] uint8)."""
    dev = state.device
    B, no = int(state.shape[0]), 3 * int(n_disks)
    n = next((int(t.shape[0]) for t in (env_index, action, perm_peg, noise) if t is not None), B)
    for name, t, dt, shape in (("env_index", env_index, torch.int32, (n,)), ("action", action, torch.int32, (n,)),
                               ("perm_disc", perm_disc, torch.int32, (B,)), ("perm_peg", perm_peg, torch.int32, (n,)),
                               ("noise", noise, torch.float64, (n, no)), ("obs", obs, torch.float32, (B, no)),
                               ("steps_total", steps_total, torch.int32, (B,)),
                               ("illegal_total", illegal_total, torch.int32, (B,)), ("solved", solved, torch.uint8, (B,))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"env_step_observe: {name} must be a contiguous {dt} {shape} tensor on {dev}")
    reward = torch.empty(n, dtype=torch.int8, device=dev) if reward is None else reward
    done = torch.empty(n, dtype=torch.uint8, device=dev) if done is None else done
    a = _lib.ObserveArgs()
    a.n_disks, a.goal_peg, a.max_steps, a.B, a.n = int(n_disks), int(goal_peg), int(max_steps), B, n
    for k, t in (("env_index", env_index), ("action", action), ("state", state), ("step_ctr", step_ctr),
                 ("active", active), ("steps_total", steps_total), ("illegal_total", illegal_total), ("solved", solved),
                 ("perm_disc", perm_disc), ("perm_peg", perm_peg), ("noise", noise), ("obs", obs), ("reward", reward),
                 ("done", done), ("err_count", err)):
        setattr(a, k, ptr(t))
    check(_lib.lib().mzh_env_step_observe(ctypes.byref(a), _lib.stream_handle(dev)), "mzh_env_step_observe")
    return reward, done


def legal_mask(n_disks, state):
    mask = torch.empty(state.shape[0], dtype=torch.uint8, device=state.device)
    check(_lib.lib().mzh_legal_mask(n_disks, state.shape[0], ptr(state), ptr(mask), _lib.stream_handle(state.device)),
          "mzh_legal_mask")
    return mask


def encode_obs(n_disks, state):
    obs = torch.empty((state.shape[0], 3 * n_disks), dtype=torch.float32, device=state.device)
    check(_lib.lib().mzh_encode_obs(n_disks, state.shape[0], ptr(state), ptr(obs), _lib.stream_handle(state.device)),
          "mzh_encode_obs")
    return obs


def hanoi_solver_batch(n_disks, state, goal_peg=2):
    moves = torch.empty(state.shape[0], dtype=torch.int32, device=state.device)
    check(_lib.lib().mzh_hanoi_solver(n_disks, goal_peg, state.shape[0], ptr(state), ptr(moves),
                                      _lib.stream_handle(state.device)), "mzh_hanoi_solver")
    return moves
