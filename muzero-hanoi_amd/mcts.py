"""MCTS drop-in (reference: MCTS/mcts.py:8-176, MCTS/node.py, MCTS/utils_mcts.py).

`MCTS.run_mcts(state, network, temperature, deterministic)` keeps the reference's signature,
return types, RNG consumption (global legacy NumPy stream, see rng.py), MinMaxStats persistence
across calls on one instance (mcts.py:23) and `return_latent_actions`.  The whole search -- root
inference, every simulation's select / MLP expansion / backup, and the play policy -- is one
fused libmzh kernel launch on the GPU (mzh_search).  Every one-root call (run_mcts, run_mcts_step,
play_episode; a network or a RecordedNetwork) goes through one host path, `_OneRootSearch`.

`MCTS.run_batch(states, ...)` runs B independent searches in one launch (each root with its own
MinMaxStats, i.e. B fresh single-root searches), the form the bench and batched self-play use.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib
from . import rng as _rng
from .engine import Engine, pack_replay
from .networks import engine_for
from .staging import Packed

_ENV_REWARD = {0: 0, 1: 100, -1: -100 / 1000}  # mzh_env_step codes -> the reference's rewards (env.py)


_REPLAY_ENGINES = {}


def _replay_engine(n_disks, n_sims):
    eng = _REPLAY_ENGINES.get(n_disks)
    if eng is None or eng.max_sims < n_sims:
        eng = Engine(n_disks, max(n_sims, 64), 1, 33)
        _REPLAY_ENGINES[n_disks] = eng
    return eng


class MinMaxStats(object):
    """utils_mcts.py:1-16 (host mirror; the device carries the same two doubles)."""

    def __init__(self, min_value_bound=None, max_value_bound=None):
        self.maximum = min_value_bound if min_value_bound else -float("inf")
        self.minimum = max_value_bound if max_value_bound else float("inf")

    def update(self, value):
        self.maximum = max(self.maximum, value)
        self.minimum = min(self.minimum, value)

    def normalize(self, value):
        if self.maximum > self.minimum:
            return (value - self.minimum) / (self.maximum - self.minimum)
        return value


class RecordedNetwork:
    """Network duck type whose outputs were recorded (tree-only mode, mzh_search_replay).

    calls: list of dicts, one per run_mcts call, each with root_pi [6] and, per simulation,
    pi [S,6], reward [S], value [S] (fp32 values, exactly what the network returned)."""

    def __init__(self, calls, n_disks, num_actions=6):
        self.calls = list(calls)
        self.n_disks = n_disks
        self.num_actions = num_actions
        self.cursor = 0

    def next_call(self):
        c = self.calls[self.cursor]
        self.cursor += 1
        return c

    def last_probe(self):
        """the action probe recorded with the call next_call() returned last (optional key "probe": reward [6],
        value [6] float32 -- recurrent_inference(represent(obs), a) for a = 0..5, legal_illegal_preds.py:39-50)"""
        call = self.calls[self.cursor - 1]
        if "probe" not in call:
            raise KeyError("RecordedNetwork: the recording holds no action probe for this call")
        return call["probe"]

    def next_replay(self, device):
        """next_call() as Engine.search's `replay` tensors: fp32 [1, ...] on `device`"""
        call = self.next_call()
        return {k: torch.as_tensor(np.asarray(call[k], np.float32)).to(device)[None]
                for k in ("root_pi", "pi", "reward", "value")}


class _OneRootSearch:
    """The host side of one one-root search: the staging records (the kernel reads its inputs from and writes
    its outputs to pinned host memory where the device can address it -- a call is one launch and one
    synchronisation -- else one copy each way), a SearchArgs with their device addresses filled in once, and the
    staging addresses rng.predraw_into writes the draws to.  `launch` does not synchronise; `read` follows the
    caller's synchronisation (pout.to_host() or an event)."""

    def __init__(self, eng, S, in_dim):
        self.eng, self.S = eng, S
        self.pin = Packed.mapped([("obs", torch.float32, (1, in_dim)), ("noise", torch.float64, (1, 6)),
                                  ("tie", torch.int32, (1,)), ("u", torch.float64, (1,)),
                                  ("mm", torch.float64, (1, 2))], eng.device)
        self.pout = Packed.mapped([("visits", torch.int32, (1, 6)), ("root_q", torch.float64, (1,)),
                                   ("minmax", torch.float64, (1, 2)), ("extra_ties", torch.int32, (1,)),
                                   ("action", torch.int32, (1,)), ("pi", torch.float64, (1, 6)),
                                   ("latent", torch.int32, (1, S + 1)), ("latent_len", torch.int32, (1,)),
                                   ("sel_steps", torch.int32, (1,))], eng.device)
        a = self.args = _lib.SearchArgs()
        a.B, a.n_sims = 1, S
        a.tie_idx = self.pin.dptr["tie"]
        for k, f in _lib.SEARCH_OUTPUTS:
            setattr(a, k, self.pout.dptr[f])
        # what every call uses, looked up once: the call itself, the draws' arrays and their addresses, views of
        # the records and the inputs' device addresses
        L = _lib.lib()
        self._call = {False: L.mzh_search, True: L.mzh_search_replay}, ctypes.byref(a)
        h, o, d = self.pin.h, self.pout.h, self.pin.dptr
        self.draws = (h["noise"], h["tie"], h["u"])
        self.addrs = tuple(x.ctypes.data for x in self.draws)
        self.obs, self.mm = h["obs"][0], h["mm"][0]
        self.d_obs, self.d_mm, self.d_noise, self.d_u = d["obs"], d["mm"], d["noise"], d["u"]
        self.out = tuple(v.reshape(-1) for v in o.values())  # flat views, in the record's field order
        self.bad_temperature = None
        self._keep = None  # a replay's tensors, alive until the next launch

    def launch(self, m, temperature, deterministic, state=None, replay=None, obs_ptr=None, minmax_ptr=None):
        """Draw (reference order, straight into the staging record), stage and launch `m`'s search on the current
        stream.  The observation is `state`, or what a device address holds (`obs_ptr`), or none for a
        `replay` (RecordedNetwork.next_replay: the tree-only kernel); MinMaxStats come from `m` or from
        `minmax_ptr` (MCTS.play_episode chains a decision to the previous one's device outputs)."""
        # the reference raises for a bad temperature inside generate_play_policy (mcts.py:113, 163-166): after
        # the whole search (Dirichlet draw, argmax tie draws, MinMaxStats updates, latent_actions) and before
        # the action draw (mcts.py:120).  So the search runs, its state is kept, no action uniform is drawn,
        # then the ValueError (in `read`).
        bad_t = not 0.0 <= temperature <= 1.0
        self.bad_temperature = temperature if bad_t else None
        eps = m.root_exploration_eps
        noisy, drew_u = _rng.predraw_into(*self.draws, deterministic=deterministic, alpha=m.root_dirichlet_alpha,
                                          eps=eps, draw_action=not bad_t, addrs=self.addrs)
        if bad_t:
            deterministic, temperature = True, 0.0  # the kernel's policy output is discarded
        temperature = float(temperature)
        if state is not None:
            self.obs[:] = state
        if minmax_ptr is None:
            mms, mm = m.min_max_stats, self.mm
            mm[0] = mms.maximum
            mm[1] = mms.minimum
        self.pin.to_device()
        a, eng = self.args, self.eng
        a.discount = float(m.discount)
        a.eps = float(eps)
        a.temperature = temperature
        a.deterministic = 1 if deterministic else 0
        a.flags = _lib.MZH_FLAG_NP1_UCB if m.np1_ucb else 0
        a.obs = None if replay is not None else (obs_ptr or self.d_obs)
        a.minmax_in = minmax_ptr or self.d_mm
        a.noise = self.d_noise if noisy else None
        a.action_u = self.d_u if drew_u else None
        pt = eng.pow_table(self.S, temperature)
        a.pow_table = None if pt is None else pt.data_ptr()
        if replay is not None:
            self._keep = (replay["root_pi"].contiguous(), pack_replay(replay))
            a.rp_root_pi, a.rp_sim = (t.data_ptr() for t in self._keep)
        fns, aref = self._call
        _lib.check(fns[replay is not None](eng._h, aref, _lib.stream_handle(eng.device)), "mzh_search")

    def read(self, m):
        """the launched search's results, once they are in the host record: MinMaxStats, the latent path and
        extra_ties go back to `m`; returns (action int, pi np.float64[6], root Q float)"""
        _, root_q, minmax, extra_ties, action, pi, latent, latent_len, _ = self.out
        mms = m.min_max_stats
        mms.maximum = float(minmax[0])
        mms.minimum = float(minmax[1])
        m._latent_host = latent[:int(latent_len[0])].tolist()  # tensors made on first access
        ties = m.last_extra_ties = int(extra_ties[0])
        if ties:
            warnings.warn("search met an argmax tie beyond the root's first selection: the NumPy RNG stream "
                          "now differs from the reference's", RuntimeWarning)
        if self.bad_temperature is not None:
            raise ValueError(f"Expect `temperature` to be in the range [0.0, 1.0], got {self.bad_temperature}")
        return int(action[0]), pi.astype(np.float64), float(root_q[0])


class MCTS:
    def __init__(self, discount, root_dirichlet_alpha, n_simulations, batch_s, device, h_dim=64, clip_grad=True,
                 root_exploration_eps=0.25, known_bounds=[]):
        self.min_max_stats = MinMaxStats()
        self.pb_c_base = 19652  # baked into the kernel's UCB table (mzh_create)
        self.pb_c_init = 1.25
        self.discount = discount
        self.root_dirichlet_alpha = root_dirichlet_alpha
        self.root_exploration_eps = root_exploration_eps
        self.n_simulations = n_simulations
        self.batch_s = batch_s
        self.dev = device
        self.latent_actions = []
        self.np1_ucb = False  # True: NumPy-1.x UCB rounding (the reference's numpy==1.25.2 pin)
        self.last_extra_ties = 0
        self._one_key, self._one = None, []

    # ------------------------------------------------------------------ reference API
    def run_mcts(self, state, network, temperature, deterministic):
        """mcts.py:34-126 -> (action int, pi np.float64[6], root Q float)."""
        if self.pb_c_base != 19652 or self.pb_c_init != 1.25:
            raise NotImplementedError("libmzh bakes pb_c_base=19652, pb_c_init=1.25 (mcts.py:24-25)")
        one = self._launch(state, network, temperature, deterministic)
        one.pout.to_host()
        return one.read(self)

    def _one_root(self, eng, S, in_dim, n=1):
        """n _OneRootSearch objects, cached per (engine, S, observation width)"""
        key = (id(eng), S, in_dim)  # the cached objects hold `eng`: its id is not reused meanwhile
        if self._one_key != key:
            self._one_key, self._one = key, []
        while len(self._one) < n:
            self._one.append(_OneRootSearch(eng, S, in_dim))
        return self._one

    def _launch(self, state, network, temperature, deterministic):
        """run_mcts up to the launch: a network's search on its engine, a RecordedNetwork's next call on the
        replay engine (tree-only kernel; the observation is staged but not read)"""
        S = int(self.n_simulations)
        x = np.asarray(state).reshape(-1)
        if isinstance(network, RecordedNetwork):
            eng = _replay_engine(network.n_disks, S)
            replay = network.next_replay(eng.device)
        else:
            eng, replay = engine_for(network, S, 1), None
        one = self._one_root(eng, S, x.size)[0]
        one.launch(self, temperature, deterministic, x, replay)
        return one

    def _chains(self, network, temperature, env):
        """whether run_mcts_step / play_episode may chain a search to `env`'s step on the device"""
        return (not isinstance(network, RecordedNetwork) and 0.0 <= temperature <= 1.0 and env.reset_check
                and self.pb_c_base == 19652 and self.pb_c_init == 1.25)

    def run_mcts_step(self, state, network, temperature, deterministic, env):
        """run_mcts(state, ...) followed by env.step(action) (Muzero._play_game's pair of calls,
        Muzero.py:165-175) as two chained launches and ONE synchronisation: the env kernel reads the
        action the search kernel wrote.  The same draws, results and env state as the two calls.
        Returns (action, pi, root_Q, env.step's tuple), or None where run_mcts itself must run (a replayed
        network, a temperature it refuses, an env not reset, other UCB constants) -- the caller then makes
        the two calls; with staging through copies or the env on another device the two run one after
        the other here."""
        if not self._chains(network, temperature, env):
            return None
        one = self._launch(state, network, temperature, deterministic)
        pout, dev = one.pout, one.eng.device
        if pout.zero_copy and env._packed().zero_copy and torch.device(dev) == env._dev:
            env._launch_step(action_ptr=pout.dptr["action"])
            _lib.synchronize(dev)
            action, pi, q = one.read(self)
            return action, pi, q, env._finish_step()
        pout.to_host()  # staging with copies: the two calls one after the other
        action, pi, q = one.read(self)
        return action, pi, q, env.step(action)

    def play_episode(self, env, network, temperature, deterministic):
        """Muzero._play_game's decision loop (run_mcts then env.step until done, Muzero.py:165-186) with the
        decisions pipelined on the device: decision k+1's search reads its observation from decision k's env
        kernel and its MinMaxStats from decision k's search, so it is launched (with its env step) BEFORE the
        host waits for decision k -- the GPU runs decision after decision while the host records the last one.
        When decision k ends the episode, the speculative decision k+1 is discarded: its env step meets an
        inactive env (left untouched, as the kernel's AssertionError path does) and the NumPy stream is put back
        to where decision k left it.  The same draws, results, MinMaxStats and env state as the per-decision calls
        (tests/test_selfplay.py).  Returns (steps, obs list, actions, rewards, pis, root Qs) or None where the
        pipeline does not apply (then the caller makes the per-decision calls)."""
        S = int(self.n_simulations)
        bg = np.random.mtrand._rand._bit_generator
        if (not self._chains(network, temperature, env) or type(bg).__name__ != "MT19937"
                or (_rng.uses_noise(deterministic, self.root_dirichlet_alpha, self.root_exploration_eps)
                    and not 0.0 < float(self.root_dirichlet_alpha) <= 1.0)):
            return None
        eng = engine_for(network, S, 1)
        x0 = np.asarray(env.oneH_c_state if hasattr(env, "oneH_c_state") else None)
        sets = self._one_root(eng, S, env.discs * 3, 2)  # alternating between decisions
        ek, eo = env._packed(), env._packed_out2()
        if not all(p.zero_copy for one in sets for p in (one.pin, one.pout)) or not (ek.zero_copy and eo.zero_copy) \
                or torch.device(eng.device) != env._dev or x0.shape != (env.discs * 3,):
            return None
        stream = _lib.stream_handle(eng.device)
        L = _lib.lib()
        outs = [(ek.h, ek.dptr), (eo.h, eo.dptr)]  # env output records, alternating
        q = ek.dptr  # state / ctr / active: one record, updated in place decision after decision
        eh = ek.h
        eh["state"][0] = env.c_state
        eh["ctr"][0] = env.step_counter
        eh["active"][0] = 1
        mt = ctypes.c_char * 2500  # struct mt19937_state {uint32 key[624]; int pos}
        saved = mt()
        st_addr = bg.ctypes.state_address
        evs = [torch.cuda.Event(), torch.cuda.Event()]

        def launch(k):
            one = sets[k % 2]
            if k == 0:
                one.launch(self, temperature, deterministic, state=x0)
            else:  # the previous decision's env observation and search MinMaxStats, on the device
                one.launch(self, temperature, deterministic, obs_ptr=outs[(k - 1) % 2][1]["obs"],
                           minmax_ptr=sets[(k - 1) % 2].pout.dptr["minmax"])
            o = outs[k % 2][1]
            _lib.check(L.mzh_env_step(env.discs, env.goal_peg, env.max_steps, 1, q["state"], one.pout.dptr["action"],
                                      o["moved"], o["obs"], o["code"], o["done"], o["illegal"], q["ctr"], q["active"],
                                      None, stream), "mzh_env_step")
            evs[k % 2].record(torch.cuda.current_stream(eng.device))

        obs_l, act_l, rwd_l, pi_l, q_l = [x0.astype(np.float64)], [], [], [], []
        launch(0)
        k = 0
        while True:
            ctypes.memmove(saved, st_addr, 2500)  # the stream before the speculative next decision's draws
            launch(k + 1)
            evs[k % 2].synchronize()
            action, pi, root_q = sets[k % 2].read(self)
            oh = outs[k % 2][0]
            act_l.append(action)
            pi_l.append(pi)
            q_l.append(root_q)
            rwd_l.append(_ENV_REWARD[int(oh["code"][0])])
            done = bool(oh["done"][0])
            if done:
                ctypes.memmove(st_addr, saved, 2500)  # the discarded decision's draws never happened
                evs[(k + 1) % 2].synchronize()  # it ran on an inactive env: state, counter untouched
                break
            obs_l.append(oh["obs"][0].astype(np.float64))
            k += 1
        env.c_state = tuple(int(v) for v in eh["state"][0])
        env.step_counter, env.reset_check = int(eh["ctr"][0]), bool(eh["active"][0])
        return k + 1, obs_l, act_l, rwd_l, pi_l, q_l

    def return_latent_actions(self):
        return self.latent_actions

    @property
    def latent_actions(self):
        """mcts.py:79, 84-86: the last simulation's path as [LongTensor[1]] on the MCTS device"""
        if self._latent_host is not None:
            self._latent = [torch.tensor([m], dtype=torch.long, device=self.dev) for m in self._latent_host]
            self._latent_host = None
        return self._latent

    @latent_actions.setter
    def latent_actions(self, value):
        self._latent = value
        self._latent_host = None

    def add_dirichlet_noise(self, prob, eps=0.25, alpha=0.25):
        """mcts.py:132-152 (host form, for callers that use it directly)."""
        if not isinstance(prob, np.ndarray) or prob.dtype not in (np.float32, np.float64):
            raise ValueError(f"Expect `prob` to be a numpy.array, got {prob}")
        noise = np.random.dirichlet(np.ones_like(prob) * alpha)
        return (1 - eps) * prob + eps * noise

    def generate_play_policy(self, visits_count, temperature):
        """mcts.py:154-176 (host form; the search kernel computes the same policy on device)."""
        if not 0.0 <= temperature <= 1.0:
            raise ValueError(f"Expect `temperature` to be in the range [0.0, 1.0], got {temperature}")
        visits_count = np.asarray(visits_count, dtype=np.int64)
        if temperature > 0.0:
            visits_count = np.power(visits_count, max(1.0, min(5.0, 1.0 / temperature)))
        return visits_count / np.sum(visits_count)

    # ------------------------------------------------------------------ batched form
    def run_batch(self, states, network, temperature, deterministic, *, legacy_rng=True, seed=None, minmax=None,
                  out=None):
        """B independent run_mcts calls in one kernel launch.

        states: [B, 3N] observations (numpy or tensor).  With legacy_rng the draws come from the
        global NumPy stream in the order B sequential run_mcts calls would consume them (each
        root with a fresh MinMaxStats, unless `minmax` [B,2] is given); otherwise a vectorised
        Generator(seed) is used.  Returns device tensors (visits, action, pi, root_q, minmax, ...).
        """
        S = int(self.n_simulations)
        obs = torch.as_tensor(states)
        B = obs.shape[0]
        if legacy_rng:
            noise, tie, u = _rng.predraw(B, deterministic=deterministic, alpha=self.root_dirichlet_alpha,
                                         eps=self.root_exploration_eps)
        else:
            noise, tie, u = _rng.synthetic_draws(B, deterministic=deterministic, alpha=self.root_dirichlet_alpha,
                                                 eps=self.root_exploration_eps, seed=seed or 0)
        eng = engine_for(network, S, B)
        dev = eng.device
        t = lambda a: None if a is None else torch.as_tensor(a).to(dev)
        return eng.search(S, obs=obs.to(dev, torch.float32), tie_idx=t(tie), noise=t(noise), action_u=t(u),
                          minmax_in=t(minmax), temperature=float(temperature), deterministic=bool(deterministic),
                          discount=float(self.discount), eps=float(self.root_exploration_eps),
                          np1_ucb=self.np1_ucb, out=out)
