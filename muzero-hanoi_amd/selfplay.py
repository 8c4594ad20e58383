"""Self-play / acting drivers on top of the search.

play_game          Muzero._play_game (Muzero.py:153-207) for one env through the drop-ins: the
                   reference's control flow, RNG consumption and episode bookkeeping, every search
                   and every env step on the GPU.
BatchedSelfPlay    B envs resident on the GPU (HanoiBatch) stepping with search-chosen actions.  Each env
                   is one agent with its own MCTS instance: its MinMaxStats (MCTS/mcts.py:23, never
                   reset) is carried from decision to decision (minmax_out -> minmax_in), starting from
                   the `minmax` handed in.  Every form runs on one lockstep move loop (_Lockstep: the
                   unfinished rows, their draws, the search with the MinMaxStats carry, the move's one
                   host read) and differs in what it does between a search and that read:
                   play            one mzh_search + one mzh_env_step_observe launch per move on the
                                   full-batch env arrays through env_index; records every move.
                   play_plans      the plan-ahead form (acting_experiments/planning_multiple_actions.py):
                                   a search's latent path executed open loop by one mzh_env_run_plan
                                   launch, the next search only for the envs whose plan ran out.
                   play_perturbed  searches on noisy / disc-permuted observations of the true envs.
                   play_probed     play plus one mzh_probe_actions launch per move (evaluate_legality).
episode_records    the reference's per-episode bookkeeping (returns, priorities,
                   organise_transitions) of every env of a BatchedSelfPlay run.
ingest_records     that bookkeeping, the success filter and Buffer.add for every env in one device call
                   (Buffer.add_episodes, csrc/mzh_ingest.hip): the same ring, priorities and RNG stream.
evaluate_networks  evaluate's batched schedule for a set of networks (an ablation sweep's variants): one batch
                   of len(networks) x episodes envs per budget, one mzh_search_multi launch per move.
evaluate           acting_ablations.get_results (acting_experiments/acting_ablations.py:72-128)
                   and illegal_move_rate (illegal_move_rate_comparison.py:27-50) over episodes:
                   error = steps - hanoi_solver(start), per-episode illegal-move rates (mean and
                   standard error).  sequential=True is the reference's own schedule -- one MCTS
                   instance, episodes one after another, the global NumPy stream -- and reproduces
                   get_results exactly; otherwise a budget's episodes run as one batch, each with
                   its own persistent MinMaxStats.  max_plan_len= scores plan-ahead episodes
                   (acting.plan_multiple_actions) in either schedule.

RNG: with legacy_rng the draws come from NumPy's global stream (rng.predraw) in the order the
reference consumes them when one env plays at a time (B = 1, or sequential=True); a batch of
B > 1 lockstep envs draws, per step, for its unfinished envs in env order -- a different
interleaving than B sequential episodes, so only the B = 1 forms are stream-identical.
"""
import numpy as np
import torch

from . import rng as _rng
from .engine import ACTIONS, LATENT, hanoi_solver_batch
from .env import HanoiBatch
from .mcts import RecordedNetwork, _replay_engine
from .networks import NetworkSet, engine_for, engine_for_set
from .utils import adjust_temperature, compute_MCreturns, compute_n_step_returns, organise_transitions

# acting_experiments/acting_ablations.py:49-68: the named 3-disk starts (distance to goal 7 / 3 / 1)
START_STATES = {"ES": (2, 2, 0), "MS": (0, 0, 2), "LS": (1, 2, 2)}


def state_index(state):
    """reference state tuple -> index into TowersOfHanoi.states (itertools.product order)"""
    idx = 0
    for s in state:
        idx = idx * 3 + int(s)
    return idx


def index_state(idx, n_disks):
    return tuple(int(idx // 3 ** (n_disks - 1 - d)) % 3 for d in range(n_disks))


def play_game(env, mcts, network, episode, deterministic=False, *, discount=0.8, TD_return=True, n_step=10,
              unroll_n_steps=5, n_action=6, temperature=None):
    """Muzero._play_game: returns (steps, states, rwds, actions, pi_probs, returns, priorities)."""
    episode_state, episode_action, episode_rwd, episode_piProb, episode_rootQ = [], [], [], [], []
    c_state = env.reset()
    done = False
    step = 0
    T = adjust_temperature(episode) if temperature is None else temperature
    # our MCTS + TowersOfHanoi: the decisions pipelined on the device (MCTS.play_episode), else the search and
    # the env step as chained launches with one synchronisation per decision (MCTS.run_mcts_step)
    ours = hasattr(env, "_launch_step")
    pipe = getattr(mcts, "play_episode", None) if ours else None
    r = pipe(env, network, T, deterministic) if pipe is not None and c_state is env.oneH_c_state else None
    if r is not None:
        step, episode_state, episode_action, episode_rwd, episode_piProb, episode_rootQ = r
        done = True
    chain = getattr(mcts, "run_mcts_step", None) if ours else None
    while not done:
        r = chain(c_state, network, T, deterministic, env) if chain is not None else None
        if r is not None:
            action, pi_prob, rootQ, (n_state, rwd, done, _) = r
        else:
            action, pi_prob, rootQ = mcts.run_mcts(c_state, network, temperature=T, deterministic=deterministic)
            n_state, rwd, done, _ = env.step(action)
        step += 1
        episode_state.append(c_state)
        episode_action.append(action)
        episode_rwd.append(rwd)
        episode_piProb.append(pi_prob)
        episode_rootQ.append(rootQ)
        c_state = n_state
    returns, priorities, trans = _bookkeeping(episode_state, episode_rwd, episode_action, episode_piProb,
                                              episode_rootQ, discount=discount, TD_return=TD_return, n_step=n_step,
                                              unroll_n_steps=unroll_n_steps, n_action=n_action)
    states, rwds, actions, pi_probs, returns = trans
    return step, states, rwds, actions, pi_probs, returns, priorities


def _bookkeeping(episode_state, episode_rwd, episode_action, episode_piProb, episode_rootQ, *, discount, TD_return,
                 n_step, unroll_n_steps, n_action):
    """Muzero.py:188-205: returns (n-step TD or Monte Carlo), priorities |return - root Q| in fp32,
    and the unroll targets (organise_transitions draws one np.random.randint)."""
    if TD_return:
        episode_returns = compute_n_step_returns(episode_rwd, episode_rootQ, n_step, discount)
    else:
        episode_returns = compute_MCreturns(episode_rwd, discount)
    priorities = np.abs(np.array(episode_returns, dtype=np.float32) - np.array(episode_rootQ, dtype=np.float32))
    trans = organise_transitions(episode_state, episode_rwd, episode_action, episode_piProb, episode_returns,
                                 unroll_n_steps, n_action)
    return episode_returns, priorities, trans


class _Lockstep:
    """One lockstep run of a BatchedSelfPlay: B envs reset to their starts, one agent (MinMaxStats) each, and
    the rows that are still playing.  A form of play is a loop body on it:

        run = _Lockstep(sp, start_idx, ...)
        while run.n:
            out = run.search()      # the rows run.idx, their MinMaxStats carried in run.mm
            ...                     # act on run.env through env_index=run.idx32
            run.advance(kernel)     # the move's one host read; the next run.idx / run.n

    eng: the engine; env: the HanoiBatch, its last_obs the starts' observations; mm [B, 2]; net_index [B] int32 on
    the device with a NetworkSet, else None; sims [B] int32 on the device (each row's own simulation budget, at most
    sp.S; a NetworkSet only) or None; start [B] int64 on the device; idx (int64) / idx32 / n: the
    unfinished rows in env order and their count; draw_index [B] on the device or None (rows)."""

    def __init__(self, sp, start_idx, minmax, seed, net_index, temperature, deterministic, legacy_rng=False,
                 draw_index=None, sims=None):
        start = torch.as_tensor(np.asarray(start_idx), dtype=torch.int64).reshape(-1)
        B = int(start.shape[0])
        if sims is not None:  # checked before any device work
            sims = np.asarray(sims)
            if not isinstance(sp.network, NetworkSet):
                raise ValueError("sims [B] needs a NetworkSet: only the multi-network search takes a budget per root")
            if sims.dtype.kind not in "iu" or sims.shape != (B,) or (B and (sims.min() < 0 or sims.max() > sp.S)):
                raise ValueError(f"sims must be {B} integer budgets in [0, {sp.S}], the play's n_simulations")
        self.sp, self.temperature, self.deterministic, self.legacy_rng = sp, temperature, deterministic, legacy_rng
        self.replay = isinstance(sp.network, RecordedNetwork)
        if self.replay and B != 1:
            raise ValueError("a RecordedNetwork replays one sequential stream of searches: B must be 1")
        multi = isinstance(sp.network, NetworkSet)
        if multi != (net_index is not None):
            raise ValueError("net_index [B] is required with a NetworkSet and only accepted with one")
        if multi:
            ni = np.asarray(net_index, np.int64).reshape(-1)
            if ni.shape[0] != B or (B and (ni.min() < 0 or ni.max() >= len(sp.network) or np.any(np.diff(ni) < 0))):
                raise ValueError(f"net_index must be {B} non-decreasing indices into the set of {len(sp.network)}")
            self.eng = engine_for_set(sp.network, sp.S, B)
        else:
            self.eng = _replay_engine(sp.N, sp.S) if self.replay else engine_for(sp.network, sp.S, B)
        dev = self.eng.device
        self.net_index = torch.as_tensor(ni, dtype=torch.int32).to(dev) if multi else None
        # the budgets of the rows still playing are a subsequence of these: dropping rows never adds a run
        self.sims, self.max_runs = None, None
        if sims is not None:
            self.sims = torch.as_tensor(sims.astype(np.int32)).to(dev)
            self.max_runs = 1 + int(np.count_nonzero((np.diff(ni) != 0) | (np.diff(sims) != 0)))
        # with the legacy stream a move's draws are those of its unfinished rows in env order, whatever draw_index
        self.draw_index, self.n_draw = None, B
        if draw_index is not None and not legacy_rng:
            di = np.asarray(draw_index, np.int64).reshape(-1)
            if di.shape[0] != B or di.min() < 0:
                raise ValueError(f"draw_index must be {B} non-negative rows")
            self.draw_index, self.n_draw = torch.from_numpy(di).to(dev), int(di.max()) + 1
        self.env = HanoiBatch(sp.N, sp.max_steps, B, goal_peg=sp.goal_peg, device=dev)
        self.start = start.to(dev)
        self.env.reset(self.start)
        self.env._tallies()  # the first observations (env.last_obs) and the per-env counts
        self.mm = torch.empty((B, 2), dtype=torch.float64, device=dev)
        if minmax is None:
            self.mm[:, 0], self.mm[:, 1] = -float("inf"), float("inf")
        else:
            self.mm.copy_(torch.as_tensor(np.asarray(minmax, np.float64)).reshape(B, 2))
        self.gen = np.random.default_rng(seed)  # of the synthetic draws' seeds
        self._pre = None
        self._unfinished(torch.arange(B, device=dev))

    def _unfinished(self, idx):
        self.idx, self.idx32, self.n = idx, idx.to(torch.int32), int(idx.shape[0])
        if self.draw_index is None:
            self.n_draw = self.n

    def _draw(self):
        """a move's draws, n_draw rows: the global NumPy stream, or synthetic ones seeded from gen"""
        kw = dict(deterministic=self.deterministic, alpha=self.sp.alpha, eps=self.sp.eps)
        if self.legacy_rng:
            return _rng.predraw(self.n_draw, **kw)
        return _rng.synthetic_draws(self.n_draw, seed=int(self.gen.integers(2**31)), **kw)

    def rows(self, x):
        """the rows of a draw x (None passes through) for the rows idx, on their device: the first n, or, with
        draw_index, x[draw_index[idx]] of a draw of max(draw_index) + 1 rows"""
        if x is None:
            return None
        x = torch.as_tensor(x).to(self.idx.device)
        return x[:self.n] if self.draw_index is None else x.index_select(0, self.draw_index.index_select(0, self.idx))

    def search(self):
        """one search over the rows idx from env.last_obs (a RecordedNetwork: its next recorded call), their
        MinMaxStats read from and carried into mm.  Returns the search's dict, plus obs: the rows searched."""
        sp, idx = self.sp, self.idx
        draws, self._pre = self._draw() if self._pre is None else self._pre, None
        noise, tie, u = (self.rows(x) for x in draws)
        obs = self.env.last_obs.index_select(0, idx)
        kw = dict(tie_idx=tie, noise=noise, action_u=u, minmax_in=self.mm.index_select(0, idx),
                  temperature=float(self.temperature), deterministic=bool(self.deterministic), discount=sp.discount,
                  eps=sp.eps, np1_ucb=sp.np1_ucb)
        if self.net_index is not None:  # a NetworkSet: idx is increasing, so the networks' envs stay consecutive
            if self.sims is not None:  # sp.S is the largest budget; the rows keep theirs as they keep their network
                kw.update(sims=self.sims.index_select(0, idx), max_runs=self.max_runs)
            out = self.eng.search_multi(sp.S, net_index=self.net_index.index_select(0, idx), obs=obs, **kw)
        elif self.replay:
            out = self.eng.search(sp.S, replay=sp.network.next_replay(self.eng.device), **kw)
        else:
            out = self.eng.search(sp.S, obs=obs, **kw)
        self.mm.index_copy_(0, idx, out["minmax"])
        out["obs"] = obs
        return out

    def advance(self, kernel, **extra_err):
        """The move's single host read: the unfinished envs left, env.err (the errors `kernel`, the move's env
        launch, counted) and extra_err (kernel name = its [1] int32 error counter).  RuntimeError naming the
        kernel if a counter is not zero.  Sets the next idx / n.
        Synthetic draws: the next move's are made here, on the host while the GPU still runs this move, for this
        move's count of rows (an upper bound); `rows` cuts them to the count left (the draws of n rows are the
        first n rows of a larger draw, rng.synthetic_draws).  Legacy-stream draws wait for the count."""
        if not self.legacy_rng and not self.replay:
            self._pre = self._draw()
        errs = {kernel: self.env.err, **extra_err}
        left, *counts = (int(x) for x in torch.stack([self.env.active.sum(dtype=torch.int32)]
                                                     + [e[0] for e in errs.values()]).cpu())
        bad = [f"{k} reported {c} error(s)" for k, c in zip(errs, counts) if c]
        if bad:
            raise RuntimeError("; ".join(bad))
        # the unfinished envs in env order, without another host read (their count is known)
        self._unfinished(torch.sort(self.env.active, descending=True, stable=True).indices[:left])


class BatchedSelfPlay:
    """B independent agents in lockstep on one GPU, one MCTS instance (MinMaxStats) each.

    network: one network for every agent, or a networks.NetworkSet -- then play / play_plans / play_episodes take
    net_index [B] (non-decreasing: the agents of one network are consecutive) and agent b searches under
    network[net_index[b]], all of them in one mzh_search_multi launch per move (play_episodes: in its one
    mzh_play_episodes_multi launch)."""

    def __init__(self, network, n_disks, max_steps, n_simulations, *, discount=0.8, dirichlet_alpha=0.25,
                 root_exploration_eps=0.25, goal_peg=2, np1_ucb=False):
        self.network = network
        self.N, self.max_steps, self.S = n_disks, max_steps, n_simulations
        self.discount, self.alpha, self.eps, self.goal_peg = discount, dirichlet_alpha, root_exploration_eps, goal_peg
        self.np1_ucb = np1_ucb

    def play(self, start_idx, temperature=1.0, deterministic=False, seed=0, legacy_rng=False, minmax=None,
             record_obs=False, net_index=None, sims=None, draw_index=None):
        """Play every env from start_idx[b] until done (goal or max_steps).

        minmax: [B, 2] (maximum, minimum) of each agent's MinMaxStats at the start (default: fresh,
        -inf / +inf); the final values come back as res["minmax"].  net_index: [B] with a NetworkSet (the
        class docstring), else None.  sims: [B] integers with a NetworkSet, env b searches sims[b] simulations per
        move (each in [0, n_simulations], any order inside a network; mzh_search_multi_budget), else None: every env
        n_simulations.  draw_index [B]: as in play_perturbed.  Per move: one search over the unfinished envs, one mzh_env_step_observe
        launch through env_index, one host read (_Lockstep.advance).  Returns device tensors:
        per step t (rows of envs that were still playing): action, reward, pi, root_q, active,
        obs (record_obs: the observation searched); per env: steps, illegal (count), start_idx, minmax.
        An empty start_idx plays nothing: no launch, empty records.  RuntimeError if the env kernel counted an
        error, which a search's own actions cannot cause."""
        run = _Lockstep(self, start_idx, minmax, seed, net_index, temperature, deterministic, legacy_rng, draw_index,
                        sims)
        env, B, dev = run.env, run.env.B, run.eng.device
        rec = dict(action=[], reward=[], pi=[], root_q=[], active=[])
        if record_obs:
            rec["obs"] = []
        while run.n:
            idx = run.idx
            out = run.search()
            r = env.step_observe(out["action"], run.idx32)
            full = lambda v, fill, dt: torch.full((B,) + tuple(v.shape[1:]), fill, dtype=dt, device=dev).index_copy(
                0, idx, v.to(dt))
            rec["action"].append(full(out["action"], -1, torch.int32))
            rec["reward"].append(full(HanoiBatch.reward_value(r["reward"]), 0.0, torch.float64))
            rec["pi"].append(full(out["pi"], 0.0, torch.float64))
            rec["root_q"].append(full(out["root_q"], 0.0, torch.float64))
            rec["active"].append(torch.zeros(B, dtype=torch.bool, device=dev).index_fill(0, idx, True))
            if record_obs:
                rec["obs"].append(full(out["obs"], 0.0, torch.float32))
            run.advance("mzh_env_step_observe (an action outside 0..5)")
        res = {k: torch.stack(v) if v else torch.empty(0, device=dev) for k, v in rec.items()}
        return dict(res, steps=env.steps_total, illegal=env.illegal_total, start_idx=run.start, minmax=run.mm)

    def play_episodes(self, start_idx, temperature=1.0, deterministic=False, seed=0, legacy_rng=False, minmax=None,
                      draws=None, net_index=None, weights="auto", sims=None, discounts=None):
        """`play(record_obs=True)` as ONE launch (Engine.play_episodes, mzh_play_episodes): a workgroup of the
        latency kernel takes an env and plays it to its end -- search, action draw, env step and record -- without
        returning to the host.  A live network or, with net_index [B] (the class docstring), a NetworkSet whose
        envs all play in that one launch (mzh_play_episodes_multi), each as under its network alone; no
        RecordedNetwork.  Returns the dict
        play(record_obs=True) returns: the same keys, dtypes, shapes and fill values (action -1 and everything
        else 0 at rows past an episode's end, reward as float64 through HanoiBatch.reward_value, active derived
        from steps), the record trimmed to max(steps) rows -- the call's one host read.

        Draw schedule: the draws are a table of max_steps x B rows, and env b takes row b of move t's draws at
        every move, whichever envs are still playing.  At B = 1 that is play's schedule; at B > 1 it differs
        (play gives row j of a move's draws to the j-th unfinished env).
        draws = (noise [T, B, 6] float64, tie [T, B] int32, u [T, B] float64), T = max_steps: an explicit table
        (arrays or tensors; noise None exactly when the searches take no root noise, rng.uses_noise, and u None
        exactly when deterministic).  draws = None: one vectorised draw of the whole table,
        rng.synthetic_draws(T * B, seed=seed) reshaped -- three child streams of `seed`, not play's per-move
        seeds (200 per-move generator constructions would cost as much as the launch).
        legacy_rng = True (B = 1 only, without draws): the table is rng.predraw(T) from NumPy's global stream;
        after the launch the stream is put back and advanced by rng.predraw(steps), so it is left exactly
        where play(legacy_rng=True) leaves it.
        weights: how a NetworkSet's engine picks up changed parameters (networks.engine_for_set).
        sims [B] integers / discounts [B] floats, with a NetworkSet only: env b searches sims[b] simulations per move
        (each in [0, n_simulations]; None: n_simulations) under discounts[b] (None: the play's discount), all envs
        still in the one launch (mzh_play_episodes_sweep), each as a lone play of its network with that budget and
        discount.  Both None: the launches above.
        RuntimeError if the kernel refused a start state (a peg outside 0..2: not reachable from start_idx)."""
        start = np.asarray(start_idx, np.int64).reshape(-1)
        B, T = int(start.shape[0]), int(self.max_steps)
        kw = dict(deterministic=deterministic, alpha=self.alpha, eps=self.eps)
        if isinstance(self.network, RecordedNetwork):
            raise ValueError("play_episodes: live networks only (no RecordedNetwork)")
        multi = isinstance(self.network, NetworkSet)
        if (sims is not None or discounts is not None) and not multi:  # checked before any device work
            raise ValueError("play_episodes: sims / discounts [B] need a NetworkSet: only the episodes of a network "
                             "set take a budget and a discount per env")
        if multi != (net_index is not None):
            raise ValueError("play_episodes: net_index [B] is required with a NetworkSet and only accepted with one")
        if sims is not None:
            sims = np.asarray(sims)
            if sims.dtype.kind not in "iu" or sims.shape != (B,) or (B and (sims.min() < 0 or sims.max() > self.S)):
                raise ValueError(f"play_episodes: sims must be {B} integer budgets in [0, {self.S}], the play's "
                                 "n_simulations")
        if discounts is not None:
            discounts = np.asarray(discounts, np.float64)
            if discounts.shape != (B,):
                raise ValueError(f"play_episodes: discounts must be {B} floats, got shape {discounts.shape}")
        if multi:
            ni = np.asarray(net_index, np.int64).reshape(-1)
            if ni.shape[0] != B or (B and (ni.min() < 0 or ni.max() >= len(self.network) or np.any(np.diff(ni) < 0))):
                raise ValueError(f"play_episodes: net_index must be {B} non-decreasing indices into the set of "
                                 f"{len(self.network)}")
        if legacy_rng and (B != 1 or draws is not None):
            raise ValueError("play_episodes: legacy_rng=True is the one-env schedule: it needs B = 1 and draws=None, "
                             f"got B = {B}")
        if T < 1:
            raise ValueError(f"play_episodes: max_steps must be >= 1, got {T}")
        if draws is not None:
            draws = _episode_draws(draws, T, B, _rng.uses_noise(**kw), not deterministic)
        if B == 0:  # nothing to play and (a checked [T, 0] table) nothing to draw: play's empty records
            return self.play(start, temperature, deterministic, seed, legacy_rng, minmax, record_obs=True,
                             net_index=net_index)
        state0 = None
        if draws is None:  # one flat draw of T * B rows, row t * B + b for move t of env b
            if legacy_rng:
                state0 = np.random.get_state()
            flat = _rng.predraw(T, **kw) if legacy_rng else _rng.synthetic_draws(T * B, seed=seed, **kw)
            draws = tuple(None if x is None else torch.from_numpy(x).reshape((T, B) + x.shape[1:]) for x in flat)
        t_max = 0
        try:
            out = self._launch_episodes(start, draws, minmax, temperature, deterministic, ni if multi else None,
                                        weights, sims, discounts)
            steps = out["steps"]
            t_max, n_err = (int(x) for x in torch.stack([steps.max(), out["err"][0]]).cpu())  # the one host read
        finally:
            if state0 is not None:  # the stream as the moves played leave it (none, if the call failed)
                np.random.set_state(state0)
                _rng.predraw(t_max, **kw)
        if n_err:
            raise RuntimeError(f"mzh_play_episodes refused {n_err} start state(s)")
        return episodes_result(out, start, t_max)

    def _launch_episodes(self, start, draws, minmax, temperature, deterministic, net_index, weights="auto", sims=None,
                         discounts=None):
        """play_episodes' launch, without its host read: Engine.play_episodes' dict for the starts `start` (int64
        array [B]) on the checked table `draws`; net_index: an int64 array [B] with a NetworkSet, else None; sims /
        discounts: checked arrays [B] (a NetworkSet only) or None"""
        B, T = int(start.shape[0]), int(self.max_steps)
        multi = net_index is not None
        eng = engine_for_set(self.network, self.S, B, weights=weights) if multi else engine_for(self.network, self.S, B)
        dev = eng.device
        noise, tie, u = (None if x is None else x.to(dev) for x in draws)
        pw = 3 ** np.arange(self.N - 1, -1, -1, dtype=np.int64)
        state = torch.from_numpy(((start[:, None] // pw) % 3).astype(np.uint8)).to(dev)
        mm = None if minmax is None else torch.as_tensor(np.asarray(minmax, np.float64)).reshape(B, 2).to(dev)
        return eng.play_episodes(self.S, state, T, tie_idx=tie, noise=noise, action_u=u, minmax_in=mm,
                                 goal_peg=self.goal_peg, temperature=float(temperature),
                                 deterministic=bool(deterministic), discount=self.discount, eps=self.eps,
                                 np1_ucb=self.np1_ucb, record_obs=True,
                                 net_index=torch.from_numpy(net_index.astype(np.int32)) if multi else None,
                                 sims=None if sims is None else torch.from_numpy(
                                     np.asarray(sims).astype(np.int32)).to(dev),
                                 discounts=None if discounts is None else torch.from_numpy(
                                     np.asarray(discounts, np.float64)).to(dev))

    def play_plans(self, start_idx, max_plan_len, temperature=1.0, deterministic=False, seed=0, legacy_rng=False,
                   minmax=None, net_index=None, sims=None):
        """Plan-ahead episodes (acting_experiments/planning_multiple_actions.py:111-183): every env searches
        once and executes the last simulation's selection path (mcts.return_latent_actions()[:max_plan_len])
        open loop, illegal moves included, and searches again only when that plan ran out before the episode
        ended (goal or max_steps; the rest of a plan is dropped).  The search's `action` is drawn as in `play`
        (the same draws and per-agent MinMaxStats carry) but not executed.

        Per round: one search over the unfinished envs, one mzh_env_run_plan launch reading the search's
        latent / latent_len where it left them and the envs' full-batch arrays through env_index, and one
        host read (unfinished envs left, error count).  Returns device tensors: per env steps, illegal
        (executed illegal moves), plans (searches), start_idx, minmax; per round r: action [R][L][B]
        (executed moves, -1 where nothing ran), reward [R][L][B] (int8 codes of mzh_env_step, 0 where nothing
        ran), root_q [R][B] and search_action [R][B] (0 / -1 for envs without a search that round).
        sims: as in play (a budget per env), each >= 1."""
        L = int(max_plan_len)
        if L < 1:
            raise ValueError(f"play_plans: max_plan_len must be >= 1, got {max_plan_len}")
        if self.S < 1:  # the reference would execute the previous search's path (mcts.py:79 is never reached)
            raise ValueError("play_plans: a plan needs n_simulations >= 1")
        if np.asarray(start_idx).size < 1:
            raise ValueError("play_plans: no start states")
        if sims is not None and np.asarray(sims).size and np.asarray(sims).min() < 1:
            raise ValueError("play_plans: a plan needs a budget >= 1 for every env")
        run = _Lockstep(self, start_idx, minmax, seed, net_index, temperature, deterministic, legacy_rng, sims=sims)
        env, B, dev = run.env, run.env.B, run.eng.device
        plans = torch.zeros(B, dtype=torch.int32, device=dev)
        rec = dict(action=[], reward=[], root_q=[], search_action=[])
        while run.n:
            idx = run.idx
            out = run.search()
            # a path has at most S + 1 moves (the row stride of `latent`): a longer max_plan_len cuts nothing more
            r = env.run_plan(out["latent"], out["latent_len"], min(L, self.S + 1), env_index=run.idx32, record=True)
            plans.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
            full = lambda v, fill: torch.full(tuple(v.shape[:-1]) + (B,), fill, dtype=v.dtype, device=dev).index_copy(
                v.dim() - 1, idx, v)
            pad = lambda v, fill: v if v.shape[0] == L else torch.cat(
                [v, torch.full((L - v.shape[0], B), fill, dtype=v.dtype, device=dev)])
            rec["action"].append(pad(full(r["action"], -1), -1))
            rec["reward"].append(pad(full(r["reward"], 0), 0))
            rec["root_q"].append(full(out["root_q"], 0.0))
            rec["search_action"].append(full(out["action"], -1))
            run.advance("mzh_env_run_plan (a search returned an empty path or an action outside 0..5)")
        res = {k: torch.stack(v) for k, v in rec.items()}
        return dict(res, steps=env.steps_total, illegal=env.illegal_total, plans=plans, start_idx=run.start,
                    minmax=run.mm)

    def play_perturbed(self, start_idx, *, noise_std=None, permute_disc=None, temperature=0.0, deterministic=True,
                       seed=0, minmax=None, net_index=None, draw_index=None):
        """Episodes on perturbed observations (noise_injection_comparison.py:17-37, permutation_importance.py:27-76):
        every agent searches from an observation that differs from its env's true state -- Gaussian noise of
        standard deviation noise_std added to the one-hot encoding, and / or disc permute_disc's peg replaced by
        a fresh random peg at every decision -- the chosen action is applied to the true env, and the episode is
        solved if a step returned reward 100 (else it ends at max_steps).  noise_std / permute_disc: None, a
        scalar, or [B] (None / 0 and None / -1: that env is not perturbed), so one batch mixes conditions.
        The defaults are the scripts' `temperature=0, deterministic=True` searches.

        Per move: one search over the unfinished envs (as in `play`: the same synthetic draws from the same
        generator in the same order, the same per-agent MinMaxStats carry), one mzh_env_step_observe launch
        through env_index that steps the true envs and writes the next perturbed observations, and one host read
        (unfinished envs left, error count).  The perturbation draws of decision t (0: the first observation)
        are rng.perturbation_draws(rows, 3N, seed_t) with seed_t the t-th int(g.integers(2**31)) of
        g = rng.perturbation_seeds(seed): row j of them serves the j-th env that was unfinished before move
        t - 1 (every env at t = 0), noise = std[env] * z[j].  Without any perturbation the result equals play's.
        draw_index [B] (optional): env b takes row draw_index[b] of every draw, search draws included, instead
        of the row of its rank among the unfinished envs -- then an env's episode does not depend on which other
        envs share its batch (evaluate_perturbed plays one batch in slices with it).
        Returns device tensors per env: steps, illegal, solved (uint8), start_idx, minmax."""
        if isinstance(self.network, RecordedNetwork):
            raise ValueError("play_perturbed: a RecordedNetwork replays recorded observations; use the acting drop-ins")
        if np.asarray(start_idx).size < 1:
            raise ValueError("play_perturbed: no start states")
        run = _Lockstep(self, start_idx, minmax, seed, net_index, temperature, deterministic, draw_index=draw_index)
        env, dev = run.env, run.eng.device
        std, disc = perturbation_arrays(env.B, self.N, noise_std, permute_disc)
        pgen = _rng.perturbation_seeds(seed)
        std_dev = None if std is None else torch.from_numpy(std).to(dev)[:, None]
        env.set_perturbation(disc)

        def perturbation():
            if std is None and disc is None:
                return None, None
            peg, z = _rng.perturbation_draws(run.n_draw, 3 * self.N, int(pgen.integers(2**31)))
            peg = None if disc is None else run.rows(peg).contiguous()
            noise = None if std is None else (std_dev.index_select(0, run.idx) * run.rows(z)).contiguous()
            return peg, noise

        peg, noise = perturbation()
        env.step_observe(None, perm_peg=peg, noise=noise)  # the first observations, perturbed
        while run.n:
            out = run.search()
            peg, noise = perturbation()
            env.step_observe(out["action"], run.idx32, perm_peg=peg, noise=noise)
            run.advance("mzh_env_step_observe (an action outside 0..5 or a perturbation outside its range)")
        return dict(steps=env.steps_total, illegal=env.illegal_total, solved=env.solved, start_idx=run.start,
                    minmax=run.mm)

    def play_probed(self, start_idx, *, seed=0, legacy_rng=False, net_index=None, draw_index=None):
        """evaluate_legality's episodes: `play` at temperature 0.0, deterministic=False, every agent fresh, with
        one mzh_probe_actions launch per move on the rows that are searched, into slot t of a device record of
        max_steps slots.  draw_index: as in play_perturbed (not used with legacy_rng, which draws for the
        unfinished rows in env order).  Returns device tensors: reward / value [T][B][6] float32 and legal [T][B]
        uint8 (zeros after an episode's end), action [T][B] int32 (-1 after it), T the moves played, and
        steps [B]."""
        run = _Lockstep(self, start_idx, None, seed, net_index, 0.0, False, legacy_rng, draw_index)
        env, B, dev, T = run.env, run.env.B, run.eng.device, self.max_steps
        rec_r = torch.zeros((T, B, 6), dtype=torch.float32, device=dev)
        rec_v = torch.zeros((T, B, 6), dtype=torch.float32, device=dev)
        rec_l = torch.zeros((T, B), dtype=torch.uint8, device=dev)
        rec_a = torch.full((T, B), -1, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        t = 0
        while run.n:
            out = run.search()
            run.eng.probe_actions(env.last_obs, env_index=run.idx32, state=env.state, err=err,
                                  net_index=None if run.net_index is None else run.net_index.index_select(0, run.idx),
                                  out=dict(reward=rec_r[t], value=rec_v[t], legal=rec_l[t]))
            rec_a[t].index_copy_(0, run.idx, out["action"])
            env.step_observe(out["action"], run.idx32)
            run.advance("mzh_env_step_observe", mzh_probe_actions=err)
            t += 1
        return dict(reward=rec_r[:t], value=rec_v[:t], legal=rec_l[:t], action=rec_a[:t], steps=env.steps_total)


def episodes_result(out, start, t_max, cols=slice(None)):
    """play(record_obs=True)'s dict from Engine.play_episodes' `out` for the envs `cols` (a slice of the batch; start:
    their start indices, an int64 array), the record trimmed to t_max >= max(steps[cols]) rows"""
    dev = out["steps"].device
    steps = out["steps"][cols]
    active = torch.arange(t_max, device=dev)[:, None] < steps[None, :]
    return dict(action=out["action"][:t_max, cols], reward=HanoiBatch.reward_value(out["reward"][:t_max, cols]),
                pi=out["pi"][:t_max, cols], root_q=out["root_q"][:t_max, cols], active=active,
                obs=out["obs"][:t_max, cols], steps=steps, illegal=out["illegal"][cols],
                start_idx=torch.from_numpy(np.asarray(start, np.int64)).to(dev), minmax=out["minmax"][cols])


def _episode_draws(draws, T, B, noisy, stochastic):
    """play_episodes' explicit draw table, checked on the host: (noise, tie, u) -> tensors noise [T, B, 6] float64
    (None exactly when not noisy), tie [T, B] int32, u [T, B] float64 (None exactly when not stochastic).
    ValueError for anything else: a wrong shape or dtype is not converted."""
    if not isinstance(draws, (tuple, list)) or len(draws) != 3:
        raise ValueError("play_episodes: draws must be (noise, tie, u)")
    out = []
    for name, x, dt, shape, want in (("noise", draws[0], torch.float64, (T, B, ACTIONS), noisy),
                                     ("tie", draws[1], torch.int32, (T, B), True),
                                     ("u", draws[2], torch.float64, (T, B), stochastic)):
        if (x is not None) != want:
            raise ValueError(f"play_episodes: draws' {name} must be {'given' if want else 'None'} for these searches")
        if x is not None:
            x = torch.as_tensor(x)
            if x.dtype != dt or tuple(x.shape) != shape:
                raise ValueError(f"play_episodes: draws' {name} must be {dt} {shape}, got {x.dtype} {tuple(x.shape)}")
        out.append(x)
    return tuple(out)


def perturbation_arrays(B, n_disks, noise_std, permute_disc):
    """play_perturbed's per-env conditions, checked on the host: noise_std (None | scalar | [B]) -> float64 [B]
    or None where no env has noise; permute_disc (None | scalar | [B], None / -1 = no disc) -> int32 [B] or None
    where no env has one.  ValueError for a std < 0 (or NaN) and a disc outside [-1, n_disks)."""
    std = disc = None
    if noise_std is not None:
        std = np.asarray(noise_std, np.float64).reshape(-1)
        std = np.full(B, std[0]) if std.size == 1 else std
        if std.shape[0] != B or not np.all(std >= 0):
            raise ValueError(f"noise_std must be a scalar or [{B}] of values >= 0, got {noise_std!r}")
        std = std if np.any(std > 0) else None
    if permute_disc is not None:
        pd = np.asarray([-1 if d is None else d for d in np.asarray(permute_disc, object).reshape(-1)])
        if np.any(pd != pd.astype(np.int64)):
            raise ValueError(f"permute_disc must hold integers, got {permute_disc!r}")
        pd = pd.astype(np.int32)
        pd = np.full(B, pd[0], np.int32) if pd.size == 1 else pd
        if pd.shape[0] != B or pd.min() < -1 or pd.max() >= n_disks:
            raise ValueError(f"permute_disc must be a scalar or [{B}] of discs in [0, {n_disks}) (None / -1: none), "
                             f"got {permute_disc!r}")
        disc = pd if np.any(pd >= 0) else None
    return std, disc


def episode_records(res, *, discount=0.8, TD_return=True, n_step=10, unroll_n_steps=5, n_action=6):
    """Muzero._play_game's return value for every env of a BatchedSelfPlay.play(record_obs=True)
    result, in env order: (steps, states, rwds, actions, pi_probs, returns, priorities)."""
    host = {k: res[k].cpu().numpy() for k in ("action", "reward", "pi", "root_q", "active", "obs", "steps")}
    out = []
    for b in range(host["steps"].shape[0]):
        T = int(host["steps"][b])
        states = [host["obs"][t, b].astype(np.float64) for t in range(T)]
        rwds = [_reward_py(host["reward"][t, b]) for t in range(T)]
        actions = [int(host["action"][t, b]) for t in range(T)]
        pis = [host["pi"][t, b] for t in range(T)]
        rootq = [float(host["root_q"][t, b]) for t in range(T)]
        _, priorities, trans = _bookkeeping(states, rwds, actions, pis, rootq, discount=discount, TD_return=TD_return,
                                            n_step=n_step, unroll_n_steps=unroll_n_steps, n_action=n_action)
        out.append((T,) + tuple(trans[:4]) + (trans[4], priorities))
    return out


def ingest_records(res, buffer, *, discount=0.8, n_step=10, unroll_n_steps=5, n_action=6):
    """episode_records + the `returns[-1, 0] > 0` filter + Buffer.add for every env of a
    BatchedSelfPlay.play(record_obs=True) result, on the device (n-step TD returns only).  The padding
    actions are organise_transitions' draws: one np.random.randint(0, n_action) per env in env order,
    successful or not -- drawn as one array, which yields the same values and leaves the legacy stream
    where the scalar calls leave it.  Returns the per-env step counts as a host array."""
    if unroll_n_steps != buffer.unroll_n_steps or n_action != buffer.n_action:
        raise ValueError("ingest_records: unroll_n_steps / n_action differ from the buffer's")
    B = int(res["steps"].shape[0])
    pad_action = np.random.randint(0, n_action, size=B)
    buffer.add_episodes(res, discount=discount, n_step=n_step, pad_action=pad_action)
    return res["steps"].cpu().numpy()


def _reward_py(r):
    """the reference's Python reward objects (env/hanoi.py:60-72: int 0 / 100 or float -0.1)"""
    r = float(r)
    return 0 if r == 0.0 else (100 if r == 100.0 else r)


# ------------------------------------------------------------------------------------------------
# evaluation (acting_ablations.get_results, illegal_move_rate_comparison.illegal_move_rate)
# ------------------------------------------------------------------------------------------------
def _start_index(start, n_disks):
    if start in START_STATES:
        if n_disks != 3:
            raise ValueError("the ES / MS / LS starts are 3-disk states (acting_ablations.py:49-68)")
        return state_index(START_STATES[start])
    return int(start)


def _random_start(n_disks, goal_peg):
    """TowersOfHanoi.random_reset's draw loop (env/hanoi.py:103-109) on the global NumPy stream"""
    goal = state_index((goal_peg,) * n_disks)
    while True:
        i = np.random.randint(3 ** n_disks)
        if i != goal:
            return i


def evaluate(network, n_disks, n_sims_range, *, episodes=1, start=None, start_idx=None, max_steps=200,
             temperature=1.0, deterministic=False, sequential=False, legacy_rng=None, seed=0, goal_peg=2, minmax=None,
             np1_ucb=False, max_plan_len=None, dirichlet_alpha=0.25):
    """Episodes per simulation budget, scored like the reference's acting scripts.

    start: None -> random_reset starts (env/hanoi.py:103-109); "ES" / "MS" / "LS" or a state index
    -> that fixed start (acting_ablations.py:49-68); start_idx: explicit per-episode start indices.
    sequential: one MCTS instance for every episode and budget (its MinMaxStats carried across all
    of them, `minmax` its initial value), episodes one after another, draws (random starts
    included) from the global NumPy stream -- get_results' schedule.  Otherwise each budget's
    episodes run as one batch, each episode its own agent with a fresh MinMaxStats.
    Returns dict(data=[[n, mean error]] (get_results' value), illegal=[[n, mean rate, std error]]
    (illegal_move_rate's value per budget), errors / steps / illegal_rates per budget, minmax).
    minmax (in and out) is the carried chain of the sequential schedule only: with
    sequential=False every agent starts fresh, `minmax` must be None and None is returned.
    max_plan_len: None -> a search per step (get_results); an integer L >= 1 -> plan-ahead episodes
    (planning_multiple_actions.py:111-183, BatchedSelfPlay.play_plans): a search's latent path, cut to L
    moves, is executed open loop and the next search runs only when it ran out; every budget must be >= 1.
    `illegal` then counts the executed illegal moves.
    dirichlet_alpha: the agents' root_dirichlet_alpha (0: no root noise, the plan-ahead script's setting)."""
    _check_plan("evaluate", max_plan_len, n_sims_range)
    if not sequential and minmax is not None:
        raise ValueError("evaluate: minmax applies to the sequential schedule only (batched agents start fresh)")
    legacy_rng = sequential if legacy_rng is None else legacy_rng
    score = _new_score()
    mm = None if minmax is None else np.asarray(minmax, np.float64).reshape(1, 2)
    for n in n_sims_range:
        sp = BatchedSelfPlay(network, n_disks, max_steps, int(n), goal_peg=goal_peg, np1_ucb=np1_ucb,
                             dirichlet_alpha=dirichlet_alpha)
        play = sp.play if max_plan_len is None else (lambda s, **kw: sp.play_plans(s, int(max_plan_len), **kw))
        if sequential:
            steps, ill, starts = [], [], []
            for ep in range(episodes):
                if start_idx is not None:
                    s0 = int(np.asarray(start_idx).reshape(-1)[ep])
                elif start is None:
                    s0 = _random_start(n_disks, goal_peg)
                else:
                    s0 = _start_index(start, n_disks)
                res = play([s0], temperature=temperature, deterministic=deterministic, legacy_rng=legacy_rng,
                           minmax=mm, seed=seed + ep)
                mm = res["minmax"].cpu().numpy()
                steps.append(int(res["steps"][0]))
                ill.append(int(res["illegal"][0]))
                starts.append(s0)
            steps, ill, starts = np.array(steps), np.array(ill), np.array(starts)
        else:
            starts = _batch_starts(n_disks, episodes, start, start_idx, seed, goal_peg)
            res = play(starts, temperature=temperature, deterministic=deterministic, legacy_rng=legacy_rng,
                       seed=seed)
            steps, ill = res["steps"].cpu().numpy(), res["illegal"].cpu().numpy()
        _score_budget(score, int(n), n_disks, goal_peg, starts, steps, ill)
    return dict(**score, minmax=mm if sequential else None)


def _check_plan(who, max_plan_len, n_sims_range):
    """max_plan_len: None, or an integer >= 1 with every budget >= 1 (a plan is a search's path)"""
    if max_plan_len is None:
        return
    if int(max_plan_len) != max_plan_len or int(max_plan_len) < 1:
        raise ValueError(f"{who}: max_plan_len must be an integer >= 1, got {max_plan_len}")
    if any(int(n) < 1 for n in n_sims_range):
        raise ValueError(f"{who}: a plan needs n_simulations >= 1 in every budget")


def _network_set(who, networks):
    """one network, a sequence of networks or a networks.NetworkSet -> a NetworkSet"""
    if isinstance(networks, NetworkSet):
        return networks
    nets = list(networks) if isinstance(networks, (list, tuple)) else [networks]
    if not nets:
        raise ValueError(f"{who}: no networks")
    return NetworkSet(nets)


def _start_indices(who, n_disks, starts, start_idx, episodes, seed, goal_peg):
    """starts (state tuples), else start_idx (state indices), else `episodes` random non-goal states of `seed`
    -> int64 [E] state indices, at least one and each in [0, 3^n_disks)"""
    if starts is not None:
        start_idx = [state_index(s) for s in starts]
    elif start_idx is None:
        if episodes is None or int(episodes) < 1:
            raise ValueError(f"{who}: no starts (give starts, start_idx or episodes >= 1)")
        start_idx = _batch_starts(n_disks, int(episodes), None, None, seed, goal_peg)
    start_idx = np.asarray(start_idx, np.int64).reshape(-1)
    if start_idx.size < 1 or start_idx.min() < 0 or start_idx.max() >= 3 ** n_disks:
        raise ValueError(f"{who}: starts must be state indices in [0, {3 ** n_disks}), at least one")
    return start_idx


def _new_score():
    return dict(data=[], illegal=[], errors=[], steps=[], illegal_rates=[])


def _score_budget(score, n, n_disks, goal_peg, starts, steps, ill):
    """one budget's episodes scored into evaluate's result lists: error = steps - hanoi_solver(start)
    (get_results), per-episode illegal-move rates with mean and standard error (illegal_move_rate)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.tensor([index_state(int(i), n_disks) for i in starts], dtype=torch.uint8, device=dev)
    opt = hanoi_solver_batch(n_disks, st, goal_peg).cpu().numpy()
    err = steps - opt
    rates = ill / np.maximum(steps, 1)
    score["data"].append([n, float(sum(int(e) for e in err) / len(err))])
    sem = float(np.std(rates, ddof=1) / np.sqrt(len(rates))) if len(rates) > 1 else float("nan")
    score["illegal"].append([n, float(np.mean(rates)), sem])
    score["errors"].append(err)
    score["steps"].append(steps)
    score["illegal_rates"].append(rates)


def _batch_starts(n_disks, episodes, start, start_idx, seed, goal_peg):
    """the start indices of one budget's batch of episodes (evaluate's batched schedule)"""
    if start_idx is not None:
        return np.asarray(start_idx, np.int64).reshape(-1)
    if start is None:
        g = np.random.default_rng(seed)
        goal = state_index((goal_peg,) * n_disks)
        starts = g.integers(0, 3 ** n_disks - 1, size=episodes)
        return starts + (starts >= goal)  # uniform over the non-goal states
    return np.full(episodes, _start_index(start, n_disks), np.int64)


def evaluate_networks(networks, n_disks, n_sims_range, *, episodes=1, start=None, start_idx=None, max_steps=200,
                      temperature=1.0, deterministic=False, seed=0, goal_peg=2, np1_ucb=False, max_plan_len=None,
                      dirichlet_alpha=0.25, max_roots=65536, launch="lockstep", budgets="each"):
    """evaluate's batched schedule for several networks at once -- the variants of an ablation sweep
    (checkpoint.ablation_variants; the reference runs acting_ablations.py once per variant): per budget one
    batch of len(networks) * episodes envs, network m's episodes consecutive and every network given the same
    starts (start / start_idx / the seed's random starts, as in evaluate), searched by one mzh_search_multi
    launch per move.  A batch above max_roots envs is played as several.  Every episode is its own agent with
    a fresh MinMaxStats and its own synthetic draws (the draws of env b of the batch: not those evaluate
    would give network m's episode alone).
    launch: "lockstep" (that move loop) or "episodes": each batch to its end in one launch
    (BatchedSelfPlay.play_episodes over the set, its draw schedule: env b takes row [t, b] of one table drawn from
    the batch's seed); search-per-step episodes only, so not with max_plan_len.
    budgets: "each" (a batch per budget, as above) or "fused": the budgets of the range play abreast -- per chunk of
    max_roots one batch of len(networks) * len(n_sims_range) * episodes envs ordered network, then budget, then
    episode, every env searching with its own budget in the one launch of a move (mzh_search_multi_budget; the
    engine is sized by the largest budget, every budget >= 0).  The fused batch's synthetic draws are a schedule of
    their own (the draws of env b of that batch: not those of the per-budget batches), so on more than one budget
    its episodes are not those of "each"; on one budget the two are the same batch.  Lockstep only.
    networks: a networks.NetworkSet or a sequence of networks.  Returns a list with, per network, the dict
    evaluate returns (minmax None), scored by the same code."""
    if budgets not in ("each", "fused"):
        raise ValueError(f"evaluate_networks: budgets must be 'each' or 'fused', not {budgets!r}")
    if budgets == "fused" and launch == "episodes":
        raise ValueError("evaluate_networks: budgets='fused' is a lockstep form: the episode launch has one budget")
    nset = _network_set("evaluate_networks", networks)
    _check_plan("evaluate_networks", max_plan_len, n_sims_range)
    if launch not in ("lockstep", "episodes"):
        raise ValueError(f"evaluate_networks: launch must be 'lockstep' or 'episodes', not {launch!r}")
    if launch == "episodes" and max_plan_len is not None:
        raise ValueError("evaluate_networks: launch='episodes' plays a search per step: it has no max_plan_len form")
    if int(max_roots) < 1:
        raise ValueError(f"evaluate_networks: max_roots must be >= 1, got {max_roots}")
    M = len(nset)
    scores = [_new_score() for _ in range(M)]
    if budgets == "fused":
        ns = [int(n) for n in n_sims_range]
        if not ns or min(ns) < 0:
            raise ValueError(f"evaluate_networks: budgets='fused' needs budgets >= 0, at least one, got {ns}")
        sp = BatchedSelfPlay(nset, n_disks, max_steps, max(ns), goal_peg=goal_peg, np1_ucb=np1_ucb,
                             dirichlet_alpha=dirichlet_alpha)
        play = sp.play if max_plan_len is None else (lambda s, **kw: sp.play_plans(s, int(max_plan_len), **kw))
        starts = _batch_starts(n_disks, episodes, start, start_idx, seed, goal_peg)
        E, K = len(starts), len(ns)
        all_starts, net_index = np.tile(starts, M * K), np.repeat(np.arange(M), K * E)
        sims = np.tile(np.repeat(np.asarray(ns, np.int64), E), M)
        steps, ill = [], []
        for k, lo in enumerate(range(0, M * K * E, int(max_roots))):
            sl = slice(lo, min(M * K * E, lo + int(max_roots)))
            res = play(all_starts[sl], temperature=temperature, deterministic=deterministic, seed=seed + k,
                       net_index=net_index[sl], sims=sims[sl])
            steps.append(res["steps"].cpu().numpy())
            ill.append(res["illegal"].cpu().numpy())
        steps, ill = np.concatenate(steps), np.concatenate(ill)
        for i, n in enumerate(ns):
            for m in range(M):
                sl = slice((m * K + i) * E, (m * K + i + 1) * E)
                _score_budget(scores[m], n, n_disks, goal_peg, starts, steps[sl], ill[sl])
        return [dict(**sc, minmax=None) for sc in scores]
    for n in n_sims_range:
        sp = BatchedSelfPlay(nset, n_disks, max_steps, int(n), goal_peg=goal_peg, np1_ucb=np1_ucb,
                             dirichlet_alpha=dirichlet_alpha)
        play = sp.play if max_plan_len is None else (lambda s, **kw: sp.play_plans(s, int(max_plan_len), **kw))
        if launch == "episodes":
            play = sp.play_episodes
        starts = _batch_starts(n_disks, episodes, start, start_idx, seed, goal_peg)
        E = len(starts)
        all_starts, net_index = np.tile(starts, M), np.repeat(np.arange(M), E)
        steps, ill = [], []
        for k, lo in enumerate(range(0, M * E, int(max_roots))):
            sl = slice(lo, min(M * E, lo + int(max_roots)))
            res = play(all_starts[sl], temperature=temperature, deterministic=deterministic, seed=seed + k,
                       net_index=net_index[sl])
            steps.append(res["steps"].cpu().numpy())
            ill.append(res["illegal"].cpu().numpy())
        steps, ill = np.concatenate(steps), np.concatenate(ill)
        for m in range(M):
            _score_budget(scores[m], int(n), n_disks, goal_peg, starts, steps[m * E:(m + 1) * E], ill[m * E:(m + 1) * E])
    return [dict(**sc, minmax=None) for sc in scores]


# ------------------------------------------------------------------------------------------------
# evaluation on perturbed observations (noise_injection_comparison.py, permutation_importance.py)
# ------------------------------------------------------------------------------------------------
def perturbed_layout(n_networks, conditions, start_idx, n_disks):
    """evaluate_perturbed's batch, on the host: one row per (network, condition, start), network-major then
    condition then start, so net_index is non-decreasing and every (network, condition) pair has the same starts.
    conditions: a list of ("baseline",), ("noise", std) and ("permute", disc).  Returns dict(net_index,
    cond_index, start_idx (int64 [R]), noise_std (float64 [R], 0 = none), permute_disc (int32 [R], -1 = none))
    with R = n_networks * len(conditions) * len(start_idx).  ValueError: an unknown condition, std < 0, a disc
    outside [0, n_disks), no conditions, no starts, n_networks < 1."""
    starts = np.asarray(start_idx, np.int64).reshape(-1)
    M, C, E = int(n_networks), len(conditions), int(starts.shape[0])
    if M < 1 or C < 1 or E < 1:
        raise ValueError(f"evaluate_perturbed: needs networks, conditions and starts, got {M}, {C}, {E}")
    if starts.min() < 0 or starts.max() >= 3 ** n_disks:
        raise ValueError(f"evaluate_perturbed: start indices must be in [0, {3 ** n_disks})")
    std, disc = np.zeros(C, np.float64), np.full(C, -1, np.int32)
    for c, cond in enumerate(conditions):
        cond = tuple(cond) if isinstance(cond, (tuple, list)) else (cond,)
        kind = cond[0] if cond else None
        if kind == "baseline" and len(cond) == 1:
            continue
        if kind == "noise" and len(cond) == 2:
            if not float(cond[1]) >= 0:
                raise ValueError(f"evaluate_perturbed: noise std must be >= 0, got {cond[1]!r}")
            std[c] = float(cond[1])
        elif kind == "permute" and len(cond) == 2:
            if int(cond[1]) != cond[1] or not 0 <= int(cond[1]) < n_disks:
                raise ValueError(f"evaluate_perturbed: permuted disc must be in [0, {n_disks}), got {cond[1]!r}")
            disc[c] = int(cond[1])
        else:
            raise ValueError(f"evaluate_perturbed: unknown condition {cond!r}: (\"baseline\",), (\"noise\", std) "
                             "or (\"permute\", disc)")
    cond_index = np.tile(np.repeat(np.arange(C), E), M)
    return dict(net_index=np.repeat(np.arange(M), C * E), cond_index=cond_index, start_idx=np.tile(starts, M * C),
                noise_std=std[cond_index], permute_disc=disc[cond_index])


def perturbed_scores(solved, n_networks, conditions):
    """solve_rate [M][C] (run_evaluation's solved / len(test_states)) and importance [M][C] from the per-row
    solved flags of a perturbed_layout batch: for a ("permute", disc) condition the network's first baseline
    rate minus its rate (permutation_importance.py:170-182); NaN for other conditions and without a baseline."""
    M, C = int(n_networks), len(conditions)
    rate = np.asarray(solved).reshape(M, C, -1).astype(np.float64).mean(axis=2)
    kinds = [(tuple(c) if isinstance(c, (tuple, list)) else (c,))[0] for c in conditions]
    importance = np.full((M, C), np.nan)
    if "baseline" in kinds:
        for c, k in enumerate(kinds):
            if k == "permute":
                importance[:, c] = rate[:, kinds.index("baseline")] - rate[:, c]
    return rate, importance


def evaluate_perturbed(networks, n_disks, *, conditions, starts=None, start_idx=None, episodes=None, n_sims=25,
                       max_steps=50, seed=0, goal_peg=2, max_roots=65536):
    """The solve rates of noise_injection_comparison.py (main: rate per noise std) and permutation_importance.py
    (main: per network a baseline rate and one per permuted disc, importance = baseline - permuted) as one batch
    of len(networks) * len(conditions) * len(starts) episodes (perturbed_layout), played by
    BatchedSelfPlay.play_perturbed in slices of max_roots rows: searches at temperature 0, deterministic, 25
    simulations and at most 50 steps by default, as the scripts run them.
    networks: one network, a sequence of networks or a networks.NetworkSet (e.g. the base network and
    acting.get_ablated_network's variants).  conditions: ("baseline",), ("noise", std), ("permute", disc).
    The starts, the same for every (network, condition): starts = state tuples (permutation_importance.py:143-156),
    or start_idx = state indices, or episodes = that many random non-goal states of `seed`.
    Every episode is its own agent with a fresh MinMaxStats (the scripts carry one MCTS instance through all
    games: acting.noise_run_evaluation / permutation_run_evaluation are that schedule) and takes row r of every
    draw, r its row of the batch, so the slicing does not change any episode.
    Returns dict(solve_rate [M][C], importance [M][C], solved [R] uint8, steps [R] int32, illegal [R] int32 and the
    layout's net_index / cond_index / start_idx [R]) as host arrays."""
    nset = _network_set("evaluate_perturbed", networks)
    if nset.in_dim != 3 * n_disks:
        raise ValueError(f"evaluate_perturbed: the networks read {nset.in_dim} inputs, n_disks={n_disks} gives {3 * n_disks}")
    if int(max_roots) < 1:
        raise ValueError(f"evaluate_perturbed: max_roots must be >= 1, got {max_roots}")
    start_idx = _start_indices("evaluate_perturbed", n_disks, starts, start_idx, episodes, seed, goal_peg)
    lay = perturbed_layout(len(nset), conditions, start_idx, n_disks)
    R = int(lay["net_index"].shape[0])
    sp = BatchedSelfPlay(nset, n_disks, max_steps, int(n_sims), goal_peg=goal_peg)
    got = dict(solved=[], steps=[], illegal=[])
    for lo in range(0, R, int(max_roots)):
        sl = slice(lo, min(R, lo + int(max_roots)))
        res = sp.play_perturbed(lay["start_idx"][sl], noise_std=lay["noise_std"][sl],
                                permute_disc=lay["permute_disc"][sl], seed=seed, net_index=lay["net_index"][sl],
                                draw_index=np.arange(sl.start, sl.stop))
        for k in got:
            got[k].append(res[k].cpu().numpy())
    got = {k: np.concatenate(v) for k, v in got.items()}
    rate, importance = perturbed_scores(got["solved"], len(nset), conditions)
    return dict(solve_rate=rate, importance=importance, **got, net_index=lay["net_index"],
                cond_index=lay["cond_index"], start_idx=lay["start_idx"])


# ------------------------------------------------------------------------------------------------
# predicted reward / value of legal versus illegal moves (legal_illegal_preds.py)
# ------------------------------------------------------------------------------------------------
def evaluate_legality(networks, n_disks, *, episodes=100, n_sims=25, max_steps=200, seed=0, starts=None,
                      start_idx=None, goal_peg=2, legacy_rng=False, record=False):
    """legal_illegal_preds.py (main: evaluate_network for the base, the policy-ablated and the value-ablated
    network) as one batch of len(networks) * episodes envs: network m's episodes consecutive, every network given
    the same starts (starts = state tuples, or start_idx = state indices, or `episodes` random non-goal states of
    `seed`).  Searches as the script runs them: 25 simulations, temperature 0.0, deterministic=False, at most 200
    steps.  Per move: one search over the unfinished rows (mzh_search_multi; mzh_search with one network), one
    mzh_probe_actions on the same rows into slot t of a device record (reward / value [T][B][6], legal [T][B]),
    one env step and one host read of the done flags.  The record is read once at the end and scored by
    acting.legality_summary, the drop-in's own statistics.
    Every episode is its own agent with a fresh MinMaxStats (the script carries one MCTS instance through a
    network's episodes: acting.legality_evaluate_network is that schedule).  Episode e of every network takes
    row e of a move's synthetic draws, so a network's result does not depend on which other networks share the
    batch; legacy_rng=True draws from NumPy's global stream instead, in env order over the unfinished rows (the
    reference's order when the batch is one env).
    networks: one network, a sequence of networks or a networks.NetworkSet.  Returns a list with, per network,
    evaluate_network's dict plus steps [E]; record=True adds the network's slice of the record: reward / value
    [T][E][6], legal [T][E], action [T][E] (-1 after the episode's end)."""
    from .acting import legality_summary  # acting imports this module

    nset = _network_set("evaluate_legality", networks)
    M = len(nset)
    start_idx = _start_indices("evaluate_legality", n_disks, starts, start_idx, episodes, seed, goal_peg)
    E = int(start_idx.shape[0])
    if int(max_steps) < 1:
        raise ValueError(f"evaluate_legality: max_steps must be >= 1, got {max_steps}")
    if nset.in_dim != 3 * n_disks:
        raise ValueError(f"evaluate_legality: the networks do not read {3 * n_disks} inputs (n_disks={n_disks})")
    multi = M > 1  # one network: mzh_search
    sp = BatchedSelfPlay(nset if multi else nset[0], n_disks, int(max_steps), int(n_sims), goal_peg=goal_peg)
    # episode e of every network takes row e of a move's draws
    got = sp.play_probed(np.tile(start_idx, M), seed=seed, legacy_rng=legacy_rng,
                         net_index=np.repeat(np.arange(M), E) if multi else None, draw_index=np.arange(M * E) % E)
    reward, value, legal, action, steps = (got[k].cpu().numpy()
                                           for k in ("reward", "value", "legal", "action", "steps"))
    res = []
    for m in range(M):
        sl = slice(m * E, (m + 1) * E)
        d = legality_summary(reward[:, sl], value[:, sl], legal[:, sl], steps[sl])
        d["steps"] = steps[sl].copy()
        if record:
            d.update(reward=reward[:, sl].copy(), value=value[:, sl].copy(), legal=legal[:, sl].copy(),
                     action=action[:, sl].copy())
        res.append(d)
    return res


def evaluate_saliency(networks, n_disks, *, states=None, start_idx=None):
    """gradient_analysis.py's atlas (compute_saliency for one state and one network per process) as one
    mzh_saliency call on a network set: every given state (states = state tuples, or start_idx = state indices;
    default all 3^n_disks states in state_index order) under every network of the list, network m's S rows
    consecutive.  networks: one network, a sequence of networks or a networks.NetworkSet.
    Returns numpy arrays: policy / value [M][S][3N] float32 (d(policy logit at its argmax)/d(obs), d(value)/d(obs)),
    picked [M][S] int32 (that argmax), disc_policy / disc_value [M][S][N] (aggregate_saliency_per_disk in fp32)
    and states [S] int64."""
    nset = _network_set("evaluate_saliency", networks)
    M = len(nset)
    if nset.in_dim != 3 * n_disks:
        raise ValueError(f"evaluate_saliency: the networks do not read {3 * n_disks} inputs (n_disks={n_disks})")
    if states is None and start_idx is None:
        start_idx = np.arange(3 ** n_disks)
    idx = _start_indices("evaluate_saliency", n_disks, states, start_idx, None, 0, 2)
    S = int(idx.shape[0])
    eng = engine_for_set(nset, 0, M * S)
    st = np.array([index_state(int(i), n_disks) for i in idx], np.int64)  # [S][N]
    obs1 = np.zeros((S, n_disks, 3), np.float32)
    obs1[np.arange(S)[:, None], np.arange(n_disks)[None, :], st] = 1.0
    obs = torch.from_numpy(np.tile(obs1.reshape(S, 3 * n_disks), (M, 1))).to(eng.device)
    net_index = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), S)).to(eng.device)
    out = eng.saliency(obs, net_index=net_index, full=True)
    if int(out["_status"][0].item()) != 0:
        raise RuntimeError("evaluate_saliency: the device refused net_index")
    res = {k: out[k].cpu().numpy().reshape((M, S) + tuple(out[k].shape[1:]))
           for k in ("policy", "value", "picked", "disc_policy", "disc_value")}
    res["states"] = idx
    return res


# ------------------------------------------------------------------------------------------------
# parameter gradients of the five sub-networks (gradient_analysis.py get_results)
# ------------------------------------------------------------------------------------------------
GRADIENT_NETS = ("representation", "dynamic", "reward", "policy", "value")
_FACTOR_KEYS = ("delta1", "delta2", "act", "h0", "z1", "h1", "pi0", "value0", "reward", "objective")


def dense_gradients(factors, obs, action, support):
    """The dense gradients of rank-one factors, in torch: [...][n_floats] float32 in load_weights' flat layout
    (weight then bias of Linear0 and Linear2 of the five nets), what mzh_pgrad_expand_kernel writes -- every
    weight element the single fp32 product delta[i] * in[j] (Linear0: delta1 (x) in with in = obs,
    cat(h0, one_hot(action)), z1, h0, h0; Linear2: delta2 (x) act), every bias a copy.  factors: a dict with
    delta1 / act [...][5][256], delta2 [...][5][64], h0 / z1 [...][64] (torch tensors or arrays, as
    Engine.param_grads or evaluate_gradients return them); obs [...][3N] float32, action [...] integers."""
    f = {k: torch.as_tensor(factors[k]) for k in ("delta1", "delta2", "act", "h0", "z1")}
    lead = tuple(f["h0"].shape[:-1])
    dev = f["h0"].device
    obs = torch.as_tensor(obs).to(dev, torch.float32).reshape(lead + (-1,))
    onehot = torch.nn.functional.one_hot(torch.as_tensor(action).to(dev, torch.int64).reshape(lead), ACTIONS).to(torch.float32)
    ins = (obs, torch.cat([f["h0"], onehot], dim=-1), f["z1"], f["h0"], f["h0"])
    outs = (LATENT, LATENT, int(support), ACTIONS, int(support))
    parts = []
    for i in range(5):
        d1, d2 = f["delta1"][..., i, :], f["delta2"][..., i, :outs[i]]
        parts += [(d1[..., :, None] * ins[i][..., None, :]).reshape(lead + (-1,)), d1,
                  (d2[..., :, None] * f["act"][..., i, None, :]).reshape(lead + (-1,)), d2]
    return torch.cat(parts, dim=-1)


def evaluate_gradients(networks, n_disks, *, states=None, start_idx=None, actions=range(6), policy_logit=None,
                       dense=False):
    """gradient_analysis.py's main loop over get_results (one state, one action and one network per call) as one
    mzh_param_grads call on a network set: every given state (states = state tuples, or start_idx = state indices;
    default all 3^n_disks states in state_index order) x every action of `actions` under every network of the
    list, rows network-major, then state, then action.  policy_logit: None the reference's mean(softmax) objective
    of the policy net, an integer k its logit k for every row, or an [S][A] array.  networks: one network, a
    sequence of networks or a networks.NetworkSet.
    Returns numpy arrays: the factors delta1 / act [M][S][A][5][256], delta2 [M][S][A][5][64], h0 / z1 / h1
    [M][S][A][64], pi0 [M][S][A][6], value0 / reward [M][S][A], objective [M][S][A][5], and states [S] int64,
    actions [A] int32; with dense=True also grad [M][S][A][n_floats] (dense_gradients expands kept factors)."""
    nset = _network_set("evaluate_gradients", networks)
    M = len(nset)
    if nset.in_dim != 3 * n_disks:
        raise ValueError(f"evaluate_gradients: the networks do not read {3 * n_disks} inputs (n_disks={n_disks})")
    if states is None and start_idx is None:
        start_idx = np.arange(3 ** n_disks)
    idx = _start_indices("evaluate_gradients", n_disks, states, start_idx, None, 0, 2)
    acts = np.asarray(list(actions), np.int32)
    if acts.ndim != 1 or acts.size < 1 or ((acts < 0) | (acts >= ACTIONS)).any():
        raise ValueError(f"evaluate_gradients: actions must be a non-empty sequence of 0..5, got {acts.tolist()}")
    S, A = int(idx.shape[0]), int(acts.shape[0])
    pl = None
    if policy_logit is not None:
        pl = np.broadcast_to(np.asarray(policy_logit, np.int32), (S, A))
        if ((pl < -1) | (pl >= ACTIONS)).any():
            raise ValueError("evaluate_gradients: policy_logit outside [-1, 6)")
    eng = engine_for_set(nset, 0, M * S * A)
    st = np.array([index_state(int(i), n_disks) for i in idx], np.int64)  # [S][N]
    obs1 = np.zeros((S, n_disks, 3), np.float32)
    obs1[np.arange(S)[:, None], np.arange(n_disks)[None, :], st] = 1.0
    obs = torch.from_numpy(np.tile(np.repeat(obs1.reshape(S, 3 * n_disks), A, axis=0), (M, 1))).to(eng.device)
    action = torch.from_numpy(np.tile(acts, M * S)).to(eng.device)
    net_index = torch.from_numpy(np.repeat(np.arange(M, dtype=np.int32), S * A)).to(eng.device)
    plt = None if pl is None else torch.from_numpy(np.tile(pl.reshape(-1), M)).to(eng.device)
    out = eng.param_grads(obs, action, net_index=net_index, policy_logit=plt, full=True, dense=dense)
    if int(out["_status"][0].item()) != 0:
        raise RuntimeError("evaluate_gradients: the device refused net_index")
    res = {k: out[k].cpu().numpy().reshape((M, S, A) + tuple(out[k].shape[1:]))
           for k in _FACTOR_KEYS + (("grad",) if dense else ())}
    res["states"] = idx
    res["actions"] = acts
    return res
