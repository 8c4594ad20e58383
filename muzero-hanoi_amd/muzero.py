"""MuZero agent drop-in (reference: Muzero.py:13-323, `Muzero`) -- SURVEY.md section 8f rank 3.

Same constructor and `training_loop(n_loops, min_replay_size, print_acc)` as the reference, so
`training_main.py` can construct it unchanged.  What runs where on the MI355X:
  * self-play (`_play_game`): every search is one fused libmzh kernel launch (mcts.MCTS) and the
    environment step is the reference's (selfplay.play_game); with selfplay="batched" the
    n_ep_x_loop episodes of a loop play in lockstep -- one search launch and one env-kernel launch
    per step for all of them (selfplay.BatchedSelfPlay), each episode an agent whose MinMaxStats
    starts from the MCTS instance's -- or, with selfplay="device", to their ends in one kernel launch
    (BatchedSelfPlay.play_episodes: for n_ep_x_loop = 1 the same episodes, buffer and RNG stream as
    "batched"), then the reference's per-episode bookkeeping
    (selfplay.episode_records) and buffer filter -- or, with ingest="device", that bookkeeping, the
    filter and the buffer writes as one device call on the play's record (selfplay.ingest_records:
    the same buffer, priorities and RNG stream).  With n_ep_x_loop > 1 that is NOT the
    reference's schedule (one MinMaxStats chain through the episodes in order, Muzero.py:55; other
    per-step draw interleaving): a RuntimeWarning says so, and "sequential" (the default) is the
    parity mode;
  * the replay buffer keeps its transitions on the training device (buffer.Buffer);
  * the update (`_update`, Muzero.py:209-274): the 5-step unrolled loss of the reference -- the
    same torch operations in the same order (represent, prediction/dynamics per unroll step,
    0.5 gradient scaling of the dynamics latent, MSE value / reward and cross-entropy policy terms,
    importance weights, 1/unroll gradient scaling, Adam) -- on PyTorch-ROCm.  After each update
    the search engine repacks the weights (networks.engine_for tracks parameter versions).
"""
import ctypes
import inspect
import logging
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd.graph import increment_version

from .buffer import Buffer
from .mcts import MCTS
from .networks import MuZeroNet, NetworkSet
from .rng import predraw, uses_noise
from .selfplay import BatchedSelfPlay, episode_records, episodes_result, ingest_records, play_game
from .utils import adjust_temperature, organise_transitions


class Muzero:
    def __init__(self, env, s_space_size, n_action, discount, dirichlet_alpha, n_mcts_simulations, unroll_n_steps,
                 batch_s, TD_return, n_TD_step, lr, buffer_size, priority_replay, device, n_ep_x_loop=1,
                 n_update_x_loop=1, update_impl="torch", selfplay="sequential", device_sampling=None, ingest="host"):
        self.dev = device
        self.env = env
        # ingest (not in the reference's signature): "host" = the reference's per-episode bookkeeping and
        # Buffer.add on the host; "device" = the batched record into the ring on the device
        # (Buffer.add_episodes), n-step TD returns only (Monte-Carlo returns stay on the host path)
        if ingest not in ("host", "device"):
            raise ValueError(f"ingest must be 'host' or 'device', not {ingest!r}")
        if ingest == "device":
            if selfplay not in ("batched", "device"):
                raise ValueError("Muzero(ingest='device') ingests a batched play's record: it needs selfplay='batched' "
                                 "or selfplay='device'")
            if not TD_return:
                raise ValueError("Muzero(ingest='device') implements the n-step TD returns: it needs TD_return=True")
            if torch.device(device).type != "cuda":
                raise ValueError("Muzero(ingest='device') needs a GPU device")
        if selfplay == "device" and torch.device(device).type != "cuda":
            raise ValueError("Muzero(selfplay='device') plays its episodes in a GPU kernel: it needs a GPU device")
        if selfplay == "device" and n_ep_x_loop > 1:
            # not the reference's algorithm, as with "batched" below; said before anything touches the device
            warnings.warn("Muzero(selfplay='device') with n_ep_x_loop > 1 plays the loop's episodes side by side, each "
                          "from the same MinMaxStats (the union kept afterwards), env b on row b of a move-major "
                          "draw table: not the reference's sequential schedule; use selfplay='sequential' for "
                          "parity runs", RuntimeWarning, stacklevel=2)
        self.ingest = ingest
        self.n_ep_x_loop = n_ep_x_loop  # episodes collected per training loop
        self.discount = discount
        self.n_action = n_action
        self.unroll_n_steps = unroll_n_steps
        self.n_update_x_loop = n_update_x_loop  # updates per training loop
        self.batch_s = batch_s
        self.TD_return = TD_return
        self.n_step = n_TD_step
        self.mcts = MCTS(discount=discount, root_dirichlet_alpha=dirichlet_alpha, n_simulations=n_mcts_simulations,
                         batch_s=batch_s, device=device)
        self.networks = MuZeroNet(rpr_input_s=s_space_size, action_s=n_action, lr=lr, TD_return=TD_return,
                                  device=device).to(device)
        # device_sampling (not in the reference's signature): the prioritised draw and the priority
        # write-back on the device (buffer.Buffer); by default with the fused update on a GPU
        if device_sampling is None:
            device_sampling = update_impl == "fused" and bool(priority_replay) and torch.device(device).type == "cuda"
        self.buffer = Buffer(buffer_size, unroll_n_steps, d_state=s_space_size, n_action=n_action, device=device,
                             device_sampling=device_sampling)
        self.priority_replay = priority_replay
        # update_impl (not in the reference's signature): "torch" = the reference's op sequence,
        # "graph" = that sequence replayed as one HIP graph (GraphedUpdate), "fused" = the two-kernel
        # HIP update of libmzh (FusedUpdate)
        if update_impl not in ("torch", "graph", "fused"):
            raise ValueError(f"update_impl must be 'torch', 'graph' or 'fused', not {update_impl!r}")
        self._graphed = {"torch": None, "graph": GraphedUpdate, "fused": FusedUpdate}[update_impl]
        if self._graphed is not None:
            self._graphed = self._graphed(self)
        # selfplay (not in the reference's signature): "sequential" = one episode after another as
        # Muzero._play_game runs them; "batched" = a loop's n_ep_x_loop episodes in lockstep; "device" = those
        # episodes played to their ends in one kernel launch (BatchedSelfPlay.play_episodes)
        if selfplay not in ("sequential", "batched", "device"):
            raise ValueError(f"selfplay must be 'sequential' or 'batched', not {selfplay!r}: the accepted values are "
                             "'sequential', 'batched' and 'device'")
        if selfplay == "batched" and n_ep_x_loop > 1:
            # not the reference's algorithm: the reference threads ONE MinMaxStats through its
            # episodes in order (Muzero.py:55) and interleaves the per-step draws differently
            warnings.warn("Muzero(selfplay='batched') with n_ep_x_loop > 1 plays the loop's episodes in lockstep, "
                          "each from the same MinMaxStats (the union kept afterwards) with its own draw order: "
                          "not the reference's sequential schedule; use selfplay='sequential' for parity runs",
                          RuntimeWarning, stacklevel=2)
        self.selfplay = selfplay

    # ------------------------------------------------------------------ Muzero.py:81-151
    def training_loop(self, n_loops, min_replay_size, print_acc=50):
        logging.info("Training started \n")
        log = self._new_log()
        for n in range(1, n_loops):
            ep_steps = []
            if self.ingest == "device":  # played, filtered and written to the buffer on the device
                ep_steps = [int(s) for s in self._play_games(self.n_ep_x_loop, episode=n * self.n_ep_x_loop,
                                                             deterministic=False)]
                episodes = ()
            elif self.selfplay in ("batched", "device"):
                episodes = self._play_games(self.n_ep_x_loop, episode=n * self.n_ep_x_loop, deterministic=False)
            else:
                episodes = (self._play_game(episode=n * self.n_ep_x_loop, deterministic=False)
                            for _ in range(self.n_ep_x_loop))
            self._ingest_loop(log, ep_steps, episodes)
            self._update_loop(log, min_replay_size)
            self._log_loop(log, n, print_acc)
        return log["tot_accuracy"]

    @staticmethod
    def _new_log():
        """what a training_loop call accumulates between its loops"""
        return dict(accuracy=[], tot_accuracy=[], value_loss=[], rwd_loss=[], pi_loss=[])

    def _finish_loop(self, log, n, ep_steps, episodes, min_replay_size, print_acc):
        """loop n after its self-play (Muzero.py:95-151), its three parts in order"""
        self._ingest_loop(log, ep_steps, episodes)
        self._update_loop(log, min_replay_size)
        self._log_loop(log, n, print_acc)

    def _ingest_loop(self, log, ep_steps, episodes):
        """the successful episodes into the buffer (ep_steps: the step counts of those already ingested) and the
        loop's accuracy"""
        for steps, states, rwds, actions, pi_probs, returns, priorities in episodes:
            ep_steps.append(steps)
            if returns[-1, 0] > 0:  # only successful episodes enter the buffer
                self.buffer.add(states, rwds, actions, pi_probs, returns, priorities)
        log["accuracy"].append(sum(ep_steps) / self.n_ep_x_loop)

    def _update_loop(self, log, min_replay_size):
        """the loop's updates once the buffer is large enough, and their losses"""
        if len(self.buffer) > min_replay_size:
            for _ in range(self.n_update_x_loop):
                if self.priority_replay:
                    states, rwds, actions, pi_probs, returns, indx, w = self.buffer.priority_sample(self.batch_s)
                else:
                    states, rwds, actions, pi_probs, returns = self.buffer.uniform_sample(self.batch_s)
                    indx, w = None, None
                new_prio, v_loss, r_loss, p_loss = self._update(states, rwds, actions, pi_probs, returns, w)
                self.buffer.update_priorities(indx, new_prio)
            log["value_loss"].append(v_loss)
            log["rwd_loss"].append(r_loss)
            log["pi_loss"].append(p_loss)

    def _log_loop(self, log, n, print_acc):
        """every print_acc episodes: the mean accuracy and losses since the last line"""
        if n * self.n_ep_x_loop % print_acc == 0:
            mean_acc = sum(log["accuracy"]) / print_acc
            logging.info("Loop %s | steps %.3f | V %.3f | rwd %.3f | Pi %.3f", n, mean_acc,
                         sum(log["value_loss"]) / print_acc, sum(log["rwd_loss"]) / print_acc,
                         sum(log["pi_loss"]) / print_acc)
            log["tot_accuracy"].append(mean_acc)
            log["accuracy"] = []
            log["value_loss"], log["rwd_loss"], log["pi_loss"] = [], [], []

    # ------------------------------------------------------------------ Muzero.py:153-207
    def _play_game(self, episode, deterministic=False):
        return play_game(self.env, self.mcts, self.networks, episode, deterministic, discount=self.discount,
                         TD_return=self.TD_return, n_step=self.n_step, unroll_n_steps=self.unroll_n_steps,
                         n_action=self.n_action)

    def _play_games(self, n_games, episode, deterministic=False):
        """n_games episodes from env.reset()'s start in lockstep (BatchedSelfPlay): each one an
        agent whose MinMaxStats starts from this MCTS instance's; afterwards the instance keeps
        the union (max of the maxima, min of the minima).  Draws come from the global NumPy stream
        (for n_games = 1 exactly the draws of _play_game).  Returns _play_game's tuple per episode; with
        ingest="device" the episodes go into the buffer here and only their step counts come back."""
        env, mm = self.env, self.mcts.min_max_stats
        sp = self._selfplay(self.networks)
        kw = dict(temperature=adjust_temperature(episode), deterministic=deterministic,
                  minmax=[[mm.maximum, mm.minimum]] * n_games)
        if self.selfplay != "device":
            res = sp.play([env.init_state_idx] * n_games, legacy_rng=True, record_obs=True, **kw)
        elif n_games == 1:  # one launch; the global stream is left where the lockstep play leaves it
            res = sp.play_episodes([env.init_state_idx], legacy_rng=True, **kw)
        else:  # the whole draw table from the global stream, move-major: row t * n_games + b for move t of env b
            res = sp.play_episodes([env.init_state_idx] * n_games, draws=self._draw_table(sp, n_games, deterministic),
                                   **kw)
        return self._games_played(res)

    def _selfplay(self, network):
        """the BatchedSelfPlay of this agent's env and search settings over `network`"""
        env = self.env
        return BatchedSelfPlay(network, env.discs, env.max_steps, int(self.mcts.n_simulations),
                               discount=self.discount, dirichlet_alpha=self.mcts.root_dirichlet_alpha,
                               root_exploration_eps=self.mcts.root_exploration_eps, goal_peg=env.goal[0],
                               np1_ucb=self.mcts.np1_ucb)

    def _draw_table(self, sp, n_games, deterministic=False, alpha=None):
        """play_episodes' table for n_games envs from the global NumPy stream, move-major (alpha: the Dirichlet alpha
        of the draws where it is not sp's, a population's agent under a launch of several configurations)"""
        T = int(self.env.max_steps)
        flat = predraw(T * n_games, deterministic=deterministic, alpha=sp.alpha if alpha is None else alpha, eps=sp.eps)
        return tuple(None if x is None else x.reshape((T, n_games) + x.shape[1:]) for x in flat)

    def _games_played(self, res):
        """what follows a play of this agent's episodes (res: play(record_obs=True)'s dict): the MCTS instance keeps
        the union of their MinMaxStats; _play_games' return value"""
        mm = self.mcts.min_max_stats
        fin = res["minmax"].cpu().numpy()
        mm.maximum, mm.minimum = float(fin[:, 0].max()), float(fin[:, 1].min())
        if self.ingest == "device":
            return ingest_records(res, self.buffer, discount=self.discount, n_step=self.n_step,
                                  unroll_n_steps=self.unroll_n_steps, n_action=self.n_action)
        return episode_records(res, discount=self.discount, TD_return=self.TD_return, n_step=self.n_step,
                               unroll_n_steps=self.unroll_n_steps, n_action=self.n_action)

    # ------------------------------------------------------------------ Muzero.py:209-274
    def _update(self, states, rwds, actions, pi_probs, returns, priority_w):
        if self._graphed is not None:
            return self._graphed(states, rwds, actions, pi_probs, returns, priority_w)
        net, U = self.networks, self.unroll_n_steps
        v_terms, r_terms, p_terms, pred_values_t = unrolled_losses(net, states, rwds, actions, pi_probs, returns, U,
                                                                    self.dev)
        loss = v_terms + r_terms + p_terms
        new_priorities = None
        if priority_w is not None:
            loss = loss * priority_w.detach()  # importance-sampling weights of the prioritised sample
            with torch.no_grad():
                pred0 = torch.stack(pred_values_t, dim=1).squeeze(-1)[:, 0]
                new_priorities = (pred0 - returns[:, 0]).abs().cpu().numpy()
        loss = loss.mean()
        loss.register_hook(lambda grad: grad * (1 / U))  # loss scaled by 1/unroll_steps (through the hook)
        net.update(loss)
        return new_priorities, v_terms.mean().detach(), r_terms.mean().detach(), p_terms.mean().detach()

    def organise_transitions(self, episode_state, episode_rwd, episode_action, episode_piProb, episode_returns):
        """Muzero.py:276-323"""
        return organise_transitions(episode_state, episode_rwd, episode_action, episode_piProb, episode_returns,
                                    self.unroll_n_steps, self.n_action)


class MuzeroPopulation:
    """Several seeds of one Muzero(selfplay="device") configuration trained abreast: every loop the agents' episodes
    play in ONE launch over the NetworkSet of their networks (BatchedSelfPlay.play_episodes with net_index: agent
    m's n_ep_x_loop envs on workgroups of their own), then each agent runs the lone loop's own ingest and updates.

    seeds: one agent per seed, built after torch.manual_seed(seed), with its own NumPy legacy stream in the state
    np.random.seed(seed) produces.  muzero_kwargs: Muzero's, without selfplay (always "device").  weights: how the
    set's engine picks up the agents' changed parameters every loop (networks.engine_for_set).  update: "each" (the
    default) or "set", the agents' update rounds as one launch sequence (SetUpdate); self.active_history then lists,
    per loop, the agents that updated in it.
    Agent m ends exactly as torch.manual_seed(s); mz = Muzero(..., selfplay="device"); np.random.seed(s);
    mz.training_loop(...) ends: parameters, optimiser state, buffer, MinMaxStats, tot_accuracy and stream
    (self.streams[m], a np.random.get_state() tuple).  The caller's global NumPy stream is left as it was found.

    overrides: None, or one dict per seed -- agent m is Muzero(**{**muzero_kwargs, **overrides[m]}), so agents of
    different configurations train abreast and the contract above holds for each with its own configuration.  The
    keys of SWEEP_KEYS may differ per agent; everything else (the env, unroll_n_steps, TD_return, n_ep_x_loop, the
    device and the selfplay / ingest / update_impl modes) is the launch's and the record's shape and stays shared.
    Agents of different n_mcts_simulations or discount play in one mzh_play_episodes_sweep launch (the set's engine
    made for the largest budget, env b with its agent's budget and discount); each agent's draw table and its
    post-launch predraw use its own dirichlet_alpha, its ingest its own n_TD_step and buffer, its updates its own
    lr, batch_s and n_update_x_loop.  Either all agents search with root noise or none does (the launch's noise table
    is all or none, and a noise-free root keeps float32 priors); update="set" shares one batch_s and n_update_x_loop.
    Without overrides, or with every dict empty, the launches and the results are those of a population of seeds."""

    SWEEP_KEYS = ("n_mcts_simulations", "discount", "dirichlet_alpha", "lr", "n_TD_step", "buffer_size", "batch_s",
                  "n_update_x_loop")

    def __init__(self, seeds, *, weights="device", update="each", overrides=None, **muzero_kwargs):
        # update: "each" = every agent runs the lone loop's own draws, updates and write-backs one after the other;
        # "set" = the agents' update rounds as one launch sequence for all of them (SetUpdate: four launches and one
        # host read per loop instead of four launches and a synchronisation per agent and round), every agent still
        # ending bit for bit as its lone run ends.  Validated before any agent is built.
        if update not in ("each", "set"):
            raise ValueError(f"MuzeroPopulation: update must be 'each' or 'set', not {update!r}")
        if update == "set" and muzero_kwargs.get("update_impl", "torch") != "fused":
            raise ValueError("MuzeroPopulation(update='set') runs the fused update of every agent in one launch "
                             "sequence: it needs update_impl='fused' with device sampling (priority_replay on a GPU)")
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("MuzeroPopulation: no seeds")
        if muzero_kwargs.setdefault("selfplay", "device") != "device":
            raise ValueError("MuzeroPopulation trains Muzero(selfplay='device') agents: selfplay must be 'device', "
                             f"not {muzero_kwargs['selfplay']!r}")
        overrides = self._check_overrides(seeds, update, overrides, muzero_kwargs)
        self.seeds, self.weights, self.update, self.overrides = seeds, weights, update, overrides
        self.agents = []
        for seed, over in zip(seeds, overrides):
            torch.manual_seed(seed)
            self.agents.append(Muzero(**{**muzero_kwargs, **over}))
        self.streams = [np.random.RandomState(seed).get_state() for seed in seeds]
        self.networks = NetworkSet([a.networks for a in self.agents])
        self.active_history = []  # update="set": per loop, the indices of the agents that updated in it
        self._set_update = SetUpdate(self.agents) if update == "set" else None

    @classmethod
    def _check_overrides(cls, seeds, update, overrides, muzero_kwargs):
        """the agents' own settings as one dict per seed (all empty without overrides), refused before any agent is
        built: a list of another length, a key outside SWEEP_KEYS, root noise for some agents only, and with
        update="set" a batch_s or n_update_x_loop of an agent's own"""
        if overrides is None:
            return [{} for _ in seeds]
        overrides = [dict(o) for o in overrides]
        if len(overrides) != len(seeds):
            raise ValueError(f"MuzeroPopulation: overrides has {len(overrides)} entries for {len(seeds)} seeds (one "
                             "dict per agent)")
        for m, over in enumerate(overrides):
            for key in over:
                if key not in cls.SWEEP_KEYS:
                    raise ValueError(f"MuzeroPopulation: agent {m} overrides {key!r}, which every agent of a "
                                     "population shares (the launch's and the record's shape); the keys an agent "
                                     f"may set are {', '.join(cls.SWEEP_KEYS)}")
                if update == "set" and key in ("batch_s", "n_update_x_loop"):
                    raise ValueError(f"MuzeroPopulation(update='set'): agent {m} overrides {key!r}, but the set's "
                                     "update rounds share one shape; use update='each'")
        if "dirichlet_alpha" in muzero_kwargs or all("dirichlet_alpha" in o for o in overrides):
            # the eps every agent's MCTS is built with (Muzero passes none: the constructor's default)
            eps = inspect.signature(MCTS.__init__).parameters["root_exploration_eps"].default
            alphas = [{**muzero_kwargs, **o}["dirichlet_alpha"] for o in overrides]
            noisy = [uses_noise(False, x, eps) for x in alphas]
            if any(noisy) != all(noisy):
                m = noisy.index(not noisy[0])
                raise ValueError(f"MuzeroPopulation: agent {m} with 'dirichlet_alpha'={alphas[m]} searches "
                                 f"{'with' if noisy[m] else 'without'} root noise and agent 0 with {alphas[0]} "
                                 f"{'with' if noisy[0] else 'without'}: the launch's noise table is for all agents or "
                                 "for none, and a noise-free root keeps float32 priors")
        return overrides

    def training_loop(self, n_loops, min_replay_size, print_acc=50):
        """Muzero.training_loop of every agent, loop by loop abreast.  Returns the list of the agents' tot_accuracy."""
        logging.info("Training started \n")
        agents, M = self.agents, len(self.agents)
        first, E = agents[0], agents[0].n_ep_x_loop
        # the launch's settings: the set's engine is made for the largest budget; where budgets or discounts differ,
        # env b plays with its agent's own (the sweep form of the launch), else the launch is a population of seeds'
        budgets = [int(a.mcts.n_simulations) for a in agents]
        T, sp = int(first.env.max_steps), agents[int(np.argmax(budgets))]._selfplay(self.networks)
        alphas = [a.mcts.root_dirichlet_alpha for a in agents]  # each agent's draws take its own Dirichlet alpha
        sweep = {}
        if len(set(budgets)) > 1 or len({float(a.discount) for a in agents}) > 1:
            sweep = dict(sims=np.repeat(np.asarray(budgets, np.int32), E),
                         discounts=np.repeat(np.asarray([a.discount for a in agents], np.float64), E))
        start = np.full(M * E, first.env.init_state_idx, np.int64)
        net_index = np.repeat(np.arange(M), E)
        logs = [a._new_log() for a in agents]
        caller = np.random.get_state()
        try:
            for n in range(1, n_loops):
                # every agent's table from its own stream, as a lone _play_games draws it; agent m's envs are
                # columns m * E .. of the launch's table
                tables, drawn_from = [], list(self.streams)
                for m, a in enumerate(agents):
                    np.random.set_state(self.streams[m])
                    tables.append(a._draw_table(sp, E, alpha=alphas[m]))
                    self.streams[m] = np.random.get_state()
                draws = tuple(None if col[0] is None else torch.from_numpy(np.concatenate(col, axis=1))
                              for col in zip(*tables))
                minmax = np.repeat([[a.mcts.min_max_stats.maximum, a.mcts.min_max_stats.minimum] for a in agents], E,
                                   axis=0)
                out = sp._launch_episodes(start, draws, minmax, adjust_temperature(n * E), False, net_index,
                                          self.weights, **sweep)
                *steps, n_err = (int(x) for x in torch.cat([out["steps"], out["err"]]).cpu())  # the one host read
                if n_err:
                    raise RuntimeError(f"mzh_play_episodes_multi refused {n_err} start state(s)")
                su = self._set_update
                if su is not None:
                    su.begin_loop()
                for m, a in enumerate(agents):
                    cols = slice(m * E, (m + 1) * E)
                    if E == 1:  # the one-env schedule: the stream as the moves played leave it
                        np.random.set_state(drawn_from[m])
                        predraw(steps[m], deterministic=False, alpha=alphas[m], eps=sp.eps)
                    else:
                        np.random.set_state(self.streams[m])
                    played = a._games_played(episodes_result(out, start[cols], max(steps[cols]), cols))
                    ep_steps, episodes = ([int(s) for s in played], ()) if a.ingest == "device" else ([], played)
                    if su is None:
                        a._finish_loop(logs[m], n, ep_steps, episodes, min_replay_size, print_acc)
                    else:  # phase A: the ingest, then this loop's uniforms off the agent's stream, where a lone
                        a._ingest_loop(logs[m], ep_steps, episodes)  # loop's updates would have drawn them
                        su.stage(m, min_replay_size)
                    self.streams[m] = np.random.get_state()
                if su is not None:  # phase B: every round of every agent, one synchronisation, then the logs
                    self.active_history.append(su.run(logs))
                    for m, a in enumerate(agents):
                        a._log_loop(logs[m], n, print_acc)
        finally:
            np.random.set_state(caller)
        return [log["tot_accuracy"] for log in logs]


def unrolled_losses(net, states, rwds, actions, pi_probs, returns, unroll_n_steps, device):
    """Per-sample value / reward / policy loss sums over the unrolled steps (Muzero.py:213-245), in
    the reference's operation order: h = represent(s); for each step t: prediction(h), then
    dynamics(h, onehot(a_t)) with the new latent's gradient halved, then the three loss terms."""
    v_sum = r_sum = p_sum = 0
    pred_values_t = []
    h = net.represent(states)
    for t in range(unroll_n_steps):
        pi_logits, values = net.prediction(h)
        onehot = F.one_hot(actions[:, t], num_classes=net.num_actions).squeeze().to(device, dtype=torch.long)
        h, pred_rwds = net.dynamics(h, onehot)
        h.register_hook(lambda grad: grad * 0.5)  # scale the dynamics gradient by 0.5
        v_sum += F.mse_loss(values.squeeze(), returns[:, t], reduction="none")
        r_sum += F.mse_loss(pred_rwds.squeeze(), rwds[:, t], reduction="none")
        p_sum += F.cross_entropy(pi_logits, pi_probs[:, t], reduction="none")  # logits in, softmax inside
        pred_values_t.append(values)
    return v_sum, r_sum, p_sum, pred_values_t


class GraphedUpdate:
    """`Muzero._update` captured once as a HIP graph and replayed per batch.

    At the reference's batch (256 transitions, 5 unroll steps, 256-wide MLPs) one update is a few
    hundred small kernels, so on the GPU it is bound by launch overhead, not by the GEMMs.  The
    graph holds the same torch operations as the eager `_update` (same order, same hooks); the
    only change is Adam's `capturable=True` form (step count and bias corrections kept on the
    device, so fp32 rather than Python-float step sizes: ulp-level differences).  Inputs are
    copied into static buffers, so the batch size and the prioritised/uniform choice are fixed
    at capture time (the first call).  Warm-up iterations run on a snapshot that is restored
    before capture, so the graph's first replay is the first real update.
    """

    def __init__(self, mz, warmup=3):
        if not str(mz.dev).startswith("cuda"):
            raise RuntimeError("graph_update needs a GPU device")
        self.mz = mz
        self.warmup = warmup
        self.graph = None
        net = mz.networks
        old = net.optimiser
        net.optimiser = opt_like(old, capturable=True, fused=True)

    def _capture(self, states, rwds, actions, pi_probs, returns, priority_w):
        mz, net, U = self.mz, self.mz.networks, self.mz.unroll_n_steps
        self.prio = priority_w is not None
        self.static_in = [t.detach().clone() for t in (states, rwds, actions, pi_probs, returns)]
        self.static_w = priority_w.detach().clone() if self.prio else None
        params = [p.detach().clone() for p in net.parameters()]
        opt_state = copy_opt_state(net.optimiser)

        def body():
            v, r, p, pred_values_t = unrolled_losses(net, *self.static_in, U, mz.dev)
            loss = v + r + p
            newp = None
            if self.prio:
                loss = loss * self.static_w
                with torch.no_grad():
                    newp = (torch.stack(pred_values_t, dim=1).squeeze(-1)[:, 0] - self.static_in[4][:, 0]).abs()
            loss = loss.mean()
            loss.register_hook(lambda grad: grad * (1 / U))
            loss.backward()
            net.optimiser.step()
            return newp, v.mean().detach(), r.mean().detach(), p.mean().detach()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self.warmup):
                net.optimiser.zero_grad(set_to_none=True)
                body()
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():  # undo the warm-up updates
            for q, p0 in zip(net.parameters(), params):
                q.copy_(p0)
            restore_opt_state(net.optimiser, opt_state)
        net.optimiser.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = body()

    def __call__(self, states, rwds, actions, pi_probs, returns, priority_w):
        if self.graph is None:
            self._capture(states, rwds, actions, pi_probs, returns, priority_w)
        else:
            if (priority_w is not None) != self.prio or states.shape != self.static_in[0].shape:
                raise ValueError("graph_update: batch shape / sampling mode changed after capture")
            for dst, src in zip(self.static_in, (states, rwds, actions, pi_probs, returns)):
                dst.copy_(src)
            if self.prio:
                self.static_w.copy_(priority_w)
        self.graph.replay()
        newp, v, r, p = self.out
        return (newp.cpu().numpy() if newp is not None else None), v.clone(), r.clone(), p.clone()


def opt_like(old, **overrides):
    """a torch.optim.Adam with `old`'s parameters, hyper-parameters and state, plus `overrides`"""
    groups = [{k: v for k, v in g.items() if k != "params"} for g in old.param_groups]
    params = [p for g in old.param_groups for p in g["params"]]
    d = dict(groups[0])
    d.update(overrides)
    new = torch.optim.Adam(params, **{k: d[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad",
                                                        "capturable", "fused") if k in d})
    st = old.state_dict()
    if st["state"]:
        for s in st["state"].values():  # capturable Adam keeps the step count on the parameter's device
            s["step"] = torch.as_tensor(float(s["step"]), dtype=torch.float32, device=params[0].device)
        st["param_groups"][0].update(overrides)
        new.load_state_dict(st)
    return new


def copy_opt_state(o):
    return {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()} for p, s in o.state.items()}


def restore_opt_state(o, saved):
    for p in list(o.state.keys()):
        if id(p) in saved:
            for k, v in saved[id(p)].items():
                if torch.is_tensor(o.state[p][k]) and torch.is_tensor(v):
                    o.state[p][k].copy_(v)
                else:
                    o.state[p][k] = v
        else:  # state created by the warm-up only: back to "no step taken yet", in place
            for k, v in o.state[p].items():
                if torch.is_tensor(v):
                    v.zero_()


class FusedUpdate:
    """`Muzero._update` + Adam as libmzh's fused HIP training update (csrc/mzh_train.hip).

    Launch 1 runs, per transition, the U-step unrolled forward and the complete backward pass of
    the reference's loss (Muzero.py:213-265) in one workgroup; launch 2 forms every weight gradient
    as a GEMM over the B*U rows on fp32 MFMA and applies torch.optim.Adam's update in place on the
    module's parameters and the optimiser's own state tensors, so `networks.state_dict()` and
    `networks.optimiser.state_dict()` (the checkpoint of training_main.py:93-103) stay the
    reference's.  Adam's step counter and bias corrections are the host-side Python floats torch
    uses.  Results match the torch update to fp32 rounding (other summation orders).
    """

    def __init__(self, mz):
        if not str(mz.dev).startswith("cuda"):
            raise RuntimeError("update_impl='fused' needs a GPU device")
        from . import _lib
        self._lib = _lib
        self.mz = mz
        net = mz.networks
        self.params = list(net.parameters())
        if len(self.params) != 20:
            raise ValueError("fused update expects MuZeroNet's 20 parameter tensors")
        g = net.optimiser.param_groups[0]
        if not isinstance(net.optimiser, torch.optim.Adam) or g["weight_decay"] != 0 or g["amsgrad"] \
                or g.get("maximize", False) or len(net.optimiser.param_groups) != 1:
            raise ValueError("fused update implements plain torch.optim.Adam (no weight decay / amsgrad)")
        self.support = net.support_size
        self.in_dim = self.params[0].shape[1]
        dev = self.params[0].device
        # transposed weight copies [in][out rounded up to 4] (16-byte rows for float4 loads)
        self.wt = [torch.zeros(p.shape[1], (p.shape[0] + 3) // 4 * 4, dtype=torch.float32, device=dev)
                   for p in self.params[0::2]]
        self.scratch = None
        self.B = None
        self._a = None
        self._seen = None  # parameter versions after our own last write

    def _versions(self):
        return tuple((p.data_ptr(), p._version) for p in self.params)

    def _state(self):
        opt = self.mz.networks.optimiser
        for p in self.params:
            st = opt.state[p]
            if len(st) == 0:  # torch.optim.Adam._init_group's lazy state
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return [opt.state[p] for p in self.params]

    def _setup(self, B, device):
        """scratch / outputs for batch size B and the argument block's fixed pointers: parameters,
        transposed copies and the optimiser's moment tensors (re-done when the optimiser's state
        objects change, e.g. after load_state_dict)"""
        L = self._lib
        U = self.mz.unroll_n_steps
        if self.B != B:
            nb = ctypes.c_size_t()
            L.check(L.lib().mzh_train_scratch_bytes(B, U, self.in_dim, self.support, nb), "mzh_train_scratch_bytes")
            self.scratch = torch.empty(nb.value // 4 + 64, dtype=torch.float32, device=device)
            self.row_loss = torch.empty(B, 3, dtype=torch.float32, device=device)
            self.new_prio = torch.empty(B, dtype=torch.float32, device=device)
            self.B = B
        states_ = self._state()
        a = L.TrainArgs()
        a.B, a.U, a.in_dim, a.support, a.rows = B, U, self.in_dim, self.support, 0
        for i, p in enumerate(self.params):
            a.param[i] = p.data_ptr()
        for i, w in enumerate(self.wt):
            a.wt[i] = w.data_ptr()
        for i, st in enumerate(states_):
            a.exp_avg[i] = st["exp_avg"].data_ptr()
            a.exp_avg_sq[i] = st["exp_avg_sq"].data_ptr()
        a.scratch = self.scratch.data_ptr()
        a.scratch_bytes = self.scratch.numel() * 4
        a.row_loss = self.row_loss.data_ptr()
        self._a = a
        # Adam's per-parameter step counters (0-dim host tensors in the optimiser's state): written through
        # NumPy views (one _foreach_add_ over 20 host tensors costs more than the update's launch)
        self._step_views = [st["step"].numpy() for st in states_]
        self._state_key = self._state_identity()

    def _state_identity(self):
        # Optimizer.load_state_dict installs a new state dict: its identity (and size) marks a reload
        opt = self.mz.networks.optimiser
        return id(opt.state), len(opt.state)

    def __call__(self, states, rwds, actions, pi_probs, returns, priority_w):
        L = self._lib
        B = states.shape[0]
        stream = torch.cuda.current_stream().cuda_stream
        if self._a is None or self.B != B or self._state_key != self._state_identity():
            self._setup(B, states.device)
        a = self._a
        if self._seen != self._versions():  # parameters written outside this update: re-transpose
            L.check(L.lib().mzh_train_transpose(a, stream), "mzh_train_transpose")
        g = self.mz.networks.optimiser.param_groups[0]
        beta1, beta2 = g["betas"]
        step = float(self._step_views[0]) + 1.0  # this update's step (written back after the launch)
        a.step_size = g["lr"] / (1 - beta1 ** step)
        a.bc2_sqrt = math.sqrt(1 - beta2 ** step)
        a.beta1, a.beta2, a.eps = beta1, beta2, g["eps"]
        ins = [states.float().contiguous(), rwds.float().contiguous(), actions.long().contiguous(),
               pi_probs.float().contiguous(), returns.float().contiguous()]
        w = priority_w.float().contiguous() if priority_w is not None else None
        a.obs, a.rwds, a.actions, a.pi, a.returns = (t.data_ptr() for t in ins)
        a.weights = w.data_ptr() if w is not None else None
        # with the buffer's device sampling the new priorities stay on the device (a new tensor per
        # update: update_priorities consumes it there); else they go to the host as the reference's do
        on_dev = w is not None and getattr(self.mz.buffer, "device_sampling", False)
        newp_t = torch.empty(B, dtype=torch.float32, device=states.device) if on_dev else self.new_prio
        a.new_prio = newp_t.data_ptr() if w is not None else None
        L.check(L.lib().mzh_train_update(a, stream), "mzh_train_update")
        for v in self._step_views:  # torch.optim.Adam's step += 1 (float32), while the kernels run
            v[...] = step
        increment_version(self.params)  # the kernel wrote the parameters in place: let version trackers know
        self._seen = self._versions()
        means = self.row_loss.mean(0)
        newp = None if w is None else (newp_t if on_dev else newp_t.cpu().numpy())
        return newp, means[0], means[1], means[2]


class SetUpdate:
    """The update rounds of several agents (update_impl="fused", device sampling) as one launch sequence
    (mzh_train_set_update, csrc/mzh_replay.hip + csrc/mzh_train.hip): per round the draws, the row kernel, the
    gradient / Adam kernel and the priority write-backs of ALL active agents are four launches, the network on the
    grid's y (or x) index, and a loop ends with one synchronisation and one read of the status words.  Every agent
    ends bit for bit as its own priority_sample + FusedUpdate + update_priorities end: the kernels run the lone
    calls' bodies, and the uniforms come off the agent's NumPy stream in the lone loop's order (nothing else draws
    between a loop's updates).

    The handle fixes every pointer: each agent's sampled batch, indices and new priorities are allocated once here
    (a lone update allocates them per call), row_loss is one [M][B][3] tensor (the logged losses are one batched
    mean over it), the importance weights are the buffer's ones.  The per-round records, uniforms and status words
    sit in mapped page-locked memory, one slot per round of a loop, rewritten only after the loop's
    synchronisation.  Agents whose buffer is still too small are inactive in a loop: the kernels skip them."""

    STEP = np.dtype([("active", np.int32), ("n", np.int32), ("step_size", np.float32), ("bc2_sqrt", np.float32)])

    def __init__(self, agents):
        from . import _lib

        for a in agents:
            if not isinstance(a._graphed, FusedUpdate) or not getattr(a.buffer, "device_sampling", False):
                raise ValueError("MuzeroPopulation(update='set') needs update_impl='fused' with device sampling on "
                                 "every agent (priority_replay on a GPU, device_sampling not switched off)")
        if len(agents) > _lib.TRAIN_SET_MAX:
            raise ValueError(f"MuzeroPopulation(update='set'): {len(agents)} agents, at most {_lib.TRAIN_SET_MAX}")
        self._lib, self.agents = _lib, agents
        self.M, self.R, self.B = len(agents), int(agents[0].n_update_x_loop), int(agents[0].batch_s)
        self.dev = agents[0].buffer.dev
        M, R, B = self.M, self.R, self.B
        self.step = torch.zeros((R, M, 4), dtype=torch.int32, pin_memory=True)
        self.step_np = self.step.numpy().view(self.STEP).reshape(R, M)
        self.u = torch.zeros((R, M, B), dtype=torch.float64, pin_memory=True)
        self.u_np = self.u.numpy()
        self.status = torch.zeros((R, M, 4), dtype=torch.int32, pin_memory=True)
        self.status_np = self.status.numpy()
        self.step_dev, self.u_dev, self.status_dev = (_lib.host_device_pointer(t.data_ptr())
                                                      for t in (self.step, self.u, self.status))
        if self.step_dev != self.step.data_ptr():  # the host reads the records through the same pointer (mzh.h)
            raise RuntimeError("SetUpdate: page-locked memory has different host and device addresses")
        self.handle, self._key = None, None
        self.active, self.final_step = [], {}

    def __del__(self):
        try:
            self._destroy()
        except Exception:  # interpreter shutdown: the library may be gone before the handle
            pass

    def _destroy(self):
        if getattr(self, "handle", None) is not None:
            self._lib.lib().mzh_train_set_destroy(self.handle)
            self.handle = None

    def _ready(self, a):
        """the agent's FusedUpdate set up for this batch size (its argument block, scratch, Adam state views)"""
        fu = a._graphed
        if fu._a is None or fu.B != self.B or fu._state_key != fu._state_identity():
            fu._setup(self.B, self.dev)
        return fu

    def _identity(self):
        return tuple((id(a._graphed._a), a._graphed._state_key, a.buffer._dev_replay.m) for a in self.agents)

    def _build(self):
        L, M, B, dev = self._lib, self.M, self.B, self.dev
        self._destroy()
        train, draw = (L.TrainArgs * M)(), (L.ReplayArgs * M)()
        self.row_loss = torch.zeros((M, B, 3), dtype=torch.float32, device=dev)
        self.keep = []  # the tensors the handle's pointers name
        for m, a in enumerate(self.agents):
            fu, buf = self._ready(a), a.buffer
            dr = buf._dev_replay
            if dr.m != B:
                dr.check_pending(block=True)
                dr._alloc_u(B)
            U, A = buf.unroll_n_steps, buf.n_action
            outs = (torch.zeros((B, buf.d_state), dtype=torch.float32, device=dev),
                    torch.zeros((B, U), dtype=torch.float32, device=dev),
                    torch.zeros((B, U), dtype=torch.int64, device=dev),
                    torch.zeros((B, U, A), dtype=torch.float32, device=dev),
                    torch.zeros((B, U), dtype=torch.float32, device=dev))
            indx = torch.zeros(B, dtype=torch.int64, device=dev)
            newp = torch.zeros(B, dtype=torch.float32, device=dev)
            self.keep.append((outs, indx, newp, dr.ones))
            g = a.networks.optimiser.param_groups[0]
            train[m] = fu._a  # a copy: parameters, moments, transposed copies, scratch
            t = train[m]
            t.obs, t.rwds, t.actions, t.pi, t.returns = (x.data_ptr() for x in outs)
            t.weights, t.row_loss, t.new_prio = dr.ones.data_ptr(), self.row_loss[m].data_ptr(), newp.data_ptr()
            (t.beta1, t.beta2), t.eps = g["betas"], g["eps"]
            t.step_size = t.bc2_sqrt = 0.0  # per round
            draw[m] = dr.args  # a copy: the ring arrays, prio, cdf
            d = draw[m]
            d.n, d.u, d.status = buf.size, None, None  # the ring's size; n, u and status come per round
            d.indx = indx.data_ptr()
            d.out_states, d.out_rwds, d.out_actions, d.out_pi, d.out_returns = (x.data_ptr() for x in outs)
        h = ctypes.c_void_p()
        L.check(L.lib().mzh_train_set_create(train, draw, M, ctypes.byref(h)), "mzh_train_set_create")
        self.handle, self._key = h, self._identity()
        self._train, self._draw = train, draw  # what the handle was made from (tools/bench_population_update.py)

    def begin_loop(self):
        self.active, self.final_step = [], {}
        self.step_np["active"][...] = 0

    def stage(self, m, min_replay_size):
        """agent m after its ingest, the global NumPy stream being its own: if its buffer is large enough, this
        loop's uniforms and Adam scalars (fp64, as FusedUpdate computes them) into the rounds' slots"""
        a = self.agents[m]
        n = len(a.buffer)
        if not n > min_replay_size:
            return
        fu = self._ready(a)
        g = a.networks.optimiser.param_groups[0]
        beta1, beta2 = g["betas"]
        step0 = float(fu._step_views[0])
        for r in range(self.R):
            self.u_np[r, m] = np.random.random_sample(self.B)  # the reference's stream: choice's random_sample(m)
            step = step0 + 1.0 + r
            self.step_np[r, m] = (1, n, g["lr"] / (1 - beta1 ** step), math.sqrt(1 - beta2 ** step))
        a.buffer._dev_replay.check_pending(block=True)
        self.active.append(m)
        self.final_step[m] = step0 + self.R

    def run(self, logs):
        """the loop's rounds of the staged agents; the losses of the last round into their logs.  Returns the active
        agents' indices.  The lone path's exceptions (ValueError for a draw NumPy's choice would refuse,
        AssertionError / IndexError for the write-back) are raised after all rounds have run and the agents' Adam
        counters and parameter versions are consistent with what the kernels wrote."""
        if not self.active:
            return []
        L, M, B = self._lib, self.M, self.B
        if self.handle is None or self._key != self._identity():
            self._build()
        stream = L.stream_handle(self.dev)
        for m in self.active:
            fu = self.agents[m]._graphed
            if fu._seen != fu._versions():  # parameters written outside the fused update: re-transpose
                L.check(L.lib().mzh_train_transpose(fu._a, stream), "mzh_train_transpose")
        for r in range(self.R):
            L.check(L.lib().mzh_train_set_update(self.handle, self.step_dev + r * M * 16, self.u_dev + r * M * B * 8,
                                                 self.status_dev + r * M * 16, stream), "mzh_train_set_update")
        means = self.row_loss.mean(1)  # [M][3], the last round's
        L.synchronize(self.dev)  # the loop's one synchronisation; the status words are read below
        for m in self.active:
            fu = self.agents[m]._graphed
            for v in fu._step_views:  # torch.optim.Adam's step counters (float32)
                v[...] = self.final_step[m]
            increment_version(fu.params)  # the kernels wrote the parameters in place: let version trackers know
            fu._seen = fu._versions()
            logs[m]["value_loss"].append(means[m, 0])
            logs[m]["rwd_loss"].append(means[m, 1])
            logs[m]["pi_loss"].append(means[m, 2])
        for r in range(self.R):
            for m in self.active:
                draw, _, wb, _ = (int(x) for x in self.status_np[r, m])
                if draw != 0:
                    raise ValueError("probabilities contain NaN or are not non-negative "
                                     f"(np.random.choice's check of the priorities, buffer.py:89-112; agent {m})")
                if wb == 1:
                    raise AssertionError("Priorities must be finite and positive.")
                if wb == 2:
                    raise IndexError(f"update_priorities: an index is outside [0, {self.agents[m].buffer.size})")
        return list(self.active)
