"""TowersOfHanoi drop-in (reference: env/hanoi.py:11-151) + a batched form.

The public surface is the reference's: constructor, `states`, `moves`, `goal`, `oneH_s_size`,
`n_pegs`, `discs`, `max_steps`, `init_state_idx`, `c_state` / `oneH_c_state` (assignable, as
noise_injection_comparison.py:20-21 and permutation_importance.py:46-47 do), `step`, `reset`,
`random_reset`, `current_state`, `_move_allowed`.  Transitions, legality and the observation are
computed by the libmzh integer kernels (mzh_env_step / mzh_legal_mask / mzh_encode_obs).

`HanoiBatch` keeps B environments resident on the GPU for batched self-play.
"""
import itertools

import numpy as np
import torch

from . import _lib, engine
from .engine import require_device
from .staging import Packed

_REWARD = {0: 0, 1: 100, -1: -100 / 1000}  # codes of mzh_env_step -> the reference's rewards


class TowersOfHanoi:
    def __init__(self, N, max_steps, init_state_idx=0, goal_peg=2):
        require_device()
        self.discs = N
        self.n_pegs = 3
        self.states = list(itertools.product(list(range(self.n_pegs)), repeat=self.discs))
        self.oneH_s_size = self.discs * self.n_pegs
        self.goal = tuple([goal_peg] * self.discs)
        self.goal_peg = goal_peg
        self.init_state_idx = init_state_idx
        self.moves = list(itertools.permutations(list(range(self.n_pegs)), 2))
        self.max_steps = max_steps
        self.reset_check = False
        self.step_counter = 0
        self._dev = torch.device("cuda", torch.cuda.current_device())
        self._pk = None

    # ------------------------------------------------------------------ reference API
    def step(self, action):
        """env/hanoi.py:47-84 -> (one-hot obs float64[3N], rwd, done, illegal_move)."""
        assert self.reset_check, "Need to reset env before taking a step"
        action = int(action)
        if not 0 <= action < 6:
            raise IndexError("list index out of range")
        pk = self._launch_step(action=action)
        pk.to_host()
        return self._finish_step()

    def _launch_step(self, action=None, action_ptr=None):
        """stage the env's state and launch mzh_env_step on the current stream; the action either goes into
        the staging record or is read by the kernel from `action_ptr` (device-readable int32, e.g. the search's
        own action output: MCTS.run_mcts_step chains the two launches)"""
        pk = self._packed()
        h = pk.h
        h["state"][0] = self.c_state
        if action_ptr is None:
            h["action"][0] = action
        h["ctr"][0] = self.step_counter
        h["active"][0] = 1
        pk.to_device()
        q = self._ptrs
        _lib.check(_lib.lib().mzh_env_step(self.discs, self.goal_peg, self.max_steps, 1, q["state"],
                                           q["action"] if action_ptr is None else action_ptr, q["moved"], q["obs"],
                                           q["code"], q["done"], q["illegal"], q["ctr"], q["active"], None,
                                           _lib.stream_handle(self._dev)), "mzh_env_step")
        return pk

    def _finish_step(self):
        """the step's results from the staging record (after the synchronisation)"""
        h = self._pk.h
        self.c_state = tuple(int(x) for x in h["state"][0])
        self.step_counter, self.reset_check = int(h["ctr"][0]), bool(h["active"][0])
        rwd, done_b, illegal_b = _REWARD[int(h["code"][0])], bool(h["done"][0]), bool(h["illegal"][0])
        return h["obs"][0].astype(np.float64), rwd, done_b, illegal_b

    def reset(self):
        self.reset_check = True
        self.c_state = self.states[self.init_state_idx]
        self.oneH_c_state = self._encode(self.c_state)
        return self.oneH_c_state

    def random_reset(self):
        """env/hanoi.py:103-115: draws from the global NumPy RNG exactly like the reference."""
        self.reset_check = True
        while True:
            random_indx = np.random.randint(len(self.states))
            self.c_state = self.states[random_indx]
            if self.c_state != self.goal:
                break
        self.oneH_c_state = self._encode(self.c_state)
        return self.oneH_c_state

    def current_state(self):
        return list(self.c_state)

    def _discs_on_peg(self, peg):
        return [disc for disc in range(self.discs) if self.c_state[disc] == peg]

    def _move_allowed(self, move):
        mask = engine.legal_mask(self.discs, torch.tensor([list(self.c_state)], dtype=torch.uint8, device=self._dev))
        return bool((int(mask.item()) >> self.moves.index(tuple(move))) & 1)

    # ------------------------------------------------------------------ helpers
    def _step_fields(self):
        """mzh_env_step's staging record: (the fields it updates in place or reads, the fields it only writes)"""
        n = self.discs
        return ([("state", torch.uint8, (1, n)), ("action", torch.int32, (1,)), ("ctr", torch.int32, (1,)),
                 ("active", torch.uint8, (1,))],
                [("moved", torch.uint8, (1, n)), ("obs", torch.float32, (1, 3 * n)), ("code", torch.int8, (1,)),
                 ("done", torch.uint8, (1,)), ("illegal", torch.uint8, (1,))])

    def _packed(self):
        if self._pk is None:
            inout, out = self._step_fields()
            self._pk = Packed.mapped(inout + out, self._dev)
            self._ptrs = self._pk.dptr  # fixed: the call passes them as is
        return self._pk

    def _packed_out2(self):
        """a second record of the step's outputs (MCTS.play_episode alternates output records between decisions)"""
        if getattr(self, "_pk2", None) is None:
            self._pk2 = Packed.mapped(self._step_fields()[1], self._dev)
        return self._pk2

    def _encode(self, state):
        st = torch.tensor([list(state)], dtype=torch.uint8, device=self._dev)
        return engine.encode_obs(self.discs, st)[0].to(torch.float64).cpu().numpy()


class HanoiBatch:
    """B independent TowersOfHanoi envs resident on one GPU (state [B,N] uint8, step counters,
    reset flags).  step() is one mzh_env_step launch; nothing leaves the device."""

    def __init__(self, N, max_steps, B, goal_peg=2, device=None):
        require_device()
        self.N, self.max_steps, self.B, self.goal_peg = N, max_steps, B, goal_peg
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.zeros((B, N), dtype=torch.uint8, device=self.device)
        self.step_ctr = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.active = torch.zeros(B, dtype=torch.uint8, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last_obs = self.steps_total = self.illegal_total = None  # run_plan's per-env arrays, made on first use
        self.solved = self.perm_disc = None  # step_observe's, likewise

    def reset(self, state_idx):
        """state_idx [B] -> reference state tuples (index = sum s[i] * 3^(N-1-i))."""
        idx = torch.as_tensor(state_idx, device=self.device).to(torch.int64)
        pw = 3 ** torch.arange(self.N - 1, -1, -1, device=self.device)
        self.state.copy_(((idx[:, None] // pw) % 3).to(torch.uint8))
        self.step_ctr.zero_()
        self.active.fill_(1)
        self.last_obs = self.steps_total = self.illegal_total = self.solved = self.perm_disc = None
        return self.obs()

    def obs(self):
        return engine.encode_obs(self.N, self.state)

    def step(self, action):
        obs = torch.empty((self.B, 3 * self.N), dtype=torch.float32, device=self.device)
        code, done, illegal = engine.env_step(self.N, self.max_steps, self.state, action.to(torch.int32).contiguous(),
                                              self.step_ctr, self.active, goal_peg=self.goal_peg, obs=obs, err=self.err)
        return obs, code, done, illegal

    def run_plan(self, plan, plan_len, max_plan_len, env_index=None, record=False):
        """Execute plan[j, :min(plan_len[j], max_plan_len)] on env env_index[j] (env j without env_index) open
        loop, one mzh_env_run_plan launch (planning_multiple_actions.py:139-178): each row steps until its plan
        runs out or its episode ends; finished envs are left untouched.  plan [n, stride] / plan_len [n] int32
        device tensors (a search's `latent` / `latent_len`), env_index [n] int32.  Updates state, step_ctr, active,
        last_obs (the observation env.step returned last), steps_total and illegal_total (per-env sums since
        reset); errors are counted in self.err.  Returns dict(executed [n], action [L, n], reward [L, n] int8
        codes -- the last two with record=True, -1 / 0 where nothing ran)."""
        self._tallies()
        executed, rec_a, rec_r = engine.env_run_plan(
            self.N, self.max_steps, self.state, self.step_ctr, self.active, self.last_obs, plan, plan_len,
            max_plan_len, self.steps_total, self.illegal_total, env_index=env_index, goal_peg=self.goal_peg,
            err=self.err, record=record)
        return dict(executed=executed, action=rec_a, reward=rec_r)

    def _tallies(self):
        """the per-env arrays of run_plan and step_observe (since reset), made on first use"""
        if self.last_obs is None:
            self.last_obs = self.obs()
            self.steps_total = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.illegal_total = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        if self.solved is None:
            self.solved = torch.zeros(self.B, dtype=torch.uint8, device=self.device)

    def set_perturbation(self, perm_disc):
        """perm_disc [B] (or a scalar for every env): the disc whose peg the model does not see, -1 / None for
        none (permutation_importance.py:55-59); holds until reset.  Values outside [-1, N) are the kernel's to
        refuse (self.err)."""
        if perm_disc is None:
            self.perm_disc = None
            return
        pd = torch.as_tensor(perm_disc, dtype=torch.int32).to(self.device).reshape(-1)
        self.perm_disc = (pd.expand(self.B) if pd.numel() == 1 else pd).contiguous()
        if self.perm_disc.shape[0] != self.B:
            raise ValueError(f"set_perturbation: perm_disc must be a scalar or [{self.B}], got {tuple(pd.shape)}")

    def step_observe(self, action, env_index=None, *, perm_peg=None, noise=None):
        """Step the true envs and write the observation the model is to see, one mzh_env_step_observe launch
        (noise_injection_comparison.py:17-37, permutation_importance.py:27-76): row j is env env_index[j] (env j
        without env_index), takes action[j] (action None: an observe-only call, the first observation of an
        episode) and, while still active, gets last_obs[env] = one-hot(state with disc perm_disc[env]'s peg
        replaced by perm_peg[j]) + noise[j] (float64 [n, 3N], already scaled; rounded once to float32).
        Finished envs are left untouched.  action / env_index / perm_peg are int32 device tensors [n]; perm_peg
        is required where set_perturbation gave a disc.  Updates state, step_ctr, active, last_obs, steps_total,
        illegal_total and solved (per-env, since reset); errors are counted in self.err.  Returns dict(reward
        [n] int8 codes, done [n] uint8)."""
        self._tallies()
        reward, done = engine.env_step_observe(
            self.N, self.max_steps, self.state, self.step_ctr, self.active, self.last_obs, self.steps_total,
            self.illegal_total, self.solved, action=action, env_index=env_index, perm_disc=self.perm_disc,
            perm_peg=perm_peg, noise=noise, goal_peg=self.goal_peg, err=self.err)
        return dict(reward=reward, done=done)

    def legal_mask(self):
        return engine.legal_mask(self.N, self.state)

    @staticmethod
    def reward_value(code):
        """int8 codes -> the reference's float rewards (0, 100, -0.1)"""
        out = torch.zeros(code.shape, dtype=torch.float64, device=code.device)
        out[code == 1] = 100.0
        out[code == -1] = -100 / 1000
        return out
