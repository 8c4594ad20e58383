// mzh_env.hip -- Tower-of-Hanoi environment kernels (env/hanoi.py, utils.py:9-25,
// env/hanoi_utils.py:4-26), one lane per env, integer-only, bit-exact with the reference.
//
// A state is N bytes (peg of disc d, disc 0 smallest), the reference's tuple layout.  The legal
// test _move_allowed (hanoi.py:123-139: from-peg non-empty and (to-peg empty or min(to) >
// min(from))) is computed as top[f] < top[t] with top[p] = smallest disc on peg p (N if empty).
//
// mzh_env_step_kernel and mzh_env_run_plan_kernel share one transition (env_transition): the step
// kernel applies it once per env, the plan kernel up to max_plan_len times per row with the state in
// registers (acting_experiments/planning_multiple_actions.py:139-178: a search's latent path executed
// open loop).  The plan kernel's reads of `plan` are a strided gather -- lane j reads
// plan[j * plan_stride + k], plan_stride = n_sims + 1 ints for the search's `latent` output, so
// consecutive lanes are plan_stride * 4 bytes apart and each lane touches at most max_plan_len
// consecutive ints (one or two 64-byte lines at max_plan_len 7).  They are not staged through LDS: no
// measurement says the gather matters next to the search that produced it.  Its record stores are laid
// out [max_plan_len][n], so consecutive lanes store consecutive addresses.
//
// mzh_env_step_observe_kernel applies the same transition once per row and then writes the observation the
// model is to see instead of the true one (noise_injection_comparison.py:17-37, permutation_importance.py:27-76).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mzh.h"
#include "mzh_env_kernels.h"

#define MZH_MAXN 32

__device__ __forceinline__ void load_state(const uint8_t* src, int n, uint8_t* st, int top[3]) {
  top[0] = top[1] = top[2] = n;
  for (int d = n - 1; d >= 0; --d) {
    st[d] = src[d];
    top[st[d]] = d;
  }
}

__device__ __forceinline__ void store_obs(float* o, int n, const uint8_t* st) {
  for (int d = 0; d < n; ++d) {
    o[3 * d + 0] = st[d] == 0 ? 1.0f : 0.0f;
    o[3 * d + 1] = st[d] == 1 ? 1.0f : 0.0f;
    o[3 * d + 2] = st[d] == 2 ? 1.0f : 0.0f;
  }
}

__global__ void mzh_env_step_kernel(int n, int goal_peg, int max_steps, int B, uint8_t* state,
                                    const int32_t* action, uint8_t* moved, float* obs, int8_t* reward,
                                    uint8_t* done, uint8_t* illegal, int32_t* step_ctr, uint8_t* active,
                                    int32_t* err_count) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint8_t st[MZH_MAXN];
  int top[3];
  load_state(state + (size_t)b * n, n, st, top);
  const int a = action[b];
  int8_t code;
  uint8_t dn = 0, ill = 0;
  if (!active[b] || a < 0 || a >= 6) {
    // assert self.reset_check (hanoi.py:49) / moves[action] IndexError: env left untouched
    code = -2;
    if (err_count) atomicAdd(err_count, 1);
  } else {
    int ctr = step_ctr[b];
    bool advanced;
    code = env_transition(n, goal_peg, max_steps, a, st, top, state + (size_t)b * n, active + b, ctr, dn, ill,
                          advanced);
    step_ctr[b] = ctr;
  }
  reward[b] = code;
  done[b] = dn;
  illegal[b] = ill;
  if (moved)
    for (int d = 0; d < n; ++d) moved[(size_t)b * n + d] = st[d];
  if (obs) store_obs(obs + (size_t)b * 3 * n, n, st);
}

// Execute each row's plan open loop (planning_multiple_actions.py:139-178): row j is env env_index[j]
// (j without env_index) of the full batch and applies plan[j * plan_stride + k] for
// k < min(plan_len[j], max_plan_len) while its env is active.  Entries at or beyond plan_len[j] are never
// read.  An env inactive on entry is left untouched (executed 0, no error).  Errors (plan_len < 1 on an
// active env, an action outside 0..5 at a position that would execute, an env index outside the batch)
// add to err_count and end the row's execution for the call.
__global__ void mzh_env_run_plan_kernel(mzh_plan_args p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n) return;
  const int n = p.n_disks, L = p.max_plan_len;
  const int e = p.env_index ? p.env_index[j] : j;
  int ex = 0;
  bool err = false;
  if (e < 0 || e >= p.B) {
    err = true;
  } else if (p.active[e]) {
    const int len = p.plan_len[j];
    if (len < 1) {
      err = true;
    } else {
      const int k_max = len < L ? len : L;
      const int32_t* pl = p.plan + (size_t)j * p.plan_stride;
      uint8_t* sp = p.state + (size_t)e * n;
      uint8_t st[MZH_MAXN];
      int top[3];
      load_state(sp, n, st, top);
      int ctr = p.step_ctr[e], ill_n = 0;
      uint8_t dn = 0;
      while (ex < k_max && !dn) {
        const int a = pl[ex];
        if (a < 0 || a >= 6) {  // moves[action] IndexError
          err = true;
          break;
        }
        uint8_t ill;
        bool advanced;
        const int8_t code = env_transition(n, p.goal_peg, p.max_steps, a, st, top, sp, p.active + e, ctr, dn, ill,
                                           advanced);
        if (advanced) {
          top[0] = top[1] = top[2] = n;
          for (int d = n - 1; d >= 0; --d) top[st[d]] = d;
        }
        if (p.rec_action) p.rec_action[(size_t)ex * p.n + j] = a;
        if (p.rec_reward) p.rec_reward[(size_t)ex * p.n + j] = code;
        ill_n += ill;
        ++ex;
      }
      if (ex > 0) {  // st: the last executed step's moved state, what env.step returned last
        store_obs(p.obs + (size_t)e * 3 * n, n, st);
        p.step_ctr[e] = ctr;
        p.steps_total[e] += ex;
        p.illegal_total[e] += ill_n;
      }
    }
  }
  if (err && p.err_count) atomicAdd(p.err_count, 1);
  p.executed[j] = ex;
  for (int k = ex; k < L; ++k) {
    if (p.rec_action) p.rec_action[(size_t)k * p.n + j] = -1;
    if (p.rec_reward) p.rec_reward[(size_t)k * p.n + j] = 0;
  }
}

// Step the true env and write the observation the model is to see (noise_injection_comparison.py:17-37,
// permutation_importance.py:27-76): row j is env env_index[j] (j without env_index) of the full batch.  An env
// inactive on entry is left untouched.  With `action` the env takes one step (tallied in steps_total /
// illegal_total / solved); if it is still active afterwards its obs row becomes one-hot(c_state with disc
// perm_disc's peg replaced by perm_peg[j]) + noise[j], the float64 sum rounded once to float32.  An error (env
// index outside the batch; on an active env a bad action, perm_disc, or needed perm_peg) adds to err_count and
// skips the row.  The obs stores of consecutive lanes are 12 * n_disks bytes apart at scattered envs; they are
// not staged through LDS: no measurement says they matter next to the search that reads them.
__global__ void mzh_env_step_observe_kernel(mzh_observe_args p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n) return;
  const int n = p.n_disks;
  const int e = p.env_index ? p.env_index[j] : j;
  int8_t code = 0;
  uint8_t dn = 0;
  bool err = false;
  if (e < 0 || e >= p.B) {
    err = true;
  } else if (p.active[e]) {
    const int pd = p.perm_disc ? p.perm_disc[e] : -1;
    const int a = p.action ? p.action[j] : 0;
    int pp = 0;
    if (pd < -1 || pd >= n) {
      err = true;
    } else if (pd >= 0) {
      pp = p.perm_peg[j];
      err = pp < 0 || pp > 2;
    }
    err = err || a < 0 || a >= 6;  // moves[action] IndexError
    if (!err) {
      uint8_t* sp = p.state + (size_t)e * n;
      uint8_t st[MZH_MAXN];
      int top[3];
      load_state(sp, n, st, top);
      if (p.action) {
        int ctr = p.step_ctr[e];
        uint8_t ill;
        bool advanced;
        code = env_transition(n, p.goal_peg, p.max_steps, a, st, top, sp, p.active + e, ctr, dn, ill, advanced);
        p.step_ctr[e] = ctr;
        p.steps_total[e] += 1;
        p.illegal_total[e] += ill;
        if (code == 1) p.solved[e] = 1;
      }
      if (!dn) {  // st == c_state here: it differs from c_state only on the goal step, which ends the episode
        float* o = p.obs + (size_t)e * 3 * n;
        const double* z = p.noise ? p.noise + (size_t)j * 3 * n : nullptr;
        for (int d = 0; d < n; ++d) {
          const int peg = d == pd ? pp : st[d];
          for (int k = 0; k < 3; ++k) {
            const double hot = peg == k ? 1.0 : 0.0;
            o[3 * d + k] = z ? (float)(hot + z[3 * d + k]) : (float)hot;
          }
        }
      }
    }
  }
  if (err && p.err_count) atomicAdd(p.err_count, 1);
  if (p.reward) p.reward[j] = code;
  if (p.done) p.done[j] = dn;
}

__global__ void mzh_legal_mask_kernel(int n, int B, const uint8_t* state, uint8_t* mask) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  mask[b] = mzh_legal_mask_row(state + (size_t)b * n, n);
}

__global__ void mzh_encode_obs_kernel(int n, int B, const uint8_t* state, float* obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // one lane per (env, disc)
  if (i >= B * n) return;
  const uint8_t s = state[i];
  float* o = obs + (size_t)i * 3;
  o[0] = s == 0 ? 1.0f : 0.0f;
  o[1] = s == 1 ? 1.0f : 0.0f;
  o[2] = s == 2 ? 1.0f : 0.0f;
}

__global__ void mzh_hanoi_solver_kernel(int n, int goal_peg, int B, const uint8_t* state, int32_t* moves) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint8_t* st = state + (size_t)b * n;
  int32_t m = 0;
  int target = goal_peg;
  for (int i = n - 1; i >= 0; --i) {  // env/hanoi_utils.py:18-24
    if (st[i] != target) {
      m += 1 << i;
      target = 3 - target - st[i];
    }
  }
  moves[b] = m;
}

static inline int nblocks(int work, int tpb) { return (work + tpb - 1) / tpb; }

hipError_t mzh_launch_env_step(int n, int goal_peg, int max_steps, int B, uint8_t* state, const int32_t* action,
                               uint8_t* moved, float* obs, int8_t* reward, uint8_t* done, uint8_t* illegal,
                               int32_t* step_ctr, uint8_t* active, int32_t* err_count, hipStream_t s) {
  hipLaunchKernelGGL(mzh_env_step_kernel, dim3(nblocks(B, 256)), dim3(256), 0, s, n, goal_peg, max_steps, B, state,
                     action, moved, obs, reward, done, illegal, step_ctr, active, err_count);
  return hipGetLastError();
}

hipError_t mzh_launch_env_run_plan(const mzh_plan_args* args, hipStream_t s) {
  hipLaunchKernelGGL(mzh_env_run_plan_kernel, dim3(nblocks(args->n, 256)), dim3(256), 0, s, *args);
  return hipGetLastError();
}

hipError_t mzh_launch_env_step_observe(const mzh_observe_args* args, hipStream_t s) {
  hipLaunchKernelGGL(mzh_env_step_observe_kernel, dim3(nblocks(args->n, 256)), dim3(256), 0, s, *args);
  return hipGetLastError();
}

hipError_t mzh_launch_legal_mask(int n, int B, const uint8_t* state, uint8_t* mask, hipStream_t s) {
  hipLaunchKernelGGL(mzh_legal_mask_kernel, dim3(nblocks(B, 256)), dim3(256), 0, s, n, B, state, mask);
  return hipGetLastError();
}

hipError_t mzh_launch_encode_obs(int n, int B, const uint8_t* state, float* obs, hipStream_t s) {
  hipLaunchKernelGGL(mzh_encode_obs_kernel, dim3(nblocks(B * n, 256)), dim3(256), 0, s, n, B, state, obs);
  return hipGetLastError();
}

hipError_t mzh_launch_hanoi_solver(int n, int goal_peg, int B, const uint8_t* state, int32_t* moves, hipStream_t s) {
  hipLaunchKernelGGL(mzh_hanoi_solver_kernel, dim3(nblocks(B, 256)), dim3(256), 0, s, n, goal_peg, B, state, moves);
  return hipGetLastError();
}
