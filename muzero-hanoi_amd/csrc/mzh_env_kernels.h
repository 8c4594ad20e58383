// mzh_env_kernels.h -- launchers of the environment kernels (mzh_env.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

hipError_t mzh_launch_env_step(int n, int goal_peg, int max_steps, int B, uint8_t* state, const int32_t* action,
                               uint8_t* moved, float* obs, int8_t* reward, uint8_t* done, uint8_t* illegal,
                               int32_t* step_ctr, uint8_t* active, int32_t* err_count, hipStream_t s);
struct mzh_plan_args;  // include/mzh.h
hipError_t mzh_launch_env_run_plan(const mzh_plan_args* args, hipStream_t s);
struct mzh_observe_args;  // include/mzh.h
hipError_t mzh_launch_env_step_observe(const mzh_observe_args* args, hipStream_t s);
hipError_t mzh_launch_legal_mask(int n, int B, const uint8_t* state, uint8_t* mask, hipStream_t s);
hipError_t mzh_launch_encode_obs(int n, int B, const uint8_t* state, float* obs, hipStream_t s);
hipError_t mzh_launch_hanoi_solver(int n, int goal_peg, int B, const uint8_t* state, int32_t* moves, hipStream_t s);

// _move_allowed for all 6 moves of one env (env/hanoi.py:117-139) from its c_state row: bit a = move a legal,
// i.e. top[from] < top[to] with top[p] the smallest disc on peg p (n if empty) and the moves in the order
// (0,1) (0,2) (1,0) (1,2) (2,0) (2,1) (env/hanoi.py:39-41).  The three tops are scalars, not an indexed
// array, so a caller keeps them in registers (mzh_legal_mask_kernel, mzh_probe_kernel).
__device__ __forceinline__ uint8_t mzh_legal_mask_row(const uint8_t* src, int n) {
  int t0 = n, t1 = n, t2 = n;
  for (int d = n - 1; d >= 0; --d) {
    const int s = src[d];
    t0 = s == 0 ? d : t0;
    t1 = s == 1 ? d : t1;
    t2 = s == 2 ? d : t2;
  }
  return (uint8_t)((t0 < t1) | (t0 < t2) << 1 | (t1 < t0) << 2 | (t1 < t2) << 3 | (t2 < t0) << 4 | (t2 < t1) << 5);
}

// the moves' pegs; one copy per translation unit (mzh_env.hip's kernels, the episode kernel of mzh_one.hip)
__attribute__((unused)) static __constant__ int8_t kMoveFrom[6] = {0, 0, 1, 1, 2, 2};  // permutations(range(3), 2),
__attribute__((unused)) static __constant__ int8_t kMoveTo[6] = {1, 2, 0, 2, 0, 1};   // env/hanoi.py:39-41

// One TowersOfHanoi.step (hanoi.py:47-84) of an active env for a move a in 0..5.  st (in: c_state, out: the
// moved state the returned observation encodes) and top (of c_state) are the lane's registers; c_state is the
// env's row of `state` and active its reset_check byte, stored to where the reference assigns them; ctr
// (step_counter) is the caller's to load and store.  Returns the reward code (0 -> 0, 1 -> 100,
// -1 -> -100/1000) and sets dn / ill; advanced tells whether c_state moved (not on an illegal move, and not
// on the goal step, hanoi.py:65-69).
__device__ __forceinline__ int8_t env_transition(int n, int goal_peg, int max_steps, int a, uint8_t* st,
                                                 const int top[3], uint8_t* c_state, uint8_t* active, int& ctr,
                                                 uint8_t& dn, uint8_t& ill, bool& advanced) {
  const int f = kMoveFrom[a], t = kMoveTo[a];
  int8_t code;
  dn = 0;
  advanced = false;
  ill = !(top[f] < top[t]);
  ctr += 1;  // hanoi.py:61
  if (!ill) {
    const int disc = top[f];  // smallest disc on the from-peg (hanoi.py:148-150)
    st[disc] = (uint8_t)t;
    bool goal = true;
    for (int d = 0; d < n; ++d) goal = goal && (st[d] == goal_peg);
    if (!goal) {
      code = 0;
      c_state[disc] = (uint8_t)t;  // c_state = moved_state
      advanced = true;
    } else {
      code = 1;  // rwd 100, done, reset_check False, counter 0; c_state NOT advanced (hanoi.py:65-69)
      dn = 1;
      *active = 0;
      ctr = 0;
    }
  } else {
    code = -1;  // rwd -100/1000, state unchanged (hanoi.py:70-74)
  }
  if (ctr == max_steps) {  // hanoi.py:77-80
    dn = 1;
    *active = 0;
    ctr = 0;
  }
  return code;
}
