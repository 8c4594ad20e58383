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
