// mzh_ingest.hip -- a batch of lockstep self-play episodes into the replay ring, on the device: the
// bookkeeping between BatchedSelfPlay.play and Buffer.add (utils.compute_n_step_returns, selfplay._bookkeeping,
// utils.organise_transitions, the success filter of Muzero.training_loop, buffer.py:62-77) for TD_return=True,
// from the device-resident record [T][B][...] straight to ring rows and priorities.
//
// Two launches.
//  plan   one workgroup: per env the filter (float32(return of the last step) > 0) and an exclusive scan of
//         the entering episodes' lengths in env order, 1,024 envs per pass with the running sum carried,
//         so every entering episode knows the sequential position g0 of its first row; status = {code, G}.
//  write  one workgroup per env (those that do not enter leave at once): row t of the episode is transition
//         g0 + t of G and lands at (ptr + g0 + t) % size.  An episode's rows are consecutive ring rows (apart
//         from the wrap), so the workgroup walks the flattened elements of each of the five arrays and of the
//         priorities: consecutive lanes store consecutive addresses, 256 B (512 B for the int64 actions) per
//         wave instruction.  A row with g < G - size is skipped: in the sequential order a later row of this
//         call overwrites it, so every ring element has exactly one writer and the scatter needs no atomics.
//
// Numerics: the n-step return is the reference's float64 chain -- 0 + d^0 r_t + d^1 r_{t+1} + ... left to
// right, then + d^n rootQ_{t+n}, products and sums rounded separately (-ffp-contract=off), the powers d^i
// computed by the Python host -- rounded to float32 once; the priority |float32(ret) - float32(rootQ)| is a
// float32 subtraction, as NumPy's.  Rewards and root values at or beyond steps[b] are 0 by the episode's
// length, whatever the record holds there, and nothing is read at t >= T.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mzh_train.h"

namespace {

constexpr int PT = 1024;  // threads of the plan workgroup = envs per scan pass
constexpr int PW = PT / 64;
constexpr int WT = 256;    // threads of a writer workgroup
constexpr int TILE = 1024; // steps of an episode whose per-step values sit in LDS at once

// one float64 through DPP (both halves); the wave scan of mzh_replay.hip: row_shr 1, 2, 4, 8 within rows of
// 16, then row_bcast 15 / 31.  The values scanned here are episode lengths (integers far below 2^53: exact).
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __double_as_longlong(v);
  int lo, hi;
  if (ROWS == 0xF) {
    lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, ROWS, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, ROWS, 0xF, true);
  } else {
    lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROWS, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWS, 0xF, false);
  }
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__device__ __forceinline__ double wave_scan(double v) {
  v += dpp_f64<0x111, 0xF>(v);
  v += dpp_f64<0x112, 0xF>(v);
  v += dpp_f64<0x114, 0xF>(v);
  v += dpp_f64<0x118, 0xF>(v);
  v += dpp_f64<0x142, 0xA>(v);
  v += dpp_f64<0x143, 0xC>(v);
  return v;
}

// float32 of compute_n_step_returns' value for step t of env b (an episode of n <= T steps)
__device__ __forceinline__ float nstep_return(const mzh_ingest_args& a, int b, int t, int n) {
  double s = 0.0;
  for (int i = 0; i < a.n_step; ++i) {
    const long long tt = (long long)t + i;
    const double r = tt < n ? a.reward[(size_t)tt * a.B + b] : 0.0;
    const double term = a.disc_pow[i] * r;
    s = s + term;
  }
  const long long tb = (long long)t + a.n_step;
  const double q = tb < n ? a.root_q[(size_t)tb * a.B + b] : 0.0;
  const double boot = a.disc_pow[a.n_step] * q;
  s = s + boot;
  return (float)s;
}

__global__ __launch_bounds__(PT) void ingest_plan_kernel(mzh_ingest_args a) {
  __shared__ double wtot[PW];
  __shared__ double wpre[PW + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double carry = 0.0;
  int bad = 0, big = 0;
  for (int c0 = 0; c0 < a.B; c0 += PT) {
    const int b = c0 + tid;
    int len = 0;
    if (b < a.B) {
      const int n = a.steps[b];
      if (n < 1 || n > a.T) {
        bad = 1;
      } else if (nstep_return(a, b, n - 1, n) > 0.0f) {  // only successful episodes enter the buffer
        len = n;
        if ((long long)n > a.size) big = 1;
      }
    }
    const double v = wave_scan((double)len);
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    if (wave == 0) {
      const double t = lane < PW ? wtot[lane] : 0.0;
      const double s = wave_scan(t);
      if (lane < PW) wpre[lane] = s - t;  // exclusive
      if (lane == 63) wpre[PW] = s;
    }
    __syncthreads();
    if (b < a.B) a.first[b] = len > 0 ? (long long)(carry + wpre[wave] + v) - len : -1;
    carry += wpre[PW];
    __syncthreads();  // wtot / wpre are rewritten by the next pass
  }
  bad = __syncthreads_or(bad);
  big = __syncthreads_or(big);
  if (tid == 0) {
    a.status[0] = bad ? 2 : (big ? 1 : 0);
    a.status[1] = (long long)carry;
  }
}

__global__ __launch_bounds__(WT) void ingest_write_kernel(mzh_ingest_args a) {
  __shared__ float s_ret[TILE];
  __shared__ float s_rwd[TILE];
  __shared__ int s_act[TILE];
  if (a.status[0] != 0) return;  // the reference's assert n <= size (or a malformed record): nothing is written
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long g0 = a.first[b];
  if (g0 < 0) return;
  const int n = a.steps[b], B = a.B, U = a.U, A = a.A, D = a.d_state;
  const long long G = a.status[1], size = a.size;
  const long long skip = G > size ? G - size : 0;  // rows g < skip are overwritten by later rows of this call
  // the episode's first row that stays, and the ring row of step 0 (may be "negative": only t >= ts is used)
  const int ts = skip > g0 ? (int)(skip - g0 < n ? skip - g0 : n) : 0;
  const long long r0 = (a.ptr + g0) % size;
  const long long pad = a.pad_action[b];
  const float absorbing = (float)(1.0 / (double)A);
  auto ring = [&](int t) { return (size_t)((r0 + t) % size); };
  for (int t0 = ts; t0 < n; t0 += TILE) {
    const int hi = min(n, t0 + TILE), nt = hi - t0;  // steps [t0, hi): this pass's rows, their values in LDS
    __syncthreads();
    for (int i = tid; i < nt; i += WT) {
      const int t = t0 + i;
      s_ret[i] = nstep_return(a, b, t, n);
      s_rwd[i] = (float)a.reward[(size_t)t * B + b];
      s_act[i] = a.action[(size_t)t * B + b];
    }
    __syncthreads();
    auto ret_at = [&](int t) { return t >= n ? 0.0f : (t < hi ? s_ret[t - t0] : nstep_return(a, b, t, n)); };
    auto rwd_at = [&](int t) { return t >= n ? 0.0f : (t < hi ? s_rwd[t - t0] : (float)a.reward[(size_t)t * B + b]); };
    auto act_at = [&](int t) {
      return t >= n ? pad : (long long)(t < hi ? s_act[t - t0] : a.action[(size_t)t * B + b]);
    };
    // priorities and states: one source step per row
    for (int i = tid; i < nt; i += WT) {
      const int t = t0 + i;
      a.prio[ring(t)] = __builtin_fabsf(s_ret[i] - (float)a.root_q[(size_t)t * B + b]);
    }
    for (int e = tid; e < nt * D; e += WT) {
      const int i = e / D, j = e - i * D, t = t0 + i;
      a.states[ring(t) * D + j] = a.obs[((size_t)t * B + b) * D + j];
    }
    // the unroll windows: element (t, k) from step t + k, the absorbing values past the episode's end
    for (int e = tid; e < nt * U; e += WT) {
      const int i = e / U, k = e - i * U, t = t0 + i;
      const size_t o = ring(t) * U + k;
      const long long tk = (long long)t + k;
      const int tq = tk < n ? (int)tk : n;
      a.rwds[o] = rwd_at(tq);
      a.returns[o] = ret_at(tq);
      a.actions[o] = act_at(tq);
    }
    const int UA = U * A;
    for (int e = tid; e < nt * UA; e += WT) {
      const int i = e / UA, w = e - i * UA, k = w / A, j = w - k * A, t = t0 + i;
      const long long tk = (long long)t + k;
      a.pi_probs[ring(t) * UA + w] = tk < n ? (float)a.pi[((size_t)tk * B + b) * A + j] : absorbing;
    }
  }
}

}  // namespace

hipError_t mzi_launch_ingest(const mzh_ingest_args& a, hipStream_t stream) {
  hipLaunchKernelGGL(ingest_plan_kernel, dim3(1), dim3(PT), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ingest_write_kernel, dim3(a.B), dim3(WT), 0, stream, a);
  return hipGetLastError();
}
