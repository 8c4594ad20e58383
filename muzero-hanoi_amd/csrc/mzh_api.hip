// mzh_api.hip -- C ABI (include/mzh.h) over the gfx950 kernels, core unit: the error state, the device and stream
// helpers, mzh_create / mzh_destroy, the checks several units share, the environment and inference entry points.
// No exceptions cross the ABI; every entry point returns a status and records a thread-local message.  The other
// host units (mzh_api_weights / _memo / _search / _rows / _train.hip) share mzh_host.h with this one.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <string>

#include "mzh_env_kernels.h"
#include "mzh_host.h"

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(MZH_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

extern "C" int mzh_abi_version(void) { return MZH_ABI_VERSION; }
extern "C" const char* mzh_last_error(void) { return g_err.c_str(); }

extern "C" int mzh_device_count(int* count) {
  if (!count) return fail(MZH_ERR_ARG, "count is NULL");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  return MZH_OK;
}

extern "C" int mzh_host_device_pointer(void* host, void** dev) {
  if (!host || !dev) return fail(MZH_ERR_ARG, "host_device_pointer: NULL argument");
  *dev = nullptr;
  return hip_status(hipHostGetDevicePointer(dev, host, 0), "hipHostGetDevicePointer");
}

extern "C" int mzh_stream_synchronize(void* stream) {
  return hip_status(hipStreamSynchronize(static_cast<hipStream_t>(stream)), "hipStreamSynchronize");
}

extern "C" int mzh_create(int device, int n_disks, int max_sims, int max_roots, int support, mzh_engine** out) {
  if (!out) return fail(MZH_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (n_disks < 1 || n_disks > 16) return fail(MZH_ERR_ARG, "n_disks must be in [1,16], got %d", n_disks);
  if (max_sims < 0 || max_sims > 32000) return fail(MZH_ERR_ARG, "max_sims must be in [0,32000], got %d", max_sims);
  if (max_roots < 1) return fail(MZH_ERR_ARG, "max_roots must be >= 1, got %d", max_roots);
  if (support != 33 && support != 1) return fail(MZH_ERR_ARG, "support must be 33 or 1, got %d", support);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MZH_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(MZH_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
  MZH_ON_DEVICE(device);
  std::unique_ptr<mzh_engine> eng(new mzh_engine());
  eng->device = device;
  eng->n_disks = n_disks;
  eng->max_sims = max_sims;
  eng->max_roots = max_roots;
  eng->support = support;
  eng->in_dim = 3 * n_disks;
  eng->kin = ((eng->in_dim + 15) / 16) * 16;
  eng->E = max_sims + 1;
  // MZH_MEMO_DEPTH: the engine's initial memo depth request, as mzh_set_memo_depth reads it (measurements
  // through programs that do not call it).  A value that is no integer, or one mzh_set_memo_depth would
  // refuse, is an error: no engine is made
  if (const char* v = getenv("MZH_MEMO_DEPTH")) {
    char* end = nullptr;
    const long d = strtol(v, &end, 10);
    int D = 0;
    if (end == v || *end != '\0' || d < -1 || d > MZH_MEMO_MAX_DEPTH)
      return fail(MZH_ERR_ARG, "MZH_MEMO_DEPTH='%s': expected an integer in [-1, %d]", v, MZH_MEMO_MAX_DEPTH);
    const int st = memo_depth_for(n_disks, (int)d, &D);
    if (st) return st;
    eng->memo.want = (int)d;
  }
  // MZH_MEMO_GROW_BYTES: likewise the initial request of mzh_set_memo_grow (-1 the default budget, 0 off)
  if (const char* v = getenv("MZH_MEMO_GROW_BYTES")) {
    char* end = nullptr;
    const long long b = strtoll(v, &end, 10);
    if (end == v || *end != '\0' || b < -1 || b > MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES)
      return fail(MZH_ERR_ARG, "MZH_MEMO_GROW_BYTES='%s': expected an integer in [-1, %lld]", v,
                  MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES);
    eng->memo.grow_want = b;
  }
  const size_t nblk = (size_t)max_roots * eng->E;
  // MzhBlock (mzh_tree.h) / MzwBlock (mzh_wave.hip): one 128-B cache line per expanded node
  hipError_t e = eng->ws.tree.alloc(nblk * 128);
  if (e == hipSuccess) e = eng->ws.htree.alloc(nblk * MZH_LATENT);
  if (e == hipSuccess) e = eng->ws.pathx.alloc(nblk);
  if (e == hipSuccess) e = eng->ws.table.alloc((size_t)(max_sims + 2));
  if (e == hipSuccess) e = eng->memo.cnt.alloc(3);
  if (e == hipSuccess) e = hipMemset(eng->memo.cnt.get(), 0, eng->memo.cnt.bytes());
  if (e != hipSuccess) return hip_fail(e, "hipMalloc (engine workspace)");
  // UCB table on the host with libm, exactly the reference's python expression (node.py:114-121)
  std::vector<double> t(max_sims + 2);
  for (int n = 0; n < max_sims + 2; ++n) t[n] = (log((double)(n + 19652 + 1) / 19652.0) + 1.25) * sqrt((double)n);
  e = hipMemcpy(eng->ws.table.get(), t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy (ucb table)");
  *out = eng.release();
  return MZH_OK;
}

extern "C" int mzh_destroy(mzh_engine* eng) {
  if (!eng) return MZH_OK;
  DeviceGuard g(eng->device);
  delete eng;
  return MZH_OK;
}

// ---- the checks several units share (mzh_host.h) ----
int rows_range_check(const char* pre, int n, int B, const int32_t* env_index) {
  if (n < 1 || B < 1 || (!env_index && B < n)) return fail(MZH_ERR_ARG, "%sbad n=%d rows for B=%d envs", pre, n, B);
  return MZH_OK;
}

int multi_args_check(const char* pre, const mzh_multi_args* m) {
  if (!m->net_index) return fail(MZH_ERR_ARG, "%snet_index is NULL", pre);
  if (m->n_networks < 1 || m->n_networks > MZH_MULTI_MAX_NETS)
    return fail(MZH_ERR_ARG, "%sn_networks=%d outside [1, %d]", pre, m->n_networks, MZH_MULTI_MAX_NETS);
  return MZH_OK;
}

int multi_engine_check(const char* pre, const mzh_multi_args* m, const mzh_engine* eng) {
  if (!m) return eng->single.m ? MZH_OK : fail(MZH_ERR_STATE, "weights not loaded");
  if (eng->set.m == 0) return fail(MZH_ERR_STATE, "no weight set loaded (mzh_load_weight_set)");
  if (m->n_networks < 1 || m->n_networks > eng->set.m)
    return fail(MZH_ERR_ARG, "%sn_networks=%d outside [1, %d], the loaded set", pre, m->n_networks, eng->set.m);
  return MZH_OK;
}

// ---- environment ----
extern "C" int mzh_env_step(int n_disks, int goal_peg, int max_steps, int B, uint8_t* state, const int32_t* action,
                            uint8_t* moved, float* obs, int8_t* reward, uint8_t* done, uint8_t* illegal,
                            int32_t* step_ctr, uint8_t* active, int32_t* err_count, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || goal_peg < 0 || goal_peg > 2 || B < 0)
    return fail(MZH_ERR_ARG, "env_step: bad n_disks=%d goal_peg=%d B=%d", n_disks, goal_peg, B);
  if (B == 0) return MZH_OK;
  if (!state || !action || !reward || !done || !illegal || !step_ctr || !active)
    return fail(MZH_ERR_ARG, "env_step: required buffer is NULL");
  return hip_status(mzh_launch_env_step(n_disks, goal_peg, max_steps, B, state, action, moved, obs, reward, done, illegal,
                                        step_ctr, active, err_count, (hipStream_t)stream),
                    "env_step launch");
}

extern "C" int mzh_env_run_plan(const mzh_plan_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "env_run_plan: args is NULL");
  if (a->n_disks < 1 || a->n_disks > 32 || a->goal_peg < 0 || a->goal_peg > 2)
    return fail(MZH_ERR_ARG, "env_run_plan: bad n_disks=%d goal_peg=%d", a->n_disks, a->goal_peg);
  const int st = rows_range_check("env_run_plan: ", a->n, a->B, a->env_index);
  if (st) return st;
  if (a->max_plan_len < 1 || a->plan_stride < a->max_plan_len)
    return fail(MZH_ERR_ARG, "env_run_plan: bad max_plan_len=%d plan_stride=%d", a->max_plan_len, a->plan_stride);
  if (!a->plan || !a->plan_len || !a->state || !a->step_ctr || !a->active || !a->obs || !a->executed ||
      !a->steps_total || !a->illegal_total)
    return fail(MZH_ERR_ARG, "env_run_plan: required buffer is NULL");
  return hip_status(mzh_launch_env_run_plan(a, (hipStream_t)stream), "env_run_plan launch");
}

extern "C" int mzh_env_step_observe(const mzh_observe_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "env_step_observe: args is NULL");
  if (a->n_disks < 1 || a->n_disks > 32 || a->goal_peg < 0 || a->goal_peg > 2)
    return fail(MZH_ERR_ARG, "env_step_observe: bad n_disks=%d goal_peg=%d", a->n_disks, a->goal_peg);
  const int st = rows_range_check("env_step_observe: ", a->n, a->B, a->env_index);
  if (st) return st;
  if (!a->state || !a->step_ctr || !a->active || !a->steps_total || !a->illegal_total || !a->solved || !a->obs ||
      (a->perm_disc && !a->perm_peg))
    return fail(MZH_ERR_ARG, "env_step_observe: required buffer is NULL");
  return hip_status(mzh_launch_env_step_observe(a, (hipStream_t)stream), "env_step_observe launch");
}

extern "C" int mzh_legal_mask(int n_disks, int B, const uint8_t* state, uint8_t* mask, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || B < 0 || (B > 0 && (!state || !mask))) return fail(MZH_ERR_ARG, "legal_mask: bad args");
  if (B == 0) return MZH_OK;
  return hip_status(mzh_launch_legal_mask(n_disks, B, state, mask, (hipStream_t)stream), "legal_mask launch");
}

extern "C" int mzh_encode_obs(int n_disks, int B, const uint8_t* state, float* obs, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || B < 0 || (B > 0 && (!state || !obs))) return fail(MZH_ERR_ARG, "encode_obs: bad args");
  if (B == 0) return MZH_OK;
  return hip_status(mzh_launch_encode_obs(n_disks, B, state, obs, (hipStream_t)stream), "encode_obs launch");
}

extern "C" int mzh_hanoi_solver(int n_disks, int goal_peg, int B, const uint8_t* state, int32_t* moves, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 30 || goal_peg < 0 || goal_peg > 2 || B < 0 || (B > 0 && (!state || !moves)))
    return fail(MZH_ERR_ARG, "hanoi_solver: bad args");
  if (B == 0) return MZH_OK;
  return hip_status(mzh_launch_hanoi_solver(n_disks, goal_peg, B, state, moves, (hipStream_t)stream), "hanoi_solver launch");
}

// ---- inference ----
// roots (rows) per workgroup of the standalone inference kernels: 16 while that fits one workgroup
// per CU (B <= 4096), else 32
int pick_rows(int B) { return B > 256 * 16 ? 32 : 16; }

// both forms: recurrent with `action` (x the latents), else initial (x the observations)
static int inference(mzh_engine* eng, const char* who, const char* what, MzhInferParams p, bool bad, mzh_stream stream) {
  if (!eng) return fail(MZH_ERR_ARG, "engine NULL");
  if (!eng->single.m) return fail(MZH_ERR_STATE, "weights not loaded");
  if (p.B < 0 || (p.B > 0 && bad)) return fail(MZH_ERR_ARG, "%s: bad args", who);
  if (p.B == 0) return MZH_OK;
  MZH_ON_DEVICE(eng->device);
  p.in_dim = eng->in_dim; p.kin = eng->kin;
  return hip_status(mzh_launch_infer(pick_rows(p.B), p.action != nullptr, eng->single.net, p, (hipStream_t)stream), what);
}

extern "C" int mzh_initial_inference(mzh_engine* eng, int B, const float* obs, float* h, float* reward, float* pi,
                                     float* value, float* policy_logits, float* value_logits, mzh_stream stream) {
  MzhInferParams p{};
  p.B = B; p.x = obs; p.h = h; p.reward = reward; p.pi = pi;
  p.value = value; p.policy_logits = policy_logits; p.value_logits = value_logits;
  return inference(eng, "initial_inference", "initial_inference launch", p, !obs || !h, stream);
}

extern "C" int mzh_recurrent_inference(mzh_engine* eng, int B, const float* h_in, const int32_t* action, float* h,
                                       float* reward, float* pi, float* value, float* policy_logits,
                                       float* value_logits, float* reward_logits, mzh_stream stream) {
  MzhInferParams p{};
  p.B = B; p.x = h_in; p.action = action; p.h = h; p.reward = reward;
  p.pi = pi; p.value = value; p.policy_logits = policy_logits; p.value_logits = value_logits;
  p.reward_logits = reward_logits;
  return inference(eng, "recurrent_inference", "recurrent_inference launch", p, !h_in || !action || !h, stream);
}
