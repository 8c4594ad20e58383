// mzh_api_rows.hip -- the calls over rows of a sub-batch: mzh_probe_actions, mzh_saliency, mzh_param_grads.  Each
// serves the engine's own network (multi == NULL) or the loaded set, and picks that record once.
#include "mzh_host.h"

// What all three refuse, in this order: what the arguments alone decide first (those refusals need neither a device
// nor an engine), then the engine, its weights or set, its capacity.  `pre` opens the text ("call: "); have / need:
// whether the call's required buffers are there, and their names.
static int rows_check(const char* pre, int B, int n, const int32_t* env_index, uint32_t flags, bool have, const char* need,
                      const mzh_multi_args* m, const mzh_engine* eng) {
  int st = rows_range_check(pre, n, B, env_index);
  if (st) return st;
  if (!have) return fail(MZH_ERR_ARG, "%srequired buffer is NULL (%s)", pre, need);
  if (flags & ~(MZH_FLAG_COOP_TILE16 | MZH_FLAG_COOP_TILE32))
    return fail(MZH_ERR_ARG, "%sflags=0x%x, only MZH_FLAG_COOP_TILE16 / 32 apply", pre, flags);
  if (m && (st = multi_args_check(pre, m)) != MZH_OK) return st;
  if (!eng) return fail(MZH_ERR_ARG, "%sengine NULL", pre);
  if ((st = multi_engine_check(pre, m, eng)) != MZH_OK) return st;
  if (n > eng->max_roots) return fail(MZH_ERR_CAPACITY, "%sn=%d > max_roots=%d", pre, n, eng->max_roots);
  return MZH_OK;
}

// the fields every row call's parameter block starts with (mzh_probe_args, mzh_saliency_args, mzh_pgrad_args)
template <class P, class ARGS>
static void row_params(P& p, const mzh_engine* eng, const ARGS* a) {
  p.B = a->B; p.n = a->n; p.in_dim = eng->in_dim; p.kin = eng->kin; p.n_disks = eng->n_disks;
  p.env_index = a->env_index; p.obs = a->obs; p.err_count = a->err_count;
}

// The six one-step lookaheads of a batch of roots in one launch (mzh_probe_kernel; with `m` the rows of a loaded
// network set, mzh_probe_multi_kernel)
extern "C" int mzh_probe_actions(mzh_engine* eng, const mzh_probe_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "probe_actions: args is NULL");
  const int st = rows_check("probe_actions: ", a->B, a->n, a->env_index, a->flags,
                            a->obs && a->reward && a->value && (!a->legal || a->state),
                            "obs, reward, value; state for legal", m, eng);
  if (st) return st;
  MZH_ON_DEVICE(eng->device);
  const MzhWeights& w = m ? eng->set : eng->single;
  MzhProbeParams p{};
  row_params(p, eng, a);
  p.state = a->state; p.reward = a->reward; p.value = a->value;
  p.legal = a->legal; p.h0 = a->h0; p.pi0 = a->pi0; p.value0 = a->value0; p.h1 = a->h1; p.pi1 = a->pi1;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  return hip_status(mzh_launch_probe(pick_tile(a->n, a->flags), w.net, p, m ? &mp : nullptr, (hipStream_t)stream),
                    "probe_actions launch");
}

// Input saliency of the policy and value heads of a batch of rows in one launch (mzh_saliency_kernel; with `m` the
// rows of a loaded network set, mzh_saliency_multi_kernel)
extern "C" int mzh_saliency(mzh_engine* eng, const mzh_saliency_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "saliency: args is NULL");
  const int st = rows_check("saliency: ", a->B, a->n, a->env_index, a->flags, a->obs && a->sal_policy && a->sal_value,
                            "obs, sal_policy, sal_value", m, eng);
  if (st) return st;
  MZH_ON_DEVICE(eng->device);
  const MzhWeights& w = m ? eng->set : eng->single;
  MzhSalParams p{};
  row_params(p, eng, a);
  p.logit_index = a->logit_index;
  p.sal_policy = a->sal_policy; p.sal_value = a->sal_value; p.picked = a->picked;
  p.disc_policy = a->disc_policy; p.disc_value = a->disc_value;
  p.h0 = a->h0; p.pi0 = a->pi0; p.value0 = a->value0;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  return hip_status(mzh_launch_saliency(pick_tile(a->n, a->flags), w.net, w.tnet, p, m ? &mp : nullptr, (hipStream_t)stream),
                    "saliency launch");
}

// w.grad (MzhPackedG), current for the weights loaded in w: the map once per engine, the buffer once per size, the
// gather once per load, on `stream` ahead of the kernel that reads it
static int pgrad_ensure(mzh_engine* eng, MzhWeights& w, hipStream_t stream) {
  if (w.grad_valid) return MZH_OK;
  auto& g = eng->pgrad;
  if (!g.maps) {
    std::unique_ptr<MzhPgradMap> m(new MzhPgradMap());
    if (!mzh_pgrad_map(eng->in_dim, eng->support, m.get())) return fail(MZH_ERR_STATE, "param_grads: no gather map for this shape");
    g.maps = std::move(m);
  }
  const std::vector<int32_t>& src = g.maps->src;
  const size_t n = src.size();
  // every source lies inside one network's main blob: the gather's reads stay in bounds
  const size_t blob = w.stride ? w.stride / sizeof(float) : w.main.count();
  for (size_t j = 0; j < n; ++j)
    if (src[j] >= 0 && (size_t)src[j] >= blob) return fail(MZH_ERR_STATE, "param_grads: gather map entry %zu out of range", j);
  if (!g.map.get()) {
    DevBuf<int32_t> d;
    HIP_OK(d.alloc(n));
    hipError_t e = hipMemcpy(d.get(), src.data(), d.bytes(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy (gather map)");
    g.map = std::move(d);
    g.stride = (n + 63) & ~(size_t)63;
  }
  if (w.grad.count() != (size_t)w.m * g.stride) {  // none yet, or a set reloaded with another M
    if (w.grad.get()) {
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(w.grad.reset());
    }
    HIP_OK(w.grad.alloc((size_t)w.m * g.stride));
  }
  hipError_t e = mzh_launch_pgrad_gather(g.map.get(), (int)n, w.main.get(), w.stride / sizeof(float), w.grad.get(), g.stride,
                                         w.m, stream);
  if (e != hipSuccess) return hip_fail(e, "param_grads gather launch");
  w.grad_valid = true;
  return MZH_OK;
}

// Parameter gradients of the five sub-networks of a batch of rows (mzh_pgrad_kernel; with `m` the rows of a loaded
// network set, mzh_pgrad_multi_kernel; with args.grad then mzh_pgrad_expand_kernel)
extern "C" int mzh_param_grads(mzh_engine* eng, const mzh_pgrad_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "param_grads: args is NULL");
  int st = rows_check("param_grads: ", a->B, a->n, a->env_index, a->flags,
                      a->obs && a->action && a->delta1 && a->delta2 && a->act && a->h0 && a->z1,
                      "obs, action, delta1, delta2, act, h0, z1", m, eng);
  if (st) return st;
  MZH_ON_DEVICE(eng->device);
  MzhWeights& w = m ? eng->set : eng->single;
  st = pgrad_ensure(eng, w, (hipStream_t)stream);
  if (st) return st;
  const auto& lay = eng->pgrad.maps->layout;
  MzhPgNetT gt{};
  gt.base = reinterpret_cast<const float4*>(w.grad.get());
  for (int i = 0; i < MZH_G_LAYERS; ++i) gt.off[i] = (int)(lay.off[i] / 4);
  gt.kb_rwd2 = lay.kb[MZH_G_RWD2];
  gt.stride = eng->pgrad.stride * sizeof(float);
  MzhPgradParams p{};
  row_params(p, eng, a);
  p.action = a->action; p.policy_logit = a->policy_logit;
  p.delta1 = a->delta1; p.delta2 = a->delta2; p.act = a->act; p.h0 = a->h0; p.z1 = a->z1; p.h1 = a->h1;
  p.pi0 = a->pi0; p.value0 = a->value0; p.reward = a->reward; p.objective = a->objective; p.grad = a->grad;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  return hip_status(mzh_launch_pgrad(pick_tile(a->n, a->flags), w.net, w.tnet, gt, p, eng->support, m ? &mp : nullptr,
                                     (hipStream_t)stream),
                    "param_grads launch");
}
