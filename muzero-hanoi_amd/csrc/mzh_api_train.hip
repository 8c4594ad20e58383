// mzh_api_train.hip -- the fused training update (mzh_train.hip), the replay draw and priority write-back
// (mzh_replay.hip), one update round of a network set (mzh_train_set_*), and the episode ingest (mzh_ingest.hip).
#include <string>

#include "mzh_host.h"
#include "mzh_train.h"

namespace {
struct TrainLayout {
  size_t off[22];
  size_t total;  // floats
};
// scratch regions in MztScratch order, each 256-B aligned
TrainLayout train_layout(int B, int U, int support) {
  const size_t BU = (size_t)B * U, ldg = support > 1 ? 48 : 16;
  const size_t sz[] = {(size_t)B * 32, (size_t)B * 256, BU * 64, BU * 256, BU * 256, BU * 256, BU * 256, BU * 64,
                       (size_t)B * 256, (size_t)B * 64, BU * 256, BU * 256, BU * 256, BU * 256, BU * 16, BU * ldg,
                       BU * ldg, BU * 64};
  TrainLayout L{};
  size_t o = 0;
  for (int i = 0; i < 18; ++i) {
    L.off[i] = o;
    o += (sz[i] + 63) & ~(size_t)63;
  }
  L.total = o;
  return L;
}
int train_rows(const mzh_train_args* a) {
  if (a->rows > 0) return a->rows;
  const char* env = getenv("MZH_TRAIN_ROWS");
  if (env) return atoi(env);
  return 1;  // one transition per workgroup: B workgroups (fastest at batch 256, MI355X)
}
}  // namespace

extern "C" int mzh_train_scratch_bytes(int B, int U, int in_dim, int support, size_t* bytes) {
  if (B < 1 || U < 1 || in_dim < 1 || in_dim > 32 || (support != 1 && support != 33) || !bytes)
    return fail(MZH_ERR_ARG, "train_scratch_bytes: bad B=%d U=%d in_dim=%d support=%d", B, U, in_dim, support);
  *bytes = train_layout(B, U, support).total * sizeof(float);
  return MZH_OK;
}

static int train_check(const mzh_train_args* a, bool need_batch) {
  if (!a) return fail(MZH_ERR_ARG, "train: null args");
  if (a->B < 1 || a->U < 1 || a->in_dim < 1 || a->in_dim > 32 || (a->support != 1 && a->support != 33))
    return fail(MZH_ERR_ARG, "train: bad B=%d U=%d in_dim=%d support=%d", a->B, a->U, a->in_dim, a->support);
  for (int i = 0; i < 20; ++i)
    if (!a->param[i] || (need_batch && (!a->exp_avg[i] || !a->exp_avg_sq[i])))
      return fail(MZH_ERR_ARG, "train: null parameter / Adam state pointer %d", i);
  for (int i = 0; i < 10; ++i)
    if (!a->wt[i]) return fail(MZH_ERR_ARG, "train: null transposed weight %d", i);
  if (!need_batch) return MZH_OK;
  if (!a->obs || !a->rwds || !a->actions || !a->pi || !a->returns || !a->row_loss || !a->scratch)
    return fail(MZH_ERR_ARG, "train: null batch / output / scratch pointer");
  if (a->scratch_bytes < train_layout(a->B, a->U, a->support).total * sizeof(float))
    return fail(MZH_ERR_ARG, "train: scratch of %zu bytes is too small", a->scratch_bytes);
  const int R = train_rows(a);
  if (R != 1 && R != 2) return fail(MZH_ERR_ARG, "train: rows must be 1 or 2 (got %d)", R);
  if (R * a->U > 64) return fail(MZH_ERR_ARG, "train: rows * U = %d exceeds 64", R * a->U);
  if (mzt_rows_smem_bytes(R, a->U) > 160 * 1024)
    return fail(MZH_ERR_ARG, "train: U=%d needs %zu B of LDS at rows=%d", a->U, mzt_rows_smem_bytes(R, a->U), R);
  return MZH_OK;
}

extern "C" int mzh_train_transpose(const mzh_train_args* a, mzh_stream stream) {
  int st = train_check(a, false);
  if (st) return st;
  const MzhCanon dims = mzh_canon_view(nullptr, a->in_dim, a->support);
  for (int l = 0; l < 10; ++l) {
    const int out = dims.out[l], in = dims.in[l];
    hipError_t e = mzt_launch_transpose(a->param[2 * l], a->wt[l], out, in, (out + 3) & ~3, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "train transpose launch");
  }
  return MZH_OK;
}

// The two kernels' parameter blocks of one network, from its mzh_train_args (mzh_train_update launches with
// them; a set keeps them in its device table).  Returns the gradient kernel's tile count.
static int train_params(const mzh_train_args* a, MztRowParams* rp_out, MztGradParams* gp_out) {
  const int B = a->B, U = a->U, SUP = a->support;
  const TrainLayout lay = train_layout(B, U, SUP);
  float* base = (float*)a->scratch;
  MztScratch s;
  float** regions[] = {&s.x0, &s.repa, &s.h, &s.ap, &s.av, &s.ad, &s.ar, &s.hp, &s.g_rep, &s.g_h0p,
                       &s.g_p, &s.g_v, &s.g_d, &s.g_r, &s.g_lp, &s.g_lv, &s.g_lr, &s.g_hp};
  for (int i = 0; i < 18; ++i) *regions[i] = base + lay.off[i];

  float* const* P = a->param;
  MztRowParams& rp = *rp_out;
  rp.B = B;
  rp.U = U;
  rp.in_dim = a->in_dim;
  rp.obs = a->obs;
  rp.rwds = a->rwds;
  rp.pi = a->pi;
  rp.returns = a->returns;
  rp.w = a->weights;
  rp.actions = a->actions;
  rp.row_loss = a->row_loss;
  rp.new_prio = a->new_prio;
  float* const* T = a->wt;
  rp.n = MztNet{P[0],  T[0], P[1],  P[2],  T[1], P[3],  P[4],  T[2], P[5],  P[6],  T[3], P[7],
                P[8],  T[4], P[9],  P[10], T[5], P[11], P[12], T[6], P[13], P[14], T[7], P[15],
                P[16], T[8], P[17], P[18], T[9], P[19]};
  rp.s = s;

  const int BU = B * U, ldg = SUP > 1 ? 48 : 16;
  // the training-scratch facts of each layer, MztGradLayer's leading {X, ldx, GY, ldg, M}; the layer shapes
  // come from the network's table (mzh_pack.h)
  MztGradParams& gp = *gp_out;
  gp = {{{s.x0, 32, s.g_rep, 256, B},  {s.repa, 256, s.g_h0p, 64, B}, {s.h, 64, s.g_d, 256, BU},
         {s.ad, 256, s.g_hp, 64, BU},  {s.hp, 64, s.g_r, 256, BU},    {s.ar, 256, s.g_lr, ldg, BU},
         {s.h, 64, s.g_p, 256, BU},    {s.ap, 256, s.g_lp, 16, BU},   {s.h, 64, s.g_v, 256, BU},
         {s.av, 256, s.g_lv, ldg, BU}}};
  const MzhCanon dims = mzh_canon_view(nullptr, a->in_dim, SUP);
  int tiles = 0;
  for (int l = 0; l < 10; ++l) {
    MztGradLayer& L = gp.L[l];
    L.out = dims.out[l];
    L.in = dims.in[l];
    L.onehot_from = l == MZH_DYN0 ? MZH_LATENT : -1;
    L.nkb = (L.in + 15) / 16;
    L.tile0 = tiles;
    tiles += ((L.out + 15) / 16) * L.nkb;
    L.W = a->param[2 * l]; L.b = a->param[2 * l + 1];
    L.mW = a->exp_avg[2 * l]; L.mb = a->exp_avg[2 * l + 1];
    L.vW = a->exp_avg_sq[2 * l]; L.vb = a->exp_avg_sq[2 * l + 1];
    L.WT = a->wt[l];
    L.ldwt = (L.out + 3) & ~3;
  }
  gp.actions = a->actions;
  gp.step_size = a->step_size;
  gp.bc2_sqrt = a->bc2_sqrt;
  gp.beta1 = a->beta1;
  gp.beta2 = a->beta2;
  gp.eps = a->eps;
  return tiles;
}

extern "C" int mzh_train_update(const mzh_train_args* a, mzh_stream stream) {
  int st = train_check(a, true);
  if (st) return st;
  MztRowParams rp;
  MztGradParams gp;
  const int tiles = train_params(a, &rp, &gp);
  hipError_t e = mzt_launch_rows(train_rows(a), a->support, rp, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "train rows kernel launch");
  return hip_status(mzt_launch_grad_adam(gp, tiles, (hipStream_t)stream), "train grad/adam kernel launch");
}

// what mzh_replay_sample refuses of its arguments; per_call: n, u and status as well (a set takes them per round)
static int replay_check(const mzh_replay_args* a, bool per_call) {
  if (!a) return fail(MZH_ERR_ARG, "replay_sample: null args");
  if (a->n < 1 || a->m < 1 || a->m > MZR_MAX_BATCH || a->d_state < 1 || a->U < 1 || a->A < 1)
    return fail(MZH_ERR_ARG, "replay_sample: bad n=%d m=%d (1..%d) d_state=%d U=%d A=%d", a->n, a->m, MZR_MAX_BATCH,
                a->d_state, a->U, a->A);
  if (!a->prio || !a->cdf || !a->states || !a->rwds || !a->actions || !a->pi || !a->returns || !a->indx ||
      !a->out_states || !a->out_rwds || !a->out_actions || !a->out_pi || !a->out_returns ||
      (per_call && (!a->u || !a->status)))
    return fail(MZH_ERR_ARG, "replay_sample: null pointer");
  if (reinterpret_cast<uintptr_t>(a->prio) % 16 != 0)
    return fail(MZH_ERR_ARG, "replay_sample: prio must be 16-byte aligned (float4 loads)");
  return MZH_OK;
}

extern "C" int mzh_replay_sample(const mzh_replay_args* a, mzh_stream stream) {
  const int st = replay_check(a, true);
  if (st) return st;
  return hip_status(mzr_launch_sample(*a, (hipStream_t)stream), "replay sample launch");
}

extern "C" int mzh_replay_set_priorities(float* prio, int64_t size, const int64_t* indx, const float* values, int m,
                                         int32_t* status, mzh_stream stream) {
  if (!prio || !indx || !values || !status || size < 1 || m < 1)
    return fail(MZH_ERR_ARG, "replay_set_priorities: bad arguments (size=%lld m=%d)", (long long)size, m);
  return hip_status(mzr_launch_set_priorities(prio, size, indx, values, m, status, (hipStream_t)stream),
                    "replay set_priorities launch");
}

// ---------------------------------------------------------------------------------------------
// one update round of a network set in four launches (mzh.h: mzh_train_set_*)
struct mzh_train_set {
  int device = 0;
  int M = 0, B = 0, U = 0, support = 0, rows = 0, tiles = 0;
  std::vector<int32_t> ring;  // each network's ring size: the bound of a round's n
  DevBuf<unsigned char> table;  // the device table: draw[M], rows[M], grad[M], prio[M], each 256-byte aligned
  MztSetParams view{};        // the table's four arrays (step, u and status come with each call)
};

extern "C" int mzh_train_set_create(const mzh_train_args* train, const mzh_replay_args* draw, int M,
                                    mzh_train_set** out) {
  if (!out) return fail(MZH_ERR_ARG, "train_set_create: out is NULL");
  *out = nullptr;
  if (!train || !draw) return fail(MZH_ERR_ARG, "train_set_create: %s is NULL", !train ? "train" : "draw");
  if (M < 1 || M > MZH_TRAIN_SET_MAX)
    return fail(MZH_ERR_ARG, "train_set_create: M=%d outside [1, %d]", M, MZH_TRAIN_SET_MAX);
  const mzh_train_args& t0 = train[0];
  for (int m = 0; m < M; ++m) {
    const mzh_train_args& t = train[m];
    const mzh_replay_args& d = draw[m];
    int st = train_check(&t, true);
    if (st == MZH_OK) st = replay_check(&d, false);
    if (st) {
      const std::string why = mzh_last_error();
      return fail(st, "train_set_create: network %d: %s", m, why.c_str());
    }
    if (!t.new_prio) return fail(MZH_ERR_ARG, "train_set_create: network %d: new_prio is NULL (the write-back's values)", m);
    const int have[] = {t.B, t.U, t.in_dim, t.support, train_rows(&t)};
    const int want[] = {t0.B, t0.U, t0.in_dim, t0.support, train_rows(&t0)};
    const char* name[] = {"B", "U", "in_dim", "support", "rows"};
    for (int i = 0; i < 5; ++i)
      if (have[i] != want[i])
        return fail(MZH_ERR_ARG, "train_set_create: network %d: %s=%d differs from network 0's %d", m, name[i], have[i],
                    want[i]);
    if (d.m != t.B) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.m=%d != train.B=%d", m, d.m, t.B);
    if (d.d_state != t.in_dim)
      return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.d_state=%d != train.in_dim=%d", m, d.d_state, t.in_dim);
    if (d.U != t.U) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.U=%d != train.U=%d", m, d.U, t.U);
    if (d.A != 6) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.A=%d != 6", m, d.A);
    const void* outs[] = {d.out_states, d.out_rwds, d.out_actions, d.out_pi, d.out_returns};
    const void* ins[] = {t.obs, t.rwds, t.actions, t.pi, t.returns};
    const char* on[] = {"out_states", "out_rwds", "out_actions", "out_pi", "out_returns"};
    const char* in[] = {"obs", "rwds", "actions", "pi", "returns"};
    for (int i = 0; i < 5; ++i)
      if (outs[i] != ins[i])
        return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.%s is not train.%s (a network's draw feeds its own update)",
                    m, on[i], in[i]);
  }
  // ---- the device from here on
  std::unique_ptr<mzh_train_set> set(new mzh_train_set);
  set->M = M; set->B = t0.B; set->U = t0.U; set->support = t0.support; set->rows = train_rows(&t0);
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t o_draw = 0, o_rows = o_draw + up(M * sizeof(mzh_replay_args)), o_grad = o_rows + up(M * sizeof(MztRowParams)),
               o_prio = o_grad + up(M * sizeof(MztGradParams)), total = o_prio + up(M * sizeof(MzrPrioArgs));
  std::vector<unsigned char> host(total, 0);
  for (int m = 0; m < M; ++m) {
    mzh_replay_args d = draw[m];
    set->ring.push_back(d.n);
    d.n = 0; d.u = nullptr; d.status = nullptr;  // per call: the kernels take them from step, u and status
    memcpy(&host[o_draw + m * sizeof(d)], &d, sizeof(d));
    MztRowParams rp;
    MztGradParams gp;
    set->tiles = train_params(&train[m], &rp, &gp);
    gp.step_size = gp.bc2_sqrt = 0.f;  // per call
    memcpy(&host[o_rows + m * sizeof(rp)], &rp, sizeof(rp));
    memcpy(&host[o_grad + m * sizeof(gp)], &gp, sizeof(gp));
    const MzrPrioArgs pa{const_cast<float*>(draw[m].prio), (long long)draw[m].n, draw[m].indx, train[m].new_prio, train[m].B};
    memcpy(&host[o_prio + m * sizeof(pa)], &pa, sizeof(pa));
  }
  hipError_t e = hipGetDevice(&set->device);
  if (e == hipSuccess) e = set->table.alloc(total);
  if (e == hipSuccess) e = hipMemcpy(set->table.get(), host.data(), total, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = mzt_rows_set_prepare(set->rows, set->support, set->U);
  if (e != hipSuccess) return hip_fail(e, "train_set_create: device table");
  const unsigned char* base = set->table.get();
  set->view.draw = (const mzh_replay_args*)(base + o_draw);
  set->view.rows = (const MztRowParams*)(base + o_rows);
  set->view.grad = (const MztGradParams*)(base + o_grad);
  set->view.prio = (const MzrPrioArgs*)(base + o_prio);
  *out = set.release();
  return MZH_OK;
}

extern "C" int mzh_train_set_destroy(mzh_train_set* set) {
  if (!set) return MZH_OK;
  DeviceGuard g(set->device);
  delete set;
  return MZH_OK;
}

extern "C" int mzh_train_set_update(mzh_train_set* set, const mzh_train_set_step* step, const double* u, int32_t* status,
                                    mzh_stream stream) {
  if (!step) return fail(MZH_ERR_ARG, "train_set_update: step is NULL");
  if (!u) return fail(MZH_ERR_ARG, "train_set_update: u is NULL");
  if (!status) return fail(MZH_ERR_ARG, "train_set_update: status is NULL");
  if (!set) return fail(MZH_ERR_ARG, "train_set_update: set is NULL");
  int n_active = 0;
  for (int m = 0; m < set->M; ++m) {
    if (!step[m].active) continue;
    ++n_active;
    if (step[m].n < 1 || step[m].n > set->ring[m])
      return fail(MZH_ERR_ARG, "train_set_update: network %d: step.n=%d outside [1, %d], its ring", m, step[m].n,
                  set->ring[m]);
  }
  if (n_active == 0) return MZH_OK;
  MztSetParams v = set->view;
  v.step = step;
  v.u = u;
  v.status = status;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = mzr_launch_sample_set(set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: draw launch");
  e = mzt_launch_rows_set(set->rows, set->support, set->B, set->U, set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: rows kernel launch");
  e = mzt_launch_grad_adam_set(set->tiles, set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: grad/adam kernel launch");
  return hip_status(mzr_launch_set_priorities_set(set->M, v, s), "train_set_update: set_priorities launch");
}

extern "C" int mzh_episode_ingest(const mzh_ingest_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "episode_ingest: null args");
  if (a->B < 1 || a->T < 1 || a->d_state < 1 || a->U < 1 || a->A < 1 || a->n_step < 1 || a->size < 1)
    return fail(MZH_ERR_ARG, "episode_ingest: bad B=%d T=%d d_state=%d U=%d A=%d n_step=%d size=%lld (each >= 1)", a->B,
                a->T, a->d_state, a->U, a->A, a->n_step, (long long)a->size);
  // the writer indexes a pass of 1,024 rows of each array with 32-bit element counts
  if (a->d_state > (1 << 20) || (int64_t)a->U * a->A > (1 << 20))
    return fail(MZH_ERR_ARG, "episode_ingest: d_state=%d / U*A=%lld above 2^20", a->d_state, (long long)a->U * a->A);
  if (a->ptr < 0 || a->ptr >= a->size)
    return fail(MZH_ERR_ARG, "episode_ingest: ptr=%lld outside [0, size=%lld)", (long long)a->ptr, (long long)a->size);
  if (!a->obs || !a->action || !a->reward || !a->pi || !a->root_q || !a->steps || !a->pad_action || !a->disc_pow ||
      !a->states || !a->rwds || !a->actions || !a->pi_probs || !a->returns || !a->prio || !a->first || !a->status)
    return fail(MZH_ERR_ARG, "episode_ingest: null pointer");
  return hip_status(mzi_launch_ingest(*a, (hipStream_t)stream), "episode ingest launch");
}
