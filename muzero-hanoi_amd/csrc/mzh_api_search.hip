// mzh_api_search.hip -- the search entry points: kernel choice and plan (make_plan), mzh_search / mzh_search_replay,
// the multi-network and budget forms, and whole episodes on the latency kernel (mzh_play_episodes*).
#include <stdio.h>

#include "mzh_host.h"

// cooperative search tile: 16 roots while that is one round of workgroups (B <= 4,096), else 32
// roots (a second round of 16-root workgroups costs more than 32-root tiles).  MZH_FLAG_COOP_TILE16 /
// MZH_FLAG_COOP_TILE32 force one (tests reach both tiles' code paths at any batch size).
int pick_tile(int B, uint32_t flags) {
  if (flags & MZH_FLAG_COOP_TILE16) return 16;
  if (flags & MZH_FLAG_COOP_TILE32) return 32;
  return B > 256 * 16 ? 32 : 16;
}

static const size_t kMaxLds = 163840;

// kernel choice: the wave-independent kernel (mzh_wave.hip) with 32 roots per wave once the batch
// gives two such waves per SIMD, with 16 roots per wave for mid-size batches (>= 1024 such waves),
// else the cooperative kernel (mzh_search.hip) whose 4 waves split every MLP layer of one 16- or
// 32-root tile.  MZH_FLAG_KERNEL_* (or MZH_KERNEL=coop|wave|wave16) force one.
static const int kWaveMinRoots = 53248, kWave16MinRoots = 8193;  // measured crossovers
struct KernelChoice {
  bool wave;
  int nt;  // wave kernel: 16-root column tiles per wave
};
static KernelChoice choose_kernel(int B, uint32_t flags) {
  if (flags & MZH_FLAG_KERNEL_WAVE16) return {true, 1};
  if (flags & MZH_FLAG_KERNEL_WAVE) return {true, 2};
  if (flags & MZH_FLAG_KERNEL_COOP) return {false, 0};
  static const int forced = [] {
    const char* v = getenv("MZH_KERNEL");
    if (!v) return 0;
    return strcmp(v, "wave") == 0 ? 2 : strcmp(v, "wave16") == 0 ? 1 : strcmp(v, "coop") == 0 ? -1 : 0;
  }();
  if (forced) return forced > 0 ? KernelChoice{true, forced} : KernelChoice{false, 0};
  if (B >= kWaveMinRoots) return {true, 2};
  if (B >= kWave16MinRoots) return {true, 1};
  return {false, 0};
}

// the latency path (mzh_one.hip): MLP searches of up to kOneMaxRoots roots take one root per workgroup
// (persistent over the roots beyond the 256 workgroups of one round) while its LDS fits; a forced kernel
// flag (or MZH_KERNEL) decides otherwise.  MZH_FLAG_KERNEL_ONE forces it (an error where it cannot run).
static const int kOneMaxRoots = 512, kOneGrid = 256;  // crossover: profiles/r06_one_probe.json
static bool one_forced_env() {
  static const bool f = [] {
    const char* v = getenv("MZH_KERNEL");
    return v && strcmp(v, "one") == 0;
  }();
  return f;
}

// every template argument of the launch (MzhSearchPlan); returns a status (capacity errors)
int make_plan(int B, int S, uint32_t flags, bool replay, int support, bool has_minmax, MzhSearchPlan* pl) {
  const uint32_t forced = flags & (MZH_FLAG_KERNEL_COOP | MZH_FLAG_KERNEL_WAVE | MZH_FLAG_KERNEL_WAVE16 | MZH_FLAG_COOP_OCC2 |
                                   MZH_FLAG_COOP_TILE16 | MZH_FLAG_COOP_TILE32);
  const bool one_fits = mzh_one_smem_bytes(S, false) <= kMaxLds;
  if (flags & MZH_FLAG_KERNEL_ONE) {
    if (replay) return fail(MZH_ERR_ARG, "MZH_FLAG_KERNEL_ONE: the latency kernel has no replay (tree-only) form");
    if (forced) return fail(MZH_ERR_ARG, "MZH_FLAG_KERNEL_ONE combined with another kernel flag");
    if (!one_fits)
      return fail(MZH_ERR_CAPACITY, "MZH_FLAG_KERNEL_ONE: n_sims=%d needs %zu B of LDS", S, mzh_one_smem_bytes(S, false));
  }
  const bool env_kernel = getenv("MZH_KERNEL") != nullptr;
  if (!replay && one_fits &&
      ((flags & MZH_FLAG_KERNEL_ONE) || one_forced_env() || (!forced && !env_kernel && B <= kOneMaxRoots))) {
    MzhSearchPlan q{};
    q.one = 1;
    q.ohl = mzh_one_smem_bytes(S, true) <= kMaxLds;  // the latents in LDS where they fit
    q.sup33 = support == 33;
    q.mmin = has_minmax ? 1 : 0;
    q.grid = B < kOneGrid ? B : kOneGrid;
    *pl = q;
    return MZH_OK;
  }
  const KernelChoice kc = choose_kernel(B, flags);
  MzhSearchPlan q{};
  q.wave = kc.wave ? 1 : 0;
  q.nt = kc.nt;
  q.replay = replay ? 1 : 0;
  q.mmin = has_minmax ? 1 : 0;
  if (kc.wave) {
    if (mzh_wave_smem_bytes(S, kc.nt) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the wave kernel's LDS table budget", S);
    q.sup33 = support == 33;
    q.mmin = 0;  // the wave kernel decides the exact normaliser per selection
  } else {
    q.R = pick_tile(B, flags);
    // the two-workgroups-per-CU 16-root kernel: forced by MZH_FLAG_COOP_OCC2 (MLP searches; its LDS must
    // leave room for the second workgroup -- a search it cannot serve is an error, never a silent fallback;
    // replay searches have no occ2 instantiation and take the cooperative replay kernel, as mzh.h says)
    if ((flags & MZH_FLAG_COOP_OCC2) && !replay && 2 * mzh_search_smem_bytes(16, S, false, true) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "MZH_FLAG_COOP_OCC2: n_sims=%d needs %zu B of LDS per workgroup, more than "
                  "half a CU's", S, mzh_search_smem_bytes(16, S, false, true));
    if ((flags & MZH_FLAG_COOP_OCC2) && !replay) {
      q.R = 16;
      q.occ2 = 1;
      q.ohl = 0;
      q.sup33 = support == 33;
      *pl = q;
      return MZH_OK;
    }
    if (mzh_search_smem_bytes(q.R, S, false) > kMaxLds) q.R = 16;
    if (mzh_search_smem_bytes(q.R, S, false) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the LDS path budget", S);
    // the one-hot columns go to LDS when they fit (never in the replay kernel, which runs no MLP)
    q.ohl = !replay && mzh_search_smem_bytes(q.R, S, true) <= kMaxLds;
    q.sup33 = replay || support == 33;
  }
  *pl = q;
  return MZH_OK;
}

static void plan_info(const MzhSearchPlan& q, int B, int S, mzh_search_plan* out) {
  memset(out, 0, sizeof(*out));
  const char* tf[2] = {"false", "true"};
  out->wave = q.wave;
  if (q.one) {
    out->roots_per_wave = 1;
    out->threads_per_workgroup = 512;
    out->roots_per_workgroup = 1;
    out->smem_bytes = (int64_t)mzh_one_smem_bytes(S, q.ohl);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_one_kernel<%s, %s, %s>", tf[q.sup33], tf[q.mmin], tf[q.ohl]);
    out->workgroups = q.grid;
    return;
  }
  if (q.wave) {
    out->roots_per_wave = 16 * q.nt;
    out->threads_per_workgroup = 256;
    out->roots_per_workgroup = 4 * 16 * q.nt;
    out->smem_bytes = (int64_t)mzh_wave_smem_bytes(S, q.nt);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_wave_kernel<%d, %s, %s>", q.nt, tf[q.replay], tf[q.sup33]);
  } else if (q.occ2) {
    out->roots_per_wave = 4;
    out->threads_per_workgroup = MZH_THREADS;
    out->roots_per_workgroup = 16;
    out->smem_bytes = (int64_t)mzh_search_smem_bytes(16, S, false, true);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_occ2_kernel<%s, %s>", tf[q.sup33], tf[q.mmin]);
  } else {
    out->roots_per_wave = q.R / 4;
    out->threads_per_workgroup = MZH_THREADS;
    out->roots_per_workgroup = q.R;
    out->smem_bytes = (int64_t)mzh_search_smem_bytes(q.R, S, q.ohl);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_kernel<%d, %s, %s, %s, %s>", q.R, tf[q.replay], tf[q.ohl],
             tf[q.sup33], tf[q.mmin]);
  }
  out->workgroups = (B + out->roots_per_workgroup - 1) / out->roots_per_workgroup;
}

extern "C" int mzh_search_plan_query(int support, int B, int n_sims, uint32_t flags, int replay, int has_minmax_in,
                                     mzh_search_plan* out) {
  if (!out) return fail(MZH_ERR_ARG, "out is NULL");
  if (B < 1 || n_sims < 0 || n_sims > 32000 || (support != 33 && support != 1))
    return fail(MZH_ERR_ARG, "search_plan: bad B=%d n_sims=%d support=%d", B, n_sims, support);
  MzhSearchPlan q;
  const int st = make_plan(B, n_sims, flags, replay != 0, support, has_minmax_in != 0, &q);
  if (st) return st;
  plan_info(q, B, n_sims, out);
  return MZH_OK;
}

// the kernels' parameter block of a search call on this engine
static MzhSearchParams search_params(const mzh_engine* eng, const mzh_search_args* a) {
  MzhSearchParams p{};
  p.B = a->B; p.S = a->n_sims; p.E = eng->E; p.in_dim = eng->in_dim; p.kin = eng->kin;
  p.deterministic = a->deterministic; p.np1 = (a->flags & MZH_FLAG_NP1_UCB) ? 1 : 0;
  p.discount = a->discount; p.eps = a->eps; p.temperature = a->temperature;
  p.obs = a->obs; p.noise = a->noise; p.tie_idx = a->tie_idx; p.action_u = a->action_u; p.minmax_in = a->minmax_in;
  p.rp_root_pi = a->rp_root_pi; p.rp_sim = a->rp_sim;
  p.tree = eng->ws.tree.get(); p.htree = eng->ws.htree.get(); p.pathx = eng->ws.pathx.get(); p.table = eng->ws.table.get();
  p.visits = a->visits; p.root_q = a->root_q; p.minmax_out = a->minmax_out; p.extra_ties = a->extra_ties;
  p.action = a->action; p.pi = a->pi; p.latent = a->latent; p.latent_len = a->latent_len; p.sel_steps = a->sel_steps; p.lockstep_levels = a->lockstep_levels;
  p.pow_table = a->pow_table;
  return p;
}

// What mzh_search, mzh_search_replay and mzh_search_multi (single = false: it needs no engine network) refuse of a
// search's arguments, in this order.  *launch = false with MZH_OK: B = 0, nothing launches and the plan says so (a
// caller naming the kernel sees "none").
static int search_args_check(const mzh_engine* eng, const mzh_search_args* a, bool replay, bool single, bool* launch) {
  *launch = false;
  if (a->B < 0 || a->n_sims < 0) return fail(MZH_ERR_ARG, "B=%d n_sims=%d", a->B, a->n_sims);
  if (a->B > eng->max_roots) return fail(MZH_ERR_CAPACITY, "B=%d > max_roots=%d", a->B, eng->max_roots);
  if (a->n_sims > eng->max_sims) return fail(MZH_ERR_CAPACITY, "n_sims=%d > max_sims=%d", a->n_sims, eng->max_sims);
  if (!(a->temperature >= 0.0 && a->temperature <= 1.0))
    return fail(MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0], got %g", a->temperature);
  if (a->B == 0) {
    if (a->plan_out) {
      memset(a->plan_out, 0, sizeof(*a->plan_out));
      snprintf(a->plan_out->kernel, sizeof(a->plan_out->kernel), "none");
    }
    return MZH_OK;
  }
  if (!a->visits) return fail(MZH_ERR_ARG, "visits output is required");
  if (replay) {
    if (!a->rp_root_pi || (a->n_sims > 0 && !a->rp_sim))
      return fail(MZH_ERR_ARG, "replay search needs rp_root_pi and rp_sim");
  } else {
    if (single && !eng->single.m) return fail(MZH_ERR_STATE, "weights not loaded");
    if (!a->obs) return fail(MZH_ERR_ARG, "obs is required");
  }
  if (!a->deterministic && !a->action_u && a->action)
    return fail(MZH_ERR_ARG, "stochastic action selection needs action_u");
  *launch = true;
  return MZH_OK;
}

// the device side of a call's mzh_multi_args: the caller's net_index and status, the engine's tile workspace and set
MzhMultiParams multi_params(const mzh_engine* eng, const mzh_multi_args* m) {
  MzhMultiParams mp{};
  mp.net_index = m->net_index;
  mp.M = m->n_networks;
  mp.tiles = eng->multi.tiles.get();
  mp.ntiles = eng->multi.ntiles.get();
  mp.status = m->status;
  mp.stride = eng->set.stride;
  mp.scal = eng->set.scal();
  return mp;
}

static int search_common(mzh_engine* eng, const mzh_search_args* a, mzh_stream stream, bool replay) {
  if (!eng || !a) return fail(MZH_ERR_ARG, "engine or args NULL");
  bool launch;
  const int ck = search_args_check(eng, a, replay, true, &launch);
  if (!launch) return ck;
  MzhSearchPlan pl;
  const int st = make_plan(a->B, a->n_sims, a->flags, replay, eng->support, a->minmax_in != nullptr, &pl);
  if (st) return st;
  if (a->plan_out) plan_info(pl, a->B, a->n_sims, a->plan_out);
  MZH_ON_DEVICE(eng->device);
  MzhSearchParams p = search_params(eng, a);
  const auto& mo = eng->memo;
  bool harvest = false;
  if (pl.wave && !replay) {  // the expansion memo: wave MLP searches only, built on first use
    const int ms = memo_ensure(eng, (hipStream_t)stream);
    if (ms) return ms;
    if (mo.D > 0) {
      p.memo_h = mo.h.get(); p.memo_rec = mo.rec.get(); p.memo_cnt = mo.cnt.get();
      p.memo_D = mo.D; p.memo_K = (int)mzh_memo_nodes(mo.D);
      if (mo.cap > 0) {  // the grown extension: its links, and the miss log the harvest below reads
        const int ls = memo_log_ensure(eng);
        if (ls) return ls;
        p.memo_link = mo.link.get(); p.memo_ctr = mo.ctr.get(); p.memo_cap = (int)mo.cap;
        p.memo_log = mo.log.get(); p.memo_logn = mo.logn.get(); p.memo_logcap = mo.log_cap;
        harvest = true;
      }
    }
  }
  hipError_t e = pl.one ? mzh_launch_one(pl, eng->single.net, eng->single.onet, p, (hipStream_t)stream)
                 : pl.wave ? mzh_launch_wave_search(pl, eng->wnet, p, (hipStream_t)stream)
                           : mzh_launch_search(pl, eng->single.net, p, (hipStream_t)stream);
  if (e == hipSuccess && harvest) {
    MzhHarvestParams h{};
    h.B = p.B; h.E = p.E; h.tree = p.tree; h.htree = p.htree;
    h.log = p.memo_log; h.logn = p.memo_logn; h.logcap = p.memo_logcap;
    h.link = mo.link.get(); h.ctr = mo.ctr.get(); h.base = (int)mo.base; h.cap = (int)mo.cap;
    h.memo_h = mo.h.get(); h.memo_rec = mo.rec.get();
    e = mzh_launch_memo_harvest(h, (hipStream_t)stream);
  }
  return hip_status(e, "search launch");
}

extern "C" int mzh_search(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream) {
  return search_common(eng, args, stream, false);
}

extern "C" int mzh_search_replay(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream) {
  return search_common(eng, args, stream, true);
}

// Search over the loaded network set: root b under network net_index[b].  Cooperative kernel only (16- or
// 32-root tiles of one network each); every refusal below returns before anything is launched.
// b: the roots' own budgets (mzh_search_multi_budget), nullptr where every root runs a->n_sims
static int search_multi_common(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m, const mzh_budget_args* b,
                               mzh_stream stream) {
  if (!eng || !a || !m) return fail(MZH_ERR_ARG, "engine or args NULL");
  // this call looks at the engine first: its set bounds n_networks on both sides, so of what the block alone
  // decides only net_index is left to refuse
  int st = multi_engine_check("", m, eng);
  if (st == MZH_OK) st = multi_args_check("", m);
  if (st) return st;
  if (a->rp_sim || a->rp_root_pi) return fail(MZH_ERR_ARG, "a multi-network search has no replay (tree-only) form");
  if (a->flags & (MZH_FLAG_KERNEL_WAVE | MZH_FLAG_KERNEL_WAVE16 | MZH_FLAG_KERNEL_ONE | MZH_FLAG_COOP_OCC2))
    return fail(MZH_ERR_ARG, "a multi-network search runs the cooperative kernel only (flags=0x%x)", a->flags);
  bool launch;
  const int ck = search_args_check(eng, a, false, false, &launch);
  if (!launch) return ck;
  const int S = a->n_sims;
  MzhSearchPlan pl{};
  pl.R = pick_tile(a->B, a->flags);
  if (mzh_search_smem_bytes(pl.R, S, false) > kMaxLds) pl.R = 16;
  if (mzh_search_smem_bytes(pl.R, S, false) > kMaxLds)
    return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the LDS path budget", S);
  pl.ohl = mzh_search_smem_bytes(pl.R, S, true) <= kMaxLds;
  pl.sup33 = eng->support == 33;
  pl.mmin = 1;
  // the tile workspace holds the tiles of max_roots roots of MZH_MULTI_MAX_NETS networks at 16 roots each
  const int cap = mzh_multi_max_tiles(eng->max_roots, 16, MZH_MULTI_MAX_NETS);
  // the grid: the most tiles the batch can make, its runs (at most max_runs) in place of the networks with budgets
  const int runs = b ? b->max_runs : m->n_networks;
  const int grid = mzh_multi_max_tiles(a->B, pl.R, runs);
  if (grid > cap)
    return fail(MZH_ERR_CAPACITY, "max_runs=%d: up to %d tiles of %d roots exceed the tile workspace (%d)", runs, grid,
                pl.R, cap);
  if (a->plan_out) {
    const char* tf[2] = {"false", "true"};
    mzh_search_plan* o = a->plan_out;
    memset(o, 0, sizeof(*o));
    o->roots_per_wave = pl.R / 4;
    o->threads_per_workgroup = MZH_THREADS;
    o->roots_per_workgroup = pl.R;
    o->smem_bytes = (int64_t)mzh_search_smem_bytes(pl.R, S, pl.ohl);
    o->workgroups = grid;
    snprintf(o->kernel, sizeof(o->kernel), "mzh_search_multi_kernel<%d, %s, %s>", pl.R, tf[pl.ohl], tf[pl.sup33]);
  }
  MZH_ON_DEVICE(eng->device);
  const MzhSearchParams p = search_params(eng, a);
  hipError_t e;
  if (b) {
    MzhBudgetParams bp{};
    bp.n_sims = b->n_sims;
    bp.S = S;
    bp.max_runs = b->max_runs < a->B ? b->max_runs : a->B;
    bp.cap = cap;
    e = mzh_launch_search_multi_budget(pl, eng->set.net, p, multi_params(eng, m), bp, (hipStream_t)stream);
  } else {
    e = mzh_launch_search_multi(pl, eng->set.net, p, multi_params(eng, m), (hipStream_t)stream);
  }
  return hip_status(e, "multi search launch");
}

extern "C" int mzh_search_multi(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m, mzh_stream stream) {
  return search_multi_common(eng, a, m, nullptr, stream);
}

// The same search with root b running budget->n_sims[b] simulations (at most a->n_sims, which sizes the launch).
// What the budget block alone decides is refused first: those refusals need neither an engine nor a device.
extern "C" int mzh_search_multi_budget(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m,
                                       const mzh_budget_args* b, mzh_stream stream) {
  if (!a || !m || !b) return fail(MZH_ERR_ARG, "search_multi_budget: args, multi or budget NULL");
  if (!b->n_sims) return fail(MZH_ERR_ARG, "search_multi_budget: n_sims is NULL");
  if (b->max_runs < 1) return fail(MZH_ERR_ARG, "search_multi_budget: max_runs=%d < 1", b->max_runs);
  return search_multi_common(eng, a, m, b, stream);
}

// Whole episodes in one launch on the latency kernel (mzh.h): mzh_play_episodes (m == NULL, the engine's network)
// and mzh_play_episodes_multi (the loaded set).  The checks that need no engine come first.
// sweep: mzh_play_episodes_sweep, the set form with the envs' own budgets and discounts (w)
static int play_episodes_common(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m, bool multi,
                                mzh_stream stream, bool sweep = false, const mzh_episode_sweep_args* w = nullptr) {
  if (!a) return fail(MZH_ERR_ARG, "play_episodes: args is NULL");
  if (a->B < 1 || a->n_sims < 0) return fail(MZH_ERR_ARG, "play_episodes: B=%d n_sims=%d", a->B, a->n_sims);
  if (a->goal_peg < 0 || a->goal_peg > 2) return fail(MZH_ERR_ARG, "play_episodes: goal_peg=%d outside 0..2", a->goal_peg);
  if (a->max_steps < 1 || a->T < a->max_steps)
    return fail(MZH_ERR_ARG, "play_episodes: T=%d rows cannot hold max_steps=%d moves (T >= max_steps >= 1)", a->T,
                a->max_steps);
  if ((int64_t)a->T * a->B > 0x7fffffff)
    return fail(MZH_ERR_ARG, "play_episodes: T=%d x B=%d rows exceed int32", a->T, a->B);
  if (a->flags & ~MZH_FLAG_NP1_UCB)
    return fail(MZH_ERR_ARG, "play_episodes: flags=0x%x (only MZH_FLAG_NP1_UCB applies)", a->flags);
  if (!(a->temperature >= 0.0 && a->temperature <= 1.0))
    return fail(MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0], got %g", a->temperature);
  if (!a->state || !a->tie_idx || !a->pi || !a->root_q || !a->action || !a->reward || !a->steps || !a->illegal ||
      !a->solved || !a->final_state || !a->minmax_out)
    return fail(MZH_ERR_ARG, "play_episodes: required buffer is NULL");
  if (!a->deterministic && !a->action_u) return fail(MZH_ERR_ARG, "play_episodes: stochastic action selection needs action_u");
  if (multi) {
    if (!m) return fail(MZH_ERR_ARG, "play_episodes_multi: multi is NULL");
    const int ms = multi_args_check("play_episodes_multi: ", m);
    if (ms) return ms;
  }
  if (sweep) {
    if (!w) return fail(MZH_ERR_ARG, "play_episodes_sweep: sweep is NULL");
    if (!w->n_sims) return fail(MZH_ERR_ARG, "play_episodes_sweep: n_sims is NULL");
  }
  if (!eng) return fail(MZH_ERR_ARG, "play_episodes: engine is NULL");
  if (a->B > eng->max_roots) return fail(MZH_ERR_CAPACITY, "play_episodes: B=%d > max_roots=%d", a->B, eng->max_roots);
  if (a->n_sims > eng->max_sims) return fail(MZH_ERR_CAPACITY, "play_episodes: n_sims=%d > max_sims=%d", a->n_sims, eng->max_sims);
  MzhSearchPlan pl;  // the latency kernel's plan: its grid, the latents in LDS where they fit, or its capacity error
  int st = make_plan(a->B, a->n_sims, MZH_FLAG_KERNEL_ONE, false, eng->support, true, &pl);
  if (st == MZH_OK) st = multi_engine_check("play_episodes_multi: ", m, eng);
  if (st) return st;
  MZH_ON_DEVICE(eng->device);
  MzhSearchParams p{};
  p.B = a->B; p.S = a->n_sims; p.E = eng->E; p.in_dim = eng->in_dim; p.kin = eng->kin;
  p.deterministic = a->deterministic; p.np1 = (a->flags & MZH_FLAG_NP1_UCB) ? 1 : 0;
  p.discount = a->discount; p.eps = a->eps; p.temperature = a->temperature;
  p.noise = a->noise; p.tie_idx = a->tie_idx; p.action_u = a->action_u; p.minmax_in = a->minmax_in;
  p.htree = eng->ws.htree.get(); p.table = eng->ws.table.get();
  p.visits = a->visits; p.root_q = a->root_q; p.action = a->action; p.pi = a->pi; p.pow_table = a->pow_table;
  MzhEpisodeParams ep{};
  ep.T = a->T; ep.n_disks = eng->n_disks; ep.goal_peg = a->goal_peg; ep.max_steps = a->max_steps;
  ep.start = a->state; ep.obs = a->obs; ep.reward = a->reward; ep.steps = a->steps; ep.illegal = a->illegal;
  ep.solved = a->solved; ep.final_state = a->final_state; ep.minmax_out = a->minmax_out; ep.err_count = a->err_count;
  const MzhWeights& wt = multi ? eng->set : eng->single;
  if (!multi) return hip_status(mzh_launch_episodes(pl, wt.net, wt.onet, p, ep, (hipStream_t)stream), "play_episodes launch");
  // the device check of net_index: the tile prologue of the other multi calls with the whole batch as the tile size
  // (one tile per network that has envs, at most min(M, B): inside the table), whose count the episode kernel reads
  const MzhMultiParams mp = multi_params(eng, m);
  // (the sweep form: of the budgets too, each in [0, n_sims], by the same workgroup)
  hipError_t e = mzh_launch_multi_tiles(mp, a->B, a->B, (hipStream_t)stream, sweep ? a->n_sims : 0,
                                        sweep ? w->n_sims : nullptr);
  if (e != hipSuccess) return hip_fail(e, "play_episodes_multi net_index check launch");
  const MzhEpisodeSet es{m->net_index, mp.ntiles, wt.stride};
  if (sweep) {
    const MzhEpisodeSweep sw{w->n_sims, w->discount};
    return hip_status(mzh_launch_episodes_sweep(pl, wt.net, wt.onet, p, ep, es, sw, (hipStream_t)stream),
                      "play_episodes_sweep launch");
  }
  return hip_status(mzh_launch_episodes_set(pl, wt.net, wt.onet, p, ep, es, (hipStream_t)stream), "play_episodes_multi launch");
}

extern "C" int mzh_play_episodes(mzh_engine* eng, const mzh_episode_args* a, mzh_stream stream) {
  return play_episodes_common(eng, a, nullptr, false, stream);
}

extern "C" int mzh_play_episodes_multi(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m,
                                       mzh_stream stream) {
  return play_episodes_common(eng, a, m, true, stream);
}

extern "C" int mzh_play_episodes_sweep(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m,
                                       const mzh_episode_sweep_args* w, mzh_stream stream) {
  return play_episodes_common(eng, a, m, true, stream, true, w);
}
