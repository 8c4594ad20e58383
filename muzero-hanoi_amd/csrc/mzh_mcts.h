// mzh_mcts.h -- the MCTS arithmetic every search kernel shares: the cooperative kernels (mzh_search.hip
// over mzh_tree.h), the wave kernel (mzh_wave.hip) and the latency kernel (mzh_one.hip).  The kernels
// differ in traversal and storage only -- who holds which child, where the blocks live, how lanes
// exchange values; whatever must agree bit for bit between them and with the reference is here, once.
//
// Reference: MCTS/mcts.py:34-176 (run_mcts, generate_play_policy), MCTS/node.py:72-123 (best_child /
// child_Q / child_U), MCTS/utils_mcts.py:1-16 (MinMaxStats).
#pragma once
#include "mzh_device.h"
#include "mzh_internal.h"

// a / b correctly rounded from y = RN(1/b) (Markstein: q = RN(a*y) is within one ulp, the fma
// residual is exact, and one correction step rounds to RN(a/b)); 3 fp64 ops instead of the
// ~12-op div_scale/rcp/fmas/fixup sequence on the select chain.  Equal to `a / b` for every
// finite non-subnormal quotient; checked against true division in tests/test_markstein.py.
__device__ __forceinline__ double mzh_div(double a, double b, double y) {
  const double q = a * y;
  const double r = __builtin_fma(-q, b, a);
  return __builtin_fma(r, y, q);
}

// MinMaxStats (utils_mcts.py:1-16) with the select-side normaliser precomputed:
// den = max - min, dinv = RN(1/den) (0 while the bounds are unset or equal)
struct MzhMinMax {
  double mmax, mmin, den, dinv;
  __device__ __forceinline__ void set(double mx, double mn) {
    mmax = mx;
    mmin = mn;
    den = mx - mn;
    dinv = mx > mn ? 1.0 / (mx - mn) : 0.0;
  }
  // MinMaxStats.update over a backup's candidates, reduced to their maximum and minimum
  __device__ __forceinline__ void update(double lmax, double lmin) {
    set(lmax > mmax ? lmax : mmax, lmin < mmin ? lmin : mmin);
  }
  __device__ __forceinline__ bool has() const { return mmax > mmin; }
};

// MinMaxStats.normalize (utils_mcts.py:12-16) with den = max - min, dinv = RN(1/den).  The
// Markstein quotient needs a normal den (its reciprocal finite, the residual exact); `exact`
// (wave-uniform: some lane of the wave has a subnormal den -- only reachable from caller-given
// MinMaxStats bounds, never from fp32 network outputs) takes the IEEE division instead
__device__ __forceinline__ double mzh_normalize(double v, bool has, double mn, double den, double dinv, bool exact) {
  return has ? (exact ? (v - mn) / den : mzh_div(v - mn, den, dinv)) : v;
}
// whether any lane of the wave needs the exact normaliser (a non-zero subnormal max - min)
__device__ __forceinline__ bool mzh_need_exact(bool has, double den) {
  return __builtin_amdgcn_ballot_w64(has && !(den >= 2.2250738585072014e-308)) != 0;
}

// ucb = fl32(Q) + fl32(U) for one child (node.py:90-123); `tnp` = table[N_parent], inv[k] = RN(1/k)
// Branch-free: both reciprocals are read together (one ds_read2_b64) and the Q and U chains run side
// by side; for Nc = 0 the Q chain computes from inv[0] = inf and its result is discarded.
__device__ __forceinline__ float mzh_ucb(int Nc, double Wc, float Rc, double P64, bool p64_semantics, double tnp,
                                         double disc, bool has, double mn, double den, double dinv,
                                         const double* inv, bool exact) {
  const double i0 = inv[Nc], i1 = inv[Nc + 1];
  const double qn = mzh_normalize((double)Rc + disc * mzh_div(Wc, (double)Nc, i0), has, mn, den, dinv, exact);
  const float q32 = Nc > 0 ? (float)qn : 0.0f;
  const double w = mzh_div(tnp, (double)(Nc + 1), i1);
  // np.float64 priors (Dirichlet-mixed root) or NumPy-1 promotion: fl32(fl64(prior * w));
  // NumPy-2 with np.float32 priors: fl32(prior * fl32(w))
  const float u32 = p64_semantics ? (float)(P64 * w) : (float)P64 * (float)w;
  return q32 + u32;
}

// the pick from the 6-bit argmax mask of a node's children, with the reference's tie handling:
// np.random.choice(argmax set) -- the first 6-way tie takes the host-drawn index `tie`, any other
// tie is counted in `extra` (RNG-stream divergence) and resolved to the lowest index.  Branch-free.
__device__ __forceinline__ int mzh_tie_pick(unsigned mask, int tie, int& firstTie, int& extra) {
  const int cnt = __popc(mask);
  const int first = __ffs(mask) - 1;
  const bool six = (cnt == MZH_A) & (firstTie == 0);
  extra += ((cnt > 1) & !six) ? 1 : 0;
  firstTie |= six ? 1 : 0;
  return six ? tie : first;
}

// a root child's prior as fp64 (mcts.py:57-69, 132-152): the widened fp32 prior, or with Dirichlet
// noise (1 - eps) * prior as a float32 array element plus eps * noise in np.float64
__device__ __forceinline__ double mzh_root_prior(float pr, bool noised, double eps, double noise) {
  if (!noised) return (double)pr;
  const float scaled = (float)(1.0 - eps) * pr;  // (1-eps) * prob, float32 array
  return (double)scaled + eps * noise;
}

// generate_play_policy (mcts.py:154-176) and the action draw (mcts.py:115-122) of one root from its visit
// counts, by one lane: writes pi where given and returns the action (the episode kernel steps its env with it)
__device__ __forceinline__ int mzh_play_policy(const MzhSearchParams& p, const int root, const int (&vis)[MZH_A]) {
  double v[MZH_A];
  for (int a = 0; a < MZH_A; ++a) v[a] = (double)vis[a];
  if (p.temperature > 0.0) {
    double ex = 1.0 / p.temperature;
    ex = ex < 5.0 ? ex : 5.0;  // max(1.0, min(5.0, 1/T))
    ex = ex > 1.0 ? ex : 1.0;
    for (int a = 0; a < MZH_A; ++a) v[a] = mzh_pow(v[a], vis[a], ex, p.pow_table);
  }
  double sum = 0.0;
  for (int a = 0; a < MZH_A; ++a) sum = sum + v[a];
  double pi[MZH_A];
  for (int a = 0; a < MZH_A; ++a) pi[a] = v[a] / sum;
  if (p.pi)
    for (int a = 0; a < MZH_A; ++a) p.pi[(size_t)root * MZH_A + a] = pi[a];
  int act = 0;
  if (p.deterministic || !p.action_u) {
    for (int a = 1; a < MZH_A; ++a)
      if (vis[a] > vis[act]) act = a;
  } else {
    double cdf[MZH_A];
    double acc = 0.0;
    for (int a = 0; a < MZH_A; ++a) {
      acc = acc + pi[a];
      cdf[a] = acc;
    }
    const double last = cdf[MZH_A - 1];
    const double u = p.action_u[root];
    act = MZH_A - 1;
    for (int a = 0; a < MZH_A; ++a) {
      if (cdf[a] / last > u) {
        act = a;
        break;
      }
    }
  }
  return act;
}

// The results of one root (mcts.py:111-126, generate_play_policy mcts.py:154-176), written by one lane:
// visits, root Q, MinMaxStats bounds, the tie and step counters, the last simulation's action path
// (path_at(j) = path entry j of that selection, its low 3 bits the child), pi and the action.
// OWN (mzh_search_multi_budget): the root ran `own` simulations, its own budget, which is at most p.S; the rows of
// p.latent keep the launch's stride p.S + 1 either way.
template <bool OWN = false, class PathAt>
__device__ __forceinline__ void mzh_write_results(const MzhSearchParams& p, const int root, const int (&vis)[MZH_A],
                                                  const double rootW, const int rootN, const double mmax,
                                                  const double mmin, const int extra, const int steps, const int depth,
                                                  PathAt path_at, const int own = 0) {
  for (int a = 0; a < MZH_A; ++a) p.visits[(size_t)root * MZH_A + a] = vis[a];
  if (p.root_q) p.root_q[root] = rootN == 0 ? 0.0 : rootW / (double)rootN;
  if (p.minmax_out) {
    p.minmax_out[2 * root] = mmax;
    p.minmax_out[2 * root + 1] = mmin;
  }
  if (p.extra_ties) p.extra_ties[root] = extra;
  if (p.sel_steps) p.sel_steps[root] = steps;
  const int PL = p.S + 1;
  if (p.latent && (OWN ? own : p.S) > 0) {
    for (int j = 0; j < depth; ++j) p.latent[(size_t)root * PL + j] = path_at(j) & 7;
    for (int j = depth; j < PL; ++j) p.latent[(size_t)root * PL + j] = -1;
  }
  if (p.latent_len) p.latent_len[root] = (OWN ? own : p.S) > 0 ? depth : 0;
  if (p.pi || p.action) {
    const int act = mzh_play_policy(p, root, vis);
    if (p.action) p.action[root] = act;
  }
}
