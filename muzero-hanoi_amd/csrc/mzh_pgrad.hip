// mzh_pgrad.hip -- parameter gradients of the five sub-networks in one fused launch (gfx950).
//
// mzh_param_grads (the reference's monosemanticity_analysis/gradient_analysis.py get_results, lines 274-338):
// per row and sub-network (representation, dynamic, reward, policy, value) the gradient of one scalar of the
// net's output with respect to the net's own parameters.  Each net is Linear0 -> ReLU -> Linear2 and a row's
// weight gradients are rank one, so the factor kernel writes delta2 (d objective / d Linear2 output), act
// (the hidden tile after the ReLU) and delta1 = (delta2 . W2) * [act > 0]; mzh_pgrad_expand_kernel makes the
// dense state_dict-shaped gradients of them when the caller asks.  One 256-thread workgroup owns R rows, as
// in mzh_saliency_kernel: row r of the tile is env sm.env[r] (-1: beyond the tile, or a skipped row -- it runs
// on a zero observation with action 0 and stores nothing).
//
// Forward: mzh_mlp_initial, then mzh_mlp_recurrent on the saved root latent and the row's action, both
// unchanged: h0 / pi0 / value0 and h1 / reward are the inference calls' bits.  The MLP block keeps three hidden
// tiles; the representation's and the dynamics' are overwritten by the prediction heads' and are made again by
// the forward's own chains (the same bits, the same mask), as mzh_saliency does for the representation.
//   initial   hidP = policy hidden, hidV = value hidden, hraw = z0, x = h0 (saved in h0s)
//   seeds     lrwd <- policy seed     seedV <- value seed     hidR[R][68] <- normalize's backward of 1/64 at z0
//   pol / val hidP <- (lrwd . pol2) * [hidP > 0]      hidV <- (seedV . val2) * [hidV > 0]       (in place)
//   rep       hidP <- relu(obs . rep0^T + b), then (hidR . rep2) * [hidP > 0] in place
//   recurrent x <- h0s: hidR = reward hidden, hraw = z1, x = h1, lrwd = reward logits
//   seeds     seedV <- reward seed    hidV[R][68] <- normalize's backward of 1/64 at z1
//   rwd       hidR <- (seedV . rwd2) * [hidR > 0]     (in place)
//   dyn       hidP <- relu(cat(h0, a) . dyn0^T + b), then (hidV . dyn2) * [hidP > 0] in place
// Every transposed product is sal_mma (mzh_backward.h) over MzhPackedT-format fragments: rep2 / pol2 / val2
// from the saliency kernel's transposed blob, dyn2 / rwd2 from the engine's MzhPackedG buffer.  Rows never mix
// in an MFMA, so a row's outputs are the same bits in any position and at either R.
#include "mzh_backward.h"
#include "mzh_rows.h"

#define MZH_PG_NETS 5

template <int R>
struct PgSmem : MlpSmem<R> {
  float h0s[R * MZH_LD64];  // the normalised root latents, in sm.x's layout
  float seedV[R * MZH_LDSEED];
  int env[R];
  int pick[R];
};

// normalize_h_state's backward (networks.py:191-196; D = max - min + 1e-8) of the constant upstream 1/64 of
// h.mean(), min and max differentiable: every element (1/64) / D, the arg-max element - sum g_i (h_i - min) / D^2,
// the arg-min element - sum g_i / D + sum g_i (h_i - min) / D^2 (mzh_saliency's "norm" step with g constant);
// arg-min / arg-max: the lowest unit index holding the min / max.  h and gr in k-block order.
__device__ __forceinline__ void pg_norm_seed(const float* h, float* gr) {
  const float gc = 0.015625f;
  float mn = h[0], mx = h[0];
  for (int i = 1; i < MZH_H; ++i) {
    mn = h[i] < mn ? h[i] : mn;
    mx = h[i] > mx ? h[i] : mx;
  }
  int amin = -1, amax = -1;
  float s1 = 0.0f, s2 = 0.0f;
  for (int k = 0; k < MZH_H; ++k) {  // unit k at position mzh_kpos(k)
    const int pk = mzh_kpos(k);
    if (amin < 0 && h[pk] == mn) amin = pk;
    if (amax < 0 && h[pk] == mx) amax = pk;
    s1 = s1 + gc;
    s2 = s2 + gc * (h[pk] - mn);
  }
  if (amin < 0) amin = 0;  // a NaN latent: no element compares equal
  if (amax < 0) amax = 0;
  const float D = (mx - mn) + 9.999999939225290290778502821922302246094e-09f;
  for (int i = 0; i < MZH_H; ++i) gr[i] = gc / D;
  const float c2 = s2 / (D * D);
  gr[amax] = gr[amax] - c2;
  gr[amin] = gr[amin] + (c2 - s1 / D);
}

// mean of a row's 64 units in unit order (row in k-block order)
__device__ __forceinline__ float pg_mean64(const float* h) {
  float s = 0.0f;
  for (int k = 0; k < MZH_H; ++k) s = s + h[mzh_kpos(k)];
  return s / 64.0f;
}

template <int R, class TILE = MzhGridTile>
__device__ __forceinline__ void mzh_pgrad_body(const MzhNet& net, const MzhSalNetT& nt, const float4* T, const MzhPgNetT& gt,
                                               const float4* GT, const MzhPgradParams& p, const TILE tile = TILE{}) {
  constexpr int MT = R / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  PgSmem<R>& sm = *reinterpret_cast<PgSmem<R>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  int li = -1, a = 0;
  mzh_rows_fill<R>(sm.env, p, p.err_count, tile, [&](int e) {  // an action outside [0, 6) or a policy_logit outside [-1, 6) skips its row
    a = p.action[e];
    bool ok = (unsigned)a < (unsigned)MZH_A;
    if (ok && p.policy_logit) {
      li = p.policy_logit[e];
      ok = li >= -1 && li < MZH_A;
    }
    if (!ok) {
      li = -1;
      a = 0;
    }
    return ok;
  }, [&]() {
    sm.pick[tid] = li;
    sm.act[tid] = a;
  });
  auto load_obs = [&]() { mzh_rows_load_obs<R>(sm.x, sm.env, p); };
  // a hidden tile (k-block order) as net `ni`'s [256] of `out` ([B][5][256])
  auto store256 = [&](float* out, int ni, const float* t) {
    for (int i = tid; i < R * MZH_F; i += MZH_THREADS) {
      const int r = i >> 8, k = i & 255;
      const int e = sm.env[r];
      if (e >= 0) out[((size_t)e * MZH_PG_NETS + ni) * MZH_F + k] = t[r * MZH_LD256 + mzh_kpos(k)];
    }
  };
  // a seed buffer (k-block order, ncols entries) as net `ni`'s [64] of delta2, +0 beyond ncols
  auto store_d2 = [&](int ni, const float* s, int ld, int ncols) {
    for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
      const int r = i >> 6, k = i & 63;
      const int e = sm.env[r];
      if (e >= 0) p.delta2[((size_t)e * MZH_PG_NETS + ni) * MZH_H + k] = k < ncols ? s[r * ld + mzh_kpos(k)] : 0.0f;
    }
  };
  // a [R][68] latent buffer (k-block order) as [B][64] (mzh_rows_store_latent's loop, kept as this kernel's own:
  // through the helper its code grows by 18 - 38 instructions)
  auto store64 = [&](float* out, const float* s) {
    for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
      const int r = i >> 6, k = i & 63;
      const int e = sm.env[r];
      if (e >= 0) out[(size_t)e * MZH_H + mzh_kpos(k)] = s[r * MZH_LD64 + k];
    }
  };
  // hid <- (seed . W2) * [hid > 0] in place, W2 transposed with KB k-blocks of outputs: wave w makes hidden
  // tiles 4w .. 4w + 3; a lane reads the element it writes
  auto back2 = [&](float* hid, const float* seed, int lds, const float4* W, int KB) {
    for (int q = 0; q < 4; ++q) {
      const int t = wave * 4 + q;
      const int pos = t * 16 + 4 * (r16 & 3) + (r16 >> 2);
      floatx4 acc[MT];
      sal_zero<MT>(acc);
      sal_mma<MT>(acc, seed, lds, W + t * KB * 64, KB, lane);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float* h = hid + (m * 16 + g * 4 + i) * MZH_LD256 + pos;
          *h = *h > 0.0f ? acc[m][i] : 0.0f;
        }
    }
  };
  auto objective = [&](int row, int ni, float v) {
    if (p.objective && sm.env[row] >= 0) p.objective[(size_t)sm.env[row] * MZH_PG_NETS + ni] = v;
  };

  load_obs();
  __syncthreads();
  MlpSmem<R>& ms = sm;  // the MLP block the inference kernels run on
  mzh_mlp_initial<R>(ms, net, wave, lane);

  // ---- the root's outputs, its latent kept for the recurrent step, the three seeds ----
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    sm.h0s[r * MZH_LD64 + k] = sm.x[r * MZH_LD64 + k];
  }
  store64(p.h0, sm.x);
  mzh_rows_store_root<R>(ms, sm.env, p.pi0, p.value0);
  store256(p.act, 3, sm.hidP);
  store256(p.act, 4, sm.hidV);
  float* seedP = sm.lrwd;  // [R][MZH_LDSUP]: 16 columns used (the initial MLP leaves lrwd alone)
  float* G = sm.hidR;      // [R][MZH_LD64]: the representation's seed (hidR is free until the recurrent step)
  if (tid < R) {
    const int row = tid;
    const int k = sm.pick[row];
    float d[MZH_A];
    float obj;
    if (k >= 0) {  // the logit k
      for (int i = 0; i < MZH_A; ++i) d[i] = i == k ? 1.0f : 0.0f;
      obj = sm.lpol[row * MZH_LDPOL + k];
    } else {  // softmax(lp).mean() as autograd differentiates it: p_i (g - sum_j g p_j) with g = 1/6
      const float* pr = sm.pi + row * 8;
      const float gc = 1.0f / 6.0f;
      float s = 0.0f, sp = 0.0f;
      for (int i = 0; i < MZH_A; ++i) {
        s = s + gc * pr[i];
        sp = sp + pr[i];
      }
      for (int i = 0; i < MZH_A; ++i) d[i] = (gc - s) * pr[i];
      obj = sp / 6.0f;
    }
    for (int i = 0; i < 16; ++i) seedP[row * MZH_LDSUP + mzh_kpos(i)] = i < MZH_A ? d[i] : 0.0f;
    objective(row, 3, obj);
  } else if (tid >= 64 && tid < 64 + R) {  // another wave: the value seeds
    const int row = tid - 64;
    sal_head_seed(net.support, sm.lval + row * MZH_LDSUP, sm.seedV + row * MZH_LDSEED);
    objective(row, 4, sm.value[row]);
  } else if (tid >= 128 && tid < 128 + R) {  // a third: the representation's
    const int row = tid - 128;
    pg_norm_seed(sm.hraw + row * MZH_LD64, G + row * MZH_LD64);
    objective(row, 0, pg_mean64(sm.x + row * MZH_LD64));
  }
  __syncthreads();

  // ---- policy and value: layer 2 transposed under the ReLU masks of hidP / hidV ----
  store_d2(0, G, MZH_LD64, MZH_H);
  store_d2(3, seedP, MZH_LDSUP, MZH_A);
  store_d2(4, sm.seedV, MZH_LDSEED, net.support);
  back2(sm.hidP, seedP, MZH_LDSUP, T + nt.off[MZH_T_POL2], 1);
  back2(sm.hidV, sm.seedV, MZH_LDSEED, T + nt.off[MZH_T_VAL2], nt.kb_val2);
  __syncthreads();
  store256(p.delta1, 3, sm.hidP);
  store256(p.delta1, 4, sm.hidV);
  load_obs();  // the normalised latent is saved in h0s
  __syncthreads();

  // ---- representation: rep0's hidden tile again (the forward's jobs), then rep2 transposed under its mask ----
  {
    MzhJob jobs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) jobs[q] = mzh_job(sm.x, MZH_LD64, net.rep0, wave * 4 + q, sm.hidP, MZH_LD256, 1);
    mzh_run_jobs<MT, 4>(jobs, net.rep0.kb, nullptr, nullptr, lane);
  }
  __syncthreads();
  store256(p.act, 0, sm.hidP);
  __syncthreads();
  back2(sm.hidP, G, MZH_LD64, T + nt.off[MZH_T_REP2], 4);
  __syncthreads();
  store256(p.delta1, 0, sm.hidP);
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    sm.x[r * MZH_LD64 + k] = sm.h0s[r * MZH_LD64 + k];
  }
  __syncthreads();

  // ---- the recurrent step on the row's action ----
  mzh_mlp_recurrent<R>(ms, net, wave, lane);
  if (p.h1) store64(p.h1, sm.x);
  store64(p.z1, sm.hraw);
  if (p.reward && tid < R && sm.env[tid] >= 0) p.reward[sm.env[tid]] = sm.reward[tid];
  store256(p.act, 2, sm.hidR);
  float* G1 = sm.hidV;  // [R][MZH_LD64]: the dynamics' seed (the next state's value hidden tile is not needed)
  if (tid < R) {  // the reward seeds
    const int row = tid;
    sal_head_seed(net.support, sm.lrwd + row * MZH_LDSUP, sm.seedV + row * MZH_LDSEED);
    objective(row, 2, sm.reward[row]);
  } else if (tid >= 64 && tid < 64 + R) {
    const int row = tid - 64;
    pg_norm_seed(sm.hraw + row * MZH_LD64, G1 + row * MZH_LD64);
    objective(row, 1, pg_mean64(sm.x + row * MZH_LD64));
  }
  __syncthreads();

  // ---- reward: rwd2 transposed under hidR's mask; the dynamics' input back into x ----
  store_d2(1, G1, MZH_LD64, MZH_H);
  store_d2(2, sm.seedV, MZH_LDSEED, net.support);
  back2(sm.hidR, sm.seedV, MZH_LDSEED, GT + gt.off[MZH_G_RWD2], gt.kb_rwd2);
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    sm.x[r * MZH_LD64 + k] = sm.h0s[r * MZH_LD64 + k];
  }
  __syncthreads();
  store256(p.delta1, 2, sm.hidR);

  // ---- dynamics: dyn0's hidden tile again (the forward's chain, one-hot column and bias order), then dyn2
  // transposed under its mask ----
  {
    MzhJob jobs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) jobs[q] = mzh_job(sm.x, MZH_LD64, net.dyn0, wave * 4 + q, sm.hidP, MZH_LD256, 1);
    mzh_run_jobs<MT, 4>(jobs, net.dyn0.kb, net.dyn0_onehot, sm.act, lane);
  }
  __syncthreads();
  store256(p.act, 1, sm.hidP);
  __syncthreads();
  back2(sm.hidP, G1, MZH_LD64, GT + gt.off[MZH_G_DYN2], 4);
  __syncthreads();
  store256(p.delta1, 1, sm.hidP);
}

template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_pgrad_kernel(MzhNet net, MzhSalNetT nt, MzhPgNetT gt, MzhPgradParams p) {
  mzh_pgrad_body<R>(net, nt, nt.base, gt, gt.base, p);
}

// rows of several networks (mzh_rows_multi_tile)
template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_pgrad_multi_kernel(MzhNet net, MzhSalNetT nt, MzhPgNetT gt,
                                                                         MzhPgradParams p, MzhMultiParams mp) {
  if (mzh_rows_no_tile(mp)) return;
  const MzhTableTile t = mzh_rows_multi_tile(net, mp);
  mzh_pgrad_body<R>(net, nt, mzh_net_ptr(nt.base, t.t.net, nt.stride), gt, mzh_net_ptr(gt.base, t.t.net, gt.stride), p, t);
}

// ------------------------------------------------------------------------------------------
// The dense gradients of the call's rows from the factors: row j's n_floats in canonical order (mzh_weights_size:
// weight [out][in] then bias [out] of the ten layers).  Layer 2i (Linear0 of net i) is delta1[i] (x) in_i with
// in = obs, cat(h0, one_hot(action)), z1, h0, h0; layer 2i + 1 is delta2[i] (x) act[i]; the biases are the
// deltas.  A workgroup copies the row's factors (about 3k floats) into LDS and streams its share of the row as
// 16-byte stores, consecutive lanes on consecutive addresses; a row the factor kernel skipped is skipped here by
// the same three conditions.  n_floats is a multiple of 4 for every shape (the odd tensors are the 6 + 2 S head
// biases), so every row starts 16-byte aligned.
// ------------------------------------------------------------------------------------------
#define MZH_PGX_THREADS 256
#define MZH_PGX_CHUNKS 4  // workgroups per row
struct PgxSmem {
  float d1[MZH_PG_NETS * MZH_F];
  float d2[MZH_PG_NETS * MZH_H];
  float act[MZH_PG_NETS * MZH_F];
  float in0[48];  // the observation
  float in1[72];  // h0 | one-hot of the action (the policy and value nets read its first 64)
  float in2[64];  // z1
  int end[20];    // canonical end of each tensor (weight, bias of the ten layers)
  int ncol[20];   // columns of a weight, 0 for a bias
  int rowf[20];   // float offset in this struct of the row factor (indexed by out)
  int colf[20];   // and of the column factor (indexed by in)
};

__global__ __launch_bounds__(MZH_PGX_THREADS) void mzh_pgrad_expand_kernel(MzhPgradParams p, int support, int n_floats,
                                                                            const int32_t* ntiles) {
  if (ntiles && *ntiles == 0) return;  // a refused net_index: nothing is written
  __shared__ __align__(16) PgxSmem sm;
  const int tid = threadIdx.x;
  const int j = blockIdx.x / MZH_PGX_CHUNKS, chunk = blockIdx.x % MZH_PGX_CHUNKS;
  const int e = p.env_index ? p.env_index[j] : j;
  if ((unsigned)e >= (unsigned)p.B) return;
  const int a = p.action[e];
  if ((unsigned)a >= (unsigned)MZH_A) return;
  if (p.policy_logit) {
    const int li = p.policy_logit[e];
    if (li < -1 || li >= MZH_A) return;
  }
  for (int i = tid; i < MZH_PG_NETS * MZH_F; i += MZH_PGX_THREADS) {
    sm.d1[i] = p.delta1[(size_t)e * MZH_PG_NETS * MZH_F + i];
    sm.act[i] = p.act[(size_t)e * MZH_PG_NETS * MZH_F + i];
  }
  for (int i = tid; i < MZH_PG_NETS * MZH_H; i += MZH_PGX_THREADS) sm.d2[i] = p.delta2[(size_t)e * MZH_PG_NETS * MZH_H + i];
  if (tid < 48) sm.in0[tid] = tid < p.in_dim ? p.obs[(size_t)e * p.in_dim + tid] : 0.0f;
  if (tid >= 64 && tid < 136) {
    const int k = tid - 64;
    sm.in1[k] = k < MZH_H ? p.h0[(size_t)e * MZH_H + k] : (k - MZH_H == a ? 1.0f : 0.0f);
  }
  if (tid >= 192) sm.in2[tid - 192] = p.z1[(size_t)e * MZH_H + tid - 192];
  if (tid == 0) {
    const float* base = sm.d1;
    const int in0off = (int)(sm.in0 - base), in1off = (int)(sm.in1 - base), in2off = (int)(sm.in2 - base);
    const int d2off = (int)(sm.d2 - base), actoff = (int)(sm.act - base);
    const int ins[MZH_PG_NETS] = {p.in_dim, MZH_H + MZH_A, MZH_H, MZH_H, MZH_H};
    const int inoff[MZH_PG_NETS] = {in0off, in1off, in2off, in1off, in1off};
    const int outs[MZH_PG_NETS] = {MZH_H, MZH_H, support, MZH_A, support};
    int pos = 0;
    for (int ni = 0; ni < MZH_PG_NETS; ++ni)
      for (int second = 0; second < 2; ++second) {
        const int O = second ? outs[ni] : MZH_F, I = second ? MZH_F : ins[ni];
        const int rf = second ? d2off + ni * MZH_H : ni * MZH_F;
        const int t = 4 * ni + 2 * second;
        pos += O * I;
        sm.end[t] = pos;
        sm.ncol[t] = I;
        sm.rowf[t] = rf;
        sm.colf[t] = second ? actoff + ni * MZH_F : inoff[ni];
        pos += O;
        sm.end[t + 1] = pos;
        sm.ncol[t + 1] = 0;
        sm.rowf[t + 1] = rf;
        sm.colf[t + 1] = 0;
      }
  }
  __syncthreads();
  const float* f = sm.d1;
  const int n4 = n_floats >> 2;
  const int per = (n4 + MZH_PGX_CHUNKS - 1) / MZH_PGX_CHUNKS;
  const int q0 = chunk * per, q1 = min(n4, q0 + per);
  float4* out = reinterpret_cast<float4*>(p.grad + (size_t)j * n_floats);
  for (int q = q0 + tid; q < q1; q += MZH_PGX_THREADS) {
    int idx = 4 * q;
    int t = 0;
    while (t < 19 && idx >= sm.end[t]) ++t;
    int start = t ? sm.end[t - 1] : 0;
    int I = sm.ncol[t];
    int o = I ? (idx - start) / I : idx - start;
    int c = I ? (idx - start) - o * I : 0;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k, ++idx) {
      while (t < 19 && idx >= sm.end[t]) {  // the next tensor begins inside this float4
        start = sm.end[t];
        ++t;
        I = sm.ncol[t];
        o = 0;
        c = 0;
      }
      const float rf = f[sm.rowf[t] + o];
      v[k] = I ? rf * f[sm.colf[t] + c] : rf;
      if (I) {
        if (++c == I) {
          c = 0;
          ++o;
        }
      } else {
        ++o;
      }
    }
    out[q] = float4{v[0], v[1], v[2], v[3]};
  }
}

// dst[m][j] = src[m][map[j]] (+0 where map[j] < 0): the MzhPackedG buffer from the main blob(s)
__global__ void mzh_pgrad_gather_kernel(const int32_t* map, int n, const float* src, size_t src_stride, float* dst,
                                        size_t dst_stride) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int s = map[j];
  const size_t m = blockIdx.y;
  dst[m * dst_stride + j] = s >= 0 ? src[m * src_stride + s] : 0.0f;
}

hipError_t mzh_launch_pgrad_gather(const int32_t* map, int n, const float* src, size_t src_stride, float* dst,
                                   size_t dst_stride, int M, hipStream_t stream) {
  hipLaunchKernelGGL(mzh_pgrad_gather_kernel, dim3((n + 255) / 256, M), dim3(256), 0, stream, map, n, src, src_stride, dst,
                     dst_stride);
  return hipGetLastError();
}

template <int R>
static size_t pgrad_smem_bytes() { return (sizeof(PgSmem<R>) + 15) & ~(size_t)15; }
size_t mzh_pgrad_smem_bytes(int R) { return R == 32 ? pgrad_smem_bytes<32>() : pgrad_smem_bytes<16>(); }

hipError_t mzh_launch_pgrad(int R, const MzhNet& net, const MzhSalNetT& nt, const MzhPgNetT& gt, const MzhPgradParams& p,
                            int support, const MzhMultiParams* mp, hipStream_t stream) {
  hipError_t e = R == 32 ? mzh_rows_launch(&mzh_pgrad_multi_kernel<32>, &mzh_pgrad_kernel<32>, 32, pgrad_smem_bytes<32>(), p.n,
                                           mp, stream, net, nt, gt, p)
                         : mzh_rows_launch(&mzh_pgrad_multi_kernel<16>, &mzh_pgrad_kernel<16>, 16, pgrad_smem_bytes<16>(), p.n,
                                           mp, stream, net, nt, gt, p);
  if (e != hipSuccess || !p.grad) return e;
  const int n_floats = (int)mzh_canon_view(nullptr, p.in_dim, support).total;
  hipLaunchKernelGGL(mzh_pgrad_expand_kernel, dim3((unsigned)p.n * MZH_PGX_CHUNKS), dim3(MZH_PGX_THREADS), 0, stream, p, support,
                     n_floats, mp ? mp->ntiles : nullptr);
  return hipGetLastError();
}
