// mzh_saliency.hip -- input saliency of the policy and value heads in one fused launch (gfx950).
//
// mzh_saliency (the reference's monosemanticity_analysis/gradient_analysis.py compute_saliency): per row
// d(policy logit k)/d(obs) and d(value)/d(obs) through represent + prediction.  One 256-thread workgroup owns
// R rows, like mzh_probe_kernel: row r of the tile is env sm.env[r] of the batch (-1: beyond the tile, or a
// skipped row -- it runs on a zero observation and stores nothing).
//
// Forward: mzh_mlp_initial, unchanged, so h0 / pi0 / value0 and the logits the backward starts from are
// bit-identical to mzh_initial_inference on the row.  It leaves in LDS: the policy / value hidden tiles
// (hidP / hidV, after ReLU), the raw latent (hraw), the normalised latent (x) and the logits (lpol / lval);
// the representation's hidden tile is gone (pol0 overwrote it) and is recomputed by the same chain.
//
// Backward: every product is dX = dY . W on v_mfma_f32_16x16x4_f32 with the transposed blob's fragments
// (MzhPackedT, mzh_pack.h) as the B operand and dY, in k-block order in LDS, as the A operand.  The two
// heads go through the trunk as 2R rows of one GEMM (policy rows [0, R), value rows [R, 2R)).
//   seeds   lrwd  <- one-hot(k)                      seedV <- dv/dlogits (33 bins) or 1
//   head 2  hidP  <- (lrwd . pol2) * [hidP > 0]      hidV  <- (seedV . val2) * [hidV > 0]     (in place)
//   head 0  G     <- hidP . pol0 | hidV . val0       (G = hidR as [2R][68]: d/d normalised latent)
//   norm    G     <- normalize_h_state's backward, min and max differentiable
//   rep0    hidP  <- relu(obs . rep0^T + b)          (the forward's chain again: the same bits, the same mask)
//   rep 2   hidV | hidP <- (G . rep2) * [hidP > 0]   (policy rows to hidV, value rows in place)
//   rep 0   DX    <- hidV . rep0 | hidP . rep0       (DX = hidR as [2R][68], natural column order)
// There is no bit contract on the backward's summation order; a row's outputs depend on that row and its
// network alone (rows never mix in an MFMA), so they are the same bits in any position and at either R.
#include "mzh_backward.h"
#include "mzh_rows.h"

template <int R>
struct SalSmem : MlpSmem<R> {
  float seedV[R * MZH_LDSEED];
  int env[R];
  int pick[R];
};

template <int R, class TILE = MzhGridTile>
__device__ __forceinline__ void mzh_saliency_body(const MzhNet& net, const MzhSalNetT& nt, const float4* T,
                                                  const MzhSalParams& p, const TILE tile = TILE{}) {
  constexpr int MT = R / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  SalSmem<R>& sm = *reinterpret_cast<SalSmem<R>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  int li = -1;
  mzh_rows_fill<R>(sm.env, p, p.err_count, tile, [&](int e) {  // a logit_index outside [-1, 6) skips its row
    if (!p.logit_index) return true;
    li = p.logit_index[e];
    if (li < -1 || li >= MZH_A) {
      li = -1;
      return false;
    }
    return true;
  }, [&]() { sm.pick[tid] = li; });
  mzh_rows_load_obs<R>(sm.x, sm.env, p);
  __syncthreads();
  MlpSmem<R>& ms = sm;  // the MLP block the inference kernels run on
  mzh_mlp_initial<R>(ms, net, wave, lane);

  // ---- the forward's outputs, and the heads' seeds (lrwd is unused by the initial MLP) ----
  if (p.h0) mzh_rows_store_latent<R>(p.h0, sm.x, sm.env);
  mzh_rows_store_root<R>(ms, sm.env, p.pi0, p.value0);
  float* seedP = sm.lrwd;  // [R][MZH_LDSUP]: 16 columns used
  if (tid < R) {
    const int row = tid;
    int k = sm.pick[row];
    if (k < 0) {  // the lowest index of the largest logit
      const float* l = sm.lpol + row * MZH_LDPOL;
      k = 0;
      float best = l[0];
      for (int i = 1; i < MZH_A; ++i)
        if (l[i] > best) {
          best = l[i];
          k = i;
        }
      sm.pick[row] = k;
    }
    for (int i = 0; i < 16; ++i) seedP[row * MZH_LDSUP + mzh_kpos(i)] = i == k ? 1.0f : 0.0f;
  } else if (tid >= 64 && tid < 64 + R) {  // another wave: the value seeds
    const int row = tid - 64;
    sal_head_seed(net.support, sm.lval + row * MZH_LDSUP, sm.seedV + row * MZH_LDSEED);
  }
  __syncthreads();

  // ---- head layer 2 transposed, the ReLU masks of hidP / hidV (in place: a lane reads the element it writes).  This
  // step, the normalisation's backward and rep0's hidden tile below are this kernel's own text although mzh_backward.h
  // has each of them for mzh_pgrad.hip: through the shared forms the 65,536-row call measured 0.3 - 0.5% slower
  // (profiles/rows_refactor_experiments.json) ----
  for (int q = 0; q < 4; ++q) {
    const int t = wave * 4 + q;
    const int pos = t * 16 + 4 * (r16 & 3) + (r16 >> 2);
    floatx4 acc[MT];
    sal_zero<MT>(acc);
    sal_mma<MT>(acc, seedP, MZH_LDSUP, T + nt.off[MZH_T_POL2] + t * 64, 1, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float* h = sm.hidP + (m * 16 + g * 4 + i) * MZH_LD256 + pos;
        *h = *h > 0.0f ? acc[m][i] : 0.0f;
      }
    sal_zero<MT>(acc);
    sal_mma<MT>(acc, sm.seedV, MZH_LDSEED, T + nt.off[MZH_T_VAL2] + t * nt.kb_val2 * 64, nt.kb_val2, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float* h = sm.hidV + (m * 16 + g * 4 + i) * MZH_LD256 + pos;
        *h = *h > 0.0f ? acc[m][i] : 0.0f;
      }
  }
  __syncthreads();

  // ---- head layer 0 transposed: wave w makes latent tile w of both heads ----
  float* G = sm.hidR;  // [2R][MZH_LD64]
  {
    const int pos = wave * 16 + 4 * (r16 & 3) + (r16 >> 2);
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) {
      floatx4 acc[MT];
      sal_zero<MT>(acc);
      sal_mma<MT>(acc, hd ? sm.hidV : sm.hidP, MZH_LD256, T + nt.off[hd ? MZH_T_VAL0 : MZH_T_POL0] + wave * 16 * 64, 16, lane);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) G[(hd * R + m * 16 + g * 4 + i) * MZH_LD64 + pos] = acc[m][i];
    }
  }
  __syncthreads();

  // ---- normalize_h_state's backward, one thread per gradient row; the observations come back into sm.x beside
  // it (nothing reads the normalised latent any more) ----
  mzh_rows_load_obs<R>(sm.x, sm.env, p);
  if (tid < 2 * R) {
    float* gr = G + tid * MZH_LD64;
    const float* h = sm.hraw + (tid < R ? tid : tid - R) * MZH_LD64;
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
      s1 = s1 + gr[pk];
      s2 = s2 + gr[pk] * (h[pk] - mn);
    }
    if (amin < 0) amin = 0;  // a NaN latent: no element compares equal
    if (amax < 0) amax = 0;
    const float D = (mx - mn) + 9.999999939225290290778502821922302246094e-09f;
    for (int i = 0; i < MZH_H; ++i) gr[i] = gr[i] / D;
    const float c2 = s2 / (D * D);
    gr[amax] = gr[amax] - c2;
    gr[amin] = gr[amin] + (c2 - s1 / D);
  }
  __syncthreads();

  // ---- rep0's hidden tile again (the forward's jobs: the same chain, the same bits) ----
  {
    MzhJob jobs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) jobs[q] = mzh_job(sm.x, MZH_LD64, net.rep0, wave * 4 + q, sm.hidP, MZH_LD256, 1);
    mzh_run_jobs<MT, 4>(jobs, net.rep0.kb, nullptr, nullptr, lane);
  }
  __syncthreads();

  // ---- rep2 transposed on the 2R rows, rep0's ReLU mask: policy rows -> hidV, value rows -> hidP in place ----
  for (int q = 0; q < 4; ++q) {
    const int t = wave * 4 + q;
    const int pos = t * 16 + 4 * (r16 & 3) + (r16 >> 2);
    floatx4 acc[2 * MT];
    sal_zero<2 * MT>(acc);
    sal_mma<2 * MT>(acc, G, MZH_LD64, T + nt.off[MZH_T_REP2] + t * 4 * 64, 4, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = (m * 16 + g * 4 + i) * MZH_LD256 + pos;
        const bool on = sm.hidP[idx] > 0.0f;
        sm.hidV[idx] = on ? acc[m][i] : 0.0f;
        sm.hidP[idx] = on ? acc[MT + m][i] : 0.0f;
      }
  }
  __syncthreads();

  // ---- rep0 transposed: (observation tile, head) jobs over the waves; DX in natural column order ----
  float* DX = sm.hidR;  // [2R][MZH_LD64]; G is dead
  for (int j = wave; j < 2 * nt.nt_rep0; j += MZH_WAVES) {
    const int hd = j & 1, t = j >> 1;
    floatx4 acc[MT];
    sal_zero<MT>(acc);
    sal_mma<MT>(acc, hd ? sm.hidP : sm.hidV, MZH_LD256, T + nt.off[MZH_T_REP0] + t * 16 * 64, 16, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) DX[(hd * R + m * 16 + g * 4 + i) * MZH_LD64 + t * 16 + r16] = acc[m][i];
  }
  __syncthreads();

  // ---- outputs ----
  for (int i = tid; i < R * p.in_dim; i += MZH_THREADS) {
    const int r = i / p.in_dim, k = i - r * p.in_dim;
    const int e = sm.env[r];
    if (e >= 0) {
      p.sal_policy[(size_t)e * p.in_dim + k] = DX[r * MZH_LD64 + k];
      p.sal_value[(size_t)e * p.in_dim + k] = DX[(R + r) * MZH_LD64 + k];
    }
  }
  if (p.disc_policy || p.disc_value)
    for (int i = tid; i < R * p.n_disks; i += MZH_THREADS) {
      const int r = i / p.n_disks, d = i - r * p.n_disks;
      const int e = sm.env[r];
      if (e >= 0) {
        const float* sp = DX + r * MZH_LD64 + 3 * d;
        const float* sv = DX + (R + r) * MZH_LD64 + 3 * d;
        if (p.disc_policy)
          p.disc_policy[(size_t)e * p.n_disks + d] = (__builtin_fabsf(sp[0]) + __builtin_fabsf(sp[1])) + __builtin_fabsf(sp[2]);
        if (p.disc_value)
          p.disc_value[(size_t)e * p.n_disks + d] = (__builtin_fabsf(sv[0]) + __builtin_fabsf(sv[1])) + __builtin_fabsf(sv[2]);
      }
    }
  if (p.picked && tid < R && sm.env[tid] >= 0) p.picked[sm.env[tid]] = sm.pick[tid];
}

template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_saliency_kernel(MzhNet net, MzhSalNetT nt, MzhSalParams p) {
  mzh_saliency_body<R>(net, nt, nt.base, p);
}

// rows of several networks (mzh_rows_multi_tile)
template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_saliency_multi_kernel(MzhNet net, MzhSalNetT nt, MzhSalParams p,
                                                                            MzhMultiParams mp) {
  if (mzh_rows_no_tile(mp)) return;
  const MzhTableTile t = mzh_rows_multi_tile(net, mp);
  mzh_saliency_body<R>(net, nt, mzh_net_ptr(nt.base, t.t.net, nt.stride), p, t);
}

template <int R>
static size_t saliency_smem_bytes() { return (sizeof(SalSmem<R>) + 15) & ~(size_t)15; }
size_t mzh_saliency_smem_bytes(int R) { return R == 32 ? saliency_smem_bytes<32>() : saliency_smem_bytes<16>(); }

hipError_t mzh_launch_saliency(int R, const MzhNet& net, const MzhSalNetT& nt, const MzhSalParams& p,
                               const MzhMultiParams* mp, hipStream_t stream) {
  if (R == 32)
    return mzh_rows_launch(&mzh_saliency_multi_kernel<32>, &mzh_saliency_kernel<32>, 32, saliency_smem_bytes<32>(), p.n, mp,
                           stream, net, nt, p);
  return mzh_rows_launch(&mzh_saliency_multi_kernel<16>, &mzh_saliency_kernel<16>, 16, saliency_smem_bytes<16>(), p.n, mp,
                         stream, net, nt, p);
}
