// mzh_backward.h -- what the backward kernels share (mzh_saliency.hip, mzh_pgrad.hip): the transposed product
// dX = dY . W on v_mfma_f32_16x16x4_f32 over MzhPackedT-format fragments, and the seed of a reward / value head.
#pragma once
#include "mzh_device.h"

#define MZH_LDSEED 52  // 33-bin head seed row: 48 columns (33 bins zero-padded to three k-blocks) + 4

// acc[m] += A[row tile m][0 : 16 KB] . W (one 16-column tile: KB k-blocks of 64 float4); A in k-block order
template <int MT>
__device__ __forceinline__ void sal_mma(floatx4* acc, const float* A, int lda, const float4* W, int KB, int lane) {
  const int r = lane & 15, g = lane >> 4;
  float4 t = W[lane];
  for (int kb = 0; kb < KB; ++kb) {
    const floatx4 b{t.x, t.y, t.z, t.w};
    if (kb + 1 < KB) t = W[(kb + 1) * 64 + lane];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(A + (m * 16 + r) * lda + kb * 16 + g * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[m], 0, 0, 0);
    }
  }
}

template <int N>
__device__ __forceinline__ void sal_zero(floatx4* acc) {
#pragma unroll
  for (int m = 0; m < N; ++m) acc[m] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// d(value)/d(value logits) of a 33-bin head (networks.py:152-189 as autograd differentiates it) into the row's
// seed, k-block order: p = softmax(l), E = sum p_i s_i (s = -16..16), v = sign(E) (z^2 - 1) with
// z = (sqrt(1 + 4 eps (eps + 1 + |E|)) - 1) / (2 eps) = 2 (eps + 1 + |E|) / (sqrt(..) + 1) (no cancellation),
// dv/dE = 2 z / sqrt(..) (0 at E = 0, as torch's sign and abs give), dv/dl_i = dv/dE p_i (s_i - E)
__device__ __forceinline__ void sal_value_seed33(const float* l, float* seed) {
  float m = l[0];
  for (int i = 1; i < 33; ++i) m = l[i] > m ? l[i] : m;
  float s = 0.0f, se = 0.0f;
  for (int i = 0; i < 33; ++i) {
    const float e = mzh_expf(l[i] - m);
    s = s + e;
    se = se + e * (float)(i - 16);
  }
  const float E = se / s;
  const float eps = 0.001f;
  const float a = __builtin_fabsf(E);
  const float u = eps + 1.0f + a;
  const float sq = __builtin_sqrtf(1.0f + 4.0f * eps * u);
  const float z = 2.0f * u / (sq + 1.0f);
  const float dv = E != 0.0f ? 2.0f * z / sq : 0.0f;
  for (int i = 0; i < 48; ++i) {
    float v = 0.0f;
    if (i < 33) v = dv * (mzh_expf(l[i] - m) / s) * ((float)(i - 16) - E);
    seed[mzh_kpos(i)] = v;
  }
}

// the seed of a reward / value head from its logits: d scalar / d logits of 33 bins, the unit seed of one bin
__device__ __forceinline__ void sal_head_seed(int support, const float* l, float* seed) {
  if (support == 33) {
    sal_value_seed33(l, seed);
  } else {
    for (int i = 0; i < 16; ++i) seed[i] = i == 0 ? 1.0f : 0.0f;
  }
}
