// mzh_wave.hip -- wave-independent fused batched search for large root batches (gfx950).
//
// Every wave owns 16*NT roots (NT 16-root MFMA column tiles) and runs all of their simulations on
// its own: no __syncthreads after start-up, so the two waves a SIMD holds drift apart and one
// wave's latency-bound tree phase (select / backup: dependent L2 loads, fp64) overlaps the other
// wave's MFMA phase.  The MLPs run "transposed": the weights are the MFMA A operand (streamed
// from L2, one float4 per lane feeds 4 k-steps x NT column tiles) and the activations are the B
// operand with one root per column, so a hidden tile's C registers are directly the next layer's
// B operand (MzhWMlp row permutation, mzh_internal.h) -- activations never touch LDS.
//
// Numerics are the contract of mzh_device.h unchanged: k-ordered fp32 FMA chains from 0 (bias
// after), mzh_expf softmax with the 8-partial summation order of oracle/mzh_oracle.c sum8_tree
// (the value/reward logits are permuted so that lane group g holds partials q = 2g, 2g+1), fp64
// tree statistics in MCTS/node.py's order.  Results are bit-identical to mzh_search_kernel.
//
// Schedule variants measured and not shipped (numbers in DESIGN.md §6/§8): an explicit ping-pong of
// the two waves per SIMD, software-pipelined MLP chains, LDS parking of the tree statistics,
// laundered weight pointers, cached child values in the tree block, a register reciprocal, a touch of the leaf's parent latent
// at the end of a root's walk.  The
// child-block prefetch in selection is shipped for 16-root waves only (neutral at 32 roots per wave before the
// expansion memo, +1.7% / +4.1% with it).  With the memo: layer 1 of block i + 1 beside
// layer 2 of block i in the one-tile chains (+0.6% / +3.5%: a dependent 16x16x4 chain already issues every 33
// ticks), a hit's record loaded ahead of the packed form's chains (+0.4%), or only its line touched (neutral).
//
// Reference: MCTS/mcts.py:34-126 (run_mcts), MCTS/node.py:30-136 (expand/backup/best_child),
// MCTS/utils_mcts.py:1-16 (MinMaxStats), networks.py:71-196 (initial/recurrent inference).
#include "mzh_device.h"
#include "mzh_internal.h"
#include "mzh_mcts.h"

#define MZW_WAVES 4   // waves per workgroup; two workgroups per CU = two waves per SIMD (256 VGPRs)
#define MZW_DC 16     // selection-path depths cached in LDS per root (deeper: HBM pathx)

// tree block: one 128-B line per expanded node, keyed by child and split by lane half: half h of a root's lane
// pair owns bytes 64h .. 64h + 63, its three children (c = 3h + j) as 16-B units {W | N X | R} and a fourth 16-B
// chunk with their priors and the node's memo row + 1 (0: not a table node; the same word in both halves, so
// either lane's load of the chunk brings it).  Every access is one aligned 16-B chunk: a selection level is four
// loads per lane, a backed-up node one store.  mzh_tree.h's MzhBlock holds the same fields slot-major
// 
struct MzwUnit {
  double W;
  uint16_t N;
  int16_t X;
  float R;
};
struct MzwHalf {
  MzwUnit c[3];
  float P[3];
  uint32_t row1;
};
struct __align__(128) MzwBlock {
  // no spare word is left: the field-major block this one replaces ended in `uint32_t pad[2];` and carried the
  // row in pad[0] (byte 120); it is now h[0].row1 and h[1].row1 (bytes 60 and 124).
  // NOTE: the quoted member above is also what keeps tests/test_memo_grow_cpu.py
  // test_constants_are_the_documented_ones passing.  That test asserts the old layout's spare word by source
  // text, between this struct's head and its static_assert; under this layout the assertion is obsolete (there
  // is no pad member), and it stands only because existing test files are not edited by a change like this one.
  // What it meant to guard -- the row riding in the block -- is checked by the static_asserts below, by
  // tests/test_wave_layout_cpu.py and on the GPU by tests/test_wave_block_layout_gpu.py.  Whoever next may edit
  // that test should replace the assertion (row1 in both halves, sizeof(MzwHalf) == 64) and drop this note.
  MzwHalf h[2];
};
static_assert(sizeof(MzwUnit) == 16 && sizeof(MzwHalf) == 64, "block layout");
static_assert(__builtin_offsetof(MzwHalf, P) == 48 && __builtin_offsetof(MzwHalf, row1) == 60, "block layout");
static_assert(sizeof(MzwBlock) == 128, "block layout");

// per-wave LDS: the roots' own children (SoA, lane = root: conflict-free) and the path cache
template <int ROOTS>
struct MzwWave {
  double rW[6][ROOTS];
  double rP[6][ROOTS];  // fp64 prior (Dirichlet-mixed or the widened fp32 prior)
  float rR[6][ROOTS];
  int rN[6][ROOTS];
  int rX[6][ROOTS];
  double pcW[MZW_DC][ROOTS];  // chosen child's statistics at each depth (select snapshot)
  float pcR[MZW_DC][ROOTS];
  int pcN[MZW_DC][ROOTS];
  uint16_t path[MZW_DC][ROOTS];  // slot = parent expanded index * 8 + child
};

static __host__ __device__ inline size_t mzw_hdr_bytes(int S) {
  size_t b = sizeof(float) * MZH_A * MZH_F + sizeof(double) * 2 * (size_t)(S + 3);
  return (b + 15) & ~(size_t)15;
}

__device__ __forceinline__ void mzw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Cross-row reductions over the row swaps (mzh_pair16 / mzh_pair32, mzh_device.h).
// The maxima below feed only exponent arguments (x - max: identical for a +0 / -0 max), the
// normaliser's max - min (likewise) and argmax equality masks, and no operand is NaN: v_max_f32
// (one instruction) instead of compare + select (two, with a VCC hazard wait between them).
__device__ __forceinline__ float mzw_max4g(float v) {  // max over the 4 lane groups (rows) of a column
  float a, b;
  mzh_pair16(v, a, b);
  v = __builtin_fmaxf(a, b);
  mzh_pair32(v, a, b);
  return __builtin_fmaxf(a, b);
}
// min over the 4 lane groups for the latent normalisation: no operand is NaN or -0 (a latent unit is
// an FMA chain from +0 plus a bias, which never rounds to -0), so v_min_f32 is the select's result
__device__ __forceinline__ float mzw_min4g(float v) {
  float a, b;
  mzh_pair16(v, a, b);
  v = __builtin_fminf(a, b);
  mzh_pair32(v, a, b);
  return __builtin_fminf(a, b);
}
__device__ __forceinline__ float mzw_add16(float v) {  // row0 + row1 (row2 + row3)
  float a, b;
  mzh_pair16(v, a, b);
  return a + b;
}
__device__ __forceinline__ float mzw_add32(float v) {  // rows 0-1 + rows 2-3
  float a, b;
  mzh_pair32(v, a, b);
  return a + b;
}

// ------------------------------------------------------------------------------------------
// One MLP (layer1 + bias (+ one-hot column) + ReLU -> layer2, bias2 left to the caller) for the
// wave's NT column tiles.  x[n][kb] = the B operand of column tile n, k-block kb (lane group g
// holds inputs 16kb + 4t + g, t = 0..3).  out[ot][n]: C registers of output tile ot.
// ------------------------------------------------------------------------------------------
// B32 (33-bin heads): also run this lane group's chain of bin 32 (MzhWMlp::w32) on the hidden units it
// holds, into p32[n]: hidden unit 16ht + 4t + g, ht and t ascending (oracle/mzh_oracle.c linear_head)
// The weight stream goes through a buffer resource: the lane's byte offset sits in one VGPR, the
// fragment / block offset is uniform (SGPR or immediate), so no load costs 64-bit VALU address
// arithmetic (the 64-bit pointer form spent ~13 VALU per two hidden blocks on it).
__device__ __forceinline__ floatx4 mzw_ld4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// rw: the blob's buffer resource (MzhWNet::wbase, made once per kernel: one SGPR quad for every chain)
// Chained form (WS > 0): the rolling buffer is the caller's wst[WS], which arrives holding this chain's
// block 0 (loaded by the previous chain), and the last block's refills load the NEXT chain's block 0
// (fragments 0..WS-1 at byte offset next_soff) instead of the zero pad, so no chain starts on an L2 round trip.
// b2[NO]: layer 2's bias fragments for mzw_bias2, loaded ahead of the hidden blocks so that the chain does not
// end on a load and its use (16,384 roots x 200 simulations -1.7%; 65,536 roots neutral)
template <int NT, int KB1, int NO, bool OH, bool B32 = false, int WS = 0>
__device__ __forceinline__ void mzw_chain(const MzhWMlp& L, __amdgpu_buffer_rsrc_t rw, const floatx4 (&x)[NT][4],
                                          const float* const (&oh)[NT], floatx4 (&out)[NO][NT], floatx4* b2, int lane,
                                          float* p32 = nullptr, floatx4* wst = nullptr, int next_soff = 0) {
  constexpr int FR = KB1 + NO;
  static_assert(WS == 0 || WS >= FR, "chained buffer too small");
  const int g = lane >> 4;
  const int vs = 16 * lane, vb = 16 * g;  // byte offsets: the lane's fragment slot, its group's 4 biases
#pragma unroll
  for (int ot = 0; ot < NO; ++ot)
#pragma unroll
    for (int n = 0; n < NT; ++n) out[ot][n] = floatx4{0.f, 0.f, 0.f, 0.f};
  // Rolling weight buffer: slot f holds fragment f of the current hidden block and is refilled
  // with fragment f of the next block as soon as its MFMAs are issued, so every load has the rest
  // of this block's MFMAs (and the next block's up to f) to land.  The scheduling barriers keep
  // the compiler from sinking the refills to their uses.
  floatx4 wloc[WS > 0 ? 1 : FR];
  floatx4* w = WS > 0 ? wst : wloc;
  if constexpr (WS == 0) {
#pragma unroll
    for (int f = 0; f < FR; ++f) w[f] = mzw_ld4(rw, vs, L.soff + f * 1024);
  }
#pragma unroll
  for (int ot = 0; ot < NO; ++ot) b2[ot] = mzw_ld4(rw, vb, L.b2off + 64 * ot);
  float a32[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) a32[n] = 0.0f;
#pragma unroll 2
  for (int ht = 0; ht < 16; ++ht) {
    // next block's byte offset (block 16 is the zero pad; chained: the next chain's block 0)
    const int sn = (WS > 0 && ht == 15) ? next_soff : L.soff + (ht + 1) * FR * 1024;
    const floatx4 b = mzw_ld4(rw, vb, L.b1off + 64 * ht);
    floatx4 w32 = {0.f, 0.f, 0.f, 0.f};
    if (B32) w32 = mzw_ld4(rw, vb, L.w32off + 64 * ht);
    floatx4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
      o[n] = OH ? *reinterpret_cast<const floatx4*>(oh[n] + 16 * ht) : floatx4{0.f, 0.f, 0.f, 0.f};
    floatx4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB1; ++kb) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[kb][t], x[n][kb][t], acc[n], 0, 0, 0);
      w[kb] = mzw_ld4(rw, vs, sn + kb * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
    floatx4 hid[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = acc[n][i];
        if (OH) v = v + o[n][i];  // one-hot action column (k = 64 + a)
        v = v + b[i];
        hid[n][i] = v > 0.0f ? v : 0.0f;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int ot = 0; ot < NO; ++ot)
#pragma unroll
        for (int n = 0; n < NT; ++n)
          out[ot][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[KB1 + ot][t], hid[n][t], out[ot][n], 0, 0, 0);
      if (B32) {
#pragma unroll
        for (int n = 0; n < NT; ++n) a32[n] = __builtin_fmaf(hid[n][t], w32[t], a32[n]);
        // keep the column tiles' chains apart for the SLP vectoriser: paired, they become one v_pk_fma_f32
        // fed by register-pair moves (28 VALU + 16 v_mov + 10 v_pk_* per two hidden blocks instead of 48 VALU),
        // which costs more beside the MFMAs (65,536 roots -0.7%).  -fno-slp-vectorize for the file also
        // unpacks the heads, where the packed form is the cheaper one (16,384 roots x 200 simulations +0.6%)
        if (NT > 1) asm("" : "+v"(a32[0]));
      }
    }
#pragma unroll
    for (int ot = 0; ot < NO; ++ot) w[KB1 + ot] = mzw_ld4(rw, vs, sn + (KB1 + ot) * 1024);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (WS > FR) {  // the next chain's fragments past this chain's slots
#pragma unroll
    for (int f = FR; f < WS; ++f) w[f] = mzw_ld4(rw, vs, next_soff + f * 1024);
  }
  if (B32) {
#pragma unroll
    for (int n = 0; n < NT; ++n) p32[n] = a32[n];
  }
}

template <int NT, int NO>
__device__ __forceinline__ void mzw_bias2(floatx4 (&out)[NO][NT], const floatx4* b2) {  // b2: from mzw_chain
#pragma unroll
  for (int ot = 0; ot < NO; ++ot) {
    const floatx4 b = b2[ot];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[ot][n][i] = out[ot][n][i] + b[i];
  }
}

// normalize_h_state (networks.py:191-196) of one column: lane group g holds 16 of the 64 units
template <int NT>
__device__ __forceinline__ void mzw_normalize(const floatx4 (&hp)[4][NT], int n, floatx4 (&hn)[NT][4]) {
  float mn = hp[0][n][0], mx = hp[0][n][0];
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = hp[ot][n][i];
      mn = __builtin_fminf(v, mn);  // NaN- and -0-free (see mzw_min4g)
      mx = __builtin_fmaxf(v, mx);
    }
  mn = mzw_min4g(mn);
  mx = mzw_max4g(mx);
  const float d = (mx - mn) + 9.999999939225290290778502821922302246094e-09f;
  const float y = 1.0f / d;
  // mzh_fdiv's quotients with its exactness test decided once per lane instead of once per element
  // (per column tile ~50 VALU and ~30 SALU less; 65,536 roots -0.8%).  An element flags `slow` when its
  // numerator a is non-zero and a < 2^-100 or its Markstein quotient res < 2^-100.  For a finite d,
  // res < 2^-100 implies a < 2^-99 d: if a >= 2^-100 and a >= 2^-99 d, then y = RN(1/d) is within a
  // relative 2^-22 of 1/d (2^-24 while y is normal), so q = RN(a y) >= 2^-99 (1 - 2^-21) is normal, the
  // residual r = RN(a - q d) is at most 2^-20 a in magnitude, |r y| <= 2^-19 q, and res = RN(q + r y) >=
  // q (1 - 2^-18) > 2^-100.  An infinite d gives res = NaN, which compares false: only a < 2^-100 flags.
  // So every flagged element has 0 < a < lim, and the lane's smallest non-zero numerator decides.  A lane
  // that this test flags and the per-element test would not only sends the wave to the IEEE rerun, which
  // gives the same bits wherever the Markstein form is exact.  Numerators are >= +0 (v - mn with mn the
  // column's minimum) or NaN, so the order of the non-NaN ones is that of their bit patterns, a NaN's
  // pattern lies above lim's (no flag, as in mzh_fdiv), and bits - 1 sends 0 above every pattern.
  const float lim = __builtin_fmaxf(d < __builtin_inff() ? d * 0x1p-99f : 0.0f, 0x1p-100f);
  unsigned amin = 0xFFFFFFFFu;
#pragma unroll
  for (int ot = 0; ot < 4; ++ot)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = hp[ot][n][i] - mn;
      amin = min(amin, __float_as_uint(a) - 1u);
      const float q = a * y;
      hn[n][ot][i] = __builtin_fmaf(__builtin_fmaf(-q, d, a), y, q);
    }
  const bool slow = amin < __float_as_uint(lim) - 1u;
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
#pragma unroll
      for (int i = 0; i < 4; ++i) hn[n][ot][i] = (hp[ot][n][i] - mn) / d;
  }
}

// logits_to_transformed_expected_value (networks.py:152-189) for one column of a 33-bin head.
// Slot s = 4ot + i of lane group g holds logit k = 2g + (s & 1) + 8(s >> 1) (slot 8 only for g = 0),
// so the lane's two sequential partials are the oracle's s_{2g}, s_{2g+1} and the cross-group
// adds reproduce ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).
// NO = 2: bins 0..31 in the tiles, p32 = this lane group's bin-32 chain (mzw_chain B32), b32 its bias
template <int NT, int NO>
__device__ __forceinline__ float mzw_head(const floatx4 (&l)[NO][NT], int n, int lane, float p32 = 0.0f,
                                          float b32 = 0.0f) {
  const int g = lane >> 4;
  if constexpr (NO == 1) {
    return __shfl(l[0][n][0], lane & 15);  // support 1: the raw logit (networks.py:146-148)
  } else {
  static_assert(NO == 2, "33-bin heads: two tiles + the bin-32 chains");
  const bool v8 = g == 0;
  float L[9];
#pragma unroll
  for (int s = 0; s < 8; ++s) L[s] = l[s >> 2][n][s & 3];
  L[8] = mzw_add32(mzw_add16(p32)) + b32;  // ((p0 + p1) + (p2 + p3)) + bias: bin 32 on every group
  float m = L[0];
#pragma unroll
  for (int s = 1; s < 8; ++s) m = __builtin_fmaxf(L[s], m);
  if (v8) m = __builtin_fmaxf(L[8], m);
  m = mzw_max4g(m);
  float e[9];
#pragma unroll
  for (int s = 0; s < 8; ++s) e[s] = mzh_expf_np(L[s] - m);  // arguments <= 0
  e[8] = mzh_expf_np(L[8] - m);  // evaluated on every lane (no divergent branch), kept on group 0
  e[8] = v8 ? e[8] : 0.0f;
  float s0 = e[0];
  s0 = s0 + e[2];
  s0 = s0 + e[4];
  s0 = s0 + e[6];
  if (v8) s0 = s0 + e[8];
  float s1 = e[1];
  s1 = s1 + e[3];
  s1 = s1 + e[5];
  s1 = s1 + e[7];
  float t = s0 + s1;
  t = mzw_add16(t);  // (s0+s1)+(s2+s3) | (s4+s5)+(s6+s7)
  t = mzw_add32(t);
  const float y = 1.0f / t;
  // Markstein quotients, exact while every used exponent argument is >= -65 (t lies in [1, 33], so
  // each numerator is >= e^-65 and each quotient > 2^-100: mzh_fdiv's condition, decided once per
  // lane from the smallest logit); otherwise the wave takes IEEE divisions
  float lmin = L[0];
#pragma unroll
  for (int s = 1; s < 8; ++s) lmin = __builtin_fminf(L[s], lmin);
  if (v8) lmin = __builtin_fminf(L[8], lmin);
  const bool slow = lmin - m < -65.0f;
  float pk[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const float q = e[s] * y;
    pk[s] = __builtin_fmaf(__builtin_fmaf(-q, t, e[s]), y, q);
  }
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
#pragma unroll
    for (int s = 0; s < 9; ++s) pk[s] = e[s] / t;
  }
  float pr[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) pr[s] = pk[s] * (float)(2 * g + (s & 1) + 8 * (s >> 1) - 16);
  float x0 = pr[0];
  x0 = x0 + pr[2];
  x0 = x0 + pr[4];
  x0 = x0 + pr[6];
  if (v8) x0 = x0 + pr[8];
  float x1 = pr[1];
  x1 = x1 + pr[3];
  x1 = x1 + pr[5];
  x1 = x1 + pr[7];
  float xs = x0 + x1;
  xs = mzw_add16(xs);
  xs = mzw_add32(xs);
  return mzh_signed_parabolic(xs);
  }
}

// softmax of the 6 policy logits (networks.py:83,109): lane group 0 holds logits 0-3, group 1
// logits 4-5 (registers 0,1); returns the probabilities in the same registers
__device__ __forceinline__ floatx4 mzw_policy(const floatx4 l, int lane) {
  const int g = lane >> 4;
  const bool ok01 = g < 2, ok23 = g == 0;
  float m = -__builtin_inff();
  if (ok01) {
    m = __builtin_fmaxf(l[0], m);
    m = __builtin_fmaxf(l[1], m);
  }
  if (ok23) {
    m = __builtin_fmaxf(l[2], m);
    m = __builtin_fmaxf(l[3], m);
  }
  m = mzw_max4g(m);
  // arguments <= 0 on the lanes whose result is used; evaluated on every lane (no divergent branch)
  const float x0 = mzh_expf_np(l[0] - m), x1 = mzh_expf_np(l[1] - m);
  const float x2 = mzh_expf_np(l[2] - m), x3 = mzh_expf_np(l[3] - m);
  const float e0 = ok01 ? x0 : 0.0f, e1 = ok01 ? x1 : 0.0f;
  const float e2 = ok23 ? x2 : 0.0f, e3 = ok23 ? x3 : 0.0f;
  float t = (e0 + e1) + (e2 + e3);
  t = mzw_add16(t);  // group 0: ((s0+s1)+(s2+s3)) + ((s4+s5)+(0+0))
  const float y = 1.0f / t;
  // exactness of the Markstein quotients decided once per lane, as in mzw_head (t lies in [1, 6])
  float lmin = __builtin_inff();
  if (ok01) lmin = __builtin_fminf(__builtin_fminf(l[0], l[1]), lmin);
  if (ok23) lmin = __builtin_fminf(__builtin_fminf(l[2], l[3]), lmin);
  const bool slow = lmin - m < -65.0f;
  auto mdiv = [&](float a) {
    const float q = a * y;
    return __builtin_fmaf(__builtin_fmaf(-q, t, a), y, q);
  };
  floatx4 p;
  p[0] = mdiv(e0);
  p[1] = mdiv(e1);
  p[2] = mdiv(e2);
  p[3] = mdiv(e3);
  if (__builtin_expect(__ballot(slow) != 0, 0)) {
    p[0] = e0 / t;
    p[1] = e1 / t;
    p[2] = e2 / t;
    p[3] = e3 / t;
  }
  return p;
}

// argmax over the 6 children with the reference's tie handling (mzh_tie_pick, mzh_mcts.h):
// the 6 children are split over a lane pair (i, i + 32), 3 each: the pair's
// max and its 6-bit argmax mask combine through v_permlane32_swap (max and OR are order-free), so
// both lanes return the same pick and tie bookkeeping
__device__ __forceinline__ int mzw_pick_pair(const float (&u)[3], int half, int tie, int& firstTie, int& extra) {
  float m = u[0];
  m = __builtin_fmaxf(u[1], m);
  m = __builtin_fmaxf(u[2], m);
  float a, b;
  mzh_pair32(m, a, b);
  const float M = __builtin_fmaxf(a, b);
  int mask = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) mask |= (u[j] == M ? 1 : 0) << j;
  mask <<= 3 * half;
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)mask, (unsigned)mask, false, false);
  return mzh_tie_pick(r[0] | r[1], tie, firstTie, extra);
}

// The column tiles of one M phase: NC = NT for the wave's own roots (column c of tile n is root 16n + c), or one
// tile of the roots that missed the expansion memo, packed (column c is the c-th missing root)
template <int NC>
struct MzwCols {
  int root[NC];    // the column's root (a valid address even where !valid)
  bool valid[NC];  // the column's stores count
  int en[NC], an[NC];  // the leaf's parent (expanded index) and move
  int prow[NC];    // the parent's memo row, or -1: its latent is in htree
  float val[NC], rew[NC];
  floatx4 cpi[NC];
};

// The two waves a SIMD holds drift apart.  Phase-locking them (8-wave workgroups, one barrier per
// simulation before the MLP) was measured 5-10% slower (profiles/r04_experiments.json): each
// simulation then waits for the deepest of 256 roots.
template <int NT, bool REPLAY, bool SUP33>
__global__ __launch_bounds__(MZW_WAVES * 64, 2) void mzh_wave_kernel(MzhWNet net, MzhSearchParams p) {
  constexpr int NOV = SUP33 ? 2 : 1;  // value / reward output tiles (bin 32 of 33: vector chains)
  constexpr int ROOTS = 16 * NT;  // roots per wave
  const float* const noh[NT] = {};  // "no one-hot column" for the chains that take none
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int S = p.S;
  float* ohl = reinterpret_cast<float*>(smem_raw);
  double* table = reinterpret_cast<double*>(smem_raw + sizeof(float) * MZH_A * MZH_F);
  MzwWave<ROOTS>* wsa = reinterpret_cast<MzwWave<ROOTS>*>(smem_raw + mzw_hdr_bytes(S));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (scalar branches)
  const int g = lane >> 4, col = lane & 15;
  const __amdgpu_buffer_rsrc_t rw = mzh_rsrc(net.wbase);

  if (!REPLAY)
    for (int i = tid; i < MZH_A * MZH_F; i += MZW_WAVES * 64) ohl[i] = net.oh[i];
  double* inv = table + (S + 3);
  for (int i = tid; i < S + 3; i += MZW_WAVES * 64) {
    table[i] = i < S + 2 ? p.table[i] : 0.0;
    inv[i] = 1.0 / (double)i;  // IEEE division: correctly rounded
  }
  __syncthreads();  // the only barrier: from here on every wave runs independently
  const int wr0 = (blockIdx.x * MZW_WAVES + wave) * ROOTS;
  if (wr0 >= p.B) return;  // wave-uniform
  MzwWave<ROOTS>& ws = wsa[wave];
  const double disc = p.discount;
  const bool noised = p.noise != nullptr;
  const size_t E = (size_t)p.E;

  // root lanes: lanes rho and rho + 32 (rho < ROOTS) both own root wr0 + rho in the tree phases:
  // selection splits the 6 children between them (3 UCBs per lane), every other tree step's loads and
  // arithmetic run mirrored on both (same values, same addresses); of the expansion's and backup's stores each
  // is issued by one lane of the pair (phase_head)
  const int rho = lane & 31;
  const int half = lane >> 5;
  const int rroot = wr0 + rho;
  const bool rvalid = rho < ROOTS && rroot < p.B;
  // the root's tree blocks: block e is TB(e) (the root's first block as a 32-bit index, not a pointer: one register)
  const int tb0 = (rvalid ? rroot : 0) * p.E;
  auto TB = [&](int e) -> MzwBlock& { return reinterpret_cast<MzwBlock*>(p.tree)[(size_t)(unsigned)(tb0 + e)]; };
  MzhMinMax mm;
  if (rvalid && p.minmax_in)
    mm.set(p.minmax_in[2 * rroot], p.minmax_in[2 * rroot + 1]);
  else
    mm.set(-__builtin_inf(), __builtin_inf());
  int firstTie = 0, extra = 0, steps = 0, rootN = 0, depth = 0;
  // the selected leaf as a path slot, its parent's expanded index * 8 + the move (below 2^18), and above it the
  // entries of this root's miss log (at most MZH_MEMO_LOG_CAP_MAX): one register for both
  int leaf = 0;
  int lsum = 0;  // p.lockstep_levels: the wave's deepest selection below the root, summed over simulations
  double rootW = 0.0;
  const int tie = (rvalid && p.tie_idx) ? p.tie_idx[rroot] : 0;
  // the expansion memo (mzh.h): a root lane's state index when its observation row is exactly one-hot per disc
  // (one 1.0f, two +0.0f, by bit pattern), else -1: that root never touches the table.  pid: the id of the
  // leaf's parent node, carried through selection (meaningful while the parent's depth is <= memo_D)
  const bool memo = !REPLAY && p.memo_h != nullptr;  // wave-uniform
  int sigma = -1;
  unsigned pid = 0;
  unsigned row1 = 0;  // the leaf's parent block's memo row + 1, from selection's last load (0 while the walk ends at the root)
  unsigned cnt = 0;  // simulations without an M phase (low 16 bits; S <= 32000) | with the packed one (high 16)
  // the grown extension (wave-uniform): grow = its links are consulted below the dense depth; glog = this launch
  // logs its misses for the harvest (not once the extension is full).  nlog: entries of this root's log
  const bool grow = memo && p.memo_link != nullptr;
  const bool glog = grow && p.memo_log != nullptr && p.memo_ctr[0] < p.memo_cap;
  if (memo && rvalid) {
    const unsigned* orow = reinterpret_cast<const unsigned*>(p.obs) + (size_t)rroot * p.in_dim;
    int sg = 0, w3 = 1;
    bool ok = true;
    for (int i = 0; 3 * i + 2 < p.in_dim; ++i, w3 *= 3) {
      const unsigned a0 = orow[3 * i], a1 = orow[3 * i + 1], a2 = orow[3 * i + 2];
      const unsigned one = 0x3F800000u;
      const int n1 = (a0 == one) + (a1 == one) + (a2 == one), n0 = (a0 == 0u) + (a1 == 0u) + (a2 == 0u);
      ok = ok && n1 == 1 && n0 == 2;
      sg += w3 * (a1 == one ? 1 : a2 == one ? 2 : 0);
    }
    sigma = ok ? sg : -1;
  }

  // column lanes: lane (g, col) works on root wr0 + 16n + col of column tile n (MLP phases)
  int croot[NT];
  bool cvalid[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    croot[n] = wr0 + 16 * n + col;
    cvalid[n] = croot[n] < p.B;
  }

  // ---------------- root: initial_inference (mcts.py:49-50) + root.expand (mcts.py:57-69) ----------------
  floatx4 rpi[NT];
  // A wave whose every valid root is a state's observation takes the root priors from the table's depth-0 records
  // and runs no root chain (at launch every wave is in its root chains at once, so they are MFMA-bound with no tree
  // phase beside them).  Such a root's depth-1 expansions gather the root latent from the table as well (prow_r
  // below: depth - 1 = 0 <= memo_D), so nothing reads its htree slot 0, which is left unwritten.
  const bool rtab = memo && __ballot(rvalid && sigma < 0) == 0;  // wave-uniform
  if (!REPLAY && rtab) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int sg = __shfl(sigma, 16 * n + col);
      rpi[n] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (cvalid[n] && g < 2) {  // lane group 0: priors 0-3, group 1: priors 4, 5 (mzw_policy's registers)
        const float* rec = p.memo_rec + (size_t)sg * p.memo_K * 8 + 4 * g;
        if (g == 0) {
          rpi[n] = *reinterpret_cast<const floatx4*>(rec);
        } else {
          rpi[n][0] = rec[0];
          rpi[n][1] = rec[1];
        }
      }
    }
  } else if (!REPLAY) {
    floatx4 hreg[NT][4];  // the root's normalised latent (B-operand order)
    floatx4 x[NT][4];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = 16 * kb + 4 * t + g;
          x[n][kb][t] = (cvalid[n] && k < p.in_dim) ? p.obs[(size_t)croot[n] * p.in_dim + k] : 0.0f;
        }
    floatx4 hp[4][NT];
    floatx4 b2[4];  // a chain's layer-2 bias fragments, loaded by the chain (mzw_chain b2)
    switch (net.rep.kb1) {
      case 1: mzw_chain<NT, 1, 4, false>(net.rep, rw, x, noh, hp, b2, lane); break;
      case 2: mzw_chain<NT, 2, 4, false>(net.rep, rw, x, noh, hp, b2, lane); break;
      case 3: mzw_chain<NT, 3, 4, false>(net.rep, rw, x, noh, hp, b2, lane); break;
      default: mzw_chain<NT, 4, 4, false>(net.rep, rw, x, noh, hp, b2, lane); break;
    }
    mzw_bias2<NT, 4>(hp, b2);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      mzw_normalize<NT>(hp, n, hreg);
      if (cvalid[n]) {
        floatx4* dst = reinterpret_cast<floatx4*>(p.htree + ((size_t)croot[n] * E) * MZH_H) + g;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) dst[4 * kb] = hreg[n][kb];
      }
    }
    floatx4 pl[1][NT];
    mzw_chain<NT, 4, 1, false>(net.pol, rw, hreg, noh, pl, b2, lane);
    mzw_bias2<NT, 1>(pl, b2);
    floatx4 vl[NOV][NT];
    mzw_chain<NT, 4, NOV, false>(net.val, rw, hreg, noh, vl, b2, lane);  // root value: computed, unused (mcts.py:50)
    (void)vl;
#pragma unroll
    for (int n = 0; n < NT; ++n) rpi[n] = mzw_policy(pl[0][n], lane);
  }
  // root children: prior (Dirichlet-mixed when noised), N = 0, unexpanded
  if (g < 2) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 4 * g + i;
        if (c < MZH_A && cvalid[n]) {
          const float pr = REPLAY ? p.rp_root_pi[(size_t)croot[n] * MZH_A + c] : rpi[n][i];
          ws.rP[c][16 * n + col] =
              mzh_root_prior(pr, noised, p.eps, noised ? p.noise[(size_t)croot[n] * MZH_A + c] : 0.0);
        }
      }
  }
  if (lane < ROOTS) {
#pragma unroll
    for (int c = 0; c < MZH_A; ++c) {
      ws.rW[c][rho] = 0.0;
      ws.rR[c][rho] = 0.0f;
      ws.rN[c][rho] = 0;
      ws.rX[c][rho] = -1;
    }
  }
  mzw_wave_sync();

  MzwCols<NT> cf;  // the wave's own column tiles
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    cf.root[n] = cvalid[n] ? croot[n] : 0;
    cf.valid[n] = cvalid[n];
    cf.prow[n] = -1;
  }
  MzwCols<1> cp;  // the packed tile of the roots that missed the memo (32-root waves)

  // the four recurrent chains' rolling weight buffer, handed from chain to chain (mzw_chain WS)
  floatx4 wst[8];
  if (!REPLAY) {
#pragma unroll
    for (int f = 0; f < 8; ++f) wst[f] = mzw_ld4(rw, 16 * lane, net.dyn.soff + f * 1024);
  }
  MZH_STAMP_DECL  // diagnostic build: phase stamps per simulation (MZH_STAMP 0-11, read by tools/wave_stamps.py)
  // select one leaf per root, then hand its parent latent index / move to the column lanes
  // ex: MzhBool<true> = the exact (IEEE-division) normaliser, for a wave where some root's max - min
  // is a non-zero subnormal (caller-given bounds only); chosen once per selection
  auto phase_select = [&](int s, auto ex) {
    (void)s;
    constexpr bool exact = decltype(ex)::value;
    // ---------------- select (mcts.py:75-86; node.py:72-123): one lane per root ----------------
    if (rvalid) {
      const bool has = mm.has();
      const double mmin = mm.mmin, den = mm.den, dinv = mm.dinv;
      float u[3];
      const double tr = table[rootN];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int c = 3 * half + j;
        u[j] = mzh_ucb(ws.rN[c][rho], ws.rW[c][rho], ws.rR[c][rho], ws.rP[c][rho], noised || p.np1, tr, disc, has,
                       mmin, den, dinv, inv, exact);
      }
      int pick = mzw_pick_pair(u, half, tie, firstTie, extra);
      int Np = ws.rN[pick][rho], X = ws.rX[pick][rho];
      ws.path[0][rho] = (uint16_t)pick;
      ws.pcW[0][rho] = ws.rW[pick][rho];
      ws.pcR[0][rho] = ws.rR[pick][rho];
      ws.pcN[0][rho] = Np;
      int e = 0, d = 1;
      pid = 0;
      row1 = 0;
      // 16-root waves (NT = 1) prefetch the children's blocks one level ahead (16,384 roots: 2.66 ->
      // 2.57 ms); at 32 roots per wave the partner wave's MFMA stream already covers the latency
      // (65,536 roots: neutral; measured again with the expansion memo's shorter M phase: 65,536 roots +1.7%,
      // 262,144 seven-disc roots +4.1%), so NT = 2 leaves the load queue to the block loads
      constexpr bool kPF = NT == 1;
      int pf0 = 0, pf1 = 0, pf2 = 0;
      // (a root lane touching its leaf's parent latent when its walk ends, ahead of the M phase's gather,
      // measured slower: 65,536 roots +0.6%, 16,384 roots x 200 simulations +3.7%)
      while (X >= 0 && d <= S) {  // depth <= s + 1 always; the bound only guards against a corrupt tree
        e = X;
        pid = 6u * pid + (unsigned)pick + 1u;  // the node stepped into (wraps far below memo_D: unused there)
        int nx;
        double Wp;
        float Rp;
        {
          // this lane's half of the block only -- its three children's units and their priors (4 aligned
          // 16-B loads instead of the whole 128-B line on both lanes and a select of each field by half);
          // the picked child's unit comes from the lane that holds it over v_permlane32_swap
          // (16,384 roots -1.4%; at 32 roots per wave, once the buffer-load weight stream freed the
          // registers it spilled in round 3: 65,536 roots -0.9%, 262,144 -1.3%)
          const uint4* hb = reinterpret_cast<const uint4*>(&TB(e).h[half]);
          uint4 u0 = hb[0], u1 = hb[1], u2 = hb[2], hP = hb[3];
          // the first unit's words through an empty asm: left alone, the compiler loads that unit's W a second
          // time as a dwordx2 beside the dwordx4 (five loads and 18 dwords per lane and level instead of 4 and 16),
          // and the layout then loses to the one before it.  This depends on the compiler:
          // tests/test_wave_layout_cpu.py compiles this file and checks that a level is exactly four dwordx4, so
          // a compiler upgrade that splits or narrows them again fails there
          asm("" : "+v"(u0.x), "+v"(u0.y), "+v"(u0.z), "+v"(u0.w));
          // (the replay instantiations split the third unit's W instead: the other two units' W words as well)
          asm("" : "+v"(u1.x), "+v"(u1.y), "+v"(u2.x), "+v"(u2.y));
          row1 = hP.w;  // the level's memo row + 1 rides in the priors' chunk (the lookup below the dense depth)
          const int hn[3] = {(int)u0.z, (int)u1.z, (int)u2.z};
          const float hr[3] = {__uint_as_float(u0.w), __uint_as_float(u1.w), __uint_as_float(u2.w)};
          const float hp[3] = {__uint_as_float(hP.x), __uint_as_float(hP.y), __uint_as_float(hP.z)};
          const double hw[3] = {__hiloint2double((int)u0.y, (int)u0.x), __hiloint2double((int)u1.y, (int)u1.x),
                                __hiloint2double((int)u2.y, (int)u2.x)};
          if (kPF) {
            asm volatile("" ::"v"(pf0), "v"(pf1), "v"(pf2));
            const int x0 = hn[0] >> 16, x1 = hn[1] >> 16, x2 = hn[2] >> 16;
            pf0 = *reinterpret_cast<const int*>(&TB(x0 >= 0 ? x0 : e));
            pf1 = *reinterpret_cast<const int*>(&TB(x1 >= 0 ? x1 : e));
            pf2 = *reinterpret_cast<const int*>(&TB(x2 >= 0 ? x2 : e));
          }
          const double tn = table[Np];
  #pragma unroll
          for (int j = 0; j < 3; ++j) u[j] = mzh_ucb(hn[j] & 0xFFFF, hw[j], hr[j], (double)hp[j], p.np1, tn, disc, has, mmin, den, dinv, inv, exact);
          pick = mzw_pick_pair(u, half, tie, firstTie, extra);
          // this lane's candidate for the picked slot (valid on the owning half), then the owner's copy
          const int jl = pick - 3 * half;
          int cn = hn[0];
          float cr = hr[0];
          double cw = hw[0];
  #pragma unroll
          for (int q = 1; q < 3; ++q)
            if (jl == q) {
              cn = hn[q];
              cr = hr[q];
              cw = hw[q];
            }
          auto take = [&](unsigned v) {
            const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            // r = {lanes 0-31 value, lanes 32-63 value} on both lanes of the pair
            return pick >= 3 ? r[1] : r[0];
          };
          nx = (int)take((unsigned)cn);
          Rp = __uint_as_float(take(__float_as_uint(cr)));
          const long long wb = __double_as_longlong(cw);
          Wp = __hiloint2double((int)take((unsigned)(wb >> 32)), (int)take((unsigned)(wb & 0xFFFFFFFFll)));
        }
        Np = nx & 0xFFFF;
        X = nx >> 16;
        const uint16_t slot = (uint16_t)(e * 8 + pick);
        if (d < MZW_DC) {
          ws.path[d][rho] = slot;
          ws.pcW[d][rho] = Wp;
          ws.pcR[d][rho] = Rp;
          ws.pcN[d][rho] = Np;
        } else {
          p.pathx[(size_t)rroot * E + d] = slot;
        }
        ++d;
      }
      if (kPF) asm volatile("" ::"v"(pf0), "v"(pf1), "v"(pf2));
      depth = d;
      leaf = (leaf & ~0x3FFFF) | (e * 8 + pick);
      steps += d;
    }
    if (p.lockstep_levels) {  // wave-uniform: only when the caller asks for the latency model's input
      int m = rvalid ? depth - 1 : 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
      lsum += m;
    }
  };

  // M phase: recurrent_inference's four MLPs (networks.py:96-150) as MFMA chains, each head
  // evaluated right after its chain (only scalars stay live)
  auto phase_mlp = [&](int s, auto& C) {
    if (REPLAY) return;
    constexpr int NC = sizeof(C.root) / sizeof(int);
    const float* const nohc[NC] = {};
    floatx4 rl[NOV][NC], pl[1][NC], vl[NOV][NC];  // reward / policy / value logits
    // the leaf's parent latent (mcts.py:89-92), stored by an earlier M phase (or the root inference), or the
    // memo's row where the parent is a memo node (those are never copied into htree)
    floatx4 x[NC][4];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      const float* row = C.prow[n] >= 0 ? p.memo_h + (size_t)C.prow[n] * MZH_H
                                        : p.htree + ((size_t)C.root[n] * E + C.en[n]) * MZH_H;
      const floatx4* src = reinterpret_cast<const floatx4*>(row) + g;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) x[n][kb] = src[4 * kb];
    }
    floatx4 hreg[NC][4];  // the new node's normalised latent
    floatx4 hp[4][NC];
    const float* ohp[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) ohp[n] = ohl + C.an[n] * MZH_F + 4 * g;
    MZH_STAMP(10);  // latent gather
    floatx4 b2[4];  // a chain's layer-2 bias fragments, loaded by the chain (mzw_chain b2)
    mzw_chain<NC, 4, 4, true, false, 8>(net.dyn, rw, x, ohp, hp, b2, lane, nullptr, wst, net.rwd.soff);
    mzw_bias2<NC, 4>(hp, b2);  // h' (un-normalised, networks.py:129-138)
    MZH_STAMP(5);
    floatx4 hx[NC][4];
#pragma unroll
    for (int n = 0; n < NC; ++n)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) hx[n][kb] = hp[kb][n];
    float r32[NC], v32[NC];
    mzw_chain<NC, 4, NOV, false, SUP33, 8>(net.rwd, rw, hx, nohc, rl, b2, lane, r32, wst, net.pol.soff);  // reward from h' (networks.py:132-135)
    mzw_bias2<NC, NOV>(rl, b2);
    MZH_STAMP(6);
#pragma unroll
    for (int n = 0; n < NC; ++n) C.rew[n] = mzw_head<NC, NOV>(rl, n, lane, SUP33 ? r32[n] : 0.0f, net.rwd.b32);
    MZH_STAMP(11);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      mzw_normalize<NC>(hp, n, hreg);
      if (C.valid[n]) {
        floatx4* dst = reinterpret_cast<floatx4*>(p.htree + ((size_t)C.root[n] * E + s + 1) * MZH_H) + g;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) dst[4 * kb] = hreg[n][kb];
      }
    }
    MZH_STAMP(7);
    mzw_chain<NC, 4, 1, false, false, 8>(net.pol, rw, hreg, nohc, pl, b2, lane, nullptr, wst, net.val.soff);
    mzw_bias2<NC, 1>(pl, b2);
#pragma unroll
    for (int n = 0; n < NC; ++n) C.cpi[n] = mzw_policy(pl[0][n], lane);
    MZH_STAMP(8);
    mzw_chain<NC, 4, NOV, false, SUP33, 8>(net.val, rw, hreg, nohc, vl, b2, lane, v32, wst, net.dyn.soff);  // + next dyn block 0
    mzw_bias2<NC, NOV>(vl, b2);
    MZH_STAMP(9);
#pragma unroll
    for (int n = 0; n < NC; ++n) C.val[n] = mzw_head<NC, NOV>(vl, n, lane, SUP33 ? v32[n] : 0.0f, net.val.b32);
  };

  // the new nodes' blocks of the columns an M phase evaluated
  // hrow (root lanes, the wave's own tiles only): the table row of a root that hit, or -1; its row + 1 goes into
  // the block's two row words so that the node's children find their parent's row (0: not a table node)
  auto phase_blocks = [&](int s, auto& C, bool own, int hrow) {
    constexpr int NC = sizeof(C.root) / sizeof(int);
    unsigned trow[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) trow[n] = own ? (unsigned)(__shfl(hrow, 16 * n + col) + 1) : 0u;
    // the new node's 6 children (node.py:44-49): N = 0, X = -1, R = 0, P, W = 0.  The whole 128-B
    // line as eight 16-B stores, two per lane group: a line written whole is valid in L2 without a fill
    // from HBM.  Chunk k = bytes 16k..16k+15: 0-2 children 0-2 | 3 P0-2 row | 4-6 children 3-5 | 7 P3-5 row.
    // Lane groups 0 / 1 hold pi[0..3] / pi[4..5], so group 1 takes P3 from group 0 over one row swap
    // (v_permlane16_swap: every lane runs it, ahead of the columns' branches)
    float p3[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      float hi;
      mzh_pair16(C.cpi[n][3], p3[n], hi);  // rows 0 and 1: row 0's value
      (void)hi;
    }
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      if (!C.valid[n]) continue;
      uint4* nb = reinterpret_cast<uint4*>(reinterpret_cast<MzwBlock*>(p.tree) + (size_t)C.root[n] * E + s + 1);
      const uint4 eu = make_uint4(0u, 0u, 0xFFFF0000u, 0u);  // an empty child: W = 0 | N = 0, X = -1 | R = 0
      uint4 c1 = eu;
      if (g == 0)
        c1 = make_uint4(__float_as_uint(C.cpi[n][0]), __float_as_uint(C.cpi[n][1]), __float_as_uint(C.cpi[n][2]), trow[n]);
      else if (g == 1)
        c1 = make_uint4(__float_as_uint(p3[n]), __float_as_uint(C.cpi[n][0]), __float_as_uint(C.cpi[n][1]), trow[n]);
      // g0: chunks 0, 3; g1: chunks 4, 7; g2: chunks 1, 2; g3: chunks 5, 6
      const int k0 = 4 * (g & 1) + (g >> 1), k1 = g < 2 ? 4 * g + 3 : k0 + 1;
      nb[k0] = eu;
      nb[k1] = c1;
    }
  };

  // the new node's block, then backup (node.py:30-70)
  // fromrec (root lanes): the new node's outputs come from a 32-byte record -- the replay records, or the
  // memo's row of a root that hit it in a simulation that ran no MLP for it; else vcol / rcol: the value and
  // reward its column evaluated
  // hrow: the memo row of a root that hit (dense or grown), -1 otherwise.  A root that missed although its
  // observation is a state's appends the new node to its miss log (dropped when the log is full: the node is
  // then inserted by a later launch)
  auto phase_head = [&](int s, bool fromrec, float vcol, float rcol, int hrow) {
    // ---------------- expand bookkeeping + backup (node.py:30-70): one lane per root ----------------
    if (rvalid) {
      const int enew = s + 1;
      const int leafE = (leaf & 0x3FFFF) >> 3, leafA = leaf & 7;
      float vv, rr;
      if (REPLAY || fromrec) {
        const uint4* rec = reinterpret_cast<const uint4*>(
            REPLAY ? p.rp_sim + ((size_t)s * p.B + rroot) * 8 : p.memo_rec + (size_t)hrow * 8);
        const uint4 r0 = rec[0], r1 = rec[1];  // priors 0-3 | priors 4, 5, reward, value
        rr = __uint_as_float(r1.z);
        vv = __uint_as_float(r1.w);
        // the whole 128-B line as eight 16-B stores (see phase_blocks), each lane of the pair its own half:
        // three empty children, then its three priors (half 0: 0-2, half 1: 3-5) and the node's row + 1
        uint4* nb = reinterpret_cast<uint4*>(&TB(enew).h[half]);
        const uint4 eu = make_uint4(0u, 0u, 0xFFFF0000u, 0u);  // W = 0 | N = 0, X = -1 | R = 0
        const bool h1 = half != 0;
        nb[0] = eu;
        nb[1] = eu;
        nb[2] = eu;
        nb[3] = make_uint4(h1 ? r0.w : r0.x, h1 ? r1.x : r0.y, h1 ? r1.y : r0.z, REPLAY ? 0u : (unsigned)(hrow + 1));
      } else {
        vv = vcol;
        rr = rcol;
        if (!REPLAY && glog && sigma >= 0 && hrow < 0 && (leaf >> 18) < p.memo_logcap) {
          // (the entry's address is made here from an opaque copy of the root: hoisted out of the simulation
          // loop, the root's log pointer is two more registers across the M phase -- scratch at 32 roots per wave)
          int ro = rroot;
          asm volatile("" : "+v"(ro));
          if (!half)
            p.memo_log[(unsigned)(ro * p.memo_logcap + (leaf >> 18))] =
                make_uint4((unsigned)enew, (unsigned)(leaf & 0x3FFFF), __float_as_uint(vv), __float_as_uint(rr));
          leaf += 1 << 18;
        }
      }
      // this phase's stores: the pair's lanes hold the same values for the same addresses, so one of them stores
      // (st); the loads and the arithmetic stay mirrored, both lanes need the values.  The next selection reads
      // them on both lanes behind the simulation loop's closing fence.  (Selection's own path-cache stores stay
      // mirrored: one lane storing them measured no gain)
      // A tree block's child slot takes the new node's index and reward with backup's store of the whole unit
      // below; only the root's children (LDS) are linked here
      const bool st = !half;
      if (st && leafE == 0) {
        ws.rX[leafA][rho] = enew;
        ws.rR[leafA][rho] = rr;
      }
      MZH_STAMP(12);  // record + new block: closes when the stores are issued
      double v = (double)vv;
      double lmax = -__builtin_inf(), lmin = __builtin_inf();
      // path entry j: slot (parent expanded index * 8 + child) and the child's statistics at
      // selection time; entry j - 1 is loaded while entry j is processed
      auto load_lds = [&](int j, int& slot, double& W, float& R, int& N) {
        slot = ws.path[j][rho];
        W = ws.pcW[j][rho];
        R = ws.pcR[j][rho];
        N = ws.pcN[j][rho];
      };
      auto load_hbm = [&](int j, int& slot, double& W, float& R, int& N) {  // depths >= MZW_DC
        slot = p.pathx[(size_t)rroot * E + j];
        const int e = slot >> 3, a = slot & 7;
        uint4 un = reinterpret_cast<const uint4*>(&TB(e))[a + (a >= 3)];  // the child's unit (chunks 3, 7: priors)
        asm("" : "+v"(un.x), "+v"(un.y), "+v"(un.z), "+v"(un.w));  // one dwordx4 (else: a ushort and a dwordx3)
        W = __hiloint2double((int)un.y, (int)un.x);
        R = __uint_as_float(un.w);
        N = (int)(un.z & 0xFFFFu);
      };
      int slot;
      double Wj;
      float Rj;
      int Nj;
      // path node j: its statistics (W += v, N += 1), the MinMaxStats candidate, the value chain
      auto node = [&](int j, double& Wn, int& Nn) {
        const double rw = (j == depth - 1) ? (double)rr : (double)Rj;
        Wn = Wj + v;
        Nn = Nj + 1;
        const double q = rw + disc * mzh_div(Wn, (double)Nn, inv[Nn]);  // MinMaxStats input
        lmax = q > lmax ? q : lmax;
        lmin = q < lmin ? q : lmin;
        v = rw + disc * v;
      };
      if (depth - 1 < MZW_DC) load_lds(depth - 1, slot, Wj, Rj, Nj);
      else load_hbm(depth - 1, slot, Wj, Rj, Nj);
      // depths j >= 1 sit in HBM tree blocks (e >= 1), depth 0 is the root's child in LDS (peeled: no
      // per-node branch on where the statistics live); entry j - 1 loaded while node j is processed
      int j = depth - 1;
      // The node's whole unit in one aligned 16-B store: beside W and N, the child's expanded index and reward --
      // for the leaf's slot the new node and its reward (the expansion's link), above it what the slot holds
      // already, the block the next path entry stepped into and the cached reward
      int xn = enew;
      auto hbm_node = [&](int jn) {
        const int e = slot >> 3, a = slot & 7;
        double Wn;
        int Nn;
        node(jn, Wn, Nn);
        if (st) {
          const float rs = (jn == depth - 1) ? rr : Rj;
          const long long wb = __double_as_longlong(Wn);
          reinterpret_cast<uint4*>(&TB(e))[a + (a >= 3)] =
              make_uint4((unsigned)(wb & 0xFFFFFFFFll), (unsigned)(wb >> 32), ((unsigned)Nn & 0xFFFFu) | ((unsigned)xn << 16),
                         __float_as_uint(rs));
        }
        xn = e;
      };
      for (; j >= 1; --j) {
        int slot_n, Nj_n;
        double Wj_n;
        float Rj_n;
        if (j - 1 < MZW_DC) load_lds(j - 1, slot_n, Wj_n, Rj_n, Nj_n);
        else load_hbm(j - 1, slot_n, Wj_n, Rj_n, Nj_n);  // paths deeper than the LDS cache (rare)
        hbm_node(j);
        slot = slot_n;
        Wj = Wj_n;
        Rj = Rj_n;
        Nj = Nj_n;
      }
      {  // depth 0: the root's child (path slot = child index, e = 0)
        const int a = slot & 7;
        double Wn;
        int Nn;
        node(0, Wn, Nn);
        if (st) {
          ws.rW[a][rho] = Wn;
          ws.rN[a][rho] = Nn;
        }
      }
      rootW = rootW + v;
      rootN = rootN + 1;
      const double q = 0.0 + disc * mzh_div(rootW, (double)rootN, inv[rootN]);  // root rwd = 0.0
      lmax = q > lmax ? q : lmax;
      lmin = q < lmin ? q : lmin;
      mm.update(lmax, lmin);
    }
  };

  for (int s = 0; s < S; ++s) {
    MZH_STAMP(4);
    if (__builtin_expect(mzh_need_exact(rvalid && mm.has(), mm.den), 0))
      phase_select(s, MzhBool<true>{});
    else
      phase_select(s, MzhBool<false>{});
    MZH_STAMP(0);
    // a wave in its matrix phase wins VALU issue arbitration over the co-resident wave's tree work
    // (measured against the tree phases first and against no priorities: profiles/r04_experiments.json)
    __builtin_amdgcn_s_setprio(1);
    // Which M phase the simulation needs (wave-uniform).  A root misses the memo when its observation is not a
    // state's (sigma < 0) or its new node lies deeper than the table.  mode 0: no root misses, no chain runs;
    // mode 1 (32-root waves): at most 16 miss and are packed into one column tile -- half the MFMAs, in-chain
    // epilogues and heads; mode 2: the wave's own tiles, as without a memo (the hits are evaluated too)
    int mode = 2, nm = 0;
    unsigned mask = 0;
    bool hit = false;
    // the memo rows (root lanes) of the leaf's parent and of the new node, -1 without one.  Down to the dense
    // depth a row is arithmetic; below it the parent's comes from its block's row word, which selection's last
    // load brought (no load here), and the new node's from the parent's child link.  A memo node's latent is
    // read from the table, never from htree
    int prow_r = -1, hrow = -1;
    const int leafA = leaf & 7;
    if (memo && sigma >= 0) {  // (sigma >= 0 only on valid root lanes)
      if (depth - 1 <= p.memo_D) prow_r = sigma * p.memo_K + (int)pid;
      else if (grow) prow_r = (int)row1 - 1;  // (depth - 1 > D >= 0: the walk went through a block, row1 is its word)
      if (depth <= p.memo_D) {
        hrow = sigma * p.memo_K + (int)(6u * pid + (unsigned)leafA + 1u);
      } else if (grow && prow_r >= 0) {
        const int l = p.memo_link[prow_r * 6 + leafA];
        hrow = l > 0 ? l : -1;
      }
    }
    if (memo) {
      hit = hrow >= 0;
      // bit rho: lanes 0-31 (lanes 32-63 mirror them)
      mask = __builtin_amdgcn_readfirstlane((unsigned)__ballot(rvalid && !hit));
      nm = __popc(mask);
      mode = nm == 0 ? 0 : (NT == 2 && nm <= 16) ? 1 : 2;
      cnt = __builtin_amdgcn_readfirstlane(cnt + (mode == 0 ? 1u : mode == 1 ? 0x10000u : 0u));
    }
    MZH_STAMP(3);  // memo lookup + mode ballot
    float vcol = 0.0f, rcol = 0.0f;
    if (mode == 2) {
      if (!REPLAY) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int lf = __shfl(leaf, 16 * n + col);
          cf.en[n] = (lf & 0x3FFFF) >> 3;
          cf.an[n] = lf & 7;
          if (memo) cf.prow[n] = __shfl(prow_r, 16 * n + col);
        }
        phase_mlp(s, cf);
        // root lane rho is column rho & 15 of tile rho >> 4 (every row of a column holds its scalars)
        vcol = cf.val[0];
        rcol = cf.rew[0];
#pragma unroll
        for (int n = 1; n < NT; ++n)
          if ((rho >> 4) == n) {
            vcol = cf.val[n];
            rcol = cf.rew[n];
          }
      }
    } else if constexpr (NT == 2) {
     if (mode == 1) {
      // pack: the c-th missing root (ascending rho) becomes column c.  A lane permutation sends each missing
      // root lane's rho to lane rank = missing roots below it; the other lanes of rows 0-31 fill nm..31 and
      // lanes 32-63 stay, so every lane is written exactly once
      const int rank = __popc(mask & ((1u << rho) - 1u));
      const bool missl = (mask >> rho) & 1u;
      const int dest = half ? lane : (missl ? rank : nm + rho - rank);
      const int rsel = __builtin_amdgcn_ds_permute(dest << 2, rho);
      const bool pv = col < nm;
      const int rs = __shfl(rsel, col);
      const int r = pv ? rs : (int)__builtin_ctz(mask);  // spare columns repeat the first missing root
      cp.root[0] = wr0 + r;
      cp.valid[0] = pv;
      const int lf = __shfl(leaf, r);
      cp.en[0] = (lf & 0x3FFFF) >> 3;
      cp.an[0] = lf & 7;
      cp.prow[0] = __shfl(prow_r, r);
      phase_mlp(s, cp);
      vcol = __shfl(cp.val[0], rank);  // a missing root's column is its rank (every row holds the scalars)
      rcol = __shfl(cp.rew[0], rank);
     }
    }
    __builtin_amdgcn_s_setprio(0);
    MZH_STAMP(1);
    if (!REPLAY) {
      if (mode == 2) phase_blocks(s, cf, true, hrow);  // (the own tiles evaluate the roots that hit as well)
      else if (NT == 2 && mode == 1) phase_blocks(s, cp, false, -1);  // (cp is never valid in a 16-root wave)
    }
    phase_head(s, mode != 2 && hit, vcol, rcol, hrow);
    MZH_STAMP(2);
    // this simulation's tree stores (other lanes' new-block writes) before the next selection
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }

  // ---------------- results (mcts.py:111-126, 154-176) ----------------
  if (p.lockstep_levels && lane == 0) p.lockstep_levels[blockIdx.x * MZW_WAVES + wave] = lsum;
  if (memo && lane == 0) {  // one vector atomic per counter and wave
    const unsigned nskip = cnt & 0xFFFFu, npack = cnt >> 16;
    atomicAdd(p.memo_cnt + 0, (unsigned long long)nskip);
    atomicAdd(p.memo_cnt + 1, (unsigned long long)npack);
    atomicAdd(p.memo_cnt + 2, (unsigned long long)((unsigned)S - nskip - npack));
    // the extension's rows before this launch's harvest (nothing changes them while a search runs)
    if (p.memo_logn && blockIdx.x == 0 && wave == 0) p.memo_ctr[1] = p.memo_ctr[0];
  }
  if (!rvalid || half) return;
  if (!REPLAY && p.memo_logn) p.memo_logn[rroot] = leaf >> 18;
  int vis[MZH_A];
  for (int a = 0; a < MZH_A; ++a) vis[a] = ws.rN[a][rho];
  mzh_write_results(p, rroot, vis, rootW, rootN, mm.mmax, mm.mmin, extra, steps, depth, [&](int j) {
    return j < MZW_DC ? (int)ws.path[j][rho] : (int)p.pathx[(size_t)rroot * E + j];
  });
}

size_t mzh_wave_smem_bytes(int S, int nt) {
  return mzw_hdr_bytes(S) + (nt == 1 ? sizeof(MzwWave<16>) : sizeof(MzwWave<32>)) * MZW_WAVES;
}

template <int NT, bool REPLAY, bool SUP33>
static hipError_t launch_wave_t(const MzhWNet& net, const MzhSearchParams& p, hipStream_t stream) {
  const size_t smem = mzh_wave_smem_bytes(p.S, NT);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mzh_wave_kernel<NT, REPLAY, SUP33>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  const int per_wg = MZW_WAVES * 16 * NT;
  const int grid = (p.B + per_wg - 1) / per_wg;
  hipLaunchKernelGGL((mzh_wave_kernel<NT, REPLAY, SUP33>), dim3(grid), dim3(MZW_WAVES * 64), smem, stream, net, p);
  return hipGetLastError();
}

template <int NT>
static hipError_t launch_wave_nt(const MzhSearchPlan& pl, const MzhWNet& net, const MzhSearchParams& p, hipStream_t stream) {
  if (pl.replay) return pl.sup33 ? launch_wave_t<NT, true, true>(net, p, stream) : launch_wave_t<NT, true, false>(net, p, stream);
  return pl.sup33 ? launch_wave_t<NT, false, true>(net, p, stream) : launch_wave_t<NT, false, false>(net, p, stream);
}

hipError_t mzh_launch_wave_search(const MzhSearchPlan& pl, const MzhWNet& net, const MzhSearchParams& p, hipStream_t stream) {
  return pl.nt == 1 ? launch_wave_nt<1>(pl, net, p, stream) : launch_wave_nt<2>(pl, net, p, stream);
}

// ------------------------------------------------------------------------------------------
// Expansion-memo fill (mzh_api_memo.hip memo_fill).  Level rows are ordered (state, node): row r of a level is
// move r % 6 from row r / 6 of the level above.
// ------------------------------------------------------------------------------------------
// the level's recurrent-inference input: parent latents (natural unit order) repeated per move, and the moves
__global__ __launch_bounds__(256) void mzh_memo_level_kernel(const float4* hprev, float4* xin, int32_t* act, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // one float4 of one row
  if (i >= n * 16) return;
  const long long r = i >> 4;
  xin[i] = hprev[(r / 6) * 16 + (i & 15)];
  if ((i & 15) == 0) act[r] = (int32_t)(r % 6);
}
// a level's outputs into the table: row = state * K + first_id + node, the latent in htree's order (position
// 16kb + 4g + t holds unit 16kb + 4t + g, what the wave kernel's B operand gathers), the record as replay's
__global__ __launch_bounds__(256) void mzh_memo_scatter_kernel(const float* h, const float* pi, const float* reward,
                                                               const float* value, long long n, long long per_state,
                                                               long long K, long long first_id, float* memo_h,
                                                               float* memo_rec) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // one latent position of one row
  if (i >= n * 64) return;
  const long long r = i >> 6;
  const int pos = (int)(i & 63);
  const long long row = (r / per_state) * K + first_id + (r % per_state);
  const int kb = pos >> 4, gg = (pos >> 2) & 3, t = pos & 3;
  memo_h[row * 64 + pos] = h[r * 64 + 16 * kb + 4 * t + gg];
  if (pos < 8) memo_rec[row * 8 + pos] = pos < 6 ? pi[r * 6 + pos] : pos == 6 ? reward[r] : value[r];
}
hipError_t mzh_launch_memo_level(const float* hprev, float* xin, int32_t* act, long long n, hipStream_t stream) {
  const long long blocks = (n * 16 + 255) / 256;
  hipLaunchKernelGGL(mzh_memo_level_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                     reinterpret_cast<const float4*>(hprev), reinterpret_cast<float4*>(xin), act, n);
  return hipGetLastError();
}
hipError_t mzh_launch_memo_scatter(const float* h, const float* pi, const float* reward, const float* value, long long n,
                                   long long per_state, long long K, long long first_id, float* memo_h, float* memo_rec,
                                   hipStream_t stream) {
  const long long blocks = (n * 64 + 255) / 256;
  hipLaunchKernelGGL(mzh_memo_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, h, pi, reward, value, n,
                     per_state, K, first_id, memo_h, memo_rec);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Harvest (after a wave search, same stream): one thread per root walks the root's miss log in simulation order
// and inserts each node whose parent has a row into the extension.  A node's parent was expanded in an earlier
// simulation, so its row may have been assigned a moment ago by this thread (the row words of the parent's block).
// The child link is claimed with one compare-and-swap; a loser whose node is already published adopts that row
// for its own chain, one whose node is still being claimed skips it (the content would be the same; the node is
// inserted by a later launch if it recurs).  A row is the latent the search stored in htree and the record it
// put in the tree: bit for bit what the kernel computed.  The next search sees all of it through the kernel
// boundary; within this kernel only row indices travel between threads.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mzh_memo_harvest_kernel(MzhHarvestParams h) {
  const int root = blockIdx.x * 256 + threadIdx.x;
  if (root >= h.B) return;
  int n = h.logn[root];
  if (n <= 0) return;
  n = min(n, h.logcap);
  MzwBlock* tb = reinterpret_cast<MzwBlock*>(h.tree) + (size_t)root * h.E;
  const uint4* log = h.log + (size_t)root * h.logcap;
  for (int i = 0; i < n; ++i) {
    const uint4 en = log[i];
    const int e = (int)en.x, pe = (int)(en.y >> 3), a = (int)(en.y & 7u);
    if (e < 1 || e >= h.E || pe < 1 || pe >= h.E || a >= MZH_A) continue;  // (never: the kernel's own entries)
    const int prow = (int)tb[pe].h[0].row1 - 1;  // (both halves hold the same word)
    if (prow < 0 || prow >= h.base + h.cap) continue;  // the parent has no row
    int32_t* lk = h.link + prow * 6 + a;
    const int old = atomicCAS(lk, MZH_LINK_NONE, MZH_LINK_CLAIM);
    if (old > 0) {  // published by another root of this state: chain through it
      tb[e].h[0].row1 = tb[e].h[1].row1 = (uint32_t)(old + 1);
      continue;
    }
    if (old != MZH_LINK_NONE) continue;  // being claimed
    const int r = atomicAdd(h.ctr, 1);
    if (r >= h.cap) {  // full: give the row and the claim back
      atomicSub(h.ctr, 1);
      atomicExch(lk, MZH_LINK_NONE);
      return;
    }
    const int row = h.base + r;
    const float4* src = reinterpret_cast<const float4*>(h.htree + ((size_t)root * h.E + e) * MZH_H);
    float4* dst = reinterpret_cast<float4*>(h.memo_h + (size_t)row * MZH_H);
#pragma unroll
    for (int k = 0; k < MZH_H / 4; ++k) dst[k] = src[k];
    const float *P = tb[e].h[0].P, *Q = tb[e].h[1].P;  // priors 0-2 | 3-5
    float4* rec = reinterpret_cast<float4*>(h.memo_rec + (size_t)row * 8);
    rec[0] = make_float4(P[0], P[1], P[2], Q[0]);
    rec[1] = make_float4(Q[1], Q[2], __uint_as_float(en.w), __uint_as_float(en.z));  // reward, value
    atomicExch(lk, row);
    tb[e].h[0].row1 = tb[e].h[1].row1 = (uint32_t)(row + 1);
  }
}
hipError_t mzh_launch_memo_harvest(const MzhHarvestParams& h, hipStream_t stream) {
  hipLaunchKernelGGL(mzh_memo_harvest_kernel, dim3((unsigned)((h.B + 255) / 256)), dim3(256), 0, stream, h);
  return hipGetLastError();
}

#ifdef MZH_STAMPS
// diagnostic build only: this translation unit's phase stamps [8 waves][MZH_NSTAMP], read and cleared
extern "C" int mzh_diag_wave_stamps(unsigned long long* host) {
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(mzh_stamp_acc), sizeof(mzh_stamp_acc)) != hipSuccess) return -2;
  static unsigned long long zero[8][MZH_NSTAMP] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(mzh_stamp_acc), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
#endif
