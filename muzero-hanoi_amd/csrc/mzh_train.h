// mzh_train.h -- parameter blocks of the fused training update (mzh_train.hip), filled by the C
// ABI (mzh_api_train.hip: mzh_train_update, with the layer shapes of mzh_pack.h's table).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mzh.h"

// kernel-1 view of the network (names follow networks.py:39-67): every weight both as torch stores
// it ([out][in]) and transposed ([in][out], suffix T), so that each GEMV direction reads coalesced
struct MztNet {
  const float *rep1, *rep1T, *rep1b, *rep2, *rep2T, *rep2b;
  const float *dyn1, *dyn1T, *dyn1b, *dyn2, *dyn2T, *dyn2b;
  const float *rwd1, *rwd1T, *rwd1b, *rwd2, *rwd2T, *rwd2b;
  const float *pol1, *pol1T, *pol1b, *pol2, *pol2T, *pol2b;
  const float *val1, *val1T, *val1b, *val2, *val2T, *val2b;
};

// per-layer inputs X and output gradients GY, rows m = b * U + t (step layers) or b (representation)
struct MztScratch {
  float *x0;    // [B][32]     observation, zero-padded
  float *repa;  // [B][256]    representation hidden activation
  float *h;     // [BU][64]    h_t (normalised), input of policy / value / dynamics layer 1
  float *ap, *av, *ad, *ar;  // [BU][256] hidden activations
  float *hp;    // [BU][64]    h'_{t+1} (before normalisation), input of reward layer 1
  float *g_rep; // [B][256]    representation hidden pre-activation gradient
  float *g_h0p; // [B][64]     representation output gradient
  float *g_p, *g_v, *g_d, *g_r;  // [BU][256] hidden pre-activation gradients
  float *g_lp;  // [BU][16]    policy logit gradient (zero-padded)
  float *g_lv, *g_lr;  // [BU][48 | 16] value / reward logit gradients (zero-padded)
  float *g_hp;  // [BU][64]    dynamics output gradient
};

struct MztRowParams {
  int B, U, in_dim;
  const float *obs, *rwds, *pi, *returns, *w;
  const int64_t* actions;
  float* row_loss;  // [B][3]
  float* new_prio;  // [B] or null
  MztNet n;
  MztScratch s;
};

struct MztGradLayer {
  const float* X;
  int ldx;
  const float* GY;
  int ldg;
  int M, out, in;
  int onehot_from;  // columns >= onehot_from are the one-hot action (dynamics layer 1), else -1
  int tile0, nkb;   // first tile of this layer in the grid, 16-column blocks of `in`
  float *W, *b, *mW, *vW, *mb, *vb;
  float* WT;        // transposed copy [in][ldwt] to refresh
  int ldwt;         // out rounded up to a multiple of 4 (16-byte rows)
};

struct MztGradParams {
  MztGradLayer L[10];
  const int64_t* actions;
  float step_size, bc2_sqrt, beta1, beta2, eps;
};

// ---- the set forms (mzh_train_set_update): the grid's y index (x for the one-workgroup kernels) is the network,
// whose arguments are row m of a table in device memory, written once when the set is created and never by a
// kernel; what changes from call to call is the per-call record step[m] (mzh_train_set_step of mzh.h: active, n,
// step_size, bc2_sqrt), read by the kernels when they run.  A workgroup of an inactive network returns before its
// first barrier and touches nothing of that network.
struct MzrPrioArgs {  // replay_set_priorities_kernel's arguments of one network
  float* prio;
  long long size;
  const int64_t* idx;
  const float* val;
  int m;
};

struct MztSetParams {
  const mzh_replay_args* draw;  // [M]  n, u and status unused: they come from step, u + m * batch, status + 4 m
  const MztRowParams* rows;     // [M]
  const MztGradParams* grad;    // [M]  step_size and bc2_sqrt unused: they come from step
  const MzrPrioArgs* prio;      // [M]
  const mzh_train_set_step* step;  // [M]
  const double* u;              // [M][batch]
  int32_t* status;              // [M][4]: draw status, exact-scan flag, set-priorities status, zero
};

size_t mzt_rows_smem_bytes(int rows, int U);
hipError_t mzt_rows_set_prepare(int rows, int support, int U);  // the set form's dynamic LDS limit, once per set
hipError_t mzt_launch_rows_set(int rows, int support, int B, int U, int M, const MztSetParams& v, hipStream_t stream);
hipError_t mzt_launch_grad_adam_set(int n_tiles, int M, const MztSetParams& v, hipStream_t stream);
hipError_t mzr_launch_sample_set(int M, const MztSetParams& v, hipStream_t stream);
hipError_t mzr_launch_set_priorities_set(int M, const MztSetParams& v, hipStream_t stream);
hipError_t mzt_launch_rows(int rows, int support, const MztRowParams& p, hipStream_t stream);
hipError_t mzt_launch_grad_adam(const MztGradParams& P, int n_tiles, hipStream_t stream);
hipError_t mzt_launch_transpose(const float* W, float* WT, int out, int in, int ldwt, hipStream_t stream);

// prioritised replay on the device (mzh_replay.hip): the draw + gather and the priority write-back
#define MZR_MAX_BATCH 4096  // batch_s per draw (the sampled indices sit in LDS)
hipError_t mzr_launch_sample(const mzh_replay_args& a, hipStream_t stream);
hipError_t mzr_launch_set_priorities(float* prio, long long size, const int64_t* idx, const float* val, int m,
                                     int32_t* status, hipStream_t stream);

// episode ingest (mzh_ingest.hip): the filter + scan launch and the ring writer launch
hipError_t mzi_launch_ingest(const mzh_ingest_args& a, hipStream_t stream);
