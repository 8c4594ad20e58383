// mzh_rows.h -- the frame of a kernel over R rows of a sub-batch (mzh_probe_kernel in mzh_search.hip,
// mzh_saliency.hip, mzh_pgrad.hip): one 256-thread workgroup owns R rows of the call; row r of its tile is env
// env[r] of the batch (MzhRowParams), -1 for a row beyond the tile or a skipped one -- such a row runs on a zero
// observation and stores nothing.  Here: the row table, the observation load, the root's output stores, the entry
// of the several-network form and the one launcher.  The search, wave and latency kernels do not use it.
#pragma once
#include "mzh_device.h"
#include "mzh_internal.h"

// The row table: thread r < R resolves row r of the tile into env[r].  `ok(env)` validates that env's further
// inputs; it runs only for an env inside [0, B), so nothing is read out of bounds, and a row skipped by either
// check counts once in err_count (the call's, nullable).  `stash()` then runs on every thread r < R and puts what
// ok read, or the kernel's defaults, into LDS beside env[r].  Ends with a barrier: all 256 threads call it.
template <int R, class TILE, class OK, class STASH>
__device__ __forceinline__ void mzh_rows_fill(int* env, const MzhRowParams& p, int32_t* err_count, const TILE& tile, OK ok,
                                              STASH stash) {
  const int tid = threadIdx.x;
  const int row0 = tile.template root0<R>();
  const int nvalid = tile.template nvalid<R>(p.n, row0);
  if (tid < R) {
    int e = -1;
    if (tid < nvalid) {
      e = p.env_index ? p.env_index[row0 + tid] : row0 + tid;
      if ((unsigned)e >= (unsigned)p.B) {
        if (err_count) atomicAdd(err_count, 1);
        e = -1;
      } else if (!ok(e)) {
        if (err_count) atomicAdd(err_count, 1);
        e = -1;
      }
    }
    env[tid] = e;
    stash();
  }
  __syncthreads();
}
// a kernel whose rows have no further inputs
template <int R, class TILE>
__device__ __forceinline__ void mzh_rows_fill(int* env, const MzhRowParams& p, int32_t* err_count, const TILE& tile) {
  mzh_rows_fill<R>(env, p, err_count, tile, [](int) { return true; }, []() {});
}

// the rows' observations into x ([R][MZH_LD64], k-block order), zero beyond in_dim and for a row without an env
template <int R>
__device__ __forceinline__ void mzh_rows_load_obs(float* x, const int* env, const MzhRowParams& p) {
  for (int i = threadIdx.x; i < R * p.kin; i += MZH_THREADS) {
    const int r = i / p.kin, k = i - r * p.kin;
    const int e = env[r];
    x[r * MZH_LD64 + mzh_kpos(k)] = (e >= 0 && k < p.in_dim) ? p.obs[(size_t)e * p.in_dim + k] : 0.0f;
  }
}

// a [R][MZH_LD64] latent in k-block order (position k of a row holds unit mzh_kpos(k), an involution) out to
// [B][64]
template <int R>
__device__ __forceinline__ void mzh_rows_store_latent(float* out, const float* s, const int* env) {
  for (int i = threadIdx.x; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    const int e = env[r];
    if (e >= 0) out[(size_t)e * MZH_H + mzh_kpos(k)] = s[r * MZH_LD64 + k];
  }
}

// the root's policy and value after mzh_mlp_initial (both nullable).  The probe has this block with `legal` on its
// spare thread, and the latent's store fused with its copy: the shared forms cost its 32-row kernel SGPR spills
// inside the six-action loop
template <int R>
__device__ __forceinline__ void mzh_rows_store_root(const MlpSmem<R>& sm, const int* env, float* pi0, float* value0) {
  const int tid = threadIdx.x;
  if (tid < R * 8) {
    const int r = tid >> 3, c = tid & 7;
    const int e = env[r];
    if (e >= 0) {
      if (pi0 && c < MZH_A) pi0[(size_t)e * MZH_A + c] = sm.pi[r * 8 + c];
      if (value0 && c == 6) value0[e] = sm.value[r];
    }
  }
}

// Rows of several networks (a set, mzh_load_weight_set): workgroup b takes tile b of the table
// mzh_multi_tiles_kernel made of this call's net_index.  One at or above the tile count has none and returns
// before its first barrier (a refused net_index leaves the count 0: nothing is written); the others take their
// tile, and `net` becomes the tile's network.
__device__ __forceinline__ bool mzh_rows_no_tile(const MzhMultiParams& mp) { return (int)blockIdx.x >= *mp.ntiles; }
__device__ __forceinline__ MzhTableTile mzh_rows_multi_tile(MzhNet& net, const MzhMultiParams& mp) {
  const MzhTableTile t{mp.tiles[blockIdx.x]};
  mzh_net_select(net, mp, t.t.net, net.support == 33);
  return t;
}
// a further per-network buffer of the set: network `net`'s at `stride` bytes
template <class T>
__device__ __forceinline__ const T* mzh_net_ptr(const T* base, int net, size_t stride) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)net * stride);
}

// The launcher: `single` on ceil(n / R) workgroups, or with mp the tile table of the n rows and then `multi` on
// mzh_multi_max_tiles(n, R, mp->M) workgroups (the arguments' net is then the set's network 0).  Callers name the
// 32-row pair before the 16-row one and `multi` before `single`: the order in which the kernels are instantiated
// is the order the compiler emits them in, and their code depends on it.
template <class... A>
static hipError_t mzh_rows_launch(void (*multi)(A..., MzhMultiParams), void (*single)(A...), int R, size_t smem, int n,
                                  const MzhMultiParams* mp, hipStream_t stream, const A&... a) {
  hipError_t e = hipFuncSetAttribute(mp ? reinterpret_cast<const void*>(multi) : reinterpret_cast<const void*>(single),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  if (!mp) {
    hipLaunchKernelGGL(single, dim3((n + R - 1) / R), dim3(MZH_THREADS), smem, stream, a...);
    return hipGetLastError();
  }
  e = mzh_launch_multi_tiles(*mp, n, R, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(multi, dim3(mzh_multi_max_tiles(n, R, mp->M)), dim3(MZH_THREADS), smem, stream, a..., *mp);
  return hipGetLastError();
}
