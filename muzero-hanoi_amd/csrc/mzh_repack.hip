// mzh_repack.hip -- repack an engine's weights on the device from the live parameter tensors
// (mzh_load_weights_device / mzh_load_weight_set_device).  The host packers (mzh_pack.cpp) only copy, so a
// blob is a fixed permutation of the canonical weights with zero fill; mzh_pack_maps records it and this
// kernel applies it: one memory-bound gather, no arithmetic, the same bytes the host packer produces.
#include "mzh_internal.h"

// A thread owns one float4 of the main or of the transposed blob of network blockIdx.y: its four map
// entries are one 16-byte load, the four sources are gathered from the 20 parameter tensors (state_dict
// order, each contiguous fp32 in torch layout), the result is one 16-byte store.  A map entry is
// (tensor << 24) | offset, or -1 for a float the layout leaves zero.  The network's 20 pointers are staged
// in LDS once per workgroup.  Values move as 32-bit patterns: NaN payloads and -0.0 arrive unchanged.
__device__ __forceinline__ uint32_t mzh_repack_fetch(const uint32_t* const* sp, int32_t e) {
  return e < 0 ? 0u : sp[e >> 24][e & 0xffffff];
}

__global__ __launch_bounds__(MZH_REPACK_THREADS) void mzh_repack_kernel(MzhRepackParams p) {
  __shared__ const uint32_t* sp[20];
  const int net = blockIdx.y;
  if (threadIdx.x < 20) sp[threadIdx.x] = reinterpret_cast<const uint32_t*>(p.ptab[(size_t)net * 20 + threadIdx.x]);
  __syncthreads();
  const int i = blockIdx.x * MZH_REPACK_THREADS + threadIdx.x;
  if (i == 0) {  // the two values the search kernels take by value (bias bin 32 of the reward / value head)
    uint32_t* s = reinterpret_cast<uint32_t*>(p.scal) + 2 * (size_t)net;
    s[0] = mzh_repack_fetch(sp, p.scal_src[0]);
    s[1] = mzh_repack_fetch(sp, p.scal_src[1]);
  }
  if (i >= p.n4m + p.n4t) return;
  const bool tr = i >= p.n4m;
  const int j = tr ? i - p.n4m : i;
  const int4 e = (tr ? p.map_t : p.map_m)[j];
  uint4 v;
  v.x = mzh_repack_fetch(sp, e.x);
  v.y = mzh_repack_fetch(sp, e.y);
  v.z = mzh_repack_fetch(sp, e.z);
  v.w = mzh_repack_fetch(sp, e.w);
  float* dst = tr ? p.dst_t + (size_t)net * p.stride_t : p.dst_m + (size_t)net * p.stride_m;
  reinterpret_cast<uint4*>(dst)[j] = v;
}

hipError_t mzh_launch_repack(const MzhRepackParams& p, int M, hipStream_t stream) {
  const int n4 = p.n4m + p.n4t;
  const dim3 grid((n4 + MZH_REPACK_THREADS - 1) / MZH_REPACK_THREADS, M);
  hipLaunchKernelGGL(mzh_repack_kernel, grid, dim3(MZH_REPACK_THREADS), 0, stream, p);
  return hipGetLastError();
}
