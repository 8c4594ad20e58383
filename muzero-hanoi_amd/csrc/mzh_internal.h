// mzh_internal.h -- parameter blocks shared by the launchers (mzh_search.hip) and the C ABI
// implementation (the host units mzh_api*.hip, through mzh_host.h), and the device-pointer form of the wave and
// latency weight layouts that mzh_pack.cpp fills (its offsets, and the MZH_ONE_* constants, come from mzh_pack.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mzh_device.h"
#include "mzh_pack.h"

struct MzhSearchParams {
  int B, S, E;          // roots, simulations, tree blocks per root (engine max_sims + 1)
  int in_dim, kin;      // observation width 3N and its zero-padded width (16 * rep0.kb)
  int deterministic, np1;
  double discount, eps, temperature;
  const float* obs;
  const double* noise;
  const int32_t* tie_idx;
  const double* action_u;
  const double* minmax_in;
  const float* rp_root_pi;
  const float* rp_sim;  // [S][B][8] replay records (6 priors, reward, value)
  unsigned char* tree;  // [B][E] MzhBlock
  float* htree;         // [B][E][64]
  uint16_t* pathx;      // [B][E] selection-path slots beyond the LDS-cached depths (wave kernel)
  const double* table;  // [S+2] UCB table (log((n+19653)/19652)+1.25)*sqrt(n)
  int32_t* visits;
  double* root_q;
  double* minmax_out;
  int32_t* extra_ties;
  int32_t* action;
  double* pi;
  int32_t* latent;
  int32_t* latent_len;
  int32_t* sel_steps;
  const double* pow_table;  // [S + 1] np.power(n, 1/T) for a non-integer exponent (nullable)
  int32_t* lockstep_levels;  // [groups] sum over simulations of each lockstep group's deepest selection (nullable)
  // the expansion memo (wave kernel, MLP searches; all null / 0 without one): rows state * memo_K + node id
  const float* memo_h;    // [rows][64] normalised latents in htree's order
  const float* memo_rec;  // [rows][8] 6 priors, reward, value
  unsigned long long* memo_cnt;  // [3] (wave, simulation) pairs without MLP / packed / full
  int memo_D, memo_K;     // depth, nodes per state 1 + 6 + ... + 6^D
  // the memo's grown extension (all null / 0 with growth off): rows after the dense ones,
  // reached through a trie of child links, filled between launches from the per-root miss log
  const int32_t* memo_link;  // [dense rows + memo_cap][6] the child's row, MZH_LINK_NONE or MZH_LINK_CLAIM
  uint4* memo_log;           // [B][memo_logcap] {new slot, parent slot e * 8 + a, value bits, reward bits}
  int32_t* memo_logn;        // [B] entries of the root's log
  int32_t* memo_ctr;         // [2] extension rows in use, and in use before the last harvest
  int memo_cap, memo_logcap; // extension rows, log entries per root
};
#define MZH_LINK_NONE 0      // (a child's row is always > 0: extension rows follow the dense ones)
#define MZH_LINK_CLAIM (-1)

// the harvest after a wave search (mzh_memo_harvest_kernel, mzh_wave.hip): one thread per root inserts the
// root's logged misses into the extension
struct MzhHarvestParams {
  int B, E;
  unsigned char* tree;   // [B][E] MzwBlock
  const float* htree;    // [B][E][64]
  const uint4* log;
  const int32_t* logn;
  int logcap;
  int32_t* link;
  int32_t* ctr;
  int base, cap;         // dense rows, extension rows
  float* memo_h;
  float* memo_rec;
};
hipError_t mzh_launch_memo_harvest(const MzhHarvestParams& h, hipStream_t stream);

// Expansion-memo arithmetic (host): nodes per state, rows and bytes at depth D, the automatic depth
static inline long long mzh_memo_nodes(int D) {  // K(D) = (6^(D+1) - 1) / 5
  long long k = 0, p = 1;
  for (int d = 0; d <= D; ++d, p *= 6) k += p;
  return k;
}
static inline long long mzh_memo_states(int n_disks) {
  long long s = 1;
  for (int i = 0; i < n_disks; ++i) s *= 3;
  return s;
}
#define MZH_MEMO_ROW_BYTES 288          // 64 fp32 latent + the 32-byte record
#define MZH_MEMO_MAX_ROWS (1ll << 26)   // a forced depth's limit (row indices stay far inside int32)
#define MZH_MEMO_MAX_DEPTH 12
// the byte budget of the automatic depth (N = 4 gets D = 5, N = 7 gets D = 3)
#define MZH_MEMO_BUDGET_BYTES (256ll << 20)
// the byte budget of the grown extension's rows (the default of mzh_set_memo_grow) and the per-root miss log's
// default entries: a cold four-disc root misses about 15 times in 50 simulations
#define MZH_MEMO_GROW_BUDGET_BYTES (64ll << 20)
#define MZH_MEMO_LOG_CAP 16
#define MZH_MEMO_LOG_CAP_MAX 1024
static inline long long mzh_memo_grow_rows(long long budget_bytes, long long dense_rows) {
  long long cap = budget_bytes / MZH_MEMO_ROW_BYTES;
  if (cap > MZH_MEMO_MAX_ROWS) cap = MZH_MEMO_MAX_ROWS;  // (dense + cap) * 6 link indices stay inside int32
  return dense_rows > 0 ? cap : 0;
}
static inline int mzh_memo_auto_depth(int n_disks) {
  const long long st = mzh_memo_states(n_disks);
  int D = 0;
  while (D < MZH_MEMO_MAX_DEPTH && st * mzh_memo_nodes(D + 1) * MZH_MEMO_ROW_BYTES <= MZH_MEMO_BUDGET_BYTES) ++D;
  return D;
}
hipError_t mzh_launch_memo_level(const float* hprev, float* xin, int32_t* act, long long n, hipStream_t stream);
hipError_t mzh_launch_memo_scatter(const float* h, const float* pi, const float* reward, const float* value, long long n,
                                   long long per_state, long long K, long long first_id, float* memo_h, float* memo_rec,
                                   hipStream_t stream);

// The device repack (mzh_repack.hip): gather the main and the transposed blob of M networks from their
// parameter tensors through the pack maps (MzhPackMaps, mzh_pack.h)
#define MZH_REPACK_THREADS 256
struct MzhRepackParams {
  const int4* map_m;         // [n4m] encoded map of the main blob (mzh_pack_map_encode), -1 padded to a float4
  const int4* map_t;         // [n4t] the transposed blob's
  int n4m, n4t;              // float4s written per network
  const float* const* ptab;  // device [M][20] parameter tensors in state_dict order
  float* dst_m;              // network m's main blob at dst_m + m * stride_m (floats, multiples of 4)
  float* dst_t;
  size_t stride_m, stride_t;
  float* scal;               // [M][2] {rwd_net.2.bias[32], value_net.2.bias[32]}, 0 without a 33-bin head
  int32_t scal_src[2];       // their encoded sources (-1: none)
};
hipError_t mzh_launch_repack(const MzhRepackParams& p, int M, hipStream_t stream);

// visits ** e as generate_play_policy computes it (np.power(int64 visits, e), mcts.py:168-174), for
// x = n visits and e = max(1, min(5, 1/T)): an integer exponent is an exact product (n^5 < 2^53);
// a non-integer one is taken from pow_table[n], the caller's np.power(arange(S + 1), e) (NumPy's
// vectorised pow -- SVML on AVX-512 hosts -- differs from any other pow in the last bit for some
// n), or from the device pow when no table is given
__device__ __forceinline__ double mzh_pow(double x, int n, double e, const double* pow_table) {
  if (e == __builtin_rint(e)) {
    double r = x;
    for (int i = 1; i < (int)e; ++i) r = r * x;
    return r;
  }
  return pow_table ? pow_table[n] : pow(x, e);
}

struct MzhInferParams {
  int B, in_dim, kin;
  const float* x;         // obs [B][in_dim] (initial) or h [B][64] (recurrent)
  const int32_t* action;  // [B] (recurrent)
  float* h;
  float* reward;
  float* pi;
  float* value;
  float* policy_logits;
  float* value_logits;
  float* reward_logits;
};

template <int R>
__device__ __forceinline__ void mzh_store_outputs(MlpSmem<R>& sm, const MzhInferParams& p, int row0, int nvalid,
                                                  int support, bool recurrent) {
  const int tid = threadIdx.x;
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    if (r < nvalid) p.h[(size_t)(row0 + r) * MZH_H + k] = sm.x[r * MZH_LD64 + mzh_kpos(k)];
  }
  for (int i = tid; i < R * 8; i += MZH_THREADS) {
    const int r = i >> 3, c = i & 7;
    if (r < nvalid && c < MZH_A) {
      if (p.pi) p.pi[(size_t)(row0 + r) * MZH_A + c] = sm.pi[r * 8 + c];
      if (p.policy_logits) p.policy_logits[(size_t)(row0 + r) * MZH_A + c] = sm.lpol[r * MZH_LDPOL + c];
    }
  }
  for (int i = tid; i < R * support; i += MZH_THREADS) {
    const int r = i / support, k = i - r * support;
    if (r < nvalid) {
      if (p.value_logits) p.value_logits[(size_t)(row0 + r) * support + k] = sm.lval[r * MZH_LDSUP + k];
      if (recurrent && p.reward_logits) p.reward_logits[(size_t)(row0 + r) * support + k] = sm.lrwd[r * MZH_LDSUP + k];
    }
  }
  if (tid < nvalid) {
    if (p.value) p.value[row0 + tid] = sm.value[tid];
    if (p.reward) p.reward[row0 + tid] = sm.reward[tid];
  }
}

// ------------------------------------------------------------------------------------------
// Wave-kernel network layout (mzh_wave.hip).  Each MLP (layer1 -> ReLU -> layer2) is one stream
// of MFMA A-fragments with the WEIGHTS as the A operand and the activations (one root per
// column) as the B operand, so a hidden tile's C registers feed the next layer's B operand
// directly (no LDS round trip).  Per hidden tile ht (16 units) the stream holds KB1 layer-1
// fragments then NO layer-2 fragments, each [64 lanes] float4:
//   layer1 frag (ht, kb)[lane][t] = W1[u(ht, lane&15)][16kb + 4t + (lane>>4)]
//   layer2 frag (ht, ot)[lane][t] = W2[pi(ot, lane&15)][16ht + 4t + (lane>>4)]
// with u(ht, r) = 16ht + 4(r&3) + (r>>2): C row 4g+i of hidden tile ht is unit 16ht + 4i + g, which
// is exactly the unit lane group g must supply at k-step i of layer 2 -- every dot product stays
// a k-ordered fp32 FMA chain from 0 (the numerics contract of mzh_device.h).  One zero ht block
// pads the stream end (unconditional prefetch).  b1/b2 are the biases in C-register order.
// ------------------------------------------------------------------------------------------
struct MzhWMlp {
  const float4* s;  // [17][KB1 + NO][64]
  const float* b1;  // [256]: b1[16ht + 4g + i] = bias1[16ht + 4i + g]
  const float* b2;  // [16 NO]: b2[16ot + 4g + i] = bias2[pi(ot, 4g + i)] (0 on padding rows)
  // 33-bin heads: bins 0..31 in the NO = 2 tiles, bin 32 as four vector-FMA chains (lane group g: hidden
  // units 16ht + 4t + g, t = 0..3): w32[4ht + g] = those units' weights, b32 its bias (MzhNet::rwd32)
  const float4* w32;
  float b32;
  int kb1, no;
  int soff, b1off, b2off, w32off;  // byte offsets of s, b1, b2, w32 in the packed blob (MzhWNet::wbase)
};
struct MzhWNet {
  MzhWMlp rep, dyn, rwd, pol, val;
  const float* wbase;  // the packed weight blob: one buffer resource serves every chain's loads
  const float* oh;  // [6][256]: oh[a][16ht + 4g + i] = dynamic_net.0.weight[u(ht, 4g + i)][64 + a]
  int support, in_dim;
};

// ------------------------------------------------------------------------------------------
// Latency-path network layout (mzh_one.hip: one root per workgroup, weights stationary on the CU).
// The hidden layers' rows live in registers for the whole launch: thread t < 256 holds unit t of
// dynamic_net.0 (64 latent + 6 one-hot columns) and rwd_net.0, thread 256 + t unit t of policy_net.0 and
// value_net.0.  The K = 256 output layers live in LDS, copied verbatim from `l2` (k-major: one
// ds_read_b128 gives a lane the 4 k-steps of its output row, 1 KiB contiguous per wave).
//   l1 [66 k4][256 units] float4: k4 0-15 dynamic_net.0 latent columns, 16-31 rwd_net.0, 32-47 policy_net.0,
//      48-63 value_net.0, 64-65 dynamic_net.0 one-hot columns 64..69 (+ 2 zero)
//   b1 [256] float4 {dynamic_net.0, rwd_net.0, policy_net.0, value_net.0} bias of the unit
//   rep0 [in_dim][256] representation_net.0 (k-major), rep2 [64 k4][64] float4 representation_net.2
//   l2: the LDS image, MZH_ONE_* offsets in float4 units (mzh_pack.h)
// ------------------------------------------------------------------------------------------
struct MzhOneNet {
  const float4* l1;
  const float4* b1;
  const float* rep0;
  const float* rep0b;
  const float4* rep2;
  const float* rep2b;
  const float4* l2;
};

// Every template argument of one search launch, decided once on the host (mzh_api_search.hip make_plan) and
// used both to launch and to report the launched instantiation (mzh_search_plan_query)
struct MzhSearchPlan {
  int wave;    // 1: mzh_wave_kernel<nt, replay, sup33>; 0: mzh_search_kernel<R, replay, ohl, sup33, mmin>
  int nt;      // wave kernel: 16-root column tiles per wave
  int R;       // cooperative kernel: roots per workgroup
  int replay;  // tree-only instantiation (recorded network outputs)
  int ohl;     // cooperative: the dynamics one-hot columns in LDS; one: the latents in LDS
  int sup33;   // 33-bin value / reward support (cooperative replay: always 1, one instantiation)
  int mmin;    // cooperative / one: caller-given MinMaxStats bounds (subnormal max - min check)
  int occ2;    // cooperative: mzh_search_occ2_kernel<sup33, mmin> (16-root tile, two workgroups per CU)
  int one;     // latency path: mzh_search_one_kernel<sup33, mmin, ohl> (one root per workgroup)
  int grid;    // one: workgroups (each loops over roots b, b + grid, ...)
};

// Search over a set of networks (mzh_search_multi; the kernels are in mzh_search.hip).  A set is M packed
// blobs of one layout (mzh_pack_network_set) at `stride` bytes in one allocation; a tile is up to R
// consecutive roots of one network, the unit one workgroup of mzh_search_multi_kernel searches.
#define MZH_MULTI_MAX_NETS 256
struct MzhTile {
  int32_t root0, n, net, sims;  // sims: the tile's simulation budget (read by mzh_search_multi_kernel only)
};
struct MzhMultiParams {
  const int32_t* net_index;  // [B] caller's, read only by mzh_multi_tiles_kernel
  int M;                     // networks this call may index
  MzhTile* tiles;            // [mzh_multi_max_tiles(max_roots, 16, MZH_MULTI_MAX_NETS)] engine workspace
  int32_t* ntiles;           // [1] engine workspace: tiles of this call (0: net_index refused)
  int32_t* status;           // [2] caller's (nullable)
  size_t stride;             // bytes between two networks' blobs
  const float* scal;         // [M][2] {rwd32b, val32b} of each network (MzhNet carries them by value)
};
// upper bound of the tiles B roots of M networks make at R roots per tile: every network with roots has at
// most one ragged tile, sum ceil(c_m / R) <= floor((B - K) / R) + K <= ceil(B / R) + K - 1 for K >= 1 of them
static inline int mzh_multi_max_tiles(int B, int R, int M) { return (B + R - 1) / R + (M < B ? M : B) - 1; }
hipError_t mzh_launch_search_multi(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p,
                                   const MzhMultiParams& mp, hipStream_t stream);
// The simulation budgets of a multi-network search (mzh_search_multi_budget): root b runs n_sims[b] simulations.  A
// run is a maximal stretch of consecutive roots with equal (net_index, n_sims); a tile never spans a run.  With
// n_sims == nullptr every root has the launch's budget S and the tiles are those of the networks' segments.
struct MzhBudgetParams {
  const int32_t* n_sims;  // [B] caller's (nullable), read only by mzh_multi_tiles_kernel
  int S;                  // the launch's n_sims: every budget lies in [0, S]
  int max_runs;           // the caller's bound on the runs (the search grid is sized by it)
  int cap;                // entries of MzhMultiParams::tiles
  // [B] caller's (nullable; only with n_sims == nullptr): budgets the prologue only checks, each in [0, S], and refuses
  // as it refuses a bad net_index -- the tiles stay the networks' segments (mzh_play_episodes_sweep, whose kernel
  // reads the budgets itself)
  const int32_t* check_sims;
};
hipError_t mzh_launch_search_multi_budget(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p,
                                          const MzhMultiParams& mp, const MzhBudgetParams& bp, hipStream_t stream);
// mzh_multi_tiles_kernel (mzh_search.hip) on mp.net_index [n]: the prologue of every multi-network launch (sims: the
// budget written into every tile, the launch's n_sims for a search, 0 for the row kernels, which never read it)
// check_sims: MzhBudgetParams::check_sims, with sims their upper bound
hipError_t mzh_launch_multi_tiles(const MzhMultiParams& mp, int n, int R, hipStream_t stream, int sims = 0,
                                  const int32_t* check_sims = nullptr);

// Where a cooperative workgroup's rows [root0, root0 + nvalid), nvalid <= R, come from: MzhGridTile (workgroup
// b owns the R rows from b * R: the single-network kernels) or a tile table entry (the multi-network kernels).
// kOwnSims: the workgroup's roots run sims() simulations, the table entry's budget, not the launch's n_sims.
struct MzhGridTile {
  template <int R>
  __device__ __forceinline__ int root0() const { return blockIdx.x * R; }
  template <int R>
  __device__ __forceinline__ int nvalid(int B, int root0) const { return min(R, B - root0); }
  static constexpr bool kOwnSims = false;
};
struct MzhTableTile {
  MzhTile t;
  template <int R>
  __device__ __forceinline__ int root0() const { return t.root0; }
  template <int R>
  __device__ __forceinline__ int nvalid(int, int) const { return t.n; }
  static constexpr bool kOwnSims = true;
  __device__ __forceinline__ int sims() const { return t.sims; }
};

// the set's network `net` from the template MzhNet of network 0: every blob of a set has the same layout, at
// a constant byte stride, so each pointer moves by net * stride (the layers' woff / boff are relative to wbase
// and stay); the two bin-32 biases MzhNet carries by value come from the set's [M][2] array
__device__ __forceinline__ void mzh_net_select(MzhNet& n, const MzhMultiParams& mp, int net, bool sup33) {
  const size_t off = (size_t)net * mp.stride;
  auto mv = [off](auto*& q) { q = reinterpret_cast<std::remove_reference_t<decltype(q)>>(reinterpret_cast<const char*>(q) + off); };
  auto layer = [&](MzhLayer& l) {
    mv(l.w);
    mv(l.b);
  };
  layer(n.rep0); layer(n.rep2); layer(n.dyn0); layer(n.dyn2); layer(n.rwd0); layer(n.rwd2);
  layer(n.pol0); layer(n.pol2); layer(n.val0); layer(n.val2);
  mv(n.wbase);
  mv(n.dyn0_onehot);
  if (sup33) {  // null without a 33-bin head
    mv(n.rwd32);
    mv(n.val32);
    n.rwd32b = mp.scal[2 * net];
    n.val32b = mp.scal[2 * net + 1];
  }
}

// What the kernels over R rows of a sub-batch share (mzh_rows.h: the probe, saliency and gradient kernels): row j
// of the call is env env_index[j] (or j) of a batch of B; every array but env_index (and a set's net_index) is
// indexed by env
// (the eighth common field, err_count, is the last member of each block below, where it has always been: moved up
// here it changes the kernels' kernarg loads and with them their register allocation and measured time)
struct MzhRowParams {
  int B, n;                  // envs of the batch, rows of the call
  int in_dim, kin;           // observation width 3N and its zero-padded width (16 * rep0.kb)
  int n_disks;
  const int32_t* env_index;  // [n] nullable
  const float* obs;          // [B][in_dim]
};

// mzh_saliency (mzh_saliency_kernel / mzh_saliency_multi_kernel, mzh_saliency.hip): rows as in MzhRowParams
struct MzhSalNetT {  // the transposed blob (MzhPackedT) of one network; a set's at `stride` bytes
  const float4* base;
  int off[MZH_T_LAYERS];  // float4 offsets of the layers' fragments
  int kb_val2;            // k-blocks of the value head's outputs: 3 (33 bins) or 1
  int nt_rep0;            // 16-column tiles of the observation
  size_t stride;
};
struct MzhSalParams : MzhRowParams {
  const int32_t* logit_index;  // [B] nullable
  float* sal_policy;           // [B][in_dim]
  float* sal_value;            // [B][in_dim]
  int32_t* picked;             // [B] nullable
  float* disc_policy;          // [B][n_disks] nullable
  float* disc_value;           // [B][n_disks] nullable
  float* h0;                   // [B][64] nullable
  float* pi0;                  // [B][6] nullable
  float* value0;               // [B] nullable
  int32_t* err_count;          // nullable: += 1 per skipped row
};
size_t mzh_saliency_smem_bytes(int R);
hipError_t mzh_launch_saliency(int R, const MzhNet& net, const MzhSalNetT& nt, const MzhSalParams& p,
                               const MzhMultiParams* mp, hipStream_t stream);

// mzh_param_grads (mzh_pgrad_kernel / mzh_pgrad_multi_kernel / mzh_pgrad_expand_kernel, mzh_pgrad.hip): rows
// as in MzhRowParams
struct MzhPgNetT {  // dynamic_net.2 and rwd_net.2 transposed (MzhPackedG) of one network; a set's at `stride` bytes
  const float4* base;
  int off[MZH_G_LAYERS];  // float4 offsets of the layers' fragments
  int kb_rwd2;            // k-blocks of the reward head's outputs: 3 (33 bins) or 1
  size_t stride;
};
struct MzhPgradParams : MzhRowParams {
  const int32_t* action;        // [B]
  const int32_t* policy_logit;  // [B] nullable
  float* delta1;                // [B][5][256]
  float* delta2;                // [B][5][64]
  float* act;                   // [B][5][256]
  float* h0;                    // [B][64]
  float* z1;                    // [B][64]
  float* h1;                    // [B][64] nullable
  float* pi0;                   // [B][6] nullable
  float* value0;                // [B] nullable
  float* reward;                // [B] nullable
  float* objective;             // [B][5] nullable
  float* grad;                  // [n][n_floats] nullable
  int32_t* err_count;           // nullable: += 1 per skipped row
};
size_t mzh_pgrad_smem_bytes(int R);
// the gather that fills a network's (M networks') MzhPackedG buffer from the main blob(s): dst[m][j] =
// src[m][map[j]], +0 where map[j] < 0; strides in floats
hipError_t mzh_launch_pgrad_gather(const int32_t* map, int n, const float* src, size_t src_stride, float* dst,
                                   size_t dst_stride, int M, hipStream_t stream);
// the factor kernel (mp as in mzh_launch_probe), then with p.grad the expansion of the call's rows
hipError_t mzh_launch_pgrad(int R, const MzhNet& net, const MzhSalNetT& nt, const MzhPgNetT& gt, const MzhPgradParams& p,
                            int support, const MzhMultiParams* mp, hipStream_t stream);

// mzh_probe_actions (mzh_probe_kernel / mzh_probe_multi_kernel, mzh_search.hip): rows as in MzhRowParams
struct MzhProbeParams : MzhRowParams {
  const uint8_t* state;  // [B][n_disks] nullable
  float* reward;         // [B][6]
  float* value;          // [B][6]
  uint8_t* legal;        // [B] nullable
  float* h0;             // [B][64] nullable
  float* pi0;            // [B][6] nullable
  float* value0;         // [B] nullable
  float* h1;             // [B][6][64] nullable
  float* pi1;            // [B][6][6] nullable
  int32_t* err_count;    // nullable: += 1 per skipped row
};
size_t mzh_probe_smem_bytes(int R);
// mp == nullptr: mzh_probe_kernel<R> on ceil(n / R) workgroups; else the tile table of the n rows, then
// mzh_probe_multi_kernel<R> on mzh_multi_max_tiles(n, R, mp->M) workgroups (net: the set's network 0)
hipError_t mzh_launch_probe(int R, const MzhNet& net, const MzhProbeParams& p, const MzhMultiParams* mp, hipStream_t stream);

// the env side of mzh_play_episodes (the episode form of mzh_search_one_kernel, mzh_one.hip); the search side is a MzhSearchParams
// whose per-search arrays have T * B rows (row t * B + b: move t of env b) and whose minmax_in is per env
struct MzhEpisodeParams {
  int T, n_disks, goal_peg, max_steps;
  const uint8_t* start;  // [B][n_disks]
  float* obs;            // [T][B][3 n_disks] nullable
  int8_t* reward;        // [T][B]
  int32_t* steps;        // [B]
  int32_t* illegal;      // [B]
  uint8_t* solved;       // [B]
  uint8_t* final_state;  // [B][n_disks]
  double* minmax_out;    // [B][2]
  int32_t* err_count;    // nullable
};
hipError_t mzh_launch_episodes(const MzhSearchPlan& pl, const MzhNet& net, const MzhOneNet& on, const MzhSearchParams& p,
                               const MzhEpisodeParams& ep, hipStream_t stream);
// the set side of mzh_play_episodes_multi (a fifth kernel argument of the episode form): env b plays under network
// net_index[b] of the loaded set, whose blobs -- each in the latency kernel's layout too -- lie `stride` bytes apart
struct MzhEpisodeSet {
  const int32_t* net_index;  // [B] caller's, checked by mzh_multi_tiles_kernel before the episode launch
  const int32_t* ntiles;     // [1] that check's verdict (MzhMultiParams::ntiles): 0 = refused, no env plays
  size_t stride;             // bytes between two networks' blobs
};
hipError_t mzh_launch_episodes_set(const MzhSearchPlan& pl, const MzhNet& net, const MzhOneNet& on, const MzhSearchParams& p,
                                   const MzhEpisodeParams& ep, const MzhEpisodeSet& es, hipStream_t stream);
// the sweep side of mzh_play_episodes_sweep (a sixth kernel argument of the episode form): env b runs n_sims[b]
// simulations per move, at most the launch's p.S, which sizes everything, under discount[b]
struct MzhEpisodeSweep {
  const int32_t* n_sims;   // [B] caller's, checked by mzh_multi_tiles_kernel before the episode launch
  const double* discount;  // [B] caller's, nullable: p.discount for every env
};
hipError_t mzh_launch_episodes_sweep(const MzhSearchPlan& pl, const MzhNet& net, const MzhOneNet& on,
                                     const MzhSearchParams& p, const MzhEpisodeParams& ep, const MzhEpisodeSet& es,
                                     const MzhEpisodeSweep& sw, hipStream_t stream);
size_t mzh_one_smem_bytes(int S, bool latl);
hipError_t mzh_launch_one(const MzhSearchPlan& pl, const MzhNet& net, const MzhOneNet& on, const MzhSearchParams& p,
                          hipStream_t stream);
size_t mzh_wave_smem_bytes(int S, int nt);
hipError_t mzh_launch_wave_search(const MzhSearchPlan& pl, const MzhWNet& net, const MzhSearchParams& p, hipStream_t stream);
size_t mzh_search_smem_bytes(int R, int S, bool ohl, bool occ2 = false);
hipError_t mzh_launch_search(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p, hipStream_t stream);
hipError_t mzh_launch_infer(int R, bool recurrent, const MzhNet& net, const MzhInferParams& p, hipStream_t stream);
