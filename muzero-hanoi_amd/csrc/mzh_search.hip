// mzh_search.hip -- fused batched MuZero search + batched MLP inference kernels (gfx950).
//
// One workgroup (256 threads = 4 waves) owns R = 16*MT roots and runs ALL of their simulations:
//   select  : 8 lanes per root, one lane per child; fp64 Q / UCB exactly as MCTS/node.py:72-123,
//             6-way argmax + tie detection by shuffles/ballot inside the 8-lane group
//   expand  : recurrent_inference for the R pending leaves as fp32 MFMA GEMMs (mzh_device.h)
//   backup  : one lane per root walks the LDS path leaf -> root (MCTS/node.py:53-70)
// Roots are independent (one owner per tree): no atomics, no inter-workgroup traffic, one launch
// per search.  Trees live in HBM as flat blocks (mzh_tree.h: one 128-B line per expanded node
// holding its 6 children's N/X/R/P/W); the per-sim path, per-root min-max, root stats, UCB table and
// the MLP activations live in LDS.  Weights stream from L2 (shared by every workgroup of an XCD).
#include "mzh_device.h"
#include "mzh_env_kernels.h"
#include "mzh_internal.h"
#include "mzh_rows.h"
#include "mzh_tree.h"

// One workgroup per CU (all 512 registers per lane): the next simulation's first weight chunks stay
// in flight across the tree phase.  Overlapping one root group's tree phase with another's MLP was
// measured slower in both forms tried: two co-resident 16-root workgroups per CU
// (<= 256 registers, no cross-phase prefetch) and a 512-thread workgroup whose waves 0-3 run the MLP
// of one 16-root half while waves 4-7 run the other half's tree work (the co-resident tree work
// took twice as long as alone) -- a v_mfma_f32_16x16x4_f32 stream holds its SIMD's vector issue, so a
// partner wave's tree work stalls beside it (tools/micro/overlap_probe.hip).  The 32-root tile on 8
// waves with both waves of a SIMD in the same phase lost 9% too.
//
// Per simulation: the MLP (all four waves split every layer's output tiles, activations in LDS),
// one barrier, then each root's own 8-lane group runs -- with no further workgroup barrier -- the
// heads of its row, the backup of this simulation and the selection of the next one, then one
// barrier.  Tree-phase mapping: root r = wave * (R / 4) + lane / 8, child slot c = lane % 8, so the
// tree work of R = 16 roots is spread over all four waves as well.
template <int R>
constexpr int search_dc() { return R == 32 ? 16 : 32; }  // LDS-cached path depths

// MMIN: the launch has caller-given MinMaxStats bounds (p.minmax_in), which could make max - min
// subnormal: the selection then checks for that (MzhTree::select)
// C8: the two-workgroups-per-CU form (mzh_search_occ2_kernel): 16-root tile, <= 256 registers, the MLP
// on 8-fragment weight chunks (mzh_mlp_recurrent_c8), DC = 16 cached path depths, no one-hot in LDS
// TILE: where the workgroup's roots [root0, root0 + nvalid), nvalid <= R, come from -- MzhGridTile (workgroup b
// owns the R roots from b * R: the single-network kernels) or a tile table entry (mzh_search_multi_kernel)

template <int R, int DC, bool C8, bool REPLAY, bool OHL, bool SUP33, bool MMIN, class TILE = MzhGridTile>
__device__ __forceinline__ void mzh_search_body(const MzhNet& net, const MzhSearchParams& p, const TILE tile = TILE{}) {
  static_assert(!C8 || (R == 16 && !OHL), "the 8-fragment MLP is the 16-root tile's");
  constexpr int NF = C8 ? 8 : 16;  // fragments per weight buffer
  using Smem = SearchSmem<R, DC>;
  // tree-phase waves: all four (R / 4 roots each), or for C8 two full waves of 8 roots -- waves 0-1 of one
  // workgroup of a CU's pair, waves 2-3 of the other (workgroups b and b + 256 share a CU when 512 of them
  // fill 256 CUs two deep), so each SIMD runs one 8-root tree wave per simulation as in the 32-root tile
  // instead of two half-empty ones (the pairing is a placement guess: correctness does not depend on it)
  constexpr int TRW = C8 ? 2 : 4;
  constexpr int RPW = R / TRW;  // roots per tree wave
  constexpr int N2 = SUP33 ? 2 : 1;  // rwd2 / val2 MFMA tiles (bin 32 of a 33-bin head: vector chains)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  MlpSmem<R>& sm = *reinterpret_cast<MlpSmem<R>*>(smem_raw);
  Smem& st = *reinterpret_cast<Smem*>(smem_raw + sizeof(MlpSmem<R>));
  double* table = reinterpret_cast<double*>(smem_raw + sizeof(MlpSmem<R>) + sizeof(Smem));
  double* inv = table + (p.S + 3);  // inv[k] = RN(1/k), k <= S + 2
  uint16_t* path = reinterpret_cast<uint16_t*>(table + 2 * (p.S + 3));
  // OHL: the dynamics one-hot columns (6 x 256 floats) live in LDS (when the launcher finds room)
  float* ohl = reinterpret_cast<float*>(path + ((R * (p.S + 1) + 7) & ~7));

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int root0 = tile.template root0<R>();
  const int nvalid = tile.template nvalid<R>(p.B, root0);
  // the simulations of this workgroup's roots: p.S, or the tile's own budget (<= p.S, workgroup-uniform, so every
  // barrier below stays uniform); the LDS layout and the path rows are those of p.S, the launch's maximum
  int sims;
  if constexpr (TILE::kOwnSims) sims = tile.sims(); else sims = p.S;
  const int S = sims;
  const int SMAX = TILE::kOwnSims ? p.S : S;  // the launch's n_sims
  const int PL = SMAX + 1;  // path row length
  const double disc = p.discount;
  const bool noised = p.noise != nullptr;
  // this lane's root (tree phases) and child slot
  const int tw = C8 ? wave - ((blockIdx.x >> 8) & 1) * 2 : wave;  // tree-wave index (wave-uniform)
  const int tr = tw * RPW + (lane >> 3), tc = lane & 7;
  const bool tgroup = (unsigned)tw < (unsigned)TRW && (lane >> 3) < RPW;  // wave-uniform per 8-lane group

  if (OHL)
    for (int i = tid; i < MZH_A * MZH_F; i += MZH_THREADS) ohl[i] = net.dyn0_onehot[i];
  if (SUP33 && !REPLAY) mzh_w32_fill<R>(sm, net, tid);
  for (int i = tid; i < SMAX + 3; i += MZH_THREADS) {
    table[i] = i < SMAX + 2 ? p.table[i] : 0.0;
    inv[i] = 1.0 / (double)i;  // IEEE division: correctly rounded
  }
  if (tid < R) {
    const int r = tid;
    st.rootN[r] = 0;
    st.rootW[r] = 0.0;
    st.firstTie[r] = 0;
    st.extra[r] = 0;
    st.steps[r] = 0;
    st.depth[r] = 0;
    st.tie[r] = (p.tie_idx && r < nvalid) ? p.tie_idx[root0 + r] : 0;
    if (p.minmax_in && r < nvalid) {
      st.mm[r].set(p.minmax_in[2 * (root0 + r)], p.minmax_in[2 * (root0 + r) + 1]);
    } else {
      st.mm[r].set(-__builtin_inf(), __builtin_inf());
    }
  }

  // ---------------- root: initial_inference (mcts.py:49-50) ----------------
  if (!REPLAY) {
    for (int i = tid; i < R * p.kin; i += MZH_THREADS) {
      const int r = i / p.kin, k = i - r * p.kin;
      sm.x[r * MZH_LD64 + mzh_kpos(k)] = (r < nvalid && k < p.in_dim) ? p.obs[(size_t)(root0 + r) * p.in_dim + k] : 0.0f;
    }
    __syncthreads();
    mzh_mlp_initial<R>(sm, net, wave, lane);
    for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
      const int r = i >> 6, k = i & 63;
      if (r < nvalid) p.htree[((size_t)(root0 + r) * p.E) * MZH_H + k] = sm.x[r * MZH_LD64 + k];
    }
  } else {
    if (tid < R * 8) {
      const int r = tid >> 3, c = tid & 7;
      sm.pi[r * 8 + c] = (r < nvalid && c < MZH_A) ? p.rp_root_pi[(size_t)(root0 + r) * MZH_A + c] : 0.0f;
    }
    __syncthreads();
  }
  // root.expand(prior, h, 0) with optional Dirichlet mixing (mcts.py:57-69, 132-152)
  if (tid < R * 8) {
    const int r = tid >> 3, c = tid & 7;
    MzhRootBlk& rb = st.root[r];
    const float pr = (r < nvalid && c < MZH_A) ? sm.pi[r * 8 + c] : 0.0f;
    rb.N[c] = 0;
    rb.X[c] = -1;
    rb.R[c] = 0.0f;
    rb.W[c] = 0.0;
    const bool mix = noised && r < nvalid && c < MZH_A;
    rb.P64[c] = mzh_root_prior(pr, mix, p.eps, mix ? p.noise[(size_t)(root0 + r) * MZH_A + c] : 0.0);
  }
  if (tid < R && tid >= nvalid) sm.act[tid] = 0;  // rows beyond the batch: any valid one-hot index
  floatx4 fa[NF], fb[NF];
  float ba[4], bb[4];
  if (!REPLAY) {
    if constexpr (C8)
      mzh_mlp_fetch12_c8(sm, net, wave, lane, fa, ba, fb, bb);
    else
      mzh_mlp_fetch12<R>(sm, net, wave, lane, fa, ba, fb, bb);
  }
  __syncthreads();

  MzhTree<R, DC, REPLAY, MlpSmem<R>> tree{p, st, sm, path, table, inv, root0, PL, lane, disc, noised};

  // within a root's 8-lane group: LDS and tree stores of one step are visible to the next step
  auto group_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  };

  // the root's state lives in its group's registers from here to the results
  MzhRootReg rs;
  const bool town = tgroup && tr < nvalid;
  if (town) rs.load(st, tr);

  // p.lockstep_levels: the workgroup's deepest selection below the root per simulation (every wave's
  // maximum through LDS, read by thread 0 after the simulation's closing barrier).  Selection k writes
  // slot k & 1: without an MLP (replay) the other waves may finish selection k + 1 before thread 0 has
  // read selection k's maxima, but selection k + 2 -- the next writer of that slot -- starts only after
  // the barrier that thread 0 reaches once it has read them
  const bool lcount = p.lockstep_levels != nullptr;
  int lsum = 0;
  auto wave_level = [&](int k) {
    int m = town ? rs.depth - 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (lane == 0) st.lvl[k & 1][wave] = m;
  };
  auto group_level = [&](int k) {
    int m = st.lvl[k & 1][0];
#pragma unroll
    for (int w = 1; w < MZH_WAVES; ++w) m = max(m, st.lvl[k & 1][w]);
    lsum += m;
  };
  MZH_STAMP_DECL
  if (town) tree.template select<MMIN>(tr, tc, 0, rs);
  if (lcount) wave_level(0);
  __syncthreads();
  if (lcount && tid == 0 && S > 0) group_level(0);
  for (int s = 0; s < S; ++s) {
    // ---------------- expand via the network (mcts.py:88-106) ----------------
    if (!REPLAY) {
      MZH_STAMP(19);
      if constexpr (C8) {
        // the previous simulation's last chunks loaded this one's A1 / A2 into the swapped buffers
        if (s > 0) mzh_c8_swap(fa, ba, fb, bb);
        mzh_mlp_recurrent_c8<N2>(sm, net, wave, lane, fa, ba, fb, bb, net.dyn0_onehot);
      } else {
        mzh_mlp_recurrent_body<R, true, N2, false>(sm, net, wave, lane, fa, ba, fb, bb, OHL ? ohl : net.dyn0_onehot);
      }
      MZH_STAMP(20);
    }
    if (town) {
      const int r = tr, c = tc;
      // this row's heads (networks.py:83,109,152-189) or its recorded network outputs, in registers
      MzhHeadOut ho;
      if (!REPLAY) {
        ho = mzh_heads_row<R, SUP33 ? 33 : 0, false, !SUP33>(sm, net, r, c, net.support, true);
      } else {
        const float* rec = p.rp_sim + ((size_t)s * p.B + root0 + r) * 8;  // 6 priors, reward, value
        ho.pp = c < MZH_A ? rec[c] : 0.0f;
        ho.reward = rec[6];
        ho.value = rec[7];
      }
      MZH_STAMP(21);
      tree.backup(r, c, s, rs, ho.value, ho.reward, ho.pp);
      MZH_STAMP(22);
      if (s + 1 < S) {
        group_sync();
        tree.template select<MMIN>(r, c, s + 1, rs);
        MZH_STAMP(30);
      }
    }
    if (lcount && s + 1 < S) wave_level(s + 1);
    __syncthreads();
    if (lcount && tid == 0 && s + 1 < S) group_level(s + 1);
    MZH_STAMP(23);
  }
  if (lcount && tid == 0) p.lockstep_levels[blockIdx.x] = lsum;

  // ---------------- results (mcts.py:111-126, 154-176) ----------------
  if (town && tc == 0) rs.store(st, tr);
  __syncthreads();
  if (tid < R * 8) {
    const int r = tid >> 3, c = tid & 7;
    if (r < nvalid && c == 0) {
      if constexpr (TILE::kOwnSims)
        tree.results(r, S);
      else
        tree.results(r);
    }
  }
}

template <int R, bool REPLAY, bool OHL, bool SUP33, bool MMIN>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_search_kernel(MzhNet net, MzhSearchParams p) {
  mzh_search_body<R, search_dc<R>(), false, REPLAY, OHL, SUP33, MMIN>(net, p);
}

// Two 16-root workgroups per CU (<= 256 registers, <= 80 KB LDS each): while one runs its MLP's MFMA
// chains the other's tree phase (dependent block loads, fp64 chains) fills the SIMDs' stalls
template <bool SUP33, bool MMIN>
__global__ __launch_bounds__(MZH_THREADS, 2) void mzh_search_occ2_kernel(MzhNet net, MzhSearchParams p) {
  mzh_search_body<16, 16, true, false, false, SUP33, MMIN>(net, p);
}

// ------------------------------------------------------------------------------------------
// Search over a set of networks (mzh_search_multi): root b is searched under network net_index[b].  The
// roots of one network are consecutive, so a one-workgroup prologue cuts the batch into tiles of up to R
// roots of one network each (MzhTile), and the search kernel's workgroup t reads tile t: which blob of the
// set it streams its weights from is decided once, before its first barrier.
// ------------------------------------------------------------------------------------------
// the int32 form of the wave scan of mzh_replay.hip / mzh_ingest.hip: row_shr 1, 2, 4, 8 within rows of 16,
// then row_bcast 15 / 31 (inclusive sums over the wave's 64 lanes; every lane active)
template <int CTRL, int ROWS>
__device__ __forceinline__ int mzh_dpp_i32(int v) {
  if (ROWS == 0xF) return __builtin_amdgcn_mov_dpp(v, CTRL, ROWS, 0xF, true);
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false);
}
__device__ __forceinline__ int mzh_wave_scan_i32(int v) {
  v += mzh_dpp_i32<0x111, 0xF>(v);
  v += mzh_dpp_i32<0x112, 0xF>(v);
  v += mzh_dpp_i32<0x114, 0xF>(v);
  v += mzh_dpp_i32<0x118, 0xF>(v);
  v += mzh_dpp_i32<0x142, 0xA>(v);
  v += mzh_dpp_i32<0x143, 0xC>(v);
  return v;
}

// The budget form of the prologue (bp.n_sims given: mzh_search_multi_budget).  Root b runs n_sims[b] simulations; a
// run is a maximal stretch of consecutive roots with equal (net_index, n_sims), and a tile is up to R consecutive
// roots of one run.  Thread t owns the roots [t C, (t + 1) C), C = ceil(B / T), and walks them three times: it checks
// them and finds its first and last run boundary; it counts its tiles per class; it writes them, a class's tiles
// from the class's first slot on.  The class of a tile is S - budget, so the table lists the deepest budgets first
// (workgroup t of the search takes tile t and dispatch is in order: the launch lasts as long as its deepest tile,
// which must not start last); tiles of one budget take their slots by an LDS atomic, in no fixed order -- no result
// depends on a tile's place in the table.  -DMZH_BUDGET_ROOT_ORDER (A/B builds only): the class is the thread, which
// leaves the tiles in root order.
// Refused as a bad net_index is (tile count 0, status[0] = 1, nothing written to the table): an entry of net_index
// outside [0, M) or below its predecessor, a budget outside [0, S] (0 is the smallest n_sims mzh_search_multi
// accepts), more runs than bp.max_runs, more tiles than the table holds.  A budget indexes LDS only after every
// root's checks have passed.
// cls: dynamic LDS, max(S + 1, T) ints.
__device__ __forceinline__ void mzh_budget_tiles(const MzhMultiParams& mp, const MzhBudgetParams& bp, const int B,
                                                 const int R, int* cls) {
  constexpr int T = MZH_MULTI_MAX_NETS;
  __shared__ int firstb[T];  // the thread's first run boundary (B: none)
  __shared__ int lastb[T];   // its last one (-1: none)
  __shared__ int wtot[T / 64];
  __shared__ int nrun, total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = mp.M, S = bp.S;
#ifdef MZH_BUDGET_ROOT_ORDER
  const int NC = T;
#else
  const int NC = S + 1;
#endif
  const int C = (B + T - 1) / T;
  const int i0 = min(B, tid * C), i1 = min(B, i0 + C);
  for (int k = tid; k < NC; k += T) cls[k] = 0;
  if (tid == 0) nrun = 0;
  __syncthreads();
  auto refuse = [&]() {
    if (tid == 0) {
      *mp.ntiles = 0;
      if (mp.status) {
        mp.status[0] = 1;
        mp.status[1] = 0;
      }
    }
  };
  // root i starts a run where it differs from root i - 1 in either value (root 0 always does)
  const bool inner = i0 > 0 && i0 < i1;
  const int pv0 = inner ? mp.net_index[i0 - 1] : -1, ps0 = inner ? bp.n_sims[i0 - 1] : -1;
  int bad = 0, fb = B, lb = -1, nb = 0;
  {
    int pv = pv0, ps = ps0;
    for (int i = i0; i < i1; ++i) {
      const int v = mp.net_index[i], s = bp.n_sims[i];
      if ((unsigned)v >= (unsigned)M || v < pv || (unsigned)s > (unsigned)S) bad = 1;
      if (i == 0 || v != pv || s != ps) {
        fb = min(fb, i);
        lb = i;
        nb++;
      }
      pv = v;
      ps = s;
    }
  }
  firstb[tid] = fb;
  lastb[tid] = lb;
  if (nb) atomicAdd(&nrun, nb);
  bad = __syncthreads_or(bad);
  if (bad || nrun > bp.max_runs) {  // workgroup-uniform
    refuse();
    return;
  }
  // the run my first root lies in started at `before`; the run my last root lies in ends at `after`
  int before = 0, after = B;
  for (int t = 0; t < tid; ++t) before = max(before, lastb[t]);
  for (int t = tid + 1; t < T; ++t) after = min(after, firstb[t]);
  // walk(f): f(i, v, s) for every root i of mine that starts a tile (a run's roots at multiples of R from its start)
  auto walk = [&](auto f) {
    int pv = pv0, ps = ps0, r0 = before;
    for (int i = i0; i < i1; ++i) {
      const int v = mp.net_index[i], s = bp.n_sims[i];
      if (i == 0 || v != pv || s != ps) r0 = i;
      if (((i - r0) & (R - 1)) == 0) f(i, v, s);
      pv = v;
      ps = s;
    }
  };
  int nt = 0;
  walk([&](int, int, int s) {
    nt++;
#ifndef MZH_BUDGET_ROOT_ORDER
    atomicAdd(&cls[S - s], 1);
#endif
  });
#ifdef MZH_BUDGET_ROOT_ORDER
  cls[tid] = nt;
#endif
  __syncthreads();
  // cls[k]: tiles of class k -> the class's first slot (thread t scans the classes [t CH, (t + 1) CH))
  const int CH = (NC + T - 1) / T;
  const int k0 = min(NC, tid * CH), k1 = min(NC, k0 + CH);
  int part = 0;
  for (int k = k0; k < k1; ++k) part += cls[k];
  const int inc = mzh_wave_scan_i32(part);
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int pre = 0;
  for (int w = 0; w < wave; ++w) pre += wtot[w];
  int slot = pre + inc - part;  // exclusive
  for (int k = k0; k < k1; ++k) {
    const int c = cls[k];
    cls[k] = slot;
    slot += c;
  }
  if (tid == T - 1) total = pre + inc;
  __syncthreads();
  // (runs <= max_runs bounds the tiles by the launcher's grid; the table's size is checked on its own)
  if (total > bp.cap) {
    refuse();
    return;
  }
  int ts = -1, tpos = 0, tnet = 0, tsims = 0;  // the open tile: its first root and slot
  walk([&](int i, int v, int s) {
    if (ts >= 0) mp.tiles[tpos] = MzhTile{ts, i - ts, tnet, tsims};
#ifdef MZH_BUDGET_ROOT_ORDER
    tpos = cls[tid]++;
#else
    tpos = atomicAdd(&cls[S - s], 1);
#endif
    ts = i;
    tnet = v;
    tsims = s;
  });
  // my last tile ends with its R-th root, its run or the batch (a later thread's first boundary, or B)
  if (ts >= 0) mp.tiles[tpos] = MzhTile{ts, min(ts + R, after) - ts, tnet, tsims};
  if (tid == 0) {
    *mp.ntiles = total;
    if (mp.status) {
      mp.status[0] = 0;
      mp.status[1] = total;
    }
  }
}

// One workgroup: check net_index [B] (each entry in [0, M), non-decreasing), find every network's segment,
// give network m ceil(count_m / R) tiles in network order and write them with their count.  A refused
// net_index leaves tile count 0 (the search kernel's workgroups all return) and status[0] = 1.  An entry
// indexes LDS only after it passed the range and order checks, and nothing else ever uses it: the search
// kernel takes the network from the table.  Every tile carries the budget bp.S.  With bp.n_sims the roots have
// budgets of their own and the tiles are cut by mzh_budget_tiles.  With bp.check_sims the tiles are the networks'
// segments still, and a budget outside [0, bp.S] refuses the call as a bad net_index does.
__global__ __launch_bounds__(MZH_MULTI_MAX_NETS) void mzh_multi_tiles_kernel(MzhMultiParams mp, int B, int R,
                                                                             MzhBudgetParams bp) {
  constexpr int T = MZH_MULTI_MAX_NETS;
  if (bp.n_sims) {
    extern __shared__ int mzh_tiles_cls[];
    mzh_budget_tiles(mp, bp, B, R, mzh_tiles_cls);
    return;
  }
  __shared__ int start[T + 1];  // start[m]: first root of network m (B where it has none left); start[M] = B
  __shared__ int toff[T + 1];   // toff[m]: first tile of network m; toff[M] = tiles
  __shared__ int wtot[T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = mp.M;
  // boundary i (0 <= i <= B) lies between entries i - 1 and i, with -1 before the first and M after the last:
  // networks prev + 1 .. v start at root i
  int bad = 0;
  if (bp.check_sims)  // budgets the launch's kernel reads itself: each in [0, bp.S], or the call is refused
    for (int i = tid; i < B; i += T)
      if ((unsigned)bp.check_sims[i] > (unsigned)bp.S) bad = 1;
  for (int i = tid; i <= B; i += T) {
    const int prev = i > 0 ? mp.net_index[i - 1] : -1;
    const int v = i < B ? mp.net_index[i] : M;
    if (prev >= (i > 0 ? 0 : -1) && prev <= v && v < M + (i == B ? 1 : 0)) {
      for (int m = prev + 1; m <= v; ++m) start[m] = i;  // m in [0, M]
    } else {
      bad = 1;
    }
  }
  bad = __syncthreads_or(bad);
  if (bad) {  // start[] is incomplete: nothing below reads it
    if (tid == 0) {
      *mp.ntiles = 0;
      if (mp.status) {
        mp.status[0] = 1;
        mp.status[1] = 0;
      }
    }
    return;
  }
  const int nt = tid < M ? (start[tid + 1] - start[tid] + R - 1) / R : 0;
  const int inc = mzh_wave_scan_i32(nt);
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int pre = 0;
  for (int w = 0; w < wave; ++w) pre += wtot[w];
  toff[tid] = pre + inc - nt;  // exclusive
  if (tid == T - 1) toff[T] = pre + inc;
  __syncthreads();
  // at most ceil(B / R) + min(M, B) - 1 tiles (the launcher's grid and the table's capacity)
  for (int m = 0; m < M; ++m) {
    const int s0 = start[m], cnt = start[m + 1] - s0, t0 = toff[m];
    for (int k = tid; k * R < cnt; k += T) mp.tiles[t0 + k] = MzhTile{s0 + k * R, min(R, cnt - k * R), m, bp.S};
  }
  if (tid == 0) {
    *mp.ntiles = toff[T];
    if (mp.status) {
      mp.status[0] = 0;
      mp.status[1] = toff[T];
    }
  }
}

// MMIN = true always: it only adds the subnormal max - min check, and is bit-identical with fresh bounds.
// A workgroup at or above the tile count (the grid is the upper bound ceil(B / R) + min(M, B) - 1) returns
// before its first barrier.  blockIdx.x is the tile index (p.lockstep_levels is indexed by tile).  The tile's roots
// run the tile's budget: p.S (mzh_search_multi) or the run's own (mzh_search_multi_budget), always from the table.
template <int R, bool OHL, bool SUP33>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_search_multi_kernel(MzhNet net, MzhSearchParams p, MzhMultiParams mp) {
  if ((int)blockIdx.x >= *mp.ntiles) return;
  const MzhTableTile t{mp.tiles[blockIdx.x]};
  mzh_net_select(net, mp, t.t.net, SUP33);
  mzh_search_body<R, search_dc<R>(), false, false, OHL, SUP33, true>(net, p, t);
}

// ------------------------------------------------------------------------------------------
// standalone batched inference kernels (MuZeroNet.initial_inference / recurrent_inference)
// ------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_initial_kernel(MzhNet net, MzhInferParams p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  MlpSmem<R>& sm = *reinterpret_cast<MlpSmem<R>*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * R;
  const int nvalid = min(R, p.B - row0);
  for (int i = tid; i < R * p.kin; i += MZH_THREADS) {
    const int r = i / p.kin, k = i - r * p.kin;
    sm.x[r * MZH_LD64 + mzh_kpos(k)] = (r < nvalid && k < p.in_dim) ? p.x[(size_t)(row0 + r) * p.in_dim + k] : 0.0f;
  }
  __syncthreads();
  mzh_mlp_initial<R>(sm, net, wave, lane);
  mzh_store_outputs<R>(sm, p, row0, nvalid, net.support, false);
}

template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_recurrent_kernel(MzhNet net, MzhInferParams p) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  MlpSmem<R>& sm = *reinterpret_cast<MlpSmem<R>*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * R;
  const int nvalid = min(R, p.B - row0);
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    sm.x[r * MZH_LD64 + mzh_kpos(k)] = r < nvalid ? p.x[(size_t)(row0 + r) * MZH_H + k] : 0.0f;
  }
  if (tid < R) sm.act[tid] = tid < nvalid ? p.action[row0 + tid] : 0;
  __syncthreads();
  mzh_mlp_recurrent<R>(sm, net, wave, lane);
  mzh_store_outputs<R>(sm, p, row0, nvalid, net.support, true);
}

// ------------------------------------------------------------------------------------------
// Action probe (mzh_probe_actions; the reference's legal_illegal_preds.py evaluate_network, lines 26-80): per
// row represent(obs), then recurrent_inference(h, a) for a = 0..5, in one launch.  The R root latents stay in
// LDS (x0) between the six lookaheads -- mzh_mlp_recurrent_body overwrites sm.x with the new latent -- so the
// launch reads each observation once and never writes or re-reads a latent through HBM unless the caller asks
// for h0 / h1.  Every dot product is the chain mzh_initial_kernel / mzh_recurrent_kernel run (the same
// mzh_mlp_initial / mzh_mlp_recurrent on the same LDS block), so a row's outputs are bit-identical to those
// two calls composed.  Row r of the tile is env sm.env[r] of the batch (-1: beyond the tile, or an env index
// outside [0, B): the row runs on a zero observation and stores nothing).
// ------------------------------------------------------------------------------------------
template <int R>
struct ProbeSmem : MlpSmem<R> {
  float x0[R * MZH_LD64];  // the normalised root latents, in sm.x's layout
  int env[R];
};

template <int R, class TILE = MzhGridTile>
__device__ __forceinline__ void mzh_probe_body(const MzhNet& net, const MzhProbeParams& p, const TILE tile = TILE{}) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  ProbeSmem<R>& sm = *reinterpret_cast<ProbeSmem<R>*>(smem_raw);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  mzh_rows_fill<R>(sm.env, p, p.err_count, tile);
  mzh_rows_load_obs<R>(sm.x, sm.env, p);
  __syncthreads();
  MlpSmem<R>& ms = sm;  // the MLP block the inference kernels run on
  mzh_mlp_initial<R>(ms, net, wave, lane);
  // the root, its latent kept for the six lookaheads in the same pass as its store (mzh_rows_store_latent's
  // mapping), and legal on the root store's spare thread
  for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
    const int r = i >> 6, k = i & 63;
    const int e = sm.env[r];
    const float v = sm.x[r * MZH_LD64 + k];
    sm.x0[r * MZH_LD64 + k] = v;
    if (p.h0 && e >= 0) p.h0[(size_t)e * MZH_H + mzh_kpos(k)] = v;
  }
  if (tid < R * 8) {
    const int r = tid >> 3, c = tid & 7;
    const int e = sm.env[r];
    if (e >= 0) {
      if (p.pi0 && c < MZH_A) p.pi0[(size_t)e * MZH_A + c] = sm.pi[r * 8 + c];
      if (p.value0 && c == 6) p.value0[e] = sm.value[r];
      if (p.legal && c == 7) p.legal[e] = mzh_legal_mask_row(p.state + (size_t)e * p.n_disks, p.n_disks);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int a = 0; a < MZH_A; ++a) {
    for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
      const int r = i >> 6, k = i & 63;
      sm.x[r * MZH_LD64 + k] = sm.x0[r * MZH_LD64 + k];
    }
    if (tid < R) sm.act[tid] = a;
    __syncthreads();
    mzh_mlp_recurrent<R>(ms, net, wave, lane);
    if (p.h1)
      for (int i = tid; i < R * MZH_H; i += MZH_THREADS) {
        const int r = i >> 6, k = i & 63;
        const int e = sm.env[r];
        if (e >= 0) p.h1[((size_t)e * MZH_A + a) * MZH_H + mzh_kpos(k)] = sm.x[r * MZH_LD64 + k];
      }
    if (tid < R * 8) {
      const int r = tid >> 3, c = tid & 7;
      const int e = sm.env[r];
      if (e >= 0) {
        if (p.pi1 && c < MZH_A) p.pi1[((size_t)e * MZH_A + a) * MZH_A + c] = sm.pi[r * 8 + c];
        if (c == 6) p.reward[(size_t)e * MZH_A + a] = sm.reward[r];
        if (c == 7) p.value[(size_t)e * MZH_A + a] = sm.value[r];
      }
    }
    __syncthreads();  // the next action's copy overwrites sm.x
  }
}

template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_probe_kernel(MzhNet net, MzhProbeParams p) {
  mzh_probe_body<R>(net, p);
}

// rows of several networks (mzh_rows_multi_tile)
template <int R>
__global__ __launch_bounds__(MZH_THREADS, 1) void mzh_probe_multi_kernel(MzhNet net, MzhProbeParams p, MzhMultiParams mp) {
  if (mzh_rows_no_tile(mp)) return;
  const MzhTableTile t = mzh_rows_multi_tile(net, mp);
  mzh_probe_body<R>(net, p, t);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <int R, int DC = search_dc<R>()>
static size_t search_smem_bytes(int S, bool ohl) {
  size_t b = sizeof(MlpSmem<R>) + sizeof(SearchSmem<R, DC>);
  b += sizeof(double) * 2 * (size_t)(S + 3);
  b += sizeof(uint16_t) * (size_t)((R * (S + 1) + 7) & ~7);
  if (ohl) b += sizeof(float) * MZH_A * MZH_F;
  return (b + 15) & ~(size_t)15;
}

template <int R, bool REPLAY, bool OHL, bool SUP33, bool MMIN>
static hipError_t launch_search_m(const MzhNet& net, const MzhSearchParams& p, hipStream_t stream) {
  const size_t smem = search_smem_bytes<R>(p.S, OHL);
  const void* fn = reinterpret_cast<const void*>(&mzh_search_kernel<R, REPLAY, OHL, SUP33, MMIN>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  const int grid = (p.B + R - 1) / R;
  hipLaunchKernelGGL((mzh_search_kernel<R, REPLAY, OHL, SUP33, MMIN>), dim3(grid), dim3(MZH_THREADS), smem, stream, net,
                     p);
  return hipGetLastError();
}
template <int R, bool REPLAY, bool OHL, bool SUP33>
static hipError_t launch_search_s(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p, hipStream_t stream) {
  // caller-given bounds: the instantiation that checks for a subnormal max - min (MzhTree::select)
  if (pl.mmin) return launch_search_m<R, REPLAY, OHL, SUP33, true>(net, p, stream);
  return launch_search_m<R, REPLAY, OHL, SUP33, false>(net, p, stream);
}
template <int R, bool REPLAY, bool OHL>
static hipError_t launch_search_t(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p, hipStream_t stream) {
  // the replay kernel never runs the network: one instantiation (SUP33 = true) serves both supports
  if (REPLAY || pl.sup33) return launch_search_s<R, REPLAY, OHL, true>(pl, net, p, stream);
  return launch_search_s<R, REPLAY, OHL, false>(pl, net, p, stream);
}

// the LDS a search launch needs at tile R (ohl: with the dynamics one-hot columns in LDS; occ2: the
// two-workgroups-per-CU kernel, 16 cached path depths)
size_t mzh_search_smem_bytes(int R, int S, bool ohl, bool occ2) {
  if (occ2) return search_smem_bytes<16, 16>(S, false);
  return R == 32 ? search_smem_bytes<32>(S, ohl) : search_smem_bytes<16>(S, ohl);
}

template <bool SUP33, bool MMIN>
static hipError_t launch_search_occ2(const MzhNet& net, const MzhSearchParams& p, hipStream_t stream) {
  const size_t smem = search_smem_bytes<16, 16>(p.S, false);
  const void* fn = reinterpret_cast<const void*>(&mzh_search_occ2_kernel<SUP33, MMIN>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  const int grid = (p.B + 15) / 16;
  hipLaunchKernelGGL((mzh_search_occ2_kernel<SUP33, MMIN>), dim3(grid), dim3(MZH_THREADS), smem, stream, net, p);
  return hipGetLastError();
}

// the instantiation the plan names (mzh_api_search.hip make_plan decides every template argument)
hipError_t mzh_launch_search(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p, hipStream_t stream) {
  if (pl.occ2) {
    if (pl.sup33) return pl.mmin ? launch_search_occ2<true, true>(net, p, stream) : launch_search_occ2<true, false>(net, p, stream);
    return pl.mmin ? launch_search_occ2<false, true>(net, p, stream) : launch_search_occ2<false, false>(net, p, stream);
  }
  if (pl.R == 32) {
    if (pl.replay) return launch_search_t<32, true, false>(pl, net, p, stream);
    if (pl.ohl) return launch_search_t<32, false, true>(pl, net, p, stream);
    return launch_search_t<32, false, false>(pl, net, p, stream);
  }
  if (pl.replay) return launch_search_t<16, true, false>(pl, net, p, stream);
  if (pl.ohl) return launch_search_t<16, false, true>(pl, net, p, stream);
  return launch_search_t<16, false, false>(pl, net, p, stream);
}

// the tile table of n rows with budgets of their own (bp.n_sims given)
static hipError_t launch_budget_tiles(const MzhMultiParams& mp, const MzhBudgetParams& bp, int n, int R, hipStream_t stream) {
  const size_t smem = sizeof(int) * (size_t)(bp.S + 1 > MZH_MULTI_MAX_NETS ? bp.S + 1 : MZH_MULTI_MAX_NETS);
  hipLaunchKernelGGL(mzh_multi_tiles_kernel, dim3(1), dim3(MZH_MULTI_MAX_NETS), smem, stream, mp, n, R, bp);
  return hipGetLastError();
}

// bp == nullptr: every root runs p.S simulations
template <int R, bool OHL, bool SUP33>
static hipError_t launch_multi_t(int grid, const MzhNet& net, const MzhSearchParams& p, const MzhMultiParams& mp,
                                 const MzhBudgetParams* bp, hipStream_t stream) {
  const size_t smem = search_smem_bytes<R>(p.S, OHL);
  const void* fn = reinterpret_cast<const void*>(&mzh_search_multi_kernel<R, OHL, SUP33>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  e = bp ? launch_budget_tiles(mp, *bp, p.B, R, stream) : mzh_launch_multi_tiles(mp, p.B, R, stream, p.S);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mzh_search_multi_kernel<R, OHL, SUP33>), dim3(grid), dim3(MZH_THREADS), smem, stream, net, p, mp);
  return hipGetLastError();
}

// the tile table of the batch, then mzh_search_multi_kernel<pl.R, pl.ohl, pl.sup33> on the table's upper bound
// of workgroups; net is the set's network 0
static hipError_t launch_multi(int grid, const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p,
                               const MzhMultiParams& mp, const MzhBudgetParams* bp, hipStream_t stream) {
  if (pl.R == 32) {
    if (pl.ohl) return pl.sup33 ? launch_multi_t<32, true, true>(grid, net, p, mp, bp, stream) : launch_multi_t<32, true, false>(grid, net, p, mp, bp, stream);
    return pl.sup33 ? launch_multi_t<32, false, true>(grid, net, p, mp, bp, stream) : launch_multi_t<32, false, false>(grid, net, p, mp, bp, stream);
  }
  if (pl.ohl) return pl.sup33 ? launch_multi_t<16, true, true>(grid, net, p, mp, bp, stream) : launch_multi_t<16, true, false>(grid, net, p, mp, bp, stream);
  return pl.sup33 ? launch_multi_t<16, false, true>(grid, net, p, mp, bp, stream) : launch_multi_t<16, false, false>(grid, net, p, mp, bp, stream);
}
hipError_t mzh_launch_search_multi(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p,
                                   const MzhMultiParams& mp, hipStream_t stream) {
  return launch_multi(mzh_multi_max_tiles(p.B, pl.R, mp.M), pl, net, p, mp, nullptr, stream);
}
// the same kernels on the tile table of the roots' own budgets, on the upper bound of the tiles bp.max_runs runs make
// (mzh_multi_max_tiles with the runs in place of the networks)
hipError_t mzh_launch_search_multi_budget(const MzhSearchPlan& pl, const MzhNet& net, const MzhSearchParams& p,
                                          const MzhMultiParams& mp, const MzhBudgetParams& bp, hipStream_t stream) {
  return launch_multi(mzh_multi_max_tiles(p.B, pl.R, bp.max_runs), pl, net, p, mp, &bp, stream);
}

template <int R>
static hipError_t launch_infer_t(bool recurrent, const MzhNet& net, const MzhInferParams& p, hipStream_t stream) {
  const size_t smem = (sizeof(MlpSmem<R>) + 15) & ~(size_t)15;
  const void* fn = recurrent ? reinterpret_cast<const void*>(&mzh_recurrent_kernel<R>)
                             : reinterpret_cast<const void*>(&mzh_initial_kernel<R>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  const int grid = (p.B + R - 1) / R;
  if (recurrent)
    hipLaunchKernelGGL((mzh_recurrent_kernel<R>), dim3(grid), dim3(MZH_THREADS), smem, stream, net, p);
  else
    hipLaunchKernelGGL((mzh_initial_kernel<R>), dim3(grid), dim3(MZH_THREADS), smem, stream, net, p);
  return hipGetLastError();
}

#ifdef MZH_STAMPS
// diagnostic build only: read and clear the accumulated phase stamps [8 waves][MZH_NSTAMP]
extern "C" int mzh_diag_stamps(unsigned long long* host) {
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(mzh_stamp_acc), sizeof(mzh_stamp_acc)) != hipSuccess) return -2;
  static unsigned long long zero[8][MZH_NSTAMP] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(mzh_stamp_acc), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
#endif

hipError_t mzh_launch_infer(int R, bool recurrent, const MzhNet& net, const MzhInferParams& p, hipStream_t stream) {
  return R == 32 ? launch_infer_t<32>(recurrent, net, p, stream) : launch_infer_t<16>(recurrent, net, p, stream);
}

template <int R>
static size_t probe_smem_bytes() { return (sizeof(ProbeSmem<R>) + 15) & ~(size_t)15; }
size_t mzh_probe_smem_bytes(int R) { return R == 32 ? probe_smem_bytes<32>() : probe_smem_bytes<16>(); }

// the tile table of n rows at R rows per tile (the prologue of every multi-network launch)
hipError_t mzh_launch_multi_tiles(const MzhMultiParams& mp, int n, int R, hipStream_t stream, int sims,
                                  const int32_t* check_sims) {
  MzhBudgetParams bp{};
  bp.S = sims;
  bp.check_sims = check_sims;
  hipLaunchKernelGGL(mzh_multi_tiles_kernel, dim3(1), dim3(MZH_MULTI_MAX_NETS), 0, stream, mp, n, R, bp);
  return hipGetLastError();
}

hipError_t mzh_launch_probe(int R, const MzhNet& net, const MzhProbeParams& p, const MzhMultiParams* mp, hipStream_t stream) {
  if (R == 32)
    return mzh_rows_launch(&mzh_probe_multi_kernel<32>, &mzh_probe_kernel<32>, 32, probe_smem_bytes<32>(), p.n, mp, stream, net, p);
  return mzh_rows_launch(&mzh_probe_multi_kernel<16>, &mzh_probe_kernel<16>, 16, probe_smem_bytes<16>(), p.n, mp, stream, net, p);
}
