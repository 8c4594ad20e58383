/*
 * mzh.h -- C ABI of libmzh.so: MI355X-native (gfx950 HIP) batched MuZero-MCTS + Tower-of-Hanoi.
 *
 * The reference (A-Andrews/Muzero-Hanoi) is pure Python; its "plugin boundary" is the duck-typed
 * Python API that training_main.py / Muzero.py / the acting scripts call.  Each entry point below
 * replaces one of those interfaces (cited file:line); the Python host layer in muzero-hanoi_amd/
 * binds them with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every buffer argument is a DEVICE pointer owned by the caller (e.g. a torch tensor's
 *    data_ptr()), except where "host" is written.  Shapes are row-major; B = batch of roots/envs.
 *  - Calls are asynchronous and stream-ordered on `stream` (a hipStream_t; NULL = null stream).
 *  - Every function returns an int status (MZH_OK = 0, negative on error) and never throws;
 *    mzh_last_error() returns a thread-local message for the last failure.
 *  - An engine is bound to one device and is not re-entrant across threads (one engine per
 *    device/stream, like the reference's single MCTS instance, MCTS/mcts.py:23).
 *  - No CPU fallback exists: without a HIP device every compute call fails with MZH_ERR_HIP.
 */
#ifndef MZH_ABI_H_
#define MZH_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZH_ABI_VERSION 6

#define MZH_OK 0
#define MZH_ERR_ARG (-1)         /* bad argument / shape (ValueError in Python)              */
#define MZH_ERR_HIP (-2)         /* HIP runtime error / no device (RuntimeError)              */
#define MZH_ERR_CAPACITY (-3)    /* B > max_roots or n_sims > max_sims of the engine          */
#define MZH_ERR_STATE (-4)       /* weights not loaded                                        */
#define MZH_ERR_TEMPERATURE (-5) /* temperature outside [0,1] (mcts.py:163-166 ValueError)    */

#define MZH_ACTIONS 6   /* itertools.permutations(range(3), 2), env/hanoi.py:39-41 */
#define MZH_LATENT 64   /* reprs_output_size, networks.py:22 */
#define MZH_HIDDEN 256  /* h1_s, networks.py:21 */

/* search flags */
#define MZH_FLAG_NP1_UCB 1u /* UCB rounding of NumPy 1.x (the reference's pin, requirements.txt:17):
                               U = fl32(fl64(prior * w)); default is NumPy 2: fl32(prior * fl32(w)) */
#define MZH_FLAG_KERNEL_COOP 2u /* force the cooperative kernel (4 waves share one 32-root tile) */
#define MZH_FLAG_KERNEL_WAVE 4u /* force the wave-independent kernel, 32 roots per wave (default for B >= 53248) */
#define MZH_FLAG_KERNEL_WAVE16 8u /* force the wave-independent kernel, 16 roots per wave (default for 8192 < B < 53248) */
#define MZH_FLAG_COOP_TILE16 16u /* cooperative kernel: 16 roots per workgroup (default for B <= 4096) */
#define MZH_FLAG_COOP_TILE32 32u /* cooperative kernel: 32 roots per workgroup (default for B > 4096) */
#define MZH_FLAG_COOP_OCC2 64u /* cooperative kernel, 16-root tiles, two workgroups per CU
                                  (mzh_search_occ2_kernel).  An MLP search whose LDS does not fit twice per
                                  CU fails with MZH_ERR_CAPACITY; a replay (tree-only) search, which has no
                                  occ2 instantiation, runs the cooperative replay kernel instead (the plan
                                  names it) */
#define MZH_FLAG_KERNEL_ONE 128u /* force the latency kernel (mzh_search_one_kernel: one root per workgroup,
                                    the network stationary on the CU; default for MLP searches of B <= 512
                                    roots whose LDS fits).  An error for replay searches, with another kernel
                                    flag, or where its LDS does not fit */

typedef struct mzh_engine mzh_engine;
typedef void* mzh_stream; /* hipStream_t */

int mzh_abi_version(void);
const char* mzh_last_error(void);
/* Provenance: a hash of the csrc/ sources, include/mzh.h and the compiler flags this library was
 * built from (muzero-hanoi_amd/build.py source_hash); the Python binding refuses a library whose id
 * differs from the checked-out sources, and bench / smoke records print it. */
const char* mzh_build_id(void);
int mzh_device_count(int* count);
/* The device address of page-locked host memory (hipHostGetDevicePointer): the one-root drop-in calls
 * (MCTS.run_mcts, TowersOfHanoi.step) hand their few inputs and outputs to the kernels in pinned host memory
 * the kernels read and write directly, so a call is one launch and one synchronisation, no copies. */
int mzh_host_device_pointer(void* host, void** dev);
/* Wait for every call issued on `stream` (hipStreamSynchronize): the one-root drop-ins' single synchronisation
 * per call, without a framework stream object per call. */
int mzh_stream_synchronize(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Engine.  Replaces the state the reference keeps in Python objects: the MuZeroNet weights
 * (networks.py:39-67) and the per-search node pool of MCTS/node.py (flat SoA tree workspace).
 *   n_disks   : Hanoi N (observation = 3N one-hot, env/hanoi.py:26-28, utils.py:9-25), 1..16: an observation of
 *               3..48 columns, zero-padded to 16, 32 or 48 (one to three k-blocks of the first representation
 *               layer).  The test suite runs every kernel that takes a network at both ends of that range and
 *               on either side of each block boundary (3, 6, 15, 18, 33 and 48 columns beside 9, 12 and 21;
 *               tests/test_widths_gpu.py); the training update (mzh_train_update) takes up to 32 columns and is
 *               run at 3 to 30.
 *   max_sims  : largest n_simulations a search on this engine may use (mcts.py:30)
 *   max_roots : largest root batch B
 *   support   : 33 (TD_return=True) or 1 (TD_return=False), networks.py:34-37
 * ------------------------------------------------------------------------------------------- */
int mzh_create(int device, int n_disks, int max_sims, int max_roots, int support, mzh_engine** out);
int mzh_destroy(mzh_engine* eng);

/* Number of floats of the canonical flat weight vector: the 20 tensors of MuZeroNet.state_dict()
 * (networks.py:39-67) concatenated in the order
 *   {representation,dynamic,rwd,policy,value}_net.{0,2}.{weight,bias},
 * each in torch layout (nn.Linear weight [out][in] row-major). */
int mzh_weights_size(int n_disks, int support, size_t* n_floats);

/* Upload + repack (host pointer, canonical layout) into the MFMA fragment layout on the device.
 * Replaces reading MuZeroNet parameters at inference time (networks.py:71-150). Synchronous. */
int mzh_load_weights(mzh_engine* eng, const float* flat_host, size_t n_floats);

/* Upload a SET of M networks of the engine's shape (1 <= M <= 256) for mzh_search_multi: flat_host holds M
 * canonical vectors of n_floats each, [M][n_floats].  The reference's ablation sweeps (acting_ablations.py,
 * multi_run_ablation_eval.py, permutation_importance.py get_ablated_network) evaluate up to 8 re-initialised
 * variants of one checkpoint one after the other; a set lets one launch search roots of all of them.
 * Each vector is packed exactly as mzh_load_weights packs it; the M blobs lie in one device allocation of
 * the set's own at a constant stride (one blob rounded up to 256 bytes).  The engine's single network
 * (mzh_load_weights) and every call that uses it are untouched by a set.  Loading a set replaces the previous
 * one.  Synchronous.  MZH_ERR_ARG: M outside [1, 256], n_floats != mzh_weights_size, a NULL pointer. */
int mzh_load_weight_set(mzh_engine* eng, const float* flat_host, size_t n_floats, int M);

/* The same loads from the LIVE parameter tensors on the device, without a host round trip: the packers only
 * copy, so a blob is a fixed permutation of the canonical weights with zero fill (mzh_pack_map), and one
 * gather kernel (mzh_repack_kernel) writes the blobs from the 20 tensors where an optimiser step left them.
 *   param : HOST array of 20 DEVICE pointers (mzh_load_weight_set_device: [M][20]), contiguous fp32 tensors in
 *           torch layout, in state_dict order -- the order of mzh_weights_size and of mzh_train_args.param.
 * After the call the engine is in the state mzh_load_weights / mzh_load_weight_set leaves it in for the same
 * values: the same blob bytes, and every later call gives bit-identical results.  Either kind of load may follow
 * the other.
 * Stream-ordered: the gather reads the parameters as they are when `stream` reaches it, and calls that use the
 * weights must be ordered after it (the same stream, or an event).  The engine's buffers are allocated by the
 * first load of either kind and kept (a set's are reallocated only when M changes); the map is uploaded once
 * per engine; the table of parameter pointers is uploaded when the pointers differ from the previous call's.
 * Otherwise the call makes no allocation, frees nothing and does not wait for the device, with two exceptions:
 *   - single network with a 33-bin head: the search kernels take bias bin 32 of the reward and the value head
 *     by value, so the call reads those two floats back (one 8-byte copy) and waits for `stream`.  Support 1
 *     and sets (whose scalars stay in device memory) do not wait;
 *   - mzh_load_weights_device drops an existing expansion memo exactly as mzh_load_weights does, which waits
 *     for the device.
 * MZH_ERR_ARG, before any device work: a NULL engine, param or entry; M outside [1, 256]. */
int mzh_load_weights_device(mzh_engine* eng, const float* const* param, mzh_stream stream);
int mzh_load_weight_set_device(mzh_engine* eng, const float* const* param, int M, mzh_stream stream);

/* The packers as index maps (host-only: no device, no engine).  which = 0 the main blob (the three kernel
 * layouts), 1 the transposed blob of mzh_saliency.  map[j] is the canonical index (the order of
 * mzh_weights_size) whose value blob float j holds, or -1 where the blob holds +0.0f; map may be NULL (sizes
 * only).  *n_floats: the blob's floats.  scalar_src (nullable) [2]: the canonical indices of rwd_net.2.bias[32]
 * and value_net.2.bias[32], the two values the kernels take by value, or -1 at support 1.
 * MZH_ERR_ARG: n_disks / support that mzh_weights_size refuses, which outside {0, 1}. */
int mzh_pack_map(int n_disks, int support, int which, int32_t* map /* nullable */, size_t* n_floats /* nullable */,
                 int64_t* scalar_src /* nullable */);

/* Debug, like mzh_memo_debug_table: a copy of a weight buffer as the kernels read it.  which = 0 / 1 the
 * engine's network (main / transposed blob), 2 / 3 the loaded set (2: the whole allocation, the M blobs at
 * their stride and the [M][2] scalar tail).  dst: device buffer of *n_floats floats, or NULL (size only).
 * Waits for the device.  MZH_ERR_ARG: NULL engine or n_floats, which outside [0, 3]; MZH_ERR_STATE: nothing of
 * that kind is loaded. */
int mzh_weights_debug_blob(mzh_engine* eng, int which, float* dst /* nullable */, size_t* n_floats);
/* Debug: counters[3] = weight buffer allocations, weight buffer frees and device-wide waits
 * (hipDeviceSynchronize) made by this engine's weight loads and memo drops since mzh_create: a refresh that
 * reuses the buffers moves none of them. */
int mzh_weights_debug_counters(mzh_engine* eng, uint64_t* counters);

/* ---------------------------------------------------------------------------------------------
 * Environment: TowersOfHanoi (env/hanoi.py), batched over B independent envs.
 * state[B][n] uint8 peg of disc d (disc 0 = smallest), the reference's tuple c_state layout.
 * ------------------------------------------------------------------------------------------- */

/* TowersOfHanoi.step (env/hanoi.py:47-84) for every env b:
 *   state      in/out  c_state (unchanged on illegal moves and on the goal step, hanoi.py:65-74)
 *   action     in      index into moves = [(0,1),(0,2),(1,0),(1,2),(2,0),(2,1)]
 *   moved      out     state encoded by the returned observation (nullable)
 *   obs        out     oneHot_encoding(moved) as float32 [B][3n] (nullable; utils.py:9-25)
 *   reward     out     int8 code: 0 -> 0, 1 -> 100 (goal), -1 -> -100/1000 (illegal)
 *   done, illegal out  uint8
 *   step_ctr   in/out  step_counter (hanoi.py:50-80; illegal steps count, reset on done)
 *   active     in/out  reset_check (hanoi.py:49); stepping an inactive env is the reference's
 *                      AssertionError: the env is left untouched, reward = -2 and *err_count += 1
 *   err_count  out     nullable device int32 accumulator */
int mzh_env_step(int n_disks, int goal_peg, int max_steps, int B, uint8_t* state,
                 const int32_t* action, uint8_t* moved, float* obs, int8_t* reward, uint8_t* done,
                 uint8_t* illegal, int32_t* step_ctr, uint8_t* active, int32_t* err_count,
                 mzh_stream stream);

/* Plan-ahead acting (acting_experiments/planning_multiple_actions.py:139-178): execute a search's latent
 * path (mcts.return_latent_actions()[:max_plan_len], MCTS/mcts.py:79-86,128-130) open loop, env.step per
 * entry (env/hanoi.py:47-84), until the plan runs out or the episode ends (goal or max_steps; the rest of
 * the plan is dropped).  Illegal moves are executed like any other.  One launch for n rows of a sub-batch:
 * row j is env env_index[j] of the full batch of B envs (env j where env_index is NULL; the indices of one
 * call must be distinct), its plan is plan[j * plan_stride + k], k < min(plan_len[j], max_plan_len) --
 * mzh_search_args.latent / latent_len of a search over those rows, with plan_stride = n_sims + 1.  Entries
 * at or beyond plan_len[j] are never read.
 *   state, step_ctr, active  in/out  [B] full-batch arrays as in mzh_env_step, indexed by env
 *   obs          in/out  [B][3n] float32: oneHot_encoding of the last executed step's moved state (what
 *                        env.step returned last); untouched where nothing was executed
 *   executed     out     [n] steps executed for row j in this call
 *   steps_total, illegal_total  in/out  [B] per-env sums of executed steps / executed illegal moves
 *   rec_action   out     [max_plan_len][n] int32 executed actions, -1 where nothing ran (nullable)
 *   rec_reward   out     [max_plan_len][n] int8 reward codes of mzh_env_step, 0 where nothing ran (nullable)
 *   err_count    out     nullable device int32 accumulator
 * An env that is inactive on entry is left untouched with executed = 0 (no error: the caller's rows may
 * include finished episodes).  Errors end the row's execution for the call and add 1 to *err_count:
 * plan_len[j] < 1 on an active env (the reference would index an empty list), an action outside 0..5 at
 * a position that would execute, an env index outside [0, B).
 * MZH_ERR_ARG: a NULL required pointer, n < 1, B < 1 (B < n without env_index), max_plan_len < 1,
 * plan_stride < max_plan_len, n_disks outside [1, 32], goal_peg outside [0, 2]. */
typedef struct mzh_plan_args {
  int32_t n_disks, goal_peg, max_steps;
  int32_t B;            /* envs of the full batch */
  int32_t n;            /* rows of this call */
  int32_t max_plan_len; /* planning_multiple_actions.py:47 */
  int32_t plan_stride;  /* ints between two rows' plans */
  const int32_t* env_index; /* [n] or NULL */
  const int32_t* plan;      /* [n][plan_stride] */
  const int32_t* plan_len;  /* [n] */
  uint8_t* state;
  int32_t* step_ctr;
  uint8_t* active;
  float* obs;
  int32_t* executed;
  int32_t* steps_total;
  int32_t* illegal_total;
  int32_t* rec_action;
  int8_t* rec_reward;
  int32_t* err_count;
} mzh_plan_args;

int mzh_env_run_plan(const mzh_plan_args* args, mzh_stream stream);

/* Acting on a perturbed observation (noise_injection_comparison.py:17-37, permutation_importance.py:27-76):
 * the agent searches from an observation that differs from the true state, its action is applied to the true
 * env, and an episode counts as solved when a step returns reward 100.  One launch for n rows of a sub-batch:
 * row j is env env_index[j] of the full batch of B envs (env j where env_index is NULL; the indices of one
 * call must be distinct).  Per row, for an env that is active on entry (an inactive one is left untouched,
 * reward = done = 0, no error: the caller's rows may include finished episodes):
 *   1. with `action`: one TowersOfHanoi.step (env/hanoi.py:47-84) of the true env, c_state not advanced on the
 *      goal step and the episode ended at max_steps as in mzh_env_step; steps_total += 1, illegal_total += 1
 *      on an illegal move, solved = 1 on reward code 1 (`if reward == 100: return True`,
 *      noise_injection_comparison.py:33-34, permutation_importance.py:71-72);
 *   2. if the env is still active: obs = the observation the next search reads -- c_state with disc
 *      perm_disc's peg replaced by perm_peg[j] (permutation_importance.py:55-59), one-hot encoded
 *      (utils.py:9-25), plus noise[j] where given (noise_injection_comparison.py:25-27), each element
 *      (float)((double)onehot + noise): the reference's float64 sum, rounded once by
 *      torch.from_numpy(...).to(float32) (MCTS/mcts.py:49).  An env whose step ended the episode keeps its
 *      obs row.
 * action = NULL is an observe-only call (the first observation of an episode, taken before any step:
 * noise_injection_comparison.py:24-27): nothing is stepped, no tally changes.
 * Errors add 1 to *err_count and leave the row's env, tallies and obs untouched (reward = done = 0): an env
 * index outside [0, B); on an active env an action outside 0..5 (moves[action] IndexError), a perm_disc
 * outside [-1, n_disks), a perm_peg outside 0..2 where the env's perm_disc >= 0.
 * MZH_ERR_ARG, before any launch: a NULL required pointer (state, step_ctr, active, steps_total,
 * illegal_total, solved, obs; perm_peg where perm_disc is given), n < 1, B < 1 (B < n without env_index),
 * n_disks outside [1, 32], goal_peg outside [0, 2]. */
typedef struct mzh_observe_args {
  int32_t n_disks, goal_peg, max_steps; /* TowersOfHanoi(N, max_steps), env/hanoi.py:13-45 */
  int32_t B;                /* envs of the full batch */
  int32_t n;                /* rows of this call */
  const int32_t* env_index; /* [n] or NULL */
  const int32_t* action;    /* [n] index into moves (env/hanoi.py:39-41), or NULL: observe only */
  uint8_t* state;           /* [B][n_disks] in/out c_state, as in mzh_env_step */
  int32_t* step_ctr;        /* [B] in/out step_counter (hanoi.py:50-80) */
  uint8_t* active;          /* [B] in/out reset_check (hanoi.py:49) */
  int32_t* steps_total;     /* [B] in/out executed steps (the play_game loops' iterations) */
  int32_t* illegal_total;   /* [B] in/out executed illegal moves (env.step's fourth value, hanoi.py:70-74) */
  uint8_t* solved;          /* [B] in/out 1 once a step returned reward 100 (hanoi.py:65-69); never cleared */
  const int32_t* perm_disc; /* [B] or NULL: permute_feature, the disc whose peg the model does not see, -1 =
                               none; constant over an episode (permutation_importance.py:55-59) */
  const int32_t* perm_peg;  /* [n] this decision's np.random.randint(0, n_pegs) (permutation_importance.py:58);
                               read only where the row's env has perm_disc >= 0 */
  const double* noise;      /* [n][3 n_disks] or NULL: this decision's np.random.normal(0, noise_std, shape),
                               already scaled by the caller (noise_injection_comparison.py:25-27) */
  float* obs;               /* [B][3 n_disks] in/out: state_one_hot as run_mcts rounds it (MCTS/mcts.py:49) */
  int8_t* reward;           /* [n] nullable: this call's step codes as in mzh_env_step (0 without a step) */
  uint8_t* done;            /* [n] nullable: this call's done flags (hanoi.py:65-80) */
  int32_t* err_count;       /* nullable device int32 accumulator */
} mzh_observe_args;

int mzh_env_step_observe(const mzh_observe_args* args, mzh_stream stream);

/* _move_allowed for all 6 moves (env/hanoi.py:117-139): bit a of mask[b] = move a legal. */
int mzh_legal_mask(int n_disks, int B, const uint8_t* state, uint8_t* mask, mzh_stream stream);

/* oneHot_encoding (utils.py:9-25): obs[b][3d + state[b][d]] = 1, float32. */
int mzh_encode_obs(int n_disks, int B, const uint8_t* state, float* obs, mzh_stream stream);

/* hanoi_solver (env/hanoi_utils.py:4-26): minimal moves to put every disc on goal_peg. */
int mzh_hanoi_solver(int n_disks, int goal_peg, int B, const uint8_t* state, int32_t* moves,
                     mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Network inference (MuZeroNet.initial_inference / recurrent_inference, networks.py:71-116),
 * batched over B rows.  Output pointers other than h may be NULL.
 *   h [B][64] normalised latent; reward [B] (0 for initial); pi [B][6] softmax policy;
 *   value [B] transformed value; *_logits raw head outputs ([B][6], [B][support]).
 * ------------------------------------------------------------------------------------------- */
int mzh_initial_inference(mzh_engine* eng, int B, const float* obs, float* h, float* reward,
                          float* pi, float* value, float* policy_logits, float* value_logits,
                          mzh_stream stream);
int mzh_recurrent_inference(mzh_engine* eng, int B, const float* h_in, const int32_t* action,
                            float* h, float* reward, float* pi, float* value,
                            float* policy_logits, float* value_logits, float* reward_logits,
                            mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Batched search: B independent MCTS.run_mcts calls (MCTS/mcts.py:34-126), one per root, all
 * simulations (select -> expand via the MLP -> backup) inside one fused kernel launch.
 * Each root carries its own MinMaxStats (utils_mcts.py): fresh unless minmax_in is given.
 * ------------------------------------------------------------------------------------------- */
typedef struct mzh_search_args {
  int32_t B;             /* roots */
  int32_t n_sims;        /* n_simulations (mcts.py:30) */
  double discount;       /* mcts.py:27 */
  double eps;            /* root_exploration_eps (mcts.py:20) */
  double temperature;    /* generate_play_policy temperature (mcts.py:154-176) */
  int32_t deterministic; /* argmax action instead of sampling (mcts.py:115-120) */
  uint32_t flags;        /* MZH_FLAG_* */
  /* inputs */
  const float* obs;         /* [B][3n] root observations (MLP mode) */
  const double* noise;      /* [B][6] Dirichlet draws, NULL = no noise (mcts.py:57-66) */
  const int32_t* tie_idx;   /* [B] pre-drawn index of np.random.choice for the first 6-way tie */
  const double* action_u;   /* [B] pre-drawn random_sample() for choice(6, p=pi); NULL if det. */
  const double* minmax_in;  /* [B][2] (maximum, minimum) or NULL (fresh: -inf, +inf) */
  /* replay (tree-only) inputs: network outputs recorded per simulation, used instead of the MLP
   * by mzh_search_replay */
  const float* rp_root_pi; /* [B][6] */
  const float* rp_sim;     /* [n_sims][B][8]: simulation s of root b = its 6 priors, reward, value --
                              simulation-major, so one simulation's reads of consecutive roots are
                              whole cache lines (32 B per root) */
  /* outputs (visits required, others nullable) */
  int32_t* visits;      /* [B][6] root child_N (node.py:133-136) */
  double* root_q;       /* [B] root_node.Q (node.py:125-131) */
  double* minmax_out;   /* [B][2] */
  int32_t* extra_ties;  /* [B] argmax ties beyond the first (RNG stream divergence indicator) */
  int32_t* action;      /* [B] chosen action (mcts.py:115-122) */
  double* pi;           /* [B][6] play policy (mcts.py:154-176) */
  int32_t* latent;      /* [B][n_sims+1] moves of the last simulation's path (mcts.py:79-86) */
  int32_t* latent_len;  /* [B] */
  int32_t* sel_steps;   /* [B] total selection steps (sum of depths), for byte accounting */
  /* play-policy power table (nullable): pow_table[n] = np.power(n, max(1, min(5, 1/T))) for
   * n = 0..n_sims as the caller's NumPy computes it (mcts.py:168-174).  Read only for a non-integer
   * exponent (integer exponents are exact products); without it the device pow is used, which can
   * differ from NumPy's vectorised pow in the last bit. */
  const double* pow_table;
  /* [lockstep groups] (nullable; entries of groups without roots are left untouched): per group of roots
   * that advance through a simulation together -- a wave of the wave kernel (16 or 32 roots, index
   * blockIdx * 4 + wave), a workgroup of the cooperative kernels, each root of the latency kernel (index =
   * root; so B entries cover every plan) -- the sum over simulations of the
   * group's deepest selection below the root, i.e. the dependent tree-block loads the group waits for in
   * sequence (the select / backup latency model, bench.py roofline.tree.latency) */
  int32_t* lockstep_levels;
  /* HOST pointer (nullable): filled with the plan of the launched instantiation (below); B = 0
   * launches nothing and reports kernel "none" */
  struct mzh_search_plan* plan_out;
} mzh_search_args;

/* What a search launch runs: the kernel instantiation chosen from B, n_sims, the flags, the
 * support and whether caller MinMaxStats bounds are given.  There is no reference counterpart (the
 * reference runs one Python MCTS per root, MCTS/mcts.py:34-126); it exists so measurements name
 * the kernel that actually ran. */
typedef struct mzh_search_plan {
  int32_t wave;                  /* 1: mzh_wave_kernel, 0: mzh_search_kernel (cooperative) */
  int32_t roots_per_wave;        /* wave: 16 or 32; cooperative: tile / 4 (tree-phase roots per wave) */
  int32_t roots_per_workgroup;   /* roots one workgroup owns */
  int32_t threads_per_workgroup;
  int32_t workgroups;            /* grid size */
  int64_t smem_bytes;            /* dynamic LDS per workgroup */
  char kernel[96];               /* the template instantiation as rocprofv3 names it, e.g.
                                    "mzh_search_kernel<32, false, true, true, false>" */
} mzh_search_plan;

int mzh_search(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream);
int mzh_search_replay(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream);
/* The plan mzh_search (replay = 0) / mzh_search_replay (replay = 1) would launch for these
 * arguments (has_minmax_in: args.minmax_in != NULL).  Host-only: needs no device and no engine. */
int mzh_search_plan_query(int support, int B, int n_sims, uint32_t flags, int replay, int has_minmax_in,
                          mzh_search_plan* out);

/* The expansion memo of the wave kernel.  A network output is a pure function of the
 * weights, the root state and the action path, and an N-disc game has only 3^N states, so an engine keeps the
 * outputs of every node up to D moves below every one-hot root state in a table: node id(path + a) =
 * 6 id(path) + a + 1 with id(empty) = 0, row = state * K(D) + id with K(D) = 1 + 6 + ... + 6^D, state =
 * sum_i peg(disc i) 3^i.  A row is the node's normalised latent (64 floats, as the search stores it) and a
 * 32-byte record (6 priors, reward, value: the replay record's layout), filled level by level with the
 * inference kernels, so every row is bit for bit what the search would compute.  The table is built by the
 * first mzh_search after mzh_load_weights whose plan is the wave kernel (on that call's stream, which it
 * waits for; never under replay or a weight set), dropped by mzh_load_weights and freed by mzh_destroy.  A
 * root whose observation is not exactly one-hot per disc never uses it.  Results do not depend on the memo.
 *   depth -1: automatic, the largest D whose table fits the byte budget (the default); 0: off; d > 0: force
 *   D = d (MZH_ERR_CAPACITY above 2^26 rows).  A change takes effect with the next search.  The environment
 *   variable MZH_MEMO_DEPTH gives a new engine its initial request; mzh_create refuses a value that is no
 *   integer or that this call would refuse.
 * A build holds, beside the table, about 1.7 times its bytes in temporaries until it returns (0.55 GiB in all
 * at four discs and D = 5).  When a forced depth's build fails, the search fails.  When the automatic depth's
 * build runs out of device memory, the next shallower depth is tried, down to no memo, the search runs as it
 * would have without one, and later searches keep that depth until this call is made again. */
int mzh_set_memo_depth(mzh_engine* eng, int depth);
typedef struct mzh_memo_info {
  int32_t depth;        /* D in use by the next wave search (0: no memo) */
  int32_t built;        /* 1: the table of the loaded weights exists */
  int64_t rows;         /* 3^N K(D) */
  int64_t table_bytes;  /* rows * 288 */
  double build_ms;      /* the last build on the host's clock: allocations, the fill, the wait for it, the frees */
  /* (wave, simulation) pairs since mzh_create that ran no MLP / the packed 16-column MLP / the full MLP,
   * counted by the wave searches that had a table (the call waits for the device) */
  uint64_t pairs_skipped, pairs_packed, pairs_full;
} mzh_memo_info;
int mzh_memo_stats(mzh_engine* eng, mzh_memo_info* out);
/* Host-only: the depth a request gives for n_disks (as mzh_set_memo_depth reads it), its rows and bytes. */
int mzh_memo_plan(int n_disks, int depth, int32_t* depth_out, int64_t* rows, int64_t* bytes);
/* Debug: the built table's rows and depth (0 / 0 before the build) and, where the device buffers are given, a
 * copy of it: latent [rows][64] (position 16kb + 4g + t of a row holds unit 16kb + 4t + g, the order the wave
 * kernel keeps latents in) and record [rows][8].  Waits for the device. */
int mzh_memo_debug_table(mzh_engine* eng, float* latent /* nullable */, float* record /* nullable */, int64_t* rows,
                         int32_t* depth);

/* The memo's grown extension.  Below depth D the roots of one state still walk almost
 * the same subtrees, so the table grows from each wave search's own misses: extension rows (same latent and
 * record as a dense row) follow the dense ones and are reached through a trie, link[row * 6 + action] = the
 * child's row, hanging off the depth-D rows.  The search kernel only reads it: a root whose new node lies below
 * D hits when its parent has a row and the link holds the child's.  Every root that missed logs the new node
 * (a bounded per-root log; an entry that does not fit is dropped and the node inserted by a later launch), and
 * mzh_search launches a harvest kernel on the same stream right after the search that claims a link per logged
 * node, takes a row and copies the latent and the record the search computed -- so an extension row, like a
 * dense one, is bit for bit what the search would compute, and results depend neither on the table's content
 * nor on the order rows were given out.  A full extension stops growing.  It is made, dropped and freed with
 * the dense table (a table of depth 0 has none) and has its scope: the wave kernels of mzh_search only.
 *   budget_bytes: bytes of extension rows (288 each; 24 more per row of the whole table go to the links);
 *     -1 the default (64 MiB), 0 off -- the search then behaves exactly as without the extension.
 *   log_entries: entries of the per-root miss log (16 bytes each, allocated for max_roots); -1 the default (16).
 * A change takes effect with the next search, which rebuilds the table when the capacity differs.  The
 * environment variable MZH_MEMO_GROW_BYTES gives a new engine its initial budget_bytes; mzh_create refuses a
 * value that is no integer or that this call would refuse. */
int mzh_set_memo_grow(mzh_engine* eng, int64_t budget_bytes, int32_t log_entries);
typedef struct mzh_memo_grow_info {
  int64_t budget_bytes;       /* the request in force (the default's value for -1) */
  int64_t capacity_rows;      /* extension rows of the built table (0: none built, or growth off) */
  int64_t rows_used;          /* rows inserted since the build (the call waits for the device) */
  int64_t rows_last_harvest;  /* rows the last harvest inserted */
  int32_t log_entries;        /* per-root miss log entries in force */
  int32_t reserved;
} mzh_memo_grow_info;
int mzh_memo_grow_stats(mzh_engine* eng, mzh_memo_grow_info* out);
/* Debug: the built table's dense rows, extension capacity and rows in use and, where the device buffers are
 * given, copies of the extension's latent [capacity][64] and record [capacity][8] (extension row i is table row
 * dense_rows + i) and of the links [dense_rows + capacity][6] (the child's table row, 0 none).  Waits for the
 * device. */
int mzh_memo_debug_grow(mzh_engine* eng, float* latent /* nullable */, float* record /* nullable */,
                        int32_t* link /* nullable */, int64_t* rows_used, int64_t* dense_rows, int64_t* capacity_rows);

/* Search roots of several networks in one launch: root b is searched under network net_index[b] of the set
 * loaded by mzh_load_weight_set, with the result mzh_search gives on an engine holding that network alone
 * (bit for bit).  `args` is mzh_search's, unchanged: every input and output is indexed by root.  The roots of
 * one network must be consecutive (net_index non-decreasing); a network without roots is fine.  Two launches:
 * a one-workgroup prologue checks net_index on the device and cuts the batch into tiles of up to 16 or 32
 * roots of one network, then mzh_search_multi_kernel searches one tile per workgroup on a grid of
 * ceil(B / tile) + min(n_networks, B) - 1 workgroups (the most tiles B roots can make; workgroups beyond the
 * tiles made return at once).  args.lockstep_levels is indexed by tile, args.plan_out names the launched
 * instantiation with that grid.
 *   MZH_FLAG_NP1_UCB, MZH_FLAG_COOP_TILE16 / 32 (default: by B as in mzh_search) and MZH_FLAG_KERNEL_COOP
 *   are honoured; only the cooperative kernel has a multi-network form.
 * Refused before anything is launched: no set loaded (MZH_ERR_STATE); n_networks outside [1, M of the set],
 * a NULL net_index, replay inputs (rp_sim / rp_root_pi), or any of MZH_FLAG_KERNEL_WAVE / _WAVE16 /
 * _KERNEL_ONE / _COOP_OCC2 (MZH_ERR_ARG: a forced kernel that cannot serve the search is an error, never a
 * fallback); B or n_sims beyond the engine (MZH_ERR_CAPACITY); the temperature as in mzh_search.
 * Refused on the device: a net_index that decreases or has an entry outside [0, n_networks) -- no root is
 * searched, no output of args is written, and status[0] = 1. */
typedef struct mzh_multi_args {
  int32_t n_networks;        /* M of the loaded set this call may index */
  const int32_t* net_index;  /* [B] device: network of root b, non-decreasing, each in [0, M) */
  int32_t* status;           /* [2] device, nullable: [0] 0 = searched, 1 = net_index refused; [1] tiles launched */
} mzh_multi_args;
int mzh_search_multi(mzh_engine* eng, const mzh_search_args* args, const mzh_multi_args* multi, mzh_stream stream);

/* mzh_search_multi with a simulation budget per root: root b runs budget->n_sims[b] simulations under network
 * net_index[b], with the result mzh_search_multi gives that root in a launch of n_sims[b] simulations on the same
 * inputs (bit for bit: the acting scripts' loop over n_mcts_simulations_range as one batch).  args.n_sims is the
 * launch's maximum: it sets the capacity check, the LDS, the length of pow_table (n_sims + 1) and the row stride
 * of args.latent (n_sims + 1; a root's row holds its latent_len entries, then -1).  Every budget lies in
 * [0, args.n_sims].
 * A run is a maximal stretch of consecutive roots with equal (net_index, n_sims).  net_index stays non-decreasing;
 * inside a network the budgets may come in any order, and equal budgets need not be adjacent -- they only make
 * more runs.  The prologue cuts at every run's end, so a tile holds up to 16 or 32 roots of one run, and lists the
 * tiles by decreasing budget (tiles of one budget in no fixed order; no result depends on a tile's place).  The
 * caller states max_runs >= the number of runs: the grid is ceil(B / tile) + min(max_runs, B) - 1 workgroups, and
 * args.lockstep_levels (indexed by tile) needs that many entries.
 * Flags, and every refusal of mzh_search_multi, are that call's.  Also refused before anything is launched, and
 * before an engine or a device is needed: a NULL args, multi, budget or n_sims, max_runs < 1 (MZH_ERR_ARG); with
 * the engine: a max_runs whose grid exceeds the engine's tile workspace (MZH_ERR_CAPACITY).
 * Refused on the device as a bad net_index is -- no root is searched, no output of args is written, status[0] = 1:
 * a budget outside [0, args.n_sims], more runs than max_runs, more tiles than the tile workspace holds. */
typedef struct mzh_budget_args {
  const int32_t* n_sims; /* [B] device: simulations of root b, each in [0, args.n_sims] */
  int32_t max_runs;      /* >= the runs of (net_index, n_sims): sizes the grid */
} mzh_budget_args;
int mzh_search_multi_budget(mzh_engine* eng, const mzh_search_args* args, const mzh_multi_args* multi,
                            const mzh_budget_args* budget, mzh_stream stream);

/* Action probe (acting_experiments/legal_illegal_preds.py evaluate_network, lines 26-80): what the model
 * predicts for each of the six moves from a state -- h = represent(obs) (networks.py:71-94), then
 * recurrent_inference(h, one_hot(a)) for a = 0..5 (networks.py:96-138) -- which the script files under legal or
 * illegal by env._move_allowed (env/hanoi.py:117-139).  One launch for n rows of a sub-batch: row j is env
 * env_index[j] of the full batch of B envs (env j where env_index is NULL; the indices of one call must be
 * distinct).  A workgroup keeps its 16 or 32 root latents in LDS across the six lookaheads; each row's outputs
 * are bit-identical to mzh_initial_inference followed by mzh_recurrent_inference on that row.  Every array
 * but env_index (and multi's net_index) is indexed by env; rows outside the call are left untouched.
 * With `multi`: row j is probed under network net_index[j] of the set loaded by mzh_load_weight_set
 * (non-decreasing over the rows), with the result this call gives on an engine holding that network alone;
 * the tile table is made by this call (two launches, as mzh_search_multi), on a grid of
 * ceil(n / tile) + min(n_networks, n) - 1 workgroups.
 * MZH_ERR_ARG, before any launch and before a device or an engine is needed: a NULL required pointer (args,
 * obs, reward, value; state where legal is given), n < 1, B < 1 (B < n without env_index), a flag other than
 * MZH_FLAG_COOP_TILE16 / 32 (default tile: 16 rows while n <= 4096, else 32); with multi a NULL net_index or
 * n_networks outside [1, 256]; then a NULL engine, and n_networks above the loaded set's M.
 * MZH_ERR_STATE: weights not loaded (without multi), no set loaded (with multi).  MZH_ERR_CAPACITY: n > max_roots.
 * On the device: a row whose env index is outside [0, B) is skipped and adds 1 to *err_count; a refused
 * net_index writes nothing and sets multi->status[0] = 1, as in mzh_search_multi. */
typedef struct mzh_probe_args {
  int32_t B;                /* envs of the full batch */
  int32_t n;                /* rows of this call */
  uint32_t flags;           /* MZH_FLAG_COOP_TILE16 / 32 only */
  const int32_t* env_index; /* [n] or NULL: row j is env env_index[j] (distinct), else env j */
  const float* obs;         /* [B][3 n_disks], indexed by env */
  const uint8_t* state;     /* [B][n_disks] nullable: c_state, for `legal` */
  float* reward;            /* [B][6] indexed by env: recurrent_inference(represent(obs), a)'s reward */
  float* value;             /* [B][6] */
  uint8_t* legal;           /* [B] nullable (needs state): bit a = move a allowed, as mzh_legal_mask */
  float* h0;                /* [B][64]   nullable: root latent                 */
  float* pi0;               /* [B][6]    nullable: root policy                 */
  float* value0;            /* [B]       nullable: root value                  */
  float* h1;                /* [B][6][64] nullable: the six next latents       */
  float* pi1;               /* [B][6][6]  nullable                             */
  int32_t* err_count;       /* nullable: += 1 per row whose env_index is outside [0, B); the row is skipped */
} mzh_probe_args;
int mzh_probe_actions(mzh_engine* eng, const mzh_probe_args* args, const mzh_multi_args* multi /* nullable */,
                      mzh_stream stream);

/* Input saliency (monosemanticity_analysis/gradient_analysis.py compute_saliency, lines 354-391): per row
 * d(policy logit k)/d(obs) and d(value)/d(obs) through represent + prediction (networks.py:71-94), in one
 * launch (mzh_saliency_kernel; with `multi` mzh_saliency_multi_kernel).  k is logit_index[env] where that is
 * given and >= 0, else the lowest index of the row's largest fp32 policy logit.  The forward is
 * mzh_initial_inference's (h0 / pi0 / value0 are bit-identical to it); the backward runs the six layers
 * transposed as fp32 MFMA products, the ReLU masks of the forward's hidden tiles, normalize_h_state's backward
 * with its min and max differentiable (lowest index on a tie) and, for a 33-bin value head, the softmax
 * expectation and the signed parabolic transform as autograd differentiates them.  A row's outputs depend on
 * that row and its network alone: the same bits in any position, at either tile size, with or without
 * env_index, single network or set.  Rows, env_index, `multi`, the tile table and the grid are
 * mzh_probe_actions'; every array but env_index (and multi's net_index) is indexed by env, rows outside the
 * call are left untouched.
 * MZH_ERR_ARG, before any launch and before a device or an engine is needed: a NULL required pointer (args,
 * obs, sal_policy, sal_value), n < 1, B < 1 (B < n without env_index), a flag other than
 * MZH_FLAG_COOP_TILE16 / 32 (default tile: 16 rows while n <= 4096, else 32); with multi a NULL net_index or
 * n_networks outside [1, 256]; then a NULL engine, and n_networks above the loaded set's M.
 * MZH_ERR_STATE: weights not loaded (without multi), no set loaded (with multi).  MZH_ERR_CAPACITY: n > max_roots.
 * On the device: a row whose env index is outside [0, B), or whose logit_index entry is outside [-1, 6), is
 * skipped and adds 1 to *err_count; a refused net_index writes nothing and sets multi->status[0] = 1. */
typedef struct mzh_saliency_args {
  int32_t B;                  /* envs of the full batch */
  int32_t n;                  /* rows of this call */
  uint32_t flags;             /* MZH_FLAG_COOP_TILE16 / 32 only */
  const int32_t* env_index;   /* [n] or NULL: row j is env env_index[j] (distinct), else env j */
  const float* obs;           /* [B][3 n_disks], indexed by env */
  const int32_t* logit_index; /* [B] nullable: the policy logit differentiated, -1 = the row's argmax */
  float* sal_policy;          /* [B][3 n_disks] d(policy logit k)/d(obs) */
  float* sal_value;           /* [B][3 n_disks] d(value)/d(obs) */
  int32_t* picked;            /* [B] nullable: k */
  float* disc_policy;         /* [B][n_disks] nullable: (|s0| + |s1|) + |s2| of each disc's three elements */
  float* disc_value;          /* [B][n_disks] nullable */
  float* h0;                  /* [B][64] nullable: root latent */
  float* pi0;                 /* [B][6]  nullable: root policy */
  float* value0;              /* [B]     nullable: root value  */
  int32_t* err_count;         /* nullable: += 1 per skipped row */
} mzh_saliency_args;
int mzh_saliency(mzh_engine* eng, const mzh_saliency_args* args, const mzh_multi_args* multi /* nullable */,
                 mzh_stream stream);

/* Parameter gradients of the five sub-networks (monosemanticity_analysis/gradient_analysis.py get_results, lines
 * 274-338): per row, for each of representation, dynamic, reward, policy and value (this order everywhere), the
 * gradient of one scalar of that sub-network's output with respect to that sub-network's own parameters, in one
 * launch (mzh_pgrad_kernel; with `multi` mzh_pgrad_multi_kernel).  With x = obs, a = one_hot(action):
 *   representation  z0 = rep(x), h0 = normalize(z0)           objective h0.mean()
 *   dynamic         z1 = dyn(cat(h0, a)), h1 = normalize(z1)  objective h1.mean()
 *   reward          lr = rwd(z1) (the raw z1, networks.py:131-132); objective the transformed scalar (33 bins) or lr
 *   policy          lp = pol(h0); objective softmax(lp).mean() where policy_logit[env] is -1 or the array is NULL
 *                   (the reference's: mathematically constant, its gradient is autograd's rounding noise
 *                   p_i (1/6 - sum_j p_j / 6)), else the logit policy_logit[env] (compute_saliency's objective)
 *   value           lv = val(h0); objective the transformed scalar (33 bins) or lv
 * Each net is Linear0 -> ReLU -> Linear2, and every weight gradient of one row is rank one, so the outputs are
 * the factors: delta2 = d objective / d (Linear2 output) (= the b2 gradient), act = relu(Linear0(in)),
 * delta1 = (delta2 . W2) * [act > 0] (= the b0 gradient); grad W2 = delta2 (x) act, grad W0 = delta1 (x) in with
 * in = x, cat(h0, a), z1, h0, h0.  The seeds of representation and dynamic are normalize_h_state's backward of a
 * constant 1/64 (min and max differentiable, lowest index on a tie), those of reward and value the softmax
 * expectation and signed parabolic transform as autograd differentiates them (1 for a scalar head).  With `grad`
 * a second launch on the same stream (mzh_pgrad_expand_kernel) writes row j's dense gradients in the layout of
 * mzh_weights_size: each weight element the single fp32 product delta[i] * in[j], each bias a copy.
 * The forward is the inference calls': h0 / pi0 / value0 are bit-identical to mzh_initial_inference, h1 / reward
 * to mzh_recurrent_inference(h0, action).  The backward runs Linear2 transposed as fp32 MFMA products; there is
 * no bit contract on its summation order, but a row's outputs depend on that row and its network alone: the same
 * bits in any position, at either tile size, with or without env_index, single network or set.  Rows, env_index,
 * `multi`, the tile table and the grid are mzh_probe_actions'; every array but env_index, grad (and multi's
 * net_index) is indexed by env, rows outside the call are left untouched.  The first call after a weight load
 * gathers dynamic_net.2 and rwd_net.2 transposed from the loaded blob into a buffer of the engine's (one more
 * launch on `stream`).
 * MZH_ERR_ARG, before any launch and before a device or an engine is needed: a NULL required pointer (args,
 * obs, action, delta1, delta2, act, h0, z1), n < 1, B < 1 (B < n without env_index), a flag other than
 * MZH_FLAG_COOP_TILE16 / 32 (default tile: 16 rows while n <= 4096, else 32); with multi a NULL net_index or
 * n_networks outside [1, 256]; then a NULL engine, and n_networks above the loaded set's M.
 * MZH_ERR_STATE: weights not loaded (without multi), no set loaded (with multi).  MZH_ERR_CAPACITY: n > max_roots.
 * On the device: a row whose env index is outside [0, B), whose action is outside [0, 6) or whose policy_logit
 * entry is outside [-1, 6) is skipped (its grad row too) and adds 1 to *err_count; a refused net_index writes
 * nothing and sets multi->status[0] = 1. */
typedef struct mzh_pgrad_args {
  int32_t B;                   /* envs of the full batch */
  int32_t n;                   /* rows of this call */
  uint32_t flags;              /* MZH_FLAG_COOP_TILE16 / 32 only */
  const int32_t* env_index;    /* [n] or NULL: row j is env env_index[j] (distinct), else env j */
  const float* obs;            /* [B][3 n_disks], indexed by env */
  const int32_t* action;       /* [B] 0..5, indexed by env */
  const int32_t* policy_logit; /* [B] nullable: -1 the reference's mean(softmax), k the logit k */
  float* delta1;               /* [B][5][256] d objective / d Linear0 output (= the b0 gradients) */
  float* delta2;               /* [B][5][64]  d objective / d Linear2 output: 64 / 64 / S / 6 / S entries, the rest +0 */
  float* act;                  /* [B][5][256] hidden activations after the ReLU */
  float* h0;                   /* [B][64] normalised root latent */
  float* z1;                   /* [B][64] raw (un-normalised) dynamics output, the reward net's input */
  float* h1;                   /* [B][64] nullable: normalised next latent */
  float* pi0;                  /* [B][6]  nullable: root policy */
  float* value0;               /* [B]     nullable: root value  */
  float* reward;               /* [B]     nullable */
  float* objective;            /* [B][5]  nullable: the five scalars */
  float* grad;                 /* [n][n_floats] nullable, by ROW of the call: the dense gradients */
  int32_t* err_count;          /* nullable: += 1 per skipped row */
} mzh_pgrad_args;
int mzh_param_grads(mzh_engine* eng, const mzh_pgrad_args* args, const mzh_multi_args* multi /* nullable */,
                    mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Reference-order host pre-draw (HOST pointers only; no device, no engine).  Replaces the NumPy
 * calls B sequential run_mcts calls make on the global legacy stream, in their order per call:
 *   np.random.dirichlet(np.ones_like(prob) * alpha)   MCTS/mcts.py:57-66,148-149  (k > 0)
 *   np.random.choice(<n_tie tied indices>)            MCTS/node.py:86             (n_tie > 1 draws)
 *   np.random.choice(np.arange(6), p=pi)              MCTS/mcts.py:118-120        (draw_action: the
 *                                                     one random_sample() it consumes)
 * NumPy's legacy RandomState algorithms (csrc/mzh_rng.cpp) on NumPy's own MT19937 state:
 *   mt_state    in/out  numpy mt19937_state {uint32 key[624]; int pos} (the bit generator's
 *                       ctypes.state_address), advanced in place exactly as NumPy would
 *   gauss_state in/out  {has_gauss, cached deviate} of the RandomState (read only for alpha > 1)
 *   alpha [k]           Dirichlet parameters as float64 (each > 0, else MZH_ERR_ARG as NumPy's
 *                       ValueError('alpha <= 0'))
 *   noise [B][k], tie [B] (index into the tied set), action_u [B]: outputs.
 * MZH_ERR_ARG for a bad argument, before anything is drawn. */
int mzh_rng_predraw(void* mt_state, double* gauss_state, int B, int k, const double* alpha, int n_tie,
                    int draw_action, double* noise, int32_t* tie, double* action_u);

/* ---------------------------------------------------------------------------------------------
 * Fused training update.  Replaces Muzero._update (Muzero.py:209-274: represent, U unrolled
 * prediction/dynamics steps, MSE value/reward and soft-target cross-entropy policy terms, the 0.5
 * latent-gradient hook, importance weights, the 1/U loss hook) and MuZeroNet.update's Adam step
 * (networks.py:69,118-122) for one sampled batch, in two kernel launches.
 *   B, U, in_dim, support : batch_s, unroll_n_steps, 3N, 33 (TD_return) or 1
 *   rows                  : transitions per workgroup of the row kernel (1 or 2; 0 = auto)
 *   step_size, bc2_sqrt   : torch.optim.Adam's lr / (1 - beta1^step) and sqrt(1 - beta2^step) for
 *                           this step (computed by the host in fp64, as torch does); beta1, beta2, eps
 *   obs [B][in_dim] f32, rwds [B][U] f32, actions [B][U] i64, pi [B][U][6] f32, returns [B][U] f32,
 *   weights [B] f32 importance weights or NULL (uniform replay)
 *   param / exp_avg / exp_avg_sq : the 20 MuZeroNet parameters in state_dict order
 *                           ({representation,dynamic,rwd,policy,value}_net.{0,2}.{weight,bias}) and
 *                           their Adam moments, updated in place
 *   wt[10]                : transposed copies [in][round_up(out, 4)] of the ten weights (param
 *                           0,2,...,18; pad columns zero), filled by mzh_train_transpose and kept
 *                           current by mzh_train_update
 *   scratch               : device workspace of mzh_train_scratch_bytes
 *   row_loss [B][3]       : per-transition value, reward and policy loss sums (their means are the
 *                           reference's returned losses); new_prio [B] = |v_0 - return_0| or NULL
 * ------------------------------------------------------------------------------------------- */
typedef struct mzh_train_args {
  int32_t B, U, in_dim, support, rows;
  float step_size, bc2_sqrt, beta1, beta2, eps;
  const float* obs;
  const float* rwds;
  const int64_t* actions;
  const float* pi;
  const float* returns;
  const float* weights;
  float* param[20];
  float* exp_avg[20];
  float* exp_avg_sq[20];
  float* wt[10];
  void* scratch;
  size_t scratch_bytes;
  float* row_loss;
  float* new_prio;
} mzh_train_args;

int mzh_train_scratch_bytes(int B, int U, int in_dim, int support, size_t* bytes);
int mzh_train_transpose(const mzh_train_args* args, mzh_stream stream);
int mzh_train_update(const mzh_train_args* args, mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Prioritised replay with the priorities resident in HBM, for the reference Buffer's defaults
 * (priority_exponent 1, importance_sampling_exponent 0: Muzero.py:72-78, buffer.py:13-14).
 *
 * mzh_replay_sample replaces Buffer.priority_sample's draw and batch (buffer.py:89-112): P = p / np.sum(p)
 * in float32, np.random.choice(np.arange(n), m, replace=True, p=P) from the uniforms u as RandomState
 * computes it (float64 cdf, cdf /= cdf[-1], searchsorted(u, side='right')), then the sampled rows.  The
 * indices equal NumPy's for the same u (np.random.random_sample(m), drawn by the caller).  One workgroup.
 *   n, m             : len(buffer) and batch_s (n >= 1, m >= 1)
 *   d_state, U, A    : row widths of the five transition arrays (states [.][d_state], rwds / returns
 *                      [.][U], actions int64 [.][U], pi [.][U][A])
 *   prio [n]         : device priorities (16-byte aligned)
 *   u [m]            : uniforms, device-readable (device or mapped page-locked memory)
 *   cdf [n]          : float64 workspace (the kernel keeps the cdf at every 4th element)
 *   indx [m]         : sampled indices (out)
 *   out_* [m][.]     : the sampled rows (out)
 *   status [2]       : device-written (out): [0] 0 = drawn, 1 = P has a NaN or negative entry (NumPy
 *                      raises ValueError there; indices and rows are then 0 / row 0); [1] 1 = the cdf
 *                      came from the exact parallel scan, 0 = from the sequential chain
 * mzh_replay_set_priorities replaces Buffer.update_priorities (buffer.py:127-134): prio[indx[k]] = values[k]
 * for k = 0..m-1, the last of repeated indices winning as in NumPy's fancy assignment, unless the
 * reference's assertion (all values finite, one > 0) fails or an index is outside [0, size): then nothing
 * is written and status[0] = 1 (assertion) / 2 (index), else 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct mzh_replay_args {
  int32_t n, m, d_state, U, A;
  const float* prio;
  const double* u;
  double* cdf;
  const float* states;
  const float* rwds;
  const int64_t* actions;
  const float* pi;
  const float* returns;
  int64_t* indx;
  float* out_states;
  float* out_rwds;
  int64_t* out_actions;
  float* out_pi;
  float* out_returns;
  int32_t* status;
} mzh_replay_args;

int mzh_replay_sample(const mzh_replay_args* args, mzh_stream stream);
int mzh_replay_set_priorities(float* prio, int64_t size, const int64_t* indx, const float* values, int m,
                              int32_t* status, mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * One update round of a set of M networks: for every active network m, what mzh_replay_sample (draw[m]) +
 * mzh_train_update (train[m]) + mzh_replay_set_priorities (prio, size of the ring, indx, train[m].new_prio) do
 * one after the other, as FOUR launches for the whole set -- the draws (grid M), the row kernel (grid rows x M),
 * the gradient / Adam kernel (grid tiles x M), the write-backs (grid M).  Every network ends bit for bit as its
 * three lone calls end: the kernels are the lone calls' own bodies with their arguments read from a table.
 *
 * mzh_train_set_create copies the shapes and uploads the table of the 2 M argument blocks once; EVERY pointer in
 * them is fixed for the handle's life: parameters, moments, wt, scratch, row_loss, new_prio, the ring arrays,
 * prio, cdf, indx and the draw's out_* buffers, which must be the very buffers train[m] names as obs / rwds /
 * actions / pi / returns (a network's draw feeds its own update).  beta1, beta2 and eps are taken per network at
 * creation; the per-call fields train[m].step_size / bc2_sqrt and draw[m].u / status are ignored, and draw[m].n
 * is here the ring's SIZE (the length of prio and cdf, Buffer.size): the write-back's index bound and the upper
 * bound of every round's n.
 * MZH_ERR_ARG, before the device is touched: a NULL train, draw or out; M outside
 * [1, MZH_TRAIN_SET_MAX]; networks that differ in B, U, in_dim, support or rows; draw[m].m != B,
 * draw[m].d_state != in_dim, draw[m].U != U, draw[m].A != 6; an out_* pointer that is not the matching train
 * input; a NULL new_prio; whatever mzh_train_update refuses of train[m] and mzh_replay_sample of draw[m] (u and
 * status apart).  The message names the field and the network.
 *
 * mzh_train_set_update makes one round.  All three arrays are read (status: written) by the KERNELS WHEN THEY RUN,
 * not at call time, so they must be device-readable and stay unchanged until the stream has passed the call:
 *   step [M]      : per network {active, n = len(buffer), step_size, bc2_sqrt of this Adam step}.  The host reads
 *                   active and n at call time as well (to launch nothing for a round without an active network,
 *                   and to refuse an active n outside [1, ring size] with MZH_ERR_ARG), so this pointer must be
 *                   valid on both sides: mapped page-locked memory, whose host and device addresses coincide.
 *   u [M][B]      : the draws' uniforms (np.random.random_sample(B) per network), device-readable
 *   status [M][4] : device-written (out), row m only if network m is active: [0] the draw's status, [1] its
 *                   exact-scan flag, [2] the write-back's status (mzh_replay_sample / _set_priorities), [3] 0
 * A network with step[m].active == 0 is skipped by all four kernels: nothing of it is read or written, its
 * status row included.  MZH_ERR_ARG for a NULL step, u, status or set.  With no active network the call launches
 * nothing and returns MZH_OK; otherwise exactly four launches on the stream, no synchronisation.
 * mzh_train_transpose stays per network (needed only after parameters were written from outside).
 * ------------------------------------------------------------------------------------------- */
#define MZH_TRAIN_SET_MAX 256
typedef struct mzh_train_set_step {
  int32_t active, n;
  float step_size, bc2_sqrt;
} mzh_train_set_step;
typedef struct mzh_train_set mzh_train_set;

int mzh_train_set_create(const mzh_train_args* train, const mzh_replay_args* draw, int M, mzh_train_set** out);
int mzh_train_set_destroy(mzh_train_set* set);
int mzh_train_set_update(mzh_train_set* set, const mzh_train_set_step* step, const double* u, int32_t* status,
                         mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Episode ingest: the record of one batched lockstep self-play run (BatchedSelfPlay.play with
 * record_obs, T recorded steps of B envs) into the replay ring, for TD_return=True.  Replaces, per
 * episode, compute_n_step_returns (utils.py:28-69), the priorities |return - root Q| in float32
 * (Muzero.py:188-205), organise_transitions (Muzero.py:276-323), the filter of the training loop (only
 * episodes whose last return is > 0 enter, Muzero.py:98) and Buffer.add (buffer.py:62-77), with the same
 * bits as that host path.  Two launches: a one-workgroup filter + scan over the envs, then one workgroup
 * per entering episode writing its rows.
 *   B, T, d_state, U, A : envs, recorded steps, observation width, unroll_n_steps, actions
 *   n_step              : n_TD_step
 *   size, ptr           : the ring's capacity in rows and Buffer.ptr before the call (0 <= ptr < size)
 *   obs [T][B][d_state] f32, action [T][B] i32, reward [T][B] f64, pi [T][B][A] f64, root_q [T][B] f64,
 *   steps [B] i32       : the record; env b played steps[b] in [1, T] steps, and what the record holds at
 *                         t >= steps[b] is never used
 *   pad_action [B] i64  : organise_transitions' np.random.randint(0, n_action) of each episode (drawn by
 *                         the caller for every env, entering or not, as the host path draws them)
 *   disc_pow [n_step+1] f64 : discount**i as the caller's Python computes it
 *   states [size][d_state] f32, rwds [size][U] f32, actions [size][U] i64, pi_probs [size][U][A] f32,
 *   returns [size][U] f32, prio [size] f32 : the ring (in/out)
 *   first [B] i64       : workspace (an entering episode's position in the sequential row order, else -1)
 *   status [2] i64      : device-written (out): [1] = G, the rows of the entering episodes in env order;
 *                         row g of them lands at (ptr + g) % size, and rows g < G - size are not written
 *                         (a later row of the same call overwrites them in the sequential order);
 *                         [0] = 0 written, 1 = an entering episode is longer than the ring (the
 *                         reference's assert n <= size), 2 = a steps[b] outside [1, T]: nothing written
 * The caller advances ptr by G modulo size after reading status.
 * ------------------------------------------------------------------------------------------- */
typedef struct mzh_ingest_args {
  int32_t B, T, d_state, U, A, n_step;
  int64_t size, ptr;
  const float* obs;
  const int32_t* action;
  const double* reward;
  const double* pi;
  const double* root_q;
  const int32_t* steps;
  const int64_t* pad_action;
  const double* disc_pow;
  float* states;
  float* rwds;
  int64_t* actions;
  float* pi_probs;
  float* returns;
  float* prio;
  int64_t* first;
  int64_t* status;
} mzh_ingest_args;

int mzh_episode_ingest(const mzh_ingest_args* args, mzh_stream stream);

/* ---------------------------------------------------------------------------------------------
 * Whole self-play episodes in one launch on the latency kernel (the episode form of mzh_search_one_kernel, mzh_one.hip: 512
 * threads, min(B, 256) workgroups, a workgroup plays env blockIdx.x, blockIdx.x + gridDim.x, ...).  Env b
 * starts from state[b] with step_counter 0 and plays moves t = 0, 1, ... until it is done (the goal, or
 * max_steps moves; Muzero._play_game's loop, Muzero.py:153-186).  Move t of env b:
 *   obs     oneHot_encoding(c_state) (utils.py:9-25), the float32 values of mzh_encode_obs;
 *   search  one MCTS.run_mcts (mcts.py:34-126) from it, as mzh_search runs it on the latency kernel, with the
 *           inputs of row t * B + b of noise / tie_idx / action_u and the agent's MinMaxStats: minmax_in[b]
 *           (fresh where NULL) at t = 0, then carried from search to search on the device as a caller would
 *           pass minmax_out on as minmax_in; pi, root_q, action (visits, obs) of row t * B + b are written;
 *   step    one TowersOfHanoi.step (env/hanoi.py:47-84) on the chosen action, as mzh_env_step: its reward
 *           code goes to reward[t * B + b].
 * Rows t >= steps[b] of every [T][B] array are neither read nor written.  At an episode's end steps[b] (moves
 * played), illegal[b] (illegal moves among them), solved[b] (1: a step returned reward 100), final_state[b]
 * (c_state: not advanced by the goal step, hanoi.py:65-69) and minmax_out[b] are written.
 * T >= max_steps is required, so every env ends inside the tables.  A start state with a peg outside 0..2 is
 * refused on the device: that env plays nothing (steps = illegal = solved = 0, final_state = state, minmax_out
 * = minmax_in or fresh) and *err_count += 1.
 * Refused before any launch -- MZH_ERR_ARG: args NULL, a NULL required pointer (state, tie_idx, pi, root_q,
 * action, reward, steps, illegal, solved, final_state, minmax_out; action_u unless deterministic), B < 1,
 * n_sims < 0, max_steps < 1, T < max_steps, T * B rows beyond int32, goal_peg outside 0..2, a flag other than
 * MZH_FLAG_NP1_UCB, engine NULL; MZH_ERR_TEMPERATURE as mzh_search; MZH_ERR_CAPACITY: B > max_roots, n_sims >
 * max_sims, or n_sims beyond the latency kernel's LDS (the MZH_FLAG_KERNEL_ONE rule); MZH_ERR_STATE: weights
 * not loaded.  The checks that need no engine come first.  Replay has no episode form; a weight set plays through
 * mzh_play_episodes_multi below.
 * ------------------------------------------------------------------------------------------- */
typedef struct mzh_episode_args {
  int32_t B;             /* envs */
  int32_t T;             /* rows (moves) of the [T][B] tables, >= max_steps */
  int32_t n_sims;        /* n_simulations (mcts.py:30) */
  int32_t goal_peg;      /* TowersOfHanoi(N, max_steps): N is the engine's n_disks */
  int32_t max_steps;
  int32_t deterministic; /* as mzh_search_args */
  uint32_t flags;        /* 0 or MZH_FLAG_NP1_UCB */
  double discount, eps, temperature; /* as mzh_search_args */
  const uint8_t* state;     /* [B][n_disks] start states (peg of disc d) */
  const double* noise;      /* [T][B][6] Dirichlet draws, NULL = no noise */
  const int32_t* tie_idx;   /* [T][B] */
  const double* action_u;   /* [T][B]; NULL if deterministic */
  const double* minmax_in;  /* [B][2] (maximum, minimum) or NULL (fresh) */
  const double* pow_table;  /* as mzh_search_args (nullable) */
  double* pi;           /* [T][B][6] */
  double* root_q;       /* [T][B] */
  int32_t* action;      /* [T][B] */
  int8_t* reward;       /* [T][B] codes of mzh_env_step */
  int32_t* visits;      /* [T][B][6] nullable */
  float* obs;           /* [T][B][3 n_disks] nullable: the observation searched */
  int32_t* steps;       /* [B] */
  int32_t* illegal;     /* [B] */
  uint8_t* solved;      /* [B] */
  uint8_t* final_state; /* [B][n_disks] */
  double* minmax_out;   /* [B][2] */
  int32_t* err_count;   /* nullable device int32 accumulator */
} mzh_episode_args;

int mzh_play_episodes(mzh_engine* eng, const mzh_episode_args* args, mzh_stream stream);

/* Episodes of several networks in one launch: env b plays its whole episode under network net_index[b] of the
 * set loaded by mzh_load_weight_set (or refreshed by mzh_load_weight_set_device), with the result
 * mzh_play_episodes gives on an engine holding that network alone, bit for bit, from the same start state, the same
 * rows of the [T][B] tables (column b) and the same minmax_in[b].  `args` is mzh_play_episodes', unchanged; `multi`
 * is mzh_search_multi's with its contract: net_index [B] on the device, non-decreasing, each entry in
 * [0, n_networks); a network without envs is fine.  Two launches: the one-workgroup prologue of the other multi
 * calls checks net_index on the device, then the set form of the episode kernel plays env blockIdx.x,
 * blockIdx.x + gridDim.x, ... on min(B, 256) workgroups, each holding the hidden layers' rows (registers) and the
 * output layers (LDS) of its env's network and loading another network's only where its next env has one (B > 256).
 * The engine's single network is neither needed nor touched.
 * Refused before any launch: everything mzh_play_episodes refuses before it uses the engine, in its order; then
 * multi NULL, net_index NULL, n_networks outside [1, 256] (MZH_ERR_ARG), all of these without an engine; then engine
 * NULL and the capacity errors of mzh_play_episodes; no set loaded (MZH_ERR_STATE); n_networks above the M of the
 * loaded set (MZH_ERR_ARG).
 * Refused on the device: a net_index that decreases or has an entry outside [0, n_networks) -- no env plays, no
 * output of args is written (err_count included), and status[0] = 1.  Otherwise status[0] = 0 and status[1] is the
 * number of networks that have envs. */
int mzh_play_episodes_multi(mzh_engine* eng, const mzh_episode_args* args, const mzh_multi_args* multi,
                            mzh_stream stream);

/* Episodes of agents of different configurations in one launch: mzh_play_episodes_multi with env b running
 * sweep->n_sims[b] simulations per move under sweep->discount[b].  Env b plays bit for bit as mzh_play_episodes plays
 * it on an engine holding network net_index[b] alone with args.n_sims = n_sims[b] and args.discount = discount[b],
 * from the same start state, the same column b of the [T][B] tables and the same minmax_in[b].  `args` and `multi`
 * are mzh_play_episodes_multi's with that call's contract (a lone network is a set of one); args.n_sims is the
 * launch's maximum: it decides the capacity check, the LDS plan (whether the latents sit in LDS) and the length of
 * pow_table (n_sims + 1 entries), none of which enters a result.  Two launches, as mzh_play_episodes_multi: the
 * prologue checks net_index and the budgets, then the sweep form of the episode kernel plays; a workgroup reads its
 * env's budget and discount once per env.
 * Refused before any launch: everything mzh_play_episodes_multi refuses without an engine, in its order; then sweep
 * NULL or sweep->n_sims NULL (MZH_ERR_ARG), still without an engine; then that call's remaining refusals in their
 * order, from engine NULL on.
 * Refused on the device, exactly as a bad net_index is (and a bad net_index still is): a budget outside
 * [0, args.n_sims] -- no env plays, no output of args is written (err_count included), and status[0] = 1. */
typedef struct mzh_episode_sweep_args {
  const int32_t* n_sims;   /* [B] device: simulations per move of env b, each in [0, args.n_sims] */
  const double* discount;  /* [B] device, nullable: NULL = args.discount for every env */
} mzh_episode_sweep_args;
int mzh_play_episodes_sweep(mzh_engine* eng, const mzh_episode_args* args, const mzh_multi_args* multi,
                            const mzh_episode_sweep_args* sweep, mzh_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MZH_ABI_H_ */
