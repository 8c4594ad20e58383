// mzh_api_memo.hip -- the wave kernel's expansion memo (mzh.h): its depth, build, drop and rebuild, the grown
// extension's miss log, and the memo's statistics and debug entry points.
#include <chrono>

#include "mzh_host.h"

// the depth a request gives: -1 the budget's, 0 off, d > 0 as asked (status: a forced table too large)
int memo_depth_for(int n_disks, int want, int* D) {
  if (want < -1 || want > MZH_MEMO_MAX_DEPTH)
    return fail(MZH_ERR_ARG, "memo depth must be -1 (automatic), 0 (off) or 1..%d, got %d", MZH_MEMO_MAX_DEPTH, want);
  if (n_disks < 1 || n_disks > 16) return fail(MZH_ERR_ARG, "n_disks must be in [1,16], got %d", n_disks);
  *D = want < 0 ? mzh_memo_auto_depth(n_disks) : want;
  if (mzh_memo_states(n_disks) * mzh_memo_nodes(*D) > MZH_MEMO_MAX_ROWS)
    return fail(MZH_ERR_CAPACITY, "memo depth %d at %d discs is %lld rows, more than %lld", *D, n_disks,
                mzh_memo_states(n_disks) * mzh_memo_nodes(*D), MZH_MEMO_MAX_ROWS);
  return MZH_OK;
}

extern "C" int mzh_memo_plan(int n_disks, int depth, int32_t* depth_out, int64_t* rows, int64_t* bytes) {
  int D = 0;
  const int st = memo_depth_for(n_disks, depth, &D);
  if (st) return st;
  const long long r = D > 0 ? mzh_memo_states(n_disks) * mzh_memo_nodes(D) : 0;
  if (depth_out) *depth_out = D;
  if (rows) *rows = r;
  if (bytes) *bytes = r * MZH_MEMO_ROW_BYTES;
  return MZH_OK;
}

extern "C" int mzh_set_memo_depth(mzh_engine* eng, int depth) {
  if (!eng) return fail(MZH_ERR_ARG, "engine NULL");
  int D = 0;
  const int st = memo_depth_for(eng->n_disks, depth, &D);
  if (st) return st;
  eng->memo.want = depth;
  eng->memo.auto_cap = MZH_MEMO_MAX_DEPTH;
  return MZH_OK;
}

// the depth the next wave search uses: the request's, the automatic one no deeper than a build's memory allowed
static int memo_effective_depth(const mzh_engine* eng, int* D) {
  const int st = memo_depth_for(eng->n_disks, eng->memo.want, D);
  if (st == MZH_OK && eng->memo.want < 0 && *D > eng->memo.auto_cap) *D = eng->memo.auto_cap;
  return st;
}

// the extension rows the engine's request gives beside `dense_rows` dense ones
static long long memo_grow_cap(const mzh_engine* eng, long long dense_rows) {
  return mzh_memo_grow_rows(eng->memo.grow_want < 0 ? MZH_MEMO_GROW_BUDGET_BYTES : eng->memo.grow_want, dense_rows);
}

// drop the expansion memo (after the device has finished with it)
hipError_t memo_drop(mzh_engine* eng) {
  auto& mo = eng->memo;
  if (!mo.h.get() && !mo.rec.get()) return hipSuccess;
  ++eng->n_wait;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  (void)mo.h.reset();
  (void)mo.rec.reset();
  (void)mo.link.reset();
  (void)mo.ctr.reset();
  mo.D = 0;
  mo.base = mo.cap = 0;
  return hipSuccess;
}

// Fill the table for the loaded weights at depth D, level by level with the inference kernels: the 3^N one-hot
// states through initial inference, then every (node, move) of the level above through recurrent inference.
// Within a level the rows are ordered (state, node): child row = 6 * parent row + move.  Runs on `stream` and
// waits for it (the temporaries are freed on return).
static int memo_fill(mzh_engine* eng, int D, hipStream_t stream, bool* oom) {
  auto& mo = eng->memo;
  const int N = eng->n_disks, in = eng->in_dim;
  const long long ST = mzh_memo_states(N), K = mzh_memo_nodes(D), rows = ST * K;
  const long long cap = memo_grow_cap(eng, rows);  // the grown extension's rows follow the dense ones
  long long top = ST;  // rows of the deepest level
  for (int d = 0; d < D; ++d) top *= 6;
  std::vector<float> obs((size_t)ST * in, 0.0f);
  for (long long s = 0; s < ST; ++s) {
    long long q = s;
    for (int i = 0; i < N; ++i, q /= 3) obs[(size_t)s * in + 3 * i + (int)(q % 3)] = 1.0f;
  }
  // temporaries: two natural-order latent levels (ping-pong), the level's expanded input, moves, heads
  DevBuf<float> dobs, hA, hB, xin, pi, rw, va;
  DevBuf<int32_t> act;
  hipError_t e = mo.h.alloc((size_t)(rows + cap) * MZH_LATENT);
  if (e == hipSuccess) e = mo.rec.alloc((size_t)(rows + cap) * 8);
  if (e == hipSuccess && cap > 0) e = mo.link.alloc((size_t)(rows + cap) * 6);
  if (e == hipSuccess && cap > 0) e = mo.ctr.alloc(2);
  if (e == hipSuccess) e = dobs.alloc(obs.size());
  if (e == hipSuccess) e = hA.alloc((size_t)top * MZH_LATENT);
  if (e == hipSuccess) e = hB.alloc((size_t)(top / 6 + 1) * MZH_LATENT);
  if (e == hipSuccess) e = xin.alloc((size_t)top * MZH_LATENT);
  if (e == hipSuccess) e = act.alloc((size_t)top);
  if (e == hipSuccess) e = pi.alloc((size_t)top * MZH_A);
  if (e == hipSuccess) e = rw.alloc((size_t)top);
  if (e == hipSuccess) e = va.alloc((size_t)top);
  if (e != hipSuccess) {
    *oom = e == hipErrorOutOfMemory;
    if (*oom) (void)hipGetLastError();  // the runtime's sticky copy of this error
    return hip_fail(e, "memo build: allocation");
  }
  e = hipMemcpyAsync(dobs.get(), obs.data(), dobs.bytes(), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemsetAsync(rw.get(), 0, (size_t)ST * sizeof(float), stream);  // a root has no reward
  if (e == hipSuccess && cap > 0) e = hipMemsetAsync(mo.link.get(), 0, mo.link.bytes(), stream);  // every link MZH_LINK_NONE
  if (e == hipSuccess && cap > 0) e = hipMemsetAsync(mo.ctr.get(), 0, mo.ctr.bytes(), stream);    // no row in use
  if (e != hipSuccess) return hip_fail(e, "memo build: upload");
  // the level's outputs go to hcur; levels alternate between hA and hB so that the deepest lands in hA
  float* hcur = (D % 2 == 0) ? hA.get() : hB.get();
  float* hprev = (D % 2 == 0) ? hB.get() : hA.get();
  long long n = ST, first = 0, per_state = 1;
  for (int d = 0; d <= D; ++d) {
    MzhInferParams p{};
    p.B = (int)n; p.in_dim = in; p.kin = eng->kin; p.h = hcur; p.pi = pi.get(); p.value = va.get();
    if (d == 0) {
      p.x = dobs.get();
    } else {
      e = mzh_launch_memo_level(hprev, xin.get(), act.get(), n, stream);
      if (e != hipSuccess) return hip_fail(e, "memo build: level input");
      p.x = xin.get(); p.action = act.get(); p.reward = rw.get();
    }
    e = mzh_launch_infer(pick_rows((int)n), d > 0, eng->single.net, p, stream);
    if (e == hipSuccess)
      e = mzh_launch_memo_scatter(hcur, pi.get(), rw.get(), va.get(), n, per_state, K, first, mo.h.get(), mo.rec.get(), stream);
    if (e != hipSuccess) return hip_fail(e, "memo build: level");
    first += per_state;
    per_state *= 6;
    n *= 6;
    float* t = hcur; hcur = hprev; hprev = t;
  }
  e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "memo build: run");
  mo.D = D;
  mo.base = rows;
  mo.cap = cap;
  return MZH_OK;
}

// the table anew at depth D; a fill that fails leaves no table
static int memo_build(mzh_engine* eng, int D, hipStream_t stream, bool* oom) {
  *oom = false;
  HIP_OK(memo_drop(eng));
  const auto t_start = std::chrono::steady_clock::now();
  const int st = memo_fill(eng, D, stream, oom);
  if (st) {
    (void)memo_drop(eng);
    return st;
  }
  // what the building search call paid: allocations, the fill, the wait and the frees, on the host's clock
  eng->memo.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  return MZH_OK;
}

// the memo of a wave MLP search: built on first use, rebuilt when the wanted depth changed.  A forced depth
// whose build fails is the call's error.  The automatic depth is an optimisation the caller did not ask for:
// when its table or the build's temporaries do not fit the device's free memory, the next shallower one is
// tried, down to no memo, and later searches keep that depth (mzh_set_memo_depth lifts the ceiling)
int memo_ensure(mzh_engine* eng, hipStream_t stream) {
  for (;;) {
    int D = 0;
    const int st = memo_effective_depth(eng, &D);
    if (st) return st;
    if (D == eng->memo.D && (D == 0 || eng->memo.cap == memo_grow_cap(eng, eng->memo.base))) return MZH_OK;
    if (D == 0) {
      HIP_OK(memo_drop(eng));
      return MZH_OK;
    }
    bool oom = false;
    const int bs = memo_build(eng, D, stream, &oom);
    if (bs == MZH_OK || eng->memo.want >= 0 || !oom) return bs;
    eng->memo.auto_cap = D - 1;
  }
}

// the per-root miss log of the grown extension: workspace for max_roots roots at the engine's log cap
int memo_log_ensure(mzh_engine* eng) {
  auto& mo = eng->memo;
  const size_t want = (size_t)eng->max_roots * mo.log_cap;
  if (mo.log.get() && mo.log.count() == want) return MZH_OK;
  if (want >= ((size_t)1 << 31))  // the kernel indexes entries in 32 bits
    return fail(MZH_ERR_CAPACITY, "memo miss log: %d roots x %d entries", eng->max_roots, mo.log_cap);
  if (mo.log.get()) {
    ++eng->n_wait;
    HIP_OK(hipDeviceSynchronize());
    (void)mo.log.reset();
  }
  HIP_OK(mo.log.alloc(want));
  if (!mo.logn.get()) {
    HIP_OK(mo.logn.alloc((size_t)eng->max_roots));
    HIP_OK(hipMemset(mo.logn.get(), 0, mo.logn.bytes()));
  }
  return MZH_OK;
}

extern "C" int mzh_set_memo_grow(mzh_engine* eng, int64_t budget_bytes, int32_t log_entries) {
  if (budget_bytes < -1 || budget_bytes > MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES)
    return fail(MZH_ERR_ARG, "memo growth budget must be -1 (default), 0 (off) or up to %lld bytes, got %lld",
                MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES, (long long)budget_bytes);
  if (log_entries < -1 || log_entries == 0 || log_entries > MZH_MEMO_LOG_CAP_MAX)
    return fail(MZH_ERR_ARG, "memo miss log entries per root must be -1 (default) or 1..%d, got %d",
                MZH_MEMO_LOG_CAP_MAX, (int)log_entries);
  if (!eng) return fail(MZH_ERR_ARG, "engine NULL");
  eng->memo.grow_want = budget_bytes;
  eng->memo.log_cap = log_entries < 0 ? MZH_MEMO_LOG_CAP : log_entries;
  return MZH_OK;
}

extern "C" int mzh_memo_grow_stats(mzh_engine* eng, mzh_memo_grow_info* out) {
  if (!eng || !out) return fail(MZH_ERR_ARG, "memo_grow_stats: engine or out NULL");
  memset(out, 0, sizeof(*out));
  out->budget_bytes = eng->memo.grow_want < 0 ? MZH_MEMO_GROW_BUDGET_BYTES : eng->memo.grow_want;
  out->log_entries = eng->memo.log_cap;
  out->capacity_rows = eng->memo.cap;
  if (eng->memo.cap == 0) return MZH_OK;
  MZH_ON_DEVICE(eng->device);
  int32_t c[2] = {0, 0};
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(c, eng->memo.ctr.get(), sizeof(c), hipMemcpyDeviceToHost));
  out->rows_used = c[0];
  out->rows_last_harvest = c[0] - c[1];
  return MZH_OK;
}

extern "C" int mzh_memo_debug_grow(mzh_engine* eng, float* latent, float* record, int32_t* link, int64_t* rows_used,
                                   int64_t* dense_rows, int64_t* capacity_rows) {
  if (!eng || !rows_used || !dense_rows || !capacity_rows) return fail(MZH_ERR_ARG, "memo_debug_grow: NULL argument");
  const auto& mo = eng->memo;
  *rows_used = 0;
  *dense_rows = mo.base;
  *capacity_rows = mo.cap;
  if (mo.cap == 0) return MZH_OK;
  MZH_ON_DEVICE(eng->device);
  int32_t used = 0;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&used, mo.ctr.get(), sizeof(used), hipMemcpyDeviceToHost));
  *rows_used = used;
  const size_t b = (size_t)mo.base, n = (size_t)mo.cap;
  if (latent) HIP_OK(hipMemcpy(latent, mo.h.get() + b * MZH_LATENT, n * MZH_LATENT * sizeof(float), hipMemcpyDeviceToDevice));
  if (record) HIP_OK(hipMemcpy(record, mo.rec.get() + b * 8, n * 8 * sizeof(float), hipMemcpyDeviceToDevice));
  if (link) HIP_OK(hipMemcpy(link, mo.link.get(), (b + n) * 6 * sizeof(int32_t), hipMemcpyDeviceToDevice));
  HIP_OK(hipDeviceSynchronize());
  return MZH_OK;
}

extern "C" int mzh_memo_stats(mzh_engine* eng, mzh_memo_info* out) {
  if (!eng || !out) return fail(MZH_ERR_ARG, "memo_stats: engine or out NULL");
  memset(out, 0, sizeof(*out));
  int D = 0;
  const int st = memo_effective_depth(eng, &D);
  if (st) return st;
  out->depth = D;
  out->built = (D > 0 && eng->memo.D == D) ? 1 : 0;
  out->rows = D > 0 ? mzh_memo_states(eng->n_disks) * mzh_memo_nodes(D) : 0;
  out->table_bytes = out->rows * MZH_MEMO_ROW_BYTES;
  out->build_ms = eng->memo.build_ms;
  MZH_ON_DEVICE(eng->device);
  unsigned long long c[3] = {0, 0, 0};
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(c, eng->memo.cnt.get(), sizeof(c), hipMemcpyDeviceToHost));
  out->pairs_skipped = c[0];
  out->pairs_packed = c[1];
  out->pairs_full = c[2];
  return MZH_OK;
}

extern "C" int mzh_memo_debug_table(mzh_engine* eng, float* latent, float* record, int64_t* rows, int32_t* depth) {
  if (!eng || !rows || !depth) return fail(MZH_ERR_ARG, "memo_debug_table: NULL argument");
  const long long n = eng->memo.D > 0 ? mzh_memo_states(eng->n_disks) * mzh_memo_nodes(eng->memo.D) : 0;
  *rows = n;
  *depth = eng->memo.D;
  if (n == 0 || (!latent && !record)) return MZH_OK;
  MZH_ON_DEVICE(eng->device);
  HIP_OK(hipDeviceSynchronize());
  if (latent) HIP_OK(hipMemcpy(latent, eng->memo.h.get(), (size_t)n * MZH_LATENT * sizeof(float), hipMemcpyDeviceToDevice));
  if (record) HIP_OK(hipMemcpy(record, eng->memo.rec.get(), (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToDevice));
  HIP_OK(hipDeviceSynchronize());
  return MZH_OK;
}
