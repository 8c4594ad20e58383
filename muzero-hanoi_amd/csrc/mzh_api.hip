// mzh_api.hip -- C ABI (include/mzh.h) over the gfx950 kernels.  No exceptions cross the ABI;
// every entry point returns a status and records a thread-local message.  The weight layouts are
// packed on the host by mzh_pack.cpp; mzh_load_weights uploads the blob and turns offsets into pointers.
#include <math.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/mzh.h"
#include "mzh_env_kernels.h"
#include "mzh_internal.h"
#include "mzh_train.h"

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static int hip_fail(hipError_t e, const char* what) {
  return fail(MZH_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

#define HIP_OK(expr)                                   \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
  } while (0)

static int memo_depth_for(int n_disks, int want, int* D);  // the expansion memo's depth of a request (below)

// RAII: run on the engine's device, restore the caller's current device afterwards
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

struct mzh_engine {
  int device = 0;
  int n_disks = 0, max_sims = 0, max_roots = 0, support = 33;
  int in_dim = 0, kin = 0, E = 0;
  void* wbuf = nullptr;
  bool loaded = false;
  MzhNet net{};
  MzhWNet wnet{};
  MzhOneNet onet{};
  unsigned char* tree = nullptr;
  float* htree = nullptr;
  uint16_t* pathx = nullptr;
  double* table = nullptr;
  // the network set of mzh_load_weight_set (its own allocation; the single-network calls never read it)
  void* setbuf = nullptr;      // [M] blobs at set_stride bytes, then [M][2] floats (MzhPackedSet)
  int set_m = 0;               // 0: no set loaded
  size_t set_stride = 0;
  MzhNet setnet{};             // network 0 of the set: the template mzh_search_multi_kernel offsets
  MzhOneNet setonet{};         // network 0's latency-kernel views: the set form of the episode kernel offsets them
  const float* set_scal = nullptr;
  MzhTile* mtiles = nullptr;   // tile table workspace of mzh_search_multi, allocated with the first set
  int32_t* mntiles = nullptr;
  // the wave kernel's expansion memo (mzh.h): built by the first wave search after a weight load
  int memo_want = -1;          // mzh_set_memo_depth: -1 automatic, 0 off, d > 0 forced
  int memo_auto_cap = MZH_MEMO_MAX_DEPTH;  // the automatic depth's ceiling: lowered when a build ran out of memory
  int memo_D = 0;              // depth of the built table (0: none)
  float* memo_h = nullptr;     // [rows][64]
  float* memo_rec = nullptr;   // [rows][8]
  unsigned long long* memo_cnt = nullptr;  // [3] device counters, zeroed by mzh_create
  double memo_build_ms = 0.0;
  // its grown extension (mzh_set_memo_grow): rows after the dense ones in memo_h / memo_rec, made and dropped
  // with them; the per-root miss log is workspace (made by the first search that logs, kept across loads)
  long long grow_want = -1;    // byte budget of the extension's rows: -1 the default, 0 off
  int log_cap = MZH_MEMO_LOG_CAP;
  long long memo_base = 0;     // dense rows of the built table
  long long memo_cap = 0;      // extension rows of the built table (0: none)
  int32_t* memo_link = nullptr;  // [memo_base + memo_cap][6]
  int32_t* memo_ctr = nullptr;   // [2] rows in use, in use before the last harvest
  uint4* memo_log = nullptr;     // [max_roots][memo_log_cap]
  int32_t* memo_logn = nullptr;  // [max_roots]
  int memo_log_cap = 0;          // what memo_log was allocated for
  // the transposed blobs of mzh_saliency (MzhPackedT; allocations of their own, uploaded with the weights they
  // are a function of and dropped with them)
  void* tbuf = nullptr;
  MzhSalNetT tnet{};
  void* settbuf = nullptr;
  MzhSalNetT settnet{};
  // dynamic_net.2 and rwd_net.2 transposed (MzhPackedG) for mzh_param_grads: gathered from the main blob(s) by
  // the first such call after a load of either kind (every load clears the valid flag); workspace, not a
  // weight buffer of the load calls (their debug counters do not count it)
  MzhPgradMap* gmaps = nullptr;    // host: the layout and the gather's source map
  int32_t* gmap = nullptr;         // device: the source map
  size_t gstride = 0;              // floats of one network's buffer (rounded up to 256 bytes)
  float* gbuf = nullptr;           // the single network's
  float* setgbuf = nullptr;        // [setg_m] at gstride
  int setg_m = 0;
  bool g_valid = false, setg_valid = false;
  // floats of wbuf / tbuf / setbuf (tail included) / settbuf (mzh_weights_debug_blob)
  size_t wn = 0, tn = 0, setn = 0, settn = 0;
  // the device repack (mzh_load_weights_device / mzh_load_weight_set_device): made by the first such call, kept
  MzhPackMaps* maps = nullptr;     // host: layouts and scalar sources of this engine's shape
  int32_t* rmap = nullptr;         // device: encoded main map [rstride], then the transposed one [rtstride]
  size_t rstride = 0, rtstride = 0;  // a blob rounded up to 256 bytes (the set strides), floats; -1 beyond the blob
  int32_t rscal[2] = {-1, -1};     // encoded sources of the two by-value scalars
  const float** ptab = nullptr;    // device [20]: the single network's parameter pointers
  std::vector<const float*> ptab_host;      // what ptab holds (uploaded again only when it differs)
  const float** set_ptab = nullptr;  // device [set_ptab_m][20]
  int set_ptab_m = 0;
  std::vector<const float*> set_ptab_host;
  float* scal2 = nullptr;          // device [2]: the single network's by-value scalars as the gather wrote them
  float* scal2_host = nullptr;     // pinned [2]: their read-back
  // weight buffer allocations, frees and device-wide waits of every load call (mzh_weights_debug_counters)
  uint64_t n_alloc = 0, n_free = 0, n_wait = 0;
};

extern "C" int mzh_abi_version(void) { return MZH_ABI_VERSION; }
extern "C" const char* mzh_last_error(void) { return g_err.c_str(); }

extern "C" int mzh_device_count(int* count) {
  if (!count) return fail(MZH_ERR_ARG, "count is NULL");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  return MZH_OK;
}

extern "C" int mzh_host_device_pointer(void* host, void** dev) {
  if (!host || !dev) return fail(MZH_ERR_ARG, "host_device_pointer: NULL argument");
  *dev = nullptr;
  hipError_t e = hipHostGetDevicePointer(dev, host, 0);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "hipHostGetDevicePointer");
}

extern "C" int mzh_stream_synchronize(void* stream) {
  hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  return e == hipSuccess ? MZH_OK : hip_fail(e, "hipStreamSynchronize");
}

extern "C" int mzh_weights_size(int n_disks, int support, size_t* n_floats) {
  if (n_disks < 1 || n_disks > 16 || (support != 33 && support != 1) || !n_floats)
    return fail(MZH_ERR_ARG, "bad n_disks=%d / support=%d", n_disks, support);
  *n_floats = mzh_canon_view(nullptr, 3 * n_disks, support).total;
  return MZH_OK;
}

extern "C" int mzh_create(int device, int n_disks, int max_sims, int max_roots, int support, mzh_engine** out) {
  if (!out) return fail(MZH_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (n_disks < 1 || n_disks > 16) return fail(MZH_ERR_ARG, "n_disks must be in [1,16], got %d", n_disks);
  if (max_sims < 0 || max_sims > 32000) return fail(MZH_ERR_ARG, "max_sims must be in [0,32000], got %d", max_sims);
  if (max_roots < 1) return fail(MZH_ERR_ARG, "max_roots must be >= 1, got %d", max_roots);
  if (support != 33 && support != 1) return fail(MZH_ERR_ARG, "support must be 33 or 1, got %d", support);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MZH_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(MZH_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
  DeviceGuard g(device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  mzh_engine* eng = new mzh_engine();
  eng->device = device;
  eng->n_disks = n_disks;
  eng->max_sims = max_sims;
  eng->max_roots = max_roots;
  eng->support = support;
  eng->in_dim = 3 * n_disks;
  eng->kin = ((eng->in_dim + 15) / 16) * 16;
  eng->E = max_sims + 1;
  // MZH_MEMO_DEPTH: the engine's initial memo depth request, as mzh_set_memo_depth reads it (measurements
  // through programs that do not call it).  A value that is no integer, or one mzh_set_memo_depth would
  // refuse, is an error: no engine is made
  if (const char* v = getenv("MZH_MEMO_DEPTH")) {
    char* end = nullptr;
    const long d = strtol(v, &end, 10);
    int D = 0;
    if (end == v || *end != '\0' || d < -1 || d > MZH_MEMO_MAX_DEPTH) {
      delete eng;
      return fail(MZH_ERR_ARG, "MZH_MEMO_DEPTH='%s': expected an integer in [-1, %d]", v, MZH_MEMO_MAX_DEPTH);
    }
    const int st = memo_depth_for(n_disks, (int)d, &D);
    if (st) {
      delete eng;
      return st;
    }
    eng->memo_want = (int)d;
  }
  // MZH_MEMO_GROW_BYTES: likewise the initial request of mzh_set_memo_grow (-1 the default budget, 0 off)
  if (const char* v = getenv("MZH_MEMO_GROW_BYTES")) {
    char* end = nullptr;
    const long long b = strtoll(v, &end, 10);
    if (end == v || *end != '\0' || b < -1 || b > MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES) {
      delete eng;
      return fail(MZH_ERR_ARG, "MZH_MEMO_GROW_BYTES='%s': expected an integer in [-1, %lld]", v,
                  MZH_MEMO_MAX_ROWS * MZH_MEMO_ROW_BYTES);
    }
    eng->grow_want = b;
  }
  const size_t nblk = (size_t)max_roots * eng->E;
  // MzhBlock (mzh_tree.h) / MzwBlock (mzh_wave.hip): one 128-B cache line per expanded node
  hipError_t e = hipMalloc(&eng->tree, nblk * 128);  // one 128-B block per expanded node
  if (e == hipSuccess) e = hipMalloc(&eng->htree, nblk * MZH_LATENT * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&eng->pathx, nblk * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc(&eng->table, sizeof(double) * (size_t)(max_sims + 2));
  if (e == hipSuccess) e = hipMalloc(&eng->memo_cnt, 3 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(eng->memo_cnt, 0, 3 * sizeof(unsigned long long));
  if (e != hipSuccess) {
    mzh_destroy(eng);
    return hip_fail(e, "hipMalloc (engine workspace)");
  }
  // UCB table on the host with libm, exactly the reference's python expression (node.py:114-121)
  std::vector<double> t(max_sims + 2);
  for (int n = 0; n < max_sims + 2; ++n) t[n] = (log((double)(n + 19652 + 1) / 19652.0) + 1.25) * sqrt((double)n);
  e = hipMemcpy(eng->table, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    mzh_destroy(eng);
    return hip_fail(e, "hipMemcpy (ucb table)");
  }
  *out = eng;
  return MZH_OK;
}

extern "C" int mzh_destroy(mzh_engine* eng) {
  if (!eng) return MZH_OK;
  DeviceGuard g(eng->device);
  if (eng->tree) (void)hipFree(eng->tree);
  if (eng->htree) (void)hipFree(eng->htree);
  if (eng->pathx) (void)hipFree(eng->pathx);
  if (eng->table) (void)hipFree(eng->table);
  if (eng->wbuf) (void)hipFree(eng->wbuf);
  if (eng->setbuf) (void)hipFree(eng->setbuf);
  if (eng->mtiles) (void)hipFree(eng->mtiles);
  if (eng->mntiles) (void)hipFree(eng->mntiles);
  if (eng->memo_h) (void)hipFree(eng->memo_h);
  if (eng->memo_rec) (void)hipFree(eng->memo_rec);
  if (eng->memo_cnt) (void)hipFree(eng->memo_cnt);
  if (eng->memo_link) (void)hipFree(eng->memo_link);
  if (eng->memo_ctr) (void)hipFree(eng->memo_ctr);
  if (eng->memo_log) (void)hipFree(eng->memo_log);
  if (eng->memo_logn) (void)hipFree(eng->memo_logn);
  if (eng->tbuf) (void)hipFree(eng->tbuf);
  if (eng->settbuf) (void)hipFree(eng->settbuf);
  if (eng->rmap) (void)hipFree(eng->rmap);
  if (eng->ptab) (void)hipFree(eng->ptab);
  if (eng->set_ptab) (void)hipFree(eng->set_ptab);
  if (eng->scal2) (void)hipFree(eng->scal2);
  if (eng->scal2_host) (void)hipHostFree(eng->scal2_host);
  if (eng->gmap) (void)hipFree(eng->gmap);
  if (eng->gbuf) (void)hipFree(eng->gbuf);
  if (eng->setgbuf) (void)hipFree(eng->setgbuf);
  delete eng->gmaps;
  delete eng->maps;
  delete eng;
  return MZH_OK;
}

// drop the expansion memo (after the device has finished with it)
static hipError_t memo_drop(mzh_engine* eng) {
  if (!eng->memo_h && !eng->memo_rec) return hipSuccess;
  ++eng->n_wait;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  if (eng->memo_h) (void)hipFree(eng->memo_h);
  if (eng->memo_rec) (void)hipFree(eng->memo_rec);
  if (eng->memo_link) (void)hipFree(eng->memo_link);
  if (eng->memo_ctr) (void)hipFree(eng->memo_ctr);
  eng->memo_h = nullptr;
  eng->memo_rec = nullptr;
  eng->memo_link = nullptr;
  eng->memo_ctr = nullptr;
  eng->memo_D = 0;
  eng->memo_base = eng->memo_cap = 0;
  return hipSuccess;
}

// the cooperative kernels' view of a packed blob uploaded at `base` (MzhPacked's offsets as pointers)
static int make_net(const MzhPacked& pk, const float* base, int sup, int in, MzhNet* out) {
  auto mk = [&](const PackedLayer& pl) {
    MzhLayer m;
    m.w = reinterpret_cast<const float4*>(base + pl.woff);
    m.b = base + pl.boff;
    m.kb = pl.kb;
    m.nt = pl.nt;
    m.woff = (int)(pl.woff * sizeof(float));
    m.boff = (int)(pl.boff * sizeof(float));
    return m;
  };
  MzhNet n{};
  n.wbase = base;
  n.rep0 = mk(pk.L[MZH_REP0]); n.rep2 = mk(pk.L[MZH_REP2]); n.dyn0 = mk(pk.L[MZH_DYN0]); n.dyn2 = mk(pk.L[MZH_DYN2]);
  n.rwd0 = mk(pk.L[MZH_RWD0]); n.rwd2 = mk(pk.L[MZH_RWD2]); n.pol0 = mk(pk.L[MZH_POL0]); n.pol2 = mk(pk.L[MZH_POL2]);
  n.val0 = mk(pk.L[MZH_VAL0]); n.val2 = mk(pk.L[MZH_VAL2]);
  if (n.val0.w != n.pol0.w + (size_t)n.pol0.nt * n.pol0.kb * 64)
    return fail(MZH_ERR_STATE, "pol0/val0 weights not contiguous");
  n.dyn0_onehot = base + pk.onehot;
  // the wave layout's bin-32 arrays serve both kernels (null and 0 without a 33-bin head)
  auto w32 = [&](const PackedW& pw) { return pw.w32off ? reinterpret_cast<const float4*>(base + pw.w32off) : nullptr; };
  n.rwd32 = w32(pk.W[2]); n.val32 = w32(pk.W[4]); n.rwd32b = pk.W[2].b32; n.val32b = pk.W[4].b32;
  n.support = sup;
  n.in_dim = in;
  *out = n;
  return MZH_OK;
}

// the saliency kernel's view of a transposed blob uploaded at `base` (`stride` bytes between a set's members)
static MzhSalNetT make_tnet(const MzhPackedT& t, const void* base, size_t stride) {
  MzhSalNetT n{};
  n.base = static_cast<const float4*>(base);
  for (int i = 0; i < MZH_T_LAYERS; ++i) n.off[i] = (int)(t.off[i] / 4);
  n.kb_val2 = t.kb[MZH_T_VAL2];
  n.nt_rep0 = t.nt[MZH_T_REP0];
  n.stride = stride;
  return n;
}

// the latency kernel's views of the blob at `base` (MzhPacked::one: offsets inside the main blob)
static MzhOneNet make_onet(const MzhPacked& pk, const float* base) {
  MzhOneNet o;
  o.l1 = reinterpret_cast<const float4*>(base + pk.one.l1);
  o.b1 = reinterpret_cast<const float4*>(base + pk.one.b1);
  o.rep0 = base + pk.one.rep0;
  o.rep0b = base + pk.one.rep0b;
  o.rep2 = reinterpret_cast<const float4*>(base + pk.one.rep2);
  o.rep2b = base + pk.one.rep2b;
  o.l2 = reinterpret_cast<const float4*>(base + pk.one.l2);
  return o;
}

// the three kernels' views (MzhNet, MzhWNet, MzhOneNet) and the saliency view of the single network whose
// blobs lie in wbuf / tbuf with the offsets of pk / pt
static int bind_single(mzh_engine* eng, const MzhPacked& pk, const MzhPackedT& pt) {
  const int in = eng->in_dim, sup = eng->support;
  eng->tnet = make_tnet(pt, eng->tbuf, 0);
  const float* base = static_cast<const float*>(eng->wbuf);
  const int nst = make_net(pk, base, sup, in, &eng->net);
  if (nst) return nst;
  auto mkw = [&](const PackedW& pw) {
    MzhWMlp m;
    m.s = reinterpret_cast<const float4*>(base + pw.soff);
    m.b1 = base + pw.b1off;
    m.b2 = base + pw.b2off;
    m.kb1 = pw.kb1;
    m.no = pw.no;
    m.w32 = pw.w32off ? reinterpret_cast<const float4*>(base + pw.w32off) : nullptr;
    m.b32 = pw.b32;
    m.soff = (int)(pw.soff * sizeof(float));
    m.b1off = (int)(pw.b1off * sizeof(float));
    m.b2off = (int)(pw.b2off * sizeof(float));
    m.w32off = (int)(pw.w32off * sizeof(float));
    return m;
  };
  MzhWNet& w = eng->wnet;
  w.wbase = base;
  w.rep = mkw(pk.W[0]); w.dyn = mkw(pk.W[1]); w.rwd = mkw(pk.W[2]); w.pol = mkw(pk.W[3]); w.val = mkw(pk.W[4]);
  w.oh = base + pk.wonehot;
  w.support = sup;
  w.in_dim = in;
  eng->onet = make_onet(pk, base);
  eng->loaded = true;
  return MZH_OK;
}

extern "C" int mzh_load_weights(mzh_engine* eng, const float* flat, size_t n_floats) {
  if (!eng || !flat) return fail(MZH_ERR_ARG, "engine or weights NULL");
  const int in = eng->in_dim, sup = eng->support;
  const size_t want = mzh_canon_view(nullptr, in, sup).total;
  if (n_floats != want) return fail(MZH_ERR_ARG, "weights: expected %zu floats, got %zu", want, n_floats);
  const MzhPacked pk = mzh_pack_network(mzh_canon_view(flat, in, sup));
  const MzhPackedT pt = mzh_pack_transposed(mzh_canon_view(flat, in, sup));

  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  eng->g_valid = false;
  if (eng->wbuf) {
    ++eng->n_wait;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(eng->wbuf));
    ++eng->n_free;
    eng->wbuf = nullptr;
    eng->loaded = false;
    if (eng->tbuf) {
      HIP_OK(hipFree(eng->tbuf));
      ++eng->n_free;
    }
    eng->tbuf = nullptr;
  }
  HIP_OK(memo_drop(eng));  // the table is a function of the weights
  HIP_OK(hipMalloc(&eng->wbuf, pk.blob.size() * sizeof(float)));
  HIP_OK(hipMemcpy(eng->wbuf, pk.blob.data(), pk.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&eng->tbuf, pt.blob.size() * sizeof(float)));
  HIP_OK(hipMemcpy(eng->tbuf, pt.blob.data(), pt.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  eng->n_alloc += 2;
  eng->wn = pk.blob.size();
  eng->tn = pt.blob.size();
  return bind_single(eng, pk, pt);
}

// the views of the loaded set (network 0's MzhNet as the template the multi kernels offset, the saliency view)
static int bind_set(mzh_engine* eng, const MzhPacked& layout, const MzhPackedT& tlayout, size_t stride, size_t tstride,
                    int M) {
  eng->settnet = make_tnet(tlayout, eng->settbuf, tstride * sizeof(float));
  const float* base = static_cast<const float*>(eng->setbuf);
  const int nst = make_net(layout, base, eng->support, eng->in_dim, &eng->setnet);
  if (nst) return nst;
  eng->setonet = make_onet(layout, base);
  eng->set_stride = stride * sizeof(float);
  eng->set_scal = base + (size_t)M * stride;
  eng->set_m = M;
  return MZH_OK;
}

// free the loaded set's buffers once the device has finished with them
static hipError_t set_release(mzh_engine* eng) {
  if (!eng->setbuf) return hipSuccess;
  ++eng->n_wait;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipFree(eng->setbuf);
  if (e != hipSuccess) return e;
  ++eng->n_free;
  eng->setbuf = nullptr;
  eng->set_m = 0;
  if (eng->settbuf) {
    e = hipFree(eng->settbuf);
    if (e != hipSuccess) return e;
    ++eng->n_free;
  }
  eng->settbuf = nullptr;
  return hipSuccess;
}

// the tile table workspace of the multi-network kernels, allocated with the first set
static hipError_t set_workspace(mzh_engine* eng) {
  hipError_t e = hipSuccess;
  if (!eng->mtiles)
    e = hipMalloc(&eng->mtiles, sizeof(MzhTile) * (size_t)mzh_multi_max_tiles(eng->max_roots, 16, MZH_MULTI_MAX_NETS));
  if (e == hipSuccess && !eng->mntiles) e = hipMalloc(&eng->mntiles, sizeof(int32_t));
  return e;
}

extern "C" int mzh_load_weight_set(mzh_engine* eng, const float* flat, size_t n_floats, int M) {
  if (!eng || !flat) return fail(MZH_ERR_ARG, "engine or weights NULL");
  if (M < 1 || M > MZH_MULTI_MAX_NETS)
    return fail(MZH_ERR_ARG, "weight set: M must be in [1,%d], got %d", MZH_MULTI_MAX_NETS, M);
  const int in = eng->in_dim, sup = eng->support;
  const size_t want = mzh_canon_view(nullptr, in, sup).total;
  if (n_floats != want) return fail(MZH_ERR_ARG, "weight set: expected %zu floats per network, got %zu", want, n_floats);
  const MzhPackedSet ps = mzh_pack_network_set(flat, M, in, sup);
  const MzhPackedTSet pts = mzh_pack_transposed_set(flat, M, in, sup);

  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  eng->setg_valid = false;
  HIP_OK(set_release(eng));
  HIP_OK(set_workspace(eng));
  HIP_OK(hipMalloc(&eng->setbuf, ps.blob.size() * sizeof(float)));
  HIP_OK(hipMemcpy(eng->setbuf, ps.blob.data(), ps.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&eng->settbuf, pts.blob.size() * sizeof(float)));
  HIP_OK(hipMemcpy(eng->settbuf, pts.blob.data(), pts.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  eng->n_alloc += 2;
  eng->setn = ps.blob.size();
  eng->settn = pts.blob.size();
  return bind_set(eng, ps.layout, pts.layout, ps.stride, pts.stride, M);
}

// ---- device repack: the same blobs gathered on the device from the live parameter tensors ----
// the pack maps of the engine's shape, on the host and (encoded, padded with -1 to the set strides) on the
// device, and the small buffers of the single-network call: made once per engine
static int repack_ensure(mzh_engine* eng) {
  if (eng->rmap) return MZH_OK;
  const int in = eng->in_dim, sup = eng->support;
  if (!eng->maps) {
    MzhPackMaps* m = new MzhPackMaps();
    if (!mzh_pack_maps(in, sup, m)) {
      delete m;
      return fail(MZH_ERR_ARG, "pack maps: the shape has 2^24 or more weights");
    }
    eng->maps = m;
  }
  const MzhPackMaps& mp = *eng->maps;
  if (mp.main.size() % 4 || mp.trans.size() % 4)
    return fail(MZH_ERR_STATE, "device repack: a blob of %zu / %zu floats is no whole number of float4", mp.main.size(),
                mp.trans.size());
  const MzhCanon sizes = mzh_canon_view(nullptr, in, sup);
  const size_t rs = (mp.main.size() + 63) & ~(size_t)63, rts = (mp.trans.size() + 63) & ~(size_t)63;
  std::vector<int32_t> enc(rs + rts, -1);
  for (size_t j = 0; j < mp.main.size(); ++j) enc[j] = mzh_pack_map_encode(sizes, mp.main[j]);
  for (size_t j = 0; j < mp.trans.size(); ++j) enc[rs + j] = mzh_pack_map_encode(sizes, mp.trans[j]);
  // every entry names an element inside its tensor: the kernel's reads stay in bounds
  for (size_t j = 0; j < enc.size(); ++j) {
    if (enc[j] < 0) continue;
    const int t = enc[j] >> 24, l = t >> 1;
    const size_t numel = (t & 1) ? (size_t)sizes.out[l] : (size_t)sizes.out[l] * sizes.in[l];
    if (t >= 20 || (size_t)(enc[j] & 0xffffff) >= numel) return fail(MZH_ERR_STATE, "device repack: map entry %zu out of range", j);
  }
  for (int i = 0; i < 2; ++i) eng->rscal[i] = mzh_pack_map_encode(sizes, mp.scalar_src[i]);
  if (!eng->ptab) HIP_OK(hipMalloc(&eng->ptab, 20 * sizeof(float*)));
  if (!eng->scal2) HIP_OK(hipMalloc(&eng->scal2, 2 * sizeof(float)));
  if (!eng->scal2_host) HIP_OK(hipHostMalloc(&eng->scal2_host, 2 * sizeof(float)));
  int32_t* d = nullptr;
  HIP_OK(hipMalloc(&d, enc.size() * sizeof(int32_t)));
  hipError_t e = hipMemcpy(d, enc.data(), enc.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy (pack maps)");
  }
  eng->rmap = d;
  eng->rstride = rs;
  eng->rtstride = rts;
  return MZH_OK;
}

// the device's pointer table follows the caller's: uploaded when it differs from what the table holds (the
// first call, or parameters that moved); the host copy is consumed before hipMemcpyAsync returns (pageable)
static int ptab_sync(const float* const* param, size_t n, const float** dev, std::vector<const float*>* host,
                     hipStream_t stream) {
  if (host->size() == n && memcmp(host->data(), param, n * sizeof(float*)) == 0) return MZH_OK;
  host->clear();  // unknown contents until the copy is issued
  HIP_OK(hipMemcpyAsync(dev, param, n * sizeof(float*), hipMemcpyHostToDevice, stream));
  host->assign(param, param + n);
  return MZH_OK;
}

static MzhRepackParams repack_params(const mzh_engine* eng, bool set) {
  MzhRepackParams p{};
  p.map_m = reinterpret_cast<const int4*>(eng->rmap);
  p.map_t = reinterpret_cast<const int4*>(eng->rmap + eng->rstride);
  // a set member is written up to its stride (zeros between the blobs), the single network up to its blob's end
  p.n4m = (int)((set ? eng->rstride : eng->maps->main.size()) / 4);
  p.n4t = (int)((set ? eng->rtstride : eng->maps->trans.size()) / 4);
  p.stride_m = eng->rstride;
  p.stride_t = eng->rtstride;
  p.scal_src[0] = eng->rscal[0];
  p.scal_src[1] = eng->rscal[1];
  return p;
}

extern "C" int mzh_load_weights_device(mzh_engine* eng, const float* const* param, mzh_stream stream) {
  if (!eng || !param) return fail(MZH_ERR_ARG, "load_weights_device: engine or param NULL");
  for (int i = 0; i < 20; ++i)
    if (!param[i]) return fail(MZH_ERR_ARG, "load_weights_device: param[%d] is NULL", i);
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  const int st = repack_ensure(eng);
  if (st) return st;
  const MzhPackMaps& mp = *eng->maps;
  eng->g_valid = false;
  if (!eng->wbuf) {
    HIP_OK(hipMalloc(&eng->wbuf, mp.main.size() * sizeof(float)));
    ++eng->n_alloc;
    eng->wn = mp.main.size();
  }
  if (!eng->tbuf) {
    HIP_OK(hipMalloc(&eng->tbuf, mp.trans.size() * sizeof(float)));
    ++eng->n_alloc;
    eng->tn = mp.trans.size();
  }
  HIP_OK(memo_drop(eng));  // the table is a function of the weights
  const hipStream_t s = (hipStream_t)stream;
  const int ps = ptab_sync(param, 20, eng->ptab, &eng->ptab_host, s);
  if (ps) return ps;
  MzhRepackParams p = repack_params(eng, false);
  p.ptab = eng->ptab;
  p.dst_m = static_cast<float*>(eng->wbuf);
  p.dst_t = static_cast<float*>(eng->tbuf);
  p.scal = eng->scal2;
  hipError_t e = mzh_launch_repack(p, 1, s);
  if (e != hipSuccess) return hip_fail(e, "repack launch");
  MzhPacked pk = mp.layout;
  if (eng->support == 33) {  // the kernels take bin 32's two biases by value: one 8-byte copy, one wait
    HIP_OK(hipMemcpyAsync(eng->scal2_host, eng->scal2, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    pk.W[2].b32 = eng->scal2_host[0];
    pk.W[4].b32 = eng->scal2_host[1];
  }
  return bind_single(eng, pk, mp.tlayout);
}

extern "C" int mzh_load_weight_set_device(mzh_engine* eng, const float* const* param, int M, mzh_stream stream) {
  if (!eng || !param) return fail(MZH_ERR_ARG, "load_weight_set_device: engine or param NULL");
  if (M < 1 || M > MZH_MULTI_MAX_NETS)
    return fail(MZH_ERR_ARG, "weight set: M must be in [1,%d], got %d", MZH_MULTI_MAX_NETS, M);
  for (int i = 0; i < 20 * M; ++i)
    if (!param[i]) return fail(MZH_ERR_ARG, "load_weight_set_device: param[%d][%d] is NULL", i / 20, i % 20);
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  const int st = repack_ensure(eng);
  if (st) return st;
  const MzhPackMaps& mp = *eng->maps;
  eng->setg_valid = false;
  const size_t setn = (size_t)M * eng->rstride + 2 * (size_t)M, settn = (size_t)M * eng->rtstride;
  if (eng->setbuf && eng->set_m != M) HIP_OK(set_release(eng));
  HIP_OK(set_workspace(eng));
  if (!eng->setbuf) {
    HIP_OK(hipMalloc(&eng->setbuf, setn * sizeof(float)));
    ++eng->n_alloc;
    eng->setn = setn;
  }
  if (!eng->settbuf) {
    HIP_OK(hipMalloc(&eng->settbuf, settn * sizeof(float)));
    ++eng->n_alloc;
    eng->settn = settn;
  }
  if (eng->set_ptab_m != M) {
    if (eng->set_ptab) HIP_OK(hipFree(eng->set_ptab));
    eng->set_ptab = nullptr;
    eng->set_ptab_m = 0;
    eng->set_ptab_host.clear();
    HIP_OK(hipMalloc(&eng->set_ptab, (size_t)M * 20 * sizeof(float*)));
    eng->set_ptab_m = M;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int ps = ptab_sync(param, (size_t)M * 20, eng->set_ptab, &eng->set_ptab_host, s);
  if (ps) return ps;
  MzhRepackParams p = repack_params(eng, true);
  p.ptab = eng->set_ptab;
  p.dst_m = static_cast<float*>(eng->setbuf);
  p.dst_t = static_cast<float*>(eng->settbuf);
  p.scal = p.dst_m + (size_t)M * eng->rstride;  // MzhPackedSet::scal
  hipError_t e = mzh_launch_repack(p, M, s);
  if (e != hipSuccess) return hip_fail(e, "repack launch");
  return bind_set(eng, mp.layout, mp.tlayout, eng->rstride, eng->rtstride, M);
}

extern "C" int mzh_pack_map(int n_disks, int support, int which, int32_t* map, size_t* n_floats, int64_t* scalar_src) {
  size_t total = 0;
  const int st = mzh_weights_size(n_disks, support, &total);
  if (st) return st;
  if (which < 0 || which > 1) return fail(MZH_ERR_ARG, "pack_map: which must be 0 (main) or 1 (transposed), got %d", which);
  MzhPackMaps mp;
  if (!mzh_pack_maps(3 * n_disks, support, &mp)) return fail(MZH_ERR_ARG, "pack_map: the shape has 2^24 or more weights");
  const std::vector<int32_t>& m = which ? mp.trans : mp.main;
  if (n_floats) *n_floats = m.size();
  if (map) memcpy(map, m.data(), m.size() * sizeof(int32_t));
  if (scalar_src) {
    scalar_src[0] = mp.scalar_src[0];
    scalar_src[1] = mp.scalar_src[1];
  }
  return MZH_OK;
}

extern "C" int mzh_weights_debug_blob(mzh_engine* eng, int which, float* dst, size_t* n_floats) {
  if (!eng || !n_floats) return fail(MZH_ERR_ARG, "weights_debug_blob: NULL argument");
  if (which < 0 || which > 3) return fail(MZH_ERR_ARG, "weights_debug_blob: which must be in [0,3], got %d", which);
  if (which < 2 ? !eng->loaded : eng->set_m == 0)
    return fail(MZH_ERR_STATE, which < 2 ? "weights not loaded" : "no weight set loaded");
  const void* src[4] = {eng->wbuf, eng->tbuf, eng->setbuf, eng->settbuf};
  const size_t n[4] = {eng->wn, eng->tn, eng->setn, eng->settn};
  *n_floats = n[which];
  if (!dst) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(dst, src[which], n[which] * sizeof(float), hipMemcpyDeviceToDevice));
  HIP_OK(hipDeviceSynchronize());
  return MZH_OK;
}

extern "C" int mzh_weights_debug_counters(mzh_engine* eng, uint64_t* counters) {
  if (!eng || !counters) return fail(MZH_ERR_ARG, "weights_debug_counters: NULL argument");
  counters[0] = eng->n_alloc;
  counters[1] = eng->n_free;
  counters[2] = eng->n_wait;
  return MZH_OK;
}

// ---- environment ----
extern "C" int mzh_env_step(int n_disks, int goal_peg, int max_steps, int B, uint8_t* state, const int32_t* action,
                            uint8_t* moved, float* obs, int8_t* reward, uint8_t* done, uint8_t* illegal,
                            int32_t* step_ctr, uint8_t* active, int32_t* err_count, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || goal_peg < 0 || goal_peg > 2 || B < 0)
    return fail(MZH_ERR_ARG, "env_step: bad n_disks=%d goal_peg=%d B=%d", n_disks, goal_peg, B);
  if (B == 0) return MZH_OK;
  if (!state || !action || !reward || !done || !illegal || !step_ctr || !active)
    return fail(MZH_ERR_ARG, "env_step: required buffer is NULL");
  hipError_t e = mzh_launch_env_step(n_disks, goal_peg, max_steps, B, state, action, moved, obs, reward, done, illegal,
                                     step_ctr, active, err_count, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "env_step launch");
}

extern "C" int mzh_env_run_plan(const mzh_plan_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "env_run_plan: args is NULL");
  if (a->n_disks < 1 || a->n_disks > 32 || a->goal_peg < 0 || a->goal_peg > 2)
    return fail(MZH_ERR_ARG, "env_run_plan: bad n_disks=%d goal_peg=%d", a->n_disks, a->goal_peg);
  if (a->n < 1 || a->B < 1 || (!a->env_index && a->B < a->n))
    return fail(MZH_ERR_ARG, "env_run_plan: bad n=%d rows for B=%d envs", a->n, a->B);
  if (a->max_plan_len < 1 || a->plan_stride < a->max_plan_len)
    return fail(MZH_ERR_ARG, "env_run_plan: bad max_plan_len=%d plan_stride=%d", a->max_plan_len, a->plan_stride);
  if (!a->plan || !a->plan_len || !a->state || !a->step_ctr || !a->active || !a->obs || !a->executed ||
      !a->steps_total || !a->illegal_total)
    return fail(MZH_ERR_ARG, "env_run_plan: required buffer is NULL");
  hipError_t e = mzh_launch_env_run_plan(a, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "env_run_plan launch");
}

extern "C" int mzh_env_step_observe(const mzh_observe_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "env_step_observe: args is NULL");
  if (a->n_disks < 1 || a->n_disks > 32 || a->goal_peg < 0 || a->goal_peg > 2)
    return fail(MZH_ERR_ARG, "env_step_observe: bad n_disks=%d goal_peg=%d", a->n_disks, a->goal_peg);
  if (a->n < 1 || a->B < 1 || (!a->env_index && a->B < a->n))
    return fail(MZH_ERR_ARG, "env_step_observe: bad n=%d rows for B=%d envs", a->n, a->B);
  if (!a->state || !a->step_ctr || !a->active || !a->steps_total || !a->illegal_total || !a->solved || !a->obs ||
      (a->perm_disc && !a->perm_peg))
    return fail(MZH_ERR_ARG, "env_step_observe: required buffer is NULL");
  hipError_t e = mzh_launch_env_step_observe(a, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "env_step_observe launch");
}

extern "C" int mzh_legal_mask(int n_disks, int B, const uint8_t* state, uint8_t* mask, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || B < 0 || (B > 0 && (!state || !mask))) return fail(MZH_ERR_ARG, "legal_mask: bad args");
  if (B == 0) return MZH_OK;
  hipError_t e = mzh_launch_legal_mask(n_disks, B, state, mask, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "legal_mask launch");
}

extern "C" int mzh_encode_obs(int n_disks, int B, const uint8_t* state, float* obs, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 32 || B < 0 || (B > 0 && (!state || !obs))) return fail(MZH_ERR_ARG, "encode_obs: bad args");
  if (B == 0) return MZH_OK;
  hipError_t e = mzh_launch_encode_obs(n_disks, B, state, obs, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "encode_obs launch");
}

extern "C" int mzh_hanoi_solver(int n_disks, int goal_peg, int B, const uint8_t* state, int32_t* moves, mzh_stream stream) {
  if (n_disks < 1 || n_disks > 30 || goal_peg < 0 || goal_peg > 2 || B < 0 || (B > 0 && (!state || !moves)))
    return fail(MZH_ERR_ARG, "hanoi_solver: bad args");
  if (B == 0) return MZH_OK;
  hipError_t e = mzh_launch_hanoi_solver(n_disks, goal_peg, B, state, moves, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "hanoi_solver launch");
}

// ---- inference ----
// roots (rows) per workgroup of the standalone inference kernels: 16 while that fits one workgroup
// per CU (B <= 4096), else 32
static int pick_rows(int B) { return B > 256 * 16 ? 32 : 16; }

// cooperative search tile: 16 roots while that is one round of workgroups (B <= 4,096), else 32
// roots (a second round of 16-root workgroups costs more than 32-root tiles).  MZH_FLAG_COOP_TILE16 /
// MZH_FLAG_COOP_TILE32 force one (tests reach both tiles' code paths at any batch size).
static int pick_tile(int B, uint32_t flags) {
  if (flags & MZH_FLAG_COOP_TILE16) return 16;
  if (flags & MZH_FLAG_COOP_TILE32) return 32;
  return B > 256 * 16 ? 32 : 16;
}

extern "C" int mzh_initial_inference(mzh_engine* eng, int B, const float* obs, float* h, float* reward, float* pi,
                                     float* value, float* policy_logits, float* value_logits, mzh_stream stream) {
  if (!eng) return fail(MZH_ERR_ARG, "engine NULL");
  if (!eng->loaded) return fail(MZH_ERR_STATE, "weights not loaded");
  if (B < 0 || (B > 0 && (!obs || !h))) return fail(MZH_ERR_ARG, "initial_inference: bad args");
  if (B == 0) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhInferParams p{};
  p.B = B; p.in_dim = eng->in_dim; p.kin = eng->kin; p.x = obs; p.h = h; p.reward = reward; p.pi = pi;
  p.value = value; p.policy_logits = policy_logits; p.value_logits = value_logits;
  hipError_t e = mzh_launch_infer(pick_rows(B), false, eng->net, p, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "initial_inference launch");
}

extern "C" int mzh_recurrent_inference(mzh_engine* eng, int B, const float* h_in, const int32_t* action, float* h,
                                       float* reward, float* pi, float* value, float* policy_logits,
                                       float* value_logits, float* reward_logits, mzh_stream stream) {
  if (!eng) return fail(MZH_ERR_ARG, "engine NULL");
  if (!eng->loaded) return fail(MZH_ERR_STATE, "weights not loaded");
  if (B < 0 || (B > 0 && (!h_in || !action || !h))) return fail(MZH_ERR_ARG, "recurrent_inference: bad args");
  if (B == 0) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhInferParams p{};
  p.B = B; p.in_dim = eng->in_dim; p.kin = eng->kin; p.x = h_in; p.action = action; p.h = h; p.reward = reward;
  p.pi = pi; p.value = value; p.policy_logits = policy_logits; p.value_logits = value_logits;
  p.reward_logits = reward_logits;
  hipError_t e = mzh_launch_infer(pick_rows(B), true, eng->net, p, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "recurrent_inference launch");
}

// ---- search ----
static const size_t kMaxLds = 163840;

// kernel choice: the wave-independent kernel (mzh_wave.hip) with 32 roots per wave once the batch
// gives two such waves per SIMD, with 16 roots per wave for mid-size batches (>= 1024 such waves),
// else the cooperative kernel (mzh_search.hip) whose 4 waves split every MLP layer of one 16- or
// 32-root tile.  MZH_FLAG_KERNEL_* (or MZH_KERNEL=coop|wave|wave16) force one.
static const int kWaveMinRoots = 53248, kWave16MinRoots = 8193;  // measured crossovers
struct KernelChoice {
  bool wave;
  int nt;  // wave kernel: 16-root column tiles per wave
};
static KernelChoice choose_kernel(int B, uint32_t flags) {
  if (flags & MZH_FLAG_KERNEL_WAVE16) return {true, 1};
  if (flags & MZH_FLAG_KERNEL_WAVE) return {true, 2};
  if (flags & MZH_FLAG_KERNEL_COOP) return {false, 0};
  static const int forced = [] {
    const char* v = getenv("MZH_KERNEL");
    if (!v) return 0;
    return strcmp(v, "wave") == 0 ? 2 : strcmp(v, "wave16") == 0 ? 1 : strcmp(v, "coop") == 0 ? -1 : 0;
  }();
  if (forced) return forced > 0 ? KernelChoice{true, forced} : KernelChoice{false, 0};
  if (B >= kWaveMinRoots) return {true, 2};
  if (B >= kWave16MinRoots) return {true, 1};
  return {false, 0};
}

// the latency path (mzh_one.hip): MLP searches of up to kOneMaxRoots roots take one root per workgroup
// (persistent over the roots beyond the 256 workgroups of one round) while its LDS fits; a forced kernel
// flag (or MZH_KERNEL) decides otherwise.  MZH_FLAG_KERNEL_ONE forces it (an error where it cannot run).
static const int kOneMaxRoots = 512, kOneGrid = 256;  // crossover: profiles/r06_one_probe.json
static bool one_forced_env() {
  static const bool f = [] {
    const char* v = getenv("MZH_KERNEL");
    return v && strcmp(v, "one") == 0;
  }();
  return f;
}

// every template argument of the launch (MzhSearchPlan); returns a status (capacity errors)
static int make_plan(int B, int S, uint32_t flags, bool replay, int support, bool has_minmax, MzhSearchPlan* pl) {
  const uint32_t forced = flags & (MZH_FLAG_KERNEL_COOP | MZH_FLAG_KERNEL_WAVE | MZH_FLAG_KERNEL_WAVE16 | MZH_FLAG_COOP_OCC2 |
                                   MZH_FLAG_COOP_TILE16 | MZH_FLAG_COOP_TILE32);
  const bool one_fits = mzh_one_smem_bytes(S, false) <= kMaxLds;
  if (flags & MZH_FLAG_KERNEL_ONE) {
    if (replay) return fail(MZH_ERR_ARG, "MZH_FLAG_KERNEL_ONE: the latency kernel has no replay (tree-only) form");
    if (forced) return fail(MZH_ERR_ARG, "MZH_FLAG_KERNEL_ONE combined with another kernel flag");
    if (!one_fits)
      return fail(MZH_ERR_CAPACITY, "MZH_FLAG_KERNEL_ONE: n_sims=%d needs %zu B of LDS", S, mzh_one_smem_bytes(S, false));
  }
  const bool env_kernel = getenv("MZH_KERNEL") != nullptr;
  if (!replay && one_fits &&
      ((flags & MZH_FLAG_KERNEL_ONE) || one_forced_env() || (!forced && !env_kernel && B <= kOneMaxRoots))) {
    MzhSearchPlan q{};
    q.one = 1;
    q.ohl = mzh_one_smem_bytes(S, true) <= kMaxLds;  // the latents in LDS where they fit
    q.sup33 = support == 33;
    q.mmin = has_minmax ? 1 : 0;
    q.grid = B < kOneGrid ? B : kOneGrid;
    *pl = q;
    return MZH_OK;
  }
  const KernelChoice kc = choose_kernel(B, flags);
  MzhSearchPlan q{};
  q.wave = kc.wave ? 1 : 0;
  q.nt = kc.nt;
  q.replay = replay ? 1 : 0;
  q.mmin = has_minmax ? 1 : 0;
  if (kc.wave) {
    if (mzh_wave_smem_bytes(S, kc.nt) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the wave kernel's LDS table budget", S);
    q.sup33 = support == 33;
    q.mmin = 0;  // the wave kernel decides the exact normaliser per selection
  } else {
    q.R = pick_tile(B, flags);
    // the two-workgroups-per-CU 16-root kernel: forced by MZH_FLAG_COOP_OCC2 (MLP searches; its LDS must
    // leave room for the second workgroup -- a search it cannot serve is an error, never a silent fallback;
    // replay searches have no occ2 instantiation and take the cooperative replay kernel, as mzh.h says)
    if ((flags & MZH_FLAG_COOP_OCC2) && !replay && 2 * mzh_search_smem_bytes(16, S, false, true) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "MZH_FLAG_COOP_OCC2: n_sims=%d needs %zu B of LDS per workgroup, more than "
                  "half a CU's", S, mzh_search_smem_bytes(16, S, false, true));
    if ((flags & MZH_FLAG_COOP_OCC2) && !replay) {
      q.R = 16;
      q.occ2 = 1;
      q.ohl = 0;
      q.sup33 = support == 33;
      *pl = q;
      return MZH_OK;
    }
    if (mzh_search_smem_bytes(q.R, S, false) > kMaxLds) q.R = 16;
    if (mzh_search_smem_bytes(q.R, S, false) > kMaxLds)
      return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the LDS path budget", S);
    // the one-hot columns go to LDS when they fit (never in the replay kernel, which runs no MLP)
    q.ohl = !replay && mzh_search_smem_bytes(q.R, S, true) <= kMaxLds;
    q.sup33 = replay || support == 33;
  }
  *pl = q;
  return MZH_OK;
}

static void plan_info(const MzhSearchPlan& q, int B, int S, mzh_search_plan* out) {
  memset(out, 0, sizeof(*out));
  const char* tf[2] = {"false", "true"};
  out->wave = q.wave;
  if (q.one) {
    out->roots_per_wave = 1;
    out->threads_per_workgroup = 512;
    out->roots_per_workgroup = 1;
    out->smem_bytes = (int64_t)mzh_one_smem_bytes(S, q.ohl);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_one_kernel<%s, %s, %s>", tf[q.sup33], tf[q.mmin], tf[q.ohl]);
    out->workgroups = q.grid;
    return;
  }
  if (q.wave) {
    out->roots_per_wave = 16 * q.nt;
    out->threads_per_workgroup = 256;
    out->roots_per_workgroup = 4 * 16 * q.nt;
    out->smem_bytes = (int64_t)mzh_wave_smem_bytes(S, q.nt);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_wave_kernel<%d, %s, %s>", q.nt, tf[q.replay], tf[q.sup33]);
  } else if (q.occ2) {
    out->roots_per_wave = 4;
    out->threads_per_workgroup = MZH_THREADS;
    out->roots_per_workgroup = 16;
    out->smem_bytes = (int64_t)mzh_search_smem_bytes(16, S, false, true);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_occ2_kernel<%s, %s>", tf[q.sup33], tf[q.mmin]);
  } else {
    out->roots_per_wave = q.R / 4;
    out->threads_per_workgroup = MZH_THREADS;
    out->roots_per_workgroup = q.R;
    out->smem_bytes = (int64_t)mzh_search_smem_bytes(q.R, S, q.ohl);
    snprintf(out->kernel, sizeof(out->kernel), "mzh_search_kernel<%d, %s, %s, %s, %s>", q.R, tf[q.replay], tf[q.ohl],
             tf[q.sup33], tf[q.mmin]);
  }
  out->workgroups = (B + out->roots_per_workgroup - 1) / out->roots_per_workgroup;
}

extern "C" int mzh_search_plan_query(int support, int B, int n_sims, uint32_t flags, int replay, int has_minmax_in,
                                     mzh_search_plan* out) {
  if (!out) return fail(MZH_ERR_ARG, "out is NULL");
  if (B < 1 || n_sims < 0 || n_sims > 32000 || (support != 33 && support != 1))
    return fail(MZH_ERR_ARG, "search_plan: bad B=%d n_sims=%d support=%d", B, n_sims, support);
  MzhSearchPlan q;
  const int st = make_plan(B, n_sims, flags, replay != 0, support, has_minmax_in != 0, &q);
  if (st) return st;
  plan_info(q, B, n_sims, out);
  return MZH_OK;
}

// the kernels' parameter block of a search call on this engine
static MzhSearchParams search_params(const mzh_engine* eng, const mzh_search_args* a) {
  MzhSearchParams p{};
  p.B = a->B; p.S = a->n_sims; p.E = eng->E; p.in_dim = eng->in_dim; p.kin = eng->kin;
  p.deterministic = a->deterministic; p.np1 = (a->flags & MZH_FLAG_NP1_UCB) ? 1 : 0;
  p.discount = a->discount; p.eps = a->eps; p.temperature = a->temperature;
  p.obs = a->obs; p.noise = a->noise; p.tie_idx = a->tie_idx; p.action_u = a->action_u; p.minmax_in = a->minmax_in;
  p.rp_root_pi = a->rp_root_pi; p.rp_sim = a->rp_sim;
  p.tree = eng->tree; p.htree = eng->htree; p.pathx = eng->pathx; p.table = eng->table;
  p.visits = a->visits; p.root_q = a->root_q; p.minmax_out = a->minmax_out; p.extra_ties = a->extra_ties;
  p.action = a->action; p.pi = a->pi; p.latent = a->latent; p.latent_len = a->latent_len; p.sel_steps = a->sel_steps; p.lockstep_levels = a->lockstep_levels;
  p.pow_table = a->pow_table;
  return p;
}

// ---- the wave kernel's expansion memo (mzh.h) ----
// the depth a request gives: -1 the budget's, 0 off, d > 0 as asked (status: a forced table too large)
static int memo_depth_for(int n_disks, int want, int* D) {
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
  eng->memo_want = depth;
  eng->memo_auto_cap = MZH_MEMO_MAX_DEPTH;
  return MZH_OK;
}

// the depth the next wave search uses: the request's, the automatic one no deeper than a build's memory allowed
static int memo_effective_depth(const mzh_engine* eng, int* D) {
  const int st = memo_depth_for(eng->n_disks, eng->memo_want, D);
  if (st == MZH_OK && eng->memo_want < 0 && *D > eng->memo_auto_cap) *D = eng->memo_auto_cap;
  return st;
}

// Fill the table for the loaded weights at depth D, level by level with the inference kernels: the 3^N one-hot
// states through initial inference, then every (node, move) of the level above through recurrent inference.
// Within a level the rows are ordered (state, node): child row = 6 * parent row + move.  Runs on `stream` and
// waits for it (the temporaries are freed on return).
// the extension rows the engine's request gives beside `dense_rows` dense ones
static long long memo_grow_cap(const mzh_engine* eng, long long dense_rows) {
  return mzh_memo_grow_rows(eng->grow_want < 0 ? MZH_MEMO_GROW_BUDGET_BYTES : eng->grow_want, dense_rows);
}

static int memo_build(mzh_engine* eng, int D, hipStream_t stream, bool* oom) {
  *oom = false;
  HIP_OK(memo_drop(eng));
  const auto t_start = std::chrono::steady_clock::now();
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
  float *dobs = nullptr, *hA = nullptr, *hB = nullptr, *xin = nullptr, *pi = nullptr, *rw = nullptr, *va = nullptr;
  int32_t* act = nullptr;
  auto release = [&]() {
    for (void* q : {(void*)dobs, (void*)hA, (void*)hB, (void*)xin, (void*)pi, (void*)rw, (void*)va, (void*)act})
      if (q) (void)hipFree(q);
  };
  auto bail = [&](hipError_t e, const char* what) {
    release();
    (void)memo_drop(eng);
    return hip_fail(e, what);
  };
  hipError_t e = hipMalloc(&eng->memo_h, (size_t)(rows + cap) * MZH_LATENT * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&eng->memo_rec, (size_t)(rows + cap) * 8 * sizeof(float));
  if (e == hipSuccess && cap > 0) e = hipMalloc(&eng->memo_link, (size_t)(rows + cap) * 6 * sizeof(int32_t));
  if (e == hipSuccess && cap > 0) e = hipMalloc(&eng->memo_ctr, 2 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(&dobs, obs.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&hA, (size_t)top * MZH_LATENT * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&hB, (size_t)(top / 6 + 1) * MZH_LATENT * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&xin, (size_t)top * MZH_LATENT * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&act, (size_t)top * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(&pi, (size_t)top * MZH_A * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&rw, (size_t)top * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&va, (size_t)top * sizeof(float));
  if (e != hipSuccess) {
    *oom = e == hipErrorOutOfMemory;
    if (*oom) (void)hipGetLastError();  // the runtime's sticky copy of this error
    return bail(e, "memo build: allocation");
  }
  e = hipMemcpyAsync(dobs, obs.data(), obs.size() * sizeof(float), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemsetAsync(rw, 0, (size_t)ST * sizeof(float), stream);  // a root has no reward
  if (e == hipSuccess && cap > 0)  // every link MZH_LINK_NONE, no row in use
    e = hipMemsetAsync(eng->memo_link, 0, (size_t)(rows + cap) * 6 * sizeof(int32_t), stream);
  if (e == hipSuccess && cap > 0) e = hipMemsetAsync(eng->memo_ctr, 0, 2 * sizeof(int32_t), stream);
  if (e != hipSuccess) return bail(e, "memo build: upload");
  // the level's outputs go to hcur; levels alternate between hA and hB so that the deepest lands in hA
  float* hcur = (D % 2 == 0) ? hA : hB;
  float* hprev = (D % 2 == 0) ? hB : hA;
  long long n = ST, first = 0, per_state = 1;
  for (int d = 0; d <= D; ++d) {
    MzhInferParams p{};
    p.B = (int)n; p.in_dim = in; p.kin = eng->kin; p.h = hcur; p.pi = pi; p.value = va;
    if (d == 0) {
      p.x = dobs;
    } else {
      e = mzh_launch_memo_level(hprev, xin, act, n, stream);
      if (e != hipSuccess) return bail(e, "memo build: level input");
      p.x = xin; p.action = act; p.reward = rw;
    }
    e = mzh_launch_infer(pick_rows((int)n), d > 0, eng->net, p, stream);
    if (e == hipSuccess) e = mzh_launch_memo_scatter(hcur, pi, rw, va, n, per_state, K, first, eng->memo_h, eng->memo_rec, stream);
    if (e != hipSuccess) return bail(e, "memo build: level");
    first += per_state;
    per_state *= 6;
    n *= 6;
    float* t = hcur; hcur = hprev; hprev = t;
  }
  e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return bail(e, "memo build: run");
  release();
  eng->memo_D = D;
  eng->memo_base = rows;
  eng->memo_cap = cap;
  // what the building search call paid: allocations, the fill, the wait and the frees, on the host's clock
  eng->memo_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  return MZH_OK;
}

// the memo of a wave MLP search: built on first use, rebuilt when the wanted depth changed.  A forced depth
// whose build fails is the call's error.  The automatic depth is an optimisation the caller did not ask for:
// when its table or the build's temporaries do not fit the device's free memory, the next shallower one is
// tried, down to no memo, and later searches keep that depth (mzh_set_memo_depth lifts the ceiling)
static int memo_ensure(mzh_engine* eng, hipStream_t stream) {
  for (;;) {
    int D = 0;
    const int st = memo_effective_depth(eng, &D);
    if (st) return st;
    if (D == eng->memo_D && (D == 0 || eng->memo_cap == memo_grow_cap(eng, eng->memo_base))) return MZH_OK;
    if (D == 0) {
      HIP_OK(memo_drop(eng));
      return MZH_OK;
    }
    bool oom = false;
    const int bs = memo_build(eng, D, stream, &oom);
    if (bs == MZH_OK || eng->memo_want >= 0 || !oom) return bs;
    eng->memo_auto_cap = D - 1;
  }
}

// the per-root miss log of the grown extension: workspace for max_roots roots at the engine's log cap
static int memo_log_ensure(mzh_engine* eng) {
  if (eng->memo_log && eng->memo_log_cap == eng->log_cap) return MZH_OK;
  if ((long long)eng->max_roots * eng->log_cap >= (1ll << 31))  // the kernel indexes entries in 32 bits
    return fail(MZH_ERR_CAPACITY, "memo miss log: %d roots x %d entries", eng->max_roots, eng->log_cap);
  if (eng->memo_log) {
    ++eng->n_wait;
    HIP_OK(hipDeviceSynchronize());
    (void)hipFree(eng->memo_log);
    eng->memo_log = nullptr;
  }
  HIP_OK(hipMalloc(&eng->memo_log, (size_t)eng->max_roots * eng->log_cap * sizeof(uint4)));
  eng->memo_log_cap = eng->log_cap;
  if (!eng->memo_logn) {
    HIP_OK(hipMalloc(&eng->memo_logn, (size_t)eng->max_roots * sizeof(int32_t)));
    HIP_OK(hipMemset(eng->memo_logn, 0, (size_t)eng->max_roots * sizeof(int32_t)));
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
  eng->grow_want = budget_bytes;
  eng->log_cap = log_entries < 0 ? MZH_MEMO_LOG_CAP : log_entries;
  return MZH_OK;
}

extern "C" int mzh_memo_grow_stats(mzh_engine* eng, mzh_memo_grow_info* out) {
  if (!eng || !out) return fail(MZH_ERR_ARG, "memo_grow_stats: engine or out NULL");
  memset(out, 0, sizeof(*out));
  out->budget_bytes = eng->grow_want < 0 ? MZH_MEMO_GROW_BUDGET_BYTES : eng->grow_want;
  out->log_entries = eng->log_cap;
  out->capacity_rows = eng->memo_cap;
  if (eng->memo_cap == 0) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  int32_t c[2] = {0, 0};
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(c, eng->memo_ctr, sizeof(c), hipMemcpyDeviceToHost));
  out->rows_used = c[0];
  out->rows_last_harvest = c[0] - c[1];
  return MZH_OK;
}

extern "C" int mzh_memo_debug_grow(mzh_engine* eng, float* latent, float* record, int32_t* link, int64_t* rows_used,
                                   int64_t* dense_rows, int64_t* capacity_rows) {
  if (!eng || !rows_used || !dense_rows || !capacity_rows) return fail(MZH_ERR_ARG, "memo_debug_grow: NULL argument");
  *rows_used = 0;
  *dense_rows = eng->memo_base;
  *capacity_rows = eng->memo_cap;
  if (eng->memo_cap == 0) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  int32_t used = 0;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&used, eng->memo_ctr, sizeof(used), hipMemcpyDeviceToHost));
  *rows_used = used;
  const size_t b = (size_t)eng->memo_base, n = (size_t)eng->memo_cap;
  if (latent) HIP_OK(hipMemcpy(latent, eng->memo_h + b * MZH_LATENT, n * MZH_LATENT * sizeof(float), hipMemcpyDeviceToDevice));
  if (record) HIP_OK(hipMemcpy(record, eng->memo_rec + b * 8, n * 8 * sizeof(float), hipMemcpyDeviceToDevice));
  if (link) HIP_OK(hipMemcpy(link, eng->memo_link, (b + n) * 6 * sizeof(int32_t), hipMemcpyDeviceToDevice));
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
  out->built = (D > 0 && eng->memo_D == D) ? 1 : 0;
  out->rows = D > 0 ? mzh_memo_states(eng->n_disks) * mzh_memo_nodes(D) : 0;
  out->table_bytes = out->rows * MZH_MEMO_ROW_BYTES;
  out->build_ms = eng->memo_build_ms;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  unsigned long long c[3] = {0, 0, 0};
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(c, eng->memo_cnt, sizeof(c), hipMemcpyDeviceToHost));
  out->pairs_skipped = c[0];
  out->pairs_packed = c[1];
  out->pairs_full = c[2];
  return MZH_OK;
}

extern "C" int mzh_memo_debug_table(mzh_engine* eng, float* latent, float* record, int64_t* rows, int32_t* depth) {
  if (!eng || !rows || !depth) return fail(MZH_ERR_ARG, "memo_debug_table: NULL argument");
  const long long n = eng->memo_D > 0 ? mzh_memo_states(eng->n_disks) * mzh_memo_nodes(eng->memo_D) : 0;
  *rows = n;
  *depth = eng->memo_D;
  if (n == 0 || (!latent && !record)) return MZH_OK;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  HIP_OK(hipDeviceSynchronize());
  if (latent) HIP_OK(hipMemcpy(latent, eng->memo_h, (size_t)n * MZH_LATENT * sizeof(float), hipMemcpyDeviceToDevice));
  if (record) HIP_OK(hipMemcpy(record, eng->memo_rec, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToDevice));
  HIP_OK(hipDeviceSynchronize());
  return MZH_OK;
}

// What mzh_search, mzh_search_replay and mzh_search_multi (single = false: it needs no engine network) refuse of a
// search's arguments, in this order.  *launch = false with MZH_OK: B = 0, nothing launches and the plan says so (a
// caller naming the kernel sees "none").
static int search_args_check(const mzh_engine* eng, const mzh_search_args* a, bool replay, bool single, bool* launch) {
  *launch = false;
  if (a->B < 0 || a->n_sims < 0) return fail(MZH_ERR_ARG, "B=%d n_sims=%d", a->B, a->n_sims);
  if (a->B > eng->max_roots) return fail(MZH_ERR_CAPACITY, "B=%d > max_roots=%d", a->B, eng->max_roots);
  if (a->n_sims > eng->max_sims) return fail(MZH_ERR_CAPACITY, "n_sims=%d > max_sims=%d", a->n_sims, eng->max_sims);
  if (!(a->temperature >= 0.0 && a->temperature <= 1.0))
    return fail(MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0], got %g", a->temperature);
  if (a->B == 0) {
    if (a->plan_out) {
      memset(a->plan_out, 0, sizeof(*a->plan_out));
      snprintf(a->plan_out->kernel, sizeof(a->plan_out->kernel), "none");
    }
    return MZH_OK;
  }
  if (!a->visits) return fail(MZH_ERR_ARG, "visits output is required");
  if (replay) {
    if (!a->rp_root_pi || (a->n_sims > 0 && !a->rp_sim))
      return fail(MZH_ERR_ARG, "replay search needs rp_root_pi and rp_sim");
  } else {
    if (single && !eng->loaded) return fail(MZH_ERR_STATE, "weights not loaded");
    if (!a->obs) return fail(MZH_ERR_ARG, "obs is required");
  }
  if (!a->deterministic && !a->action_u && a->action)
    return fail(MZH_ERR_ARG, "stochastic action selection needs action_u");
  *launch = true;
  return MZH_OK;
}

// the device side of a call's mzh_multi_args: the caller's net_index and status, the engine's tile workspace and set
static MzhMultiParams multi_params(const mzh_engine* eng, const mzh_multi_args* m) {
  MzhMultiParams mp{};
  mp.net_index = m->net_index;
  mp.M = m->n_networks;
  mp.tiles = eng->mtiles;
  mp.ntiles = eng->mntiles;
  mp.status = m->status;
  mp.stride = eng->set_stride;
  mp.scal = eng->set_scal;
  return mp;
}

static int search_common(mzh_engine* eng, const mzh_search_args* a, mzh_stream stream, bool replay) {
  if (!eng || !a) return fail(MZH_ERR_ARG, "engine or args NULL");
  bool launch;
  const int ck = search_args_check(eng, a, replay, true, &launch);
  if (!launch) return ck;
  MzhSearchPlan pl;
  const int st = make_plan(a->B, a->n_sims, a->flags, replay, eng->support, a->minmax_in != nullptr, &pl);
  if (st) return st;
  if (a->plan_out) plan_info(pl, a->B, a->n_sims, a->plan_out);
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhSearchParams p = search_params(eng, a);
  bool harvest = false;
  if (pl.wave && !replay) {  // the expansion memo: wave MLP searches only, built on first use
    const int ms = memo_ensure(eng, (hipStream_t)stream);
    if (ms) return ms;
    if (eng->memo_D > 0) {
      p.memo_h = eng->memo_h; p.memo_rec = eng->memo_rec; p.memo_cnt = eng->memo_cnt;
      p.memo_D = eng->memo_D; p.memo_K = (int)mzh_memo_nodes(eng->memo_D);
      if (eng->memo_cap > 0) {  // the grown extension: its links, and the miss log the harvest below reads
        const int ls = memo_log_ensure(eng);
        if (ls) return ls;
        p.memo_link = eng->memo_link; p.memo_ctr = eng->memo_ctr; p.memo_cap = (int)eng->memo_cap;
        p.memo_log = eng->memo_log; p.memo_logn = eng->memo_logn; p.memo_logcap = eng->memo_log_cap;
        harvest = true;
      }
    }
  }
  hipError_t e = pl.one ? mzh_launch_one(pl, eng->net, eng->onet, p, (hipStream_t)stream)
                 : pl.wave ? mzh_launch_wave_search(pl, eng->wnet, p, (hipStream_t)stream)
                           : mzh_launch_search(pl, eng->net, p, (hipStream_t)stream);
  if (e == hipSuccess && harvest) {
    MzhHarvestParams h{};
    h.B = p.B; h.E = p.E; h.tree = p.tree; h.htree = p.htree;
    h.log = p.memo_log; h.logn = p.memo_logn; h.logcap = p.memo_logcap;
    h.link = eng->memo_link; h.ctr = eng->memo_ctr; h.base = (int)eng->memo_base; h.cap = (int)eng->memo_cap;
    h.memo_h = eng->memo_h; h.memo_rec = eng->memo_rec;
    e = mzh_launch_memo_harvest(h, (hipStream_t)stream);
  }
  return e == hipSuccess ? MZH_OK : hip_fail(e, "search launch");
}

extern "C" int mzh_search(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream) {
  return search_common(eng, args, stream, false);
}

extern "C" int mzh_search_replay(mzh_engine* eng, const mzh_search_args* args, mzh_stream stream) {
  return search_common(eng, args, stream, true);
}

// Search over the loaded network set: root b under network net_index[b].  Cooperative kernel only (16- or
// 32-root tiles of one network each); every refusal below returns before anything is launched.
// b: the roots' own budgets (mzh_search_multi_budget), nullptr where every root runs a->n_sims
static int search_multi_common(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m, const mzh_budget_args* b,
                               mzh_stream stream) {
  if (!eng || !a || !m) return fail(MZH_ERR_ARG, "engine or args NULL");
  if (eng->set_m == 0) return fail(MZH_ERR_STATE, "no weight set loaded (mzh_load_weight_set)");
  if (m->n_networks < 1 || m->n_networks > eng->set_m)
    return fail(MZH_ERR_ARG, "n_networks=%d outside [1, %d], the loaded set", m->n_networks, eng->set_m);
  if (!m->net_index) return fail(MZH_ERR_ARG, "net_index is NULL");
  if (a->rp_sim || a->rp_root_pi) return fail(MZH_ERR_ARG, "a multi-network search has no replay (tree-only) form");
  if (a->flags & (MZH_FLAG_KERNEL_WAVE | MZH_FLAG_KERNEL_WAVE16 | MZH_FLAG_KERNEL_ONE | MZH_FLAG_COOP_OCC2))
    return fail(MZH_ERR_ARG, "a multi-network search runs the cooperative kernel only (flags=0x%x)", a->flags);
  bool launch;
  const int ck = search_args_check(eng, a, false, false, &launch);
  if (!launch) return ck;
  const int S = a->n_sims;
  MzhSearchPlan pl{};
  pl.R = pick_tile(a->B, a->flags);
  if (mzh_search_smem_bytes(pl.R, S, false) > kMaxLds) pl.R = 16;
  if (mzh_search_smem_bytes(pl.R, S, false) > kMaxLds)
    return fail(MZH_ERR_CAPACITY, "n_sims=%d exceeds the LDS path budget", S);
  pl.ohl = mzh_search_smem_bytes(pl.R, S, true) <= kMaxLds;
  pl.sup33 = eng->support == 33;
  pl.mmin = 1;
  // the tile workspace holds the tiles of max_roots roots of MZH_MULTI_MAX_NETS networks at 16 roots each
  const int cap = mzh_multi_max_tiles(eng->max_roots, 16, MZH_MULTI_MAX_NETS);
  // the grid: the most tiles the batch can make, its runs (at most max_runs) in place of the networks with budgets
  const int runs = b ? b->max_runs : m->n_networks;
  const int grid = mzh_multi_max_tiles(a->B, pl.R, runs);
  if (grid > cap)
    return fail(MZH_ERR_CAPACITY, "max_runs=%d: up to %d tiles of %d roots exceed the tile workspace (%d)", runs, grid,
                pl.R, cap);
  if (a->plan_out) {
    const char* tf[2] = {"false", "true"};
    mzh_search_plan* o = a->plan_out;
    memset(o, 0, sizeof(*o));
    o->roots_per_wave = pl.R / 4;
    o->threads_per_workgroup = MZH_THREADS;
    o->roots_per_workgroup = pl.R;
    o->smem_bytes = (int64_t)mzh_search_smem_bytes(pl.R, S, pl.ohl);
    o->workgroups = grid;
    snprintf(o->kernel, sizeof(o->kernel), "mzh_search_multi_kernel<%d, %s, %s>", pl.R, tf[pl.ohl], tf[pl.sup33]);
  }
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  const MzhSearchParams p = search_params(eng, a);
  hipError_t e;
  if (b) {
    MzhBudgetParams bp{};
    bp.n_sims = b->n_sims;
    bp.S = S;
    bp.max_runs = b->max_runs < a->B ? b->max_runs : a->B;
    bp.cap = cap;
    e = mzh_launch_search_multi_budget(pl, eng->setnet, p, multi_params(eng, m), bp, (hipStream_t)stream);
  } else {
    e = mzh_launch_search_multi(pl, eng->setnet, p, multi_params(eng, m), (hipStream_t)stream);
  }
  return e == hipSuccess ? MZH_OK : hip_fail(e, "multi search launch");
}

extern "C" int mzh_search_multi(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m, mzh_stream stream) {
  return search_multi_common(eng, a, m, nullptr, stream);
}

// The same search with root b running budget->n_sims[b] simulations (at most a->n_sims, which sizes the launch).
// What the budget block alone decides is refused first: those refusals need neither an engine nor a device.
extern "C" int mzh_search_multi_budget(mzh_engine* eng, const mzh_search_args* a, const mzh_multi_args* m,
                                       const mzh_budget_args* b, mzh_stream stream) {
  if (!a || !m || !b) return fail(MZH_ERR_ARG, "search_multi_budget: args, multi or budget NULL");
  if (!b->n_sims) return fail(MZH_ERR_ARG, "search_multi_budget: n_sims is NULL");
  if (b->max_runs < 1) return fail(MZH_ERR_ARG, "search_multi_budget: max_runs=%d < 1", b->max_runs);
  return search_multi_common(eng, a, m, b, stream);
}

// ---- the calls over rows of a sub-batch: mzh_probe_actions, mzh_saliency, mzh_param_grads ----
// What all three refuse, in this order: what the arguments alone decide first (those refusals need neither a device
// nor an engine), then the engine, its weights or set, its capacity.  `who` prefixes the text; have / need: whether
// the call's required buffers are there, and their names.
static int rows_check(const char* who, int B, int n, const int32_t* env_index, uint32_t flags, bool have, const char* need,
                      const mzh_multi_args* m, const mzh_engine* eng) {
  if (n < 1 || B < 1 || (!env_index && B < n)) return fail(MZH_ERR_ARG, "%s: bad n=%d rows for B=%d envs", who, n, B);
  if (!have) return fail(MZH_ERR_ARG, "%s: required buffer is NULL (%s)", who, need);
  if (flags & ~(MZH_FLAG_COOP_TILE16 | MZH_FLAG_COOP_TILE32))
    return fail(MZH_ERR_ARG, "%s: flags=0x%x, only MZH_FLAG_COOP_TILE16 / 32 apply", who, flags);
  if (m) {
    if (!m->net_index) return fail(MZH_ERR_ARG, "%s: net_index is NULL", who);
    if (m->n_networks < 1 || m->n_networks > MZH_MULTI_MAX_NETS)
      return fail(MZH_ERR_ARG, "%s: n_networks=%d outside [1, %d]", who, m->n_networks, MZH_MULTI_MAX_NETS);
  }
  if (!eng) return fail(MZH_ERR_ARG, "%s: engine NULL", who);
  if (m) {
    if (eng->set_m == 0) return fail(MZH_ERR_STATE, "no weight set loaded (mzh_load_weight_set)");
    if (m->n_networks > eng->set_m)
      return fail(MZH_ERR_ARG, "%s: n_networks=%d outside [1, %d], the loaded set", who, m->n_networks, eng->set_m);
  } else if (!eng->loaded) {
    return fail(MZH_ERR_STATE, "weights not loaded");
  }
  if (n > eng->max_roots) return fail(MZH_ERR_CAPACITY, "%s: n=%d > max_roots=%d", who, n, eng->max_roots);
  return MZH_OK;
}

// the fields every row call's parameter block starts with (mzh_probe_args, mzh_saliency_args, mzh_pgrad_args)
template <class P, class ARGS>
static void row_params(P& p, const mzh_engine* eng, const ARGS* a) {
  p.B = a->B; p.n = a->n; p.in_dim = eng->in_dim; p.kin = eng->kin; p.n_disks = eng->n_disks;
  p.env_index = a->env_index; p.obs = a->obs; p.err_count = a->err_count;
}

// The six one-step lookaheads of a batch of roots in one launch (mzh_probe_kernel; with `m` the rows of a loaded
// network set, mzh_probe_multi_kernel)
extern "C" int mzh_probe_actions(mzh_engine* eng, const mzh_probe_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "probe_actions: args is NULL");
  const int st = rows_check("probe_actions", a->B, a->n, a->env_index, a->flags,
                            a->obs && a->reward && a->value && (!a->legal || a->state),
                            "obs, reward, value; state for legal", m, eng);
  if (st) return st;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhProbeParams p{};
  row_params(p, eng, a);
  p.state = a->state; p.reward = a->reward; p.value = a->value;
  p.legal = a->legal; p.h0 = a->h0; p.pi0 = a->pi0; p.value0 = a->value0; p.h1 = a->h1; p.pi1 = a->pi1;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  hipError_t e = mzh_launch_probe(pick_tile(a->n, a->flags), m ? eng->setnet : eng->net, p, m ? &mp : nullptr, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "probe_actions launch");
}

// Input saliency of the policy and value heads of a batch of rows in one launch (mzh_saliency_kernel; with `m` the
// rows of a loaded network set, mzh_saliency_multi_kernel)
extern "C" int mzh_saliency(mzh_engine* eng, const mzh_saliency_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "saliency: args is NULL");
  const int st = rows_check("saliency", a->B, a->n, a->env_index, a->flags, a->obs && a->sal_policy && a->sal_value,
                            "obs, sal_policy, sal_value", m, eng);
  if (st) return st;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhSalParams p{};
  row_params(p, eng, a);
  p.logit_index = a->logit_index;
  p.sal_policy = a->sal_policy; p.sal_value = a->sal_value; p.picked = a->picked;
  p.disc_policy = a->disc_policy; p.disc_value = a->disc_value;
  p.h0 = a->h0; p.pi0 = a->pi0; p.value0 = a->value0;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  hipError_t e = mzh_launch_saliency(pick_tile(a->n, a->flags), m ? eng->setnet : eng->net, m ? eng->settnet : eng->tnet, p,
                                     m ? &mp : nullptr, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "saliency launch");
}

// the MzhPackedG buffer of the loaded network (set = false) or set, current for the loaded weights: the map once
// per engine, the buffer once per size, the gather once per load, on `stream` ahead of the kernel that reads it
static int pgrad_ensure(mzh_engine* eng, bool set, hipStream_t stream) {
  if (set ? eng->setg_valid : eng->g_valid) return MZH_OK;
  if (!eng->gmaps) {
    MzhPgradMap* m = new MzhPgradMap();
    if (!mzh_pgrad_map(eng->in_dim, eng->support, m)) {
      delete m;
      return fail(MZH_ERR_STATE, "param_grads: no gather map for this shape");
    }
    eng->gmaps = m;
  }
  const MzhPgradMap& gm = *eng->gmaps;
  const size_t n = gm.src.size();
  // every source lies inside one network's main blob: the gather's reads stay in bounds
  const size_t blob = set ? eng->set_stride / sizeof(float) : eng->wn;
  for (size_t j = 0; j < n; ++j)
    if (gm.src[j] >= 0 && (size_t)gm.src[j] >= blob) return fail(MZH_ERR_STATE, "param_grads: gather map entry %zu out of range", j);
  if (!eng->gmap) {
    int32_t* d = nullptr;
    HIP_OK(hipMalloc(&d, n * sizeof(int32_t)));
    hipError_t e = hipMemcpy(d, gm.src.data(), n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e, "hipMemcpy (gather map)");
    }
    eng->gmap = d;
    eng->gstride = (n + 63) & ~(size_t)63;
  }
  if (!set) {
    if (!eng->gbuf) HIP_OK(hipMalloc(&eng->gbuf, eng->gstride * sizeof(float)));
    hipError_t e = mzh_launch_pgrad_gather(eng->gmap, (int)n, static_cast<const float*>(eng->wbuf), 0, eng->gbuf, 0, 1, stream);
    if (e != hipSuccess) return hip_fail(e, "param_grads gather launch");
    eng->g_valid = true;
    return MZH_OK;
  }
  if (eng->setgbuf && eng->setg_m != eng->set_m) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(eng->setgbuf));
    eng->setgbuf = nullptr;
  }
  if (!eng->setgbuf) {
    HIP_OK(hipMalloc(&eng->setgbuf, (size_t)eng->set_m * eng->gstride * sizeof(float)));
    eng->setg_m = eng->set_m;
  }
  hipError_t e = mzh_launch_pgrad_gather(eng->gmap, (int)n, static_cast<const float*>(eng->setbuf),
                                         eng->set_stride / sizeof(float), eng->setgbuf, eng->gstride, eng->set_m, stream);
  if (e != hipSuccess) return hip_fail(e, "param_grads gather launch");
  eng->setg_valid = true;
  return MZH_OK;
}

// Parameter gradients of the five sub-networks of a batch of rows (mzh_pgrad_kernel; with `m` the rows of a loaded
// network set, mzh_pgrad_multi_kernel; with args.grad then mzh_pgrad_expand_kernel)
extern "C" int mzh_param_grads(mzh_engine* eng, const mzh_pgrad_args* a, const mzh_multi_args* m, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "param_grads: args is NULL");
  int st = rows_check("param_grads", a->B, a->n, a->env_index, a->flags,
                      a->obs && a->action && a->delta1 && a->delta2 && a->act && a->h0 && a->z1,
                      "obs, action, delta1, delta2, act, h0, z1", m, eng);
  if (st) return st;
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  st = pgrad_ensure(eng, m != nullptr, (hipStream_t)stream);
  if (st) return st;
  MzhPgNetT gt{};
  gt.base = reinterpret_cast<const float4*>(m ? eng->setgbuf : eng->gbuf);
  for (int i = 0; i < MZH_G_LAYERS; ++i) gt.off[i] = (int)(eng->gmaps->layout.off[i] / 4);
  gt.kb_rwd2 = eng->gmaps->layout.kb[MZH_G_RWD2];
  gt.stride = eng->gstride * sizeof(float);
  MzhPgradParams p{};
  row_params(p, eng, a);
  p.action = a->action; p.policy_logit = a->policy_logit;
  p.delta1 = a->delta1; p.delta2 = a->delta2; p.act = a->act; p.h0 = a->h0; p.z1 = a->z1; p.h1 = a->h1;
  p.pi0 = a->pi0; p.value0 = a->value0; p.reward = a->reward; p.objective = a->objective; p.grad = a->grad;
  const MzhMultiParams mp = m ? multi_params(eng, m) : MzhMultiParams{};
  hipError_t e = mzh_launch_pgrad(pick_tile(a->n, a->flags), m ? eng->setnet : eng->net, m ? eng->settnet : eng->tnet, gt, p,
                                  eng->support, m ? &mp : nullptr, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "param_grads launch");
}

// ---------------------------------------------------------------------------------------------
// fused training update (mzh_train.hip)
namespace {
struct TrainLayout {
  size_t off[22];
  size_t total;  // floats
};
// scratch regions in MztScratch order, each 256-B aligned
TrainLayout train_layout(int B, int U, int support) {
  const size_t BU = (size_t)B * U, ldg = support > 1 ? 48 : 16;
  const size_t sz[] = {(size_t)B * 32, (size_t)B * 256, BU * 64, BU * 256, BU * 256, BU * 256, BU * 256, BU * 64,
                       (size_t)B * 256, (size_t)B * 64, BU * 256, BU * 256, BU * 256, BU * 256, BU * 16, BU * ldg,
                       BU * ldg, BU * 64};
  TrainLayout L{};
  size_t o = 0;
  for (int i = 0; i < 18; ++i) {
    L.off[i] = o;
    o += (sz[i] + 63) & ~(size_t)63;
  }
  L.total = o;
  return L;
}
int train_rows(const mzh_train_args* a) {
  if (a->rows > 0) return a->rows;
  const char* env = getenv("MZH_TRAIN_ROWS");
  if (env) return atoi(env);
  return 1;  // one transition per workgroup: B workgroups (fastest at batch 256, MI355X)
}
}  // namespace

extern "C" int mzh_train_scratch_bytes(int B, int U, int in_dim, int support, size_t* bytes) {
  if (B < 1 || U < 1 || in_dim < 1 || in_dim > 32 || (support != 1 && support != 33) || !bytes)
    return fail(MZH_ERR_ARG, "train_scratch_bytes: bad B=%d U=%d in_dim=%d support=%d", B, U, in_dim, support);
  *bytes = train_layout(B, U, support).total * sizeof(float);
  return MZH_OK;
}

static int train_check(const mzh_train_args* a, bool need_batch) {
  if (!a) return fail(MZH_ERR_ARG, "train: null args");
  if (a->B < 1 || a->U < 1 || a->in_dim < 1 || a->in_dim > 32 || (a->support != 1 && a->support != 33))
    return fail(MZH_ERR_ARG, "train: bad B=%d U=%d in_dim=%d support=%d", a->B, a->U, a->in_dim, a->support);
  for (int i = 0; i < 20; ++i)
    if (!a->param[i] || (need_batch && (!a->exp_avg[i] || !a->exp_avg_sq[i])))
      return fail(MZH_ERR_ARG, "train: null parameter / Adam state pointer %d", i);
  for (int i = 0; i < 10; ++i)
    if (!a->wt[i]) return fail(MZH_ERR_ARG, "train: null transposed weight %d", i);
  if (!need_batch) return MZH_OK;
  if (!a->obs || !a->rwds || !a->actions || !a->pi || !a->returns || !a->row_loss || !a->scratch)
    return fail(MZH_ERR_ARG, "train: null batch / output / scratch pointer");
  if (a->scratch_bytes < train_layout(a->B, a->U, a->support).total * sizeof(float))
    return fail(MZH_ERR_ARG, "train: scratch of %zu bytes is too small", a->scratch_bytes);
  const int R = train_rows(a);
  if (R != 1 && R != 2) return fail(MZH_ERR_ARG, "train: rows must be 1 or 2 (got %d)", R);
  if (R * a->U > 64) return fail(MZH_ERR_ARG, "train: rows * U = %d exceeds 64", R * a->U);
  if (mzt_rows_smem_bytes(R, a->U) > 160 * 1024)
    return fail(MZH_ERR_ARG, "train: U=%d needs %zu B of LDS at rows=%d", a->U, mzt_rows_smem_bytes(R, a->U), R);
  return MZH_OK;
}

extern "C" int mzh_train_transpose(const mzh_train_args* a, mzh_stream stream) {
  int st = train_check(a, false);
  if (st) return st;
  const MzhCanon dims = mzh_canon_view(nullptr, a->in_dim, a->support);
  for (int l = 0; l < 10; ++l) {
    const int out = dims.out[l], in = dims.in[l];
    hipError_t e = mzt_launch_transpose(a->param[2 * l], a->wt[l], out, in, (out + 3) & ~3, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "train transpose launch");
  }
  return MZH_OK;
}

// The two kernels' parameter blocks of one network, from its mzh_train_args (mzh_train_update launches with
// them; a set keeps them in its device table).  Returns the gradient kernel's tile count.
static int train_params(const mzh_train_args* a, MztRowParams* rp_out, MztGradParams* gp_out) {
  const int B = a->B, U = a->U, SUP = a->support;
  const TrainLayout lay = train_layout(B, U, SUP);
  float* base = (float*)a->scratch;
  MztScratch s;
  float** regions[] = {&s.x0, &s.repa, &s.h, &s.ap, &s.av, &s.ad, &s.ar, &s.hp, &s.g_rep, &s.g_h0p,
                       &s.g_p, &s.g_v, &s.g_d, &s.g_r, &s.g_lp, &s.g_lv, &s.g_lr, &s.g_hp};
  for (int i = 0; i < 18; ++i) *regions[i] = base + lay.off[i];

  float* const* P = a->param;
  MztRowParams& rp = *rp_out;
  rp.B = B;
  rp.U = U;
  rp.in_dim = a->in_dim;
  rp.obs = a->obs;
  rp.rwds = a->rwds;
  rp.pi = a->pi;
  rp.returns = a->returns;
  rp.w = a->weights;
  rp.actions = a->actions;
  rp.row_loss = a->row_loss;
  rp.new_prio = a->new_prio;
  float* const* T = a->wt;
  rp.n = MztNet{P[0],  T[0], P[1],  P[2],  T[1], P[3],  P[4],  T[2], P[5],  P[6],  T[3], P[7],
                P[8],  T[4], P[9],  P[10], T[5], P[11], P[12], T[6], P[13], P[14], T[7], P[15],
                P[16], T[8], P[17], P[18], T[9], P[19]};
  rp.s = s;

  const int BU = B * U, ldg = SUP > 1 ? 48 : 16;
  // the training-scratch facts of each layer, MztGradLayer's leading {X, ldx, GY, ldg, M}; the layer shapes
  // come from the network's table (mzh_pack.h)
  MztGradParams& gp = *gp_out;
  gp = {{{s.x0, 32, s.g_rep, 256, B},  {s.repa, 256, s.g_h0p, 64, B}, {s.h, 64, s.g_d, 256, BU},
         {s.ad, 256, s.g_hp, 64, BU},  {s.hp, 64, s.g_r, 256, BU},    {s.ar, 256, s.g_lr, ldg, BU},
         {s.h, 64, s.g_p, 256, BU},    {s.ap, 256, s.g_lp, 16, BU},   {s.h, 64, s.g_v, 256, BU},
         {s.av, 256, s.g_lv, ldg, BU}}};
  const MzhCanon dims = mzh_canon_view(nullptr, a->in_dim, SUP);
  int tiles = 0;
  for (int l = 0; l < 10; ++l) {
    MztGradLayer& L = gp.L[l];
    L.out = dims.out[l];
    L.in = dims.in[l];
    L.onehot_from = l == MZH_DYN0 ? MZH_LATENT : -1;
    L.nkb = (L.in + 15) / 16;
    L.tile0 = tiles;
    tiles += ((L.out + 15) / 16) * L.nkb;
    L.W = a->param[2 * l]; L.b = a->param[2 * l + 1];
    L.mW = a->exp_avg[2 * l]; L.mb = a->exp_avg[2 * l + 1];
    L.vW = a->exp_avg_sq[2 * l]; L.vb = a->exp_avg_sq[2 * l + 1];
    L.WT = a->wt[l];
    L.ldwt = (L.out + 3) & ~3;
  }
  gp.actions = a->actions;
  gp.step_size = a->step_size;
  gp.bc2_sqrt = a->bc2_sqrt;
  gp.beta1 = a->beta1;
  gp.beta2 = a->beta2;
  gp.eps = a->eps;
  return tiles;
}

extern "C" int mzh_train_update(const mzh_train_args* a, mzh_stream stream) {
  int st = train_check(a, true);
  if (st) return st;
  MztRowParams rp;
  MztGradParams gp;
  const int tiles = train_params(a, &rp, &gp);
  hipError_t e = mzt_launch_rows(train_rows(a), a->support, rp, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "train rows kernel launch");
  e = mzt_launch_grad_adam(gp, tiles, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "train grad/adam kernel launch");
}

// what mzh_replay_sample refuses of its arguments; per_call: n, u and status as well (a set takes them per round)
static int replay_check(const mzh_replay_args* a, bool per_call) {
  if (!a) return fail(MZH_ERR_ARG, "replay_sample: null args");
  if (a->n < 1 || a->m < 1 || a->m > MZR_MAX_BATCH || a->d_state < 1 || a->U < 1 || a->A < 1)
    return fail(MZH_ERR_ARG, "replay_sample: bad n=%d m=%d (1..%d) d_state=%d U=%d A=%d", a->n, a->m, MZR_MAX_BATCH,
                a->d_state, a->U, a->A);
  if (!a->prio || !a->cdf || !a->states || !a->rwds || !a->actions || !a->pi || !a->returns || !a->indx ||
      !a->out_states || !a->out_rwds || !a->out_actions || !a->out_pi || !a->out_returns ||
      (per_call && (!a->u || !a->status)))
    return fail(MZH_ERR_ARG, "replay_sample: null pointer");
  if (reinterpret_cast<uintptr_t>(a->prio) % 16 != 0)
    return fail(MZH_ERR_ARG, "replay_sample: prio must be 16-byte aligned (float4 loads)");
  return MZH_OK;
}

extern "C" int mzh_replay_sample(const mzh_replay_args* a, mzh_stream stream) {
  const int st = replay_check(a, true);
  if (st) return st;
  hipError_t e = mzr_launch_sample(*a, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "replay sample launch");
}

extern "C" int mzh_replay_set_priorities(float* prio, int64_t size, const int64_t* indx, const float* values, int m,
                                         int32_t* status, mzh_stream stream) {
  if (!prio || !indx || !values || !status || size < 1 || m < 1)
    return fail(MZH_ERR_ARG, "replay_set_priorities: bad arguments (size=%lld m=%d)", (long long)size, m);
  hipError_t e = mzr_launch_set_priorities(prio, size, indx, values, m, status, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "replay set_priorities launch");
}

// ---------------------------------------------------------------------------------------------
// one update round of a network set in four launches (mzh.h: mzh_train_set_*)
struct mzh_train_set {
  int device = 0;
  int M = 0, B = 0, U = 0, support = 0, rows = 0, tiles = 0;
  std::vector<int32_t> ring;  // each network's ring size: the bound of a round's n
  void* table = nullptr;      // the device table: draw[M], rows[M], grad[M], prio[M], each 256-byte aligned
  MztSetParams view{};        // the table's four arrays (step, u and status come with each call)
};

extern "C" int mzh_train_set_create(const mzh_train_args* train, const mzh_replay_args* draw, int M,
                                    mzh_train_set** out) {
  if (!out) return fail(MZH_ERR_ARG, "train_set_create: out is NULL");
  *out = nullptr;
  if (!train || !draw) return fail(MZH_ERR_ARG, "train_set_create: %s is NULL", !train ? "train" : "draw");
  if (M < 1 || M > MZH_TRAIN_SET_MAX)
    return fail(MZH_ERR_ARG, "train_set_create: M=%d outside [1, %d]", M, MZH_TRAIN_SET_MAX);
  const mzh_train_args& t0 = train[0];
  for (int m = 0; m < M; ++m) {
    const mzh_train_args& t = train[m];
    const mzh_replay_args& d = draw[m];
    int st = train_check(&t, true);
    if (st == MZH_OK) st = replay_check(&d, false);
    if (st) {
      const std::string why = g_err;
      return fail(st, "train_set_create: network %d: %s", m, why.c_str());
    }
    if (!t.new_prio) return fail(MZH_ERR_ARG, "train_set_create: network %d: new_prio is NULL (the write-back's values)", m);
    const int have[] = {t.B, t.U, t.in_dim, t.support, train_rows(&t)};
    const int want[] = {t0.B, t0.U, t0.in_dim, t0.support, train_rows(&t0)};
    const char* name[] = {"B", "U", "in_dim", "support", "rows"};
    for (int i = 0; i < 5; ++i)
      if (have[i] != want[i])
        return fail(MZH_ERR_ARG, "train_set_create: network %d: %s=%d differs from network 0's %d", m, name[i], have[i],
                    want[i]);
    if (d.m != t.B) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.m=%d != train.B=%d", m, d.m, t.B);
    if (d.d_state != t.in_dim)
      return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.d_state=%d != train.in_dim=%d", m, d.d_state, t.in_dim);
    if (d.U != t.U) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.U=%d != train.U=%d", m, d.U, t.U);
    if (d.A != 6) return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.A=%d != 6", m, d.A);
    const void* outs[] = {d.out_states, d.out_rwds, d.out_actions, d.out_pi, d.out_returns};
    const void* ins[] = {t.obs, t.rwds, t.actions, t.pi, t.returns};
    const char* on[] = {"out_states", "out_rwds", "out_actions", "out_pi", "out_returns"};
    const char* in[] = {"obs", "rwds", "actions", "pi", "returns"};
    for (int i = 0; i < 5; ++i)
      if (outs[i] != ins[i])
        return fail(MZH_ERR_ARG, "train_set_create: network %d: draw.%s is not train.%s (a network's draw feeds its own update)",
                    m, on[i], in[i]);
  }
  // ---- the device from here on
  auto* set = new mzh_train_set;
  set->M = M; set->B = t0.B; set->U = t0.U; set->support = t0.support; set->rows = train_rows(&t0);
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t o_draw = 0, o_rows = o_draw + up(M * sizeof(mzh_replay_args)), o_grad = o_rows + up(M * sizeof(MztRowParams)),
               o_prio = o_grad + up(M * sizeof(MztGradParams)), total = o_prio + up(M * sizeof(MzrPrioArgs));
  std::vector<unsigned char> host(total, 0);
  for (int m = 0; m < M; ++m) {
    mzh_replay_args d = draw[m];
    set->ring.push_back(d.n);
    d.n = 0; d.u = nullptr; d.status = nullptr;  // per call: the kernels take them from step, u and status
    memcpy(&host[o_draw + m * sizeof(d)], &d, sizeof(d));
    MztRowParams rp;
    MztGradParams gp;
    set->tiles = train_params(&train[m], &rp, &gp);
    gp.step_size = gp.bc2_sqrt = 0.f;  // per call
    memcpy(&host[o_rows + m * sizeof(rp)], &rp, sizeof(rp));
    memcpy(&host[o_grad + m * sizeof(gp)], &gp, sizeof(gp));
    const MzrPrioArgs pa{const_cast<float*>(draw[m].prio), (long long)draw[m].n, draw[m].indx, train[m].new_prio, train[m].B};
    memcpy(&host[o_prio + m * sizeof(pa)], &pa, sizeof(pa));
  }
  hipError_t e = hipGetDevice(&set->device);
  if (e == hipSuccess) e = hipMalloc(&set->table, total);
  if (e == hipSuccess) e = hipMemcpy(set->table, host.data(), total, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = mzt_rows_set_prepare(set->rows, set->support, set->U);
  if (e != hipSuccess) {
    if (set->table) (void)hipFree(set->table);
    delete set;
    return hip_fail(e, "train_set_create: device table");
  }
  unsigned char* base = (unsigned char*)set->table;
  set->view.draw = (const mzh_replay_args*)(base + o_draw);
  set->view.rows = (const MztRowParams*)(base + o_rows);
  set->view.grad = (const MztGradParams*)(base + o_grad);
  set->view.prio = (const MzrPrioArgs*)(base + o_prio);
  *out = set;
  return MZH_OK;
}

extern "C" int mzh_train_set_destroy(mzh_train_set* set) {
  if (!set) return MZH_OK;
  DeviceGuard g(set->device);
  if (set->table) (void)hipFree(set->table);
  delete set;
  return MZH_OK;
}

extern "C" int mzh_train_set_update(mzh_train_set* set, const mzh_train_set_step* step, const double* u, int32_t* status,
                                    mzh_stream stream) {
  if (!step) return fail(MZH_ERR_ARG, "train_set_update: step is NULL");
  if (!u) return fail(MZH_ERR_ARG, "train_set_update: u is NULL");
  if (!status) return fail(MZH_ERR_ARG, "train_set_update: status is NULL");
  if (!set) return fail(MZH_ERR_ARG, "train_set_update: set is NULL");
  int n_active = 0;
  for (int m = 0; m < set->M; ++m) {
    if (!step[m].active) continue;
    ++n_active;
    if (step[m].n < 1 || step[m].n > set->ring[m])
      return fail(MZH_ERR_ARG, "train_set_update: network %d: step.n=%d outside [1, %d], its ring", m, step[m].n,
                  set->ring[m]);
  }
  if (n_active == 0) return MZH_OK;
  MztSetParams v = set->view;
  v.step = step;
  v.u = u;
  v.status = status;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = mzr_launch_sample_set(set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: draw launch");
  e = mzt_launch_rows_set(set->rows, set->support, set->B, set->U, set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: rows kernel launch");
  e = mzt_launch_grad_adam_set(set->tiles, set->M, v, s);
  if (e != hipSuccess) return hip_fail(e, "train_set_update: grad/adam kernel launch");
  e = mzr_launch_set_priorities_set(set->M, v, s);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "train_set_update: set_priorities launch");
}

extern "C" int mzh_episode_ingest(const mzh_ingest_args* a, mzh_stream stream) {
  if (!a) return fail(MZH_ERR_ARG, "episode_ingest: null args");
  if (a->B < 1 || a->T < 1 || a->d_state < 1 || a->U < 1 || a->A < 1 || a->n_step < 1 || a->size < 1)
    return fail(MZH_ERR_ARG, "episode_ingest: bad B=%d T=%d d_state=%d U=%d A=%d n_step=%d size=%lld (each >= 1)", a->B,
                a->T, a->d_state, a->U, a->A, a->n_step, (long long)a->size);
  // the writer indexes a pass of 1,024 rows of each array with 32-bit element counts
  if (a->d_state > (1 << 20) || (int64_t)a->U * a->A > (1 << 20))
    return fail(MZH_ERR_ARG, "episode_ingest: d_state=%d / U*A=%lld above 2^20", a->d_state, (long long)a->U * a->A);
  if (a->ptr < 0 || a->ptr >= a->size)
    return fail(MZH_ERR_ARG, "episode_ingest: ptr=%lld outside [0, size=%lld)", (long long)a->ptr, (long long)a->size);
  if (!a->obs || !a->action || !a->reward || !a->pi || !a->root_q || !a->steps || !a->pad_action || !a->disc_pow ||
      !a->states || !a->rwds || !a->actions || !a->pi_probs || !a->returns || !a->prio || !a->first || !a->status)
    return fail(MZH_ERR_ARG, "episode_ingest: null pointer");
  hipError_t e = mzi_launch_ingest(*a, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "episode ingest launch");
}

// Whole episodes in one launch on the latency kernel (mzh.h): mzh_play_episodes (m == NULL, the engine's network)
// and mzh_play_episodes_multi (the loaded set).  The checks that need no engine come first.
// sweep: mzh_play_episodes_sweep, the set form with the envs' own budgets and discounts (w)
static int play_episodes_common(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m, bool multi,
                                mzh_stream stream, bool sweep = false, const mzh_episode_sweep_args* w = nullptr) {
  if (!a) return fail(MZH_ERR_ARG, "play_episodes: args is NULL");
  if (a->B < 1 || a->n_sims < 0) return fail(MZH_ERR_ARG, "play_episodes: B=%d n_sims=%d", a->B, a->n_sims);
  if (a->goal_peg < 0 || a->goal_peg > 2) return fail(MZH_ERR_ARG, "play_episodes: goal_peg=%d outside 0..2", a->goal_peg);
  if (a->max_steps < 1 || a->T < a->max_steps)
    return fail(MZH_ERR_ARG, "play_episodes: T=%d rows cannot hold max_steps=%d moves (T >= max_steps >= 1)", a->T,
                a->max_steps);
  if ((int64_t)a->T * a->B > 0x7fffffff)
    return fail(MZH_ERR_ARG, "play_episodes: T=%d x B=%d rows exceed int32", a->T, a->B);
  if (a->flags & ~MZH_FLAG_NP1_UCB)
    return fail(MZH_ERR_ARG, "play_episodes: flags=0x%x (only MZH_FLAG_NP1_UCB applies)", a->flags);
  if (!(a->temperature >= 0.0 && a->temperature <= 1.0))
    return fail(MZH_ERR_TEMPERATURE, "Expect `temperature` to be in the range [0.0, 1.0], got %g", a->temperature);
  if (!a->state || !a->tie_idx || !a->pi || !a->root_q || !a->action || !a->reward || !a->steps || !a->illegal ||
      !a->solved || !a->final_state || !a->minmax_out)
    return fail(MZH_ERR_ARG, "play_episodes: required buffer is NULL");
  if (!a->deterministic && !a->action_u) return fail(MZH_ERR_ARG, "play_episodes: stochastic action selection needs action_u");
  if (multi) {
    if (!m) return fail(MZH_ERR_ARG, "play_episodes_multi: multi is NULL");
    if (!m->net_index) return fail(MZH_ERR_ARG, "play_episodes_multi: net_index is NULL");
    if (m->n_networks < 1 || m->n_networks > MZH_MULTI_MAX_NETS)
      return fail(MZH_ERR_ARG, "play_episodes_multi: n_networks=%d outside [1, %d]", m->n_networks, MZH_MULTI_MAX_NETS);
  }
  if (sweep) {
    if (!w) return fail(MZH_ERR_ARG, "play_episodes_sweep: sweep is NULL");
    if (!w->n_sims) return fail(MZH_ERR_ARG, "play_episodes_sweep: n_sims is NULL");
  }
  if (!eng) return fail(MZH_ERR_ARG, "play_episodes: engine is NULL");
  if (a->B > eng->max_roots) return fail(MZH_ERR_CAPACITY, "play_episodes: B=%d > max_roots=%d", a->B, eng->max_roots);
  if (a->n_sims > eng->max_sims) return fail(MZH_ERR_CAPACITY, "play_episodes: n_sims=%d > max_sims=%d", a->n_sims, eng->max_sims);
  MzhSearchPlan pl;  // the latency kernel's plan: its grid, the latents in LDS where they fit, or its capacity error
  const int st = make_plan(a->B, a->n_sims, MZH_FLAG_KERNEL_ONE, false, eng->support, true, &pl);
  if (st) return st;
  if (multi) {
    if (eng->set_m == 0) return fail(MZH_ERR_STATE, "no weight set loaded (mzh_load_weight_set)");
    if (m->n_networks > eng->set_m)
      return fail(MZH_ERR_ARG, "play_episodes_multi: n_networks=%d outside [1, %d], the loaded set", m->n_networks,
                  eng->set_m);
  } else if (!eng->loaded) {
    return fail(MZH_ERR_STATE, "weights not loaded");
  }
  DeviceGuard g(eng->device);
  if (g.err != hipSuccess) return hip_fail(g.err, "hipSetDevice");
  MzhSearchParams p{};
  p.B = a->B; p.S = a->n_sims; p.E = eng->E; p.in_dim = eng->in_dim; p.kin = eng->kin;
  p.deterministic = a->deterministic; p.np1 = (a->flags & MZH_FLAG_NP1_UCB) ? 1 : 0;
  p.discount = a->discount; p.eps = a->eps; p.temperature = a->temperature;
  p.noise = a->noise; p.tie_idx = a->tie_idx; p.action_u = a->action_u; p.minmax_in = a->minmax_in;
  p.htree = eng->htree; p.table = eng->table;
  p.visits = a->visits; p.root_q = a->root_q; p.action = a->action; p.pi = a->pi; p.pow_table = a->pow_table;
  MzhEpisodeParams ep{};
  ep.T = a->T; ep.n_disks = eng->n_disks; ep.goal_peg = a->goal_peg; ep.max_steps = a->max_steps;
  ep.start = a->state; ep.obs = a->obs; ep.reward = a->reward; ep.steps = a->steps; ep.illegal = a->illegal;
  ep.solved = a->solved; ep.final_state = a->final_state; ep.minmax_out = a->minmax_out; ep.err_count = a->err_count;
  if (!multi) {
    hipError_t e = mzh_launch_episodes(pl, eng->net, eng->onet, p, ep, (hipStream_t)stream);
    return e == hipSuccess ? MZH_OK : hip_fail(e, "play_episodes launch");
  }
  // the device check of net_index: the tile prologue of the other multi calls with the whole batch as the tile size
  // (one tile per network that has envs, at most min(M, B): inside the table), whose count the episode kernel reads
  const MzhMultiParams mp = multi_params(eng, m);
  // (the sweep form: of the budgets too, each in [0, n_sims], by the same workgroup)
  hipError_t e = mzh_launch_multi_tiles(mp, a->B, a->B, (hipStream_t)stream, sweep ? a->n_sims : 0,
                                        sweep ? w->n_sims : nullptr);
  if (e != hipSuccess) return hip_fail(e, "play_episodes_multi net_index check launch");
  const MzhEpisodeSet es{m->net_index, eng->mntiles, eng->set_stride};
  if (sweep) {
    const MzhEpisodeSweep sw{w->n_sims, w->discount};
    e = mzh_launch_episodes_sweep(pl, eng->setnet, eng->setonet, p, ep, es, sw, (hipStream_t)stream);
    return e == hipSuccess ? MZH_OK : hip_fail(e, "play_episodes_sweep launch");
  }
  e = mzh_launch_episodes_set(pl, eng->setnet, eng->setonet, p, ep, es, (hipStream_t)stream);
  return e == hipSuccess ? MZH_OK : hip_fail(e, "play_episodes_multi launch");
}

extern "C" int mzh_play_episodes(mzh_engine* eng, const mzh_episode_args* a, mzh_stream stream) {
  return play_episodes_common(eng, a, nullptr, false, stream);
}

extern "C" int mzh_play_episodes_multi(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m,
                                       mzh_stream stream) {
  return play_episodes_common(eng, a, m, true, stream);
}

extern "C" int mzh_play_episodes_sweep(mzh_engine* eng, const mzh_episode_args* a, const mzh_multi_args* m,
                                       const mzh_episode_sweep_args* w, mzh_stream stream) {
  return play_episodes_common(eng, a, m, true, stream, true, w);
}
