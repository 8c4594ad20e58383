// mzh_host.h -- what the host units of the C ABI (mzh_api*.hip) share: the error state, the device guard, the
// owning buffer type, the engine, and the few helpers that cross a unit.  Host only: no kernel unit includes it.
// Ownership rule: an engine allocation is a DevBuf member and is freed by its destructor; a drop function resets.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/mzh.h"
#include "mzh_internal.h"

#pragma GCC visibility push(hidden)  // nothing below is part of the library's interface

// record the calling thread's message (mzh_last_error) and return `code`; defined in mzh_api.hip
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define HIP_OK(expr)                                   \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);  \
  } while (0)

// the status of an entry point whose last act was a launch (or any HIP call) named `what`
static inline int hip_status(hipError_t e, const char* what) { return e == hipSuccess ? MZH_OK : hip_fail(e, what); }

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
// run the rest of the scope on device `dev`, or return the error
#define MZH_ON_DEVICE(dev)    \
  DeviceGuard device_guard_(dev); \
  if (device_guard_.err != hipSuccess) return hip_fail(device_guard_.err, "hipSetDevice")

// A device allocation (pinned host memory with Pinned) of `count` elements, freed by its destructor.  Move-only.
// It neither waits for the device nor counts: a caller that must do either does so around reset() / alloc().
template <class T, bool Pinned = false>
class DevBuf {
  T* p_ = nullptr;
  size_t n_ = 0;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }
  T* get() const { return p_; }
  size_t count() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  hipError_t reset() {
    T* p = p_;
    p_ = nullptr, n_ = 0;
    return !p ? hipSuccess : Pinned ? hipHostFree((void*)p) : hipFree((void*)p);
  }
  hipError_t alloc(size_t count) {  // drops what it held
    (void)reset();
    void* p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, count * sizeof(T)) : hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) p_ = static_cast<T*>(p), n_ = count;
    return e;
  }
};

// A loaded network (mzh_load_weights*: eng->single) or network set (mzh_load_weight_set*: eng->set): the blobs and
// the kernels' views of them.  A call that serves both picks the record once.
struct MzhWeights {
  DevBuf<float> main;   // MzhPacked blob; a set: [m] blobs at `stride` bytes, then [m][2] floats (MzhPackedSet)
  DevBuf<float> trans;  // MzhPackedT blob(s) of mzh_saliency: uploaded with the weights they are a function of
  // dynamic_net.2 and rwd_net.2 transposed (MzhPackedG) for mzh_param_grads: gathered from `main` by the first such
  // call after a load (every load clears the valid flag); workspace, not a weight buffer of the load calls (their
  // debug counters do not count it)
  DevBuf<float> grad;   // [m] at the engine's pgrad.stride
  bool grad_valid = false;
  int m = 0;            // members: 0 nothing loaded, 1 for the single network
  size_t stride = 0;    // bytes between the members' blobs in `main` (0 for the single network)
  MzhNet net{};         // a set: network 0's, the template the multi kernels offset
  MzhOneNet onet{};     // the latency kernel's views, likewise
  MzhSalNetT tnet{};
  // a set's [m][2] tail: the two by-value scalars of each member
  const float* scal() const { return main.get() + (size_t)m * (stride / sizeof(float)); }
};

struct mzh_engine {
  int device = 0;
  int n_disks = 0, max_sims = 0, max_roots = 0, support = 33;
  int in_dim = 0, kin = 0, E = 0;
  struct {                      // the search workspace, made by mzh_create
    DevBuf<unsigned char> tree;  // [max_roots][E] 128-B blocks (MzhBlock / MzwBlock)
    DevBuf<float> htree;         // [max_roots][E][64]
    DevBuf<uint16_t> pathx;      // [max_roots][E]
    DevBuf<double> table;        // [max_sims + 2] the UCB table
  } ws;
  MzhWeights single, set;       // the single-network calls never read `set`
  MzhWNet wnet{};               // the wave kernel's view of the single network, which alone has one
  struct {                      // tile table workspace of the multi-network kernels, allocated with the first set
    DevBuf<MzhTile> tiles;
    DevBuf<int32_t> ntiles;
  } multi;
  // the wave kernel's expansion memo (mzh.h): built by the first wave search after a weight load
  struct {
    int want = -1;              // mzh_set_memo_depth: -1 automatic, 0 off, d > 0 forced
    int auto_cap = MZH_MEMO_MAX_DEPTH;  // the automatic depth's ceiling: lowered when a build ran out of memory
    int D = 0;                  // depth of the built table (0: none)
    DevBuf<float> h;            // [rows][64]
    DevBuf<float> rec;          // [rows][8]
    DevBuf<unsigned long long> cnt;  // [3] device counters, zeroed by mzh_create
    double build_ms = 0.0;
    // its grown extension (mzh_set_memo_grow): rows after the dense ones in h / rec, made and dropped with them;
    // the per-root miss log is workspace (made by the first search that logs, kept across loads)
    long long grow_want = -1;   // byte budget of the extension's rows: -1 the default, 0 off
    int log_cap = MZH_MEMO_LOG_CAP;
    long long base = 0;         // dense rows of the built table
    long long cap = 0;          // extension rows of the built table (0: none)
    DevBuf<int32_t> link;       // [base + cap][6]
    DevBuf<int32_t> ctr;        // [2] rows in use, in use before the last harvest
    DevBuf<uint4> log;          // [max_roots][the log_cap it was made for]
    DevBuf<int32_t> logn;       // [max_roots]
  } memo;
  struct {                      // mzh_param_grads' gather: the map once per engine
    std::unique_ptr<MzhPgradMap> maps;  // host: the layout and the gather's source map
    DevBuf<int32_t> map;        // device: the source map
    size_t stride = 0;          // floats of one network's MzhWeights::grad (rounded up to 256 bytes)
  } pgrad;
  // the device repack (mzh_load_weights_device / mzh_load_weight_set_device): made by the first such call, kept
  struct {
    std::unique_ptr<MzhPackMaps> maps;  // host: layouts and scalar sources of this engine's shape
    DevBuf<int32_t> map;        // device: encoded main map [stride], then the transposed one [tstride]
    size_t stride = 0, tstride = 0;  // a blob rounded up to 256 bytes (the set strides), floats; -1 beyond the blob
    int32_t scal_src[2] = {-1, -1};  // encoded sources of the two by-value scalars
    DevBuf<const float*> ptab;  // [20]: the single network's parameter pointers
    DevBuf<const float*> set_ptab;  // [M][20]
    std::vector<const float*> ptab_host, set_ptab_host;  // what they hold (uploaded again only when it differs)
    DevBuf<float> scal2;        // [2]: the single network's by-value scalars as the gather wrote them
    DevBuf<float, true> scal2_host;  // pinned [2]: their read-back
  } repack;
  // weight buffer allocations, frees and device-wide waits of every load call (mzh_weights_debug_counters)
  uint64_t n_alloc = 0, n_free = 0, n_wait = 0;
};

// ---- the helpers that cross a unit ----
// mzh_api.hip: rows (roots) per workgroup of the standalone inference kernels
int pick_rows(int B);
// What a call refuses of its rows: n rows of B envs, env_index or the first n.  `pre` opens the text ("call: ").
int rows_range_check(const char* pre, int n, int B, const int32_t* env_index);
// What a call refuses of its mzh_multi_args, in the two phases every caller uses: what the block alone decides
// (before the engine is looked at), then what the engine decides -- with m == NULL that its own network is loaded.
int multi_args_check(const char* pre, const mzh_multi_args* m);
int multi_engine_check(const char* pre, const mzh_multi_args* m, const mzh_engine* eng);
// mzh_api_search.hip
int pick_tile(int B, uint32_t flags);
int make_plan(int B, int S, uint32_t flags, bool replay, int support, bool has_minmax, MzhSearchPlan* pl);
MzhMultiParams multi_params(const mzh_engine* eng, const mzh_multi_args* m);
// mzh_api_memo.hip
int memo_depth_for(int n_disks, int want, int* D);  // the expansion memo's depth of a request
hipError_t memo_drop(mzh_engine* eng);
int memo_ensure(mzh_engine* eng, hipStream_t stream);
int memo_log_ensure(mzh_engine* eng);

#pragma GCC visibility pop
