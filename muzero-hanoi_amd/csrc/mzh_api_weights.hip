// mzh_api_weights.hip -- the weights of an engine: mzh_load_weights / mzh_load_weight_set (packed on the host by
// mzh_pack.cpp, uploaded, offsets turned into pointers), their device forms (the same blobs gathered on the device
// from the live parameter tensors), the debug blob and counters, mzh_pack_map.
#include "mzh_host.h"

extern "C" int mzh_weights_size(int n_disks, int support, size_t* n_floats) {
  if (n_disks < 1 || n_disks > 16 || (support != 33 && support != 1) || !n_floats)
    return fail(MZH_ERR_ARG, "bad n_disks=%d / support=%d", n_disks, support);
  *n_floats = mzh_canon_view(nullptr, 3 * n_disks, support).total;
  return MZH_OK;
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

// the wave kernel's view of the single network's blob at `base`
static MzhWNet make_wnet(const MzhPacked& pk, const float* base, int sup, int in) {
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
  MzhWNet w;
  w.wbase = base;
  w.rep = mkw(pk.W[0]); w.dyn = mkw(pk.W[1]); w.rwd = mkw(pk.W[2]); w.pol = mkw(pk.W[3]); w.val = mkw(pk.W[4]);
  w.oh = base + pk.wonehot;
  w.support = sup;
  w.in_dim = in;
  return w;
}

// The kernels' views of the M networks whose blobs lie in w.main / w.trans with the offsets of pk / pt, `stride` /
// `tstride` floats apart (a set: network 0's views, the template the multi kernels offset).  Marks the record loaded.
static int bind(mzh_engine* eng, MzhWeights& w, const MzhPacked& pk, const MzhPackedT& pt, size_t stride, size_t tstride,
                int M) {
  const float* base = w.main.get();
  w.tnet = make_tnet(pt, w.trans.get(), tstride * sizeof(float));
  const int nst = make_net(pk, base, eng->support, eng->in_dim, &w.net);
  if (nst) return nst;
  w.onet = make_onet(pk, base);
  w.stride = stride * sizeof(float);
  w.m = M;
  return MZH_OK;
}

// the single network has the wave kernel's view as well
static int bind_single(mzh_engine* eng, const MzhPacked& pk, const MzhPackedT& pt) {
  const int st = bind(eng, eng->single, pk, pt, 0, 0, 1);
  if (st == MZH_OK) eng->wnet = make_wnet(pk, eng->single.main.get(), eng->support, eng->in_dim);
  return st;
}

// free a record's blobs once the device has finished with them
static hipError_t weights_release(mzh_engine* eng, MzhWeights& w) {
  if (!w.main.get()) return hipSuccess;
  ++eng->n_wait;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = w.main.reset();
  if (e != hipSuccess) return e;
  ++eng->n_free;
  w.m = 0;
  if (w.trans.get()) {
    e = w.trans.reset();
    if (e != hipSuccess) return e;
    ++eng->n_free;
  }
  return hipSuccess;
}

// a record's two blobs from the host (the load calls released the old ones: the sizes may differ)
static hipError_t weights_upload(mzh_engine* eng, MzhWeights& w, const std::vector<float>& blob, const std::vector<float>& tblob) {
  hipError_t e = w.main.alloc(blob.size());
  if (e == hipSuccess) e = hipMemcpy(w.main.get(), blob.data(), w.main.bytes(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = w.trans.alloc(tblob.size());
  if (e == hipSuccess) e = hipMemcpy(w.trans.get(), tblob.data(), w.trans.bytes(), hipMemcpyHostToDevice);
  if (e == hipSuccess) eng->n_alloc += 2;
  return e;
}

// a record's two blobs for the device repack to fill: kept from one load to the next
static hipError_t weights_reserve(mzh_engine* eng, MzhWeights& w, size_t n, size_t tn) {
  if (!w.main.get()) {
    hipError_t e = w.main.alloc(n);
    if (e != hipSuccess) return e;
    ++eng->n_alloc;
  }
  if (!w.trans.get()) {
    hipError_t e = w.trans.alloc(tn);
    if (e != hipSuccess) return e;
    ++eng->n_alloc;
  }
  return hipSuccess;
}

// the tile table workspace of the multi-network kernels, allocated with the first set
static hipError_t set_workspace(mzh_engine* eng) {
  hipError_t e = hipSuccess;
  if (!eng->multi.tiles.get()) e = eng->multi.tiles.alloc((size_t)mzh_multi_max_tiles(eng->max_roots, 16, MZH_MULTI_MAX_NETS));
  if (e == hipSuccess && !eng->multi.ntiles.get()) e = eng->multi.ntiles.alloc(1);
  return e;
}

extern "C" int mzh_load_weights(mzh_engine* eng, const float* flat, size_t n_floats) {
  if (!eng || !flat) return fail(MZH_ERR_ARG, "engine or weights NULL");
  const int in = eng->in_dim, sup = eng->support;
  const size_t want = mzh_canon_view(nullptr, in, sup).total;
  if (n_floats != want) return fail(MZH_ERR_ARG, "weights: expected %zu floats, got %zu", want, n_floats);
  const MzhPacked pk = mzh_pack_network(mzh_canon_view(flat, in, sup));
  const MzhPackedT pt = mzh_pack_transposed(mzh_canon_view(flat, in, sup));

  MZH_ON_DEVICE(eng->device);
  eng->single.grad_valid = false;
  HIP_OK(weights_release(eng, eng->single));
  HIP_OK(memo_drop(eng));  // the table is a function of the weights
  HIP_OK(weights_upload(eng, eng->single, pk.blob, pt.blob));
  return bind_single(eng, pk, pt);
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

  MZH_ON_DEVICE(eng->device);
  eng->set.grad_valid = false;
  HIP_OK(weights_release(eng, eng->set));
  HIP_OK(set_workspace(eng));
  HIP_OK(weights_upload(eng, eng->set, ps.blob, pts.blob));
  return bind(eng, eng->set, ps.layout, pts.layout, ps.stride, pts.stride, M);
}

// ---- device repack: the same blobs gathered on the device from the live parameter tensors ----
// the pack maps of the engine's shape, on the host and (encoded, padded with -1 to the set strides) on the
// device, and the small buffers of the single-network call: made once per engine
static int repack_ensure(mzh_engine* eng) {
  auto& r = eng->repack;
  if (r.map.get()) return MZH_OK;
  const int in = eng->in_dim, sup = eng->support;
  if (!r.maps) {
    std::unique_ptr<MzhPackMaps> m(new MzhPackMaps());
    if (!mzh_pack_maps(in, sup, m.get())) return fail(MZH_ERR_ARG, "pack maps: the shape has 2^24 or more weights");
    r.maps = std::move(m);
  }
  const MzhPackMaps& mp = *r.maps;
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
  for (int i = 0; i < 2; ++i) r.scal_src[i] = mzh_pack_map_encode(sizes, mp.scalar_src[i]);
  if (!r.ptab.get()) HIP_OK(r.ptab.alloc(20));
  if (!r.scal2.get()) HIP_OK(r.scal2.alloc(2));
  if (!r.scal2_host.get()) HIP_OK(r.scal2_host.alloc(2));
  DevBuf<int32_t> d;
  HIP_OK(d.alloc(enc.size()));
  hipError_t e = hipMemcpy(d.get(), enc.data(), d.bytes(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy (pack maps)");
  r.map = std::move(d);
  r.stride = rs;
  r.tstride = rts;
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

// the gather of M networks' parameters (ptab) into w's blobs, with the two by-value scalars of each to `scal`
static hipError_t repack_launch(const mzh_engine* eng, MzhWeights& w, const float** ptab, float* scal, int M, bool set,
                                hipStream_t stream) {
  const auto& r = eng->repack;
  MzhRepackParams p{};
  p.map_m = reinterpret_cast<const int4*>(r.map.get());
  p.map_t = reinterpret_cast<const int4*>(r.map.get() + r.stride);
  // a set member is written up to its stride (zeros between the blobs), the single network up to its blob's end
  p.n4m = (int)((set ? r.stride : r.maps->main.size()) / 4);
  p.n4t = (int)((set ? r.tstride : r.maps->trans.size()) / 4);
  p.stride_m = r.stride;
  p.stride_t = r.tstride;
  p.scal_src[0] = r.scal_src[0];
  p.scal_src[1] = r.scal_src[1];
  p.ptab = ptab;
  p.dst_m = w.main.get();
  p.dst_t = w.trans.get();
  p.scal = scal;
  return mzh_launch_repack(p, M, stream);
}

extern "C" int mzh_load_weights_device(mzh_engine* eng, const float* const* param, mzh_stream stream) {
  if (!eng || !param) return fail(MZH_ERR_ARG, "load_weights_device: engine or param NULL");
  for (int i = 0; i < 20; ++i)
    if (!param[i]) return fail(MZH_ERR_ARG, "load_weights_device: param[%d] is NULL", i);
  MZH_ON_DEVICE(eng->device);
  const int st = repack_ensure(eng);
  if (st) return st;
  auto& r = eng->repack;
  const MzhPackMaps& mp = *r.maps;
  MzhWeights& w = eng->single;
  w.grad_valid = false;
  HIP_OK(weights_reserve(eng, w, mp.main.size(), mp.trans.size()));
  HIP_OK(memo_drop(eng));  // the table is a function of the weights
  const hipStream_t s = (hipStream_t)stream;
  const int ps = ptab_sync(param, 20, r.ptab.get(), &r.ptab_host, s);
  if (ps) return ps;
  hipError_t e = repack_launch(eng, w, r.ptab.get(), r.scal2.get(), 1, false, s);
  if (e != hipSuccess) return hip_fail(e, "repack launch");
  MzhPacked pk = mp.layout;
  if (eng->support == 33) {  // the kernels take bin 32's two biases by value: one 8-byte copy, one wait
    HIP_OK(hipMemcpyAsync(r.scal2_host.get(), r.scal2.get(), 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    pk.W[2].b32 = r.scal2_host.get()[0];
    pk.W[4].b32 = r.scal2_host.get()[1];
  }
  return bind_single(eng, pk, mp.tlayout);
}

extern "C" int mzh_load_weight_set_device(mzh_engine* eng, const float* const* param, int M, mzh_stream stream) {
  if (!eng || !param) return fail(MZH_ERR_ARG, "load_weight_set_device: engine or param NULL");
  if (M < 1 || M > MZH_MULTI_MAX_NETS)
    return fail(MZH_ERR_ARG, "weight set: M must be in [1,%d], got %d", MZH_MULTI_MAX_NETS, M);
  for (int i = 0; i < 20 * M; ++i)
    if (!param[i]) return fail(MZH_ERR_ARG, "load_weight_set_device: param[%d][%d] is NULL", i / 20, i % 20);
  MZH_ON_DEVICE(eng->device);
  const int st = repack_ensure(eng);
  if (st) return st;
  auto& r = eng->repack;
  MzhWeights& w = eng->set;
  w.grad_valid = false;
  if (w.main.get() && w.m != M) HIP_OK(weights_release(eng, w));
  HIP_OK(set_workspace(eng));
  HIP_OK(weights_reserve(eng, w, (size_t)M * r.stride + 2 * (size_t)M, (size_t)M * r.tstride));
  if (r.set_ptab.count() != (size_t)M * 20) {
    r.set_ptab_host.clear();
    HIP_OK(r.set_ptab.alloc((size_t)M * 20));
  }
  const hipStream_t s = (hipStream_t)stream;
  const int ps = ptab_sync(param, (size_t)M * 20, r.set_ptab.get(), &r.set_ptab_host, s);
  if (ps) return ps;
  // the scalars go to the main blob's tail (MzhPackedSet::scal)
  hipError_t e = repack_launch(eng, w, r.set_ptab.get(), w.main.get() + (size_t)M * r.stride, M, true, s);
  if (e != hipSuccess) return hip_fail(e, "repack launch");
  return bind(eng, w, r.maps->layout, r.maps->tlayout, r.stride, r.tstride, M);
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
  const MzhWeights& w = which < 2 ? eng->single : eng->set;
  if (w.m == 0) return fail(MZH_ERR_STATE, which < 2 ? "weights not loaded" : "no weight set loaded");
  const DevBuf<float>& src = which % 2 ? w.trans : w.main;
  *n_floats = src.count();
  if (!dst) return MZH_OK;
  MZH_ON_DEVICE(eng->device);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(dst, src.get(), src.bytes(), hipMemcpyDeviceToDevice));
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
