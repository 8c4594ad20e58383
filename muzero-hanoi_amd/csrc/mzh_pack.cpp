// mzh_pack.cpp -- canonical flat weights -> the packed blob of the three kernel layouts (mzh_pack.h).
// No floating-point arithmetic, only copies; tests/pack_check.cpp checks every element on the CPU.
#include "mzh_pack.h"

// [out][in] of the ten layers; -1: in_dim (representation layer 1 in), support (reward / value layer 2 out)
static constexpr int H = MZH_LATENT, F = MZH_HIDDEN, A = MZH_ACTIONS;
static constexpr int kOut[10] = {F, H, F, H, F, -1, F, A, F, -1};
static constexpr int kIn[10] = {-1, F, H + A, F, H, F, H, F, H, F};

MzhCanon mzh_canon_view(const float* flat, int in_dim, int support) {
  MzhCanon c{};
  c.in_dim = in_dim;
  c.support = support;
  for (int l = 0; l < 10; ++l) {
    c.out[l] = kOut[l] < 0 ? support : kOut[l];
    c.in[l] = kIn[l] < 0 ? in_dim : kIn[l];
    if (flat) c.w[l] = flat + c.total;
    c.total += (size_t)c.out[l] * c.in[l];
    if (flat) c.b[l] = flat + c.total;
    c.total += c.out[l];
  }
  return c;
}

// a new array of n zeros at the next float4 boundary (16-byte aligned on the device); returns its offset
static size_t append_zeros(std::vector<float>& buf, size_t n) {
  const size_t off = (buf.size() + 3) & ~(size_t)3;
  buf.resize(off + n, 0.0f);
  return off;
}

// ---- cooperative layout: torch [N][K] -> MFMA fragment tiles (see MzhLayer in mzh_device.h) ----
static void pack_weights(std::vector<float>& buf, PackedLayer& L, const float* W, int N, int K, int ldw) {
  L.nt = (N + 15) / 16;
  L.kb = (K + 15) / 16;
  L.woff = append_zeros(buf, (size_t)L.nt * L.kb * 64 * 4);
  float* dst = buf.data() + L.woff;
  for (int nt = 0; nt < L.nt; ++nt)
    for (int kb = 0; kb < L.kb; ++kb)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j) {
          const int n = 16 * nt + (lane & 15);
          const int k = 16 * kb + 4 * j + (lane >> 4);
          dst[(((size_t)nt * L.kb + kb) * 64 + lane) * 4 + j] = (n < N && k < K) ? W[(size_t)n * ldw + k] : 0.0f;
        }
}
static void pack_bias(std::vector<float>& buf, PackedLayer& L, const float* b, int N) {
  L.boff = append_zeros(buf, (size_t)L.nt * 16);
  for (int n = 0; n < N; ++n) buf[L.boff + n] = b[n];
}
// rows [0, N) and columns [0, K) of layer l
static PackedLayer pack_layer(std::vector<float>& buf, const MzhCanon& c, int l, int N, int K) {
  PackedLayer L;
  pack_weights(buf, L, c.w[l], N, K, c.in[l]);
  pack_bias(buf, L, c.b[l], N);
  return L;
}

// ---- wave layout (MzhWMlp, mzh_internal.h): weights as the MFMA A operand ----
static int wperm_u(int ht, int r) { return 16 * ht + 4 * (r & 3) + (r >> 2); }
enum WOut { WOUT_LATENT, WOUT_HEAD33, WOUT_NATURAL };
// output unit held by C row r (= 4g + i) of output tile ot, -1 for a padding row
static int wperm_out(WOut kind, int ot, int r, int n_out) {
  if (kind == WOUT_LATENT) return wperm_u(ot, r);
  if (kind == WOUT_HEAD33) {
    const int g = r >> 2, i = r & 3, sl = 4 * ot + i;
    const int k = 2 * g + (sl & 1) + 8 * (sl >> 1);  // partial q = 2g + (sl & 1), term sl >> 1
    return k < n_out ? k : -1;
  }
  const int k = 16 * ot + r;
  return k < n_out ? k : -1;
}

// bin 32 of a 33-bin head (MzhNet::rwd32 / MzhWMlp::w32): [16 blocks b][4 chains g] float4
// {W2[32][16b + g], W2[32][16b + 4 + g], W2[32][16b + 8 + g], W2[32][16b + 12 + g]}
static size_t pack_bin32(std::vector<float>& buf, const float* W2) {
  const size_t off = append_zeros(buf, 16 * 4 * 4);
  const float* row = W2 + (size_t)32 * MZH_HIDDEN;
  for (int b = 0; b < 16; ++b)
    for (int g = 0; g < 4; ++g)
      for (int t = 0; t < 4; ++t) buf[off + (size_t)(b * 4 + g) * 4 + t] = row[16 * b + 4 * t + g];
  return off;
}
// MLP i (layers 2i, 2i + 1); K1: the layer-1 columns taken (the dynamics one-hot columns go to MzhWNet::oh)
static PackedW pack_wmlp(std::vector<float>& buf, const MzhCanon& c, int i, int K1, WOut kind) {
  const float *W1 = c.w[2 * i], *b1 = c.b[2 * i], *W2 = c.w[2 * i + 1], *b2 = c.b[2 * i + 1];
  const int ldw1 = c.in[2 * i], n_out = c.out[2 * i + 1];
  PackedW P;
  P.kb1 = (K1 + 15) / 16;
  // a 33-bin head keeps bins 0..31 in two tiles; bin 32 goes to the vector chains (pack_bin32)
  P.no = kind == WOUT_HEAD33 ? 2 : (n_out + 15) / 16;
  const int FR = P.kb1 + P.no;
  P.soff = append_zeros(buf, (size_t)17 * FR * 64 * 4);  // ht block 16 = zero pad
  float* s = buf.data() + P.soff;
  for (int ht = 0; ht < 16; ++ht)
    for (int lane = 0; lane < 64; ++lane)
      for (int t = 0; t < 4; ++t) {
        const int r = lane & 15, gk = lane >> 4;
        for (int kb = 0; kb < P.kb1; ++kb) {
          const int k = 16 * kb + 4 * t + gk;
          s[(((size_t)ht * FR + kb) * 64 + lane) * 4 + t] = k < K1 ? W1[(size_t)wperm_u(ht, r) * ldw1 + k] : 0.0f;
        }
        for (int ot = 0; ot < P.no; ++ot) {
          const int row = wperm_out(kind, ot, r, n_out);
          const int k = 16 * ht + 4 * t + gk;
          s[(((size_t)ht * FR + P.kb1 + ot) * 64 + lane) * 4 + t] = row >= 0 ? W2[(size_t)row * MZH_HIDDEN + k] : 0.0f;
        }
      }
  P.b1off = append_zeros(buf, MZH_HIDDEN);
  for (int ht = 0; ht < 16; ++ht)
    for (int r = 0; r < 16; ++r) buf[P.b1off + 16 * ht + r] = b1[wperm_u(ht, r)];
  P.b2off = append_zeros(buf, (size_t)16 * P.no);
  for (int ot = 0; ot < P.no; ++ot)
    for (int r = 0; r < 16; ++r) {
      const int row = wperm_out(kind, ot, r, n_out);
      buf[P.b2off + 16 * ot + r] = row >= 0 ? b2[row] : 0.0f;
    }
  if (kind == WOUT_HEAD33) {
    P.w32off = pack_bin32(buf, W2);
    P.b32 = b2[32];
  }
  return P;
}

// ---- latency layout (MzhOneNet, mzh_internal.h) ----
static PackedOne pack_one(std::vector<float>& buf, const MzhCanon& c) {
  const int in = c.in_dim, sup = c.support;
  const float *rep0w = c.w[MZH_REP0], *rep0b = c.b[MZH_REP0], *rep2w = c.w[MZH_REP2], *rep2b = c.b[MZH_REP2];
  const float *dyn0w = c.w[MZH_DYN0], *dyn0b = c.b[MZH_DYN0], *dyn2w = c.w[MZH_DYN2], *dyn2b = c.b[MZH_DYN2];
  const float *rwd0w = c.w[MZH_RWD0], *rwd0b = c.b[MZH_RWD0], *rwd2w = c.w[MZH_RWD2], *rwd2b = c.b[MZH_RWD2];
  const float *pol0w = c.w[MZH_POL0], *pol0b = c.b[MZH_POL0], *pol2w = c.w[MZH_POL2], *pol2b = c.b[MZH_POL2];
  const float *val0w = c.w[MZH_VAL0], *val0b = c.b[MZH_VAL0], *val2w = c.w[MZH_VAL2], *val2b = c.b[MZH_VAL2];
  PackedOne o;
  // l1 [66 k4][256 units] float4
  o.l1 = append_zeros(buf, (size_t)66 * F * 4);
  for (int k4 = 0; k4 < 66; ++k4)
    for (int u = 0; u < F; ++u)
      for (int i = 0; i < 4; ++i) {
        float v = 0.0f;
        if (k4 < 16) v = dyn0w[(size_t)u * (H + A) + 4 * k4 + i];
        else if (k4 < 32) v = rwd0w[(size_t)u * H + 4 * (k4 - 16) + i];
        else if (k4 < 48) v = pol0w[(size_t)u * H + 4 * (k4 - 32) + i];
        else if (k4 < 64) v = val0w[(size_t)u * H + 4 * (k4 - 48) + i];
        else if (4 * (k4 - 64) + i < A) v = dyn0w[(size_t)u * (H + A) + H + 4 * (k4 - 64) + i];
        buf[o.l1 + ((size_t)k4 * F + u) * 4 + i] = v;
      }
  o.b1 = append_zeros(buf, (size_t)F * 4);
  for (int u = 0; u < F; ++u) {
    buf[o.b1 + 4 * u] = dyn0b[u];
    buf[o.b1 + 4 * u + 1] = rwd0b[u];
    buf[o.b1 + 4 * u + 2] = pol0b[u];
    buf[o.b1 + 4 * u + 3] = val0b[u];
  }
  // representation_net.0 k-major [in][256], its bias; representation_net.2 [64 k4][64] float4, its bias
  o.rep0 = append_zeros(buf, (size_t)in * F);
  for (int k = 0; k < in; ++k)
    for (int u = 0; u < F; ++u) buf[o.rep0 + (size_t)k * F + u] = rep0w[(size_t)u * in + k];
  o.rep0b = buf.size();
  buf.insert(buf.end(), rep0b, rep0b + F);
  o.rep2 = append_zeros(buf, (size_t)64 * 64 * 4);
  for (int k4 = 0; k4 < 64; ++k4)
    for (int j = 0; j < 64; ++j)
      for (int i = 0; i < 4; ++i) buf[o.rep2 + ((size_t)k4 * 64 + j) * 4 + i] = rep2w[(size_t)j * F + 4 * k4 + i];
  o.rep2b = buf.size();
  buf.insert(buf.end(), rep2b, rep2b + H);
  // the LDS image
  o.l2 = append_zeros(buf, (size_t)MZH_ONE_L2F4 * 4);
  float* L = buf.data() + o.l2;
  const int nb = sup < 32 ? sup : 32;  // bins of each head in the A2 rows
  for (int k4 = 0; k4 < 64; ++k4)
    for (int j = 0; j < 64; ++j)
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * k4 + i;
        L[((size_t)MZH_ONE_D2 + k4 * 64 + j) * 4 + i] = dyn2w[(size_t)j * F + k];
        const int row = j & 31;
        const float* W2 = j < 32 ? rwd2w : val2w;
        L[((size_t)MZH_ONE_A2 + k4 * 64 + j) * 4 + i] = row < nb ? W2[(size_t)row * F + k] : 0.0f;
        if (j < 8) L[((size_t)MZH_ONE_P2 + k4 * 8 + j) * 4 + i] = j < A ? pol2w[(size_t)j * F + k] : 0.0f;
      }
  if (sup == 33)
    for (int i = 0; i < 64; ++i)
      for (int ln = 0; ln < 8; ++ln) {
        const float* W2 = ln < 4 ? rwd2w : val2w;
        L[(size_t)MZH_ONE_C32 * 4 + ln * 64 + i] = W2[(size_t)32 * F + (ln & 3) + 4 * i];
      }
  float* B2 = L + (size_t)MZH_ONE_B2 * 4;
  for (int j = 0; j < 64; ++j) {
    B2[j] = dyn2b[j];
    B2[64 + j] = (j & 31) < nb ? (j < 32 ? rwd2b : val2b)[j & 31] : 0.0f;
  }
  for (int j = 0; j < A; ++j) B2[128 + j] = pol2b[j];
  if (sup == 33) {
    B2[136] = rwd2b[32];
    B2[137] = val2b[32];
  }
  return o;
}

MzhPacked mzh_pack_network(const MzhCanon& c) {
  const float* dyn0w = c.w[MZH_DYN0];
  MzhPacked P;
  std::vector<float>& buf = P.blob;
  // 33-bin heads: bins 0..31 as MFMA tiles, bin 32 by vector chains (MzhNet::rwd32 / val32)
  const int nhead = c.support == 33 ? 32 : c.support;
  for (int l = 0; l < 6; ++l)  // dynamic_net.0: the h part only (k < 64)
    P.L[l] = pack_layer(buf, c, l, l == MZH_RWD2 ? nhead : c.out[l], l == MZH_DYN0 ? H : c.in[l]);
  // pol0 and val0 weights back to back: the search kernel's prediction chunks take consecutive
  // tiles of this 32-tile strip and load them as one contiguous run (mzh_mma_store ring refill)
  pack_weights(buf, P.L[MZH_POL0], c.w[MZH_POL0], F, H, H);
  pack_weights(buf, P.L[MZH_VAL0], c.w[MZH_VAL0], F, H, H);
  pack_bias(buf, P.L[MZH_POL0], c.b[MZH_POL0], F);
  pack_bias(buf, P.L[MZH_VAL0], c.b[MZH_VAL0], F);
  P.L[MZH_POL2] = pack_layer(buf, c, MZH_POL2, A, F);
  P.L[MZH_VAL2] = pack_layer(buf, c, MZH_VAL2, nhead, F);
  P.onehot = append_zeros(buf, (size_t)A * F);
  for (int a = 0; a < A; ++a)
    for (int n = 0; n < F; ++n) buf[P.onehot + (size_t)a * F + n] = dyn0w[(size_t)n * (H + A) + H + a];
  // wave layout
  const WOut vkind = c.support == 33 ? WOUT_HEAD33 : WOUT_NATURAL;
  const WOut kinds[5] = {WOUT_LATENT, WOUT_LATENT, vkind, WOUT_NATURAL, vkind};
  for (int i = 0; i < 5; ++i) P.W[i] = pack_wmlp(buf, c, i, i == 0 ? c.in_dim : H, kinds[i]);
  P.wonehot = append_zeros(buf, (size_t)A * F);
  for (int a = 0; a < A; ++a)
    for (int j = 0; j < F; ++j) buf[P.wonehot + (size_t)a * F + j] = dyn0w[(size_t)wperm_u(j >> 4, j & 15) * (H + A) + H + a];
  P.one = pack_one(buf, c);
  return P;
}

// ---- transposed layout (MzhPackedT, mzh_pack.h): the saliency backward's B operands ----
MzhPackedT mzh_pack_transposed(const MzhCanon& c) {
  static constexpr int kLayers[MZH_T_LAYERS] = {MZH_REP0, MZH_REP2, MZH_POL0, MZH_POL2, MZH_VAL0, MZH_VAL2};
  MzhPackedT T;
  for (int t = 0; t < MZH_T_LAYERS; ++t) {
    const int l = kLayers[t], O = c.out[l], I = c.in[l];
    const float* W = c.w[l];
    T.layer[t] = l;
    T.nt[t] = (I + 15) / 16;
    T.kb[t] = (O + 15) / 16;
    T.off[t] = append_zeros(T.blob, (size_t)T.nt[t] * T.kb[t] * 64 * 4);
    float* dst = T.blob.data() + T.off[t];
    for (int nt = 0; nt < T.nt[t]; ++nt)
      for (int kb = 0; kb < T.kb[t]; ++kb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int i = 16 * nt + (lane & 15);
            const int o = 16 * kb + 4 * j + (lane >> 4);
            dst[(((size_t)nt * T.kb[t] + kb) * 64 + lane) * 4 + j] = (o < O && i < I) ? W[(size_t)o * I + i] : 0.0f;
          }
  }
  return T;
}

MzhPackedTSet mzh_pack_transposed_set(const float* flat, int M, int in_dim, int support) {
  MzhPackedTSet S;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  for (int m = 0; m < M; ++m) {
    MzhPackedT T = mzh_pack_transposed(mzh_canon_view(flat + (size_t)m * n, in_dim, support));
    if (m == 0) {
      S.stride = (T.blob.size() + 63) & ~(size_t)63;
      S.blob.assign((size_t)M * S.stride, 0.0f);
    }
    for (size_t i = 0; i < T.blob.size(); ++i) S.blob[(size_t)m * S.stride + i] = T.blob[i];
    if (m == 0) {
      T.blob.clear();
      S.layout = T;
    }
  }
  return S;
}

MzhPackedSet mzh_pack_network_set(const float* flat, int M, int in_dim, int support) {
  MzhPackedSet S;
  S.M = M;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  for (int m = 0; m < M; ++m) {
    MzhPacked P = mzh_pack_network(mzh_canon_view(flat + (size_t)m * n, in_dim, support));
    if (m == 0) {
      S.stride = (P.blob.size() + 63) & ~(size_t)63;
      S.scal = (size_t)M * S.stride;
      S.blob.assign(S.scal + 2 * (size_t)M, 0.0f);
    }
    for (size_t i = 0; i < P.blob.size(); ++i) S.blob[(size_t)m * S.stride + i] = P.blob[i];
    S.blob[S.scal + 2 * m] = P.W[2].b32;
    S.blob[S.scal + 2 * m + 1] = P.W[4].b32;
    if (m == 0) {
      P.blob.clear();
      S.layout = P;
    }
  }
  return S;
}

// ---- the packers as index maps (MzhPackMaps, mzh_pack.h) ----
// blob float of the pack of i -> (float)(i + 1): i + 1 where it holds element i, +0.0f where it is padding
static int32_t map_entry(float v) { return (int32_t)v - 1; }

bool mzh_pack_maps(int in_dim, int support, MzhPackMaps* out) {
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  if (n >= ((size_t)1 << 24)) return false;
  std::vector<float> id(n);
  for (size_t i = 0; i < n; ++i) id[i] = (float)(i + 1);
  const MzhCanon c = mzh_canon_view(id.data(), in_dim, support);
  MzhPacked P = mzh_pack_network(c);
  MzhPackedT T = mzh_pack_transposed(c);
  out->main.resize(P.blob.size());
  for (size_t j = 0; j < P.blob.size(); ++j) out->main[j] = map_entry(P.blob[j]);
  out->trans.resize(T.blob.size());
  for (size_t j = 0; j < T.blob.size(); ++j) out->trans[j] = map_entry(T.blob[j]);
  out->scalar_src[0] = map_entry(P.W[2].b32);
  out->scalar_src[1] = map_entry(P.W[4].b32);
  for (int i = 0; i < 5; ++i) P.W[i].b32 = 0.0f;  // an index, not a weight: the caller fills the value in
  P.blob.clear();
  T.blob.clear();
  out->layout = P;
  out->tlayout = T;
  return true;
}

// ---- the parameter-gradient kernel's two further transposed layers (MzhPackedG, mzh_pack.h) ----
MzhPackedG mzh_pack_pgrad(const MzhCanon& c) {
  static constexpr int kLayers[MZH_G_LAYERS] = {MZH_DYN2, MZH_RWD2};
  MzhPackedG T;
  for (int t = 0; t < MZH_G_LAYERS; ++t) {
    const int l = kLayers[t], O = c.out[l], I = c.in[l];
    const float* W = c.w[l];
    T.nt[t] = (I + 15) / 16;
    T.kb[t] = (O + 15) / 16;
    T.off[t] = append_zeros(T.blob, (size_t)T.nt[t] * T.kb[t] * 64 * 4);
    float* dst = T.blob.data() + T.off[t];
    for (int nt = 0; nt < T.nt[t]; ++nt)
      for (int kb = 0; kb < T.kb[t]; ++kb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int i = 16 * nt + (lane & 15);
            const int o = 16 * kb + 4 * j + (lane >> 4);
            dst[(((size_t)nt * T.kb[t] + kb) * 64 + lane) * 4 + j] = (o < O && i < I) ? W[(size_t)o * I + i] : 0.0f;
          }
  }
  return T;
}

bool mzh_pgrad_map(int in_dim, int support, MzhPgradMap* out) {
  MzhPackMaps mp;
  if (!mzh_pack_maps(in_dim, support, &mp)) return false;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  std::vector<int32_t> where(n, -1);  // canonical index -> the first main-blob float holding it
  for (size_t j = 0; j < mp.main.size(); ++j)
    if (mp.main[j] >= 0 && where[mp.main[j]] < 0) where[mp.main[j]] = (int32_t)j;
  std::vector<float> id(n);
  for (size_t i = 0; i < n; ++i) id[i] = (float)(i + 1);
  MzhPackedG G = mzh_pack_pgrad(mzh_canon_view(id.data(), in_dim, support));
  out->src.assign(G.blob.size(), -1);
  for (size_t j = 0; j < G.blob.size(); ++j) {
    const int32_t ci = map_entry(G.blob[j]);
    if (ci < 0) continue;
    if (where[ci] < 0) return false;
    out->src[j] = where[ci];
  }
  G.blob.clear();
  out->layout = G;
  return true;
}

int32_t mzh_pack_map_encode(const MzhCanon& sizes, int64_t canon_index) {
  if (canon_index < 0) return -1;
  size_t first = 0;
  for (int l = 0; l < 10; ++l) {
    const size_t nw = (size_t)sizes.out[l] * sizes.in[l], nb = (size_t)sizes.out[l];
    if ((size_t)canon_index < first + nw) return (int32_t)((2 * l) << 24 | (int32_t)(canon_index - first));
    first += nw;
    if ((size_t)canon_index < first + nb) return (int32_t)((2 * l + 1) << 24 | (int32_t)(canon_index - first));
    first += nb;
  }
  return -1;
}
