// pack_check.cpp -- CPU check of the weight packers (csrc/mzh_pack.cpp), built with the host sanitizers
// and run as a child process by tests/test_pack_cpu.py:   pack_check <n_disks> <support> <fnv1a64 hex>
//
// Canonical weight i is (float)(i + 1) (exact: fewer than 2^24 weights), so every blob float names its
// source.  The packers loop blob position -> source element; this program goes the other way: for every
// source element it computes, from the layout comments (MzhLayer / MzhNet in mzh_device.h, MzhWMlp /
// MzhWNet / MzhOneNet in mzh_internal.h, MZH_ONE_* in mzh_pack.h, the 33-bin slot order in mzh_wave.hip),
// every blob position that must hold it.  Then: each position is claimed once, every unclaimed float is
// +0.0f, each element occurs in the blob exactly as often as the layouts say, float4 arrays are 16-byte
// aligned, the pol0 / val0 strips are adjacent, and the blob's bytes hash to the recorded constant.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../muzero-hanoi_amd/csrc/mzh_pack.h"

static int g_errors = 0;
#define EXPECT(cond, ...)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_errors++ < 20) {                               \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

static const int H = 64, F = 256, A = 6;

struct Blob {
  const std::vector<float>& v;
  std::vector<unsigned char> claimed;
  std::vector<int> copies;  // per source element: positions claimed for it
  Blob(const std::vector<float>& b, size_t n_src) : v(b), claimed(b.size(), 0), copies(n_src, 0) {}
  // blob position `pos` must hold source element `src`
  void at(size_t pos, size_t src, const char* what) {
    if (pos >= v.size()) {
      EXPECT(false, "%s: position %zu outside the blob (%zu floats)", what, pos, v.size());
      return;
    }
    EXPECT(v[pos] == (float)(src + 1), "%s: blob[%zu] = %.1f, want source element %zu", what, pos, v[pos], src);
    EXPECT(!claimed[pos], "%s: blob[%zu] claimed twice", what, pos);
    claimed[pos] = 1;
    ++copies[src];
  }
};

// cooperative layout: W4[(nt*KB + kb)*64 + lane][j] = W[16nt + (lane&15)][16kb + 4j + (lane>>4)]
static size_t coop_pos(const PackedLayer& L, int n, int k) {
  const int nt = n / 16, kb = k / 16, j = (k % 16) / 4, g = k % 4, lane = n % 16 + 16 * g;
  return L.woff + (((size_t)nt * L.kb + kb) * 64 + lane) * 4 + j;
}
// wave layout: the C row r of hidden tile ht that holds unit n, u(ht, r) = 16ht + 4(r&3) + (r>>2)
static int wave_row(int n) { return (n % 16) / 4 + 4 * (n % 4); }
// frag (ht, f)[lane][t] of the stream [17][KB1 + NO][64] float4, lane = r + 16g
static size_t wave_pos(const PackedW& P, int ht, int f, int r, int g, int t) {
  return P.soff + (((size_t)ht * (P.kb1 + P.no) + f) * 64 + r + 16 * g) * 4 + t;
}

int main(int argc, char** argv) {
  if (argc != 4) return fprintf(stderr, "usage: pack_check n_disks support fnv1a64-hex\n"), 2;
  const int n_disks = atoi(argv[1]), sup = atoi(argv[2]), in = 3 * n_disks;
  const unsigned long long want_hash = strtoull(argv[3], nullptr, 16);

  // ---- the layer table ----
  const int out_[10] = {F, H, F, H, F, sup, F, A, F, sup}, in_[10] = {in, F, H + A, F, H, F, H, F, H, F};
  const MzhCanon sizes = mzh_canon_view(nullptr, in, sup);
  size_t sum = 0;
  for (int l = 0; l < 10; ++l) sum += (size_t)out_[l] * in_[l] + out_[l];
  EXPECT(sizes.total == sum, "table total %zu, per-layer sum %zu", sizes.total, sum);
  if (n_disks == 4 && sup == 33) EXPECT(sizes.total == 122824, "total %zu at (4, 33)", sizes.total);
  std::vector<float> flat(sum);
  for (size_t i = 0; i < sum; ++i) flat[i] = (float)(i + 1);
  const MzhCanon c = mzh_canon_view(flat.data(), in, sup);
  EXPECT(c.total == sum && c.in_dim == in && c.support == sup, "view header");
  size_t off = 0;
  for (int l = 0; l < 10; ++l) {
    EXPECT(sizes.w[l] == nullptr && sizes.b[l] == nullptr, "sizes-only view has pointers");
    EXPECT(c.out[l] == out_[l] && c.in[l] == in_[l], "layer %d is [%d][%d]", l, c.out[l], c.in[l]);
    EXPECT(c.w[l] == flat.data() + off, "w[%d] offset", l);
    off += (size_t)out_[l] * in_[l];
    EXPECT(c.b[l] == flat.data() + off, "b[%d] offset", l);
    off += out_[l];
  }
  if (g_errors) return 1;  // the source indices below rely on the table

  const MzhPacked P = mzh_pack_network(c);
  Blob blob(P.blob, sum);
  auto W = [&](int l, int n, int k) { return (size_t)(c.w[l] - flat.data()) + (size_t)n * in_[l] + k; };
  auto Bs = [&](int l, int n) { return (size_t)(c.b[l] - flat.data()) + n; };
  const int nhead = sup == 33 ? 32 : sup;  // rows of a value / reward head held as tiles

  // ---- cooperative layout (MzhLayer, MzhNet) ----
  for (int l = 0; l < 10; ++l) {
    const bool head = l == MZH_RWD2 || l == MZH_VAL2;
    const int N = head ? nhead : out_[l], K = l == MZH_DYN0 ? H : in_[l];
    EXPECT(P.L[l].nt == (N + 15) / 16 && P.L[l].kb == (K + 15) / 16, "coop layer %d: nt %d kb %d", l, P.L[l].nt, P.L[l].kb);
    EXPECT(P.L[l].woff % 4 == 0, "coop layer %d: w not float4-aligned", l);
    for (int n = 0; n < N; ++n) {
      for (int k = 0; k < K; ++k) blob.at(coop_pos(P.L[l], n, k), W(l, n, k), "coop w");
      blob.at(P.L[l].boff + n, Bs(l, n), "coop b");
    }
  }
  EXPECT(P.L[MZH_VAL0].woff == P.L[MZH_POL0].woff + (size_t)P.L[MZH_POL0].nt * P.L[MZH_POL0].kb * 64 * 4,
         "pol0 / val0 weight strips not adjacent");
  for (int a = 0; a < A; ++a)  // dyn0_onehot [6][256] = dynamic_net.0.weight[:, 64 + a]
    for (int n = 0; n < F; ++n) blob.at(P.onehot + (size_t)a * F + n, W(MZH_DYN0, n, H + a), "coop onehot");

  // ---- wave layout (MzhWMlp, MzhWNet) ----
  for (int i = 0; i < 5; ++i) {
    const PackedW& Q = P.W[i];
    const int l1 = 2 * i, l2 = 2 * i + 1, K1 = i == 1 ? H : in_[l1];
    const bool head33 = sup == 33 && (i == 2 || i == 4), latent = i < 2;
    const int N2 = head33 ? 32 : out_[l2];
    EXPECT(Q.kb1 == (K1 + 15) / 16 && Q.no == (N2 + 15) / 16, "wave mlp %d: kb1 %d no %d", i, Q.kb1, Q.no);
    EXPECT(Q.soff % 4 == 0, "wave mlp %d: s not float4-aligned", i);
    for (int n = 0; n < F; ++n) {  // layer 1: frag (ht, kb)[lane][t] = W1[u(ht, lane&15)][16kb + 4t + (lane>>4)]
      for (int k = 0; k < K1; ++k)
        blob.at(wave_pos(Q, n / 16, k / 16, wave_row(n), k % 4, (k % 16) / 4), W(l1, n, k), "wave w1");
      blob.at(Q.b1off + 16 * (n / 16) + wave_row(n), Bs(l1, n), "wave b1");  // b1[16ht + 4g + i] = bias1[16ht + 4i + g]
    }
    for (int n = 0; n < N2; ++n) {  // layer 2: frag (ht, ot)[lane][t] = W2[pi(ot, lane&15)][16ht + 4t + (lane>>4)]
      int ot = n / 16, r = n % 16;  // natural order
      if (latent) r = wave_row(n);  // pi = u
      if (head33) {  // slot s = 4ot + i of lane group g (row r = 4g + i) holds logit 2g + (s & 1) + 8(s >> 1)
        const int q = n % 8, s = 2 * (n / 8) + (q & 1);
        ot = s / 4;
        r = 4 * (q / 2) + s % 4;
      }
      for (int k = 0; k < F; ++k) blob.at(wave_pos(Q, k / 16, Q.kb1 + ot, r, k % 4, (k % 16) / 4), W(l2, n, k), "wave w2");
      blob.at(Q.b2off + 16 * ot + r, Bs(l2, n), "wave b2");
    }
    if (head33) {  // w32 [16 b][4 g] float4 {W[32][16b + g], [16b + 4 + g], [16b + 8 + g], [16b + 12 + g]}
      EXPECT(Q.w32off != 0 && Q.w32off % 4 == 0, "wave mlp %d: w32 offset %zu", i, Q.w32off);
      for (int k = 0; k < F; ++k) blob.at(Q.w32off + (size_t)((k / 16) * 4 + k % 4) * 4 + (k % 16) / 4, W(l2, 32, k), "w32");
      EXPECT(Q.b32 == (float)(Bs(l2, 32) + 1), "wave mlp %d: b32 = %.1f", i, Q.b32);
    } else {
      EXPECT(Q.w32off == 0 && Q.b32 == 0.0f, "wave mlp %d: bin-32 fields set without a 33-bin head", i);
    }
    // the 17th hidden block pads the stream end with zeros (unconditional prefetch)
    for (size_t p = wave_pos(Q, 16, 0, 0, 0, 0); p < wave_pos(Q, 17, 0, 0, 0, 0); ++p)
      EXPECT(p < P.blob.size() && P.blob[p] == 0.0f, "wave mlp %d: pad block float %zu not zero", i, p);
  }
  for (int a = 0; a < A; ++a)  // oh[a][16ht + 4g + i] = dynamic_net.0.weight[u(ht, 4g + i)][64 + a]
    for (int n = 0; n < F; ++n)
      blob.at(P.wonehot + (size_t)a * F + 16 * (n / 16) + wave_row(n), W(MZH_DYN0, n, H + a), "wave oh");

  // ---- latency layout (MzhOneNet, MZH_ONE_*) ----
  const PackedOne& O = P.one;
  EXPECT(O.l1 % 4 == 0 && O.b1 % 4 == 0 && O.rep2 % 4 == 0 && O.l2 % 4 == 0, "latency float4 array not aligned");
  const int l1_layers[4] = {MZH_DYN0, MZH_RWD0, MZH_POL0, MZH_VAL0};  // l1 k4 blocks 0-15, 16-31, 32-47, 48-63
  for (int u = 0; u < F; ++u) {
    for (int j = 0; j < 4; ++j) {
      for (int k = 0; k < H; ++k)
        blob.at(O.l1 + ((size_t)(16 * j + k / 4) * F + u) * 4 + k % 4, W(l1_layers[j], u, k), "one l1");
      blob.at(O.b1 + 4 * u + j, Bs(l1_layers[j], u), "one b1");
    }
    for (int a = 0; a < A; ++a)  // k4 64-65: the one-hot columns 64..69
      blob.at(O.l1 + ((size_t)(64 + a / 4) * F + u) * 4 + a % 4, W(MZH_DYN0, u, H + a), "one l1 one-hot");
    for (int k = 0; k < in; ++k) blob.at(O.rep0 + (size_t)k * F + u, W(MZH_REP0, u, k), "one rep0");  // [in_dim][256]
    blob.at(O.rep0b + u, Bs(MZH_REP0, u), "one rep0b");
  }
  const size_t D2 = O.l2 + (size_t)MZH_ONE_D2 * 4, A2 = O.l2 + (size_t)MZH_ONE_A2 * 4, P2 = O.l2 + (size_t)MZH_ONE_P2 * 4;
  const size_t C32 = O.l2 + (size_t)MZH_ONE_C32 * 4, B2 = O.l2 + (size_t)MZH_ONE_B2 * 4;
  EXPECT(O.l2 + (size_t)MZH_ONE_L2F4 * 4 == P.blob.size(), "the LDS image does not end the blob");
  for (int j = 0; j < H; ++j) {
    for (int k = 0; k < F; ++k) {
      blob.at(O.rep2 + ((size_t)(k / 4) * 64 + j) * 4 + k % 4, W(MZH_REP2, j, k), "one rep2");  // [64 k4][64] float4
      blob.at(D2 + ((size_t)(k / 4) * 64 + j) * 4 + k % 4, W(MZH_DYN2, j, k), "one D2");
    }
    blob.at(O.rep2b + j, Bs(MZH_REP2, j), "one rep2b");
    blob.at(B2 + j, Bs(MZH_DYN2, j), "one B2 dyn2");
  }
  for (int n = 0; n < nhead; ++n) {  // A2: reward bins in lanes 0-31, value bins in lanes 32-63
    for (int k = 0; k < F; ++k) {
      blob.at(A2 + ((size_t)(k / 4) * 64 + n) * 4 + k % 4, W(MZH_RWD2, n, k), "one A2 rwd");
      blob.at(A2 + ((size_t)(k / 4) * 64 + 32 + n) * 4 + k % 4, W(MZH_VAL2, n, k), "one A2 val");
    }
    blob.at(B2 + 64 + n, Bs(MZH_RWD2, n), "one B2 rwd");
    blob.at(B2 + 96 + n, Bs(MZH_VAL2, n), "one B2 val");
  }
  for (int j = 0; j < A; ++j) {  // P2 [64 k4][8 lanes]
    for (int k = 0; k < F; ++k) blob.at(P2 + ((size_t)(k / 4) * 8 + j) * 4 + k % 4, W(MZH_POL2, j, k), "one P2");
    blob.at(B2 + 128 + j, Bs(MZH_POL2, j), "one B2 pol");
  }
  if (sup == 33) {  // C32 [8 lanes][64 i] floats: lane g the reward chain g (k = g + 4i), lane 4 + g the value chain
    for (int k = 0; k < F; ++k) {
      blob.at(C32 + (size_t)(k % 4) * 64 + k / 4, W(MZH_RWD2, 32, k), "one C32 rwd");
      blob.at(C32 + (size_t)(4 + k % 4) * 64 + k / 4, W(MZH_VAL2, 32, k), "one C32 val");
    }
    blob.at(B2 + 136, Bs(MZH_RWD2, 32), "one B2 rwd bin 32");
    blob.at(B2 + 137, Bs(MZH_VAL2, 32), "one B2 val bin 32");
  }

  // ---- padding: every unclaimed float is +0.0f ----
  for (size_t p = 0; p < P.blob.size(); ++p) {
    uint32_t bits;
    memcpy(&bits, &P.blob[p], 4);
    if (!blob.claimed[p]) EXPECT(bits == 0, "padding float blob[%zu] = %g", p, P.blob[p]);
  }
  // ---- how often the layouts hold each element: once per layout (the one-hot columns in the three
  // one-hot tables instead of the tiles), except bin 32 of a 33-bin head -- its weights sit in the one
  // bin-32 array the cooperative and wave nets share and in the latency image, never in the tiles; its
  // bias travels in the blob only for the latency image (MzhNet::rwd32b / MzhWMlp::b32 are struct fields)
  for (int l = 0; l < 10; ++l)
    for (int n = 0; n < out_[l]; ++n) {
      const bool bin32 = (l == MZH_RWD2 || l == MZH_VAL2) && n == 32;
      for (int k = 0; k < in_[l]; ++k)
        EXPECT(blob.copies[W(l, n, k)] == (bin32 ? 2 : 3), "W(%d, %d, %d) held %d times", l, n, k, blob.copies[W(l, n, k)]);
      EXPECT(blob.copies[Bs(l, n)] == (bin32 ? 1 : 3), "b(%d, %d) held %d times", l, n, blob.copies[Bs(l, n)]);
    }

  // ---- blob identity: FNV-1a 64 over the bytes ----
  uint64_t h = 1469598103934665603ull;
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(P.blob.data());
  for (size_t i = 0; i < P.blob.size() * sizeof(float); ++i) h = (h ^ bytes[i]) * 1099511628211ull;
  EXPECT(h == want_hash, "blob hash %016llx, want %016llx (%zu floats)", (unsigned long long)h, want_hash, P.blob.size());

  if (g_errors) fprintf(stderr, "pack_check(%d, %d): %d failure(s)\n", n_disks, sup, g_errors);
  else printf("pack_check(%d, %d): %zu canonical -> %zu blob floats OK\n", n_disks, sup, sum, P.blob.size());
  return g_errors ? 1 : 0;
}
