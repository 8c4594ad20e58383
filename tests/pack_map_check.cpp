// pack_map_check.cpp -- CPU check of the pack maps (mzh_pack_maps, csrc/mzh_pack.cpp), built with the host
// sanitizers and run as a child process by tests/test_repack_cpu.py:
//     pack_map_check <n_disks> <support> <fnv1a64 hex>
//
// The device repack gathers blob[j] = map[j] < 0 ? 0 : canonical[map[j]] from the live parameters; this program
// applies the same rule on the host and compares with what the packers write:
//   - applied to i -> i + 1 the main map gives the blob whose FNV-1a 64 hash tests/test_pack_cpu.py records;
//   - applied to seeded random 32-bit patterns (NaNs of every payload, infinities, denormals and -0.0 among
//     them) both maps give mzh_pack_network(...).blob / mzh_pack_transposed(...).blob under memcmp;
//   - the -1 entries are exactly the zeros of an all-ones pack;
//   - every canonical index occurs in the main map; the transposed map holds the six layers it packs once each;
//   - the scalar sources are rwd_net.2.bias[32] / value_net.2.bias[32], -1 at support 1;
//   - the offsets returned are the packers', and every encoded entry names (tensor, offset) of its index.
// On success it prints "<main floats> <transposed floats>" for the Python side to compare with mzh_pack_map.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../muzero-hanoi_amd/csrc/mzh_pack.h"

static int g_errors = 0;
#define EXPECT(cond, ...)                                    \
  do {                                                       \
    if (!(cond)) {                                           \
      if (g_errors++ < 20) {                                 \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
      }                                                      \
    }                                                        \
  } while (0)

// what the gather kernel computes, on 32-bit patterns
static std::vector<float> apply(const std::vector<int32_t>& map, const std::vector<float>& flat) {
  std::vector<float> out(map.size());
  for (size_t j = 0; j < map.size(); ++j) {
    uint32_t bits = 0;
    if (map[j] >= 0) memcpy(&bits, &flat[(size_t)map[j]], 4);
    memcpy(&out[j], &bits, 4);
  }
  return out;
}

static bool same_bytes(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static uint64_t fnv1a(const std::vector<float>& v) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ bytes[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc != 4) return fprintf(stderr, "usage: pack_map_check n_disks support fnv1a64-hex\n"), 2;
  const int n_disks = atoi(argv[1]), sup = atoi(argv[2]), in = 3 * n_disks;
  const unsigned long long want_hash = strtoull(argv[3], nullptr, 16);
  const MzhCanon sizes = mzh_canon_view(nullptr, in, sup);
  const size_t n = sizes.total;

  MzhPackMaps M;
  if (!mzh_pack_maps(in, sup, &M)) return fprintf(stderr, "mzh_pack_maps refused (%d, %d)\n", in, sup), 1;
  for (size_t j = 0; j < M.main.size(); ++j) EXPECT(M.main[j] >= -1 && (size_t)(M.main[j] + 1) <= n, "main[%zu] = %d", j, M.main[j]);
  for (size_t j = 0; j < M.trans.size(); ++j) EXPECT(M.trans[j] >= -1 && (size_t)(M.trans[j] + 1) <= n, "trans[%zu] = %d", j, M.trans[j]);
  if (g_errors) return 1;  // apply() below indexes with the entries

  // ---- i -> i + 1: the recorded hash ----
  std::vector<float> id(n);
  for (size_t i = 0; i < n; ++i) id[i] = (float)(i + 1);
  const uint64_t h = fnv1a(apply(M.main, id));
  EXPECT(h == want_hash, "map applied to i + 1 hashes to %016llx, want %016llx", (unsigned long long)h, want_hash);

  // ---- random bit patterns: memcmp against the packers ----
  std::vector<float> rnd(n);
  uint64_t s = 0x9e3779b97f4a7c15ull ^ ((uint64_t)n_disks << 8) ^ (uint64_t)sup;
  size_t n_nan = 0, n_negzero = 0;
  for (size_t i = 0; i < n; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    uint32_t bits = (uint32_t)(s >> 32);
    if (i % 7 == 3) bits |= 0x7f800000u;   // exponent all ones: NaNs (and a few infinities)
    if (i % 11 == 5) bits = 0x80000000u;   // -0.0
    if (i % 13 == 6) bits &= 0x807fffffu;  // denormals
    n_nan += (bits & 0x7f800000u) == 0x7f800000u && (bits & 0x007fffffu);
    n_negzero += bits == 0x80000000u;
    memcpy(&rnd[i], &bits, 4);
  }
  EXPECT(n_nan > 0 && n_negzero > 0, "the random vector has %zu NaNs and %zu -0.0", n_nan, n_negzero);
  const MzhCanon cr = mzh_canon_view(rnd.data(), in, sup);
  const MzhPacked P = mzh_pack_network(cr);
  const MzhPackedT T = mzh_pack_transposed(cr);
  EXPECT(same_bytes(apply(M.main, rnd), P.blob), "main map applied to random patterns differs from mzh_pack_network");
  EXPECT(same_bytes(apply(M.trans, rnd), T.blob), "transposed map applied to random patterns differs from mzh_pack_transposed");

  // ---- the -1 entries are exactly the zeros of an all-ones pack ----
  const std::vector<float> ones(n, 1.0f);
  const MzhCanon c1 = mzh_canon_view(ones.data(), in, sup);
  const MzhPacked P1 = mzh_pack_network(c1);
  const MzhPackedT T1 = mzh_pack_transposed(c1);
  EXPECT(P1.blob.size() == M.main.size() && T1.blob.size() == M.trans.size(), "map sizes %zu / %zu, blobs %zu / %zu",
         M.main.size(), M.trans.size(), P1.blob.size(), T1.blob.size());
  for (size_t j = 0; j < M.main.size() && j < P1.blob.size(); ++j)
    EXPECT((M.main[j] < 0) == (P1.blob[j] == 0.0f), "main[%zu] = %d where the all-ones pack holds %g", j, M.main[j], P1.blob[j]);
  for (size_t j = 0; j < M.trans.size() && j < T1.blob.size(); ++j)
    EXPECT((M.trans[j] < 0) == (T1.blob[j] == 0.0f), "trans[%zu] = %d where the all-ones pack holds %g", j, M.trans[j], T1.blob[j]);

  // ---- coverage ----
  std::vector<int> seen(n, 0), seen_t(n, 0);
  for (int32_t e : M.main)
    if (e >= 0) ++seen[(size_t)e];
  for (int32_t e : M.trans)
    if (e >= 0) ++seen_t[(size_t)e];
  for (size_t i = 0; i < n; ++i) EXPECT(seen[i] > 0, "canonical index %zu does not occur in the main map", i);
  {  // the transposed blob: the weights (not the biases) of its six layers, once each
    std::vector<int> want_t(n, 0);
    for (int t = 0; t < MZH_T_LAYERS; ++t) {
      const int l = M.tlayout.layer[t];
      const size_t first = (size_t)(cr.w[l] - rnd.data());
      for (size_t i = 0; i < (size_t)sizes.out[l] * sizes.in[l]; ++i) want_t[first + i] = 1;
    }
    for (size_t i = 0; i < n; ++i) EXPECT(seen_t[i] == want_t[i], "canonical index %zu occurs %d times in the transposed map", i, seen_t[i]);
  }

  // ---- the two by-value scalars ----
  const int64_t rwd32 = (int64_t)(cr.b[MZH_RWD2] - rnd.data()) + 32, val32 = (int64_t)(cr.b[MZH_VAL2] - rnd.data()) + 32;
  if (sup == 33) {
    EXPECT(M.scalar_src[0] == rwd32 && M.scalar_src[1] == val32, "scalar sources %lld / %lld, want %lld / %lld",
           (long long)M.scalar_src[0], (long long)M.scalar_src[1], (long long)rwd32, (long long)val32);
    uint32_t a, b;
    memcpy(&a, &P.W[2].b32, 4);
    memcpy(&b, &rnd[(size_t)M.scalar_src[0]], 4);
    EXPECT(a == b, "W[2].b32 is not the value at its scalar source");
    memcpy(&a, &P.W[4].b32, 4);
    memcpy(&b, &rnd[(size_t)M.scalar_src[1]], 4);
    EXPECT(a == b, "W[4].b32 is not the value at its scalar source");
  } else {
    EXPECT(M.scalar_src[0] == -1 && M.scalar_src[1] == -1, "scalar sources %lld / %lld at support %d",
           (long long)M.scalar_src[0], (long long)M.scalar_src[1], sup);
  }

  // ---- the layouts returned are the packers' (blobs empty, b32 left for the caller) ----
  EXPECT(M.layout.blob.empty() && M.tlayout.blob.empty(), "the layouts carry a blob");
  for (int l = 0; l < 10; ++l)
    EXPECT(M.layout.L[l].woff == P.L[l].woff && M.layout.L[l].boff == P.L[l].boff && M.layout.L[l].kb == P.L[l].kb &&
               M.layout.L[l].nt == P.L[l].nt, "layout.L[%d]", l);
  for (int i = 0; i < 5; ++i)
    EXPECT(M.layout.W[i].soff == P.W[i].soff && M.layout.W[i].b1off == P.W[i].b1off && M.layout.W[i].b2off == P.W[i].b2off &&
               M.layout.W[i].w32off == P.W[i].w32off && M.layout.W[i].kb1 == P.W[i].kb1 && M.layout.W[i].no == P.W[i].no &&
               M.layout.W[i].b32 == 0.0f, "layout.W[%d]", i);
  EXPECT(M.layout.onehot == P.onehot && M.layout.wonehot == P.wonehot, "layout one-hot offsets");
  EXPECT(M.layout.one.l1 == P.one.l1 && M.layout.one.b1 == P.one.b1 && M.layout.one.rep0 == P.one.rep0 &&
             M.layout.one.rep0b == P.one.rep0b && M.layout.one.rep2 == P.one.rep2 && M.layout.one.rep2b == P.one.rep2b &&
             M.layout.one.l2 == P.one.l2, "layout.one");
  for (int t = 0; t < MZH_T_LAYERS; ++t)
    EXPECT(M.tlayout.off[t] == T.off[t] && M.tlayout.nt[t] == T.nt[t] && M.tlayout.kb[t] == T.kb[t] &&
               M.tlayout.layer[t] == T.layer[t], "tlayout[%d]", t);

  // ---- the device encoding: (tensor << 24) | offset of every canonical index ----
  EXPECT(mzh_pack_map_encode(sizes, -1) == -1, "encode(-1)");
  EXPECT(mzh_pack_map_encode(sizes, (int64_t)n) == -1, "encode(total) names an element");
  for (int l = 0; l < 10; ++l) {
    const size_t w0 = (size_t)(cr.w[l] - rnd.data()), b0 = (size_t)(cr.b[l] - rnd.data());
    const size_t nw = (size_t)sizes.out[l] * sizes.in[l];
    for (size_t i : {(size_t)0, nw / 2, nw - 1})
      EXPECT(mzh_pack_map_encode(sizes, (int64_t)(w0 + i)) == (int32_t)(((2 * l) << 24) | (int32_t)i), "encode weight %d + %zu", l, i);
    for (size_t i : {(size_t)0, (size_t)sizes.out[l] - 1})
      EXPECT(mzh_pack_map_encode(sizes, (int64_t)(b0 + i)) == (int32_t)(((2 * l + 1) << 24) | (int32_t)i), "encode bias %d + %zu", l, i);
  }

  // ---- a shape of 2^24 or more weights is refused (no such engine exists; the guard of i + 1 being exact) ----
  MzhPackMaps big;
  EXPECT(!mzh_pack_maps(70000, 33, &big) && big.main.empty(), "a shape of more than 2^24 weights was mapped");

  if (g_errors) {
    fprintf(stderr, "pack_map_check(%d, %d): %d failure(s)\n", n_disks, sup, g_errors);
    return 1;
  }
  printf("%zu %zu\n", M.main.size(), M.trans.size());
  return 0;
}
