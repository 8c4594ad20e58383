// saliency_pack_check.cpp -- CPU check of the transposed weight blob (mzh_pack_transposed, csrc/mzh_pack.cpp),
// built with the host sanitizers and run as a child process by tests/test_saliency_cpu.py:
//     saliency_pack_check <n_disks> <support>
//
// Canonical weight i of three networks' vectors laid end to end is (float)(i + 1) (exact: fewer than 2^24
// weights), so every blob float names its source and its network.
// The packer loops blob position -> source element; this program goes the other way: for every weight W[o][i]
// of the six layers between the observation and the two heads it computes, from the layout comment of
// MzhPackedT (mzh_pack.h), the one blob position that must hold it:
//     T4[(nt*KB + kb)*64 + lane][j] = W[16kb + 4j + (lane>>4)][16nt + (lane&15)]
// Then: each position is claimed once, every unclaimed float is +0.0f (the zero padding to 16 of both
// dimensions), every weight of the six layers occurs exactly once and no other element of the canonical vector
// at all, the layers are 16-byte aligned and back to back, the set form lays M such blobs at a 256-byte-multiple
// stride with zeros between them, and mzh_pack_network's blob is the same bytes with or without this packer run.
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

static void check_blob(const float* blob, size_t size, const MzhPackedT& T, const MzhCanon& c, const float* flat) {
  static const int want_layer[MZH_T_LAYERS] = {MZH_REP0, MZH_REP2, MZH_POL0, MZH_POL2, MZH_VAL0, MZH_VAL2};
  std::vector<unsigned char> claimed(size, 0);
  size_t expect_off = 0, weights = 0;
  for (int t = 0; t < MZH_T_LAYERS; ++t) {
    const int l = T.layer[t];
    EXPECT(l == want_layer[t], "entry %d is layer %d, want %d", t, l, want_layer[t]);
    const int O = c.out[l], I = c.in[l];
    EXPECT(T.nt[t] == (I + 15) / 16 && T.kb[t] == (O + 15) / 16, "entry %d: nt=%d kb=%d for [%d][%d]", t, T.nt[t],
           T.kb[t], O, I);
    EXPECT(T.off[t] % 4 == 0 && T.off[t] == expect_off, "entry %d: offset %zu, want %zu", t, T.off[t], expect_off);
    expect_off = T.off[t] + (size_t)T.nt[t] * T.kb[t] * 256;
    for (int o = 0; o < O; ++o)
      for (int i = 0; i < I; ++i) {
        const int nt = i / 16, kb = o / 16, j = (o % 16) / 4, g = o % 4, lane = i % 16 + 16 * g;
        const size_t pos = T.off[t] + (((size_t)nt * T.kb[t] + kb) * 64 + lane) * 4 + j;
        if (pos >= size) {
          EXPECT(false, "entry %d [%d][%d]: position %zu outside the blob (%zu floats)", t, o, i, pos, size);
          continue;
        }
        const size_t src = (size_t)(c.w[l] - flat) + (size_t)o * I + i;
        EXPECT(blob[pos] == (float)(src + 1), "entry %d [%d][%d]: blob[%zu] = %.1f, want source element %zu", t, o, i, pos,
               blob[pos], src);
        EXPECT(!claimed[pos], "entry %d [%d][%d]: blob[%zu] claimed twice", t, o, i, pos);
        claimed[pos] = 1;
        ++weights;
      }
  }
  EXPECT(expect_off == size, "blob has %zu floats, the six layers take %zu", size, expect_off);
  size_t nonzero = 0;
  for (size_t p = 0; p < size; ++p) {
    if (!claimed[p]) {
      uint32_t bits;
      memcpy(&bits, &blob[p], 4);
      EXPECT(bits == 0, "padding blob[%zu] = %g (bits %08x), want +0.0f", p, blob[p], bits);
    } else {
      ++nonzero;
    }
  }
  EXPECT(nonzero == weights, "%zu positions claimed for %zu weights", nonzero, weights);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: saliency_pack_check <n_disks> <support>\n");
    return 2;
  }
  const int n_disks = atoi(argv[1]), support = atoi(argv[2]), in_dim = 3 * n_disks, M = 3;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  std::vector<float> flat((size_t)M * n);
  for (size_t i = 0; i < flat.size(); ++i) flat[i] = (float)(i + 1);  // every member's weights distinct
  const MzhCanon c = mzh_canon_view(flat.data(), in_dim, support);

  const MzhPacked before = mzh_pack_network(c);
  const MzhPackedT T = mzh_pack_transposed(c);
  const MzhPacked after = mzh_pack_network(c);
  EXPECT(before.blob.size() == after.blob.size() &&
             memcmp(before.blob.data(), after.blob.data(), before.blob.size() * sizeof(float)) == 0,
         "mzh_pack_network's blob changed");
  check_blob(T.blob.data(), T.blob.size(), T, c, flat.data());
  EXPECT(T.kb[MZH_T_VAL2] == (support == 33 ? 3 : 1), "value head k-blocks %d", T.kb[MZH_T_VAL2]);

  // the set: member m is network m's blob at m * stride, zeros up to the next member
  const MzhPackedTSet S = mzh_pack_transposed_set(flat.data(), M, in_dim, support);
  EXPECT(S.stride % 64 == 0 && S.stride >= T.blob.size() && S.stride < T.blob.size() + 64, "stride %zu for %zu floats",
         S.stride, T.blob.size());
  EXPECT(S.blob.size() == (size_t)M * S.stride, "set blob %zu floats", S.blob.size());
  EXPECT(S.layout.blob.empty(), "layout keeps a blob");
  for (int m = 0; m < M && S.blob.size() == (size_t)M * S.stride; ++m) {
    const MzhCanon cm = mzh_canon_view(flat.data() + (size_t)m * n, in_dim, support);
    check_blob(S.blob.data() + (size_t)m * S.stride, T.blob.size(), S.layout, cm, flat.data());
    for (size_t p = T.blob.size(); p < S.stride; ++p)
      EXPECT(S.blob[(size_t)m * S.stride + p] == 0.0f, "set member %d: gap float %zu not zero", m, p);
  }
  if (g_errors) {
    fprintf(stderr, "%d errors\n", g_errors);
    return 1;
  }
  printf("ok n_disks=%d support=%d floats=%zu stride=%zu\n", n_disks, support, T.blob.size(), S.stride);
  return 0;
}
