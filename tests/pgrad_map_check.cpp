// pgrad_map_check.cpp -- the gather map of mzh_param_grads' extra transposed buffer (mzh_pgrad_map, mzh_pack.h),
// checked on the host as its own program: a random network packed by mzh_pack_network, gathered through the map
// as the device gather does it, must equal the direct transposed pack (mzh_pack_pgrad) float for float, and that
// pack must hold every weight of dynamic_net.2 and rwd_net.2 where MzhPackedT's formula puts it.
//     g++ -std=c++17 -I include tests/pgrad_map_check.cpp muzero-hanoi_amd/csrc/mzh_pack.cpp && ./a.out 3 33
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../muzero-hanoi_amd/csrc/mzh_pack.h"

int main(int argc, char** argv) {
  const int n_disks = argc > 1 ? atoi(argv[1]) : 3, support = argc > 2 ? atoi(argv[2]) : 33;
  const int in_dim = 3 * n_disks;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  std::vector<float> flat(n);
  unsigned s = 12345u + 7u * n_disks + support;
  for (size_t i = 0; i < n; ++i) {  // distinct non-zero values: a wrong source cannot pass by coincidence
    s = s * 1664525u + 1013904223u;
    flat[i] = (float)(i + 1) + (float)(s >> 24) / 512.0f;
  }
  const MzhCanon c = mzh_canon_view(flat.data(), in_dim, support);
  const MzhPacked P = mzh_pack_network(c);
  const MzhPackedG G = mzh_pack_pgrad(c);
  MzhPgradMap M;
  if (!mzh_pgrad_map(in_dim, support, &M)) {
    printf("FAIL no map\n");
    return 1;
  }
  if (M.src.size() != G.blob.size() || M.src.size() % 4) {
    printf("FAIL sizes map %zu blob %zu\n", M.src.size(), G.blob.size());
    return 1;
  }
  for (int t = 0; t < MZH_G_LAYERS; ++t)
    if (M.layout.off[t] != G.off[t] || M.layout.nt[t] != G.nt[t] || M.layout.kb[t] != G.kb[t] || G.off[t] % 4) {
      printf("FAIL layout of layer %d\n", t);
      return 1;
    }
  size_t copies = 0;
  for (size_t j = 0; j < M.src.size(); ++j) {
    const int32_t src = M.src[j];
    if (src >= (int64_t)P.blob.size()) {
      printf("FAIL entry %zu = %d beyond the main blob of %zu floats\n", j, src, P.blob.size());
      return 1;
    }
    const float got = src >= 0 ? P.blob[src] : 0.0f;
    if (memcmp(&got, &G.blob[j], sizeof(float)) != 0) {
      printf("FAIL float %zu: gathered %g, direct pack %g\n", j, got, G.blob[j]);
      return 1;
    }
    copies += src >= 0;
  }
  // the direct pack against the formula T4[(nt*KB + kb)*64 + lane][j] = W[16kb + 4j + (lane>>4)][16nt + (lane&15)]
  const int layers[MZH_G_LAYERS] = {MZH_DYN2, MZH_RWD2};
  size_t weights = 0;
  for (int t = 0; t < MZH_G_LAYERS; ++t) {
    const int l = layers[t], O = c.out[l], I = c.in[l];
    if (G.nt[t] != (I + 15) / 16 || G.kb[t] != (O + 15) / 16) {
      printf("FAIL tiles of layer %d\n", t);
      return 1;
    }
    for (int nt = 0; nt < G.nt[t]; ++nt)
      for (int kb = 0; kb < G.kb[t]; ++kb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int o = 16 * kb + 4 * j + (lane >> 4), i = 16 * nt + (lane & 15);
            const float want = (o < O && i < I) ? c.w[l][(size_t)o * I + i] : 0.0f;
            if (G.blob[G.off[t] + (((size_t)nt * G.kb[t] + kb) * 64 + lane) * 4 + j] != want) {
              printf("FAIL layer %d element [%d][%d]\n", t, o, i);
              return 1;
            }
          }
    weights += (size_t)O * I;
  }
  if (copies != weights) {
    printf("FAIL %zu copies for %zu weights\n", copies, weights);
    return 1;
  }
  printf("ok n_disks=%d support=%d floats=%zu copies=%zu\n", n_disks, support, M.src.size(), copies);
  return 0;
}
