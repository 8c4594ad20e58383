// pack_set_check.cpp -- CPU check of mzh_pack_network_set (csrc/mzh_pack.cpp): three different canonical
// vectors packed as a set against mzh_pack_network of each vector alone.  Built with the host sanitizers as a
// stand-alone program (tests/test_multi_cpu.py); usage: pack_set_check <n_disks> <support>.
//   - every blob of the set equals the single-network blob byte for byte, at m * stride
//   - stride = the blob size rounded up to 256 bytes; the floats between two blobs are zero
//   - the [M][2] scalars after the blobs are each network's bin-32 biases (MzhNet::rwd32b / val32b)
//   - the set's layout offsets are those of every member
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../muzero-hanoi_amd/csrc/mzh_pack.h"

static int failures = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++failures;                 \
      std::printf("FAIL: ");      \
      std::printf(__VA_ARGS__);   \
      std::printf("\n");          \
    }                             \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: pack_set_check <n_disks> <support>\n");
    return 2;
  }
  const int in_dim = 3 * std::atoi(argv[1]), support = std::atoi(argv[2]);
  const int M = 3;
  const size_t n = mzh_canon_view(nullptr, in_dim, support).total;
  // three different vectors: every element distinct within a vector and across the vectors
  std::vector<float> flat((size_t)M * n);
  for (int m = 0; m < M; ++m)
    for (size_t i = 0; i < n; ++i) flat[(size_t)m * n + i] = (float)(i + 1) + 0.25f * (float)m;

  const MzhPackedSet S = mzh_pack_network_set(flat.data(), M, in_dim, support);
  CHECK(S.M == M, "M = %d", S.M);
  CHECK(S.layout.blob.empty(), "the layout keeps a blob of %zu floats", S.layout.blob.size());
  for (int m = 0; m < M; ++m) {
    const MzhPacked P = mzh_pack_network(mzh_canon_view(flat.data() + (size_t)m * n, in_dim, support));
    const size_t nb = P.blob.size();
    if (m == 0) {
      CHECK(S.stride % 64 == 0, "stride %zu floats is not a multiple of 256 bytes", S.stride);
      CHECK(S.stride >= nb && S.stride < nb + 64, "stride %zu floats for a blob of %zu", S.stride, nb);
      CHECK(S.scal == (size_t)M * S.stride, "scal at %zu, blobs end at %zu", S.scal, (size_t)M * S.stride);
      CHECK(S.blob.size() == S.scal + 2 * (size_t)M, "set of %zu floats", S.blob.size());
      if (failures) return 1;  // the comparisons below index by these
    }
    CHECK(nb <= S.stride, "network %d: blob of %zu floats above the stride", m, nb);
    const float* got = S.blob.data() + (size_t)m * S.stride;
    CHECK(std::memcmp(got, P.blob.data(), nb * sizeof(float)) == 0, "network %d: blob differs from mzh_pack_network's", m);
    for (size_t i = nb; i < S.stride; ++i) CHECK(got[i] == 0.0f, "network %d: gap float %zu = %g", m, i, (double)got[i]);
    CHECK(std::memcmp(&S.blob[S.scal + 2 * m], &P.W[2].b32, sizeof(float)) == 0, "network %d: reward bin-32 bias", m);
    CHECK(std::memcmp(&S.blob[S.scal + 2 * m + 1], &P.W[4].b32, sizeof(float)) == 0, "network %d: value bin-32 bias", m);
    if (support == 33) {
      const MzhCanon c = mzh_canon_view(flat.data() + (size_t)m * n, in_dim, support);
      CHECK(S.blob[S.scal + 2 * m] == c.b[MZH_RWD2][32] && S.blob[S.scal + 2 * m + 1] == c.b[MZH_VAL2][32],
            "network %d: the scalars are not rwd_net.2.bias[32] / value_net.2.bias[32]", m);
    }
    // one layout for every member
    for (int l = 0; l < 10; ++l)
      CHECK(S.layout.L[l].woff == P.L[l].woff && S.layout.L[l].boff == P.L[l].boff && S.layout.L[l].kb == P.L[l].kb &&
                S.layout.L[l].nt == P.L[l].nt, "network %d: layer %d layout", m, l);
    for (int i = 0; i < 5; ++i)
      CHECK(S.layout.W[i].soff == P.W[i].soff && S.layout.W[i].b1off == P.W[i].b1off && S.layout.W[i].b2off == P.W[i].b2off &&
                S.layout.W[i].w32off == P.W[i].w32off, "network %d: wave MLP %d layout", m, i);
    CHECK(S.layout.onehot == P.onehot && S.layout.wonehot == P.wonehot && S.layout.one.l2 == P.one.l2,
          "network %d: one-hot / latency layout", m);
  }
  // the members really differ (a set that repeated network 0 would pass the layout checks alone)
  CHECK(std::memcmp(S.blob.data(), S.blob.data() + S.stride, S.stride * sizeof(float)) != 0, "networks 0 and 1 are equal");
  CHECK(std::memcmp(S.blob.data() + S.stride, S.blob.data() + 2 * S.stride, S.stride * sizeof(float)) != 0,
        "networks 1 and 2 are equal");
  if (failures) return 1;
  std::printf("ok: %d networks, stride %zu floats\n", M, S.stride);
  return 0;
}
