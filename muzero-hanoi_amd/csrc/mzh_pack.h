// mzh_pack.h -- the canonical flat weight vector and its three packed device layouts.  Host-only plain
// C++ (no HIP types; mzh_pack.cpp is compiled by g++): the packers only copy, the kernels define what the
// copies mean.  The layouts are documented where the kernels read them:
//   cooperative  MzhLayer / MzhNet            (mzh_device.h)
//   wave         MzhWMlp / MzhWNet            (mzh_internal.h)
//   latency      MzhOneNet, MZH_ONE_* below   (mzh_internal.h)
#pragma once
#include <vector>

#include "../../include/mzh.h"

// the ten nn.Linear layers in state_dict order (engine.WEIGHT_KEYS: weight then bias of each);
// MLP i (representation, dynamics, reward, policy, value) is the layer pair 2i, 2i + 1
enum MzhLayerId { MZH_REP0, MZH_REP2, MZH_DYN0, MZH_DYN2, MZH_RWD0, MZH_RWD2, MZH_POL0, MZH_POL2, MZH_VAL0, MZH_VAL2 };

// view over the canonical flat vector: layer l is w[l] [out[l]][in[l]] then b[l] [out[l]]
struct MzhCanon {
  const float* w[10];
  const float* b[10];
  int out[10], in[10];
  int in_dim, support;
  size_t total;  // floats
};
// flat == nullptr: sizes only (w / b stay null)
MzhCanon mzh_canon_view(const float* flat, int in_dim, int support);

// float offsets into the blob of one cooperative-layout layer, one wave-layout MLP, the latency layout
struct PackedLayer {
  size_t woff = 0, boff = 0;
  int kb = 0, nt = 0;
};
struct PackedW {
  size_t soff = 0, b1off = 0, b2off = 0, w32off = 0;
  float b32 = 0.0f;
  int kb1 = 0, no = 0;
};
struct PackedOne {
  size_t l1 = 0, b1 = 0, rep0 = 0, rep0b = 0, rep2 = 0, rep2b = 0, l2 = 0;
};

struct MzhPacked {
  std::vector<float> blob;  // the device buffer's contents
  PackedLayer L[10];        // by MzhLayerId
  size_t onehot = 0;        // MzhNet::dyn0_onehot
  PackedW W[5];             // by MLP
  size_t wonehot = 0;       // MzhWNet::oh
  PackedOne one;
};
MzhPacked mzh_pack_network(const MzhCanon& c);

// A set of M networks of one shape (mzh_load_weight_set): each canonical vector packed by mzh_pack_network,
// unchanged, and the M blobs laid at a constant stride -- one blob rounded up to 256 bytes -- in one buffer.
// The offsets depend only on in_dim and support, so `layout` (network 0's, its blob moved into `blob`)
// describes every member.  The two scalars MzhNet carries by value follow the blobs as [M][2] floats.
struct MzhPackedSet {
  std::vector<float> blob;  // [M] blobs at `stride` floats (zero between them), then scal [M][2]
  size_t stride = 0;        // floats between two networks' blobs (a multiple of 64: 256 bytes)
  size_t scal = 0;          // float offset of [M][2] {W[2].b32 (reward bin 32 bias), W[4].b32 (value)}
  int M = 0;
  MzhPacked layout;         // offsets of one member; layout.blob is empty
};
// flat: [M][n] canonical vectors, n = mzh_canon_view(nullptr, in_dim, support).total
MzhPackedSet mzh_pack_network_set(const float* flat, int M, int in_dim, int support);

// The transposed layout of the saliency kernel's backward (mzh_saliency.hip): dX = dY . W takes W with
// k = out as the MFMA B operand, so layer [O][I] is stored as the cooperative layout of its transpose --
// tile nt (16 input columns) x k-block kb (16 outputs) x lane -> one float4:
//     T4[(nt*KB + kb)*64 + lane][j] = W[16kb + 4j + (lane>>4)][16nt + (lane&15)]
// with NT = ceil(I / 16), KB = ceil(O / 16), zero beyond O and I.  Only the six layers between the
// observation and the two heads, all 33 bins of a 33-bin value head as tiles (KB = 3).  A blob of its own:
// mzh_pack_network's bytes and offsets are not touched.
enum { MZH_T_REP0, MZH_T_REP2, MZH_T_POL0, MZH_T_POL2, MZH_T_VAL0, MZH_T_VAL2, MZH_T_LAYERS };
struct MzhPackedT {
  std::vector<float> blob;
  size_t off[MZH_T_LAYERS];  // float offsets, each a multiple of 4
  int nt[MZH_T_LAYERS], kb[MZH_T_LAYERS];
  int layer[MZH_T_LAYERS];   // MzhLayerId of each entry
};
MzhPackedT mzh_pack_transposed(const MzhCanon& c);
// M such blobs at `stride` floats (one blob rounded up to 256 bytes); layout.blob is empty
struct MzhPackedTSet {
  std::vector<float> blob;
  size_t stride = 0;
  MzhPackedT layout;
};
MzhPackedTSet mzh_pack_transposed_set(const float* flat, int M, int in_dim, int support);

// The packers as a permutation with zero fill (they only copy): entry j of a map is the canonical index
// (mzh_canon_view order) whose value blob float j holds, or -1 where the blob holds +0.0f.  Derived by running
// mzh_pack_network / mzh_pack_transposed on the vector i -> (float)(i + 1), so the layouts keep their one
// definition above.  The device repack (mzh_repack.hip) gathers through these maps from the live parameters.
struct MzhPackMaps {
  std::vector<int32_t> main, trans;  // one entry per blob float of MzhPacked / MzhPackedT
  MzhPacked layout;                  // the offsets make_net needs; blob empty, W[i].b32 zero
  MzhPackedT tlayout;                // the offsets make_tnet needs; blob empty
  int64_t scalar_src[2];             // canonical index of W[2].b32 / W[4].b32 (bias bin 32 of the reward / value
                                     // head, taken by value by the kernels), -1 without a 33-bin head
};
// false (nothing written) for a shape with 2^24 or more weights: i + 1 would no longer be exact in a float
bool mzh_pack_maps(int in_dim, int support, MzhPackMaps* out);
// a map entry as the device reads it: (tensor << 24) | offset inside that tensor, tensor = 2 * layer (weight) or
// 2 * layer + 1 (bias) in state_dict order; -1 stays -1.  The largest tensor has 256 * 96 < 2^24 elements
int32_t mzh_pack_map_encode(const MzhCanon& sizes, int64_t canon_index);

// The two further transposed layers of the parameter-gradient kernel (mzh_pgrad.hip): dynamic_net.2 and
// rwd_net.2 in MzhPackedT's fragment format (all 33 bins of a 33-bin reward head as tiles, KB = 3).  No load
// packs them: the engine gathers them on the device from the main blob through `src`, which composes this
// layout with the inverse of mzh_pack_maps' main map (every canonical element lies somewhere in the main blob).
enum { MZH_G_DYN2, MZH_G_RWD2, MZH_G_LAYERS };
struct MzhPackedG {
  std::vector<float> blob;
  size_t off[MZH_G_LAYERS];  // float offsets, each a multiple of 4
  int nt[MZH_G_LAYERS], kb[MZH_G_LAYERS];
};
// the direct pack from the canonical vector (what the gather must reproduce; tests/pgrad_map_check.cpp)
MzhPackedG mzh_pack_pgrad(const MzhCanon& c);
struct MzhPgradMap {
  std::vector<int32_t> src;  // entry j: the main-blob float that buffer float j copies, -1 where it is +0.0f
  MzhPackedG layout;         // blob empty
};
// false (nothing written) where mzh_pack_maps refuses the shape, or an element is missing from the main blob
bool mzh_pgrad_map(int in_dim, int support, MzhPgradMap* out);

// the latency layout's LDS image `l2`: offsets in float4 units
#define MZH_ONE_D2 0                        // dynamic_net.2 [64 k4][64 lanes]
#define MZH_ONE_A2 (64 * 64)                // rwd_net.2 bins 0-31 (lanes 0-31) | value_net.2 bins 0-31 (lanes 32-63)
#define MZH_ONE_P2 (2 * 64 * 64)            // policy_net.2 [64 k4][8 lanes] (6 rows + 2 zero)
#define MZH_ONE_C32 (MZH_ONE_P2 + 64 * 8)   // bin 32 chains [8 lanes][64 i] floats: lane g < 4 the reward head's
                                            // chain g (k = g + 4i), lane 4 + g the value head's (128 float4)
#define MZH_ONE_B2 (MZH_ONE_C32 + 128)      // biases (floats): [0,64) dynamic_net.2, [64,128) the A2 rows,
                                            // [128,136) policy_net.2, 136 / 137 bin 32 of reward / value
#define MZH_ONE_L2F4 (MZH_ONE_B2 + 36)      // float4s of the LDS image
