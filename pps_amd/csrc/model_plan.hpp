// The structure of the PPS test net, host only: the layer plan the reference's
// builders produce, with the same blob and parameter names (mirrored one for
// one by pps_amd/model.py, compared field by field in
// tests/test_model_plan_host.py), and the decoder of the plan's tile words.
// Nothing here touches the device; the only includes are the standard library
// and the ABI header.
//   add_ResNet50_conv5_body  detectron/modeling/ResNet.py:39-40,91-126
//     basic_bn_stem          ResNet.py:246-256
//     add_stage              ResNet.py:60-88
//     add_residual_block     ResNet.py:153-195 (stride rule :169-171)
//     bottleneck_transformation ResNet.py:276-333 (STRIDE_1X1 :290)
//     basic_bn_shortcut      ResNet.py:203-220
//   FPN coarsest level       detectron/modeling/FPN_reid.py:160-174 (gated)
//   add_pps_part_head        detectron/modeling/pps_heads.py:38-96
//     add_uniform_partition  detectron/modeling/bpm_heads.py:18-55
//   add_reid_outputs         detectron/modeling/reid_heads.py:34-127
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/pps_abi.h"

// internal to the library: the inline definitions below stay out of its
// dynamic symbol table
#pragma GCC visibility push(hidden)
namespace pps {

// ---- tile words ---------------------------------------------------------------
// A layer's tile word: a GemmTile id in the low byte, PPS_TILE_* flags above it.
constexpr int kTileFlagMask = 0x3f00;
static_assert(kTileFlagMask == (PPS_TILE_B_TILED | PPS_TILE_COL_ORDER | PPS_TILE_SEAM |
                                PPS_TILE_H2 | PPS_TILE_H2P | PPS_TILE_H2E),
              "a new PPS_TILE_* flag belongs in kTileFlagMask");
static_assert((kTileFlagMask & 0xff) == 0, "the tile flags overlap the tile id byte");

constexpr int tile_base(int t) { return t & ~kTileFlagMask; }  // the id (a stray high bit stays)
constexpr bool tile_h2(int t) { return (t & PPS_TILE_H2) != 0; }
// the two plane flags modify an f16x2 tile: without PPS_TILE_H2 they mean nothing
constexpr bool tile_h2p(int t) { return tile_h2(t) && (t & PPS_TILE_H2P) != 0; }
constexpr bool tile_h2e(int t) { return tile_h2(t) && (t & PPS_TILE_H2E) != 0; }
constexpr bool tile_seam(int t) { return (t & PPS_TILE_SEAM) != 0; }

// ---- plan (structure only) ----------------------------------------------------
enum class Op { Conv, ConvDual, MaxPool, StemPool, Pps, ConvPps, Heads, Normalize };

inline const char* op_name(Op op) {
  switch (op) {
    case Op::Conv: return "conv";
    case Op::ConvDual: return "conv_dual";
    case Op::MaxPool: return "maxpool";
    case Op::StemPool: return "stem_pool";
    case Op::Pps: return "pps";
    case Op::ConvPps: return "conv_pps";
    case Op::Heads: return "heads";
    case Op::Normalize: return "normalize";
  }
  return "?";
}

struct PlanLayer {
  Op op;
  std::string name, bn, input, output, residual;
  int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, dil = 1;
  bool relu = false;
  std::vector<int> split;  // pps
  bool max_ave = false;
  std::vector<std::string> prefixes;
  int dim = 0, dim_inner = 0;
};

struct Plan {
  std::vector<PlanLayer> layers;
  std::map<std::string, std::vector<int64_t>> params;
  std::string output;
  int feat_dim = 0;

  std::string conv(const std::string& in, const std::string& prefix, int din, int dout, int k,
                   int stride, int pad, int dil = 1, bool relu = false,
                   const std::string& residual = "", const std::string& out = "",
                   bool bias = false, const std::string& bn_name = "") {
    params[prefix + "_w"] = {dout, din, k, k};
    if (bias) params[prefix + "_b"] = {dout};
    const std::string bn = bn_name.empty() ? prefix + "_bn" : bn_name;
    for (const char* s : {"_s", "_b", "_rm", "_riv"}) params[bn + s] = {dout};
    PlanLayer L;
    L.op = Op::Conv; L.name = prefix; L.bn = bn; L.input = in;
    L.output = out.empty() ? bn : out;
    L.cin = din; L.cout = dout; L.k = k; L.stride = stride; L.pad = pad; L.dil = dil;
    L.relu = relu; L.residual = residual;
    layers.push_back(L);
    return L.output;
  }
};

// model.py basic_bn_stem (ResNet.py:246-256)
inline std::string basic_bn_stem(Plan& p) {
  const std::string c = p.conv("data", "conv1", 3, 64, 7, 2, 3, 1, true, "", "", false, "res_conv1_bn");
  PlanLayer L;
  L.op = Op::MaxPool; L.input = c; L.output = "pool1"; L.k = 3; L.stride = 2; L.pad = 1;
  p.layers.push_back(L);
  return "pool1";
}

// ResNet.py:276-333 (+ the Sum/Relu of add_residual_block :186-195)
inline std::string bottleneck(Plan& p, const PpsModelConfig& c, const std::string& in, int din,
                              int dout, int stride, const std::string& prefix, int dinner, int dil,
                              const std::string& shortcut, const std::string& out) {
  const int s1 = c.stride_1x1 ? stride : 1, s3 = c.stride_1x1 ? 1 : stride;
  std::string cur = p.conv(in, prefix + "_branch2a", din, dinner, 1, s1, 0, 1, true);
  cur = p.conv(cur, prefix + "_branch2b", dinner, dinner, 3, s3, dil, dil, true);
  return p.conv(cur, prefix + "_branch2c", dinner, dout, 1, 1, 0, 1, true, shortcut, out);
}

// ResNet.py:153-195 with basic_bn_shortcut :203-220
inline std::string residual_block(Plan& p, const PpsModelConfig& c, const std::string& prefix,
                                  const std::string& in, int din, int dout, int dinner, int dil,
                                  int stride_init, bool inplace_sum) {
  const int stride = (din != dout && din != 64 && dil == 1) ? stride_init : 1;
  std::string sc = in;
  if (din != dout) sc = p.conv(in, prefix + "_branch1", din, dout, 1, stride, 0);
  const std::string out = prefix + (inplace_sum ? "_branch2c_bn" : "_sum");
  return bottleneck(p, c, in, din, dout, stride, prefix, dinner, dil, sc, out);
}

// ResNet.py:60-88
inline std::string add_stage(Plan& p, const PpsModelConfig& c, const std::string& prefix,
                             std::string in, int n, int& din, int dout, int dinner, int dil,
                             int stride_init) {
  for (int i = 0; i < n; ++i) {
    in = residual_block(p, c, prefix + "_" + std::to_string(i), in, din, dout, dinner, dil,
                        stride_init, i < n - 1);
    din = dout;
  }
  return in;
}

// bpm_heads.py:18-35: strip heights along H
inline std::vector<int> uniform_partition_split(const PpsModelConfig& c, double spatial_scale) {
  static const std::map<int, std::vector<int>> table = {
      {7, {3, 3, 4, 4, 4, 3, 3}}, {5, {5, 5, 4, 5, 5}},
      {9, {2, 3, 3, 3, 3, 3, 3, 2, 2}}, {10, {2, 2, 2, 3, 3, 3, 3, 2, 2, 2}}};
  std::vector<int> out;
  auto it = table.find(c.strip_num);
  if (it != table.end() && c.height == 16 * 24) {
    const double scale = 16 * spatial_scale;
    for (int s : it->second) out.push_back((int)(s * scale));
    return out;
  }
  const int h = (int)(c.height * spatial_scale / c.strip_num);
  out.assign(c.strip_num, h);
  return out;
}

inline Plan build_plan(const PpsModelConfig& c) {
  Plan p;
  std::string s = basic_bn_stem(p);
  int din = 64;
  const int db = c.num_groups * c.width_per_group;
  s = add_stage(p, c, "res2", s, 3, din, 256, db, 1, 2);
  s = add_stage(p, c, "res3", s, 4, din, 512, db * 2, 1, 2);
  s = add_stage(p, c, "res4", s, 6, din, 1024, db * 4, 1, 2);
  s = add_stage(p, c, "res5", s, 3, din, 2048, db * 8, c.res5_dilation, c.res5_stride);
  const double scale = 1. / 16. * c.res5_dilation / c.res5_stride;
  int dim = din;
  if (c.fpn_on && dim != c.fpn_dim) {  // FPN_reid.py:160-174 (coarsest level only)
    s = p.conv(s, "fpn_inner_" + s, dim, c.fpn_dim, 1, 1, 0, 1, true, "", "", true,
               "fpn_inner_" + s + "_bn");
    dim = c.fpn_dim;
  }
  // pps_heads.py:38-96: subset i = bits of i; blob prefix pps + digits
  PlanLayer P;
  P.op = Op::Pps; P.input = s; P.output = "pps_pool2_all"; P.dim = dim;
  P.split = uniform_partition_split(c, scale);
  P.max_ave = c.max_ave != 0;
  for (int i = 1; i < (1 << c.strip_num); ++i) {
    std::string pre = "pps";
    for (int j = 0; j < c.strip_num; ++j)
      if (i & (1 << j)) pre += std::to_string(j);
    P.prefixes.push_back(pre);
  }
  p.layers.push_back(P);
  // reid_heads.py:34-127 (test branch; the unused FC logits are not built)
  for (const auto& pre : P.prefixes) {
    p.params[pre + "_conv_w"] = {c.bpm_dim, dim, 1, 1};
    p.params[pre + "_conv_b"] = {c.bpm_dim};
    for (const char* sfx : {"_s", "_b", "_rm", "_riv"}) p.params[pre + "_bn" + sfx] = {c.bpm_dim};
  }
  PlanLayer H;
  H.op = Op::Heads; H.input = P.output; H.prefixes = P.prefixes; H.dim = dim;
  H.dim_inner = c.bpm_dim; H.output = "reid_feature_concat";
  p.layers.push_back(H);
  p.output = H.output;
  if (c.normalize) {
    PlanLayer N;
    N.op = Op::Normalize; N.input = H.output; N.output = "reid_feature_concat_norm";
    p.layers.push_back(N);
    p.output = N.output;
  }
  p.feat_dim = (int)P.prefixes.size() * c.bpm_dim;
  return p;
}

}  // namespace pps
#pragma GCC visibility pop
