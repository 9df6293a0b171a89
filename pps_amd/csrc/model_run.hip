// The run side of the whole-network plan: tensor shapes and the per-batch
// workspace, the structural predicates of the tile table, one layer's launch
// (run_layer: the tile word decoded once, then one function per op) and the
// forward over a layer range.  Each launch goes through the same pps_* entry
// point, with the same arguments, as the Python orchestrator (pps_amd/model.py
// PPSModel), so the two give identical bits for the same tile / plane /
// split-K table.
#include <algorithm>

#include "model_internal.hpp"

namespace pps {

// ---- shapes -------------------------------------------------------------------
namespace {
int conv_out(int h, int pad, int dil, int k, int stride) {
  return (h + 2 * pad - dil * (k - 1) - 1) / stride + 1;
}
}  // namespace

int count_readers(const PpsModel& m, const std::string& blob, bool all_keys) {
  int n = 0;
  for (const auto& L : m.layers) {
    if (L.input == blob) ++n;
    if (all_keys && (L.input2 == blob || L.residual == blob)) ++n;
  }
  return n;
}

Shapes infer_shapes(const PpsModel& m, int N) {
  Shapes s;
  s["data"] = Shape{{N, m.cfg.height, m.cfg.width, 4}};
  for (const auto& L : m.layers) {
    const Shape& x = s.at(L.input);
    switch (L.op) {
      case Op::Conv: case Op::ConvDual:
        s[L.output] = Shape{{x.d[0], conv_out((int)x.d[1], L.pad, L.dil, L.k, L.stride),
                             conv_out((int)x.d[2], L.pad, L.dil, L.k, L.stride), L.cout}};
        break;
      case Op::MaxPool:
        s[L.output] = Shape{{x.d[0], (x.d[1] + 2 * L.pad - L.k) / L.stride + 1,
                             (x.d[2] + 2 * L.pad - L.k) / L.stride + 1, x.d[3]}};
        break;
      case Op::StemPool: {
        const int64_t hc = (x.d[1] - 1) / 2 + 1, wc = (x.d[2] - 1) / 2 + 1;
        s[L.output] = Shape{{x.d[0], (hc - 1) / 2 + 1, (wc - 1) / 2 + 1, L.cout}};
        break;
      }
      case Op::Pps:
        s[L.output] = Shape{{L.nsub, x.d[0], x.d[3], 1}};
        break;
      case Op::ConvPps:
        s[L.conv_output] = Shape{{x.d[0], conv_out((int)x.d[1], L.pad, L.dil, L.k, L.stride),
                                  conv_out((int)x.d[2], L.pad, L.dil, L.k, L.stride), L.cout}};
        s[L.output] = Shape{{L.nsub, x.d[0], L.cout, 1}};
        break;
      case Op::Heads:
        s[L.output] = Shape{{N, (int64_t)L.nsub * L.dim_inner, 1, 1}};
        s[L.output + "_partials"] = Shape{{kHeadSplitK, N, (int64_t)L.nsub * L.dim_inner, 1}};
        break;
      case Op::Normalize:
        s[L.output] = x;
        break;
    }
  }
  return s;
}

std::vector<int> pps_tiles(const Layer& L, const Shape& conv_shape) {
  std::vector<int> out;
  const int rows = (int)(conv_shape.d[1] * conv_shape.d[2]);
  for (int t = GEMM_TILE_P_FIRST; t < GEMM_NUM_TILES; ++t) {
    const int r = x3p_tile_rows(t, L.planes_in), c = x3p_tile_cols(t, L.planes_in);
    if (r == rows && c > 0 && c <= kPpsFuseMaxCols) out.push_back(t);
  }
  return out;
}

bool tunable(const Layer& L) {
  return L.op == Op::Conv || L.op == Op::ConvDual || L.op == Op::Heads || L.op == Op::ConvPps;
}

double layer_flops(const Layer& L, const Shapes& s, int N) {
  switch (L.op) {
    case Op::StemPool: {
      const Shape& x = s.at(L.input);
      const double hc = (double)((x.d[1] - 1) / 2 + 1), wc = (double)((x.d[2] - 1) / 2 + 1);
      return 2.0 * N * hc * wc * L.cout * L.k * L.k * L.cin;  // true Cin = 3
    }
    case Op::Conv: case Op::ConvDual: case Op::ConvPps: {
      const Shape& y = s.at(L.op == Op::ConvPps ? L.conv_output : L.output);
      return 2.0 * y.d[0] * y.d[1] * y.d[2] * y.d[3] * ((double)L.k * L.k * L.cin + L.shortcut_cin);
    }
    case Op::Heads:
      return 2.0 * N * L.nsub * L.dim_inner * L.dim;
    default:
      return 0.0;
  }
}

// algorithmic HBM bytes per launch: every operand read once, the output
// written once (model.py PPSModel._alloc)
double layer_bytes(const PpsModel& m, const Layer& L, const Shapes& s, int N) {
  const double wb = m.x3 && !tile_h2(L.tile) ? 6.0 : 4.0;  // f16x2 weights: 4 B
  switch (L.op) {
    case Op::StemPool:
      return 4.0 * s.at(L.input).numel() + 4.0 * s.at(L.output).numel() +
             wb * L.cout * pps_stem_k();
    case Op::Conv: case Op::ConvDual: {
      const Shape& y = s.at(L.output);
      const double pix = (double)y.d[0] * y.d[1] * y.d[2];
      // a 1x1 (k < stride) conv reads only the pixels under its taps: one
      // input pixel per output position and tap, not the whole tensor
      const double in = L.k < L.stride ? 4.0 * pix * L.k * L.k * L.cin
                                       : 4.0 * s.at(L.input).numel();
      double b = in + 4.0 * y.numel() + wb * L.cout * ((double)L.k * L.k * L.cin + L.shortcut_cin);
      if (!L.residual.empty()) b += 4.0 * y.numel();
      if (L.op == Op::ConvDual)  // the 1x1 shortcut, stride2
        b += L.stride2 > 1 ? 4.0 * pix * L.shortcut_cin : 4.0 * s.at(L.input2).numel();
      return b;
    }
    case Op::ConvPps: {
      const Shape& y = s.at(L.conv_output);
      return 4.0 * s.at(L.input).numel() + 4.0 * y.numel() +
             wb * L.cout * (double)L.k * L.k * L.cin + 4.0 * s.at(L.output).numel();
    }
    case Op::Heads:
      return 4.0 * s.at(L.input).numel() + wb * L.nsub * L.dim_inner * L.dim +
             4.0 * kHeadSplitK * N * L.nsub * L.dim_inner;
    default:
      return 0.0;
  }
}

// ---- structural predicates of the tile table ----------------------------------
bool seam_ok(const PpsModel& m, const Layer& L) {
  if (L.seam_next < 0) return false;
  const Layer& X = m.layers[L.seam_next];
  return !L.planes_in && !L.planes_out && !X.planes_out && L.splitk == 1 && X.splitk == 1;
}

namespace {
// A layer the f16x2 weight-stationary kernel takes (gemm_ws.hip ws_eligible):
// a 1x1 / stride-1 / unpadded conv, or the fused shortcut conv, whose K =
// Cin (+ the shortcut's Cin) is 64, 128 or 256
bool ws_h2_layer(const Layer& L) {
  if (!is_conv(L)) return false;
  if (L.k != 1 || L.stride != 1 || L.pad != 0 || L.kpad != L.cin_eff) return false;
  const int K = layer_k(L);
  return (K == 64 || K == 128 || K == 256) && L.cout % 64 == 0;
}
}  // namespace

// A PPS_TILE_H2 tile this layer can run (the word carries PPS_TILE_H2)
bool h2_tile_ok(const Layer& L, int tile) {
  const int base = tile_base(tile);
  if (!L.w2 || tile_seam(tile)) return false;
  // the fused stem: its own kernel, no tile id, no planes at either end
  if (L.op == Op::StemPool) return tile == PPS_TILE_H2;
  // activation planes: plain convs and conv_pps (the fused shortcut reads f32)
  if ((tile_h2p(tile) || tile_h2e(tile)) && L.op == Op::ConvDual) return false;
  if (tile_h2p(tile) && tile_h2e(tile)) return false;
  if (L.op != Op::Conv && L.op != Op::ConvDual && L.op != Op::ConvPps) return false;
  if (!L.relu && L.op == Op::Conv) return false;  // the f16x2 epilogues end in a ReLU
  if (base == 0) return true;
  if (base == GEMM_TILE_WS)  // the weight-stationary 1x1 (f32 input, K = 64 / 128 / 256)
    return ws_h2_layer(L) && !tile_h2p(tile) && !tile_h2e(tile);
  if (!tile_rounds_16(base)) return false;
  return L.op == Op::Conv || tile_kind(base) != TileKind::Patch;  // patch tiles: plain convs
}

// The producer whose f16x2-planes output a PPS_TILE_H2E layer C reads, or -1
int h2e_producer(const PpsModel& m, const Layer& C) {
  if (C.op != Op::Conv && C.op != Op::ConvPps) return -1;
  for (size_t i = 0; i < m.layers.size(); ++i) {
    const Layer& P = m.layers[i];
    if (P.output != C.input) continue;
    if (P.op != Op::Conv || !P.relu || !P.residual.empty() || P.h2o_bw <= 0.f) return -1;
    if (count_readers(m, P.output, true) != 1) return -1;
    if (i > 0 && m.layers[i - 1].seam_next == (int)i) return -1;  // a seam pair's second half
    return (int)i;
  }
  return -1;
}

// tiles built with the one-launch split-K epilogue (the tile table's FX)
bool fix_tile(int tile) { return x3p_tile_fix(tile_base(tile)); }

// ---- workspaces -----------------------------------------------------------------
namespace {
// f16x2 activation planes of the largest PPS_TILE_H2P input (2 x int16 per element)
size_t h2p_need(const PpsModel& m, const Shapes& shapes) {
  size_t need = 0;
  for (const auto& L : m.layers)
    if (tile_h2p(L.tile)) need = std::max(need, (size_t)shapes.at(L.input).numel());
  return need;
}

size_t part_need(const PpsModel& m, const Shapes& shapes) {
  size_t need = 0;
  for (const auto& L : m.layers)
    if (L.op == Op::Conv && L.splitk > 1)
      need = std::max(need, (size_t)L.splitk * (size_t)shapes.at(L.output).numel());
  return need;
}

// tile counters for the one-launch split-K: an upper bound on the output
// tiles of any split conv (the smallest FIX tile is 96 x 128 / 192 x 64)
size_t cnt_need(const PpsModel& m, const Shapes& shapes) {
  size_t need = 0;
  for (const auto& L : m.layers)
    if (L.op == Op::Conv && L.splitk > 1) {
      const Shape& y = shapes.at(L.output);
      const size_t M = (size_t)(y.d[0] * y.d[1] * y.d[2]);
      need = std::max(need, ((M + 95) / 96) * (((size_t)L.cout + 63) / 64));
    }
  return need;
}

// One buffer the tuning table sizes, grown to `need` elements of `esz` bytes
// (never under a reserved batch's captured graph)
void grow(Workspace& w, Buf& buf, size_t& have, size_t need, size_t esz, bool allow_alloc,
          hipStream_t st, const std::string& pinned_msg, const char* capture_msg) {
  if (need <= have) return;
  PPS_MCHECK(!w.pinned, pinned_msg);
  PPS_MCHECK(allow_alloc && !capturing(st), capture_msg);
  buf = std::make_shared<DevBuf>(need * esz);
  have = need;
}

void grow_tuned_buffers(const PpsModel& m, Workspace& w, hipStream_t st, bool allow_alloc) {
  const std::string batch = "the buffers of batch " + std::to_string(w.N);
  const std::string pinned_msg =
      batch + " are pinned by pps_model_reserve (a captured graph may hold them) and the tuning "
              "table now needs larger split-K ";
  grow(w, w.part, w.part_floats, part_need(m, w.shapes), sizeof(float), allow_alloc, st,
       pinned_msg + "partials: pps_model_release, reserve again, recapture",
       "split-K partials grew after pps_model_reserve: reserve again outside capture");
  grow(w, w.h2p, w.h2p_elems, h2p_need(m, w.shapes), 2 * sizeof(uint16_t), allow_alloc, st,
       batch + " are pinned by pps_model_reserve and the tuning table now needs "
               "larger f16x2 activation planes: pps_model_release, reserve "
               "again, recapture",
       "f16x2 activation planes grew after pps_model_reserve: reserve again outside "
       "capture");
  const size_t had = w.cnt_ints;
  grow(w, w.cnt, w.cnt_ints, cnt_need(m, w.shapes), sizeof(int), allow_alloc, st,
       pinned_msg + "counters: pps_model_release, reserve again, recapture",
       "split-K counters grew after pps_model_reserve: reserve again outside capture");
  if (w.cnt_ints > had)  // the counters are zero between launches
    hip_check(hipMemsetAsync(w.cnt->p, 0, w.cnt->bytes, st), "hipMemsetAsync");
}
}  // namespace

bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
  return cs != hipStreamCaptureStatusNone;
}

Workspace& workspace(const PpsModel& m, int N, hipStream_t st, bool allow_alloc) {
  auto it = m.ws.find(N);
  if (it != m.ws.end()) {
    grow_tuned_buffers(m, it->second, st, allow_alloc);
    return it->second;
  }
  PPS_MCHECK(allow_alloc && !capturing(st),
             "no workspace for batch " + std::to_string(N) +
                 ": call pps_model_reserve before capturing pps_forward");
  Workspace w;
  w.N = N;
  w.shapes = infer_shapes(m, N);
  bool need_conv_out = false;
  for (const auto& L : m.layers)
    if (L.op == Op::ConvPps && pps_tiles(L, w.shapes.at(L.conv_output)).empty())
      need_conv_out = true;
  for (const auto& kv : w.shapes) {
    if (kv.first == "data") continue;
    bool fused_away = false;
    for (const auto& L : m.layers)
      if (L.op == Op::ConvPps && L.conv_output == kv.first && !need_conv_out) fused_away = true;
    if (fused_away) continue;
    const size_t esz = m.plane_capable.count(kv.first) ? 6 : 4;
    w.bufs[kv.first] = std::make_shared<DevBuf>((size_t)kv.second.numel() * esz);
  }
  grow_tuned_buffers(m, w, st, allow_alloc);
  w.amax = std::make_shared<DevBuf>(m.slot.size() * PPS_AMAX_SLOT_FLOATS * sizeof(float));
  hip_check(hipMemsetAsync(w.amax->p, 0, w.amax->bytes, st), "hipMemsetAsync");
  return m.ws.emplace(N, std::move(w)).first->second;
}

float* nhwc4_buffer(const PpsModel& m, Workspace& w, hipStream_t st) {
  if (!w.nhwc4) {
    PPS_MCHECK(!capturing(st), "input staging buffer: call pps_model_reserve before capture");
    w.nhwc4 = std::make_shared<DevBuf>((size_t)w.N * m.cfg.height * m.cfg.width * 4 * sizeof(float));
  }
  return w.nhwc4->as<float>();
}

// ---- one layer ----------------------------------------------------------------
namespace {

struct Act {  // an activation operand: f32 NHWC or bf16x3 planes
  const float* f = nullptr;
  const uint16_t* pl = nullptr;
  int64_t plane = 0;
  Shape s;
};

// A layer's tile word as one launch uses it, decoded once: the f16x2 flags,
// the consumer that wants this layer's output as f16x2 planes, the split-K
// form, and `tile` = the id plus the flags the op-level entry still honours
struct TileUse {
  int tile = 0;
  bool h2 = false, h2p = false, h2e = false;  // PPS_TILE_H2 arithmetic; its input as planes
  bool seam = false;                          // PPS_TILE_SEAM: the launch also runs seam_next
  const Layer* h2e_c = nullptr;  // the PPS_TILE_H2E reader of this layer's output
  bool fused_sk = false;         // split conv in one launch (a FIX tile)
  bool wtiled = false;           // PPS_TILE_B_TILED: the chunk-tiled weight copy
};

TileUse decode_tile(const PpsModel& m, const Layer& L, int tile, int sk) {
  TileUse t;
  // PPS_TILE_H2: the f16x2 arithmetic on the base tile (weights always the
  // chunk-tiled f16x2 split; COL_ORDER kept)
  t.h2 = tile_h2(tile);
  t.h2p = tile_h2p(tile);
  t.h2e = tile_h2e(tile);
  if (t.h2) {
    PPS_MCHECK(L.w2 && !L.planes_in && !L.planes_out && sk == 1,
               "layer '" + L.name + "': PPS_TILE_H2 needs the f16x2 weights, f32 activations "
               "at both ends and no split-K");
    tile &= ~(kTileFlagMask & ~PPS_TILE_COL_ORDER);
  }
  // PPS_TILE_H2E on the layer that reads this one's output: write it as
  // f16x2 planes on the output bound's scale (the bound into the slot)
  const Layer* h2e_c = nullptr;
  if (L.op == Op::Conv && L.h2o_bw > 0.f)
    for (const Layer& C : m.layers)
      if (C.input == L.output && tile_h2e(C.tile)) h2e_c = &C;
  if (h2e_c) {
    PPS_MCHECK(h2e_producer(m, *h2e_c) == (int)(&L - &m.layers[0]) && !L.planes_in &&
                   !L.planes_out && sk == 1 && !(tile & PPS_TILE_SEAM),
               "layer '" + h2e_c->name + "': PPS_TILE_H2E needs its producer '" + L.name +
                   "' to be a conv + BN + ReLU read by it alone, f32 input, no split-K");
    tile &= ~(PPS_TILE_B_TILED | PPS_TILE_SEAM);
  }
  t.h2e_c = h2e_c;
  // split convs run in one launch on the FIX tiles (same bits as the
  // two-pass split-K), else raw partials + the summing pass (plain weights)
  t.fused_sk = sk > 1 && L.op == Op::Conv && fix_tile(tile) && L.relu &&
               !(L.planes_out && !L.residual.empty());
  if (sk > 1 && !t.fused_sk) tile &= ~PPS_TILE_B_TILED;
  // PPS_TILE_B_TILED in the tile: the chunk-tiled weight copy (plain convs)
  t.wtiled = tile > 0 && (tile & PPS_TILE_B_TILED) && L.wt;
  if (L.op == Op::Heads) tile &= ~PPS_TILE_COL_ORDER;
  if (!t.wtiled) tile &= ~PPS_TILE_B_TILED;
  t.seam = L.op == Op::Conv && tile_seam(tile);
  t.tile = tile;
  return t;
}

// `want` if it is one of `ok`, else the first of them
int tile_among(const std::vector<int>& ok, int want) {
  return std::find(ok.begin(), ok.end(), want) != ok.end() ? want : ok[0];
}

// One launch of layer L: what it works on, and one function per op
struct LayerRun {
  const PpsModel& m;
  const Layer& L;
  Workspace& w;
  const float* x;  // the forward's input ("data")
  float* feat;     // the forward's output, written by the last layer
  bool last;
  int sk;
  hipStream_t st;
  TileUse t;

  Act act(const std::string& name, bool planes) const {
    Act a;
    a.s = w.shapes.at(name);
    if (name == "data") { a.f = x; return a; }
    void* p = w.bufs.at(name)->p;
    if (planes) { a.pl = static_cast<const uint16_t*>(p); a.plane = a.s.numel(); }
    else a.f = static_cast<const float*>(p);
    return a;
  }
  float* fbuf(const std::string& name) const { return pps::fbuf(w, name); }
  float* slotp(const std::string& tensor) const { return slot_ptr(m, w, tensor); }
  // the weights in the model's arithmetic (bf16x3 planes, plain or
  // chunk-tiled; else f32) and the folded BN
  const uint16_t* w3() const {
    return m.x3 && L.w ? (t.wtiled ? L.wt->as<uint16_t>() : L.w->as<uint16_t>()) : nullptr;
  }
  const float* wf() const { return !m.x3 && L.w ? L.w->as<float>() : nullptr; }
  const float* sc() const { return L.scale ? L.scale->as<float>() : nullptr; }
  const float* sh() const { return L.shift ? L.shift->as<float>() : nullptr; }

  // The input of an f16x2 layer as f16x2 planes: the ones its producer wrote
  // (PPS_TILE_H2E), else split once here (PPS_TILE_H2P, same bits)
  const uint16_t* h2_planes(const Act& a, int64_t* plane) const {
    const int64_t n = a.s.numel();
    *plane = n;
    if (t.h2e) return w.bufs.at(L.input)->as<uint16_t>();
    PPS_MCHECK(w.h2p && (size_t)n <= w.h2p_elems, "layer '" + L.name +
                                                     "': no f16x2 activation-plane workspace");
    uint16_t* pl = w.h2p->as<uint16_t>();
    rc_check(split_act_h2(a.f, n, slotp(L.input), pl, n, st));
    return pl;
  }

  // pps_conv1x1_seam_x3 with the two outputs' maxima reported
  void seam() const {
    PPS_MCHECK(seam_ok(m, L), "layer '" + L.name + "': PPS_TILE_SEAM needs f32 activations "
                              "at both ends and no split-K");
    const Layer& X = m.layers[L.seam_next];
    const Act a = act(L.input, false);
    const int64_t M = a.s.d[0] * a.s.d[1] * a.s.d[2];
    SeamParams sp{a.f, fbuf(L.residual), L.w->as<uint16_t>(), sc(), sh(), fbuf(L.output),
                  X.w->as<uint16_t>(), X.scale->as<float>(), X.shift->as<float>(),
                  fbuf(X.output), (int)M};
    sp.amax_t = slotp(L.output);
    sp.amax_y = slotp(X.output);
    rc_check(launch_seam_x3(sp, L.cin_eff, L.cout, X.cout, st));
  }

  // the op-level entry points' implementation (same arguments as
  // pps_conv2d_bn_act_x3p[_splitk[_fused]] / _x3 / _h2), reporting max |y|
  void conv() const {
    const Act a = act(L.input, L.planes_in);
    const Shape ys = w.shapes.at(L.output);
    float* amo = slotp(L.output);
    // f16x2 planes out (the consumer's PPS_TILE_H2E): the output buffer
    // holds the two planes, the bound goes to the output's slot
    uint16_t* yh2 = t.h2e_c ? w.bufs.at(L.output)->as<uint16_t>() : nullptr;
    if (t.h2e_c)
      PPS_MCHECK(amo && slotp(L.input), "layer '" + L.name + "': f16x2 planes out needs the "
                                        "input's and the output's activation slots");
    ConvArgs c;
    c.x = a.f; c.N = (int)a.s.d[0]; c.H = (int)a.s.d[1]; c.W = (int)a.s.d[2];
    c.Cin = L.cin_eff; c.ldx = (int)a.s.d[3];
    c.w = m.x3 ? (const void*)w3() : (const void*)wf(); c.x3 = m.x3;
    c.Cout = L.cout; c.Kpad = L.kpad; c.KH = c.KW = L.k;
    c.stride = L.stride; c.pad = L.pad; c.dil = L.dil;
    c.scale = sc(); c.shift = sh();
    c.residual = L.residual.empty() ? nullptr : fbuf(L.residual); c.relu = L.relu;
    c.y = fbuf(L.output); c.Ho = (int)ys.d[1]; c.Wo = (int)ys.d[2]; c.ldy = L.cout;
    c.tile = t.tile; c.stream = st;
    if (m.x3) c.amax_out = amo;  // (the f32 path is pps_conv2d_bn_act: no max reported)
    if (yh2) {  // f16x2 planes out, from either arithmetic
      c.y = nullptr; c.y_h2 = yh2; c.y_h2_plane = ys.numel();
      c.h2o_in = slotp(L.input); c.h2o_bw = L.h2o_bw; c.h2o_bb = L.h2o_bb;
    }
    if (t.h2) {
      c.w = L.w2->as<uint16_t>(); c.w_rs = L.wrs->as<float>(); c.amax_in = slotp(L.input);
      if (t.h2p || t.h2e) {
        c.x_pl = h2_planes(a, &c.x_plane);
        if (c.x_pl) c.x = nullptr;
      }
    } else if (m.x3 && !yh2 && (L.planes_in || L.planes_out || sk > 1)) {
      c.tile = tile_lands_pipelined(t.tile) ? t.tile : 0;
      c.x_pl = a.pl; c.x_plane = a.plane;
      if (L.planes_out) {
        c.y = nullptr; c.y_pl = w.bufs.at(L.output)->as<uint16_t>(); c.y_plane = ys.numel();
      }
      c.splitk = sk;
      if (sk > 1) c.part = w.part->as<float>();
      if (t.fused_sk) { c.fix_cnt = w.cnt->as<int>(); c.n_cnt = (int64_t)w.cnt_ints; }
    }
    rc_check(conv_impl(c));
  }

  void conv_dual() const {
    const Act a = act(L.input, false), b = act(L.input2, false);
    const Shape ys = w.shapes.at(L.output);
    const int C2 = (int)b.s.d[3];
    DualArgs c;
    c.x = a.f; c.N = (int)a.s.d[0]; c.H = (int)a.s.d[1]; c.W = (int)a.s.d[2];
    c.Cin = L.cin_eff; c.ldx = (int)a.s.d[3];
    c.KH = c.KW = L.k; c.stride = L.stride; c.pad = L.pad;
    c.x2 = b.f; c.H2 = (int)b.s.d[1]; c.W2 = (int)b.s.d[2]; c.Cin2 = c.ldx2 = C2;
    c.stride2 = L.stride2;
    c.w = m.x3 ? (const void*)w3() : (const void*)wf(); c.x3 = m.x3;
    c.Cout = L.cout; c.Kpad = L.kpad; c.Kpad2 = C2; c.shift = sh(); c.relu = L.relu;
    c.y = fbuf(L.output); c.Ho = (int)ys.d[1]; c.Wo = (int)ys.d[2]; c.ldy = L.cout;
    c.tile = t.tile; c.stream = st;
    if (m.x3) c.amax_out = slotp(L.output);  // (the f32 path is pps_conv2d_dual_bn_act)
    if (m.x3 && t.h2) {
      c.w = L.w2->as<uint16_t>(); c.w_rs = L.wrs->as<float>();
      c.amax_in = slotp(L.input); c.amax_in2 = slotp(L.input2);
    }
    rc_check(dual_impl(c));
  }

  void maxpool() const {
    const Act a = act(L.input, false);
    const Shape ys = w.shapes.at(L.output);
    PPS_MCHECK(a.s.d[3] % 4 == 0, "max pooling needs C % 4 == 0");
    rc_check(maxpool2d(a.f, (int)a.s.d[0], (int)a.s.d[1], (int)a.s.d[2], (int)a.s.d[3], L.k,
                       L.stride, L.pad, fbuf(L.output), (int)ys.d[1], (int)ys.d[2], st,
                       slotp(L.output)));
  }

  // pps_stem_conv_pool_x3 / _h2 (shapes checked when the stem was fused), max |y| reported
  void stem() const {
    const Act a = act(L.input, false);
    const Shape ys = w.shapes.at(L.output);
    const int Hin = (int)a.s.d[1];
    if (t.h2) {  // pps_stem_conv_pool_h2: the input's max from its slot
      PPS_MCHECK(slotp(L.input), "layer '" + L.name + "': the f16x2 stem needs its input's "
                                 "activation-max slot");
      rc_check(stem_conv_pool_h2(a.f, (int)a.s.d[0], Hin, L.w2->as<uint16_t>(),
                                 L.wrs->as<float>(), sc(), sh(), fbuf(L.output),
                                 (Hin + 2 * 3 - 7) / 2 + 1, (int)ys.d[1], st, slotp(L.output),
                                 slotp(L.input)));
      return;
    }
    rc_check(stem_conv_pool_x3(a.f, (int)a.s.d[0], Hin, w3(), sc(), sh(), fbuf(L.output),
                               (Hin + 2 * 3 - 7) / 2 + 1, (int)ys.d[1], st, slotp(L.output)));
  }

  void pps() const {
    const Act a = act(L.input, false);
    rc_check(pps_part_power_set(a.f, (int)a.s.d[0], (int)a.s.d[1], (int)a.s.d[2],
                                (int)a.s.d[3], L.split.data(), (int)L.split.size(), L.max_ave,
                                fbuf(L.output), st));
  }

  void conv_pps() const {
    const Act a = act(L.input, L.planes_in);
    const Shape cs = w.shapes.at(L.conv_output);
    const std::vector<int> ok = pps_tiles(L, cs);
    ConvArgs c;
    c.x = a.f; c.x_pl = a.pl; c.x_plane = a.plane;
    c.N = (int)a.s.d[0]; c.H = (int)a.s.d[1]; c.W = (int)a.s.d[2]; c.ldx = (int)a.s.d[3];
    c.Cin = L.cin_eff; c.w = w3(); c.x3 = 1; c.Cout = L.cout; c.Kpad = L.kpad; c.KH = c.KW = L.k;
    c.stride = L.stride; c.pad = L.pad; c.dil = L.dil;
    c.scale = sc(); c.shift = sh(); c.residual = fbuf(L.residual);
    c.Ho = (int)cs.d[1]; c.Wo = (int)cs.d[2];
    c.splits = L.split.data(); c.S = (int)L.split.size(); c.max_ave = L.max_ave;
    c.pps_out = fbuf(L.output); c.stream = st;
    if (t.h2) {  // f16x2: the 192-row tiles on 16x16x32 blocks
      std::vector<int> ok16;
      for (int id : ok)
        if (id >= GEMM_TILE_P16_FIRST) ok16.push_back(id);
      PPS_MCHECK(!ok16.empty(), "layer '" + L.name + "': no f16x2 tile holds one image");
      c.tile = tile_among(ok16, tile_base(t.tile)) | (t.tile & PPS_TILE_COL_ORDER);
      if (t.h2p || t.h2e) {
        c.x_pl = h2_planes(a, &c.x_plane);
        c.x = nullptr;
      }
      c.w = L.w2->as<uint16_t>(); c.w_rs = L.wrs->as<float>(); c.amax_in = slotp(L.input);
    } else if (!ok.empty()) {
      c.tile = tile_among(ok, tile_base(t.tile)) | (t.tile & PPS_TILE_COL_ORDER);
      if (t.wtiled) c.tile |= PPS_TILE_B_TILED;
    } else {  // no tile holds exactly one image: conv, then the pooling kernel
      c.relu = 1; c.y = fbuf(L.conv_output); c.ldy = L.cout;
      c.tile = tile_lands_pipelined(t.tile) ? t.tile | (t.wtiled ? PPS_TILE_B_TILED : 0) : 0;
      rc_check(conv_impl(c));
      rc_check(pps_part_power_set(c.y, c.N, c.Ho, c.Wo, L.cout, L.split.data(), c.S, L.max_ave,
                                  fbuf(L.output), st));
      return;
    }
    rc_check(conv_pps_impl(c));
  }

  void heads() const {
    const int N = w.N;
    float* part = fbuf(L.output + "_partials");
    const float* xin = fbuf(L.input);
    if (m.x3)
      rc_check(pps_gemm_splitk_batched_x3(xin, N, L.dim, w3(), L.dim_inner, L.nsub, kHeadSplitK,
                                          part, t.tile, st));
    else
      rc_check(pps_gemm_splitk_batched(xin, N, L.dim, wf(), L.dim_inner, L.nsub, kHeadSplitK,
                                       part, t.tile, st));
    float* y = last ? feat : fbuf(L.output);
    rc_check(pps_splitk_bn_act_normalize(part, kHeadSplitK, N, L.nsub * L.dim_inner, sc(), sh(), 1,
                                         L.normalize ? 1 : 0, y, st));
  }

  void normalize() const {
    const Act a = act(L.input, false);
    rc_check(pps_l2_normalize(a.f, a.s.d[0], (int)a.s.d[1], last ? feat : fbuf(L.output), st));
  }
};

}  // namespace

void run_layer(const PpsModel& m, const Layer& L, Workspace& w, const float* x, float* feat,
               bool last, int tile, int sk, hipStream_t st) {
  const LayerRun r{m, L, w, x, feat, last, sk, st, decode_tile(m, L, tile, sk)};
  if (r.t.seam) return r.seam();
  switch (L.op) {
    case Op::Conv: return r.conv();
    case Op::ConvDual: return r.conv_dual();
    case Op::MaxPool: return r.maxpool();
    case Op::StemPool: return r.stem();
    case Op::Pps: return r.pps();
    case Op::ConvPps: return r.conv_pps();
    case Op::Heads: return r.heads();
    case Op::Normalize: return r.normalize();
  }
}

// ---- one forward ------------------------------------------------------------------
namespace {

// The tensors whose maxima this forward needs: all of them (autotune,
// PPS_AMAX_ALL), else the inputs of the f16x2 layers
void mark_amax_needs(const PpsModel& m, Workspace& w) {
  const bool all = m.amax_all || getenv_flag_on("PPS_AMAX_ALL");
  w.amax_need.assign(m.slot.size(), all ? 1 : 0);
  if (all) return;
  for (const Layer& L : m.layers)
    if (tile_h2(L.tile)) {
      for (const std::string* t : {&L.input, &L.input2})
        if (!t->empty() && m.slot.count(*t)) w.amax_need[m.slot.at(*t)] = 1;
      // PPS_TILE_H2E: the producer's bound reads its own input's max
      const int pi = tile_h2e(L.tile) ? h2e_producer(m, L) : -1;
      if (pi >= 0 && m.slot.count(m.layers[pi].input))
        w.amax_need[m.slot.at(m.layers[pi].input)] = 1;
    }
}

void zero_slot(float* slot, hipStream_t st) {
  hip_check(hipMemsetAsync(slot, 0, PPS_AMAX_SLOT_FLOATS * sizeof(float), st), "hipMemsetAsync");
}

// A whole forward: every producer reports its output's max afresh, and the
// input's max is measured when an f16x2 layer (the stem) reads it
void prepare_amax_forward(const PpsModel& m, Workspace& w, const float* x,
                          const std::function<void(float*)>* pre, hipStream_t st) {
  hip_check(hipMemsetAsync(w.amax->p, 0, w.amax->bytes, st), "hipMemsetAsync");
  float* dslot = slot_ptr(m, w, "data");
  if (pre) (*pre)(dslot);  // the producer of x reports its max
  else if (dslot) rc_check(amax_of(x, w.shapes.at("data").numel(), dslot, st));
}

// A layer range: the f32 tensors it reads but does not produce are measured
// afresh (their producers ran in an earlier call)
void prepare_amax_range(const PpsModel& m, Workspace& w, const float* x, int first, int last,
                        hipStream_t st) {
  std::set<std::string> made, done;
  for (int i = first; i < last; ++i) {
    const Layer& L = m.layers[i];
    for (const std::string* t : {&L.input, &L.input2}) {
      float* slot = t->empty() || made.count(*t) || done.count(*t) ? nullptr : slot_ptr(m, w, *t);
      if (!slot) continue;
      bool planes = false;
      for (const auto& P : m.layers)
        if (P.output == *t && P.planes_out) planes = true;
      // an f16x2-planes edge (PPS_TILE_H2E): its slot keeps the producer's bound
      if (L.input == *t && tile_h2e(L.tile)) planes = true;
      const float* src = *t == "data" ? x : (w.bufs.count(*t) ? fbuf(w, *t) : nullptr);
      if (planes || !src) continue;
      zero_slot(slot, st);
      rc_check(amax_of(src, w.shapes.at(*t).numel(), slot, st));
      done.insert(*t);
    }
    made.insert(L.output);
    if (!L.conv_output.empty()) made.insert(L.conv_output);
    if (L.seam_next >= 0 && tile_seam(L.tile)) made.insert(m.layers[L.seam_next].output);
  }
  // and the tensors it produces start from zero, as in a whole forward:
  // their producers combine into the slot with atomicMax, so a larger max
  // left by an earlier call would otherwise set a stale scale
  for (const std::string& t : made)
    if (m.slot.count(t)) zero_slot(slot_at(w, m.slot.at(t)), st);
}

}  // namespace

// pre (whole forwards only): writes x before the layers run -- the
// preprocessing of pps_forward_bgr -- and reports max|x| into the slot it is
// given (null when no f16x2 layer reads the input)
void forward_range(const PpsModel& m, const float* x, int N, float* feat, int first, int last,
                   hipStream_t st, bool keep_amax, const std::function<void(float*)>* pre) {
  Workspace& w = workspace(m, N, st, true);
  mark_amax_needs(m, w);
  if (first == 0 && !keep_amax) prepare_amax_forward(m, w, x, pre, st);
  else if (!keep_amax) prepare_amax_range(m, w, x, first, last, st);
  for (int i = first; i < last; ++i) {
    const Layer& L = m.layers[i];
    // computed by the previous layer's seam launch (when that ran here too)
    if (i > first && tile_seam(m.layers[i - 1].tile) && m.layers[i - 1].seam_next == i) continue;
    // (the range's last layer runs alone: its seam partner is outside it)
    run_layer(m, L, w, x, feat, i + 1 == (int)m.layers.size(),
              i + 1 == last ? L.tile & ~PPS_TILE_SEAM : L.tile, L.splitk, st);
  }
}

}  // namespace pps
