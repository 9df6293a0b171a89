// pps_model_create's work: the plan (model_plan.hpp) compiled into the fused
// launches of the op-level ABI -- test-mode BN folded into conv epilogues,
// projection shortcuts K-concatenated into their branch2c GEMM, stem conv +
// pool fused, part pooling in the last conv's epilogue, 31 heads as one
// split-K batched GEMM + one BN/ReLU/Normalize pass -- with the weights packed,
// uploaded and split (bf16x3, chunk-tiled, f16x2) once.
#include <algorithm>
#include <cmath>

#include "model_internal.hpp"

namespace pps {
namespace {

constexpr double kBnEps = 1e-5;  // Caffe2 SpatialBN default epsilon (pytorch v1.0.1)

// ---- weights (host) -------------------------------------------------------------
struct Blob {
  const float* data;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};
using Blobs = std::map<std::string, Blob>;

// model.py fold_bn: test-mode SpatialBN y = (x - rm) * s / sqrt(riv + eps) + b as
// y = x * scale + shift, in float64 then rounded to float32 (conv bias in shift)
void fold_bn(const Blobs& blobs, const std::string& bn, const Blob* bias,
             std::vector<float>& scale, std::vector<float>& shift) {
  const Blob& s = blobs.at(bn + "_s");
  const Blob& b = blobs.at(bn + "_b");
  const Blob& rm = blobs.at(bn + "_rm");
  const Blob& riv = blobs.at(bn + "_riv");
  const int64_t n = s.numel();
  scale.resize(n);
  shift.resize(n);
  for (int64_t i = 0; i < n; ++i) {
    const double sc = (double)s.data[i] / std::sqrt((double)riv.data[i] + kBnEps);
    const double cb = bias ? (double)bias->data[i] : 0.0;
    scale[i] = (float)sc;
    shift[i] = (float)((cb - (double)rm.data[i]) * sc + (double)b.data[i]);
  }
}

// [Cout][Cin][KH][KW] -> [Cout][Kpad], K ordered (kh, kw, cin), Kpad % 16 == 0
std::vector<float> pack_conv(const Blob& w, int cin_pad, int& kpad) {
  const int64_t co = w.shape[0], ci = w.shape[1], kh = w.shape[2], kw = w.shape[3];
  const int64_t cp = std::max<int64_t>(cin_pad, ci);
  const int64_t k = kh * kw * cp;
  kpad = (int)((k + 15) / 16 * 16);
  std::vector<float> out((size_t)co * kpad, 0.f);
  for (int64_t o = 0; o < co; ++o)
    for (int64_t y = 0; y < kh; ++y)
      for (int64_t x = 0; x < kw; ++x)
        for (int64_t c = 0; c < ci; ++c)
          out[o * kpad + (y * kw + x) * cp + c] = w.data[((o * ci + c) * kh + y) * kw + x];
  return out;
}

// conv1 [64][3][7][7] -> the fused stem's [64][pps_stem_k()] layout: K index
// (kh * 3 + c) * 8 + kw, kw = 7 and the tail zero (stem.hip, model.py pack_stem_weight)
std::vector<float> pack_stem(const Blob& w) {
  const int K = pps_stem_k();
  std::vector<float> out((size_t)64 * K, 0.f);
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int c = 0; c < 3; ++c)
        for (int kw = 0; kw < 7; ++kw)
          out[(size_t)o * K + (kh * 3 + c) * 8 + kw] = w.data[((o * 3 + c) * 7 + kh) * 7 + kw];
  return out;
}

// ---- weights (device) -----------------------------------------------------------
Buf upload(const std::vector<float>& h, hipStream_t st) {
  auto b = std::make_shared<DevBuf>(h.size() * sizeof(float));
  hip_check(hipMemcpyAsync(b->p, h.data(), b->bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");  // h may die after return
  return b;
}

// f32 weights -> bf16x3 planes [nbatch][3][n] (pps_split_bf16x3)
Buf split3(const Buf& w, int64_t n, int nbatch, hipStream_t st) {
  auto b = std::make_shared<DevBuf>((size_t)n * nbatch * 3 * sizeof(uint16_t));
  rc_check(pps_split_bf16x3(w->as<float>(), n, nbatch, b->as<uint16_t>(), st));
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  return b;
}

// f32 weights [rows][K] -> the f16x2 split (pps_split_f16x2_sqnorm_tiled):
// chunk-tiled planes [2][rows16 / 16][K / 32][16][32] and per-row scales
void split_h2w(const Buf& w, int rows, int64_t K, Buf& w2, Buf& wrs, hipStream_t st) {
  const int64_t r16 = (rows + 15) / 16 * 16;
  w2 = std::make_shared<DevBuf>((size_t)2 * r16 * K * sizeof(uint16_t));
  wrs = std::make_shared<DevBuf>((size_t)rows * sizeof(float));
  DevBuf sq((size_t)rows * sizeof(float));
  rc_check(pps_split_f16x2_sqnorm_tiled(w->as<float>(), rows, (int)K, K, w2->as<uint16_t>(),
                                        wrs->as<float>(), sq.as<float>(), st));
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
}

// ---- compile steps, in the order compile() runs them ----------------------------
const Blob* find_blob(const Blobs& blobs, const std::string& n) {
  auto it = blobs.find(n);
  return it == blobs.end() ? nullptr : &it->second;
}

// A block's branch2c with its projection shortcut S: one GEMM over the two
// inputs (K concat), both BN scales folded into the weights
void lower_dual(const PlanLayer& P, const PlanLayer& S, const Blobs& blobs, Layer& L,
                hipStream_t st) {
  int kpad1 = 0, kpad2 = 0;
  std::vector<float> w1 = pack_conv(blobs.at(P.name + "_w"), 0, kpad1);
  std::vector<float> w2 = pack_conv(blobs.at(S.name + "_w"), 0, kpad2);
  PPS_MCHECK(kpad1 == P.cin && kpad2 == S.cin, "fused shortcut needs Cin % 16 == 0");
  std::vector<float> s1, h1, s2, h2;
  fold_bn(blobs, P.bn, nullptr, s1, h1);
  fold_bn(blobs, S.bn, nullptr, s2, h2);
  const int K = kpad1 + kpad2;
  std::vector<float> w((size_t)P.cout * K), sh(P.cout);
  for (int o = 0; o < P.cout; ++o) {
    for (int k = 0; k < kpad1; ++k) w[(size_t)o * K + k] = w1[(size_t)o * kpad1 + k] * s1[o];
    for (int k = 0; k < kpad2; ++k)
      w[(size_t)o * K + kpad1 + k] = w2[(size_t)o * kpad2 + k] * s2[o];
    sh[o] = h1[o] + h2[o];
  }
  L.op = Op::ConvDual;
  L.w = upload(w, st); L.shift = upload(sh, st);
  L.kpad = kpad1; L.cin_eff = P.cin;
  L.input2 = S.input; L.stride2 = S.stride; L.residual.clear(); L.shortcut_cin = S.cin;
}

void lower_heads(const PlanLayer& P, const Blobs& blobs, Layer& L, hipStream_t st) {
  const int nb = (int)P.prefixes.size();
  std::vector<float> w((size_t)nb * P.dim_inner * P.dim), sc, sh, s1, h1;
  for (int b = 0; b < nb; ++b) {
    const Blob& wb = blobs.at(P.prefixes[b] + "_conv_w");
    std::copy(wb.data, wb.data + (size_t)P.dim_inner * P.dim,
              w.begin() + (size_t)b * P.dim_inner * P.dim);
    fold_bn(blobs, P.prefixes[b] + "_bn", find_blob(blobs, P.prefixes[b] + "_conv_b"), s1, h1);
    sc.insert(sc.end(), s1.begin(), s1.end());
    sh.insert(sh.end(), h1.begin(), h1.end());
  }
  L.w = upload(w, st); L.scale = upload(sc, st); L.shift = upload(sh, st);
  L.dim = P.dim; L.dim_inner = P.dim_inner; L.nsub = nb;
}

// plan layers -> launches with f32 weights: BN folded, projection shortcuts
// inside their block's branch2c, Normalize inside the heads' summing pass
void lower_plan(PpsModel& m, const Blobs& blobs, hipStream_t st) {
  const Plan& plan = m.plan;
  std::map<std::string, const PlanLayer*> shortcut_of;
  for (const auto& L : plan.layers)
    if (L.op == Op::Conv && L.name.size() > 8 &&
        L.name.compare(L.name.size() - 8, 8, "_branch1") == 0 && L.k == 1)
      shortcut_of[L.output] = &L;
  for (const auto& P : plan.layers) {
    Layer L;
    L.op = P.op; L.name = P.name.empty() ? P.output : P.name;
    L.input = P.input; L.output = P.output; L.residual = P.residual;
    L.cin = P.cin; L.cout = P.cout; L.k = P.k; L.stride = P.stride; L.pad = P.pad; L.dil = P.dil;
    L.relu = P.relu;
    if (P.op == Op::Conv && shortcut_of.count(P.output)) continue;  // inside its branch2c
    if (P.op == Op::Conv && shortcut_of.count(P.residual)) {
      lower_dual(P, *shortcut_of.at(P.residual), blobs, L, st);
    } else if (P.op == Op::Conv) {
      const int cin_pad = P.cin == 3 ? 4 : 0;
      std::vector<float> w = pack_conv(blobs.at(P.name + "_w"), cin_pad, L.kpad);
      std::vector<float> sc, sh;
      fold_bn(blobs, P.bn, find_blob(blobs, P.name + "_b"), sc, sh);
      L.w = upload(w, st); L.scale = upload(sc, st); L.shift = upload(sh, st);
      L.cin_eff = cin_pad ? cin_pad : P.cin;
    } else if (P.op == Op::Heads) {
      lower_heads(P, blobs, L, st);
    } else if (P.op == Op::Pps) {
      L.split = P.split; L.max_ave = P.max_ave; L.nsub = (int)P.prefixes.size();
    } else if (P.op == Op::Normalize && !m.layers.empty() && m.layers.back().op == Op::Heads) {
      // heads as split-K partials + one reduce/BN/ReLU/Normalize pass
      m.layers.back().normalize = true;
      m.layers.back().output = P.output;
      m.layers.back().name = P.output;
      continue;
    }
    m.layers.push_back(L);
  }
}

// x3: every GEMM's weights as bf16x3 planes, with the chunk-tiled copy and the
// f16x2 split where a layer can use them
void split_weights(PpsModel& m, hipStream_t st) {
  for (auto& L : m.layers) {
    // the f16x2 split beside the bf16x3 one where an f16x2 tile can run
    // the layer (PPS_TILE_H2: Cin % 32 == 0, no K padding)
    if (is_conv(L) && h2_weights_capable(L) && (L.op == Op::Conv || L.shortcut_cin % 32 == 0))
      split_h2w(L.w, L.cout, layer_k(L), L.w2, L.wrs, st);
    // a conv + BN + ReLU that may write f16x2 planes for its consumer
    // (PPS_TILE_H2E): the bound constants, from the f32 weights
    if (L.op == Op::Conv && L.relu && L.residual.empty() && h2_weights_capable(L) && L.scale &&
        L.shift) {
      float b2[2];
      rc_check(pps_h2_out_bound(L.w->as<float>(), L.cout, L.kpad, L.scale->as<float>(),
                                L.shift->as<float>(), b2, st));
      L.h2o_bw = b2[0];
      L.h2o_bb = b2[1];
    }
    if (is_conv(L)) L.w = split3(L.w, (int64_t)L.cout * layer_k(L), 1, st);
    const int64_t kt = layer_k(L);
    if (is_conv(L) && kt % 32 == 0 && L.cin_eff % 32 == 0) {
      const int64_t c16 = (L.cout + 15) / 16 * 16;
      L.wt = std::make_shared<DevBuf>((size_t)3 * c16 * kt * sizeof(uint16_t));
      rc_check(pps_tile_planes(L.w->as<uint16_t>(), L.cout, (int)kt, kt, (int64_t)L.cout * kt,
                               L.wt->as<uint16_t>(), st));
      hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    } else if (L.op == Op::Heads) {
      L.w = split3(L.w, (int64_t)L.dim_inner * L.dim, L.nsub, st);
    }
  }
}

// conv1 + BN + ReLU + pool1 as one kernel (x3, input width 128 only)
bool fuse_stem(PpsModel& m, const Blobs& blobs, hipStream_t st) {
  for (size_t i = 0; i + 1 < m.layers.size(); ++i) {
    Layer& L = m.layers[i];
    const Layer& P = m.layers[i + 1];
    if (L.op == Op::Conv && L.input == "data" && L.k == 7 && L.stride == 2 && L.pad == 3 &&
        L.dil == 1 && L.cin == 3 && L.cout == 64 && L.relu && L.residual.empty() &&
        P.op == Op::MaxPool && P.input == L.output && P.k == 3 && P.stride == 2 && P.pad == 1 &&
        count_readers(m, L.output, false) == 1) {
      Layer F = L;
      F.op = Op::StemPool; F.output = P.output; F.conv_output = L.output;
      const Buf wf = upload(pack_stem(blobs.at(L.name + "_w")), st);
      F.w = split3(wf, 64LL * pps_stem_k(), 1, st);
      // and the f16x2 split (PPS_TILE_H2 on the stem): [2][64][K] f16 + 2^-s per channel
      F.w2 = std::make_shared<DevBuf>((size_t)2 * 64 * pps_stem_k() * sizeof(uint16_t));
      F.wrs = std::make_shared<DevBuf>((size_t)64 * sizeof(float));
      rc_check(stem_split_h2(wf->as<float>(), F.w2->as<uint16_t>(), F.wrs->as<float>(), st));
      hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
      m.layers[i] = F;
      m.layers.erase(m.layers.begin() + i + 1);
      return true;
    }
  }
  return false;
}

// the last conv (+ residual + ReLU) and the part pooling that is its only
// reader as one conv_pps layer (x3)
bool fuse_pps(PpsModel& m) {
  for (size_t i = 0; i + 1 < m.layers.size(); ++i) {
    Layer& L = m.layers[i];
    const Layer& P = m.layers[i + 1];
    if (L.op == Op::Conv && !L.residual.empty() && L.relu && P.op == Op::Pps &&
        P.input == L.output && L.output != m.plan.output && h2_weights_capable(L) &&
        count_readers(m, L.output, true) == 1) {
      Layer F = L;
      F.op = Op::ConvPps; F.output = P.output; F.conv_output = L.output;
      F.split = P.split; F.max_ave = P.max_ave; F.nsub = P.nsub;
      m.layers[i] = F;
      m.layers.erase(m.layers.begin() + i + 1);
      return true;
    }
  }
  return false;
}

// (producer, consumer) conv pairs whose tensor may travel as bf16x3 planes:
// one reader, a plain conv / conv_pps taking it as main input, Cin % 32 == 0
void find_plane_edges(PpsModel& m) {
  for (size_t i = 0; i < m.layers.size(); ++i) {
    const Layer& L = m.layers[i];
    if (L.op != Op::Conv || L.cin_eff % 4 || L.cout % 4 || L.output == m.plan.output) continue;
    int nread = 0, j = -1;
    bool main_input = false;
    for (size_t r = 0; r < m.layers.size(); ++r) {
      const Layer& R = m.layers[r];
      if (R.input == L.output) { ++nread; j = (int)r; main_input = true; }
      if (R.input2 == L.output) { ++nread; j = (int)r; main_input = false; }
      if (R.residual == L.output) { ++nread; j = (int)r; main_input = false; }
    }
    if (nread == 1 && main_input &&
        (m.layers[j].op == Op::Conv || m.layers[j].op == Op::ConvPps) &&
        m.layers[j].cin_eff % 32 == 0) {
      m.edges.emplace_back((int)i, j);
      m.plane_capable.insert(L.output);
    }
  }
  // heuristic before any autotune: the 3x3 consumers with Cin >= 256
  for (auto& e : m.edges) {
    const Layer& C = m.layers[e.second];
    const bool on = C.k > 1 && C.cin >= 256;
    m.layers[e.first].planes_out = m.layers[e.second].planes_in = on;
  }
}

// one activation-max slot per tensor (the input and every layer output):
// each producer reports max |y| there, the f16x2 layers scale by it
void assign_slots(PpsModel& m) {
  m.slot["data"] = 0;
  for (const auto& L : m.layers)
    for (const std::string* t : {&L.output, &L.conv_output})
      if (!t->empty() && !m.slot.count(*t)) {
        const int n = (int)m.slot.size();
        m.slot[*t] = n;
      }
}

// A branch2c -> next branch2a pair the seam kernel covers (structure only;
// seam_ok adds the table's conditions)
bool seam_pair(const PpsModel& m, size_t i) {
  if (!m.x3 || i + 1 >= m.layers.size()) return false;
  const Layer& L = m.layers[i];
  const Layer& X = m.layers[i + 1];
  auto plain1x1 = [](const Layer& A) {
    return A.op == Op::Conv && A.k == 1 && A.stride == 1 && A.pad == 0 && A.relu &&
           A.kpad == A.cin_eff && A.w;
  };
  return plain1x1(L) && plain1x1(X) && !L.residual.empty() && X.residual.empty() &&
         X.input == L.output && X.cin_eff == L.cout && seam_supported(L.cin_eff, L.cout, X.cout);
}

void compile(PpsModel& m, const Blobs& blobs, hipStream_t st) {
  lower_plan(m, blobs, st);
  if (m.x3) split_weights(m, st);
  if (m.fused_stem) m.fused_stem = fuse_stem(m, blobs, st);
  if (m.fused_pps) m.fused_pps = fuse_pps(m);
  if (m.act_planes) find_plane_edges(m);
  assign_slots(m);
}

// The caller's blob table by name, every parameter of the plan present (the
// head conv biases are optional) and of the plan's size
Blobs match_blobs(const Plan& plan, const PpsBlob* blobs, int nblobs) {
  Blobs bmap;
  for (int i = 0; i < nblobs; ++i) {
    const PpsBlob& b = blobs[i];
    PPS_MCHECK(b.name && (b.data || b.ndim == 0) && b.ndim >= 0 && b.ndim <= 4, "bad blob entry");
    Blob B{b.data, std::vector<int64_t>(b.shape, b.shape + b.ndim)};
    bmap[b.name] = B;
  }
  std::vector<std::string> missing;
  for (const auto& kv : plan.params) {
    auto it = bmap.find(kv.first);
    const bool optional = kv.first.size() > 7 &&
                          kv.first.compare(kv.first.size() - 7, 7, "_conv_b") == 0;
    if (it == bmap.end()) {
      if (!optional) missing.push_back(kv.first);
      continue;
    }
    int64_t want = 1;
    for (auto s : kv.second) want *= s;
    PPS_MCHECK(it->second.numel() == want,
               "blob " + kv.first + " has " + std::to_string(it->second.numel()) +
                   " elements, the net needs " + std::to_string(want));
    it->second.shape = kv.second;
  }
  PPS_MCHECK(missing.empty(), "weights missing " + std::to_string(missing.size()) +
                                  " blobs, e.g. " + (missing.empty() ? "" : missing[0]));
  return bmap;
}

}  // namespace

std::unique_ptr<PpsModel> build_model(const PpsBlob* blobs, int nblobs, const PpsModelConfig& c) {
  auto m = std::make_unique<PpsModel>();
  m->cfg = c;
  m->plan = build_plan(c);
  m->x3 = c.math == PPS_MATH_X3;
  m->fused_stem = m->x3 && c.fused_stem && c.width == 128;  // the fused stem's kernel is W = 128
  m->fused_pps = m->x3 && c.fused_pps;
  m->act_planes = m->x3 && c.act_planes;
  const Blobs bmap = match_blobs(m->plan, blobs, nblobs);
  hipStream_t st = nullptr;
  hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
  try {
    compile(*m, bmap, st);
  } catch (...) {
    (void)hipStreamDestroy(st);
    throw;
  }
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  (void)hipStreamDestroy(st);
  for (size_t i = 0; i < m->layers.size(); ++i)
    if (seam_pair(*m, i)) m->layers[i].seam_next = (int)i + 1;
  return m;
}

}  // namespace pps
