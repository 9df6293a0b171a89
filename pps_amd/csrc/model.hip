// Whole-network entry points of libpps_hip.so (include/pps_abi.h, "feature
// extractor as one call"): pps_model_create builds the PPS test net from a
// Detectron weights blob map, owns its packed / bf16x3-split weights, the
// activation buffers per batch size and the per-layer tile / plane / split-K
// table; pps_forward enqueues the whole forward on one stream.
//
// The work is in four files, sharing model_internal.hpp:
//   model_plan.hpp     the layer plan, by the same builders the reference uses
//                      (host only), and the tile-word decoder
//   model_compile.hip  plan -> fused launches with packed / split weights
//   model_run.hip      shapes, workspaces, one layer's launch, one forward
//   model_tune.hip     the autotune
// Each entry point here checks its arguments and makes one call.
//
// This replaces the reference's `workspace.RunNet(model.net)` of the test net
// (detectron/core/test.py:163-165) behind a C ABI.
#include <algorithm>
#include <cstring>

#include "model_internal.hpp"

using namespace pps;

namespace {
template <class F> int guarded(F&& f) {
  try {
    f();
    return PPS_OK;
  } catch (const ModelError& e) {
    set_error(e.what());
    return e.code;
  } catch (const std::exception& e) {
    set_error(std::string("pps model: ") + e.what());
    return PPS_ERR_INVALID_ARG;
  }
}

Layer* find_layer(PpsModel* m, const char* name) {
  PPS_MCHECK(m && name, "null argument");
  for (auto& L : m->layers)
    if (L.name == name) return &L;
  throw ModelError(PPS_ERR_INVALID_ARG, std::string("no layer named '") + name + "'");
}

__global__ void nchw_to_nhwc4_kernel(const float* __restrict__ x, int64_t npix_img, int64_t total,
                                     float4* __restrict__ y) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / npix_img, p = i - n * npix_img;
    const float* src = x + n * 3 * npix_img + p;
    y[i] = make_float4(src[0], src[npix_img], src[2 * npix_img], 0.f);
  }
}
}  // namespace

extern "C" {

int pps_model_config_default(PpsModelConfig* c) {
  if (!c) return PPS_ERR_INVALID_ARG;
  std::memset(c, 0, sizeof(*c));
  c->struct_size = (int)sizeof(PpsModelConfig);
  // configs/market1501/pps_crm_triplet_R-50_1x.yaml (the reference's PPS
  // Market-1501 test configuration)
  c->height = 384; c->width = 128;
  c->strip_num = 5; c->bpm_dim = 128;
  c->num_groups = 1; c->width_per_group = 64; c->stride_1x1 = 1;
  c->res5_stride = 1; c->res5_dilation = 1;
  c->fpn_on = 0; c->fpn_dim = 256;
  c->max_ave = 1; c->normalize = 1;
  c->math = PPS_MATH_X3;
  c->fused_stem = 1; c->fused_pps = 1; c->act_planes = 1;
  c->pixel_means[0] = 102.9801f; c->pixel_means[1] = 115.9465f; c->pixel_means[2] = 122.7717f;
  return PPS_OK;
}

int pps_model_create(const PpsBlob* blobs, int nblobs, const PpsModelConfig* cfg,
                     PpsModel** out) {
  return guarded([&] {
    PPS_MCHECK(out && cfg && (blobs || nblobs == 0) && nblobs >= 0, "null argument");
    PPS_MCHECK(cfg->struct_size == (int)sizeof(PpsModelConfig),
               "PpsModelConfig.struct_size mismatch (use pps_model_config_default)");
    *out = nullptr;
    const PpsModelConfig& c = *cfg;
    PPS_MCHECK(c.height > 0 && c.width > 0 && c.strip_num >= 1 && c.strip_num <= 10 &&
                   c.bpm_dim > 0 && c.num_groups > 0 && c.width_per_group > 0 &&
                   c.res5_stride >= 1 && c.res5_dilation >= 1 && c.fpn_dim > 0,
               "bad config");
    PPS_MCHECK(c.math == PPS_MATH_X3 || c.math == PPS_MATH_F32, "math must be PPS_MATH_X3 or _F32");
    *out = build_model(blobs, nblobs, c).release();
  });
}

int pps_model_destroy(PpsModel* m) {
  return guarded([&] {
    if (!m) return;
    (void)hipDeviceSynchronize();  // no launch of this model may still read its buffers
    delete m;
  });
}

int pps_model_feat_dim(const PpsModel* m) { return m ? m->plan.feat_dim : -1; }
int pps_model_num_layers(const PpsModel* m) { return m ? (int)m->layers.size() : -1; }

int pps_model_layer_info(const PpsModel* m, int i, int N, PpsLayerInfo* info) {
  return guarded([&] {
    PPS_MCHECK(m && info, "null argument");
    PPS_MCHECK(i >= 0 && i < (int)m->layers.size(), "layer index out of range");
    PPS_MCHECK(N > 0, "N must be positive");
    const Layer& L = m->layers[i];
    const auto shapes = infer_shapes(*m, N);
    std::memset(info, 0, sizeof(*info));
    info->name = L.name.c_str();
    info->op = op_name(L.op);
    info->tile = L.tile;
    info->splitk = L.splitk;
    info->planes_in = L.planes_in;
    info->planes_out = L.planes_out;
    info->gemm = tunable(L) || L.op == Op::StemPool;
    info->flops = layer_flops(L, shapes, N);
    info->bytes = layer_bytes(*m, L, shapes, N);
    const Shape& y = shapes.at(L.output);
    for (int d = 0; d < 4; ++d) info->out_shape[d] = y.d[d];
    info->output = L.output.c_str();
  });
}

int pps_model_set_tile(PpsModel* m, const char* layer, int tile) {
  return guarded([&] {
    Layer* L = find_layer(m, layer);
    // the fused stem takes 0 (bf16x3) or PPS_TILE_H2 (f16x2) only
    if (L->op == Op::StemPool) {
      PPS_MCHECK(tile == 0 || (tile == PPS_TILE_H2 && h2_tile_ok(*L, tile)),
                 std::string("stem '") + layer + "': tile 0 or PPS_TILE_H2 (f16x2) only");
      L->tile = tile;
      return;
    }
    PPS_MCHECK(tunable(*L), std::string("layer '") + layer + "' has no GEMM tile");
    // (the conditions of the checks are part of their error texts: kept as written)
    const int base = tile_base(tile);
    PPS_MCHECK(tile >= 0 && base < GEMM_NUM_TILES, "tile out of range");
    PPS_MCHECK(!(tile & PPS_TILE_H2) || h2_tile_ok(*L, tile),
               std::string("PPS_TILE_H2: '") + layer +
                   "' has no f16x2 weights (Cin % 32 == 0) or the base tile is not 0, 38..53, "
                   "55, 60 or (convs) 56..59; PPS_TILE_H2P: plain convs and conv_pps only");
    PPS_MCHECK(!(tile & PPS_TILE_H2P) || (tile & PPS_TILE_H2),
               "PPS_TILE_H2P goes with PPS_TILE_H2");
    PPS_MCHECK(!(tile & PPS_TILE_H2E) || ((tile & PPS_TILE_H2) && h2e_producer(*m, *L) >= 0),
               std::string("PPS_TILE_H2E: '") + layer + "' needs PPS_TILE_H2 and a producer "
               "that is a conv + BN + ReLU read by it alone (Cin % 32 == 0)");
    PPS_MCHECK(!(tile & PPS_TILE_SEAM) ||
                   (L->seam_next >= 0 && base == GEMM_TILE_WS &&
                    !(tile & (PPS_TILE_B_TILED | PPS_TILE_COL_ORDER))),
               std::string("PPS_TILE_SEAM: '") + layer +
                   "' is not a branch2c feeding a seam-capable branch2a (base tile 54)");
    PPS_MCHECK(!(tile & PPS_TILE_B_TILED) ||
                   (L->wt && tile_lands_pipelined(base) && tile_kind(base) != TileKind::WS),
               "PPS_TILE_B_TILED: x3 conv with Cin % 32 == 0 on a pipelined tile only");
    PPS_MCHECK(!(tile & PPS_TILE_COL_ORDER) ||
                   (L->op != Op::Heads && tile_lands_pipelined(base) &&
                    tile_kind(base) != TileKind::WS),
               "PPS_TILE_COL_ORDER: conv layers on a pipelined tile only");
    L->tile = tile;
  });
}

int pps_model_set_splitk(PpsModel* m, const char* layer, int splitk) {
  return guarded([&] {
    Layer* L = find_layer(m, layer);
    PPS_MCHECK(L->op == Op::Conv, std::string("split-K applies to plain convs, not '") + layer + "'");
    PPS_MCHECK(splitk == 1 || !(L->tile & PPS_TILE_H2),
               std::string("'") + layer + "' runs an f16x2 tile: no split-K");
    PPS_MCHECK(splitk >= 1 && splitk <= kMaxSplitK, "splitk must be in [1, 4]");
    PPS_MCHECK(splitk == 1 || (m->x3 && L->cin_eff % 32 == 0 && L->kpad == L->k * L->k * L->cin_eff &&
                               L->kpad % (32 * splitk) == 0),
               "split-K " + std::to_string(splitk) + " not possible for " + layer);
    L->splitk = splitk;
  });
}

int pps_model_num_plane_edges(const PpsModel* m) { return m ? (int)m->edges.size() : -1; }

int pps_model_plane_edge(const PpsModel* m, int i, const char** producer, const char** consumer,
                         int* on) {
  return guarded([&] {
    PPS_MCHECK(m && producer && consumer && on, "null argument");
    PPS_MCHECK(i >= 0 && i < (int)m->edges.size(), "edge index out of range");
    const Layer& P = m->layers[m->edges[i].first];
    *producer = P.name.c_str();
    *consumer = m->layers[m->edges[i].second].name.c_str();
    *on = P.planes_out;
  });
}

int pps_model_set_planes(PpsModel* m, const char* producer, int on) {
  return guarded([&] {
    PPS_MCHECK(m && producer, "null argument");
    for (auto& e : m->edges)
      if (m->layers[e.first].name == producer) {
        PPS_MCHECK(!on || !((m->layers[e.first].tile | m->layers[e.second].tile) & PPS_TILE_H2),
                   std::string("plane edge '") + producer + "': an f16x2 (PPS_TILE_H2) layer "
                   "takes and writes f32 activations");
        m->layers[e.first].planes_out = m->layers[e.second].planes_in = on != 0;
        return;
      }
    throw ModelError(PPS_ERR_INVALID_ARG,
                     std::string("not a plane-eligible producer: '") + producer + "'");
  });
}

int pps_model_reserve(PpsModel* m, int N) {
  return guarded([&] {
    PPS_MCHECK(m && N > 0, "bad arguments");
    Workspace& w = workspace(*m, N, nullptr, true);
    nhwc4_buffer(*m, w, nullptr);
    w.pinned = true;
  });
}

int pps_model_release(PpsModel* m, int N) {
  return guarded([&] {
    PPS_MCHECK(m, "null argument");
    (void)hipDeviceSynchronize();
    if (N > 0) m->ws.erase(N);
    else m->ws.clear();
  });
}

int pps_model_tensor(const PpsModel* m, int N, const char* blob, void** ptr, int* planes,
                     int64_t* shape4) {
  return guarded([&] {
    PPS_MCHECK(m && blob && ptr && planes && shape4, "null argument");
    auto it = m->ws.find(N);
    PPS_MCHECK(it != m->ws.end(), "no workspace for this batch size (pps_model_reserve)");
    auto b = it->second.bufs.find(blob);
    PPS_MCHECK(b != it->second.bufs.end(), std::string("no device tensor '") + blob + "'");
    *ptr = b->second->p;
    *planes = 0;
    for (const auto& L : m->layers) {
      if (L.output == blob && L.planes_out) *planes = 1;
      // read by a PPS_TILE_H2E layer: f16x2 planes on the slot's scale
      if (L.input == blob && tile_h2e(L.tile) && h2e_producer(*m, L) >= 0) *planes = 2;
    }
    const Shape& s = it->second.shapes.at(blob);
    for (int d = 0; d < 4; ++d) shape4[d] = s.d[d];
  });
}

int pps_model_tensor_amax(const PpsModel* m, int N, const char* blob, float* out) {
  return guarded([&] {
    PPS_MCHECK(m && blob && out, "null argument");
    auto it = m->ws.find(N);
    PPS_MCHECK(it != m->ws.end(), "no workspace for this batch size (pps_model_reserve)");
    auto s = m->slot.find(blob);
    PPS_MCHECK(s != m->slot.end(), std::string("no activation-max slot for '") + blob + "'");
    float h[PPS_AMAX_SLOT_FLOATS];
    hip_check(hipMemcpy(h, slot_at(it->second, s->second), sizeof(h), hipMemcpyDeviceToHost),
              "hipMemcpy");
    float mx = 0.f;
    for (int j = 0; j < kAmaxSubs; ++j) mx = std::max(mx, h[j * kAmaxStride]);
    *out = mx;
  });
}

int pps_forward_layers_flags(const PpsModel* m, const float* x, int N, float* feat, int first,
                             int last, int flags, void* stream) {
  return guarded([&] {
    PPS_MCHECK(m && x && feat, "null pointer");
    PPS_MCHECK(N > 0, "N must be positive");
    PPS_MCHECK(0 <= first && first <= last && last <= (int)m->layers.size(), "bad layer range");
    PPS_MCHECK(aligned16(x) && aligned16(feat), "x / feat must be 16-byte aligned");
    PPS_MCHECK((flags & ~PPS_FWD_KEEP_AMAX) == 0, "unknown pps_forward_layers flags");
    forward_range(*m, x, N, feat, first, last, as_stream(stream), (flags & PPS_FWD_KEEP_AMAX) != 0);
  });
}

int pps_forward_layers(const PpsModel* m, const float* x, int N, float* feat, int first,
                       int last, void* stream) {
  return pps_forward_layers_flags(m, x, N, feat, first, last, 0, stream);
}

int pps_forward(const PpsModel* m, const float* nhwc4, int N, float* feat, void* stream) {
  return pps_forward_layers(m, nhwc4, N, feat, 0, m ? (int)m->layers.size() : 0, stream);
}

int pps_forward_nchw(const PpsModel* m, const float* nchw, int N, float* feat, void* stream) {
  return guarded([&] {
    PPS_MCHECK(m && nchw && feat, "null pointer");
    PPS_MCHECK(N > 0, "N must be positive");
    const hipStream_t st = as_stream(stream);
    Workspace& w = workspace(*m, N, st, true);
    float* x = nhwc4_buffer(*m, w, st);
    const int64_t npix = (int64_t)m->cfg.height * m->cfg.width, total = npix * N;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, nchw, npix,
                       total, reinterpret_cast<float4*>(x));
    hip_check(hipGetLastError(), "nchw_to_nhwc4_kernel");
    forward_range(*m, x, N, feat, 0, (int)m->layers.size(), st);
  });
}

int pps_forward_bgr(const PpsModel* m, const uint8_t* img, int N, int Hi, int Wi, float* feat,
                    void* stream) {
  return guarded([&] {
    PPS_MCHECK(m && img && feat, "null pointer");
    PPS_MCHECK(N > 0, "N must be positive");
    const hipStream_t st = as_stream(stream);
    Workspace& w = workspace(*m, N, st, true);
    float* x = nhwc4_buffer(*m, w, st);
    PPS_MCHECK(Hi > 0 && Wi > 0, "bad image shape");
    // preprocessing inside the forward, after the maxima slots are zeroed:
    // it reports max|x| for an f16x2 stem (no separate pass over x)
    const std::function<void(float*)> pre = [&](float* slot) {
      rc_check(preprocess_bgr(img, N, Hi, Wi, nullptr, nullptr, nullptr, m->cfg.pixel_means,
                              m->cfg.height, m->cfg.width, x, st, slot));
    };
    forward_range(*m, x, N, feat, 0, (int)m->layers.size(), st, false, &pre);
  });
}

int pps_model_autotune(PpsModel* m, const float* x, int N, int flags, void* stream) {
  return guarded([&] {
    PPS_MCHECK(m && x, "null pointer");
    PPS_MCHECK(N > 0, "N must be positive");
    const hipStream_t st = as_stream(stream);
    PPS_MCHECK(!capturing(st), "autotune cannot run inside a graph capture");
    autotune(*m, x, N, flags, st);
  });
}

}  // extern "C"
