// pps_model_autotune: the per-layer tile / plane-edge / split-K / seam search
// (the reference's cudnn_exhaustive_search analogue, modeling/detector.py:58;
// same procedure as PPSModel.autotune), as a list of passes over one state.
#include <algorithm>

#include "model_internal.hpp"

#ifndef PPS_TUNE_FINALISTS
#define PPS_TUNE_FINALISTS 4  // probes: more screened tiles into the interleaved final rounds
#endif

namespace pps {
namespace {

// isolated launches: screen every candidate, then the best few in interleaved rounds
constexpr int kReps = 3, kFinalists = PPS_TUNE_FINALISTS, kFinalReps = 10, kFinalRounds = 3;
// whole forwards (the in-forward passes)
constexpr int kFwdReps = 6, kFwdRounds = 3;
// a change is kept if it is > 2 % faster in isolation, > 0.5 % inside the forward
constexpr float kAccept = 0.98f, kAcceptFwd = 0.995f;

struct Timer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  Timer() {
    hip_check(hipEventCreate(&e0), "hipEventCreate");
    hip_check(hipEventCreate(&e1), "hipEventCreate");
  }
  Timer(const Timer&) = delete;
  ~Timer() {
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  void start(hipStream_t st) { hip_check(hipEventRecord(e0, st), "hipEventRecord"); }
  float stop_ms(hipStream_t st) {
    hip_check(hipEventRecord(e1, st), "hipEventRecord");
    hip_check(hipEventSynchronize(e1), "hipEventSynchronize");
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    return ms;
  }
};

using Ranked = std::vector<std::pair<float, int>>;  // (ms, tile), best first

struct Tune {
  PpsModel& m;
  const float* x;
  int N;
  int flags;
  hipStream_t st;
  Workspace* w;
  Timer t;
  // f16x2 candidates (PPS_TILE_H2) beside the bf16x3 tiles of a layer with
  // f32 activations at both ends and no split-K
  bool try_h2 = false;
  std::vector<float> cost;  // per layer: its launch's best time so far
  // every tuned layer's finalists, best first, and an f16x2-planes reader's
  // pick before the planes / on them, kept or not (the in-forward group pass)
  std::map<const Layer*, Ranked> ranked;
  std::map<const Layer*, int> pre_h2e, h2e_best;
};

float time_forward(Tune& s, float* feat, int reps) {
  const int n = (int)s.m.layers.size();
  forward_range(s.m, s.x, s.N, feat, 0, n, s.st);
  s.t.start(s.st);
  for (int i = 0; i < reps; ++i) forward_range(s.m, s.x, s.N, feat, 0, n, s.st);
  return s.t.stop_ms(s.st) / reps;
}

float time_layer(Tune& s, const Layer& L, int tile, int sk, int reps) {
  for (int i = 0; i < 2; ++i) run_layer(s.m, L, *s.w, s.x, nullptr, false, tile, sk, s.st);
  s.t.start(s.st);
  for (int i = 0; i < reps; ++i) run_layer(s.m, L, *s.w, s.x, nullptr, false, tile, sk, s.st);
  return s.t.stop_ms(s.st) / reps;
}

// min over the final rounds of one launch
float time_layer_final(Tune& s, const Layer& L, int tile) {
  float ms = 1e30f;
  for (int r = 0; r < kFinalRounds; ++r) ms = std::min(ms, time_layer(s, L, tile, 1, kFinalReps));
  return ms;
}

// The tiles a layer is screened on
std::vector<int> cands_of(const Layer& L, const Shapes& shapes, bool try_h2) {
  std::vector<int> c;
  const bool h2ok = try_h2 && L.w2 && !L.planes_in && !L.planes_out && L.splitk == 1;
  if (L.op == Op::ConvPps) {
    c = pps_tiles(L, shapes.at(L.conv_output));
    if (h2ok) {
      const size_t n = c.size();
      for (size_t i = 0; i < n; ++i)
        if (c[i] >= GEMM_TILE_P16_FIRST) c.push_back(c[i] | PPS_TILE_H2);
    }
  } else {
    const bool pipelined_only = L.planes_in || L.planes_out;
    for (int tl = pipelined_only ? GEMM_TILE_P_FIRST : 1; tl < GEMM_NUM_TILES; ++tl)
      if (tl != GEMM_TILE_P16_192x128W41) c.push_back(tl);   // (f16x2 only)
    // (PPS_AUTOTUNE_NO_WSH2=1, A/B runs: no f16x2 weight-stationary tile)
    static const bool no_wsh2 = getenv_flag_on("PPS_AUTOTUNE_NO_WSH2");
    if (h2ok)
      for (int tl = GEMM_TILE_P16_FIRST; tl < GEMM_NUM_TILES; ++tl)
        if (h2_tile_ok(L, tl | PPS_TILE_H2) && !(no_wsh2 && tl == GEMM_TILE_WS) &&
            !(tl >= GEMM_TILE_C16_FIRST && tl != GEMM_TILE_P16_192x128W41 &&
              (L.k != 3 || L.stride != 1)))
          c.push_back(tl | PPS_TILE_H2);
  }
  if (c.empty()) c.push_back(0);
  return c;
}

// One layer's tile: screen the candidates, then the finalists -- each also on
// the chunk-tiled weight copy and / or in column-major tile order -- timed in
// interleaved rounds (min per variant), so a drifting clock does not favour
// whichever ran first.  extra: flags or-ed into every candidate
// (PPS_TILE_H2E: the f16x2 tiles only, reading the planes the producer wrote)
float tune_layer(Tune& s, Layer& L, int extra = 0) {
  Ranked screen;
  for (int tl : cands_of(L, s.w->shapes, s.try_h2)) {
    if (extra && !(tile_h2(tl) && h2_tile_ok(L, tl | extra))) continue;
    tl |= extra;
    screen.emplace_back(time_layer(s, L, tl, L.splitk, kReps), tl);
  }
  std::sort(screen.begin(), screen.end());
  std::vector<int> var;
  for (int i = 0; i < (int)screen.size() && i < kFinalists; ++i) {
    const int tl = screen[i].second;
    var.push_back(tl);
    // f16x2 finalists also with the input split once into planes
    if (tile_h2(tl) && h2_tile_ok(L, tl | PPS_TILE_H2P)) var.push_back(tl | PPS_TILE_H2P);
    // (the weight-stationary kernel has no tile order to choose)
    const int tb = tile_base(tl);
    if (L.splitk == 1 && L.op != Op::Heads && tile_lands_pipelined(tb) &&
        tile_kind(tb) != TileKind::WS)
      for (int f : {PPS_TILE_B_TILED, PPS_TILE_COL_ORDER, PPS_TILE_B_TILED | PPS_TILE_COL_ORDER})
        if (!(f & PPS_TILE_B_TILED) || (L.wt && !tile_h2(tl))) var.push_back(tl | f);
  }
  std::vector<float> tmin(var.size(), 1e30f);
  for (int r = 0; r < kFinalRounds; ++r)
    for (size_t v = 0; v < var.size(); ++v)
      tmin[v] = std::min(tmin[v], time_layer(s, L, var[v], L.splitk, kFinalReps));
  float best = 1e30f;
  Ranked& rk = s.ranked[&L];
  rk.clear();
  for (size_t v = 0; v < var.size(); ++v) {
    rk.emplace_back(tmin[v], var[v]);
    if (tmin[v] < best) { best = tmin[v]; L.tile = var[v]; }
  }
  std::sort(rk.begin(), rk.end());
  return best;
}

void set_edge(PpsModel& m, const std::pair<int, int>& e, bool on) {
  m.layers[e.first].planes_out = m.layers[e.second].planes_in = on;
}

// ---- the passes, in the order autotune() runs them ------------------------------

// 1. every GEMM layer on its own (plane edges off when they are tuned below)
void screen_pass(Tune& s) {
  for (size_t i = 0; i < s.m.layers.size(); ++i)
    if (tunable(s.m.layers[i])) s.cost[i] = tune_layer(s, s.m.layers[i]);
}

// 2. the fused stem: f16x2 (plus the pass that measures the input's max, run
// by every forward that takes it) against bf16x3, interleaved rounds
void stem_pass(Tune& s) {
  for (Layer& L : s.m.layers)
    if (L.op == Op::StemPool) L.tile = 0;
  if (!s.try_h2) return;
  for (Layer& L : s.m.layers) {
    float* ds = slot_ptr(s.m, *s.w, "data");
    if (L.op != Op::StemPool || !h2_tile_ok(L, PPS_TILE_H2) || !ds) continue;
    const int64_t n = s.w->shapes.at("data").numel();
    float tx = 1e30f, th = 1e30f, ta = 1e30f;
    for (int r = 0; r < kFinalRounds; ++r) {
      tx = std::min(tx, time_layer(s, L, 0, 1, kFinalReps));
      th = std::min(th, time_layer(s, L, PPS_TILE_H2, 1, kFinalReps));
      s.t.start(s.st);
      for (int i = 0; i < kFinalReps; ++i) rc_check(amax_of(s.x, n, ds, s.st));  // same max again
      ta = std::min(ta, s.t.stop_ms(s.st) / kFinalReps);
    }
    L.tile = th + ta < kAccept * tx ? PPS_TILE_H2 : 0;
  }
}

// 3. bf16x3 plane edges: producer and consumer re-tuned with the tensor as
// planes, kept if the pair gets faster
void plane_edge_pass(Tune& s) {
  for (auto& e : s.m.edges) {
    Layer& P = s.m.layers[e.first];
    Layer& C = s.m.layers[e.second];
    const float before = s.cost[e.first] + s.cost[e.second];
    const int tp = P.tile, tc = C.tile;
    set_edge(s.m, e, true);
    const float cp = tune_layer(s, P), cc = tune_layer(s, C);
    if (cp + cc < kAccept * before) {
      s.cost[e.first] = cp; s.cost[e.second] = cc;
    } else {
      set_edge(s.m, e, false);
      P.tile = tp; C.tile = tc;
    }
  }
}

// 4. conv split-K 2..kMaxSplitK on the one-launch split-K tiles, plain and
// chunk-tiled weights
void splitk_pass(Tune& s) {
  for (size_t i = 0; i < s.m.layers.size(); ++i) {
    Layer& L = s.m.layers[i];
    if (L.op != Op::Conv || !h2_weights_capable(L)) continue;
    std::vector<std::pair<float, std::pair<int, int>>> screen;
    for (int sk = 2; sk <= kMaxSplitK; ++sk) {
      if (L.kpad % (32 * sk)) continue;
      const int save = L.splitk;
      L.splitk = sk;
      s.w = &workspace(s.m, s.N, s.st, true);  // grow the partials buffer
      L.splitk = save;
      for (int tl = GEMM_TILE_P16_FIRST + 7; tl <= GEMM_TILE_P16_96x128W24; ++tl) {
        if (!fix_tile(tl)) continue;
        for (int f : {0, PPS_TILE_B_TILED})
          if (!f || L.wt) screen.push_back({time_layer(s, L, tl | f, sk, kReps), {tl | f, sk}});
      }
    }
    if (screen.empty()) continue;
    std::sort(screen.begin(), screen.end());
    float best = 1e30f;
    std::pair<int, int> pick{0, 1};
    for (int j = 0; j < (int)screen.size() && j < kFinalists; ++j) {
      const auto o = screen[j].second;
      const float ms = time_layer(s, L, o.first, o.second, kFinalReps);
      if (ms < best) { best = ms; pick = o; }
    }
    if (best < kAccept * s.cost[i]) {
      L.tile = pick.first; L.splitk = pick.second; s.cost[i] = best;
    }
  }
}

// 5. bottleneck seams: branch2c + the next branch2a in one launch, kept
// if > 2 % faster than the two tuned launches
void seam_pass(Tune& s) {
  for (size_t i = 0; i < s.m.layers.size(); ++i) {
    Layer& L = s.m.layers[i];
    if (!seam_ok(s.m, L)) continue;
    const float ts = time_layer_final(s, L, GEMM_TILE_WS | PPS_TILE_SEAM);
    if (ts < kAccept * (s.cost[i] + s.cost[L.seam_next])) {
      L.tile = GEMM_TILE_WS | PPS_TILE_SEAM;
      s.cost[i] = ts;
      s.cost[L.seam_next] = 0.f;
    }
  }
}

// 6. f16x2 planes from the producer's epilogue (PPS_TILE_H2E): the consumer
// re-tuned over the f16x2 tiles reading them (the planes input favours other
// tiles than f32 does), kept if the producer + consumer pair is > 2 % faster
void h2e_pass(Tune& s) {
  PpsModel& m = s.m;
  // (a seam launch keeps its pair: its cost also holds the next layer's)
  auto plain_f32 = [](const Layer& L) {
    return !L.planes_in && !L.planes_out && L.splitk == 1 && !tile_seam(L.tile);
  };
  for (size_t ci = 0; ci < m.layers.size(); ++ci) {
    Layer& C = m.layers[ci];
    if (!C.w2 || !plain_f32(C)) continue;
    const int pi = h2e_producer(m, C);
    if (pi < 0) continue;
    Layer& P = m.layers[pi];
    if (!plain_f32(P)) continue;
    int first = -1;   // an f16x2 tile of C, so P writes the planes from here on
    for (int tl : cands_of(C, s.w->shapes, s.try_h2))
      if (tile_h2(tl) && h2_tile_ok(C, tl | PPS_TILE_H2E)) { first = tl; break; }
    if (first < 0) continue;
    const int save = C.tile;
    const Ranked save_rank = s.ranked[&C];
    C.tile = first | PPS_TILE_H2E;
    run_layer(m, P, *s.w, s.x, nullptr, false, P.tile, 1, s.st);
    const float tc = tune_layer(s, C, PPS_TILE_H2E);
    s.h2e_best[&C] = C.tile;
    const float tp = time_layer_final(s, P, P.tile);
    if (tp + tc < kAccept * (s.cost[pi] + s.cost[ci])) {
      s.cost[pi] = tp;
      s.cost[ci] = tc;
      s.pre_h2e[&C] = save;
    } else {
      C.tile = save;
      s.ranked[&C] = save_rank;
      run_layer(m, P, *s.w, s.x, nullptr, false, P.tile, 1, s.st);   // f32 output again
    }
  }
}

// 7. The in-forward pass over layers of one shape: the members' three best
// distinct tiles (their own f16x2-plane flags kept), each applied to the whole
// group, and the group's planes edges all on (each reader on its best planes
// variant, h2e_best) or all off (pre_h2e), timed as whole forwards in
// interleaved rounds; the group moves to the best assignment if it beats the
// current one by > 0.5 %.  A layer of its own shape tries its three best
// variants as they are.  Seam pairs keep their launch.
void group_pass(Tune& s) {
  PpsModel& m = s.m;
  constexpr int kKeep = PPS_TILE_H2E | PPS_TILE_H2P;
  std::map<std::string, std::vector<int>> groups;
  for (size_t i = 0; i < m.layers.size(); ++i) {
    const Layer& L = m.layers[i];
    if (!s.ranked.count(&L) || tile_seam(L.tile) || L.op == Op::Heads) continue;
    if (i > 0 && tile_seam(m.layers[i - 1].tile) && m.layers[i - 1].seam_next == (int)i) continue;
    const Shape& sh = s.w->shapes.at(L.input);
    std::string key = std::to_string((int)L.op);
    for (int v : {L.cin_eff, L.cout, L.kpad, L.k, L.stride, L.pad, L.dil, L.shortcut_cin,
                  (int)L.relu, (int)L.residual.empty(), (int)L.planes_in, (int)L.planes_out,
                  L.splitk})
      key += "," + std::to_string(v);
    for (int d = 0; d < 4; ++d) key += "," + std::to_string(sh.d[d]);
    groups[key].push_back((int)i);
  }
  DevBuf feat((size_t)s.N * m.plan.feat_dim * sizeof(float));
  for (const auto& g : groups) {
    const std::vector<int>& mem = g.second;
    const bool single = mem.size() == 1;
    std::vector<int> save;
    for (int i : mem) save.push_back(m.layers[i].tile);
    // candidate assignments (one tile per member); [0] = the current one
    std::vector<std::vector<int>> cands{save};
    auto add = [&](const std::vector<int>& a) {
      if (std::find(cands.begin(), cands.end(), a) == cands.end()) cands.push_back(a);
    };
    std::vector<int> bases;
    for (int i : mem) {
      int taken = 0;
      for (const auto& r : s.ranked.at(&m.layers[i])) {
        const int c = single ? r.second : r.second & ~kKeep;
        if (std::find(bases.begin(), bases.end(), c) == bases.end()) bases.push_back(c);
        if (++taken == 3) break;
      }
    }
    for (int c : bases) {   // one tile for the whole group (members' plane flags kept)
      std::vector<int> a(mem.size());
      for (size_t j = 0; j < mem.size(); ++j) {
        const Layer& L = m.layers[mem[j]];
        int tl = single ? c : c | (tile_h2(c) ? (save[j] & kKeep) : 0);
        if (tile_h2p(tl) && !h2_tile_ok(L, tl)) tl &= ~PPS_TILE_H2P;
        if (tile_h2e(tl) && !h2_tile_ok(L, tl)) tl &= ~PPS_TILE_H2E;
        a[j] = tl;
      }
      add(a);
    }
    // the f16x2-planes edges into the group: every reader on its best planes
    // variant, and every reader back on its pick without them
    std::vector<int> on = save, off = save;
    for (size_t j = 0; j < mem.size(); ++j) {
      const Layer* L = &m.layers[mem[j]];
      if (s.h2e_best.count(L)) on[j] = s.h2e_best.at(L);
      if (s.pre_h2e.count(L) && tile_h2e(save[j])) off[j] = s.pre_h2e.at(L);
    }
    add(on);
    add(off);
    if (cands.size() < 2) continue;
    auto apply = [&](const std::vector<int>& a) {
      for (size_t j = 0; j < mem.size(); ++j) m.layers[mem[j]].tile = a[j];
    };
    std::vector<float> tmin(cands.size(), 1e30f);
    for (int r = 0; r < kFwdRounds; ++r)
      for (size_t v = 0; v < cands.size(); ++v) {
        apply(cands[v]);
        tmin[v] = std::min(tmin[v], time_forward(s, feat.as<float>(), kFwdReps));
      }
    size_t best = 0;
    for (size_t v = 1; v < cands.size(); ++v)
      if (tmin[v] < tmin[best]) best = v;
    apply(best > 0 && tmin[best] < kAcceptFwd * tmin[0] ? cands[best] : save);
  }
}

// 8. The bottleneck seams judged inside whole forwards too: each seam-capable
// branch2c with its launch toggled (on: the seam tile; off: its best tile of
// its own, ranked), kept if the forward gets > 0.5 % faster.  The seam pass
// before it judged the pair's two isolated launches.
void seam_forward_pass(Tune& s) {
  DevBuf feat((size_t)s.N * s.m.plan.feat_dim * sizeof(float));
  for (Layer& L : s.m.layers) {
    if (!seam_ok(s.m, L) || !s.ranked.count(&L)) continue;
    const int save = L.tile;
    int alt = GEMM_TILE_WS | PPS_TILE_SEAM;
    if (tile_seam(save)) {   // off: the layer's best variant of its own
      alt = -1;
      for (const auto& r : s.ranked.at(&L))
        if (!tile_seam(r.second)) { alt = r.second; break; }
      if (alt < 0) continue;
    }
    float t0 = 1e30f, t1 = 1e30f;
    for (int r = 0; r < kFwdRounds; ++r) {
      L.tile = save;
      t0 = std::min(t0, time_forward(s, feat.as<float>(), kFwdReps));
      L.tile = alt;
      t1 = std::min(t1, time_forward(s, feat.as<float>(), kFwdReps));
    }
    L.tile = t1 < kAcceptFwd * t0 ? alt : save;
  }
}

// planes workspace for the PPS_TILE_H2P candidates
void grow_h2p_for_candidates(const PpsModel& m, Workspace* w) {
  size_t hneed = 0;
  for (const Layer& L : m.layers)
    if (L.w2 && (L.op == Op::Conv || L.op == Op::ConvPps))
      hneed = std::max(hneed, (size_t)w->shapes.at(L.input).numel());
  if (hneed <= w->h2p_elems) return;
  PPS_MCHECK(!w->pinned, "autotune: the batch's buffers are pinned (pps_model_reserve); "
                         "release them first");
  w->h2p = std::make_shared<DevBuf>(hneed * 2 * sizeof(uint16_t));
  w->h2p_elems = hneed;
}

}  // namespace

void autotune(PpsModel& m, const float* x, int N, int flags, hipStream_t st) {
  Workspace* w = &workspace(m, N, st, true);
  // every candidate may be an f16x2 tile: all producers report maxima
  struct AmaxAll {
    const PpsModel& m;
    ~AmaxAll() { m.amax_all = false; }
  } amax_guard{m};
  m.amax_all = true;
  DevBuf feat((size_t)N * m.plan.feat_dim * sizeof(float));
  forward_range(m, x, N, feat.as<float>(), 0, (int)m.layers.size(), st);
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  Tune s{m, x, N, flags, st, w};
  s.try_h2 = m.x3 && !(flags & PPS_AUTOTUNE_NO_H2);
  s.cost.assign(m.layers.size(), 0.f);
  if (s.try_h2) grow_h2p_for_candidates(m, w);
  const bool tune_planes = (flags & PPS_AUTOTUNE_NO_PLANES) == 0 && m.act_planes;
  if (tune_planes)
    for (auto& e : m.edges) set_edge(m, e, false);
  screen_pass(s);
  stem_pass(s);
  if (tune_planes) plane_edge_pass(s);
  if (m.x3 && (flags & PPS_AUTOTUNE_SPLITK)) splitk_pass(s);
  if (!(flags & PPS_AUTOTUNE_NO_SEAM)) seam_pass(s);
  if (s.try_h2 && !(flags & PPS_AUTOTUNE_NO_H2E)) h2e_pass(s);
  if (!(flags & PPS_AUTOTUNE_NO_GROUPS)) {
    group_pass(s);
    if (!(flags & PPS_AUTOTUNE_NO_SEAM)) seam_forward_pass(s);
  }
  hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace pps
