// What the whole-network translation units share (model.hip: the C entry
// points; model_compile.hip: plan -> packed weights and fused launches;
// model_run.hip: shapes, workspaces, one layer, one forward; model_tune.hip:
// the autotune): the error type, device buffers, the compiled layer, the
// per-batch workspace and the model itself.
#pragma once
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "model_plan.hpp"
#include "pps_internal.hpp"

#pragma GCC visibility push(hidden)
namespace pps {

constexpr int kHeadSplitK = 8;  // K = 2048 head GEMMs cut 8 ways (pps_amd/model.py HEAD_SPLITK)
constexpr int kMaxSplitK = 4;   // conv split-K factors the autotune tries

struct ModelError : std::runtime_error {
  int code;
  ModelError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
#define PPS_MCHECK(cond, msg)                                                         \
  do {                                                                                \
    if (!(cond))                                                                      \
      throw ModelError(PPS_ERR_INVALID_ARG, std::string("[enforce fail at ") +       \
                                                __func__ + "] " + #cond + ". " + (msg)); \
  } while (0)

inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw ModelError(PPS_ERR_LAUNCH, std::string(what) + ": " + hipGetErrorString(e));
}
inline void rc_check(int rc) {  // an op-level entry point failed: its message is already set
  if (rc != PPS_OK) throw ModelError(rc, pps_last_error());
}

inline bool getenv_flag_on(const char* name) {
  const char* v = std::getenv(name);
  return v && v[0] && std::strcmp(v, "0") != 0;
}

// ---- device memory ------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  explicit DevBuf(size_t n) : bytes(n) {
    if (n) hip_check(hipMalloc(&p, n), "hipMalloc");
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
using Buf = std::shared_ptr<DevBuf>;

// ---- compiled layers ----------------------------------------------------------
struct Layer {
  Op op;
  std::string name;  // tuning key: conv name, or the output blob for heads / pooling
  std::string input, input2, output, residual, conv_output;
  int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, dil = 1, stride2 = 1;
  bool relu = false;
  int cin_eff = 0, kpad = 0, shortcut_cin = 0;
  Buf w, scale, shift;  // w: f32 [Cout][Kpad] or bf16x3 planes
  Buf wt;               // x3 plain convs with Kpad % 32 == 0: the planes chunk-tiled
                        // (pps_tile_planes), used when tile carries PPS_TILE_B_TILED
  float h2o_bw = 0.f, h2o_bb = 0.f;  // output bound constants (pps_h2_out_bound; 0: none)
  Buf w2, wrs;          // the f16x2 split (PPS_TILE_H2): two chunk-tiled f16 planes
                        // [2][Cout16/16][K/32][16][32] and per-channel scales [Cout]
  std::vector<int> split;
  bool max_ave = false, normalize = false;
  int nsub = 0, dim = 0, dim_inner = 0;
  int tile = 0, splitk = 1;
  bool planes_in = false, planes_out = false;
  int seam_next = -1;   // the next layer a PPS_TILE_SEAM launch also computes
};

inline bool is_conv(const Layer& L) { return L.op == Op::Conv || L.op == Op::ConvDual; }
// The GEMM's whole K: the conv's own (padded) K, then the fused shortcut's Cin
inline int layer_k(const Layer& L) {
  return L.op == Op::ConvDual ? L.kpad + L.shortcut_cin : L.kpad;
}
// The f16x2 split can run this layer's own conv (PPS_TILE_H2; also what conv
// split-K asks): Cin % 32 == 0, no K padding
inline bool h2_weights_capable(const Layer& L) {
  return L.cin_eff % 32 == 0 && L.kpad == L.k * L.k * L.cin_eff;
}

struct Shape {
  int64_t d[4] = {0, 0, 0, 0};
  int64_t numel() const { return d[0] * d[1] * d[2] * d[3]; }
};
using Shapes = std::map<std::string, Shape>;

struct Workspace {
  int N = 0;
  Shapes shapes;
  std::map<std::string, Buf> bufs;  // plane-capable tensors hold 6 B per element
  Buf part;                         // conv split-K partials
  size_t part_floats = 0;
  Buf h2p;                          // f16x2 activation planes of a PPS_TILE_H2P layer's input
  size_t h2p_elems = 0;
  Buf cnt;                          // one-launch split-K tile counters (zero between launches)
  size_t cnt_ints = 0;
  Buf nhwc4;                        // input staging for pps_forward_nchw / _bgr
  Buf amax;                         // per-tensor max |x| (PpsModel::slot), zeroed per forward
  std::vector<char> amax_need;      // slots this forward reports (set by forward_range)
  // set by pps_model_reserve: a graph captured afterwards may hold these
  // buffers' addresses, so they are never reallocated until pps_model_release
  bool pinned = false;
};

inline float* fbuf(const Workspace& w, const std::string& name) {
  return w.bufs.at(name)->as<float>();
}
inline float* slot_at(const Workspace& w, int slot) {
  return w.amax->as<float>() + (size_t)slot * PPS_AMAX_SLOT_FLOATS;
}

}  // namespace pps
#pragma GCC visibility pop

struct PpsModel {
  PpsModelConfig cfg;
  pps::Plan plan;
  std::vector<pps::Layer> layers;
  std::vector<std::pair<int, int>> edges;  // plane-eligible (producer, consumer) layer indices
  std::set<std::string> plane_capable;     // outputs of edge producers
  bool x3 = true, fused_stem = false, fused_pps = false, act_planes = false;
  std::map<std::string, int> slot;         // activation tensor -> its max |x| slot
  // every producer reports its maximum (autotune: any layer may try an f16x2
  // tile; env PPS_AMAX_ALL=1), else only the inputs of PPS_TILE_H2 layers
  mutable bool amax_all = false;
  mutable std::map<int, pps::Workspace> ws;
  mutable std::vector<std::string> names;  // storage for pps_model_layer_info
};

#pragma GCC visibility push(hidden)
namespace pps {

// A tensor's activation-max slot in this forward: its producer reports
// max |y| there and the f16x2 layers that read it scale by it.  Null when the
// tensor has no slot or no layer of this forward needs it.
inline float* slot_ptr(const PpsModel& m, const Workspace& w, const std::string& tensor) {
  const auto it = m.slot.find(tensor);
  return it == m.slot.end() || it->second >= (int)w.amax_need.size() || !w.amax_need[it->second]
             ? nullptr
             : slot_at(w, it->second);
}

// ---- model_compile.hip ----------------------------------------------------------
// The model of a checked config: plan, packed / split weights, fused launches,
// plane edges, slots and seam pairs.  Throws ModelError on a bad blob table.
std::unique_ptr<PpsModel> build_model(const PpsBlob* blobs, int nblobs, const PpsModelConfig& c);

// ---- model_run.hip ----------------------------------------------------------------
int count_readers(const PpsModel& m, const std::string& blob, bool all_keys);
Shapes infer_shapes(const PpsModel& m, int N);
std::vector<int> pps_tiles(const Layer& L, const Shape& conv_shape);
bool tunable(const Layer& L);
double layer_flops(const Layer& L, const Shapes& s, int N);
double layer_bytes(const PpsModel& m, const Layer& L, const Shapes& s, int N);
bool capturing(hipStream_t st);
Workspace& workspace(const PpsModel& m, int N, hipStream_t st, bool allow_alloc);
float* nhwc4_buffer(const PpsModel& m, Workspace& w, hipStream_t st);
// structure only; planes and split-K are checked when the layer runs
bool seam_ok(const PpsModel& m, const Layer& L);
bool h2_tile_ok(const Layer& L, int tile);
int h2e_producer(const PpsModel& m, const Layer& C);
bool fix_tile(int tile);
void run_layer(const PpsModel& m, const Layer& L, Workspace& w, const float* x, float* feat,
               bool last, int tile, int sk, hipStream_t st);
void forward_range(const PpsModel& m, const float* x, int N, float* feat, int first, int last,
                   hipStream_t st, bool keep_amax = false,
                   const std::function<void(float*)>* pre = nullptr);

// ---- model_tune.hip ---------------------------------------------------------------
void autotune(PpsModel& m, const float* x, int N, int flags, hipStream_t st);

}  // namespace pps
#pragma GCC visibility pop
