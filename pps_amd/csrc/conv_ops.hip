// Op-level conv / GEMM implementations behind the pps_conv2d_* and
// pps_gemm_splitk_batched* entry points (abi.hip) and the whole-network plan
// (model_run.hip): validate ENFORCE-style, fill the launch parameters, enqueue.
#include <string>

#include "pps_internal.hpp"

namespace pps {

int splitk_conv_epilogue(const float*, int, int64_t, int, const float*, const float*,
                         const float*, int, float*, uint16_t*, int64_t, hipStream_t, float*);

// bf16 weight planes as the B operand: [planes][Cout][K], or chunk-tiled
// [planes][Cout16 / 16][K / 32][16][32] (Cout16 = Cout rounded up to 16)
static void set_plane_weights(GemmParams& p, const void* w, int Cout, int K, bool tiled) {
  p.b3 = static_cast<const uint16_t*>(w);
  p.b_plane = (int64_t)(tiled ? (Cout + 15) / 16 * 16 : Cout) * K;
  p.b_bytes = (uint32_t)(p.b_plane * 2);
  p.tiled = tiled ? 2 : 0;
}

// weights either f32 [Cout][Kpad] (x3 = 0) or bf16x3 planes [3][Cout][Kpad]
// x_pl / y_pl: bf16x3 activation planes (plane strides in elements) instead of
// f32 x / y -- gemm_x3p.hip tiles only
// y_h2: the output as f16x2 planes on the scale of the bound
// h2o_bw * max|x| + h2o_bb (EPI_F_H2OUT; the bound goes to amax_out)
int conv_impl(const ConvArgs& a) {
  PPS_ENFORCE((a.x != nullptr) != (a.x_pl != nullptr) &&
                  (int)(a.y != nullptr) + (int)(a.y_pl != nullptr) + (int)(a.y_h2 != nullptr) == 1,
              "exactly one of x / x planes and one of y / y planes / y f16x2 planes must be given");
  const int N = a.N, H = a.H, W = a.W, Cin = a.Cin, ldx = a.ldx, Cout = a.Cout, Kpad = a.Kpad;
  const int KH = a.KH, KW = a.KW, Ho = a.Ho, Wo = a.Wo, ldy = a.ldy, splitk = a.splitk;
  if (a.y_h2) {
    PPS_ENFORCE(a.relu && !a.residual && splitk == 1 && a.h2o_in && a.amax_out && a.x3 &&
                    a.y_h2_plane >= (int64_t)N * Ho * Wo * ldy && Cin % 32 == 0 &&
                    Kpad == KH * KW * Cin && a.h2o_bw >= 0.f && a.h2o_bb >= 0.f,
                "f16x2 planes out: conv + BN + ReLU (no residual, no split-K), Cin % 32 == 0, "
                "the input's slot, an output slot, a plane stride >= N*Ho*Wo*ldy");
  }
  // PPS_TILE_B_TILED or-ed into tile: the bf16x3 weights are chunk-tiled;
  // PPS_TILE_COL_ORDER: column-major tile order
  const bool wtiled = a.tile > 0 && (a.tile & PPS_TILE_B_TILED) != 0;
  const bool colmajor = a.tile > 0 && (a.tile & PPS_TILE_COL_ORDER) != 0;
  const int tile = a.tile & ~(PPS_TILE_B_TILED | PPS_TILE_COL_ORDER);
  if (wtiled) {
    PPS_ENFORCE(a.x3 && (splitk == 1 || a.fix_cnt), "tiled weights: bf16x3 weights, no two-pass split-K");
    PPS_ENFORCE(Kpad % 32 == 0 && Cin % 32 == 0, "tiled weights need Cin % 32 == 0");
    PPS_ENFORCE(tile_dma_staged(tile), "tiled weights need a pipelined tile (29..53, 55+)");
  }
  if (a.x_pl || a.y_pl) {
    PPS_ENFORCE(a.x3, "activation planes need the bf16x3 weights");
    // (54 and 56+ pass: launch_gemm_x3 runs them on tile 38)
    PPS_ENFORCE(tile == 0 || tile_lands_pipelined(tile),
                "activation planes need a pipelined tile (0 or >= " +
                    std::to_string((int)GEMM_TILE_P_FIRST) + ")");
    PPS_ENFORCE(!a.x_pl || a.x_plane >= (int64_t)N * H * W * ldx, "x plane stride too small");
    PPS_ENFORCE(!a.y_pl || a.y_plane >= (int64_t)N * Ho * Wo * ldy, "y plane stride too small");
  }
  // whichever form the input / output takes: its base address
  const void* xin = a.x_pl ? (const void*)a.x_pl : (const void*)a.x;
  const void* yout = a.y_h2 ? (const void*)a.y_h2 : a.y_pl ? (const void*)a.y_pl : (const void*)a.y;
  PPS_ENFORCE(xin && a.w && a.scale && a.shift && yout, "null pointer");
  PPS_ENFORCE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "bad shape");
  PPS_ENFORCE(Cin % 4 == 0 && ldx % 4 == 0 && ldx >= Cin,
              "input channels must be a multiple of 4 (pad NHWC), got " +
                  std::to_string(Cin));
  PPS_ENFORCE(Kpad % 16 == 0 && Kpad >= KH * KW * Cin, "Kpad must be >= KH*KW*Cin, %16");
  PPS_ENFORCE(a.stride >= 1 && a.dil >= 1 && a.pad >= 0, "bad stride/pad/dilation");
  PPS_ENFORCE(Ho == (H + 2 * a.pad - a.dil * (KH - 1) - 1) / a.stride + 1 &&
                  Wo == (W + 2 * a.pad - a.dil * (KW - 1) - 1) / a.stride + 1,
              "output size does not match conv arithmetic");
  PPS_ENFORCE(ldy >= Cout, "ldy < Cout");
  PPS_ENFORCE(aligned16(xin) && aligned16(a.w), "x/w must be 16-byte aligned");
  PPS_ENFORCE((int64_t)N * Ho * Wo < (1ll << 31), "too many output pixels");
  GemmParams p{};
  p.splitk = 1;
  PPS_ENFORCE(KH * KW <= 64, "at most 64 filter taps");
  PPS_ENFORCE(Cin >= 16 || ((Cin & (Cin - 1)) == 0 && Kpad <= 64 * Cin),
              "channels < 16 must be a power of two with Kpad <= 64*Cin");
  PPS_ENFORCE((int64_t)N * H * W * ldx * 4 < kMaxBufBytes, "input larger than 2 GiB");
  PPS_ENFORCE((int64_t)Cout * Kpad * 6 < kMaxBufBytes, "weights larger than 2 GiB");
  p.a = a.x; p.H = H; p.W = W; p.Cin = Cin; p.lda = ldx;
  p.a_bytes = (uint32_t)((int64_t)N * H * W * ldx * 4);
  if (a.x_pl) {
    p.a3 = a.x_pl; p.a_plane = a.x_plane;
    p.a_bytes = (uint32_t)((int64_t)N * H * W * ldx * 2);
  }
  p.b_bytes = (uint32_t)((int64_t)Cout * Kpad * 4);
  p.KH = KH; p.KW = KW; p.stride = a.stride; p.pad = a.pad; p.dil = a.dil;
  p.Ho = Ho; p.Wo = Wo; p.M = N * Ho * Wo;
  p.ldb = Kpad; p.kb_valid = Kpad; p.Ncol = Cout; p.Kloop = Kpad;
  p.scale = a.scale; p.shift = a.shift; p.residual = a.residual; p.ldr = ldy;
  p.out = a.y; p.ldo = ldy; p.relu = a.relu; p.tile = tile;
  p.colmajor = colmajor ? 1 : 0;
  p.amax_out = a.amax_out;
  int h2o = 0;
  if (a.y_h2) {
    p.out3 = a.y_h2; p.out_plane = a.y_h2_plane;
    p.h2o_in = a.h2o_in; p.h2o_bw = a.h2o_bw; p.h2o_bb = a.h2o_bb;
    h2o = EPI_F_H2OUT;
  }
  if (a.w_rs) {
    // f16x2 (pps_conv2d_bn_act_h2, the whole-network plan's PPS_TILE_H2):
    // f32 activations scaled by their tensor's max, chunk-tiled two-plane
    // weights [2][Cout16 / 16][Kpad / 32][16][32] with per-channel scales
    // x_pl: f16x2 activation planes [2][x_plane] (pps_split_f16x2_act of x
    // with the same max): same bits as the f32 input, no split in the loop
    PPS_ENFORCE(!a.y_pl && splitk == 1, "f16x2 conv: f32 output, no split-K");
    PPS_ENFORCE(a.amax_in != nullptr, "f16x2 conv: the input tensor's max (amax_x) is required");
    PPS_ENFORCE(Cin % 32 == 0 && Kpad == KH * KW * Cin,
                "f16x2 conv: Cin % 32 == 0 and Kpad == KH*KW*Cin");
    PPS_ENFORCE(tile == 0 || tile_rounds_16(tile),
                "f16x2 conv: tile 0 or 38..60 (54: the weight-stationary 1x1 where it "
                "applies, else 38)");
    set_plane_weights(p, a.w, Cout, Kpad, true);
    p.rs_b = a.w_rs;
    p.amax_a = a.amax_in;
    return launch_gemm_x3(p, EPI_CONV | EPI_F_H2 | h2o, 1, as_stream(a.stream));
  }
  if (splitk > 1) {
    // conv split-K: raw partial sums of K slices [splitk][M][Cout] on the
    // pipelined kernel, then one pass that sums them in slice order and
    // applies BN [+ residual] [ReLU] (f32 or bf16x3-plane output)
    PPS_ENFORCE(a.x3 && a.part, "split-K needs the bf16x3 weights and a partials buffer");
    PPS_ENFORCE(Cin % 32 == 0 && Kpad % (32 * splitk) == 0 && Kpad == KH * KW * Cin,
                "split-K needs Cin % 32 == 0 and Kpad % (32 * splitk) == 0");
    PPS_ENFORCE(ldy == Cout && Cout % 4 == 0 && aligned16(a.part), "split-K: dense output");
    PPS_ENFORCE(tile == 0 || tile_lands_pipelined(tile), "split-K needs a pipelined tile");
    const int64_t M = (int64_t)N * Ho * Wo;
    p.splitk = splitk; p.ksplit_conv = 1;
    p.Kloop = Kpad / splitk; p.kb_valid = p.Kloop;
    set_plane_weights(p, a.w, Cout, Kpad, wtiled);  // (tiled: the one-launch form only)
    // tile 0: the same default for both forms (same rounding group, so they
    // give the same bits at tile 0 as at any equal id)
    p.tile = tile ? tile : kDefaultFixTile;
    if (a.fix_cnt) {
      // one launch: the last K slice of each tile to finish sums the parked
      // partials (slice order) and runs BN [+ residual] + ReLU [-> planes]
      PPS_ENFORCE(a.relu, "one-launch split-K: conv + BN + ReLU epilogues only");
      PPS_ENFORCE(!(a.residual && a.y_pl), "one-launch split-K: residual with f32 output only");
      const int bm = x3p_tile_rows(p.tile, a.x_pl != nullptr);
      const int bn = x3p_tile_cols(p.tile, a.x_pl != nullptr);
      PPS_ENFORCE(bm > 0 && bn > 0, "one-launch split-K needs a pipelined tile");
      const int64_t ntile = ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn);
      PPS_ENFORCE(a.n_cnt >= ntile, "one-launch split-K: " + std::to_string(ntile) +
                                        " tile counters needed, " + std::to_string(a.n_cnt) + " given");
      p.part = a.part; p.part_sstride = M * Cout; p.fix_cnt = a.fix_cnt;
      p.out_sstride = 0;
      if (a.y_pl) { p.out3 = a.y_pl; p.out_plane = a.y_plane; }
      return launch_gemm_x3(p, (a.y_pl ? EPI_CONV | EPI_F_PLANES : EPI_CONV) | EPI_F_FIX, 1,
                            as_stream(a.stream));
    }
    p.out = a.part; p.out3 = nullptr; p.ldo = Cout; p.out_sstride = M * Cout;
    p.residual = nullptr; p.relu = 0;
    const int rc = launch_gemm_x3(p, EPI_CONV | EPI_F_RAW, 1, as_stream(a.stream));
    if (rc != PPS_OK) return rc;
    return splitk_conv_epilogue(a.part, splitk, M, Cout, a.scale, a.shift, a.residual, a.relu,
                                a.y, a.y_pl, a.y_plane, as_stream(a.stream), a.amax_out);
  }
  if (a.y_pl) { p.out3 = a.y_pl; p.out_plane = a.y_plane; }
  if (a.x3) {
    set_plane_weights(p, a.w, Cout, Kpad, wtiled);
    PPS_ENFORCE(!h2o || !a.x_pl, "f16x2 planes out from a bf16x3 conv: f32 activations in");
    return launch_gemm_x3(p, (a.y_pl ? EPI_CONV | EPI_F_PLANES : EPI_CONV) | h2o, 1,
                          as_stream(a.stream));
  }
  p.b = static_cast<const float*>(a.w);
  return launch_gemm(p, EPI_CONV, 1, as_stream(a.stream));
}

// The last res5 conv with the part pooling fused into its epilogue
// (ResNet.py:276-333 res5_2 branch2c + Sum + Relu, then bpm_heads.py:18-55 /
// pps_heads.py:38-80): conv + BN + residual + ReLU on a pipelined tile whose
// rows are exactly one image (Ho * Wo); each tile pools its image's strips
// and writes the 2^S - 1 part subsets into pps_out [2^S - 1][N][Cout] as
// pps_part_power_set does (same bits).  y (the conv output) may be null: it
// is then never written.
int conv_pps_impl(const ConvArgs& a) {
  const int N = a.N, H = a.H, W = a.W, Cin = a.Cin, ldx = a.ldx, Cout = a.Cout, Kpad = a.Kpad;
  const int KH = a.KH, KW = a.KW, Ho = a.Ho, Wo = a.Wo, S = a.S;
  PPS_ENFORCE((a.x != nullptr) != (a.x_pl != nullptr), "exactly one of x / x planes must be given");
  PPS_ENFORCE(a.w && a.scale && a.shift && a.residual && a.pps_out && a.splits, "null pointer");
  PPS_ENFORCE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cout % 4 == 0, "bad shape");
  PPS_ENFORCE(Cin % 32 == 0 && ldx % 8 == 0 && ldx >= Cin && Kpad == KH * KW * Cin,
              "pipelined conv: Cin % 32 == 0, Kpad == KH*KW*Cin");
  PPS_ENFORCE(KH * KW <= 64 && a.stride >= 1 && a.dil >= 1 && a.pad >= 0, "bad filter");
  PPS_ENFORCE(Ho == (H + 2 * a.pad - a.dil * (KH - 1) - 1) / a.stride + 1 &&
                  Wo == (W + 2 * a.pad - a.dil * (KW - 1) - 1) / a.stride + 1,
              "output size does not match conv arithmetic");
  PPS_ENFORCE(S >= 1 && S <= kPpsFuseMaxStrips, "1..10 strips");
  int hsum = 0;
  for (int j = 0; j < S; ++j) {
    PPS_ENFORCE(a.splits[j] > 0, "strip heights must be positive");
    hsum += a.splits[j];
  }
  PPS_ENFORCE(hsum == Ho, "strip heights must sum to the output height");
  const bool pl = a.x_pl != nullptr;
  // chunk-tiled weights (always for f16x2: two planes, per-channel scales)
  const bool wtiled = a.w_rs != nullptr || (a.tile > 0 && (a.tile & PPS_TILE_B_TILED) != 0);
  PPS_ENFORCE(!a.w_rs || a.amax_in, "f16x2: the activations' max is required");
  const bool colmajor = a.tile > 0 && (a.tile & PPS_TILE_COL_ORDER) != 0;
  int tile = a.tile & ~(PPS_TILE_B_TILED | PPS_TILE_COL_ORDER);
  if (tile == 0) tile = pl ? GEMM_TILE_P16_FIRST + 1 : GEMM_TILE_P16_192x128W42;
  PPS_ENFORCE(!a.w_rs || tile >= GEMM_TILE_P16_FIRST, "f16x2: a 16x16x32 tile (38+)");
  // the pooling epilogue takes one image per tile: the rows the launch will
  // instantiate (the same table row) must be exactly the image
  PPS_ENFORCE(x3p_tile_rows(tile, pl) == Ho * Wo && x3p_tile_cols(tile, pl) <= kPpsFuseMaxCols,
              "the fused pooling needs a pipelined tile of exactly Ho*Wo = " +
                  std::to_string(Ho * Wo) + " rows and <= 256 columns, tile " +
                  std::to_string(tile) + " has " + std::to_string(x3p_tile_rows(tile, pl)));
  PPS_ENFORCE((int64_t)N * H * W * ldx * (pl ? 2 : 4) < kMaxBufBytes, "input larger than 2 GiB");
  PPS_ENFORCE((int64_t)(1 << S) * N * Cout < (1ll << 31), "part output too large");
  PPS_ENFORCE(aligned16(pl ? (const void*)a.x_pl : (const void*)a.x) && aligned16(a.w) &&
                  aligned16(a.scale) && aligned16(a.shift) && aligned16(a.residual) &&
                  (!a.y || aligned16(a.y)),
              "16-byte aligned pointers");
  PPS_ENFORCE(!pl || a.x_plane >= (int64_t)N * H * W * ldx, "x plane stride too small");
  GemmParams p{};
  p.splitk = 1;
  p.a = a.x; p.H = H; p.W = W; p.Cin = Cin; p.lda = ldx;
  p.a_bytes = (uint32_t)((int64_t)N * H * W * ldx * (pl ? 2 : 4));
  if (pl) { p.a3 = a.x_pl; p.a_plane = a.x_plane; }
  p.KH = KH; p.KW = KW; p.stride = a.stride; p.pad = a.pad; p.dil = a.dil;
  p.Ho = Ho; p.Wo = Wo; p.M = N * Ho * Wo;
  p.ldb = Kpad; p.kb_valid = Kpad; p.Ncol = Cout; p.Kloop = Kpad;
  set_plane_weights(p, a.w, Cout, Kpad, wtiled);
  p.colmajor = colmajor ? 1 : 0;
  p.scale = a.scale; p.shift = a.shift; p.residual = a.residual; p.ldr = Cout;
  p.out = a.y; p.ldo = Cout; p.relu = 1; p.tile = tile;
  p.pps_out = a.pps_out; p.pps_S = S; p.pps_max_ave = a.max_ave ? 1 : 0; p.pps_nimg = N;
  p.pps_write_y = a.y ? 1 : 0;
  for (int j = 0; j < S; ++j) p.pps_h[j] = a.splits[j];
  PPS_ENFORCE(x3p_eligible(p, EPI_CONV | EPI_F_RES | EPI_F_RELU), "shape not eligible for the pipelined GEMM");
  const int h2 = a.w_rs ? EPI_F_H2 : 0;
  p.rs_b = a.w_rs;
  p.amax_a = a.amax_in;
  return launch_gemm_x3p(p, EPI_CONV | EPI_F_RES | EPI_F_RELU | EPI_F_PPS | h2, 1,
                         as_stream(a.stream), tile);
}

// conv (x, weights' first Kpad columns) + 1x1 / stride2 shortcut conv (x2, the
// next Kpad2 columns) in one GEMM, BN folded into the weights: shift [+ ReLU]
int dual_impl(const DualArgs& a) {
  const int N = a.N, H = a.H, W = a.W, Cin = a.Cin, ldx = a.ldx, Cout = a.Cout;
  const int KH = a.KH, KW = a.KW, Ho = a.Ho, Wo = a.Wo, H2 = a.H2, W2 = a.W2, Cin2 = a.Cin2;
  const int ldx2 = a.ldx2, Kpad1 = a.Kpad, Kpad2 = a.Kpad2;
  PPS_ENFORCE(a.x && a.x2 && a.w && a.shift && a.y, "null pointer");
  PPS_ENFORCE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin2 > 0, "bad shape");
  const bool wtiled = a.tile > 0 && (a.tile & PPS_TILE_B_TILED) != 0;  // chunk-tiled weights
  const bool colmajor = a.tile > 0 && (a.tile & PPS_TILE_COL_ORDER) != 0;
  const int tile = a.tile & ~(PPS_TILE_B_TILED | PPS_TILE_COL_ORDER);
  if (wtiled)
    PPS_ENFORCE(a.x3 && (Kpad1 + Kpad2) % 32 == 0 && tile_dma_staged(tile),
                "tiled weights: bf16x3, K % 32 == 0, a pipelined tile");
  PPS_ENFORCE(Cin % 4 == 0 && ldx % 4 == 0 && Cin2 % 16 == 0 && ldx2 % 4 == 0,
              "channel counts must be multiples of 4 (second operand: 16)");
  PPS_ENFORCE(Kpad1 % 16 == 0 && Kpad1 >= KH * KW * Cin && Kpad2 == Cin2,
              "Kpad1 >= KH*KW*Cin (%16), Kpad2 == Cin2");
  PPS_ENFORCE(KH * KW <= 64, "at most 64 filter taps");
  PPS_ENFORCE(Ho == (H + 2 * a.pad - (KH - 1) - 1) / a.stride + 1 &&
                  Wo == (W + 2 * a.pad - (KW - 1) - 1) / a.stride + 1,
              "output size does not match conv arithmetic");
  PPS_ENFORCE(Ho == (H2 - 1) / a.stride2 + 1 && Wo == (W2 - 1) / a.stride2 + 1,
              "second operand (1x1, stride2) does not map onto the output grid");
  PPS_ENFORCE((int64_t)N * H * W * ldx * 4 < kMaxBufBytes &&
                  (int64_t)N * H2 * W2 * ldx2 * 4 < kMaxBufBytes,
              "input larger than 2 GiB");
  PPS_ENFORCE(aligned16(a.x) && aligned16(a.x2) && aligned16(a.w), "16-byte alignment");
  GemmParams p{};
  p.splitk = 1;
  p.a = a.x; p.H = H; p.W = W; p.Cin = Cin; p.lda = ldx;
  p.a_bytes = (uint32_t)((int64_t)N * H * W * ldx * 4);
  p.KH = KH; p.KW = KW; p.stride = a.stride; p.pad = a.pad; p.dil = 1;
  p.Ho = Ho; p.Wo = Wo; p.M = N * Ho * Wo;
  p.a2 = a.x2; p.a2_bytes = (uint32_t)((int64_t)N * H2 * W2 * ldx2 * 4);
  p.H2 = H2; p.W2 = W2; p.lda2 = ldx2; p.stride2 = a.stride2; p.Kloop1 = Kpad1;
  p.ldb = Kpad1 + Kpad2; p.kb_valid = Kpad1 + Kpad2; p.Ncol = Cout;
  p.Kloop = Kpad1 + Kpad2;
  p.scale = nullptr; p.shift = a.shift; p.out = a.y; p.ldo = a.ldy; p.relu = a.relu; p.tile = tile;
  p.colmajor = colmajor ? 1 : 0;
  PPS_ENFORCE((int64_t)Cout * (Kpad1 + Kpad2) * 6 < kMaxBufBytes, "weights larger than 2 GiB");
  p.amax_out = a.amax_out;
  if (a.w_rs) {  // f16x2: both operands share their maxima's scale (conv_impl)
    PPS_ENFORCE(a.amax_in && a.amax_in2, "f16x2 conv: both inputs' maxima are required");
    PPS_ENFORCE(Cin % 32 == 0 && Kpad1 == KH * KW * Cin && Kpad2 % 32 == 0,
                "f16x2 conv: Cin % 32 == 0, Kpad1 == KH*KW*Cin, Cin2 % 32 == 0");
    // (the patch tiles have no fused-shortcut epilogue)
    PPS_ENFORCE(tile == 0 || (tile_rounds_16(tile) && tile_kind(tile) != TileKind::Patch),
                "f16x2 fused-shortcut conv: tile 0, 38..55 or 60");
    set_plane_weights(p, a.w, Cout, Kpad1 + Kpad2, true);
    p.rs_b = a.w_rs;
    p.amax_a = a.amax_in;
    p.amax_a2 = a.amax_in2;
    return launch_gemm_x3(p, EPI_CONV | EPI_F_H2, 1, as_stream(a.stream));
  }
  if (a.x3) {
    set_plane_weights(p, a.w, Cout, Kpad1 + Kpad2, wtiled);
    return launch_gemm_x3(p, EPI_CONV, 1, as_stream(a.stream));
  }
  p.b = static_cast<const float*>(a.w);
  p.b_bytes = (uint32_t)((int64_t)Cout * (Kpad1 + Kpad2) * 4);
  return launch_gemm(p, EPI_CONV, 1, as_stream(a.stream));
}

// raw partial sums of the K slices of B batched GEMMs (the heads), f32 or
// bf16x3 weights
int splitk_impl(const float* x, int M, int K, const void* w, int x3, int Cout, int B, int splitk,
                float* part, int tile, void* stream) {
  PPS_ENFORCE(x && w && part, "null pointer");
  PPS_ENFORCE(M > 0 && K > 0 && Cout > 0 && B > 0 && splitk >= 1, "bad shape");
  PPS_ENFORCE(K % (16 * splitk) == 0, "K must be a multiple of 16*splitk");
  PPS_ENFORCE((int64_t)M * K * 4 < kMaxBufBytes && (int64_t)Cout * K * 4 < kMaxBufBytes,
              "operands larger than 2 GiB");
  PPS_ENFORCE(aligned16(x) && aligned16(w), "x/w must be 16-byte aligned");
  GemmParams p{};
  p.splitk = splitk;
  p.a = x; p.a_bstride = (int64_t)M * K; p.H = 1; p.W = M; p.Cin = K / splitk; p.lda = K;
  p.a_bytes = (uint32_t)((int64_t)M * K * 4);
  p.KH = p.KW = 1; p.stride = 1; p.dil = 1; p.Ho = 1; p.Wo = M; p.M = M;
  p.ldb = K; p.kb_valid = K / splitk; p.Ncol = Cout;
  p.Kloop = K / splitk;
  p.out = part; p.ldo = (int64_t)B * Cout; p.out_bstride = Cout;
  p.out_sstride = (int64_t)M * B * Cout; p.tile = tile;
  if (x3) {
    PPS_ENFORCE((int64_t)Cout * K * 6 < kMaxBufBytes, "weights larger than 2 GiB");
    p.b3 = static_cast<const uint16_t*>(w); p.b_plane = (int64_t)Cout * K;
    p.b_bstride = 3 * p.b_plane; p.b_bytes = (uint32_t)(p.b_plane * 2);
    return launch_gemm_x3(p, EPI_CONV | EPI_F_RAW, B, as_stream(stream));
  }
  p.b = static_cast<const float*>(w); p.b_bstride = (int64_t)Cout * K;
  p.b_bytes = (uint32_t)((int64_t)Cout * K * 4);
  return launch_gemm(p, EPI_CONV | EPI_F_RAW, B, as_stream(stream));
}

}  // namespace pps
