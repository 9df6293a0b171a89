// GEMM tile ids (the `tile` argument of the C ABI), their classes, and the one
// table of the LDS-DMA pipelined (gemm_x3p.hip) and patch-staged (gemm_x3c.hip)
// tiles: shapes, one-launch split-K capability and the launched template
// arguments all come from these rows.
#pragma once

namespace pps {

enum GemmTile {
  GEMM_TILE_AUTO = 0,
  GEMM_TILE_128x128 = 1,
  GEMM_TILE_128x64 = 2,
  GEMM_TILE_64x128 = 3,
  GEMM_TILE_64x64 = 4,
  GEMM_TILE_256x128 = 5,
  GEMM_TILE_128x128_K32 = 6,  // same shapes with a 32-wide K chunk per barrier
  GEMM_TILE_128x64_K32 = 7,
  GEMM_TILE_64x128_K32 = 8,
  GEMM_TILE_64x64_K32 = 9,
  GEMM_TILE_256x128_K32 = 10,
  // 11..20: ids 1..10 with the bf16x3 kernel's A operand kept f32 in LDS
  // 21..28 (bf16x3 kernel): 192x128 K16, 192x64 K16, 192x128 K32, 192x64 K32,
  // then the same four with A kept f32 in LDS
  GEMM_TILE_192_FIRST = 21,
  // 29..35 (bf16x3 only): LDS-DMA pipelined kernel (gemm_x3p.hip), K chunk 32:
  // 128x128, 192x128, 128x64, 192x64 (4 waves, 3 stages), 256x128, 128x256,
  // 192x256 (8 waves, 2 stages)
  GEMM_TILE_P_FIRST = 29,
  // 36, 37: 128x128 and 192x128 with 8 waves
  // 38..46 (bf16x3 only): ids 29..37 on 16x16x32 MFMA blocks (own rounding)
  GEMM_TILE_P16_FIRST = 38,
  // 45: 128x128 with 8 waves, the split-K convs' default (tile 0)
  GEMM_TILE_P16_128x128W42 = 45,
  // 47 (bf16x3 only, 16x16x32 rounding): 192x128 with 8 waves as 4 x 2 (48 x 64
  // per wave) -- 256 tiles for the res5 layers' M = 12,288 x N = 512
  GEMM_TILE_P16_192x128W42 = 47,
  // 48, 49 (16x16x32): 192x64 (4 x 1 waves) and 96x128 (2 x 2 waves), 48 x 64
  // per wave -- 256 tiles for M = 12,288 x N = 256 (res4 2a / 2b)
  GEMM_TILE_P16_192x64W41 = 48,
  GEMM_TILE_P16_96x128W22 = 49,
  // 50 (16x16x32): 96x128 with 8 waves as 2 x 4 (48 x 32 per wave)
  GEMM_TILE_P16_96x128W24 = 50,
  // 51, 52 (16x16x32): 128x128 and 192x128 with 8 waves as 4 x 2 and three
  // LDS stages (192x128 with plane activations: two)
  GEMM_TILE_P16_128x128W42S3 = 51,
  GEMM_TILE_P16_192x128W42S3 = 52,
  // 53 (16x16x32): 96x128 with 8 waves as 2 x 4 and three LDS stages
  GEMM_TILE_P16_96x128W24S3 = 53,
  // 54 (16x16x32 rounding): weight-stationary persistent kernel
  // (gemm_ws.hip) for 1x1 convs with K = 64 / 128 / 256; other shapes run
  // tile 38
  GEMM_TILE_WS = 54,
  // 55 (16x16x32): 64x128 with 8 waves as 2 x 4 and four LDS stages -- short
  // M (the 64-row head GEMMs: 248 split-K workgroups, three chunks in flight)
  GEMM_TILE_P16_64x128W24S4 = 55,
  // 56..59 (16x16x32, own rounding group: K in (channel chunk, tap) order):
  // patch-staged stride-1 3x3 convs (gemm_x3c.hip) -- 192x128 (8 waves), 192x64 (4 waves), 96x128 (8 waves),
  // 192x64 (8 waves); other shapes run tile 38
  GEMM_TILE_C16_FIRST = 56,
  GEMM_TILE_C16_192x128 = 56,
  GEMM_TILE_C16_192x64 = 57,
  GEMM_TILE_C16_96x128 = 58,
  GEMM_TILE_C16_192x64W42 = 59,  // 192x64 with 8 waves (4 x 2)
  // pipelined 16x16x32, 192x128 as 4 x 1 waves: f16x2 only (bf16x3 runs 47)
  GEMM_TILE_P16_192x128W41 = 60,
  GEMM_NUM_TILES = 61
};

// The kernel family an id names.
enum class TileKind {
  None,    // 0 (heuristic), negative, or past the table
  Staged,  // 1..28: register-staged (gemm_f32.hip / gemm_x3.hip)
  P32,     // 29..37: pipelined, 32x32x16 MFMA blocks
  P16,     // 38..53, 55, 60: pipelined, 16x16x32 MFMA blocks
  WS,      // 54: weight-stationary 1x1
  Patch    // 56..59: patch-staged 3x3
};
constexpr TileKind tile_kind(int t) {
  if (t < GEMM_TILE_128x128 || t >= GEMM_NUM_TILES) return TileKind::None;
  if (t < GEMM_TILE_P_FIRST) return TileKind::Staged;
  if (t < GEMM_TILE_P16_FIRST) return TileKind::P32;
  if (t == GEMM_TILE_WS) return TileKind::WS;
  if (t >= GEMM_TILE_C16_FIRST && t <= GEMM_TILE_C16_192x64W42) return TileKind::Patch;
  return TileKind::P16;
}
// A pipelined tile the bf16x3 arithmetic is built for (60 is f16x2 only; the
// bf16x3 launches of it are rerouted to 47 before any such check): 29..53, 55.
constexpr bool tile_pipelined_x3(int t) {
  return (tile_kind(t) == TileKind::P32 || tile_kind(t) == TileKind::P16) &&
         t != GEMM_TILE_P16_192x128W41;
}
// Tiles that stage their operands by LDS DMA -- pipelined and patch -- and so
// read chunk-tiled weights: 29..53, 55..60.
constexpr bool tile_dma_staged(int t) {
  return tile_kind(t) == TileKind::P32 || tile_kind(t) == TileKind::P16 ||
         tile_kind(t) == TileKind::Patch;
}
// The 16x16x32 rounding groups, the ids an f16x2 conv names: 38..60.
constexpr bool tile_rounds_16(int t) {
  return tile_kind(t) == TileKind::P16 || tile_kind(t) == TileKind::WS ||
         tile_kind(t) == TileKind::Patch;
}
// Ids that launch_gemm_x3 ends on a pipelined tile for: the pipelined ids, and
// 54, 56..59 and anything past the table, which fall back to tile 38 where
// their own kernel does not apply.  Everything from 29 up.
constexpr bool tile_lands_pipelined(int t) { return t > 0 && tile_kind(t) != TileKind::Staged; }
// Ids launch_gemm_x3 reroutes to tile 38 when their own kernel does not apply
constexpr bool tile_falls_to_38(int t) {
  return tile_kind(t) == TileKind::WS || tile_kind(t) == TileKind::Patch || t >= GEMM_NUM_TILES;
}

constexpr int kPpsFuseMaxStrips = 10;
constexpr int kPpsFuseMaxCols = 256;  // widest tile the fused pooling takes (two column passes)

// ---- pipelined tiles (gemm_x3p.hip) -----------------------------------------
struct X3pTile {
  int id;
  int S;               // MFMA block: 32 (32x32x16) or 16 (16x16x32)
  int BM, BN, WM, WN;  // tile rows / columns, waves along each
  int NSF, NSP;        // LDS stages with f32 / bf16-plane A operands (NSP = 0: the
                       // tile does not take plane activations)
  bool FX;             // also built with the one-launch split-K epilogues (EPI_F_FIX)
  int planes_id;       // plane activations launch this id's row instead (0: its own)
  int x3_id;           // an f16x2-only tile: bf16x3 launches run this id's row (0: none)
};
// 4-wave tiles up to 80 KB of LDS take two stages: two workgroups per CU, so
// one's epilogue overlaps the other's loads (measured 10-30 % faster than three
// stages at one workgroup per CU on every layer shape, scripts/gemm_probe.py);
// 192x128 needs 96 KB for two stages anyway.
constexpr X3pTile kX3pTiles[] = {
    // 29..37: 32x32x16 MFMA blocks (bit-identical to gemm_x3.hip)
    {29, 32, 128, 128, 2, 2, 2, 2, false, 0, 0},
    {30, 32, 192, 128, 2, 2, 3, 2, false, 0, 0},
    {31, 32, 128, 64, 2, 2, 2, 2, false, 0, 0},
    {32, 32, 192, 64, 2, 2, 2, 2, false, 0, 0},
    {33, 32, 256, 128, 4, 2, 2, 2, false, 0, 0},
    {34, 32, 128, 256, 2, 4, 2, 2, false, 0, 0},
    // 192x256 with plane A needs 168 KB for two stages: 128x256 (id 34) instead
    {35, 32, 192, 256, 2, 4, 2, 0, false, 34, 0},
    // 8-wave versions of 128x128 / 192x128 (two waves per SIMD in one workgroup;
    // 128x128 also two workgroups per CU): res3/res4 3x3 and res4 2c run
    // 6-10 % faster on them
    {36, 32, 128, 128, 4, 2, 2, 2, false, 0, 0},
    // plane A: 12 pieces of 16 rows over 8 waves (uneven, two stages)
    {37, 32, 192, 128, 2, 4, 2, 2, false, 0, 0},
    // 38..46: the same on 16x16x32 MFMA blocks (bit-identical among themselves,
    // f32-level like the others); 192x256 would need more than the 256 VGPRs
    // of an 8-wave workgroup, so 44 is a second 128x256
    {38, 16, 128, 128, 2, 2, 2, 2, false, 0, 0},
    {39, 16, 192, 128, 2, 2, 3, 2, false, 0, 0},
    {40, 16, 128, 64, 2, 2, 2, 2, false, 0, 0},
    {41, 16, 192, 64, 2, 2, 2, 2, false, 0, 0},
    {42, 16, 256, 128, 4, 2, 2, 2, false, 0, 0},
    {43, 16, 128, 256, 2, 4, 2, 2, false, 0, 0},
    {44, 16, 128, 256, 2, 4, 2, 2, false, 0, 0},
    {GEMM_TILE_P16_128x128W42, 16, 128, 128, 4, 2, 2, 2, true, 0, 0},
    {46, 16, 192, 128, 2, 4, 2, 2, false, 0, 0},
    // plane A on the 192-row 8-wave and 96-row tiles: 12 / 6 pieces of 16 rows
    // spread unevenly over the waves (two stages)
    {GEMM_TILE_P16_192x128W42, 16, 192, 128, 4, 2, 2, 2, true, 0, 0},
    {GEMM_TILE_P16_192x64W41, 16, 192, 64, 4, 1, 2, 2, true, 0, 0},
    {GEMM_TILE_P16_96x128W22, 16, 96, 128, 2, 2, 2, 2, true, 0, 0},
    // 96x128 with 8 waves as 2 x 4 (48 x 32 per wave): 256 tiles for
    // M = 12,288 x N = 256 at two waves per SIMD
    {GEMM_TILE_P16_96x128W24, 16, 96, 128, 2, 4, 2, 2, true, 0, 0},
    // three LDS stages (two chunks in flight behind the one being consumed) on
    // the 8-wave 128x128 / 192x128 tiles, for long-K GEMMs whose operands come
    // from the Infinity Cache rather than L2 (distance matrix, res5);
    // 192-row plane A keeps two stages (uneven pieces)
    {GEMM_TILE_P16_128x128W42S3, 16, 128, 128, 4, 2, 3, 3, false, 0, 0},
    {GEMM_TILE_P16_192x128W42S3, 16, 192, 128, 4, 2, 3, 2, false, 0, 0},
    // 96x128 as 2 x 4 waves with three stages (uneven pieces, per-wave waits)
    {GEMM_TILE_P16_96x128W24S3, 16, 96, 128, 2, 4, 3, 3, false, 0, 0},
    // 64x128, 8 waves as 2 x 4, four stages (three chunks in flight): the
    // 64-row split-K head GEMMs, whose 8-chunk slices are all pipeline fill
    {GEMM_TILE_P16_64x128W24S4, 16, 64, 128, 2, 4, 4, 4, false, 0, 0},
    // f16x2 only: 192x128 as 4 x 1 waves (48 x 128 per wave): each activation
    // fragment split once feeds eight 16x16 column blocks (the split is the
    // f16x2 kernels' VALU cost; 4 x 2 waves split every fragment twice and
    // feed four).  bf16x3 launches of this id run tile 47 (same rounding group).
    {GEMM_TILE_P16_192x128W41, 16, 192, 128, 4, 1, 2, 0, false, 0, GEMM_TILE_P16_192x128W42},
};
constexpr int kNumX3pTiles = sizeof(kX3pTiles) / sizeof(kX3pTiles[0]);

// Index of an id's row, -1 if the id is not a pipelined tile.
constexpr int x3p_tile_index(int tile) {
  for (int i = 0; i < kNumX3pTiles; ++i)
    if (kX3pTiles[i].id == tile) return i;
  return -1;
}
// Index of the row an id launches with f32 (a3 = false) or plane activations.
constexpr int x3p_shape_index(int tile, bool a3) {
  const int i = x3p_tile_index(tile);
  return i >= 0 && a3 && kX3pTiles[i].planes_id ? x3p_tile_index(kX3pTiles[i].planes_id) : i;
}
// Rows (BM) / columns (BN) of the tile a pipelined id launches, 0 for any other id.
constexpr int x3p_tile_rows(int tile, bool a3) {
  return x3p_shape_index(tile, a3) < 0 ? 0 : kX3pTiles[x3p_shape_index(tile, a3)].BM;
}
constexpr int x3p_tile_cols(int tile, bool a3) {
  return x3p_shape_index(tile, a3) < 0 ? 0 : kX3pTiles[x3p_shape_index(tile, a3)].BN;
}
// Whether the id's launches include the one-launch split-K epilogues.
constexpr bool x3p_tile_fix(int tile) {
  return x3p_tile_index(tile) >= 0 && kX3pTiles[x3p_tile_index(tile)].FX;
}
// Split-K convs at tile 0 (both the one-launch and the two-pass entry, so they
// give the same bits at tile 0 as at any equal id)
constexpr int kDefaultFixTile = GEMM_TILE_P16_128x128W42;

// What the guards on buffer sizes rely on (conv_impl sizes the split-K tile
// counters from a row's BM / BN; conv_pps_impl admits a tile whose BM is one image).
constexpr bool x3p_table_ok() {
  for (int id = 0; id < GEMM_NUM_TILES; ++id) {  // one row per pipelined id, none for others
    int n = 0;
    for (const X3pTile& t : kX3pTiles) n += t.id == id;
    if (n != (tile_kind(id) == TileKind::P32 || tile_kind(id) == TileKind::P16)) return false;
  }
  for (const X3pTile& t : kX3pTiles) {
    if (t.id < GEMM_TILE_P_FIRST || t.id >= GEMM_NUM_TILES) return false;
    if (tile_kind(t.id) != (t.S == 32 ? TileKind::P32 : TileKind::P16)) return false;
    if (t.FX && (t.S != 16 || t.NSP == 0)) return false;
    // a row launched in another's place launches itself and takes what it is sent
    const int pl = x3p_tile_index(t.planes_id), x3 = x3p_tile_index(t.x3_id);
    if (t.planes_id && (pl < 0 || kX3pTiles[pl].NSP == 0 || kX3pTiles[pl].S != t.S)) return false;
    if (t.x3_id && (x3 < 0 || t.FX || kX3pTiles[x3].x3_id || kX3pTiles[x3].BM != t.BM ||
                    kX3pTiles[x3].BN != t.BN))
      return false;
  }
  return true;
}
// ids[0..n): exactly the tiles of 192 rows (one 24 x 8 image) and <= kPpsFuseMaxCols columns
constexpr bool x3p_pps_tiles_are(bool a3, const int* ids, int n) {
  int k = 0;
  for (int t = 0; t < GEMM_NUM_TILES; ++t)
    if (x3p_tile_rows(t, a3) == 192 && x3p_tile_cols(t, a3) <= kPpsFuseMaxCols)
      if (k >= n || ids[k++] != t) return false;
  return k == n;
}
// (the lists of tests/test_lib_abi.py::test_pipelined_tile_shapes)
constexpr int kPpsTilesF32[] = {30, 32, 35, 37, 39, 41, 46, 47, 48, 52, 60};
constexpr int kPpsTilesPlanes[] = {30, 32, 37, 39, 41, 46, 47, 48, 52, 60};
static_assert(x3p_table_ok(), "pipelined tile table: ids 29..53, 55, 60 once each; FX rows and aliases");
static_assert(x3p_pps_tiles_are(false, kPpsTilesF32, 11) && x3p_pps_tiles_are(true, kPpsTilesPlanes, 10),
              "the fused pooling's tile set (192 rows, <= 256 columns) changed");
static_assert(x3p_tile_fix(kDefaultFixTile), "the split-K default must be a FIX tile");

// ---- patch-staged tiles (gemm_x3c.hip), 16x16x32 blocks -----------------------
struct X3cTile {
  int id;
  int BM, BN, WM, WN;
  int NSF, NSP;  // weight stages with f32 / plane activations
  int PMAX;      // patch pixels the LDS holds
};
constexpr X3cTile kX3cTiles[] = {
    // 4 x 2 waves (48 x 64 each); weights in three stages (two with plane
    // activations: 104 KB of patches)
    {GEMM_TILE_C16_192x128, 192, 128, 4, 2, 3, 2, 272},
    {GEMM_TILE_C16_192x64, 192, 64, 4, 1, 4, 4, 272},
    {GEMM_TILE_C16_96x128, 96, 128, 2, 4, 4, 4, 144},
    // 8 waves as 4 x 2 (48 x 32 each): half the weight bytes per tile of
    // tile 57's neighbours at 256+ tiles for N = 256 (res4) / 128 (res3)
    {GEMM_TILE_C16_192x64W42, 192, 64, 4, 2, 4, 4, 272},
};
constexpr int kNumX3cTiles = sizeof(kX3cTiles) / sizeof(kX3cTiles[0]);
constexpr int x3c_tile_index(int tile) {  // -1 if the id is not a patch tile
  return tile_kind(tile) == TileKind::Patch ? tile - GEMM_TILE_C16_FIRST : -1;
}
constexpr int x3c_tile_rows(int tile) {  // rows (BM) of a patch-staged tile id, 0 if none
  return x3c_tile_index(tile) < 0 ? 0 : kX3cTiles[x3c_tile_index(tile)].BM;
}
constexpr int x3c_tile_cols(int tile) {
  return x3c_tile_index(tile) < 0 ? 0 : kX3cTiles[x3c_tile_index(tile)].BN;
}
static_assert(kNumX3cTiles == 4 && kX3cTiles[0].id == 56 && kX3cTiles[1].id == 57 &&
                  kX3cTiles[2].id == 58 && kX3cTiles[3].id == 59,
              "patch tile table: ids 56..59 in order");

}  // namespace pps
