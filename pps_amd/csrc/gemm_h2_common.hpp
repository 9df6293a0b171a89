// The K loop of the f16x2 distance kernels (gemm_h2.hip, search_h2.hip): one
// BM x BN tile of dot products accumulated in f32 from the two chunk-tiled f16
// planes of each operand.  Every kernel that calls h2_kloop adds the same
// products in the same order (chunks ascending, the three MFMA terms of
// mfma_h2t), so their accumulators agree bit for bit.
#pragma once
#include <type_traits>

#include "gemm_x3p_common.hpp"

namespace pps {

#ifndef H2_ABL
#define H2_ABL 0  // probes: 1 = no DMA after the prologue, 2 = no MFMAs (timing ablations)
#endif
// A blocks multiplied after the chunk barrier by waves 0 .. NW/2 - 1 (O) and
// NW/2 .. NW - 1 (Y); -1: 2 / 4 on the three-stage tiles (Market 3368 x 15913:
// tile 6 1061 / 1067 -> 1049 / 1058 us, tiles 3 / 4 1114-1130 -> 1101-1105;
// the two-stage 256-row tiles would spill), 1 / 1 on the others
#ifndef H2_STAG_O
#define H2_STAG_O -1
#endif
#ifndef H2_STAG_Y
#define H2_STAG_Y -1
#endif
#ifndef H2_SPREAD
#define H2_SPREAD 1  // DMA pieces spread over the chunk's MFMA blocks (NS >= 3 tiles); 0: a burst after the barrier
#endif

// The three terms with the gallery fragment as the MFMA "A" operand, so the
// accumulator is transposed like the x3p kernels': lane l keeps query row
// (l & 15) and gallery columns 4 (l >> 4) + e, e = 0..3.
__device__ inline f32x4 mfma_h2t(const f16x8& a0, const f16x8& a1, const f16x8& b0,
                                 const f16x8& b1, f32x4 c) {
#if H2_ABL == 2
  asm volatile("" ::"v"(a0), "v"(a1), "v"(b0), "v"(b1));
  return c;
#endif
  c = mfma16_f16(b0, a0, c);
  c = mfma16_f16(b1, a0, c);
  c = mfma16_f16(b0, a1, c);
  return c;
}

// LDS layout of a tile: NS stages of NPIECE KiB DMA pieces (+ a spare KiB for
// the dummy pieces of uneven tiles), reused by the epilogue as the parked
// [BM][BN / HB + 4] f32 image (HB column passes).
template <int BM, int BN, int WM, int WN, int NS>
struct H2Tile {
  static constexpr int BK = 32;
  static constexpr int NW = WM * WN;
  static constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  static constexpr int ABLK = BM / 16, BBLK = BN / 16;  // 16-row blocks per plane and chunk
  static constexpr int NPIECE = 2 * (ABLK + BBLK);      // KiB DMA pieces per chunk
  // pieces per wave; uneven tiles give the last waves dummy pieces (zeros
  // into a spare KiB after the stages) so every wave's wait counts are equal
  static constexpr int PPW = (NPIECE + NW - 1) / NW;
  static constexpr bool EVEN = NPIECE % NW == 0;
  static constexpr int STAGE = NPIECE * 1024;
  static_assert(TM % 2 == 0 && TM >= 2 && TN >= 1, "wave tile");
  static_assert(NS >= 2 && NS <= 4 && NS * STAGE <= 160 * 1024, "LDS stages");
  static_assert(PPW * (NS - 1) <= 63, "vmcnt range");
  static constexpr int HB = BM * (BN + 4) * 4 <= 160 * 1024 ? 1 : 2;
  static constexpr int EPI_BYTES = BM * (BN / HB + 4) * 4;
  static_assert(EPI_BYTES <= 160 * 1024, "epilogue image");
  static constexpr int PIPE_BYTES = NS * STAGE + (EVEN ? 0 : 1024);
  static constexpr int LDS_BYTES = PIPE_BYTES > EPI_BYTES ? PIPE_BYTES : EPI_BYTES;
  static_assert(PIPE_BYTES <= 160 * 1024, "LDS stages");
};

// acc = the dot products of query rows m0 .. m0 + BM - 1 and gallery rows
// n0 .. n0 + BN - 1 (rows past the planes read as zeros).  `lds` holds
// H2Tile::PIPE_BYTES; on return every DMA of the calling wave has landed (the
// caller's next block barrier retires the other waves').
template <int BM, int BN, int WM, int WN, int NS>
__device__ __forceinline__ void h2_kloop(const GemmParams& p, unsigned char* lds, int m0, int n0,
                                         int wave, int lane, int wm, int wn,
                                         f32x4 (&acc)[BM / WM / 16][BN / WN / 16]) {
  using T = H2Tile<BM, BN, WM, WN, NS>;
  constexpr int BK = T::BK, NW = T::NW, TM = T::TM, TN = T::TN, ABLK = T::ABLK, BBLK = T::BBLK;
  constexpr int NPIECE = T::NPIECE, PPW = T::PPW, STAGE = T::STAGE;
  constexpr bool EVEN = T::EVEN;
  const int nkc = p.Kloop / BK;

  // ---- DMA pieces.  Piece q of a chunk: A plane q / ABLK, block q % ABLK
  // (q < 2 ABLK), else B; its LDS image is stage + q KiB.  Lane l fills row
  // l >> 2 of the 16-row block, physical 16-byte slot l & 3 with logical slot
  // (l & 3) ^ sw64(row) (bank-conflict swizzle on the source address).
  const rsrc_t ra = make_rsrc(p.a3, p.a_bytes);
  const rsrc_t rb = make_rsrc(p.b3, p.b_bytes);
  const int ablocks = (int)(p.a_plane / (16 * (int64_t)p.Kloop));
  const int bblocks = (int)(p.b_plane / (16 * (int64_t)p.Kloop));
  const int lr = lane >> 2;
  const int loff = lr * 64 + (((lane & 3) ^ sw64(lr)) << 4);
  int src[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int q = wave * PPW + i;
    int blk = 0, nblk = 0;
    int64_t pbase = 0;
    if (q >= NPIECE) {
      // dummy piece (uneven tiles): reads zeros
    } else if (q < 2 * ABLK) {
      const int pl = q / ABLK;
      blk = m0 / 16 + (q - pl * ABLK);
      nblk = ablocks;
      pbase = pl * p.a_plane * 2;
    } else {
      const int qq = q - 2 * ABLK;
      const int pl = qq / BBLK;
      blk = n0 / 16 + (qq - pl * BBLK);
      nblk = bblocks;
      pbase = pl * p.b_plane * 2;
    }
    // out-of-range blocks: an offset >= 2^31 > num_records reads zeros
    src[i] = blk < nblk ? (int)(pbase + (int64_t)blk * nkc * 1024 + loff) : (int)0x80000000;
  }
  // piece i of this wave for chunk kc into its stage
  auto issue_piece = [&](int kc, int stage, int i) {
    const unsigned char* st = lds + stage * STAGE;
    const int q = wave * PPW + i;
    if (EVEN || q < NPIECE)
      glds16(q < 2 * ABLK ? ra : rb, st + q * 1024, src[i] + kc * 1024);
    else
      glds16(rb, lds + NS * STAGE, (int)0x80000000);
  };
  auto issue = [&](int kc, int stage) {
    if (H2_ABL == 1 && kc >= NS) return;
#pragma unroll
    for (int i = 0; i < PPW; ++i) issue_piece(kc, stage, i);
  };

  // ---- fragments: lane l reads row l & 15 of a block, logical 16-byte slot
  // l >> 4 (K elements 8 (l >> 4) .. + 7), at its swizzled position
  const int r16 = lane & 15;
  const int foff = r16 * 64 + (((lane >> 4) ^ sw64(r16)) << 4);
  auto readA = [&](const unsigned char* st, int i, f16x8 (&f)[2]) {
    const unsigned char* a = st + (wm * (BM / WM / 16) + i) * 1024 + foff;
    f[0] = *reinterpret_cast<const f16x8*>(a);
    f[1] = *reinterpret_cast<const f16x8*>(a + ABLK * 1024);
  };
  auto readB = [&](const unsigned char* st, f16x8 (&fb)[TN][2]) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const unsigned char* b = st + (2 * ABLK + wn * (BN / WN / 16) + j) * 1024 + foff;
      fb[j][0] = *reinterpret_cast<const f16x8*>(b);
      fb[j][1] = *reinterpret_cast<const f16x8*>(b + BBLK * 1024);
    }
  };

#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Chunk c lives in stage c % NS.  The prologue requests chunks 0 .. NS-1;
  // the barrier in chunk c's tail (every wave done reading stage c % NS, and
  // chunk c + 1 landed: the NS - 2 younger chunks may stay in flight) is
  // followed by the request of chunk c + NS into the stage just freed.
  // Requests past the last chunk stay inside the operand buffers (or read
  // zeros beyond them) and are never consumed: every wait count is uniform.
#pragma unroll
  for (int c = 0; c < NS; ++c) issue(c, c);
  wait_vmcnt<PPW * (NS - 1)>();  // chunk 0 landed
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  constexpr bool SPREAD = H2_SPREAD && NS >= 3 && H2_ABL == 0;
  constexpr int SO = H2_STAG_O >= 0 ? H2_STAG_O : (NS >= 3 ? 2 : 1);
  constexpr int SY = H2_STAG_Y >= 0 ? H2_STAG_Y : (NS >= 3 ? 4 : 1);
  constexpr int DO = SO < TM ? SO : TM - 1;
  constexpr int DY = SY < TM ? SY : TM - 1;
  if constexpr (DO == 1 && DY == 1) {
    f16x8 fb0[TN][2], fb1[TN][2], fa0[2], fa1[2];
    readB(lds, fb0);
    readA(lds, 0, fa0);
    // One chunk: block i's MFMAs beside block i + 1's A reads; before the last
    // block, the barrier that retires this stage's reads and the next chunk's
    // DMA, the request two chunks ahead into this stage, and the next chunk's B
    // fragments and first A block beside the last block's MFMAs.
    int scur = 0;  // stage of chunk kc
    // SPREAD (three or more stages): chunk kc - 1 + NS goes into the stage the
    // previous chunk's barrier freed, its pieces spread over this chunk's
    // first TM - 1 blocks (an MFMA block between two DMA pieces) instead of a
    // burst right after the barrier, where both waves of a SIMD stall on
    // their DMA issue at once; all pieces are out before the chunk's wait
    auto chunk = [&](int kc, f16x8 (&fbc)[TN][2], f16x8 (&fbn)[TN][2]) {
      const unsigned char* st = lds + scur * STAGE;
      const int sprev = scur == 0 ? NS - 1 : scur - 1;
#pragma unroll
      for (int i = 0; i < TM - 1; ++i) {
        if (SPREAD && kc >= 1) {
#pragma unroll
          for (int j = i * PPW / (TM - 1); j < (i + 1) * PPW / (TM - 1); ++j)
            issue_piece(kc - 1 + NS, sprev, j);
        }
        if (i & 1) {
          readA(st, i + 1, fa0);
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = mfma_h2t(fa1[0], fa1[1], fbc[j][0], fbc[j][1], acc[i][j]);
        } else {
          readA(st, i + 1, fa1);
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = mfma_h2t(fa0[0], fa0[1], fbc[j][0], fbc[j][1], acc[i][j]);
        }
      }
      if (kc + 1 < nkc) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_vmcnt<PPW * (NS - 2)>();  // chunk kc + 1 landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (!SPREAD) issue(kc + NS, scur);
        scur = scur + 1 == NS ? 0 : scur + 1;
        const unsigned char* sn = lds + scur * STAGE;
        readB(sn, fbn);
        readA(sn, 0, fa0);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[TM - 1][j] = mfma_h2t(fa1[0], fa1[1], fbc[j][0], fbc[j][1], acc[TM - 1][j]);
    };
    int kc = 0;
    for (; kc + 1 < nkc; kc += 2) {
      chunk(kc, fb0, fb1);
      chunk(kc + 1, fb1, fb0);
    }
    if (kc < nkc) chunk(kc, fb0, fb1);
  } else {
    // One chunk, D blocks deferred: blocks 0 .. TM-1-D multiply before the
    // chunk's barrier (each beside the A read of a later block), every A block
    // of the chunk is in registers by the barrier; after it (the barrier that
    // retires this stage's reads and the next chunk's DMA), the next chunk's B
    // fragments and first A block are read beside the last D blocks' MFMAs.
    // The two halves of the workgroup run different D (H2_STAG_O for waves
    // 0 .. NW/2-1, H2_STAG_Y for the rest): the two waves of a SIMD then carry
    // different amounts of MFMA work across the barrier, so the one that
    // reaches it first leaves the matrix pipe to its partner instead of both
    // idling there together (MI355X_MICROARCH "try a stagger").
    // SPREAD (three or more stages): chunk kc - 1 + NS goes into the stage the
    // previous chunk's barrier freed, its pieces spread over this chunk's
    // pre-barrier blocks (an MFMA block between two DMA pieces) instead of a
    // burst right after the barrier, where both waves of a SIMD stall on
    // their DMA issue at once; all pieces are out before the chunk's wait
    f16x8 fb0[TN][2], fb1[TN][2];
    f16x8 fa[TM + 1][2];  // the chunk's A blocks; [TM]: the next chunk's block 0
    readB(lds, fb0);
    readA(lds, 0, fa[0]);
    int scur = 0;  // stage of chunk kc
    auto chunk = [&](auto dtag, int kc, f16x8 (&fbc)[TN][2], f16x8 (&fbn)[TN][2]) {
      constexpr int D = decltype(dtag)::value;
      constexpr int PRE = TM - D;  // blocks multiplied before the barrier
      constexpr int SPB = PRE > 0 ? PRE : 1;  // blocks the DMA pieces spread over
      const unsigned char* st = lds + scur * STAGE;
      const int sprev = scur == 0 ? NS - 1 : scur - 1;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if (SPREAD && kc >= 1 && i < SPB) {
#pragma unroll
          for (int j = i * PPW / SPB; j < (i + 1) * PPW / SPB; ++j)
            issue_piece(kc - 1 + NS, sprev, j);
        }
        if (i + 1 < TM) readA(st, i + 1, fa[i + 1]);
        if (i < PRE) {
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = mfma_h2t(fa[i][0], fa[i][1], fbc[j][0], fbc[j][1], acc[i][j]);
        }
      }
      if (kc + 1 < nkc) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_vmcnt<PPW * (NS - 2)>();  // chunk kc + 1 landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (!SPREAD) issue(kc + NS, scur);
        scur = scur + 1 == NS ? 0 : scur + 1;
        const unsigned char* sn = lds + scur * STAGE;
        readB(sn, fbn);
        readA(sn, 0, fa[TM]);
      }
#pragma unroll
      for (int i = PRE; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = mfma_h2t(fa[i][0], fa[i][1], fbc[j][0], fbc[j][1], acc[i][j]);
      fa[0][0] = fa[TM][0];
      fa[0][1] = fa[TM][1];
    };
    auto loop = [&](auto dtag) {
      int kc = 0;
      for (; kc + 1 < nkc; kc += 2) {
        chunk(dtag, kc, fb0, fb1);
        chunk(dtag, kc + 1, fb1, fb0);
      }
      if (kc < nkc) chunk(dtag, kc, fb0, fb1);
    };
    if (DO == DY || wave < NW / 2)
      loop(std::integral_constant<int, DO>{});
    else
      loop(std::integral_constant<int, DY>{});
  }
  wait_vmcnt<0>();
}

}  // namespace pps
