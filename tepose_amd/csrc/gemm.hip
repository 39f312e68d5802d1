// fp32 GEMM and fused GRU-cell step on the gfx950 matrix cores.
//
// Why fp32 MFMA: the 1e-4 parity budget (BASELINE.json north_star) goes through 2 GRU
// layers x T steps, 3 regressor iterations and LBS; gfx950 has an exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32 == k-ordered fmaf chain) and no TF32, so products stay fp32.
//
// Tiling (both kernels): 256 threads = 4 waves as 2(M) x 2(N); block tile 128 x (64*WN),
// wave tile 64 x (32*WN) = 2 x WN MFMA tiles of 32x32; K-tile 32.  A and W tiles are
// K-contiguous [rows][32] fp32 images in LDS, filled by LDS-DMA (global_load_lds_dwordx4,
// no VGPR staging) and double-buffered.  One 16-byte LDS read gives a lane 4 consecutive
// k of its row; lanes 0-31 take k-slots 2c, lanes 32-63 slots 2c+1, and MFMA #m of a
// chunk consumes register m of both operands -- a fixed permutation of k applied equally
// to A and W, so the dot product is unchanged.  The 16-byte slot index is XOR-swizzled
// with (row>>1)&7 on the DMA *source* address and on the read (the LDS image itself
// must stay lane-linear for LDS-DMA), which makes every ds_read_b128 conflict-free.
#include "device.h"
#include "walk.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace tepose {

constexpr int BM = 128;
#ifndef TEPOSE_BK
#define TEPOSE_BK 32
#endif
#ifndef TEPOSE_BK_GRU
#define TEPOSE_BK_GRU TEPOSE_BK
#endif
constexpr int BK_GEMM = TEPOSE_BK;     // K-tile (floats) of the plain GEMM: 32 -> 64 KB LDS per block
constexpr int BK_GRU = TEPOSE_BK_GRU;  // K-tile of the GRU step: 32 -> 80 KB, 16 -> 40 KB per block
#ifndef TEPOSE_GEMM_OCC
#define TEPOSE_GEMM_OCC 2
#endif
#ifndef TEPOSE_PIPE
#define TEPOSE_PIPE 1
#endif
#ifndef TEPOSE_ABL
#define TEPOSE_ABL 0   // diagnostic timing builds only: 1 no DMA, 2 no fragment reads, 3 no barrier, 4 no epilogue
#endif
#ifndef TEPOSE_GRU_OCC
#define TEPOSE_GRU_OCC 2
#endif

// Block id -> (tile_m, tile_n): walk.h's walk_block_tile with groups of 8 M-tiles -- the ~64 blocks
// resident on an XCD then cover about 8 x 8 tiles and each A / W K-slab is fetched once per XCD
// instead of 8 times.
constexpr int kTileGM = 8;

template <int WN, bool RELU, int BK, int WMF>
__device__ __forceinline__ void mainloop(const float* __restrict__ A, long lda, int M, int m0,
                                         const float* __restrict__ W, int Kp, int n0, float* lds,
                                         f32x16 (&acc)[WMF][WN]) {
  constexpr int BM = 64 * WMF;               // block rows: 2 waves along M x WMF 32-row fragments each
  static_assert(BK == 16 || BK == 32, "K-tile must be 16 or 32");
  constexpr int SLOTS = BK / 4;              // 16-byte slots per tile row
  constexpr int RPI = 64 / SLOTS;            // tile rows moved by one wave-wide DMA instruction
  constexpr int SWZ_SH = BK == 32 ? 1 : 2;   // rows per 256-B LDS bank row = 2 (BK 32) or 4 (BK 16)
  constexpr int BN = 64 * WN;
  constexpr int NAQ = BM / RPI / 4;          // A-tile DMA instructions per wave
  constexpr int NWQ = BN / RPI / 4;          // W-tile DMA instructions per wave
  constexpr int STAGE = (BM + BN) * BK;      // floats per pipeline stage
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  // ---- DMA source pointers: one wave-instruction moves 8 rows x 128 B ------------------
  const int lrow = lane / SLOTS, lslot = lane % SLOTS;
  const float* ga[NAQ];
  const float* gw[NWQ];
#pragma unroll
  for (int q = 0; q < NAQ; ++q) {
    const int row = (wave * NAQ + q) * RPI + lrow;
    const int grow = min(m0 + row, M - 1);   // tail rows re-read the last valid row
    ga[q] = A + (long)grow * lda + 4 * (lslot ^ ((row >> SWZ_SH) & (SLOTS - 1)));
  }
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    const int row = (wave * NWQ + q) * RPI + lrow;
    gw[q] = W + (long)(n0 + row) * Kp + 4 * (lslot ^ ((row >> SWZ_SH) & (SLOTS - 1)));
  }
  auto issue = [&](int kt, int buf) {
    float* la = lds + buf * STAGE;
    float* lw = la + BM * BK;
#pragma unroll
    for (int q = 0; q < NAQ; ++q) glds16(ga[q] + kt * BK, la + (wave * NAQ + q) * 256);
#pragma unroll
    for (int q = 0; q < NWQ; ++q) glds16(gw[q] + kt * BK, lw + (wave * NWQ + q) * 256);
  };

  // ---- fragment read offsets (floats) ---------------------------------------------------
  const int sw = (r >> SWZ_SH) & (SLOTS - 1);
  int aoff[WMF], boff[WN];
#pragma unroll
  for (int i = 0; i < WMF; ++i) aoff[i] = (wm * 32 * WMF + i * 32 + r) * BK;
#pragma unroll
  for (int j = 0; j < WN; ++j) boff[j] = BM * BK + (wn * 32 * WN + j * 32 + r) * BK;

  const int KT = Kp / BK;
  constexpr int NC = BK / 8;                 // 8-k chunks per K-tile
  auto load_frags = [&](const float* st, int c, f32x4 (&a)[WMF], f32x4 (&b)[WN]) {
    const int sx = 4 * ((2 * c + h) ^ sw);
#pragma unroll
    for (int i = 0; i < WMF; ++i) a[i] = *(const f32x4*)(st + aoff[i] + sx);
#pragma unroll
    for (int j = 0; j < WN; ++j) b[j] = *(const f32x4*)(st + boff[j] + sx);
  };
  auto mma = [&](f32x4 (&a)[WMF], f32x4 (&b)[WN]) {
    if (RELU) {
#pragma unroll
      for (int i = 0; i < WMF; ++i)
#pragma unroll
        for (int m = 0; m < 4; ++m) a[i][m] = fmaxf(a[i][m], 0.f);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < WMF; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][m], b[j][m], acc[i][j], 0, 0, 0);
  };
#if TEPOSE_PIPE
  // Software pipeline: fragments of chunk c+1 are read while chunk c's MFMAs run; the
  // stage barrier sits in front of the LAST chunk's MFMAs, so the first fragments of the
  // next stage are fetched underneath them and no ds_read latency is exposed per K-tile.
  f32x4 fa[2][WMF], fb[2][WN];
  issue(0, 0);
  __syncthreads();
  load_frags(lds, 0, fa[0], fb[0]);
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
#if TEPOSE_ABL != 1
    if (kt + 1 < KT) issue(kt + 1, buf ^ 1);
#endif
    const float* st = lds + buf * STAGE;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#if TEPOSE_ABL != 2
      if (c + 1 < NC) {
        load_frags(st, c + 1, fa[(c + 1) & 1], fb[(c + 1) & 1]);
      } else {
#if TEPOSE_ABL != 3
        __syncthreads();                                     // DMA(kt+1) landed; reads of `buf` issued
#endif
        if (kt + 1 < KT) load_frags(lds + (buf ^ 1) * STAGE, 0, fa[(c + 1) & 1], fb[(c + 1) & 1]);
      }
#else
      if (c + 1 == NC) __syncthreads();
#endif
      mma(fa[c & 1], fb[c & 1]);
    }
  }
#else
  issue(0, 0);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) issue(kt + 1, buf ^ 1);
    const float* st = lds + buf * STAGE;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f32x4 a[WMF], b[WN];
      load_frags(st, c, a, b);
      mma(a, b);
    }
    __syncthreads();   // all reads of `buf` done; DMA of the next stage has landed (vmcnt(0))
  }
#endif
}

// ------------------------------------------------------------------------------ plain GEMM
template <bool RELU, int WMF>
__global__ void __launch_bounds__(256, WMF == 2 ? TEPOSE_GEMM_OCC : 3) gemm_f32_kernel(GemmArgs a, int tilesM, int tilesN) {
  constexpr int BMT = 64 * WMF;
  __shared__ __attribute__((aligned(16))) float lds[2 * (BMT + 128) * BK_GEMM];
  int tm, tn;
  walk_block_tile(blockIdx.x, gridDim.x, tilesM, tilesN, kTileGM, &tm, &tn);
  const int m0 = tm * BMT, n0 = tn * 128;
  f32x16 acc[WMF][2];
#pragma unroll
  for (int i = 0; i < WMF; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  mainloop<2, RELU, BK_GEMM, WMF>(a.A, a.lda, a.M, m0, a.W, a.Kp, n0, lds, acc);
#if TEPOSE_ABL == 4
  if (a.scale != 123.f) {
    float sacc = 0.f;
    for (int i = 0; i < WMF; ++i) for (int j = 0; j < 2; ++j) for (int e = 0; e < 16; ++e) sacc += acc[i][j][e];
    if (sacc == 1.2345f) a.C[0] = sacc;
    return;
  }
#endif

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn * 64 + j * 32 + r;
    if (col >= a.N) continue;
    const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < WMF; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 32 * WMF + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row < a.M) {
          float v = acc[i][j][e] + bv;
          if (a.addend) v += a.addend[(long)row * a.ldadd + col];
          a.C[(long)row * a.ldc + col] = v * a.scale;
        }
      }
    }
  }
}

hipError_t launch_gemm(const GemmArgs& a, hipStream_t s, const Options& o) {   // (callers outside a TePose forward: the kernel plan chooses there)
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  return a.M <= gemm_skinny_max_m(o) ? launch_skinny_gemm(a, s) : launch_gemm_tiles(a, s, o);
}

hipError_t launch_gemm_tiles(const GemmArgs& a, hipStream_t s, const Options& o) {
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  const Launch l = f32_tiles_shape(a.M, a.N, o);
  switch (l.kernel) {
    case kF32Rows64:
      if (a.relu_a) hipLaunchKernelGGL((gemm_f32_kernel<true, 1>), grid_of(l), block_of(l), 0, s, a, l.a0, l.a1);
      else hipLaunchKernelGGL((gemm_f32_kernel<false, 1>), grid_of(l), block_of(l), 0, s, a, l.a0, l.a1);
      break;
    default:
      if (a.relu_a) hipLaunchKernelGGL((gemm_f32_kernel<true, 2>), grid_of(l), block_of(l), 0, s, a, l.a0, l.a1);
      else hipLaunchKernelGGL((gemm_f32_kernel<false, 2>), grid_of(l), block_of(l), 0, s, a, l.a0, l.a1);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ GRU step
// The W_hh tile of a block is 64 hidden units x 3 gates; packed row order inside the tile
// is [wave_n(2)][gate(3)][32], so a wave's three N-subtiles are the r, z, n pre-activations
// of the same 32 hidden units and the whole cell update (device.h gru_cell) happens in registers.

__global__ void __launch_bounds__(256, TEPOSE_GRU_OCC) gru_step_kernel(GruArgs a, int tilesM, int tilesJ) {
  __shared__ __attribute__((aligned(16))) float lds[2 * (BM + 192) * BK_GRU];
  const GruDir& d = a.d[blockIdx.y];
  int tm, tj;
  walk_block_tile(blockIdx.x, gridDim.x, tilesM, tilesJ, kTileGM, &tm, &tj);
  const int m0 = tm * BM;
  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][g][e] = 0.f;
#if TEPOSE_ABL != 5
  if (!a.first) mainloop<3, false, BK_GRU, 2>(d.hprev, d.ldh, a.M, m0, d.Whh, a.Hp, tj * 192, lds, acc);
#endif
#if TEPOSE_ABL == 4
  {
    float sacc = 0.f;
    for (int i = 0; i < 2; ++i) for (int g = 0; g < 3; ++g) for (int e = 0; e < 16; ++e) sacc += acc[i][g][e];
    if (sacc == 1.2345f) d.hout[0] = sacc;
    return;
  }
#endif

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int Hp = a.Hp;
  const int j = tj * 64 + wn * 32 + r;
  const float* __restrict__ gip = d.gi;
  const float* __restrict__ hpp = d.hprev;
  float* __restrict__ hop = d.hout;
  const float br = d.bhh[j], bz = d.bhh[Hp + j], bn = d.bhh[2 * Hp + j];
  const bool first = a.first != 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rbase = m0 + wm * 64 + i * 32 + 4 * h;
    // all loads of this 32-row fragment first (rows past M re-read row M-1, never stored)
    float gr[16], gz[16], gn[16], hp[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = min(rbase + (e & 3) + 8 * (e >> 2), a.M - 1);
      const float* gi = gip + (long)row * d.ldgi + j;
      gr[e] = gi[0]; gz[e] = gi[Hp]; gn[e] = gi[2 * Hp];
      hp[e] = first ? 0.f : hpp[(long)row * d.ldh + j];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = rbase + (e & 3) + 8 * (e >> 2);
      const float hv = gru_cell(gr[e], gz[e], gn[e], acc[i][0][e] + br, acc[i][1][e] + bz, acc[i][2][e] + bn, hp[e]);
      if (row < a.M) hop[(long)row * d.ldo + j] = hv;
    }
  }
}

hipError_t launch_gru_step(const GruArgs& a, hipStream_t s, const Options& o) {
  if (a.M <= 0 || a.ndir <= 0) return hipSuccess;
  return a.M <= o.skinny_max_m ? launch_skinny_gru(a, s) : launch_gru_step_tiles(a, s);
}

hipError_t launch_gru_step_tiles(const GruArgs& a, hipStream_t s) {
  if (a.M <= 0 || a.ndir <= 0) return hipSuccess;
  const int tilesM = (a.M + BM - 1) / BM, tilesJ = a.Hp / 64;
  dim3 grid(tilesM * tilesJ, a.ndir), block(256);
  hipLaunchKernelGGL(gru_step_kernel, grid, block, 0, s, a, tilesM, tilesJ);
  return hipGetLastError();
}

}  // namespace tepose
