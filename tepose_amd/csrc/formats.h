// The memory formats every producer and consumer agrees on: operand planes (blocked / scaled), the 16 x 16-blocked fp32 scratch of large batches, and
// the row widths they are applied to.  Pure index arithmetic, device code and plain C++ alike: nothing from HIP is included, so the host compiler
// alone builds it (tests/test_state_layout.py).  common.h includes this header; state.h builds the encoder's workspace addressing on it.
#pragma once
#include <stddef.h>

#ifndef TEPOSE_HD
#if defined(__HIPCC__)
#define TEPOSE_HD __host__ __device__
#else
#define TEPOSE_HD
#endif
#endif

namespace tepose {

constexpr int kFeat = 2048;
constexpr int kTheta = 85;
constexpr int kInput = 2133;
constexpr int kInputP = 2144;   // 2133 padded to a multiple of the GEMM K-tile (32)
constexpr int kNV = 6890;
constexpr int kNJ = 24;
constexpr int kNPose = 144;
constexpr int kState = 160;     // regressor state row: pose6d(144) | shape(10) | cam(3) | pad(3)
constexpr int kBlendK = 224;    // [1 | betas(10) | pose_feature(207) | pad(6)]
constexpr int kBlendN = 20736;  // 3*6890 = 20670 padded to a multiple of 128
constexpr int kVertLd = 20672;  // row stride of the v_posed scratch (>= 20670, multiple of 4)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------- blocked planes (gemm_h3.hip, split-precision fp16x3 GEMM)
// Operand planes are stored K-tile-blocked and slot-swizzled: element (row, c) of an [R x C] matrix (C multiple
// of 32) lives at
//   ((c / 32) * R + row) * 32 + (((c / 8) % 4) ^ ((row / 4) % 4)) * 8 + c % 8        (halfs)
// * blocked: the 64 bytes a K-tile takes from each of a block's rows form one contiguous run, so an LDS-DMA
//   instruction (16 rows) moves one contiguous KiB = 8 whole 128-byte lines;
// * swizzled in memory: the XOR that makes the LDS image bank-conflict-free for ds_read_b128 is already in
//   the data, so the DMA's global addresses simply ascend with the lane number.
// Measured against row-major planes with the XOR applied in the lane addresses, this layout is worth 0-3 % on
// the layer-0 projection (within box-to-box noise; profiles/r01_README.md) -- it is kept because it makes the
// DMA addressing trivial, not because it is faster.
// A view of rows [r0, r0+M) x columns [c0, c0+K), r0 % 16 == 0 and c0 % 32 == 0, is the pointer to block
// (r0, c0) plus the K-tile stride R * 32.
constexpr int kPlaneK = 32;
// halfs from the start of a row's K-tile to its 16-byte slot q (0..3, 8 halfs): the swizzle, stated once
TEPOSE_HD inline int plane_slot(long row, int q) { return (q ^ (int)((row >> 2) & 3)) << 3; }
TEPOSE_HD inline long plane_index(long row, long c, long R) {
  return ((c >> 5) * R + row) * 32 + plane_slot(row, (int)((c >> 3) & 3)) + (c & 7);
}
// ---------------------------------------------------------------- scaled planes (gemm_h3s.hip: single accumulator, 256 x 256 tiles), [K/16][R][16] layout:
// element (row, k) of an [R x Kp] matrix (Kp multiple of 16), value v stored as hi = fp16(v p), lo = fp16(v p - hi)
TEPOSE_HD inline int plane16_slot(long row, int q) { return (q ^ (int)((row >> 3) & 1)) << 3; }   // slot q (0..1) of a row's 16-wide K-tile, in halfs
TEPOSE_HD inline long plane16_index(long row, long k, long R) {
  return ((k >> 4) * R + row) * 16 + plane16_slot(row, (int)((k >> 3) & 1)) + (k & 7);
}

// ---------------------------------------------------------------- 16 x 16-blocked fp32 scratch of large batches
// fp32 recurrent state of large batches between two cell steps (its only reader is the next step's cell update): element (row, unit) of a view
TEPOSE_HD inline long st_blk_offset(long row, int unit, long rt_stride) {
  return (row >> 4) * rt_stride + (long)(unit >> 4) * 256 + ((((unit & 15) >> 2) * 16 + (row & 15)) << 2) + (unit & 3);
}
// Blocked layout of the gate pre-activations of large batches (round 4; internal scratch between the barrier-free projection kernel
// and the fused GRU step / first-step kernels): 16 rows x 16 hidden units of one gate = one 1 KB block, stored in the order of the
// 16x16x32 MFMA's transposed C fragment (lane = (unit % 16 / 4) * 16 + row % 16 holds 4 consecutive units) -- a wave instruction of the
// producer's tile store and of the consumer's cell-update load moves ONE contiguous KB instead of 16 rows x 64 bytes.  Inside a
// 16-row tile the blocks are ordered [unit / 32][unit / 16 & 1][gate]: the six blocks a wave reads per row tile are 6 KB in a row.
// Offset (floats) of element (row, gate, unit) relative to the view's first row tile; rt_stride = 3 Hp * 16 for a [rows][3 Hp] matrix.
TEPOSE_HD inline long gi_blk_block(int gate, int unit) { return ((long)(unit >> 5) * 6 + ((unit >> 4) & 1) * 3 + gate) * 256; }
// column `col` of a [rows][ND * 3 Hp] matrix ([dir][gate][unit]): the block's offset inside its row tile (directions are 3 Hp * 16 floats apart)
TEPOSE_HD inline long gi_blk_col_block(int col, int hp) {
  const int dgi = col / hp, unit = col - dgi * hp, dir = dgi / 3;
  return (long)dir * 3 * hp * 16 + gi_blk_block(dgi - 3 * dir, unit);
}
TEPOSE_HD inline long gi_blk_offset(long row, int gate, int unit, long rt_stride) {
  return (row >> 4) * rt_stride + gi_blk_block(gate, unit) + ((((unit & 15) >> 2) * 16 + (row & 15)) << 2) + (unit & 3);
}

}  // namespace tepose
