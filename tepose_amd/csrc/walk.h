// The tile walk of the persistent scaled-plane product (gemm_h3s16c.hip): which 256 x 256 tile of C the k-th unit of work is -- and, as its
// one-round special case walk_block_tile, the block -> tile map of every one-tile-per-workgroup kernel.
// One function, device code and plain C++ alike (tests/test_tile_walk.py compiles it with the host compiler and checks it exhaustively).
//
// A workgroup takes the units  blockIdx.x, blockIdx.x + grid, blockIdx.x + 2 grid, ...;  unit `tile` is slot  b = tile % grid  of round
// r = tile / grid.  Workgroups are placed on the XCDs round-robin (slot b runs on XCD b & 7 -- a speed assumption only, nothing depends on
// it for correctness), so an XCD's grid / 8 resident workgroups are the slots  b = xcd, xcd + 8, ...
//
// Both modes map a unit to a LINEAR index `lin` first and share the rest: lin runs through groups of GM row tiles, inside a group down the
// GM rows first and then along the tilesN columns (the last group has  tilesM - group GM  rows), so grid / 8 consecutive lin values are a
// patch of GM row tiles x grid / (8 GM) column tiles: the A and W panels an XCD's workgroups share in its L2.
//   mode 0  every XCD owns one contiguous eighth of [0, ntiles) for the whole launch (the first  ntiles % 8  XCDs one value more): at any
//           moment the eight XCDs sit in eight different row groups -- 8 GM A panels are live chip-wide.
//   mode 1  all eight XCDs walk the SAME row group: the patches of round r are the eight consecutive ones  P = 8 r + xcd,
//           lin = P (grid / 8) + loc -- a round is `grid` consecutive lin values, which lie in at most two row groups while a group has at
//           least `grid` tiles (GM tilesN >= grid), so at most 2 GM A panels are live chip-wide and the operands the XCDs re-read beyond
//           their L2 are the same ones.  The last, partial round deals its  ntiles - r grid  values to the XCDs the way mode 0 deals all
//           of them.  grid % 8 != 0 or ntiles < grid: mode 0.
// Either mode is a permutation of [0, ntiles): the walk decides who computes a tile and when, never what is computed.
#pragma once

#ifndef TEPOSE_WALK_HD
#if defined(__HIPCC__)
#define TEPOSE_WALK_HD __host__ __device__
#else
#define TEPOSE_WALK_HD
#endif
#endif

namespace tepose {

// n values dealt to the 8 XCDs in contiguous runs (the first n % 8 runs one longer): the value of slot b < n
TEPOSE_WALK_HD inline int walk_deal8(int n, int b) {
  const int q = n >> 3, r = n & 7, xcd = b & 7, loc = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

TEPOSE_WALK_HD inline void walk_tile(int tile, int ntiles, int grid, int tilesM, int tilesN, int GM, int mode, int* tm, int* tn) {
  int lin;
  if (mode == 1 && grid > 0 && (grid & 7) == 0 && ntiles >= grid) {
    const int base = tile / grid * grid, b = tile - base, left = ntiles - base;
    lin = base + (left >= grid ? (b & 7) * (grid >> 3) + (b >> 3) : walk_deal8(left, b));
  } else {
    lin = walk_deal8(ntiles, tile);
  }
  const int group = lin / (GM * tilesN), rem = lin - group * GM * tilesN;
  const int gm = GM < tilesM - group * GM ? GM : tilesM - group * GM;
  *tm = group * GM + rem % gm;
  *tn = rem / gm;
}

// The one-tile-per-workgroup kernels (gemm.hip, gemm_h3.hip, gemm_h3s.hip, gru_step16.hip): block bid of nwg = tilesM * tilesN is unit bid of a
// single round of walk 0 -- blocks are dealt round-robin to the 8 XCDs (bid % 8 shares an L2), so each XCD gets one contiguous run of the
// grouped order, in which GM row tiles share every W panel.
TEPOSE_WALK_HD inline void walk_block_tile(int bid, int nwg, int tilesM, int tilesN, int GM, int* tm, int* tn) {
  walk_tile(bid, nwg, nwg, tilesM, tilesN, GM, 0, tm, tn);
}

}  // namespace tepose
