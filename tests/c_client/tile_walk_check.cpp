/* Host check of the persistent product's tile walk (tepose_amd/csrc/walk.h), compiled with the host compiler alone: tests/test_tile_walk.py.
 * For both walks and every combination of the group size, grid and tile counts below:
 *   - the map is a permutation of the tilesM x tilesN tiles, the partial last round included;
 *   - walk 0 is the map the kernel had before walk.h existed (ref_walk0: those four lines, kept here as the reference), and walk_block_tile --
 *     the block -> tile map of the one-tile-per-workgroup kernels, which each carried a copy of those lines -- is that map with grid = tile count;
 *   - walk 1 with a grid that is no multiple of 8, or with fewer tiles than workgroups, is walk 0;
 *   - walk 1: the slots of one XCD in one full round are grid / 8 CONSECUTIVE values of the linear tile order (what walk 0 gives an XCD too --
 *     the L2 patch is unchanged), hence at most GM row tiles and ceil(n / gm) + 1 column tiles where the patch lies inside one row group of gm
 *     rows (n = grid / 8; gm = GM except in the ragged last group: ceil(32 / GM) + 1 at the kernel's grid of 256);
 *   - walk 1: one full round is `grid` consecutive values, hence lies in at most ceil(grid / (GM tilesN)) + 1 row groups and touches at most
 *     GM times that many row tiles: 2 GM wherever a row group holds at least one round (GM tilesN >= grid), which is the property the walk
 *     exists for.  (With fewer tiles per group than workgroups NO map can stay within 2 GM row tiles -- tilesN = 1, GM = 1, grid = 256: 256
 *     tiles are 256 row tiles -- so the bound is stated in groups.)
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure. */
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "walk.h"

static void ref_walk0(int bid, int nwg, int tilesM, int tilesN, int& tm, int& tn, int GM) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  const int group = lin / (GM * tilesN), rem = lin - group * GM * tilesN;
  const int gm = std::min(GM, tilesM - group * GM);
  tm = group * GM + rem % gm;
  tn = rem / gm;
}

// the linear index of a tile in the group order (the inverse of the tail of walk_tile)
static int lin_of(int tm, int tn, int tilesM, int tilesN, int GM) {
  const int group = tm / GM, gm = std::min(GM, tilesM - group * GM);
  return group * GM * tilesN + tn * gm + (tm - group * GM);
}

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

static void check(int mode, int GM, int grid, int tilesM, int tilesN) {
  const int ntiles = tilesM * tilesN;
  std::vector<int> tms(ntiles), tns(ntiles);
  std::vector<char> seen(ntiles, 0);
  const bool fallback = grid % 8 != 0 || ntiles < grid;
  for (int tile = 0; tile < ntiles; ++tile) {
    int tm = -1, tn = -1;
    tepose::walk_tile(tile, ntiles, grid, tilesM, tilesN, GM, mode, &tm, &tn);
    tms[tile] = tm; tns[tile] = tn;
    if (tm < 0 || tm >= tilesM || tn < 0 || tn >= tilesN) { FAIL("range mode %d GM %d grid %d %dx%d tile %d -> (%d, %d)", mode, GM, grid, tilesM, tilesN, tile, tm, tn); continue; }
    if (seen[tm * tilesN + tn]++) FAIL("twice mode %d GM %d grid %d %dx%d tile %d -> (%d, %d)", mode, GM, grid, tilesM, tilesN, tile, tm, tn);
    if (mode == 0 || fallback) {
      int rm, rn;
      ref_walk0(tile, ntiles, tilesM, tilesN, rm, rn, GM);
      if (rm != tm || rn != tn) FAIL("walk0 mode %d GM %d grid %d %dx%d tile %d -> (%d, %d), reference (%d, %d)", mode, GM, grid, tilesM, tilesN, tile, tm, tn, rm, rn);
      // the one-tile-per-workgroup kernels: block `tile` of ntiles workgroups (their grid IS the tile count, whatever `grid` says here)
      int bm = -1, bn = -1;
      tepose::walk_block_tile(tile, ntiles, tilesM, tilesN, GM, &bm, &bn);
      if (bm != rm || bn != rn) FAIL("walk_block_tile GM %d %dx%d block %d -> (%d, %d), reference (%d, %d)", GM, tilesM, tilesN, tile, bm, bn, rm, rn);
    }
  }
  if (mode != 1 || fallback) return;
  const int n = grid / 8, per_group = GM * tilesN;
  for (int base = 0; base + grid <= ntiles; base += grid) {
    std::set<int> rows;
    for (int b = 0; b < grid; ++b) rows.insert(tms[base + b]);
    const int bound = GM * (ceil_div(grid, per_group) + 1);          // = 2 GM when per_group >= grid
    if ((int)rows.size() > bound) FAIL("round rows mode 1 GM %d grid %d %dx%d round at %d: %d row tiles > %d", GM, grid, tilesM, tilesN, base, (int)rows.size(), bound);
    if (per_group >= grid && (int)rows.size() > 2 * GM) FAIL("round rows > 2 GM: GM %d grid %d %dx%d round at %d: %d", GM, grid, tilesM, tilesN, base, (int)rows.size());
    for (int xcd = 0; xcd < 8; ++xcd) {
      std::set<int> prow, pcol, plin;
      for (int loc = 0; loc < n; ++loc) {
        const int t = base + xcd + 8 * loc;
        prow.insert(tms[t]); pcol.insert(tns[t]); plin.insert(lin_of(tms[t], tns[t], tilesM, tilesN, GM));
      }
      const int l0 = base + xcd * n;
      if ((int)plin.size() != n || *plin.begin() != l0 || *plin.rbegin() != l0 + n - 1)
        FAIL("patch not consecutive: GM %d grid %d %dx%d round at %d xcd %d: %d values %d..%d, expected %d..%d", GM, grid, tilesM, tilesN, base, xcd, (int)plin.size(),
             *plin.begin(), *plin.rbegin(), l0, l0 + n - 1);
      const int g0 = l0 / per_group, g1 = (l0 + n - 1) / per_group;
      if (g0 == g1) {                                                // inside one row group: the patch shape
        const int gm = std::min(GM, tilesM - g0 * GM);
        if ((int)prow.size() > GM || (int)pcol.size() > ceil_div(n, gm) + 1)
          FAIL("patch shape: GM %d grid %d %dx%d round at %d xcd %d: %d rows x %d columns (gm %d)", GM, grid, tilesM, tilesN, base, xcd, (int)prow.size(), (int)pcol.size(), gm);
      } else if ((int)prow.size() > GM * (ceil_div(n, per_group) + 1)) {
        FAIL("patch rows: GM %d grid %d %dx%d round at %d xcd %d: %d rows", GM, grid, tilesM, tilesN, base, xcd, (int)prow.size());
      }
    }
  }
}

int main() {
  const int GMs[] = {1, 4, 8, 16, 32}, grids[] = {8, 64, 256, 12, 100, 250}, tMs[] = {1, 2, 7, 8, 9, 40, 41, 512}, tNs[] = {1, 4, 12, 36, 81};
  int combos = 0;
  for (int mode = 0; mode <= 1; ++mode)
    for (int GM : GMs)
      for (int grid : grids)
        for (int tM : tMs)
          for (int tN : tNs) { check(mode, GM, grid, tM, tN); ++combos; }
  // a walk value that is neither 0 nor 1 is walk 0
  for (int tile = 0; tile < 512 * 36; tile += 97) {
    int a, b, c, d;
    tepose::walk_tile(tile, 512 * 36, 256, 512, 36, 8, 7, &a, &b);
    ref_walk0(tile, 512 * 36, 512, 36, c, d, 8);
    if (a != c || b != d) FAIL("walk 7 is not walk 0 at tile %d", tile);
  }
  // the workload's layer-0 projection (512 x 36 tiles, GM 8, 256 workgroups): walk 0 has 64 row tiles live in a round, walk 1 at most 16
  for (int mode = 0; mode <= 1; ++mode) {
    std::set<int> rows;
    for (int b = 0; b < 256; ++b) {
      int tm, tn;
      tepose::walk_tile(256 * 3 + b, 512 * 36, 256, 512, 36, 8, mode, &tm, &tn);
      rows.insert(tm);
    }
    std::printf("cfg-C projection, round 3, walk %d: %d row tiles live\n", mode, (int)rows.size());
    if (mode == 0 ? (int)rows.size() != 64 : (int)rows.size() > 16) FAIL("cfg-C live rows walk %d: %d", mode, (int)rows.size());
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok %d\n", combos);
  return 0;
}
