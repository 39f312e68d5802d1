// Host check of the SMPL backward's rules in tepose_amd/csrc/shapes.h: the launch shapes of its kernels cover every (person,
// vertex), every table row and every (person, column) exactly once; the buffer sizes the entry point carves (smpl_bwd_floats, the one function behind
// tepose_smpl_bwd_workspace_bytes too) hold what those launches write and grow with N; and the order in which the chain kernel finishes joints
// (chain_bwd_order) visits every child before its parent.  Plain C++: the header includes nothing from HIP.
//   smpl_bwd_shape_check                 the shape and size rules
//   smpl_bwd_shape_check p0 .. p23       the levels and the order for a tree given as its 24 parents (p0 ignored)
//   smpl_bwd_shape_check N               prints the blend backward's launch for N persons: "blend <persons per workgroup> <splits> <skin blocks> <chunks>"
//                                        (tools/smpl_backward_bench.py restates the rule for its byte floors; tests/test_smpl_bwd_host.py compares)
#include <stdio.h>
#include <stdlib.h>

#include "shapes.h"

using namespace tepose;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      ++fails;                                                    \
      printf("FAIL line %d: %s\n", __LINE__, #c);                 \
    }                                                             \
  } while (0)

static int check_order(char** argv) {
  int par[kNJ], order[kNJ], pos[kNJ];
  for (int j = 0; j < kNJ; ++j) par[j] = atoi(argv[1 + j]);
  for (int j = 1; j < kNJ; ++j) CHECK(par[j] >= 0 && par[j] < j);        // what tepose_pack_smpl admits
  if (fails) return 1;
  for (int j = 0; j < kNJ; ++j) { order[j] = -1; pos[j] = -1; }
  int dep[kNJ];
  const int maxd = chain_depths(par, dep);                               // what tepose_pack_smpl packs and both chain kernels walk
  CHECK(dep[0] == 0 && maxd >= 1 && maxd <= kNJ - 1);
  for (int j = 1; j < kNJ; ++j) CHECK(dep[j] == dep[par[j]] + 1 && dep[j] >= 1 && dep[j] <= maxd);      // a child is exactly one level below its parent
  chain_bwd_order(par, order);
  for (int i = 0; i < kNJ; ++i) {
    CHECK(order[i] >= 0 && order[i] < kNJ);
    if (order[i] >= 0 && order[i] < kNJ) { CHECK(pos[order[i]] < 0); pos[order[i]] = i; }      // every joint once
  }
  for (int j = 0; j < kNJ; ++j) CHECK(pos[j] >= 0);
  for (int j = 1; j < kNJ; ++j) CHECK(pos[j] < pos[par[j]]);              // a child is finished before its parent
  CHECK(order[kNJ - 1] == 0);                                             // the root last
  if (fails) return 1;
  printf("ok order");
  for (int i = 0; i < kNJ; ++i) printf(" %d", order[i]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1 + kNJ) return check_order(argv);
  if (argc == 2) {
    const Launch bl = blend_bwd_shape(atoi(argv[1]));
    printf("blend %d %u %d %d\n", blend_bwd_persons(bl.kernel), bl.gx, kBwdSkinBlocks, kBwdChunks);
    return 0;
  }
  int combos = 0;
  const int Ns[] = {1, 2, 4, 5, 8, 9, 16, 31, 32, 33, 64, 130, 450, 511, 512, 513, 1000, 8192, 8193, 65535, kSmplBwdMaxN};
  size_t prev_total = 0;
  SmplBwdFloats prev = {0, 0, 0, 0, 0};
  for (int N : Ns) {
    // skinning: every vertex has a thread, every person a block row; a block's persons are a1
    const Launch sk = skin_bwd_shape(N);
    CHECK(sk.threads == (unsigned)kBwdSkinVB && sk.gx == (unsigned)kBwdSkinBlocks && sk.gz == 1u);
    CHECK((long)sk.gx * kBwdSkinVB >= kNV && ((long)sk.gx - 1) * kBwdSkinVB < kNV);
    CHECK(sk.a1 >= 1 && sk.a1 <= kSkinPG && (long)sk.gy * sk.a1 >= N && ((long)sk.gy - 1) * sk.a1 < N && sk.gy <= 65535u);
    // blend: the splits cover every chunk once, none is empty; the tiles cover every person
    const Launch bl = blend_bwd_shape(N);
    const int pt = blend_bwd_persons(bl.kernel);
    CHECK(bl.threads == 128u && 2 * 112 == kBlendK && bl.gz == 1u);
    CHECK(bl.a0 >= 1 && (long)bl.gx * bl.a0 >= kBwdChunks && ((long)bl.gx - 1) * bl.a0 < kBwdChunks && bl.gx >= 1u && bl.gx <= (unsigned)kBwdChunks);
    CHECK((long)bl.gy * pt >= N && ((long)bl.gy - 1) * pt < N && bl.gy <= 65535u);
    CHECK((N <= 8) == (bl.kernel == kBlendBwd8));
    CHECK((long)bl.gx * bl.gy >= 4 * kChipCUs || bl.gx == (unsigned)kBwdChunks);      // at least four workgroups per CU unless K runs out
    const Launch ch = chain_bwd_shape(N), jo = joints_bwd_shape(N), su = blend_bwd_sum_shape(N);
    CHECK(ch.threads == 256u && (long)ch.gx * 4 >= N && ((long)ch.gx - 1) * 4 < N);
    CHECK(jo.gx == (unsigned)N && jo.threads >= (unsigned)(kBwdSrc * 3));
    CHECK(su.threads == 256u && (long)su.gx * 64 >= (long)N * kBlendK && ((long)su.gx - 1) * 64 < (long)N * kBlendK);      // 64 elements x 4 quarters
    // sizes: exactly what the launches write
    const SmplBwdFloats f = smpl_bwd_floats(N);
    CHECK(f.gsrc == (size_t)N * kBwdSrc * 3 && f.gvp == (size_t)N * kVertLd && f.gf == (size_t)N * kBlendK);
    CHECK(f.skin_part == (size_t)N * sk.gx * kNJ * 12);                   // one 24 x 12 partial per (person, skinning workgroup)
    CHECK(f.blend_part >= (size_t)bl.gx * N * kBlendK);                   // one [N, 224] partial per split fits ...
    CHECK(f.blend_part <= 2 * (size_t)bl.gx * N * kBlendK + 64 * kBlendK); // ... in a bound that is at most about twice that
    CHECK(f.gsrc > prev.gsrc && f.gvp > prev.gvp && f.skin_part > prev.skin_part && f.blend_part > prev.blend_part && f.gf > prev.gf);   // every buffer monotone in N
    const size_t total = f.gsrc + f.gvp + f.skin_part + f.blend_part + f.gf;
    CHECK(total > prev_total);
    CHECK((long)N * kVertLd < (1L << 31));                                // (offsets are formed as long anyway)
    prev = f; prev_total = total;
    ++combos;
  }
  // every N: the partials of the chosen split fit their buffer, whose size never falls
  size_t rows_prev = 0;
  int bad = 0;
  for (int N = 1; N <= kSmplBwdMaxN; ++N) {
    const size_t rows = blend_bwd_part_rows(N);
    if (rows < (size_t)blend_bwd_shape(N).gx * N || rows <= rows_prev) ++bad;
    rows_prev = rows;
  }
  CHECK(bad == 0);
  CHECK(kBwdChunks == 323 && kBwdSkinBlocks == 14 && kBwdSkinSlices == 21);
  CHECK((kBwdChunks - 1) * kBwdChunk < kBwdBlendRows && kBwdBlendRows <= kVertLd && kBwdBlendRows <= kBlendN);
  // what DESIGN.md section 19 states
  CHECK(blend_bwd_shape(1).gx == 323u && blend_bwd_shape(1).gy == 1u);
  CHECK(blend_bwd_shape(192).gx == 323u && blend_bwd_shape(192).gy == 6u);
  CHECK(blend_bwd_shape(450).gx == 108u && blend_bwd_shape(450).gy == 15u);
  CHECK(blend_bwd_shape(8192).gx == 8u && blend_bwd_shape(8192).gy == 256u);
  if (fails) return 1;
  printf("ok %d\n", combos);
  return 0;
}
