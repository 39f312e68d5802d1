/* Host check of the launch-shape rules (tepose_amd/csrc/shapes.h on options.h and formats.h), compiled with the host compiler alone:
 * tests/test_launch_shapes.py.
 *   - Every rule equals the expressions the launchers and select_kernels carried before shapes.h existed.  Those are kept here verbatim as ref_*
 *     functions (a launch line became `return rec(...)` of the same grid, block and arguments) and every field of every result is compared -- kernel
 *     instantiation, grid x / y / z, threads, the integer kernel arguments, and the three cost figures of the blocked-plane tile model -- over the
 *     full cross product of the shapes and the option variants below, and at a value on each side of every threshold.
 *   - A table of literals: the outcomes DESIGN.md and the comments of shapes.h state, at default options, pinned independently of ref_*.
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure.  `--time`: ns per decision, shapes.h against ref_*, for the
 * launches of a B = 1 forward. */
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "shapes.h"

using namespace tepose;

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

// ------------------------------------------------------------------ what the launch lines of the parent commit passed
struct dim3 { unsigned x, y, z; dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {} };
static Launch rec(int kernel, dim3 grid, dim3 block, int a0 = 0, int a1 = 0) { return {kernel, grid.x, grid.y, grid.z, block.x, a0, a1}; }
struct RefP { int M, N; };
struct RefBatch { RefP p[3]; int n; int Hp; };
struct RefCosts { double c128, c64, c192; };     // -1: the launcher did not compute it on this path

// gemm_h3.hip launch_gemm_h3
static Launch ref_gemm_h3(const RefBatch& b, const Options& o, RefCosts* costs) {
  *costs = {-1., -1., -1.};
  const int tilesM = (b.p[0].M + 255) / 256, tilesN = (b.p[0].N + 127) / 128;
  const int tile_dbg = o.h3_tile;   // A/B: force a tile shape
  if (tile_dbg == 64) {
    const int tm = (b.p[0].M + 63) / 64;
    return rec(kH3Tile64x128, dim3(tm * tilesN, b.n), dim3(256), tm, tilesN);
  }
  if (tile_dbg == 192) {
    const int tm = (b.p[0].M + 127) / 128, tn = (b.p[0].N + 191) / 192;
    return rec(kH3Tile128x192, dim3(tm * tn, b.n), dim3(512), tm, tn);
  }
  if (tile_dbg == 256) {
    return rec(kH3Tile256x128, dim3(tilesM * tilesN, b.n), dim3(512), tilesM, tilesN);
  }
  if (b.p[0].M <= 2048 && tilesM * tilesN * b.n < 1024) {
    const int tm = (b.p[0].M + 127) / 128;
    const int t64 = o.h3_tile64;     // 0: never (A/B)
    const int tm64 = (b.p[0].M + 63) / 64;
    const double w128 = (double)tm * tilesN * b.n, w64 = (double)tm64 * tilesN * b.n;
    const double c128 = 47. * (double)(long)((w128 + 255.) / 256.), c64 = 33. * (w64 <= 256. ? 1. : (w64 / 256. > 1.55 ? w64 / 256. : 1.55));
    costs->c128 = c128; costs->c64 = c64;
    if (o.h3_tile192 && b.p[0].N % 192 == 0) {
      const double w192 = (double)tm * (b.p[0].N / 192) * b.n, c192 = 70. * (double)(long)((w192 + 255.) / 256.);
      costs->c192 = c192;
      if (c192 < 0.9 * c128 && c192 <= c64) {
        return rec(kH3Tile128x192, dim3(tm * (b.p[0].N / 192), b.n), dim3(512), tm, b.p[0].N / 192);
      }
    }
    if (t64 && c64 < 0.9 * c128) {
      return rec(kH3Tile64x128, dim3(tm64 * tilesN, b.n), dim3(256), tm64, tilesN);
    }
    return rec(kH3Tile128x128, dim3(tm * tilesN, b.n), dim3(512), tm, tilesN);
  }
  return rec(kH3Tile256x128, dim3(tilesM * tilesN, b.n), dim3(512), tilesM, tilesN);
}

// gemm_h3.hip launch_gru_h3
static Launch ref_gru_h3(const RefBatch& b) {
  int tilesM = (b.p[0].M + 127) / 128;
  const int tilesJ = b.Hp / 64;                      // block = 128 rows x (64 hidden units x 3 gates)
  if (tilesM * tilesJ * b.n <= 160) {                // mid-size batches: 64-row blocks (4 waves) fill more CUs
    tilesM = (b.p[0].M + 63) / 64;
    return rec(kGruH3Rows64, dim3(tilesM * tilesJ, b.n), dim3(256), tilesM, tilesJ);
  }
  return rec(kGruH3Rows128, dim3(tilesM * tilesJ, b.n), dim3(512), tilesM, tilesJ);
}

// skinny_h3.hip launch_skinny_gemm_h3_batch (after its maxM / maxN loop)
static Launch ref_skinny_gemm_h3_batch(int maxM, int maxN, const RefBatch& b, const Options& o) {
  const int nt = (maxN + 47) / 48;
  const int nt1_max = o.skinny_nt1_below;
  {
    const bool mt1 = o.skinny_mt1 != 0;
    const int blocks16 = (maxN + 15) / 16 * b.n, rowtiles = (maxM + 15) / 16;
    if (mt1 && nt * b.n < nt1_max && blocks16 * rowtiles <= 256) {
      return rec(kSkinnyH3_1x1w8, dim3((maxN + 15) / 16, rowtiles, b.n), dim3(512));
    }
  }
  if (maxM <= 32 && nt * b.n < nt1_max) {
    const bool w8 = o.skinny_w8 != 0;
    if (w8 && (maxN + 15) / 16 * b.n <= 128)
      return rec(kSkinnyH3_2x1w8, dim3((maxN + 15) / 16, 1, b.n), dim3(512));
    else
      return rec(kSkinnyH3_2x1w4, dim3((maxN + 15) / 16, 1, b.n), dim3(256));
  } else if (maxM <= 64 && maxM > 32 && nt * b.n < 96 && o.skinny_narrow64 != 0) {
    const bool w8 = o.skinny_w8 != 0;
    if (w8 && (maxN + 15) / 16 * b.n <= 128)
      return rec(kSkinnyH3_4x1w8, dim3((maxN + 15) / 16, 1, b.n), dim3(512));
    else
      return rec(kSkinnyH3_4x1w4, dim3((maxN + 15) / 16, 1, b.n), dim3(256));
  } else {
    const int tiles = (maxM + 15) / 16, passes = (tiles + 3) / 4;
    const int mt = o.skinny_mt1 != 0 ? (tiles + passes - 1) / passes : (maxM <= 32 ? 2 : 4);
    const dim3 grid(nt, (tiles + mt - 1) / mt, b.n);
    if (mt <= 1) return rec(kSkinnyH3_1, grid, dim3(256));
    else if (mt == 2) return rec(kSkinnyH3_2, grid, dim3(256));
    else if (mt == 3) return rec(kSkinnyH3_3, grid, dim3(256));
    else return rec(kSkinnyH3_4, grid, dim3(256));
  }
}

// skinny_h3.hip launch_skinny_gru_h3
static Launch ref_skinny_gru_h3(const RefBatch& b) {
  const int M = b.p[0].M;
  const int jt = b.Hp / 16;
  if (M <= 32) {
    return rec(kSkinnyRows32, dim3(jt, 1, b.n), dim3(256));
  } else {
    return rec(kSkinnyRows64, dim3(jt, (M + 63) / 64, b.n), dim3(256));
  }
}

// skinny.hip launch_skinny_gemm / launch_skinny_gru (SK_NW1: waves per block of the 16-row form)
struct RefG { int M, N, Hp, ndir; };
static Launch ref_skinny_gemm(const RefG& g, int SK_NW1) {
  const int nt = (g.N + 47) / 48;
  if (g.M <= 16) {
    return rec(kSkinnyRows16, dim3(nt, 1), dim3(64 * SK_NW1));
  } else if (g.M <= 32) {
    return rec(kSkinnyRows32, dim3(nt, 1), dim3(256));
  } else {
    return rec(kSkinnyRows64, dim3(nt, (g.M + 63) / 64), dim3(256));
  }
}
static Launch ref_skinny_gru(const RefG& a, int SK_NW1) {
  const int jt = a.Hp / 16;
  if (a.M <= 16) {
    return rec(kSkinnyRows16, dim3(jt, 1, a.ndir), dim3(64 * SK_NW1));
  } else if (a.M <= 32) {
    return rec(kSkinnyRows32, dim3(jt, 1, a.ndir), dim3(256));
  } else {
    return rec(kSkinnyRows64, dim3(jt, (a.M + 63) / 64, a.ndir), dim3(256));
  }
}

// gemm.hip launch_gemm_tiles
static Launch ref_gemm_tiles(const RefG& a, const Options& o) {
  const int tilesN = (a.N + 127) / 128;
  const int half_max_blocks = o.gemm_half_max_blocks;
  const int tiles128 = (a.M + 127) / 128;
  if (tiles128 * tilesN <= half_max_blocks) {
    const int tilesM = (a.M + 63) / 64;
    dim3 grid(tilesM * tilesN), block(256);
    return rec(kF32Rows64, grid, block, tilesM, tilesN);
  }
  dim3 grid(tiles128 * tilesN), block(256);
  return rec(kF32Rows128, grid, block, tiles128, tilesN);
}

// gru_seq.hip gru_seq_gran_rows / gru_seq_ok (cus: what device_cus returned) / launch_gru_seq; common.h predicates
static int ref_gru_seq_gran_rows(const Options& o) { return o.seq_gran_max_m > (int)4 ? (int)4 : o.seq_gran_max_m; }
static bool ref_gru_seq_shape_ok(int Hp) { return Hp % 256 == 0 && Hp <= 1024; }
static bool ref_gru_first16_shape_ok(int Hp) { return Hp % 128 == 0; }
static bool ref_split_rows_few_ok(long rows, int Kp, int permT, const Options& o) { return rows <= o.split_few_max_rows && Kp <= 4096 && !permT; }
static int ref_gemm_skinny_max_m(const Options& o) { return o.skinny_max_m_gemm >= 0 ? o.skinny_max_m_gemm : o.skinny_max_m; }
static bool ref_gru_seq_ok(int ndir, int M, int Hp, int T, const Options& o, int cus) {
  const int max_m = o.seq_max_m > 64 ? 64 : o.seq_max_m;
  return M >= 1 && M <= max_m && T >= 2 && T <= 36 && ref_gru_seq_shape_ok(Hp) && ndir >= 1 &&
         ndir <= 3 && ndir * (Hp / 16) <= cus;
}
static Launch ref_gru_seq(const RefG& a) {
  dim3 grid(a.Hp / 16, 1, a.ndir);
  if (a.M <= 16) return rec(1, grid, dim3(512));
  if (a.M <= 32) return rec(2, grid, dim3(512));
  if (a.M <= 48) return rec(3, grid, dim3(512));
  return rec(4, grid, dim3(512));
}

// gemm_h3s16c.hip launch_gemm_h3s16c, gru_step16.hip launch_gru_step16, gemm_h3s.hip launch_gemm_h3s_mid
static Launch ref_gemm_h3s16c(const RefG& a, int gm_opt, int walk_opt, int* gm_out) {
  const int tilesM = (a.M + 255) / 256, tilesN = (a.N + 255) / 256;
  const int nt = tilesM * tilesN;
  const int gm = (gm_opt >= 1 && gm_opt <= 32 ? gm_opt : 8) | (walk_opt == 1 ? 1 << 16 : 0);
  *gm_out = gm;
  return rec(0, dim3(nt < 256 ? nt : 256), dim3(512), tilesM, tilesN);
}
static Launch ref_gru_step16(const RefBatch& b, int gm_opt, int* gm_out) {
  const int tm = (b.p[0].M + 127) / 128, tj = b.Hp / 64;
  const int gm = gm_opt >= 1 && gm_opt <= 64 ? gm_opt : 4;
  *gm_out = gm;
  return rec(0, dim3(tm * tj, b.n), dim3(256), tm, tj);
}
static bool ref_mid_cols_ok(const RefG& a) { return a.N % 288 == 0; }
static Launch ref_gemm_h3s_mid(const RefG& a) {
  const int tilesM = (a.M + 127) / 128, tilesN = a.N / 288;
  return rec(0, dim3(tilesM * tilesN, 1), dim3(768), tilesM, tilesN);
}

// plan.hip select_kernels: the two lines after `bool g0mid = ... && (9 * Hp) % 288 == 0`
static bool ref_g0mid(long BT, int Hp) {
  const long rt = (BT + 127) / 128;
  const long r_mid = (rt * (9 * Hp / 288) + 255) / 256, r_old = (rt * ((9 * Hp + 127) / 128) + 255) / 256;
  return 2.1 * (double)r_mid <= (double)r_old + 0.15;
}

// smpl.hip launch_smpl_skin (kNV = 6890, kSkinPG = 32)
static Launch ref_smpl_skin(int N) {
  const int vb = (6890 + 255) / 256;
  int pg = (int)((long)N * vb / 512);
  pg = pg < 1 ? 1 : (pg > 32 ? 32 : pg);
  dim3 grid(vb, (N + pg - 1) / pg);
  return rec(0, grid, dim3(256), 0, pg);
}

// ------------------------------------------------------------------ comparison
static const char* g_variant = "default";
static void same(const char* rule, long p0, long p1, long p2, const Launch& got, const Launch& ref) {
  if (got.kernel != ref.kernel || got.gx != ref.gx || got.gy != ref.gy || got.gz != ref.gz || got.threads != ref.threads || got.a0 != ref.a0 || got.a1 != ref.a1)
    FAIL("%s(%ld, %ld, %ld) [%s]: kernel %d grid (%u, %u, %u) threads %u args (%d, %d), reference kernel %d grid (%u, %u, %u) threads %u args (%d, %d)", rule, p0, p1, p2,
         g_variant, got.kernel, got.gx, got.gy, got.gz, got.threads, got.a0, got.a1, ref.kernel, ref.gx, ref.gy, ref.gz, ref.threads, ref.a0, ref.a1);
}
static void same_v(const char* rule, long p0, long p1, long p2, double got, double ref) {
  if (got != ref) FAIL("%s(%ld, %ld, %ld) [%s]: %.17g, reference %.17g", rule, p0, p1, p2, g_variant, got, ref);
}

// every rule that takes (rows, columns, products)
static void check_product(int M, int N, int n, const Options& o) {
  const RefBatch b{{{M, N}, {M, N}, {M, N}}, n, 0};
  const RefG g{M, N, 0, n};
  RefCosts c;
  const Launch r = ref_gemm_h3(b, o, &c);
  same("h3_product_shape", M, N, n, h3_product_shape(M, N, n, o), r);
  if (c.c128 >= 0.) {      // the cost figures, where the launcher computed them: the same tile counts in, the same microseconds out
    const int tilesN = (N + 127) / 128;
    same_v("h3_cost128", M, N, n, h3_cost128((double)((M + 127) / 128) * tilesN * n), c.c128);
    same_v("h3_cost64", M, N, n, h3_cost64((double)((M + 63) / 64) * tilesN * n), c.c64);
    if (c.c192 >= 0.) same_v("h3_cost192", M, N, n, h3_cost192((double)((M + 127) / 128) * (N / 192) * n), c.c192);
  }
  same("skinny_h3_product_shape", M, N, n, skinny_h3_product_shape(M, N, n, o), ref_skinny_gemm_h3_batch(M, N, b, o));
  same("f32_tiles_shape", M, N, n, f32_tiles_shape(M, N, o), ref_gemm_tiles(g, o));
  for (int nw1 : {4, 8}) same("skinny_f32_product_shape", M, N, nw1, skinny_f32_product_shape(M, N, nw1), ref_skinny_gemm(g, nw1));
  int gm = 0;
  same("h3s16c_shape", M, N, n, h3s16c_shape(M, N), ref_gemm_h3s16c(g, o.s16_gm, o.s16_walk, &gm));
  same_v("h3s16c_gm_arg", o.s16_gm, o.s16_walk, 0, h3s16c_gm_arg(o.s16_gm, o.s16_walk), gm);
  same_v("h3s_mid_cols_ok", M, N, n, h3s_mid_cols_ok(N), ref_mid_cols_ok(g));
  if (ref_mid_cols_ok(g)) same("h3s_mid_shape", M, N, n, h3s_mid_shape(M, N), ref_gemm_h3s_mid(g));
  for (int permT : {0, 16})      // rows = M, padded K = N
    same_v("split_rows_few_ok", M, N, permT, split_rows_few_ok(M, N, permT, o), ref_split_rows_few_ok(M, N, permT, o));
  same("skin_shape", M, 0, 0, skin_shape(M), ref_smpl_skin(M));      // M persons
}

// every rule that takes (rows, padded hidden size, directions)
static void check_step(int M, int Hp, int n, const Options& o) {
  const RefBatch b{{{M, 0}, {M, 0}, {M, 0}}, n, Hp};
  const RefG g{M, 0, Hp, n};
  same("gru_h3_shape", M, Hp, n, gru_h3_shape(M, Hp, n), ref_gru_h3(b));
  same("skinny_h3_step_shape", M, Hp, n, skinny_h3_step_shape(M, Hp, n), ref_skinny_gru_h3(b));
  for (int nw1 : {4, 8}) same("skinny_f32_step_shape", M, Hp, n, skinny_f32_step_shape(M, Hp, n, nw1), ref_skinny_gru(g, nw1));
  same("gru_seq_shape", M, Hp, n, gru_seq_shape(M, Hp, n), ref_gru_seq(g));
  same_v("gru_seq_row_tiles", M, Hp, n, gru_seq_row_tiles(M), ref_gru_seq(g).kernel);
  for (int cus : {0, 47, 48, 127, 128, 191, 192, 256, 304})
    for (int T : {1, 2, 16, 36, 37})
      same_v("gru_seq_ok", M, Hp, n * 1000 + T, gru_seq_ok(n, M, Hp, T, o, cus), ref_gru_seq_ok(n, M, Hp, T, o, cus));
  int gm = 0;
  same("gru_step16_shape", M, Hp, n, gru_step16_shape(M, Hp, n), ref_gru_step16(b, o.gru_gm, &gm));
  same_v("gru_step16_gm", o.gru_gm, 0, 0, gru_step16_gm(o.gru_gm), gm);
  same_v("g0_mid_fewer_rounds", M, Hp, 0, g0_mid_fewer_rounds(M, Hp), ref_g0mid(M, Hp));      // M = B * T rows
  same_v("gru_seq_shape_ok", Hp, 0, 0, gru_seq_shape_ok(Hp), ref_gru_seq_shape_ok(Hp));
  same_v("gru_first16_shape_ok", Hp, 0, 0, gru_first16_shape_ok(Hp), ref_gru_first16_shape_ok(Hp));
  same_v("gru_seq_gran_rows", o.seq_gran_max_m, 0, 0, gru_seq_gran_rows(o), ref_gru_seq_gran_rows(o));
  same_v("gemm_skinny_max_m", o.skinny_max_m_gemm, o.skinny_max_m, 0, gemm_skinny_max_m(o), ref_gemm_skinny_max_m(o));
}

// ------------------------------------------------------------------ the outcomes the documents state (default options), independent of ref_*
static void expect(const char* what, const Launch& l, int kernel, unsigned gx, unsigned gy, unsigned gz, unsigned threads) {
  if (l.kernel != kernel || l.gx != gx || l.gy != gy || l.gz != gz || l.threads != threads)
    FAIL("literal %s: kernel %d grid (%u, %u, %u) threads %u, stated kernel %d grid (%u, %u, %u) threads %u", what, l.kernel, l.gx, l.gy, l.gz, l.threads, kernel, gx, gy, gz, threads);
}
static int check_literals() {
  const Options o;
  int rows = 0;
  // blocked-plane product (M, N, products): tile, workgroups per product
  expect("444 x 9216", h3_product_shape(444, 9216, 1, o), kH3Tile64x128, 504, 1, 1, 256); ++rows;
  expect("128 x 9216", h3_product_shape(128, 9216, 1, o), kH3Tile64x128, 144, 1, 1, 256); ++rows;
  expect("288 x 3072", h3_product_shape(288, 3072, 1, o), kH3Tile64x128, 120, 1, 1, 256); ++rows;
  expect("1024 x 3072", h3_product_shape(1024, 3072, 1, o), kH3Tile128x128, 192, 1, 1, 512); ++rows;
  expect("2 x (1024 x 3072)", h3_product_shape(1024, 3072, 2, o), kH3Tile128x192, 128, 2, 1, 512); ++rows;
  expect("1536 x 3072", h3_product_shape(1536, 3072, 1, o), kH3Tile128x192, 192, 1, 1, 512); ++rows;
  expect("2048 x 9216", h3_product_shape(2048, 9216, 1, o), kH3Tile128x192, 768, 1, 1, 512); ++rows;
  expect("2049 x 9216", h3_product_shape(2049, 9216, 1, o), kH3Tile256x128, 648, 1, 1, 512); ++rows;
  // two-accumulator step (M, Hp, directions): 5 x 16 x 2 = 160 blocks of 128 rows -> 64-row blocks; 240 -> 128-row blocks
  expect("step 640 x 1024 x 2", gru_h3_shape(640, 1024, 2), kGruH3Rows64, 160, 2, 1, 256); ++rows;
  expect("step 640 x 1024 x 3", gru_h3_shape(640, 1024, 3), kGruH3Rows128, 80, 3, 1, 512); ++rows;
  // width-first split product (rows, columns)
  expect("skinny 64 x 160", skinny_h3_product_shape(64, 160, 1, o), kSkinnyH3_1x1w8, 10, 4, 1, 512); ++rows;
  expect("skinny 37 x 160", skinny_h3_product_shape(37, 160, 1, o), kSkinnyH3_1x1w8, 10, 3, 1, 512); ++rows;
  expect("skinny 16 x 2048", skinny_h3_product_shape(16, 2048, 1, o), kSkinnyH3_1x1w8, 128, 1, 1, 512); ++rows;
  expect("skinny 20 x 3072", skinny_h3_product_shape(20, 3072, 1, o), kSkinnyH3_2x1w4, 192, 1, 1, 256); ++rows;
  expect("skinny 48 x 2048", skinny_h3_product_shape(48, 2048, 1, o), kSkinnyH3_4x1w8, 128, 1, 1, 512); ++rows;
  expect("skinny 74 x 3072", skinny_h3_product_shape(74, 3072, 1, o), kSkinnyH3_3, 64, 2, 1, 256); ++rows;
  expect("skinny 192 x 3072", skinny_h3_product_shape(192, 3072, 1, o), kSkinnyH3_4, 64, 3, 1, 256); ++rows;
  expect("skinny 128 x 9216", skinny_h3_product_shape(128, 9216, 1, o), kSkinnyH3_4, 192, 2, 1, 256); ++rows;
  // exact-fp32 tiles: 32 x 32 = 1024 blocks of 128 rows -> 64-row tiles; 33 x 32 -> 128-row tiles
  expect("f32 4096 x 4096", f32_tiles_shape(4096, 4096, o), kF32Rows64, 64 * 32, 1, 1, 256); ++rows;
  expect("f32 4097 x 4096", f32_tiles_shape(4097, 4096, o), kF32Rows128, 33 * 32, 1, 1, 256); ++rows;
  // gru_seq_kernel row tiles
  const int seq_rows[] = {16, 17, 32, 33, 48, 49, 64}, seq_tiles[] = {1, 2, 2, 3, 3, 4, 4};
  for (int i = 0; i < 7; ++i, ++rows)
    if (gru_seq_row_tiles(seq_rows[i]) != seq_tiles[i]) FAIL("literal gru_seq_row_tiles(%d) = %d, stated %d", seq_rows[i], gru_seq_row_tiles(seq_rows[i]), seq_tiles[i]);
  if (kChipCUs != 256) FAIL("kChipCUs = %d", kChipCUs);
  return rows;
}

// ------------------------------------------------------------------ option variants: the default, each A/B switch alone, each forced tile, each threshold moved
struct Variant { const char* name; std::function<void(Options&)> set; };
static const Variant kVariants[] = {
    {"default", [](Options&) {}},
    {"H3_TILE64=0", [](Options& o) { o.h3_tile64 = 0; }}, {"H3_TILE192=0", [](Options& o) { o.h3_tile192 = 0; }},
    {"H3_TILE64=0 H3_TILE192=0", [](Options& o) { o.h3_tile64 = 0; o.h3_tile192 = 0; }},
    {"H3_TILE=64", [](Options& o) { o.h3_tile = 64; }}, {"H3_TILE=192", [](Options& o) { o.h3_tile = 192; }}, {"H3_TILE=256", [](Options& o) { o.h3_tile = 256; }},
    {"H3_TILE=128", [](Options& o) { o.h3_tile = 128; }},      // not a forced shape: the cost model
    {"SKINNY_MT1=0", [](Options& o) { o.skinny_mt1 = 0; }}, {"SKINNY_W8=0", [](Options& o) { o.skinny_w8 = 0; }}, {"SKINNY_NARROW64=0", [](Options& o) { o.skinny_narrow64 = 0; }},
    // SKINNY_NT1_BELOW against column blocks x products: 2048 columns = 43 blocks of 48, 3072 = 64, 1536 x 3 = 96
    {"SKINNY_NT1_BELOW=0", [](Options& o) { o.skinny_nt1_below = 0; }}, {"SKINNY_NT1_BELOW=43", [](Options& o) { o.skinny_nt1_below = 43; }},
    {"SKINNY_NT1_BELOW=44", [](Options& o) { o.skinny_nt1_below = 44; }}, {"SKINNY_NT1_BELOW=64", [](Options& o) { o.skinny_nt1_below = 64; }},
    {"SKINNY_NT1_BELOW=65", [](Options& o) { o.skinny_nt1_below = 65; }}, {"SKINNY_NT1_BELOW=97", [](Options& o) { o.skinny_nt1_below = 97; }},
    {"SKINNY_NT1_BELOW=1000", [](Options& o) { o.skinny_nt1_below = 1000; }},
    // GEMM_HALF_MAX_BLOCKS: 8192 x 2048 is 64 x 16 = 1024 blocks of 128 rows
    {"GEMM_HALF_MAX_BLOCKS=0", [](Options& o) { o.gemm_half_max_blocks = 0; }}, {"GEMM_HALF_MAX_BLOCKS=1023", [](Options& o) { o.gemm_half_max_blocks = 1023; }},
    {"GEMM_HALF_MAX_BLOCKS=1025", [](Options& o) { o.gemm_half_max_blocks = 1025; }},
    {"SPLIT_FEW_MAX_ROWS=1023", [](Options& o) { o.split_few_max_rows = 1023; }}, {"SPLIT_FEW_MAX_ROWS=1025", [](Options& o) { o.split_few_max_rows = 1025; }},
    {"S16_GM=0", [](Options& o) { o.s16_gm = 0; }}, {"S16_GM=1", [](Options& o) { o.s16_gm = 1; }}, {"S16_GM=32", [](Options& o) { o.s16_gm = 32; }},
    {"S16_GM=33", [](Options& o) { o.s16_gm = 33; }}, {"S16_WALK=1", [](Options& o) { o.s16_walk = 1; }}, {"S16_WALK=2", [](Options& o) { o.s16_walk = 2; }},
    {"GRU_GM=0", [](Options& o) { o.gru_gm = 0; }}, {"GRU_GM=1", [](Options& o) { o.gru_gm = 1; }}, {"GRU_GM=64", [](Options& o) { o.gru_gm = 64; }},
    {"GRU_GM=65", [](Options& o) { o.gru_gm = 65; }},
    {"SEQ_MAX_M=0", [](Options& o) { o.seq_max_m = 0; }}, {"SEQ_MAX_M=16", [](Options& o) { o.seq_max_m = 16; }}, {"SEQ_MAX_M=63", [](Options& o) { o.seq_max_m = 63; }},
    {"SEQ_MAX_M=65", [](Options& o) { o.seq_max_m = 65; }}, {"SEQ_MAX_M=4096", [](Options& o) { o.seq_max_m = 4096; }},
    {"SEQ_GRAN_MAX_M=0", [](Options& o) { o.seq_gran_max_m = 0; }}, {"SEQ_GRAN_MAX_M=3", [](Options& o) { o.seq_gran_max_m = 3; }},
    {"SEQ_GRAN_MAX_M=5", [](Options& o) { o.seq_gran_max_m = 5; }},
    {"SKINNY_MAX_M_GEMM=0", [](Options& o) { o.skinny_max_m_gemm = 0; }}, {"SKINNY_MAX_M_GEMM=100", [](Options& o) { o.skinny_max_m_gemm = 100; }},
};

static const int kM[] = {1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 74, 128, 129, 192, 193, 288, 444, 640, 768, 1024, 1030, 1536, 2048, 2049, 4096, 8192, 131072};
static const int kN[] = {16, 160, 384, 640, 1152, 1536, 2048, 3072, 9216, 20736};
static const int kProducts[] = {1, 2, 3};
static const int kHp[] = {64, 192, 256, 1024, 2048};
// A shape on each side of every threshold the cross product above does not straddle (products: M, N, n; steps: M, Hp, n)
static const int kEdgeProducts[][3] = {
    {2048, 16256, 1}, {2048, 16384, 1}, {2049, 16256, 1},            // 8 x 127 = 1016 | 8 x 128 = 1024 tiles of 256 rows (< 1024), and one row more
    {1024, 8064, 3}, {1024, 10880, 3}, {1024, 10944, 3},             // 4 x 63 x 3 = 756 | 4 x 85 x 3 = 1020 | 4 x 86 x 3 = 1032
    {64, 32768, 1}, {65, 32768, 1}, {64, 32896, 1},                  // 256 | 512 | 257 workgroups of 64 rows: the first CU sharing (1.55 rounds)
    {128, 25344, 1}, {128, 25472, 1}, {128, 25600, 1},               // 396 | 398 | 400 workgroups of 64 rows: either side of 1.55 x 256 = 396.8
    {640, 9216, 1}, {576, 9216, 1}, {704, 9216, 1},                  // c64 = 92.8 | 83.5 | 102.1 us against 0.9 x 94 = 84.6 (H3_TILE192=0 reaches it)
    {256, 16320, 1}, {256, 16384, 1}, {256, 16448, 1}, {256, 16512, 1},   // 255 | 256 | 257 | 258 tiles of 128 x 128: one round | two
    {384, 16384, 1}, {384, 16320, 1}, {384, 16512, 1},               // 256 tiles of 128 x 192 (N % 192 == 0: 16320, 16512) against 384 of 128 x 128
    {16, 4096, 1}, {16, 4112, 1}, {32, 2048, 1}, {32, 2064, 1}, {33, 2048, 1},   // 256 | 257 blocks of 16 x 16; 128 | 129 16-column blocks at 32 / 33 rows
    {64, 4560, 1}, {64, 4608, 1}, {64, 4609, 1},                     // 95 | 96 | 97 column blocks of 48: the literal 96 of the 33..64-row rule
    {32, 4560, 1}, {32, 4608, 1}, {32, 4609, 1}, {65, 4560, 1},
    {80, 3072, 1}, {81, 3072, 1}, {96, 3072, 1}, {97, 3072, 1}, {144, 3072, 1}, {145, 3072, 1},   // 5 | 6 | 7 | 9 | 10 row tiles over the fewest passes
    {4096, 4096, 1}, {4097, 4096, 1},                                // 1024 | 1056 exact-fp32 blocks of 128 rows
    {65536, 65536, 1}, {65280, 256, 1}, {65281, 256, 1}, {65536, 256, 1},   // 255 | 256 tiles of 256 x 256: the persistent product's grid
    {73, 16, 1}, {74, 16, 1}, {75, 16, 1}, {606, 16, 1}, {607, 16, 1}, {637, 16, 1},   // persons per skinning block: 1 | 2; 31 | 32 | capped
    {1023, 4096, 1}, {1025, 4096, 1}, {1024, 4128, 1},               // one workgroup per row: rows either side of 1024, padded K above 4096
};
static const int kEdgeSteps[][3] = {
    {640, 1024, 2}, {641, 1024, 2}, {1280, 1024, 1}, {1281, 1024, 1}, {384, 1152, 3}, {385, 1152, 3}, {2560, 256, 1}, {2561, 256, 1}, {896, 1472, 1},   // 160 | 161 (7 x 23) and more blocks of 128 rows
    {512, 1024, 1}, {8191, 1024, 1}, {1152, 1024, 1}, {1153, 1024, 1}, {1024, 256, 1}, {3585, 64, 1},      // rounds of 128 x 288 against 128 x 128 tiles
    {4, 1024, 3}, {5, 1024, 3}, {64, 768, 3}, {64, 512, 2}, {64, 1280, 1}, {1, 1024, 4}, {0, 1024, 1},      // the persistent kernel's shapes
};

static long time_ns(const std::function<long()>& f, int reps) {
  const auto t0 = std::chrono::steady_clock::now();
  long sink = 0;
  for (int i = 0; i < reps; ++i) sink += f();
  const auto t1 = std::chrono::steady_clock::now();
  if (sink == 42) std::printf(" ");
  return (long)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}

// the decisions a forward of B = 1 windows x T frames makes (L = 2, Hp = 1024): three width-first products per layer, the persistent kernel per layer,
// the tail / collapsed regressor products
static int time_decisions() {
  const int reps = 200000;
  volatile int vT = 16;
  Options o;
  const long t_new = time_ns([&]() {
    const int T = vT;
    long k = 0;
    k += skinny_h3_product_shape(T, 9216, 1, o).gx + skinny_h3_product_shape(16 * T, 3072, 2, o).gy + skinny_h3_product_shape(1, 3072, 1, o).gx;
    k += gru_seq_ok(3, 1, 1024, T, o, 256) + gru_seq_shape(1, 1024, 3).gx + gru_seq_ok(2, 1, 1024, T, o, 256) + gru_seq_shape(1, 1024, 2).gx;
    k += skinny_h3_product_shape(1, 2048, 1, o).kernel + skinny_h3_product_shape(1, 160, 1, o).kernel + h3_product_shape(16 * T, 3072, 2, o).kernel;
    return k;
  }, reps);
  const long t_ref = time_ns([&]() {
    const int T = vT;
    long k = 0;
    RefCosts c;
    const RefBatch b1{{}, 1, 0}, b2{{{16 * T, 3072}}, 2, 0};
    k += ref_skinny_gemm_h3_batch(T, 9216, b1, o).gx + ref_skinny_gemm_h3_batch(16 * T, 3072, b2, o).gy + ref_skinny_gemm_h3_batch(1, 3072, b1, o).gx;
    k += ref_gru_seq_ok(3, 1, 1024, T, o, 256) + ref_gru_seq(RefG{1, 0, 1024, 3}).gx + ref_gru_seq_ok(2, 1, 1024, T, o, 256) + ref_gru_seq(RefG{1, 0, 1024, 2}).gx;
    k += ref_skinny_gemm_h3_batch(1, 2048, b1, o).kernel + ref_skinny_gemm_h3_batch(1, 160, b1, o).kernel + ref_gemm_h3(b2, o, &c).kernel;
    return k;
  }, reps);
  std::printf("10 decisions of a B = 1 forward, %d repetitions: shapes.h %.1f ns, ref_* %.1f ns per set\n", reps, (double)t_new / reps, (double)t_ref / reps);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return time_decisions();
  long combos = 0;
  for (const Variant& v : kVariants) {
    Options o;
    v.set(o);
    g_variant = v.name;
    for (int M : kM)
      for (int N : kN)
        for (int n : kProducts) { check_product(M, N, n, o); ++combos; }
    for (int M : kM)
      for (int Hp : kHp)
        for (int n : kProducts) { check_step(M, Hp, n, o); ++combos; }
    for (const auto& e : kEdgeProducts) { check_product(e[0], e[1], e[2], o); ++combos; }
    for (const auto& e : kEdgeSteps) { check_step(e[0], e[1], e[2], o); ++combos; }
  }
  // the option table names every int field once, and only those
  {
    Options o;
    const size_t n = sizeof(kOptNames) / sizeof(kOptNames[0]);
    for (size_t i = 0; i < n; ++i) {
      char env[64];
      std::snprintf(env, sizeof(env), "TEPOSE_%s", kOptNames[i].name);
      if (option_field(o, kOptNames[i].name) != &(o.*(kOptNames[i].field)) || option_field(o, env) != &(o.*(kOptNames[i].field))) FAIL("option_field(%s)", kOptNames[i].name);
      for (size_t j = 0; j < i; ++j)
        if (kOptNames[i].field == kOptNames[j].field || std::strcmp(kOptNames[i].name, kOptNames[j].name) == 0) FAIL("option %s listed twice", kOptNames[i].name);
    }
    if (option_field(o, "NO_SUCH") || option_field(o, nullptr)) FAIL("option_field of an unknown name");
    if (n * sizeof(int) + sizeof(unsigned long long) != sizeof(Options)) FAIL("%zu option names for %zu bytes of Options", n, sizeof(Options));
  }
  combos += check_literals();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok %ld\n", combos);
  return 0;
}
