// Launch shapes: which instantiation of a kernel family a shape gets, with which grid and block -- and the shape predicates of the kernel plan.
// plan.hip (select_kernels) chooses the family; the functions here decide everything below that, and a launcher is one call into this header and one
// switch over the result.  Pure functions of (shape, Options), plain C++ on options.h and formats.h: nothing from HIP is included, so the host
// compiler alone builds it, and tests/test_launch_shapes.py pins every rule -- against the expressions the launchers used to carry, and against the
// outcomes DESIGN.md states -- on a machine without a GPU.
#pragma once
#include "formats.h"
#include "options.h"

namespace tepose {

constexpr int kChipCUs = 256;    // compute units of the MI355X: the cost models below count in rounds of the chip

// What a launcher needs from a rule.  kernel: the rule's enum (0 where a family has one instantiation); a0 / a1: the integer kernel arguments the
// rule decides -- tile counts (rows, columns) everywhere but skin_shape (persons per block).
struct Launch { int kernel; unsigned gx, gy, gz, threads; int a0, a1; };

// ---------------------------------------------------------------- plan predicates
// Shape predicates of plan.hip's select_kernels: which input-split kernel, which first-step kernel, the persistent recurrent kernel.  The launchers
// take the plan's choice as an argument; launch_gru_first and launch_gru_seq still refuse a choice their shape cannot take.
inline bool split_rows_few_ok(long rows, int Kp, int permT, const Options& o) { return rows <= o.split_few_max_rows && Kp <= 4096 && !permT; }
inline bool gru_first16_shape_ok(int Hp) { return Hp % 128 == 0; }
inline bool gru_seq_shape_ok(int Hp) { return Hp % 256 == 0 && Hp <= 1024; }
inline int gemm_skinny_max_m(const Options& o) { return o.skinny_max_m_gemm >= 0 ? o.skinny_max_m_gemm : o.skinny_max_m; }

// ---------------------------------------------------------------- products on blocked planes (gemm_h3_kernel, gemm_h3.hip)
enum H3Tile { kH3Tile64x128, kH3Tile128x128, kH3Tile128x192, kH3Tile256x128 };      // block tile rows x columns
inline Launch h3_tile_launch(H3Tile k, int tm, int tn, int n) { return {k, (unsigned)(tm * tn), (unsigned)n, 1u, k == kH3Tile64x128 ? 256u : 512u, tm, tn}; }
inline double chip_rounds(double workgroups) { return (double)(long)((workgroups + (kChipCUs - 1.)) / (double)kChipCUs); }     // whole rounds of the chip
// us per launch of w tiles.  Measured per round at K = 2144 (profiles/r05_mid_rows_gemm.txt): a 128-row tile 47 us, one workgroup per CU; a 64-row
// tile 33 us, and 33 us x workgroups / 256 once they share CUs (more than one 64-row workgroup per CU: the first sharing costs 1.55 rounds whatever
// the count -- 288 workgroups 51.8 us, 384: 53.0, 504: 62.8).  A 128 x 192 tile's time follows its operand bytes, (128 + 192) against (128 + 128)
// rows per K-tile, measured 70 us per round at K = 2048 (profiles/r06_README.md).
inline double h3_cost128(double w) { return 47. * chip_rounds(w); }
inline double h3_cost64(double w) {
  const double rounds = w / (double)kChipCUs, first_sharing = 1.55;
  return 33. * (w <= (double)kChipCUs ? 1. : (rounds > first_sharing ? rounds : first_sharing));
}
inline double h3_cost192(double w) { return 70. * chip_rounds(w); }
// up to 3 products of the same M x N in one launch (launch_gemm_h3): 256 x 128 block tile, 3-stage ring of 48 KB stages, unless ...
inline Launch h3_product_shape(int M, int N, int n, const Options& o) {
  const int tilesM = (M + 255) / 256, tilesN = (N + 127) / 128;
  if (o.h3_tile == 64) return h3_tile_launch(kH3Tile64x128, (M + 63) / 64, tilesN, n);      // A/B: force a tile shape
  if (o.h3_tile == 192) return h3_tile_launch(kH3Tile128x192, (M + 127) / 128, (N + 191) / 192, n);
  if (o.h3_tile == 256) return h3_tile_launch(kH3Tile256x128, tilesM, tilesN, n);
  if (M <= 2048 && tilesM * tilesN * n < 1024) {     // few rows and < 4 rounds of 256-row tiles: 128-row
    // tiles quantise better (B=64: layer-0 projection 288 -> 576 tiles; B=64 forward 0.95 -> 0.89 ms)
    const int tm = (M + 127) / 128;
    // ... and 64-row tiles (4 waves, 72 KB ring: two workgroups per CU) where they need fewer rounds of the chip.
    // 444 x 9216: 97.8 -> 62.8 us; 128 x 9216: 44.9 -> 34.4; 288 x 3072: 44.0 -> 33.2; 1024 x 3072 stays (49.2 against 53.0).
    const int tm64 = (M + 63) / 64;
    const double w128 = (double)tm * tilesN * n, w64 = (double)tm64 * tilesN * n;
    const double c64 = h3_cost64(w64), keep128 = 0.9 * h3_cost128(w128);      // another shape has to win by a tenth
    // ... and 128 x 192 tiles (round 6) where they turn "a round and a bit" of 128 x 128 tiles into exactly one round -- the layer-1 projections of
    // cfg-B (two products of 1024 x 3072: 384 tiles of 128 x 128 = 1.5 rounds, 256 tiles of 128 x 192 = one round): 81.8 -> 72.4 us
    // (profiles/r06_README.md).  Column counts that are whole 192-column tiles only (3 Hp always is): the W planes are padded to 128 rows, not to 192.
    if (o.h3_tile192 && N % 192 == 0) {       // h3_tile192 / h3_tile64 == 0: never (A/B)
      const double c192 = h3_cost192((double)tm * (N / 192) * n);
      if (c192 < keep128 && c192 <= c64) return h3_tile_launch(kH3Tile128x192, tm, N / 192, n);
    }
    if (o.h3_tile64 && c64 < keep128) return h3_tile_launch(kH3Tile64x128, tm64, tilesN, n);
    return h3_tile_launch(kH3Tile128x128, tm, tilesN, n);
  }
  return h3_tile_launch(kH3Tile256x128, tilesM, tilesN, n);
}

// the fused two-accumulator GRU step (launch_gru_h3): block = 128 rows x (64 hidden units x 3 gates); mid-size batches: 64-row blocks (4 waves) fill more CUs
enum GruH3Rows { kGruH3Rows64, kGruH3Rows128 };
inline Launch gru_h3_shape(int M, int Hp, int n) {
  const int tilesJ = Hp / 64;
  if ((M + 127) / 128 * tilesJ * n <= 160) return {kGruH3Rows64, (unsigned)((M + 63) / 64 * tilesJ), (unsigned)n, 1u, 256u, (M + 63) / 64, tilesJ};
  return {kGruH3Rows128, (unsigned)((M + 127) / 128 * tilesJ), (unsigned)n, 1u, 512u, (M + 127) / 128, tilesJ};
}

// ---------------------------------------------------------------- width-first split kernels (skinny_h3.hip)
// skinny_gemm_h3_kernel<MT, NT, NW, KS>: MT 16-row tiles x NT 16-column tiles per block, K split over NW waves; kSkinnyH3_<MT>: <MT> with 48-column blocks
enum SkinnyH3 { kSkinnyH3_1x1w8, kSkinnyH3_2x1w8, kSkinnyH3_2x1w4, kSkinnyH3_4x1w8, kSkinnyH3_4x1w4, kSkinnyH3_1, kSkinnyH3_2, kSkinnyH3_3, kSkinnyH3_4 };
// up to 3 independent products in one launch (launch_skinny_gemm_h3_batch); maxM, maxN: the largest row / column count among them
inline Launch skinny_h3_product_shape(int maxM, int maxN, int n, const Options& o) {
  const int nt = (maxN + 47) / 48;
  const int nt1_max = o.skinny_nt1_below;
  const unsigned gx16 = (unsigned)((maxN + 15) / 16);      // 16-column blocks of the widest product
  // narrow products (the collapsed regressor product: 160 columns = 10 blocks of 16; the 2048-column tail linears at <= 16 rows): a CU takes in ~50 GB/s,
  // so the launch lasts as long as its busiest block's bytes -- one 16-row tile per block (W re-read per row tile from L2, A never clamped-and-repeated)
  // puts them on rows x more CUs: 64 rows x 160 x 3072 on 40 blocks of 392 KB instead of 10 of 960 KB
  const int rowtiles = (maxM + 15) / 16;
  if (o.skinny_mt1 != 0 && nt * n < nt1_max && (maxN + 15) / 16 * n * rowtiles <= kChipCUs) return {kSkinnyH3_1x1w8, gx16, (unsigned)rowtiles, (unsigned)n, 512u, 0, 0};
  // <= 128 16-column blocks (the 2048-column tail linears; the collapsed regressor product, N = 160: 10 blocks): 8 waves split K -- twice the weight
  // bytes in flight per CU, the block's chain of dependent weight chunks halves
  const bool w8 = o.skinny_w8 != 0 && (maxN + 15) / 16 * n <= 128;
  if (maxM <= 32 && nt * n < nt1_max)          // few rows, narrow product: 16-column blocks put a weight stream on 3x the CUs
    return {w8 ? kSkinnyH3_2x1w8 : kSkinnyH3_2x1w4, gx16, 1u, (unsigned)n, w8 ? 512u : 256u, 0, 0};
  if (maxM <= 64 && maxM > 32 && nt * n < 96 && o.skinny_narrow64 != 0)      // (a literal 96, not skinny_nt1_below: SKINNY_NARROW64 is this rule's switch)
    return {w8 ? kSkinnyH3_4x1w8 : kSkinnyH3_4x1w4, gx16, 1u, (unsigned)n, w8 ? 512u : 256u, 0, 0};
  // row tiles dealt evenly over the fewest passes of <= 4 tiles: a block never loads a clamped-and-repeated tile beyond the last one of the batch
  // (74 rows = 5 tiles: 3 + 2 instead of 4 + 1 and three repeats; 16 rows: 1 tile instead of 2)
  const int tiles = (maxM + 15) / 16, passes = (tiles + 3) / 4;
  const int mt = o.skinny_mt1 != 0 ? (tiles + passes - 1) / passes : (maxM <= 32 ? 2 : 4);
  return {mt <= 1 ? kSkinnyH3_1 : mt == 2 ? kSkinnyH3_2 : mt == 3 ? kSkinnyH3_3 : kSkinnyH3_4, (unsigned)nt, (unsigned)((tiles + mt - 1) / mt), (unsigned)n, 256u, 0, 0};
}
// the width-first GRU steps, split (skinny_gru_h3_kernel<MT>) and exact fp32 (skinny_gru_kernel), and the exact-fp32 product (skinny_gemm_kernel):
// one, two or four 16-row tiles per block, 64-row passes above 32 rows.  nw1: waves per block of the one-tile form (skinny.hip SK_NW1)
enum SkinnyRows { kSkinnyRows16, kSkinnyRows32, kSkinnyRows64 };
inline Launch skinny_h3_step_shape(int M, int Hp, int n) {
  if (M <= 32) return {kSkinnyRows32, (unsigned)(Hp / 16), 1u, (unsigned)n, 256u, 0, 0};
  return {kSkinnyRows64, (unsigned)(Hp / 16), (unsigned)((M + 63) / 64), (unsigned)n, 256u, 0, 0};
}
inline Launch skinny_f32_shape(int M, int blocks_x, int n, int nw1) {
  if (M <= 16) return {kSkinnyRows16, (unsigned)blocks_x, 1u, (unsigned)n, (unsigned)(64 * nw1), 0, 0};
  if (M <= 32) return {kSkinnyRows32, (unsigned)blocks_x, 1u, (unsigned)n, 256u, 0, 0};
  return {kSkinnyRows64, (unsigned)blocks_x, (unsigned)((M + 63) / 64), (unsigned)n, 256u, 0, 0};
}
inline Launch skinny_f32_product_shape(int M, int N, int nw1) { return skinny_f32_shape(M, (N + 47) / 48, 1, nw1); }      // 48-column blocks
inline Launch skinny_f32_step_shape(int M, int Hp, int ndir, int nw1) { return skinny_f32_shape(M, Hp / 16, ndir, nw1); }  // 16 hidden units x 3 gates

// ---------------------------------------------------------------- exact-fp32 tiles (gemm_f32_kernel, gemm.hip)
// 64-row tiles (3 blocks per CU) when 128-row tiles would not fill the 512 block slots twice:
// finer quantisation for the mid-size batches (measured: +4-6 % at B = 64-128, +4.5 % at B = 1024, neutral at B = 8192)
enum F32Rows { kF32Rows64, kF32Rows128 };
inline Launch f32_tiles_shape(int M, int N, const Options& o) {
  const int tilesN = (N + 127) / 128, tiles128 = (M + 127) / 128;
  if (tiles128 * tilesN <= o.gemm_half_max_blocks) return {kF32Rows64, (unsigned)((M + 63) / 64 * tilesN), 1u, 1u, 256u, (M + 63) / 64, tilesN};
  return {kF32Rows128, (unsigned)(tiles128 * tilesN), 1u, 1u, 256u, tiles128, tilesN};
}

// ---------------------------------------------------------------- the persistent recurrent kernel (gru_seq_kernel, gru_seq.hip)
constexpr int kSeqMaxT = 36;             // the table travels in the kernel arguments (4 KB)
constexpr size_t kSeqGranRows = 4;       // granule mode serves <= 4 rows (gru_seq_gran_rows)
// rows up to which the state travels as tagged granules (Options::seq_gran_max_m, at most the kernel's granule capacity; 0: never)
inline int gru_seq_gran_rows(const Options& o) { return o.seq_gran_max_m > (int)kSeqGranRows ? (int)kSeqGranRows : o.seq_gran_max_m; }
// usable for this layer shape on a device of `cus` CUs (gru_seq.hip device_cus)?  Every workgroup must be resident at once (one per CU).
inline bool gru_seq_ok(int ndir, int M, int Hp, int T, const Options& o, int cus) {
  const int max_m = o.seq_max_m > 64 ? 64 : o.seq_max_m;
  return M >= 1 && M <= max_m && T >= 2 && T <= kSeqMaxT && gru_seq_shape_ok(Hp) && ndir >= 1 &&
         ndir <= 3 && ndir * (Hp / 16) <= cus;
}
// 16-row tiles per workgroup.  33..48 rows (37 clips in lock-step): three tiles -- a quarter less state through the L2 port per step than four.
// (Round 2 had an opt-in row split for 2-direction layers -- two workgroups per unit slice, 256 workgroups, -15 us per forward at B = 64 -- removed in
// round 5: it needs EVERY CU of the chip resident at once, which a second process's launch on the same GPU can deny until the bounded wait expires.)
inline int gru_seq_row_tiles(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 48 ? 3 : 4; }
inline Launch gru_seq_shape(int M, int Hp, int ndir) { return {gru_seq_row_tiles(M), (unsigned)(Hp / 16), 1u, (unsigned)ndir, 512u, 0, 0}; }   // kernel: the row tiles

// ---------------------------------------------------------------- scaled planes of large batches (gemm_h3s16c.hip, gru_step16.hip, gemm_h3s.hip)
// the barrier-free persistent product: 256 x 256 tiles handed to at most one workgroup per CU
inline Launch h3s16c_shape(int M, int N) {
  const int tilesM = (M + 255) / 256, tilesN = (N + 255) / 256, nt = tilesM * tilesN;
  return {0, (unsigned)(nt < kChipCUs ? nt : kChipCUs), 1u, 1u, 512u, tilesM, tilesN};
}
// its GM argument: row tiles per XCD group of the walk (the 32 workgroups of an XCD take GM x 32 / GM tiles at a time; Options::s16_gm), and the walk
// (Options::s16_walk; walk.h) in the upper half: the kernels keep their parameter lists
inline int h3s16c_gm_arg(int gm_opt, int walk_opt) { return (gm_opt >= 1 && gm_opt <= 32 ? gm_opt : 8) | (walk_opt == 1 ? 1 << 16 : 0); }
// the fused step: 128 rows x 64 hidden units per workgroup; GM = tile rows per XCD group (Options::gru_gm): the 64 workgroups resident on an XCD cover
// GM row tiles x 64 / GM unit tiles of one direction
inline Launch gru_step16_shape(int M, int Hp, int n) { return {0, (unsigned)((M + 127) / 128 * (Hp / 64)), (unsigned)n, 1u, 256u, (M + 127) / 128, Hp / 64}; }
inline int gru_step16_gm(int gm_opt) { return gm_opt >= 1 && gm_opt <= 64 ? gm_opt : 4; }
// Mid-size products (a few hundred to a few thousand rows) whose N is a multiple of 288 -- the stacked layer-0 block, 9 Hp
// columns: 128 x 288 tiles, 12 waves of 32 x 96 (three per SIMD).  B * T = 1024 rows x 9216 columns are exactly 256 tiles
// = one round of the chip, where 128 x 128 tiles of the two-accumulator kernel make 576 = 2.25 rounds.
inline bool h3s_mid_cols_ok(int N) { return N % 288 == 0; }
inline Launch h3s_mid_shape(int M, int N) { return {0, (unsigned)((M + 127) / 128 * (N / 288)), 1u, 1u, 768u, (M + 127) / 128, N / 288}; }
// select_kernels' g0mid: the 128 x 288 tiles for a layer-0 projection of BT rows x 9 Hp columns where they need less time in whole rounds of the
// chip than 128 x 128 tiles (a 128 x 288 tile takes ~2.1x a 128 x 128 one)
inline bool g0_mid_fewer_rounds(long BT, int Hp) {
  const long rt = (BT + 127) / 128;
  const long r_mid = (rt * (9 * Hp / 288) + (kChipCUs - 1)) / kChipCUs, r_old = (rt * ((9 * Hp + 127) / 128) + (kChipCUs - 1)) / kChipCUs;
  return 2.1 * (double)r_mid <= (double)r_old + 0.15;
}

// ---------------------------------------------------------------- skinning (smpl_skin_kernel / smpl_skin4_kernel, smpl.hip)
constexpr int kSkinPG = 32;
// persons per block (a1): up to kSkinPG (the per-vertex weights are loaded once per block), fewer for small batches so
// that the grid still covers the chip (N = 64: 27 x 22 blocks instead of 27 x 2: 36 -> 8 us)
inline Launch skin_shape(int N) {
  const int vb = (kNV + 255) / 256;
  int pg = (int)((long)N * vb / 512);
  pg = pg < 1 ? 1 : (pg > kSkinPG ? kSkinPG : pg);
  return {0, (unsigned)vb, (unsigned)((N + pg - 1) / pg), 1u, 256u, 0, pg};
}

// ---------------------------------------------------------------- SMPL backward (smpl_bwd.hip)
constexpr int kBwdSrc = 54;                 // sources of the 49 joints: 24 posed joints | 21 picked vertices | 9 regressed rows
// skinning backward (smpl_skin_bwd_kernel): thread = vertex, 512 vertices per workgroup, persons looped.  A workgroup leaves one 24 x 12 partial of the
// transform gradient per person: 14 partials of 288 floats, summed in ascending workgroup order by the chain kernel.
constexpr int kBwdSkinVB = 512;
constexpr int kBwdSkinBlocks = (kNV + kBwdSkinVB - 1) / kBwdSkinVB;
constexpr int kBwdSkinSlice = 25;           // vertices one reducing thread sums: 21 slices x 24 joints = 504 of the 512 threads
constexpr int kBwdSkinSlices = (kBwdSkinVB + kBwdSkinSlice - 1) / kBwdSkinSlice;
static_assert(kBwdSkinSlices * kNJ <= kBwdSkinVB, "one reducing thread per (slice, joint)");
// persons per block (a1), as skin_shape: fewer for small batches so that the grid covers the chip
inline Launch skin_bwd_shape(int N) {
  int pg = (int)((long)N * kBwdSkinBlocks / 512);
  pg = pg < 1 ? 1 : (pg > kSkinPG ? kSkinPG : pg);
  return {0, (unsigned)kBwdSkinBlocks, (unsigned)((N + pg - 1) / pg), 1u, (unsigned)kBwdSkinVB, 0, pg};
}
// blend shapes backward (smpl_blend_bwd_kernel<PT>): g_f[N,224] = g_vposed[N,20670] x blendW[20670,224], K = 20670 split over workgroups in whole
// chunks of 64 table rows.  A workgroup owns PT persons x all 224 columns (2 adjacent columns per thread) over a0 chunks and writes one partial
// [PT,224]; gx = splits, gy = person tiles.  The split count puts eight workgroups of 2 waves on every CU (four waves per SIMD hide each other's table
// and scalar loads; profiles/smpl_backward.txt) and never exceeds the chunk count: N <= 192: 323 splits of one chunk; N = 450: 108 x 15 tiles; N = 8192: 8 x 256.
constexpr int kBwdBlendRows = 3 * kNV;      // the product's K: table rows (vertex coordinates)
constexpr int kBwdChunk = 64;
constexpr int kBwdChunks = (kBwdBlendRows + kBwdChunk - 1) / kBwdChunk;
enum BlendBwdTile { kBlendBwd8, kBlendBwd32 };                  // persons per workgroup
inline int blend_bwd_persons(int kernel) { return kernel == kBlendBwd8 ? 8 : 32; }
inline Launch blend_bwd_shape(int N) {
  const int kernel = N <= 8 ? kBlendBwd8 : kBlendBwd32, pt = blend_bwd_persons(kernel);
  const int tiles = (N + pt - 1) / pt;
  int splits = (8 * kChipCUs + tiles - 1) / tiles;
  splits = splits < 1 ? 1 : (splits > kBwdChunks ? kBwdChunks : splits);
  const int per = (kBwdChunks + splits - 1) / splits;           // chunks per split
  splits = (kBwdChunks + per - 1) / per;                        // no empty split
  return {kernel, (unsigned)splits, (unsigned)tiles, 1u, 128u, per, 0};
}
// one wave per person, four per block (smpl_chain_bwd_kernel); one block of 192 threads per person (smpl_joints_bwd_kernel); one thread per
// (person, column) of the split-K sum (smpl_blend_bwd_sum_kernel)
inline Launch chain_bwd_shape(int N) { return {0, (unsigned)((N + 3) / 4), 1u, 1u, 256u, 0, 0}; }
inline Launch joints_bwd_shape(int N) { return {0, (unsigned)N, 1u, 1u, 192u, 0, 0}; }
inline Launch blend_bwd_sum_shape(int N) { return {0, (unsigned)(((long)N * kBlendK + 63) / 64), 1u, 1u, 256u, 0, 0}; }      // 64 elements x 4 quarters of the splits
constexpr int kSmplBwdMaxN = 1 << 16;       // N above it: TEPOSE_E_SHAPE (N * 20672 floats of one buffer stay below 2^31 elements; grid y of the skinning)
// What the backward carves behind the forward's buffers, in floats, in carve order: the joint sources [N][54][3], g_vposed [N][kVertLd], the skinning
// partials [N][14][288], the split-K partials [splits][N][224] and their sum [N][224].  One function for the size query and the entry point.
// The split count falls as N grows (323 up to N = 192, 162 at N = 193), so splits x N is not monotone in N; its bound min(323 N, 65568 + N) is (t
// tiles: N <= 32 t and splits <= 2048 / t + 1), and a workspace sized for N persons then serves every smaller call as well.
struct SmplBwdFloats { size_t gsrc, gvp, skin_part, blend_part, gf; };
inline size_t blend_bwd_part_rows(int N) {
  const size_t a = (size_t)kBwdChunks * (size_t)N, b = (size_t)(8 * kChipCUs * 32 + 32) + (size_t)N;
  return a < b ? a : b;
}
inline SmplBwdFloats smpl_bwd_floats(int N) {
  const size_t n = (size_t)N;
  return {n * kBwdSrc * 3, n * kVertLd, n * kBwdSkinBlocks * kNJ * 12, blend_bwd_part_rows(N) * kBlendK, n * kBlendK};
}
// Levels of the kinematic tree: depth[j] of every joint (root 0) and, returned, the deepest level.  tepose_pack_smpl writes exactly these into the
// blob, and they are all the chain kernels know of the tree's shape: the forward walks the levels 1 .. maxdepth, the backward maxdepth .. 1.  Parents must
// precede their children (parents[j] < j; the pack refuses anything else); parents[0] is ignored.
inline int chain_depths(const int* parents, int* depth) {
  int maxd = 0;
  depth[0] = 0;
  for (int j = 1; j < kNJ; ++j) { depth[j] = depth[parents[j]] + 1; if (depth[j] > maxd) maxd = depth[j]; }
  return maxd;
}
// The order in which smpl_chain_bwd_kernel finishes joints, as a host model of its walk over those levels: level by level from the deepest (all joints
// of a level at once, one lane each), a parent taking its children's contributions in ascending joint index.  order[i]: the i-th joint finished.  The
// host check pins the levels (what the kernel consumes) and this model; the kernel's own walk is held to the fp64 gradients by the GPU tests.
inline void chain_bwd_order(const int* parents, int* order) {
  int depth[kNJ], n = 0;
  const int maxd = chain_depths(parents, depth);
  for (int lvl = maxd; lvl >= 0; --lvl)
    for (int j = 0; j < kNJ; ++j)
      if (depth[j] == lvl) order[n++] = j;
}

// ---------------------------------------------------------------- live-session windows (session_advance_kernel / session_commit_kernel, session.hip)
constexpr int kSessionMaxSlots = 4096;      // S above it: TEPOSE_E_SHAPE (grid y; S * 85 stays far below 2^31)
// one thread per column of a slot's window rows (it walks the T rows itself): 9 blocks of 256 cover the 2133 columns, one grid row per slot
inline Launch session_advance_shape(int S) { return {0, (unsigned)((kInput + 255) / 256), (unsigned)S, 1u, 256u, 0, 0}; }
// one thread per (slot, theta column)
inline Launch session_commit_shape(int S) { return {0, (unsigned)((S * kTheta + 127) / 128), 1u, 1u, 128u, 0, 0}; }
// the one-euro step of a smoothing session (session_smooth_kernel, filters.hip): one thread per (slot, theta column) as well -- 72 filter a pose
// component, 13 copy cam and betas
inline Launch session_smooth_shape(int S) { return {0, (unsigned)((S * kTheta + 127) / 128), 1u, 1u, 128u, 0, 0}; }

// ---------------------------------------------------------------- person crops (crop_frames_u8_kernel / crop_boxes_u8_kernel, crop.hip)
constexpr int kCropBlock = 256;
constexpr int kCropMaxSide = 32768;         // S above it: TEPOSE_E_SHAPE (S * S stays below 2^31; at most 2^22 blocks per crop)
// one thread per crop pixel (its three channels), one grid row per crop; above 65535 crops the rows stride (crop_boxes takes at most kSessionMaxSlots)
inline Launch crop_shape(int S, int n) { return {0, (unsigned)(((long)S * S + kCropBlock - 1) / kCropBlock), (unsigned)(n < 65535 ? n : 65535), 1u, (unsigned)kCropBlock, 0, 0}; }

}  // namespace tepose
