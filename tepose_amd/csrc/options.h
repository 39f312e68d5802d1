// Per-handle options: every launch threshold of the library, the one table of their names, and the environment's view of them.  Plain C++: nothing
// from HIP is included, so the host compiler alone builds it (tests/test_launch_shapes.py).  common.h includes this header; shapes.h turns the
// thresholds into launch shapes.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace tepose {

// Every launch threshold of the library.  A handle owns ONE Options object: tepose_create fills it from the environment (options_from_env, the only
// place the library reads TEPOSE_* threshold variables), tepose_set_option(m, "NAME", value) changes a field before anything is packed, and every
// launcher that consults a threshold takes the handle's object as an argument -- no function-local static, no process-wide state: two handles of one
// process can differ (SURVEY.md 8b "no global mutable state").  Defaults = the measured best.
struct Options {
  int skinny_max_m = 768;            // TEPOSE_SKINNY_MAX_M: rows at or below which the width-first fp32 kernels (skinny.hip) win over 128-row tiles (measured crossover)
  int skinny_max_m_gemm = -1;        // TEPOSE_SKINNY_MAX_M_GEMM: the same for plain products only (-1: skinny_max_m)
  int split_min_m = 0;               // TEPOSE_SPLIT_MIN_M: rows ABOVE which a split-mode handle runs its matmuls on the fp16x3 kernels (round 2: they win at every batch size)
  int skinny_h3_max_m = 128;         // TEPOSE_SKINNY_H3_MAX_M: rows up to which a split-mode GRU step uses the width-first kernel of skinny_h3.hip
  int gemm_half_max_blocks = 1024;   // TEPOSE_GEMM_HALF_MAX_BLOCKS: 64-row tiles of gemm_f32_kernel while 128-row tiles would make at most this many blocks
  int split_few_max_rows = 1024;     // TEPOSE_SPLIT_FEW_MAX_ROWS: rows up to which launch_split_rows runs one workgroup per row (222 rows 12.3 -> 5 us, 1024 rows 13 -> 8)
  int h3_tile = 0;                   // TEPOSE_H3_TILE: A/B, force a tile shape of gemm_h3_kernel (64 / 192 / 256)
  int h3_tile64 = 1;                 // TEPOSE_H3_TILE64: 0 = never pick 64-row tiles (A/B)
  int h3_tile192 = 1;                // TEPOSE_H3_TILE192: 0 = never pick 128 x 192 tiles (A/B)
  int s16_gm = 8;                    // TEPOSE_S16_GM: row tiles per XCD group of the barrier-free projection's walk (layer-0 projection ms at 2 / 4 / 8 / 16 / 32: 10.92 / 10.82 / 10.74 / 11.37 / 12.37)
  int s16_walk = 0;                  // TEPOSE_S16_WALK: that walk's order (csrc/walk.h): 0 = every XCD its own eighth of the tile order, 1 = all eight XCDs in the same row group (any other value: 0).  Same-box windows/s against the parent, profiles/r07_walk_ab.txt: walk 1 +0.9 % on plain C stores, -0.3 % on the non-temporal ones that ship
  int gru_gm = 4;                   // TEPOSE_GRU_GM: the same for the fused step (recurrent ms per forward at 1 / 2 / 4 / 8 / 16 / 32: 11.31 / 11.27 / 11.22 / 11.41 / 11.41 / 11.77)
  int seq_gran_max_m = 4;            // TEPOSE_SEQ_GRAN_MAX_M: rows up to which the persistent recurrent kernel hands its state over as tagged granules (B = 1 -14 %, 4 -5 %, 8 +20 %)
  int seq_max_m = 64;                // TEPOSE_SEQ_MAX_M: rows up to which a layer's T steps run as ONE persistent launch (0: never)
  int reg_seq_max_n = 64;            // TEPOSE_REG_SEQ_MAX_N: the same for the persistent FC-loop kernel
  int assume_cus = 0;                // TEPOSE_ASSUME_CUS: plan as if the device had this many CUs (planning without a device: tests/test_dispatch.py)
  int skinny_narrow64 = 1;           // TEPOSE_SKINNY_NARROW64, TEPOSE_SKINNY_MT1, TEPOSE_SKINNY_NT1_BELOW, TEPOSE_SKINNY_W8: block shapes of the width-first
  int skinny_mt1 = 1;                //   split kernel for narrow products (shapes.h skinny_h3_product_shape)
  int skinny_nt1_below = 96;
  int skinny_w8 = 1;
  int smpl_small_max_n = 4;          // TEPOSE_SMPL_SMALL_MAX_N: persons up to which prep + blend shapes + skinning run as one launch
  int l1_skinny_max_rows = 192;      // TEPOSE_L1_SKINNY_MAX_ROWS: real rows up to which a layer >= 1 projection runs on the width-first kernel
  int g0_mid_min_rows = 512;         // TEPOSE_G0_MID_MIN_ROWS: rows from which the layer-0 projection may take the 128 x 288 tiles
  int g0_skinny_max_m = 128;         // TEPOSE_G0_SKINNY_MAX_M: rows up to which the layer-0 projection runs on the width-first kernel
  unsigned long long seq_stamp_ptr = 0;   // TEPOSE_SEQ_STAMP_PTR: device buffer for the per-step time stamps of a -DTEPOSE_SEQ_STAMPS build (tools/seq_stamps.py)
};

// The one table of option names: environment variable TEPOSE_<NAME> at tepose_create, tepose_set_option(m, "<NAME>", v) afterwards.
struct OptName { const char* name; int Options::*field; };
inline constexpr OptName kOptNames[] = {
    {"SKINNY_MAX_M", &Options::skinny_max_m}, {"SKINNY_MAX_M_GEMM", &Options::skinny_max_m_gemm}, {"SPLIT_MIN_M", &Options::split_min_m},
    {"SKINNY_H3_MAX_M", &Options::skinny_h3_max_m}, {"GEMM_HALF_MAX_BLOCKS", &Options::gemm_half_max_blocks},
    {"SPLIT_FEW_MAX_ROWS", &Options::split_few_max_rows}, {"H3_TILE", &Options::h3_tile}, {"H3_TILE64", &Options::h3_tile64}, {"H3_TILE192", &Options::h3_tile192}, {"S16_GM", &Options::s16_gm}, {"S16_WALK", &Options::s16_walk},
    {"GRU_GM", &Options::gru_gm}, {"SEQ_GRAN_MAX_M", &Options::seq_gran_max_m}, {"SEQ_MAX_M", &Options::seq_max_m}, {"REG_SEQ_MAX_N", &Options::reg_seq_max_n},
    {"ASSUME_CUS", &Options::assume_cus}, {"SKINNY_NARROW64", &Options::skinny_narrow64}, {"SKINNY_MT1", &Options::skinny_mt1},
    {"SKINNY_NT1_BELOW", &Options::skinny_nt1_below}, {"SKINNY_W8", &Options::skinny_w8}, {"SMPL_SMALL_MAX_N", &Options::smpl_small_max_n},
    {"L1_SKINNY_MAX_ROWS", &Options::l1_skinny_max_rows}, {"G0_MID_MIN_ROWS", &Options::g0_mid_min_rows}, {"G0_SKINNY_MAX_M", &Options::g0_skinny_max_m},
};

// "SKINNY_MAX_M" (or "TEPOSE_SKINNY_MAX_M") -> &o.skinny_max_m; nullptr: no such option
inline int* option_field(Options& o, const char* name) {
  if (!name) return nullptr;
  if (strncmp(name, "TEPOSE_", 7) == 0) name += 7;
  for (const OptName& n : kOptNames)
    if (strcmp(n.name, name) == 0) return &(o.*(n.field));
  return nullptr;
}

// the environment's view of the options, read when a handle is created (and by the handle-less test entry points, per call)
inline Options options_from_env() {
  Options o;
  char var[64];
  for (const OptName& n : kOptNames) {
    snprintf(var, sizeof(var), "TEPOSE_%s", n.name);
    const char* e = getenv(var);
    if (e) o.*(n.field) = atoi(e);
  }
  const char* e = getenv("TEPOSE_SEQ_STAMP_PTR");
  o.seq_stamp_ptr = e ? strtoull(e, nullptr, 0) : 0ull;
  return o;
}

}  // namespace tepose
