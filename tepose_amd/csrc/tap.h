// Reading a finished encoder forward back out of its workspace (tepose_encoder_tap): which buffer holds a stage -- the gate pre-activations of a
// layer's direction, the state a cell step wrote, the tail product's A operand --, in which form the plan's producer left it there, and the offset of
// element (slab, row, column) in that form.  Built on state.h's carve and cell_step, so a tap reads the places the forward's launches were given.
// Plain ints and offsets, nothing from HIP: misc.hip's gather kernel and the host compiler (tests/test_encoder_stages_helper.py) share tap_index.
#pragma once
#include "state.h"

namespace tepose {

enum TapStage { kTapGi = 0, kTapH = 1, kTapTail = 2 };
// fp32 rows | fp32 16 x 16 blocks of a state (st_blk_offset) | of gate pre-activations (gi_blk_offset) | hi + lo planes, blocked [K/32][R][32] | scaled [K/16][R][16]
enum TapForm { kTapRows = 0, kTapStateBlocks = 1, kTapGiBlocks = 2, kTapPlanes32 = 3, kTapPlanes16 = 4 };

// What select_kernels fixes about the forms: planes0 / planes1 -- the cell steps of layer 0 / layers >= 1 are gru_step16_kernel<true>, which writes no
// fp32 copy of a blocked state: there the planes are the value
struct TapPlan {
  int L, Hp, B, T;
  bool h3, g0blk, planes0, planes1;
};

// One stage as [slabs][rows][cols] values
struct TapView {
  int form = kTapRows;
  int slabs = 1, rows = 0, cols = 0;
  size_t off = 0;                  // element (0, 0, 0): float offset in the workspace; plane forms: half offset inside either plane
  long slab = 0;                   // floats between slabs
  long ld = 0;                     // rows: floats between rows; blocks: floats between 16-row tiles; planes: halfs between K-tiles
  int hp = 0;                      // gi blocks: hidden units per gate
  int c1 = 0; size_t off2 = 0; long ld2 = 0;   // rows, c1 > 0: columns c1.. come from a second matrix (the exact-fp32 tail operand: [last forward state | ytop])
  size_t hi = 0, lo = 0;           // plane forms: float offsets of the planes' starts
  float scale = 1.f, lo_scale = 1.f;           // plane forms: value = (hi + lo * lo_scale) * scale
  long rs = -1;                    // plane forms, >= 0: float offset of per-row scales, value *= ws[rs + row] (the decoder's pf16)
  bool relu = false;               // the consumer applies ReLU on the fly (exact-fp32 tail): the gather does, too
  size_t count() const { return (size_t)slabs * rows * cols; }
};

// offset of element (t, row, col) in the view's form (floats; plane forms: halfs from either plane's start)
TEPOSE_HD inline size_t tap_index(const TapView& v, long t, long row, long col) {
  const size_t o = v.off + (size_t)(t * v.slab);
  switch (v.form) {
    case kTapStateBlocks: return o + (size_t)st_blk_offset(row, (int)col, v.ld);
    case kTapGiBlocks: return o + (size_t)gi_blk_offset(row, (int)(col / v.hp), (int)(col % v.hp), v.ld);
    case kTapPlanes32: return o + (size_t)((col >> 5) * v.ld + plane_index(row, col & 31, 0));
    case kTapPlanes16: return o + (size_t)((col >> 4) * v.ld + plane16_index(row, col & 15, 0));
    default: break;
  }
  if (v.c1 > 0 && col >= v.c1) return v.off2 + (size_t)(row * v.ld2 + (col - v.c1));
  return o + (size_t)(row * v.ld + col);
}

// the state a cell step wrote, in the form its producer left for its consumer
inline TapView tap_state(const EncLayout& w, const TapPlan& p, int l, const StateRef& q) {
  TapView v;
  v.rows = p.B; v.cols = p.Hp;
  const bool planes = l == 0 ? p.planes0 : p.planes1;
  if (p.h3 && q.b != kNoRef && planes) {
    const bool s16 = w.ytop.tile == 16;
    v.form = s16 ? kTapPlanes16 : kTapPlanes32;
    v.off = q.p; v.ld = q.kst; v.hi = w.state_hi; v.lo = w.state_lo;
    v.scale = s16 ? 1.f / 16384.f : 1.f; v.lo_scale = s16 ? 1.f : 1.f / 2048.f;      // common.h kStateScale, kLoScale
  } else if (p.h3 && q.b != kNoRef) {
    v.form = kTapStateBlocks; v.off = q.b; v.ld = q.bst;
  } else {
    v.off = q.f; v.ld = q.ld;
  }
  return v;
}

// Stage -> view.  false: no such stage in this model, or nothing of it is left once the forward has finished (TEPOSE_E_SHAPE).
//   gi(l, d)      l = 0: the column slices of g0 (and g0c) in frame order; l >= 1: gf / grr / grf in slab order -- only the LAST layer's, every layer >= 1
//                 projects into the same three buffers.  The top layer's gru_rec forward direction (d = 2) is one slab.
//   h(l, d, st)   below the top layer every step (sf / sr; a layer two below another one has been overwritten by it); on the top layer steps T - 1 and T - 2
//                 of gru_fwd and gru_rec reverse (the ping-pong's two halves and ytop) and the one step of gru_rec forward (d = 2, st = 0)
//   tail          [B][3 Hp] = relu[last forward state | ytop]
inline bool tap_resolve(const EncLayout& w, const TapPlan& p, int stage, int l, int d, int st, TapView* out) {
  const int L = p.L, Hp = p.Hp, B = p.B, T = p.T, H3 = 3 * Hp;
  TapView v;
  if (stage == kTapTail) {
    v.rows = B; v.cols = H3;
    if (p.h3) {
      v.form = kTapPlanes32; v.off = 0; v.ld = w.tailA.kst; v.hi = w.tailA.hi; v.lo = w.tailA.lo; v.lo_scale = 1.f / 2048.f;
    } else {
      v.off = w.pf[(T - 1) & 1].off; v.ld = Hp; v.c1 = Hp; v.off2 = w.ytop.off; v.ld2 = 2 * Hp; v.relu = true;
    }
    *out = v;
    return true;
  }
  if (l < 0 || l >= L || d < 0 || d > 2) return false;
  const bool top = l == L - 1;
  if (stage == kTapGi) {
    v.rows = B; v.cols = H3;
    if (l == 0) {
      const long ld0 = (long)(L >= 2 ? 9 : 6) * Hp;
      if (top && d == 2) { v.off = w.g0c; v.ld = H3; }                       // 1-layer model: the one consumed step of gru_rec forward
      else if (p.g0blk) { v.form = kTapGiBlocks; v.slabs = T; v.off = w.g0 + (size_t)d * H3 * 16; v.slab = (long)B * ld0; v.ld = ld0 * 16; v.hp = Hp; }
      else { v.slabs = T; v.off = w.g0 + (size_t)d * H3; v.slab = ld0; v.ld = (long)T * ld0; }          // batch-major: row b * T + t
    } else {
      if (!top) return false;
      const StateBuf& g = d == 0 ? w.gf : d == 1 ? w.grr : w.grf;
      v.slabs = d == 2 ? 1 : T; v.off = g.off; v.slab = (long)(g.Bs * g.C);
      if (g.blk) { v.form = kTapGiBlocks; v.ld = (long)g.C * 16; v.hp = Hp; }
      else v.ld = (long)g.C;
    }
    *out = v;
    return true;
  }
  if (stage != kTapH || st < 0 || st >= T) return false;
  if (top) {
    if (d == 2) {
      if (st != 0) return false;
      *out = tap_state(w, p, l, cell_top_rec_fwd(w, l).d[0].hout);
      return true;
    }
    if (st < T - 2) return false;
  } else if (l + 2 < L - 1) return false;
  *out = tap_state(w, p, l, cell_step(w, L, T, l, st).d[d].hout);
  return true;
}

// ---- the decoder half (tepose_decoder_tap): one stage of a finished regressor / SMPL call as [N][cols].  Where the buffers lie is carve_regressor's
// answer (state.h RegLayout, read as it is); which forms exist is select_kernels' (RegLayout's absent buffers, Smpl::small, Reg::seq).
enum DecStage { kDecXs = 0, kDecH1, kDecH2, kDecPf, kDecPfPlanes, kDecPf16, kDecAmat, kDecPosed, kDecVposed, kDecStages };

// What the plan adds to the carve: small -- the one-launch small-N kernel ran; reg_seq -- reg_seq_kernel, which leaves the FC activations as planes only
// (it writes no fp32 rows); xs -- where the state rows are: the carve's, or the feature slot of a tail-collapsed forward
struct DecPlan { bool small, reg_seq; size_t xs; };

inline int dec_cols(int stage) {
  switch (stage) {
    case kDecXs: return kState;
    case kDecH1: case kDecH2: return 1024;
    case kDecPf: case kDecPfPlanes: case kDecPf16: return kBlendK;
    case kDecAmat: return kNJ * 12;
    case kDecPosed: return kNJ * 3;
    case kDecVposed: return 3 * kNV;
    default: return 0;
  }
}

// false: the plan never writes this stage (TEPOSE_E_SHAPE) -- the one-launch small-N kernel keeps neither pose features nor v_posed
inline bool tap_decoder(const RegLayout& w, const DecPlan& p, int stage, int N, TapView* out) {
  TapView v;
  v.rows = N; v.cols = dec_cols(stage);
  auto planes32 = [&](const APlanes& P) { v.form = kTapPlanes32; v.off = 0; v.ld = P.kst; v.hi = P.hi; v.lo = P.lo; v.lo_scale = 1.f / 2048.f; };
  switch (stage) {
    case kDecXs: v.off = p.xs; v.ld = kState; break;
    case kDecH1: case kDecH2: {
      const RegAct& h = stage == kDecH1 ? w.h1 : w.h2;
      if (p.reg_seq) planes32(h.P);
      else { v.off = h.rows; v.ld = h.ld; }
      break;
    }
    case kDecAmat: v.off = w.amat; v.ld = kNJ * 12; break;
    case kDecPosed: v.off = w.posed; v.ld = kNJ * 3; break;
    case kDecPf: if (p.small) return false; v.off = w.pf.rows; v.ld = w.pf.ld; break;
    case kDecVposed: if (p.small) return false; v.off = w.vposed; v.ld = kVertLd; break;
    case kDecPfPlanes:
      if (p.small || w.pf.P.hi == kNoRef) return false;
      planes32(w.pf.P);
      break;
    case kDecPf16:
      if (p.small || w.pf16h == kNoRef) return false;
      v.form = kTapPlanes16; v.off = 0; v.ld = (long)N * 16; v.hi = w.pf16h; v.lo = w.pf16l; v.rs = (long)w.pfrs;
      break;
    default: return false;
  }
  *out = v;
  return true;
}

}  // namespace tepose
