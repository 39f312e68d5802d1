// The workspaces as numbers: where every buffer of every forward path lies -- the encoder's (carve_encoder), the regressor's and the SMPL entries'
// (carve_regressor, carve_smpl_bwd), a frame projection's (carve_projection), the VIBE encoder's (carve_vibe) and how a whole forward shares one
// workspace between them (forward_layout, forward_bytes) --, what one place of a recurrent-state buffer looks like in every form a kernel takes it
// (StateBuf::at), and which places each direction of each cell step reads and writes (cell_step, cell_top_rec_fwd).
// Plain ints and offsets in, offsets out: nothing from HIP, no pointer.  forward.hip adds the workspace base at the last moment; every sizing pass
// runs the same carve without one.  tests/test_state_layout.py compiles this header with the host compiler and checks it exhaustively against
// written-out expressions.
#pragma once
#include <assert.h>
#include <initializer_list>

#include "formats.h"
#include "shapes.h"

namespace tepose {

constexpr size_t kNoRef = ~(size_t)0;     // "this form does not exist": no mirror, not blocked, no previous state, a buffer this shape does not have

// Sequential carve of a workspace: n floats -> their float offset; every buffer starts on a 256-byte boundary
struct Carve {
  size_t cur = 0;                          // bytes taken so far
  size_t take(size_t n) {
    const size_t o = cur;
    cur = align_up(cur + n * sizeof(float), 256);
    return o / sizeof(float);
  }
  size_t take_if(bool have, size_t n) { const size_t o = take(have ? n : 0); return have ? o : kNoRef; }   // (an absent buffer takes nothing)
};

// One place of a state buffer -- slab t, row 0, column c0 -- in every form a consumer may take
struct StateRef {
  size_t f = kNoRef; long ld = 0;          // fp32 rows: float offset in the workspace, leading dimension
  size_t p = kNoRef; long kst = 0;         // hi / lo planes in the forward's format: half offset inside the state mirrors, halfs between K-tiles
  size_t b = kNoRef; long bst = 0;         // fp32 as 16 x 16 blocks (st_blk_offset / gi_blk_offset): float offset of the first row tile, floats between row tiles
  StateRef rows_only() const { StateRef r = *this; r.b = kNoRef; r.bst = 0; return r; }   // a place whose next reader wants it row-major
};

// A carved [T][Bs][C] fp32 buffer: T time slabs of Bs rows (B, or B rounded up to 16 on the split path, so that every slab starts on a swizzle period;
// the pad rows are never consumed).  With a mirror, the [T * Bs x C] matrix also exists as hi / lo planes from half `poff` of the state mirrors, in the
// ONE plane format of the forward: tile 16 = scaled [K/16][R][16], tile 32 = blocked [K/32][R][32].  blk: the plan keeps this buffer's rows as 16 x 16 blocks.
struct StateBuf {
  size_t off = 0, T = 0, Bs = 0, C = 0, poff = kNoRef;
  int tile = 32;
  bool blk = false;
  size_t floats() const { return T * Bs * C; }
  StateRef at(size_t t, size_t c0 = 0) const {
    const long R = (long)(T * Bs), row = (long)(t * Bs);
    StateRef r;
    r.f = off + (size_t)row * C + c0; r.ld = (long)C;
    if (poff != kNoRef) { r.p = poff + (size_t)(tile == 32 ? plane_index(row, (long)c0, R) : plane16_index(row, (long)c0, R)); r.kst = R * tile; }
    if (blk) { r.b = off + (size_t)row * C + c0 * 16; r.bst = (long)C * 16; }   // column c0's blocks start c0 * 16 floats into every row tile
    return r;
  }
};

// Blocked hi / lo planes [K/32][R][32] of an operand carved on its own (the tail linears' A): float offsets of the two planes, halfs between K-tiles
struct APlanes {
  size_t hi = 0, lo = 0; long kst = 0;
  size_t k(long k0) const { return (size_t)(k0 / 32) * (size_t)kst; }      // halfs from either plane's start to the K range that begins at column k0
};

// What a forward's shape and plan fix about the encoder's workspace
struct EncShape {
  int L, Hp, B, T;
  bool h3, scaled, gblk;                   // KernelPlan: planes carved; their format is the scaled one; fp32 states / layer >= 1 gate pre-activations blocked
  size_t sync_words, gran_words;           // the sync region and, where the persistent kernel's granule mode can run, its buffers (0: none)
};

// Buffers of one encoder forward.  Offsets in floats from the workspace base.
struct EncLayout {
  size_t sync = 0, gran = 0;               // arrival counters + status words; right behind them the granule buffers: one clearing zeroes both
  size_t xp = 0, g0 = 0, g0c = 0, y1 = 0;
  StateBuf gf, grr, grf;                   // layer >= 1 gate pre-activations per direction (no mirror); grf of the top layer: the one step it consumes
  // layers below the top keep every state: sf [T][Bs][Hp], sr [T][Bs][2 Hp] (gru_rec's halves side by side: forward | reverse); the top layer ping-pongs
  // pf / pr and leaves [rec forward's one step | rec reverse's last state] in ytop
  StateBuf sf[2], sr[2], pf[2], pr[2], ytop;
  size_t state_hi = 0, state_lo = 0;       // the mirrors every StateRef::p refers to
  size_t x0h = 0, x0l = 0;                 // compact planes of the frames a 1-layer model's rec.l0 forward direction consumes
  size_t rs = 0, rs0 = 0;                  // per-row scales of the input planes: [B*T] and, 1-layer models, [B]
  APlanes tailA;                           // [relu(last forward state) | relu(ytop)] = [B x 3Hp], A operand of the tail linears
  size_t Bs = 0, plane_halfs = 0;
};

inline EncLayout carve_encoder(const EncShape& s, Carve& c) {
  const size_t Hp = (size_t)s.Hp, B = (size_t)s.B, T = (size_t)s.T, BT = B * T;
  const int L = s.L;
  const size_t Bs = s.h3 ? (size_t)round_up(s.B, 16) : B;
  // what every StateBuf::at relies on, stated once: slabs start on a 16-row boundary and columns 0 / Hp on a K-tile of either format
  assert(Hp % 32 == 0 && (!s.h3 || Bs % 16 == 0));
  EncLayout w;
  w.Bs = Bs;
  auto buf = [&](bool need, size_t t, size_t rows, size_t cols, bool mirror) {
    StateBuf b;
    b.off = c.take(need ? t * rows * cols : 0);
    if (!need) return b;
    b.T = t; b.Bs = rows; b.C = cols; b.tile = s.scaled ? 16 : 32; b.blk = s.gblk;
    if (mirror && s.h3) { b.poff = w.plane_halfs; w.plane_halfs += b.floats(); }
    return b;
  };
  w.sync = c.take(s.sync_words);
  w.gran = c.take(s.gran_words);
  w.xp = c.take(BT * kInputP);
  w.g0 = c.take(BT * (L >= 2 ? 9 : 6) * Hp);
  w.g0c = c.take(L >= 2 ? 0 : B * 3 * Hp);
  w.gf = buf(L >= 2, T, Bs, 3 * Hp, false);
  w.grr = buf(L >= 2, T, Bs, 3 * Hp, false);
  // the one step a 2-layer model's top layer consumes: B rows -- Bs where it is blocked: a ragged last tile of 16 x 16 blocks is as long as a whole one, and
  // what lies behind it (layer 0's states) is read back by tepose_encoder_tap.  The extra rows come out of y1, which such a plan never uses: sizes stay
  const size_t grf_pad = s.gblk && L == 2 ? (Bs - B) * 3 * Hp : 0;
  w.grf = L >= 3 ? buf(true, T, Bs, 3 * Hp, false) : buf(L == 2, 1, s.gblk ? Bs : B, 3 * Hp, false);
  for (int i = 0; i < 2; ++i) {
    const bool need = (i == 0 && L >= 2) || (i == 1 && L >= 3);
    w.sf[i] = buf(need, T, Bs, Hp, true);
    w.sr[i] = buf(need, T, Bs, 2 * Hp, true);
    w.pf[i] = buf(true, 1, Bs, Hp, true);
    w.pr[i] = buf(true, 1, Bs, Hp, true);
  }
  w.ytop = buf(true, 1, Bs, 2 * Hp, true);
  w.y1 = c.take(B * kFeat > grf_pad ? B * kFeat - grf_pad : 0);      // the exact-fp32 tail's scratch (a plan that blocks nothing)
  w.state_hi = c.take(s.h3 ? w.plane_halfs / 2 + 64 : 0);
  w.state_lo = c.take(s.h3 ? w.plane_halfs / 2 + 64 : 0);
  w.x0h = c.take(s.h3 && L == 1 ? B * kInputP / 2 + 64 : 0);
  w.x0l = c.take(s.h3 && L == 1 ? B * kInputP / 2 + 64 : 0);
  w.rs = c.take(s.h3 ? BT : 0);
  w.rs0 = c.take(s.h3 && L == 1 ? B : 0);
  w.tailA.hi = c.take(s.h3 ? B * 3 * Hp / 2 + 64 : 0);
  w.tailA.lo = c.take(s.h3 ? B * 3 * Hp / 2 + 64 : 0);
  w.tailA.kst = (long)B * 32;
  return w;
}

// ---- the regressor and the SMPL entries -------------------------------------------------------------------------------------------------------------
struct RegShape {
  int N;
  bool h3, blend16;                        // KernelPlan: operand planes carved; the pose features again as scaled planes (large batches)
  size_t sync_words;
};

// An activation matrix [N x ld] of the regressor: fp32 rows and -- split path -- the blocked planes the previous product (or a split) leaves
struct RegAct {
  size_t rows = kNoRef; long ld = 0;
  APlanes P{kNoRef, kNoRef, 0};
};

// Buffers of one regressor / SMPL call.  Offsets in floats from the workspace base.
struct RegLayout {
  size_t sync = 0;                         // model.h sync_words(): the first carve here too, so that both halves of a forward share one
  RegAct feat, xs, h1, h2, pf;             // feat: planes only, its rows are the caller's
  size_t base = 0, amat = 0, posed = 0, vposed = 0;
  size_t pf16h = kNoRef, pf16l = kNoRef, pfrs = kNoRef;   // blend16: scaled planes [K/16][N][16] of the pose features + per-row scales
};

inline RegLayout carve_regressor(const RegShape& s, Carve& c) {
  const size_t N = (size_t)s.N;
  RegLayout w;
  w.sync = c.take(s.sync_words);
  w.feat.ld = kFeat; w.xs.ld = kState; w.h1.ld = w.h2.ld = 1024; w.pf.ld = kBlendK;
  for (RegAct* a : {&w.feat, &w.xs, &w.h1, &w.h2, &w.pf}) {
    a->P.hi = c.take_if(s.h3, N * a->ld / 2 + 64);
    a->P.lo = c.take_if(s.h3, N * a->ld / 2 + 64);
    a->P.kst = (long)N * 32;
  }
  w.base = c.take(N * 1024);
  for (RegAct* a : {&w.h1, &w.h2, &w.xs, &w.pf}) a->rows = c.take(N * a->ld);
  w.amat = c.take(N * kNJ * 12);
  w.posed = c.take(N * kNJ * 3);
  w.vposed = c.take(N * kVertLd);
  w.pf16h = c.take_if(s.blend16, N * kBlendK / 2);
  w.pf16l = c.take_if(s.blend16, N * kBlendK / 2);
  w.pfrs = c.take_if(s.blend16, N);
  return w;
}

// the SMPL backward: the forward's buffers (recomputed) and behind them its own, in the order of shapes.h smpl_bwd_floats
struct SmplBwdLayout { RegLayout fwd; size_t gsrc, gvp, skin_part, blend_part, gf; };
inline SmplBwdLayout carve_smpl_bwd(const RegShape& s, Carve& c) {
  SmplBwdLayout w;
  w.fwd = carve_regressor(s, c);
  const SmplBwdFloats f = smpl_bwd_floats(s.N);
  w.gsrc = c.take(f.gsrc); w.gvp = c.take(f.gvp); w.skin_part = c.take(f.skin_part); w.blend_part = c.take(f.blend_part); w.gf = c.take(f.gf);
  return w;
}

// ---- a frame projection of M rows (tepose_project_frames, the pair product): the padded fp32 rows and, where the product runs on the split-precision
// kernel, ONE block for both planes -- the lo plane starts half-way in, as many halfs behind the hi plane as the padded rows take floats -- and per-row scales
struct ProjLayout { size_t xp = 0; APlanes P{kNoRef, kNoRef, 0}; size_t rs = kNoRef; };
inline ProjLayout carve_projection(size_t M, bool h3, Carve& c) {
  ProjLayout w;
  w.xp = c.take(M * kInputP);
  const size_t xbytes = c.cur - w.xp * sizeof(float);      // the rows, rounded up to the carve's 256 bytes
  w.P.hi = c.take_if(h3, xbytes / 4 + 128);
  if (h3) { w.P.lo = w.P.hi + xbytes / 8; w.P.kst = (long)M * 32; }
  w.rs = c.take_if(h3, M);
  return w;
}

// ---- the VIBE encoder: gate pre-activations [BN][D][3 Hp] and two state buffers [BN][D][Hp] that its layers alternate between
struct VibeLayout { size_t G, S[2]; };
inline VibeLayout carve_vibe(size_t BN, size_t D, size_t Hp, Carve& c) {
  VibeLayout w;
  w.G = c.take(BN * D * 3 * Hp);
  w.S[0] = c.take(BN * D * Hp);
  w.S[1] = c.take(BN * D * Hp);
  return w;
}

// ---- a whole forward (tepose_forward, tepose_forward_cached, tepose_window_step): [scratch | feature].  The scratch is shared: encoder and regressor are
// both carved from offset 0 -- the encoder's buffers are dead once the feature exists --, so the sync region with the forward's status words is the first
// carve of either and sits at the workspace base for every entry point (tepose_forward_status reads it there).  The feature slot, [B][2 x 2048] floats, is
// cut off the END of whatever workspace the caller gave.
struct FwdLayout { size_t scratch_bytes, feat; };          // the scratch starts at offset 0; feat: float offset of the feature slot
inline FwdLayout forward_layout(size_t ws_bytes, int B) {
  const size_t feat_bytes = align_up((size_t)B * 2 * kFeat * sizeof(float), 256);
  const size_t scratch_bytes = (ws_bytes & ~(size_t)255) - feat_bytes;
  return FwdLayout{scratch_bytes, scratch_bytes / sizeof(float)};
}
// What tepose_workspace_bytes answers: the encoder, the feature and a regressor of 2 B rows (is_train regresses two per window) one behind the other,
// plus one granule.  A workspace of that size holds the layout above: every term is a multiple of 256, so forward_layout leaves
// scratch_bytes = encoder + regressor(2 B) + 256 >= encoder; and regressor(2 B) >= regressor(B) under any two plans, because every plan carves 24488
// floats of rows per person and a split plan's planes, scaled planes and row scales add only 4705 more (and under 8 KB of rounding in all).
inline size_t forward_bytes(const EncShape& enc, const RegShape& reg2) {
  Carve c;
  carve_encoder(enc, c);
  c.take((size_t)enc.B * 2 * kFeat);
  carve_regressor(reg2, c);
  return c.cur + 256;
}

// ---- the recurrence's addressing ------------------------------------------------------------------------------------------------------------------
// One direction of one cell step: where it reads its gate pre-activations and its previous state and where it writes its new state.  Layer 0 takes its
// gate pre-activations from frame `frame` of the caller's projections (forward.hip G0Src; -1: its single-step source), not from the workspace: gi is then empty.
struct DirStep {
  int frame = 0;
  StateRef gi, hprev, hout;                // hprev of a first step: empty -- no address in front of a buffer is ever formed
};
struct CellStep {
  int ndir = 0;
  bool first = false;                      // h_{-1} = 0
  DirStep d[3];                            // the cell-step order of a layer's directions: gru_fwd, gru_rec reverse, gru_rec forward
};

// Step st of layer l of L: gru_fwd at frame st; gru_rec's reverse direction at flipped index T-1-st (layer 0: frame st); below the top layer, gru_rec's
// forward direction at flipped index st (layer 0: frame T-1-st).  Layers >= 1 read time-major slab `flipped index` of layer_projections' output.
inline CellStep cell_step(const EncLayout& w, int L, int T, int l, int st) {
  const bool top = l == L - 1, last = st == T - 1;
  const size_t Hp = w.ytop.C / 2;
  const int i = T - 1 - st;
  CellStep s;
  s.first = st == 0; s.ndir = top ? 2 : 3;
  const int frame[3] = {st, st, i}, slab[3] = {st, i, st};
  const StateBuf* g[3] = {&w.gf, &w.grr, &w.grf};
  for (int k = 0; k < s.ndir; ++k) {
    s.d[k].frame = frame[k];
    if (l > 0) s.d[k].gi = g[k]->at((size_t)slab[k]);
  }
  if (!top) {
    const StateBuf &sf = w.sf[l & 1], &sr = w.sr[l & 1];
    s.d[0].hout = sf.at(st);
    s.d[1].hout = sr.at(i, Hp);
    s.d[2].hout = sr.at(st);
    if (!s.first) { s.d[0].hprev = sf.at(st - 1); s.d[1].hprev = sr.at(i + 1, Hp); s.d[2].hprev = sr.at(st - 1); }
  } else {
    // (the last states are read row-major by the tail; every earlier one only by the next step)
    s.d[0].hout = last ? w.pf[st & 1].at(0).rows_only() : w.pf[st & 1].at(0);
    s.d[1].hout = last ? w.ytop.at(0, Hp).rows_only() : w.pr[st & 1].at(0);
    if (!s.first) { s.d[0].hprev = w.pf[(st + 1) & 1].at(0); s.d[1].hprev = w.pr[(st + 1) & 1].at(0); }
  }
  return s;
}

// the top layer's forward direction of gru_rec: one cell step from h = 0 into ytop's first half (layer 0: from the caller's single-step projections)
inline CellStep cell_top_rec_fwd(const EncLayout& w, int l) {
  CellStep s;
  s.first = true; s.ndir = 1;
  s.d[0].frame = -1;
  if (l > 0) s.d[0].gi = w.grf.at(0);
  s.d[0].hout = w.ytop.at(0).rows_only();
  return s;
}

}  // namespace tepose
