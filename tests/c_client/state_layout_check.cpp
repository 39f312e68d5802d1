/* Host check of the encoder's workspace addressing (tepose_amd/csrc/state.h, formats.h), compiled with the host compiler alone: tests/test_state_layout.py.
 * The lines state.h replaced are kept here as the reference, with float addresses as integers (workspace base = kBase floats, so that the address the old
 * code formed in front of a buffer at step 0 stays representable): ref_carve (the carve of forward.hip and its registry of mirrored buffers), ref_view
 * (EncWs::view, the address -> planes search), ref_cell_dirs / ref_cell_top_rec_fwd (the written-out slab expressions) and the tail / persistent-kernel
 * offsets of carve_encoder and launch_layer_seq.
 * For every L, Hp, B, T, plan-flag and granule combination below:
 *   (a) every carved buffer's offset, the mirror size and the total equal the reference carve;
 *   (b) for every (layer, step, direction) the fp32 / plane / blocked reference of gi, hprev and hout equals the reference expression (hprev: from step 1
 *       on; the reference's step-0 value is an address nobody reads), and so do the projections' input views, ytop's view and the tail offsets;
 *   (c) stated without either: the hout of step st is the hprev of step st + 1 in all three forms; the reverse direction works on index T - 1 - st; the top
 *       layer ping-pongs pf / pr, its last reverse state lands in ytop + Hp and the extra step writes ytop; the tail planes are the K ranges [0, Hp),
 *       [Hp, 2Hp), [2Hp, 3Hp) of one [B x 3Hp] operand; every reference lies inside one carved buffer in each of its forms; a first step has no hprev.
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure. */
#include <cstdio>

#include "state.h"

using namespace tepose;

typedef long long Addr;                       // a float address: kBase + float offset in the workspace (0: null)
static const Addr kBase = (Addr)1 << 40;

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

// ---------------------------------------------------------------- the reference: the parent's lines
struct RefCarver {
  size_t cur = 0;
  Addr f(size_t n) {
    const size_t o = cur;
    cur = align_up(cur + n * sizeof(float), 256);
    return kBase + (Addr)(o / sizeof(float));
  }
};
struct RefPlanes { long long e; long kst; };   // e: halfs from the start of state_hi / state_lo (-1: no view)
struct RefWs {
  Addr sync, gran, xp, g0, g0c, gf, grr, grf, sf[2], sr[2], pf[2], pr[2], ytop, y1, state_hi, state_lo, x0h, x0l, rs, rs0, tail_hi, tail_lo;
  long tail_kst;
  long long tailR_off;                         // halfs from tailA.hi to tailR.hi
  size_t Bs = 0;
  struct Buf { Addr base; size_t T, B, C, poff; };
  Buf bufs[9]; int nbufs = 0;
  size_t plane_halfs = 0;
  void add(Addr base, size_t T, size_t B, size_t C) {
    bufs[nbufs++] = Buf{base, T, B, C, plane_halfs};
    plane_halfs += T * B * C;
  }
  RefPlanes view(Addr p, int tile = 32) const {
    for (int i = 0; i < nbufs; ++i) {
      const Buf& b = bufs[i];
      if (p >= b.base && p < b.base + (Addr)(b.T * b.B * b.C)) {
        const size_t off = (size_t)(p - b.base), t = off / (b.B * b.C), rem = off % (b.B * b.C);
        if (rem / b.C != 0 || (rem % b.C) % tile != 0) break;
        const long R = (long)(b.T * b.B), row = (long)(t * b.B), col = (long)(rem % b.C);
        const size_t e = b.poff + (size_t)(tile == 32 ? plane_index(row, col, R) : plane16_index(row, col, R));
        return RefPlanes{(long long)e, R * tile};
      }
    }
    return RefPlanes{-1, 0};
  }
};

static void ref_carve(int L, size_t Hp, int B, int T, bool h3, bool gblk, size_t sync_words, size_t gran_words, RefCarver& c, RefWs& w) {
  const size_t BT = (size_t)B * T;
  const size_t Bs = h3 ? (size_t)round_up(B, 16) : (size_t)B, BTs = Bs * T;
  w.Bs = Bs;
  w.sync = c.f(sync_words);
  w.gran = c.f(gran_words);
  w.xp = c.f(BT * kInputP);
  w.g0 = c.f(BT * (L >= 2 ? 9 : 6) * Hp);
  w.g0c = c.f(L >= 2 ? 0 : (size_t)B * 3 * Hp);
  w.gf = c.f(L >= 2 ? BTs * 3 * Hp : 0);
  w.grr = c.f(L >= 2 ? BTs * 3 * Hp : 0);
  // (the parent gave a 2-layer model's one-step grf B rows in every plan, and a blocked one's ragged last tile ran into sf[0]: where it is blocked it now has Bs
  // rows, taken out of y1, which such a plan never uses -- the total is the parent's)
  const size_t grf_rows = gblk ? Bs : (size_t)B, grf_pad = L == 2 ? (grf_rows - B) * 3 * Hp : 0;
  w.grf = c.f(L >= 3 ? BTs * 3 * Hp : (L == 2 ? grf_rows * 3 * Hp : 0));
  for (int i = 0; i < 2; ++i) {
    const bool need = (i == 0 && L >= 2) || (i == 1 && L >= 3);
    w.sf[i] = c.f(need ? BTs * Hp : 0);
    w.sr[i] = c.f(need ? BTs * 2 * Hp : 0);
    w.pf[i] = c.f(Bs * Hp);
    w.pr[i] = c.f(Bs * Hp);
    if (need) {
      w.add(w.sf[i], T, Bs, Hp);
      w.add(w.sr[i], T, Bs, 2 * Hp);
    }
    w.add(w.pf[i], 1, Bs, Hp);
    w.add(w.pr[i], 1, Bs, Hp);
  }
  w.ytop = c.f(Bs * 2 * Hp);
  w.add(w.ytop, 1, Bs, 2 * Hp);
  w.y1 = c.f((size_t)B * kFeat > grf_pad ? (size_t)B * kFeat - grf_pad : 0);
  w.state_hi = c.f(h3 ? w.plane_halfs / 2 + 64 : 0);
  w.state_lo = c.f(h3 ? w.plane_halfs / 2 + 64 : 0);
  w.x0h = c.f(h3 && L == 1 ? (size_t)B * kInputP / 2 + 64 : 0);
  w.x0l = c.f(h3 && L == 1 ? (size_t)B * kInputP / 2 + 64 : 0);
  w.rs = c.f(h3 ? BT : 0);
  w.rs0 = c.f(h3 && L == 1 ? (size_t)B : 0);
  w.tail_hi = c.f(h3 ? (size_t)B * 3 * Hp / 2 + 64 : 0);      // carve_planes(c, B, 3 * Hp, h3)
  w.tail_lo = c.f(h3 ? (size_t)B * 3 * Hp / 2 + 64 : 0);
  w.tail_kst = (long)B * 32;
  w.tailR_off = h3 ? (long long)((size_t)(Hp / 32) * w.tail_kst) : 0;
}

struct RefDir {
  Addr gi = 0; long ldgi = 0, gi_blk = 0;
  int frame = -1;                              // layer 0: the frame gi0 was asked for
  Addr hprev = 0; long ldh = 0;
  Addr hout = 0; long ldo = 0;
  Addr hprev_b = 0; long hp_blk = 0;
  Addr hout_b = 0; long ho_blk = 0;
};
struct RefArgs { RefDir d[3]; int ndir; int first; };

static RefArgs ref_cell_dirs(const RefWs& w, int L, int Hp, int T, int l, int st, bool gblk) {
  const int H3 = 3 * Hp;
  const long Bs = (long)w.Bs;
  const bool top = l == L - 1;
  const Addr sf = w.sf[l & 1];
  const Addr sr = w.sr[l & 1];
  RefArgs a{};
  a.first = st == 0; a.ndir = top ? 2 : 3;
  auto dir = [&](int k, Addr g, int frame, int slab) -> RefDir& {
    RefDir& d = a.d[k];
    if (l == 0) { d.frame = frame; }
    else { d.gi = g + (long)slab * Bs * H3; d.ldgi = H3; d.gi_blk = gblk ? (long)H3 * 16 : 0; }
    return d;
  };
  {  // gru_fwd
    RefDir& d = dir(0, w.gf, st, st);
    if (!top) {
      d.hprev = sf + (long)(st - 1) * Bs * Hp; d.ldh = Hp;
      d.hout = sf + (long)st * Bs * Hp; d.ldo = Hp;
      if (gblk) { d.hprev_b = d.hprev; d.hp_blk = (long)Hp * 16; d.hout_b = d.hout; d.ho_blk = (long)Hp * 16; }
    } else {
      d.hprev = w.pf[(st + 1) & 1]; d.ldh = Hp;
      d.hout = w.pf[st & 1]; d.ldo = Hp;
      if (gblk) { d.hprev_b = d.hprev; d.hp_blk = (long)Hp * 16; if (st < T - 1) { d.hout_b = d.hout; d.ho_blk = (long)Hp * 16; } }
    }
  }
  {  // gru_rec, reverse direction
    const int i = T - 1 - st;
    RefDir& d = dir(1, w.grr, st, i);
    if (!top) {
      d.hprev = sr + (long)(i + 1) * Bs * 2 * Hp + Hp; d.ldh = 2 * Hp;
      d.hout = sr + (long)i * Bs * 2 * Hp + Hp; d.ldo = 2 * Hp;
      if (gblk) {
        d.hprev_b = sr + (long)(i + 1) * Bs * 2 * Hp + (long)Hp * 16; d.hp_blk = (long)2 * Hp * 16;
        d.hout_b = sr + (long)i * Bs * 2 * Hp + (long)Hp * 16; d.ho_blk = (long)2 * Hp * 16;
      }
    } else {
      d.hprev = w.pr[(st + 1) & 1]; d.ldh = Hp;
      if (st == T - 1) { d.hout = w.ytop + Hp; d.ldo = 2 * Hp; }
      else { d.hout = w.pr[st & 1]; d.ldo = Hp; }
      if (gblk) { d.hprev_b = d.hprev; d.hp_blk = (long)Hp * 16; if (st < T - 1) { d.hout_b = d.hout; d.ho_blk = (long)Hp * 16; } }
    }
  }
  if (!top) {  // gru_rec, forward direction
    RefDir& d = dir(2, w.grf, T - 1 - st, st);
    d.hprev = sr + (long)(st - 1) * Bs * 2 * Hp; d.ldh = 2 * Hp;
    d.hout = sr + (long)st * Bs * 2 * Hp; d.ldo = 2 * Hp;
    if (gblk) { d.hprev_b = d.hprev; d.hp_blk = (long)2 * Hp * 16; d.hout_b = d.hout; d.ho_blk = (long)2 * Hp * 16; }
  }
  return a;
}

static RefArgs ref_cell_top_rec_fwd(const RefWs& w, int Hp, int l, bool gblk) {
  const int H3 = 3 * Hp;
  RefArgs a{};
  a.first = 1; a.ndir = 1;
  RefDir& d = a.d[0];
  if (l == 0) { d.frame = -1; }                // src.single
  else { d.gi = w.grf; d.ldgi = H3; d.gi_blk = gblk ? (long)H3 * 16 : 0; }
  d.hout = w.ytop; d.ldo = 2 * Hp;
  return a;
}

// ---------------------------------------------------------------- the comparison
struct Case { int L, Hp, B, T; bool h3, scaled, gblk, gran; };
#define CASE_FMT "L %d Hp %d B %d T %d h3 %d scaled %d gblk %d gran %d"
#define CASE_ARGS(c) c.L, c.Hp, c.B, c.T, (int)c.h3, (int)c.scaled, (int)c.gblk, (int)c.gran

static Addr addr(size_t off) { return off == kNoRef ? 0 : kBase + (Addr)off; }

// (b): one reference in its three forms against the old expressions: row-major address + ld, the planes EncWs::view found for that address in the
// forward's format, the blocked base + stride (0 / 0 where the old code left them unset)
static void same_ref(const Case& c, const char* what, int l, int st, int k, const StateRef& r, const RefWs& rw, Addr p, long ld, bool mirrored, Addr pb, long blk) {
  if (addr(r.f) != p || r.ld != ld) FAIL(CASE_FMT " layer %d step %d dir %d %s: rows %lld ld %ld, reference %lld ld %ld", CASE_ARGS(c), l, st, k, what, addr(r.f) - kBase, r.ld, p - kBase, ld);
  if (mirrored) {
    const RefPlanes v = rw.view(p, c.scaled ? 16 : 32);
    if (v.e < 0 || (long long)r.p != v.e || r.kst != v.kst) FAIL(CASE_FMT " layer %d step %d dir %d %s: planes %lld kst %ld, reference %lld kst %ld", CASE_ARGS(c), l, st, k, what, (long long)r.p, r.kst, v.e, v.kst);
  } else if (r.p != kNoRef) FAIL(CASE_FMT " layer %d step %d dir %d %s: planes of a buffer without mirror", CASE_ARGS(c), l, st, k, what);
  if (addr(r.b) != pb || r.bst != blk) FAIL(CASE_FMT " layer %d step %d dir %d %s: blocked %lld stride %ld, reference %lld stride %ld", CASE_ARGS(c), l, st, k, what, addr(r.b) - kBase, r.bst, pb - kBase, blk);
}

static bool same3(const StateRef& a, const StateRef& b) { return a.f == b.f && a.ld == b.ld && a.p == b.p && a.kst == b.kst && a.b == b.b && a.bst == b.bst; }
static bool none(const StateRef& r) { return r.f == kNoRef && r.p == kNoRef && r.b == kNoRef && r.ld == 0 && r.kst == 0 && r.bst == 0; }

// (c): rows x width elements from reference r lie inside ONE carved buffer, in every form r has
static void inside(const Case& c, const char* what, int l, int st, int k, const EncLayout& w, const StateRef& r, size_t width) {
  const StateBuf* all[] = {&w.gf, &w.grr, &w.grf, &w.sf[0], &w.sr[0], &w.pf[0], &w.pr[0], &w.sf[1], &w.sr[1], &w.pf[1], &w.pr[1], &w.ytop};
  const StateBuf* in = nullptr;
  for (const StateBuf* b : all)
    if (b->T && r.f >= b->off && r.f < b->off + b->floats()) { if (in) FAIL(CASE_FMT " buffers overlap at %zu", CASE_ARGS(c), r.f); in = b; }
  if (!in) { FAIL(CASE_FMT " layer %d step %d dir %d %s: rows at %zu in no buffer", CASE_ARGS(c), l, st, k, what, r.f); return; }
  const size_t rows = in->Bs, end = in->off + in->floats(), rel = r.f - in->off, row0 = rel / in->C, c0 = rel % in->C;
  if (r.ld != (long)in->C || c0 + width > in->C || row0 % in->Bs != 0 || r.f + (rows - 1) * (size_t)r.ld + width > end)
    FAIL(CASE_FMT " layer %d step %d dir %d %s: rows leave their buffer", CASE_ARGS(c), l, st, k, what);
  if (r.p != kNoRef) {
    // the view's corner elements through the format's own index function, from the buffer's mirror
    const long R = (long)(in->T * in->Bs);
    const long first = c.scaled ? plane16_index((long)row0, (long)c0, R) : plane_index((long)row0, (long)c0, R);
    const long lastk = c.scaled ? plane16_index((long)(row0 + rows - 1), (long)(c0 + width - 1), R) : plane_index((long)(row0 + rows - 1), (long)(c0 + width - 1), R);
    if (in->poff == kNoRef || r.p != in->poff + (size_t)first || r.kst != R * (c.scaled ? 16 : 32) || (size_t)lastk >= in->floats() || in->poff + in->floats() > w.plane_halfs ||
        row0 % 16 != 0 || c0 % 32 != 0)
      FAIL(CASE_FMT " layer %d step %d dir %d %s: planes leave their mirror", CASE_ARGS(c), l, st, k, what);
  }
  if (r.b != kNoRef) {
    // whole row tiles: a ragged last tile's blocks are as long as a whole one's, so no blocked buffer may have a ragged number of rows
    const bool ragged = rows % 16 != 0;
    if (ragged || r.bst != (long)in->C * 16 || r.b != in->off + row0 * in->C + c0 * 16 || r.b >= end ||
        (rows >= 16 && r.b + (rows / 16 - 1) * (size_t)r.bst + width * 16 > end))
      FAIL(CASE_FMT " layer %d step %d dir %d %s: blocks leave their buffer", CASE_ARGS(c), l, st, k, what);
  }
}

static void check(const Case& c) {
  const int L = c.L, Hp = c.Hp, T = c.T;
  const size_t sync_words = (size_t)L * 96 + 32 + 96 + 32, gran_words = c.gran ? (size_t)3 * 2 * 4 * Hp * 2 : 0;
  RefCarver rc;
  RefWs rw;
  ref_carve(L, (size_t)Hp, c.B, T, c.h3, c.gblk, sync_words, gran_words, rc, rw);
  Carve cv;
  const EncLayout w = carve_encoder(EncShape{L, Hp, c.B, T, c.h3, c.scaled, c.gblk, sync_words, gran_words}, cv);

  // (a) offsets
  const struct { const char* name; size_t got; Addr want; } offs[] = {
      {"sync", w.sync, rw.sync}, {"gran", w.gran, rw.gran}, {"xp", w.xp, rw.xp}, {"g0", w.g0, rw.g0}, {"g0c", w.g0c, rw.g0c}, {"gf", w.gf.off, rw.gf},
      {"grr", w.grr.off, rw.grr}, {"grf", w.grf.off, rw.grf}, {"sf0", w.sf[0].off, rw.sf[0]}, {"sr0", w.sr[0].off, rw.sr[0]}, {"pf0", w.pf[0].off, rw.pf[0]},
      {"pr0", w.pr[0].off, rw.pr[0]}, {"sf1", w.sf[1].off, rw.sf[1]}, {"sr1", w.sr[1].off, rw.sr[1]}, {"pf1", w.pf[1].off, rw.pf[1]}, {"pr1", w.pr[1].off, rw.pr[1]},
      {"ytop", w.ytop.off, rw.ytop}, {"y1", w.y1, rw.y1}, {"state_hi", w.state_hi, rw.state_hi}, {"state_lo", w.state_lo, rw.state_lo}, {"x0h", w.x0h, rw.x0h},
      {"x0l", w.x0l, rw.x0l}, {"rs", w.rs, rw.rs}, {"rs0", w.rs0, rw.rs0}, {"tailA.hi", w.tailA.hi, rw.tail_hi}, {"tailA.lo", w.tailA.lo, rw.tail_lo}};
  for (const auto& o : offs)
    if (addr(o.got) != o.want) FAIL(CASE_FMT " offset of %s: %zu, reference %lld", CASE_ARGS(c), o.name, o.got, o.want - kBase);
  if (cv.cur != rc.cur) FAIL(CASE_FMT " total %zu, reference %zu", CASE_ARGS(c), cv.cur, rc.cur);
  // (the exact-fp32 path carves no mirror: the old registry counted halfs there that nothing used)
  if (w.plane_halfs != (c.h3 ? rw.plane_halfs : 0) || w.Bs != rw.Bs || w.tailA.kst != rw.tail_kst) FAIL(CASE_FMT " plane_halfs / Bs / tail kst", CASE_ARGS(c));
  // the mirrored buffers, in registry order
  {
    const StateBuf* mir[9]; int n = 0;
    for (int i = 0; i < 2; ++i) {
      if (w.sf[i].T) { mir[n++] = &w.sf[i]; mir[n++] = &w.sr[i]; }
      mir[n++] = &w.pf[i]; mir[n++] = &w.pr[i];
    }
    mir[n++] = &w.ytop;
    if (n != rw.nbufs) FAIL(CASE_FMT " %d mirrored buffers, reference %d", CASE_ARGS(c), n, rw.nbufs);
    for (int i = 0; i < n && i < rw.nbufs; ++i) {
      const RefWs::Buf& b = rw.bufs[i];
      if (addr(mir[i]->off) != b.base || mir[i]->T != b.T || mir[i]->Bs != b.B || mir[i]->C != b.C || mir[i]->poff != (c.h3 ? b.poff : kNoRef)) FAIL(CASE_FMT " mirrored buffer %d", CASE_ARGS(c), i);
    }
  }

  // tail operand: tailF = K range [0, Hp) = the operand's start; tailR from Hp; the persistent kernel's r_off[0], x_roff, r_off[1] (launch_layer_seq)
  if (c.h3 && (long long)w.tailA.k(Hp) != rw.tailR_off) FAIL(CASE_FMT " tailR", CASE_ARGS(c));
  if (w.tailA.k(0) != 0 || w.tailA.k(Hp) != (size_t)(Hp / 32) * rw.tail_kst || w.tailA.k(2 * Hp) != (size_t)(2 * Hp / 32) * rw.tail_kst) FAIL(CASE_FMT " tail r_off / x_roff", CASE_ARGS(c));
  // (c) ... which are three consecutive K ranges of Hp columns that fill the [B x 3Hp] planes exactly
  if (w.tailA.k(Hp) - w.tailA.k(0) != (size_t)c.B * Hp || w.tailA.k(2 * Hp) - w.tailA.k(Hp) != (size_t)c.B * Hp || w.tailA.k(3 * Hp) != (size_t)c.B * 3 * Hp)
    FAIL(CASE_FMT " tail K ranges", CASE_ARGS(c));

  // the input views of layer_projections (layers >= 1 read the states of the layer below) and ytop's view
  if (c.h3) {
    for (int l = 1; l < L; ++l) {
      same_ref(c, "projection input sf", l, 0, 0, w.sf[(l - 1) & 1].at(0), rw, rw.sf[(l - 1) & 1], Hp, true, c.gblk ? rw.sf[(l - 1) & 1] : 0, c.gblk ? (long)Hp * 16 : 0);
      same_ref(c, "projection input sr", l, 0, 0, w.sr[(l - 1) & 1].at(0), rw, rw.sr[(l - 1) & 1], 2 * Hp, true, c.gblk ? rw.sr[(l - 1) & 1] : 0, c.gblk ? (long)2 * Hp * 16 : 0);
    }
  }

  for (int l = 0; l < L; ++l) {
    const bool top = l == L - 1;
    CellStep prev;
    for (int st = 0; st < T; ++st) {
      const CellStep s = cell_step(w, L, T, l, st);
      const RefArgs a = ref_cell_dirs(rw, L, Hp, T, l, st, c.gblk);
      if (s.ndir != a.ndir || (int)s.first != a.first || s.ndir != (top ? 2 : 3) || s.first != (st == 0)) FAIL(CASE_FMT " layer %d step %d: ndir / first", CASE_ARGS(c), l, st);
      for (int k = 0; k < s.ndir; ++k) {
        const DirStep& d = s.d[k];
        const RefDir& r = a.d[k];
        // (b)
        if (l == 0) { if (d.frame != r.frame || !none(d.gi)) FAIL(CASE_FMT " layer 0 step %d dir %d: frame %d, reference %d", CASE_ARGS(c), st, k, d.frame, r.frame); }
        else same_ref(c, "gi", l, st, k, d.gi, rw, r.gi, r.ldgi, false, r.gi_blk ? r.gi : 0, r.gi_blk);
        same_ref(c, "hout", l, st, k, d.hout, rw, r.hout, r.ldo, c.h3, r.hout_b, r.ho_blk);
        if (st > 0) same_ref(c, "hprev", l, st, k, d.hprev, rw, r.hprev, r.ldh, c.h3, r.hprev_b, r.hp_blk);
        // (c)
        if (st == 0 && !none(d.hprev)) FAIL(CASE_FMT " layer %d dir %d: a first step with a previous state", CASE_ARGS(c), l, k);
        if (st > 0 && !same3(d.hprev.rows_only(), prev.d[k].hout.rows_only())) FAIL(CASE_FMT " layer %d step %d dir %d: hprev is not the hout of the step before", CASE_ARGS(c), l, st, k);
        // (blocked: the hand-over is blocked wherever the plan blocks states at all -- every hprev then has the form, and it is its producer's)
        if (st > 0 && (d.hprev.b != prev.d[k].hout.b || d.hprev.bst != prev.d[k].hout.bst || (d.hprev.b != kNoRef) != c.gblk))
          FAIL(CASE_FMT " layer %d step %d dir %d: blocked hprev is not the blocked hout of the step before", CASE_ARGS(c), l, st, k);
        if (l > 0) inside(c, "gi", l, st, k, w, d.gi, 3 * (size_t)Hp);
        inside(c, "hout", l, st, k, w, d.hout, Hp);
        if (st > 0) inside(c, "hprev", l, st, k, w, d.hprev, Hp);
      }
      const size_t i = (size_t)(T - 1 - st), slabH = w.Bs * Hp;
      if (l == 0 && (s.d[0].frame != st || s.d[1].frame != st || (!top && s.d[2].frame != (int)i))) FAIL(CASE_FMT " layer 0 step %d: frames", CASE_ARGS(c), st);
      if (l > 0 && (s.d[0].gi.f != w.gf.off + st * 3 * slabH || s.d[1].gi.f != w.grr.off + i * 3 * slabH || (!top && s.d[2].gi.f != w.grf.off + st * 3 * slabH)))
        FAIL(CASE_FMT " layer %d step %d: gate pre-activation slabs", CASE_ARGS(c), l, st);
      if (!top) {
        const StateBuf &sf = w.sf[l & 1], &sr = w.sr[l & 1];
        if (s.d[0].hout.f != sf.off + st * slabH || s.d[1].hout.f != sr.off + i * 2 * slabH + Hp || s.d[2].hout.f != sr.off + st * 2 * slabH)
          FAIL(CASE_FMT " layer %d step %d: state slabs (reverse index T - 1 - st)", CASE_ARGS(c), l, st);
      } else {
        const bool last = st == T - 1;
        if (s.d[0].hout.f != w.pf[st & 1].off || s.d[0].hout.ld != Hp) FAIL(CASE_FMT " top step %d: forward state not in pf[st & 1]", CASE_ARGS(c), st);
        if (!last && (s.d[1].hout.f != w.pr[st & 1].off || s.d[1].hout.ld != Hp)) FAIL(CASE_FMT " top step %d: reverse state not in pr[st & 1]", CASE_ARGS(c), st);
        if (last && (s.d[1].hout.f != w.ytop.off + Hp || s.d[1].hout.ld != 2 * Hp)) FAIL(CASE_FMT " top: last reverse state not in ytop + Hp", CASE_ARGS(c));
        if (last && (s.d[0].hout.b != kNoRef || s.d[1].hout.b != kNoRef)) FAIL(CASE_FMT " top: a last state in blocks (the tail reads rows)", CASE_ARGS(c));
        if (!last && ((s.d[0].hout.b != kNoRef) != c.gblk || (s.d[1].hout.b != kNoRef) != c.gblk)) FAIL(CASE_FMT " top step %d: blocked form", CASE_ARGS(c), st);
      }
      prev = s;
    }
    if (top) {
      const CellStep x = cell_top_rec_fwd(w, l);
      const RefArgs a = ref_cell_top_rec_fwd(rw, Hp, l, c.gblk);
      const DirStep& d = x.d[0];
      if (x.ndir != 1 || !x.first || !none(d.hprev)) FAIL(CASE_FMT " extra step: ndir / first / hprev", CASE_ARGS(c));
      if (l == 0) { if (d.frame != a.d[0].frame || !none(d.gi)) FAIL(CASE_FMT " extra step of layer 0: not the single-step source", CASE_ARGS(c)); }
      else { same_ref(c, "extra gi", l, 0, 0, d.gi, rw, a.d[0].gi, a.d[0].ldgi, false, a.d[0].gi_blk ? a.d[0].gi : 0, a.d[0].gi_blk); inside(c, "extra gi", l, 0, 0, w, d.gi, 3 * (size_t)Hp); }
      same_ref(c, "extra hout", l, 0, 0, d.hout, rw, a.d[0].hout, a.d[0].ldo, c.h3, 0, 0);       // (with ytop's view of launch_layer_seq: x_poff, x_pkst)
      inside(c, "extra hout", l, 0, 0, w, d.hout, Hp);
      if (d.hout.f != w.ytop.off || d.hout.ld != 2 * Hp) FAIL(CASE_FMT " extra step does not write ytop", CASE_ARGS(c));
    }
  }
}

int main() {
  const int Ls[] = {1, 2, 3}, Hps[] = {64, 256}, Bs[] = {1, 15, 16, 17, 128}, Ts[] = {1, 2, 3, 5, 36};
  const bool flags[4][3] = {{false, false, false}, {true, false, false}, {true, true, false}, {true, true, true}};   // exact | h3 | h3 + scaled | h3 + scaled + gblk
  int combos = 0;
  for (int L : Ls)
    for (int Hp : Hps)
      for (int B : Bs)
        for (int T : Ts)
          for (const auto& f : flags)
            for (int gran = 0; gran <= 1; ++gran) { check(Case{L, Hp, B, T, f[0], f[1], f[2], gran != 0}); ++combos; }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok %d\n", combos);
  return 0;
}
