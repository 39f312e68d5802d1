/* Host check of the encoder tap's index arithmetic (tepose_amd/csrc/tap.h), compiled with the host compiler alone: tests/test_encoder_stages_helper.py.
 * For every L, Hp, B (ragged ones included), T and plan-flag combination below, every stage tap_resolve accepts is walked element by element (all of a small
 * stage, a stride of a large one) and tap_index compared with the offset WRITTEN OUT LONGHAND here from the buffer starts of state.h's carve (which
 * tests/test_state_layout.py pins): fp32 rows, 16 x 16 blocks of states and of gate pre-activations, blocked [K/32][R][32] and scaled [K/16][R][16] planes.
 * Also: what must not be tappable is refused, every offset stays inside the carve, and no two elements of a stage share an offset.
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure. */
#include <cstdio>
#include <algorithm>
#include <vector>

#include "tap.h"

using namespace tepose;

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

struct Case { int L, Hp, B, T; bool h3, scaled, gblk, g0blk, planes0, planes1; };
#define CF "L=%d Hp=%d B=%d T=%d h3=%d scaled=%d gblk=%d g0blk=%d planes=%d%d"
#define CA(c) c.L, c.Hp, c.B, c.T, (int)c.h3, (int)c.scaled, (int)c.gblk, (int)c.g0blk, (int)c.planes0, (int)c.planes1

// ---- longhand: element (row, col) of a [rows][C] matrix in each form
static size_t lh_rows(size_t base, long ld, long row, long col) { return base + (size_t)(row * ld + col); }
static size_t lh_state_blocks(size_t base, long C, long row, long unit) {      // 16 rows x 16 units = 256 floats, lane (unit % 16 / 4) * 16 + row % 16 holds 4 units
  return base + (size_t)((row / 16) * C * 16 + (unit / 16) * 256 + (((unit % 16) / 4) * 16 + row % 16) * 4 + unit % 4);
}
static size_t lh_gi_blocks(size_t base, long C, int Hp, long row, long col) {  // blocks of a row tile ordered [unit / 32][unit / 16 & 1][gate]
  const long gate = col / Hp, unit = col % Hp;
  return base + (size_t)((row / 16) * C * 16 + ((unit / 32) * 6 + ((unit / 16) % 2) * 3 + gate) * 256 + (((unit % 16) / 4) * 16 + row % 16) * 4 + unit % 4);
}
static size_t lh_planes32(size_t base, long R, long row, long col) {           // [K/32][R][32], 8-half slots XORed with (row / 4) % 4
  return base + (size_t)(((col / 32) * R + row) * 32 + ((((col / 8) % 4) ^ ((row / 4) % 4)) * 8) + col % 8);
}
static size_t lh_planes16(size_t base, long R, long row, long col) {           // [K/16][R][16], the two slots XORed with (row / 8) % 2
  return base + (size_t)(((col / 16) * R + row) * 16 + ((((col / 8) % 2) ^ ((row / 8) % 2)) * 8) + col % 8);
}

static void walk(const Case& c, const char* what, int l, int d, int st, const TapView& v, size_t total_floats, size_t (*want)(const void*, long, long, long), const void* ctx) {
  std::vector<size_t> seen;
  const long n = (long)v.count(), stride = n > 20000 ? 7 : 1;
  for (long i = 0; i < n; i += stride) {
    const long t = i / ((long)v.rows * v.cols), rem = i % ((long)v.rows * v.cols), row = rem / v.cols, col = rem % v.cols;
    const size_t got = tap_index(v, t, row, col), exp = want(ctx, t, row, col);
    if (got != exp) { FAIL(CF " %s(%d, %d, %d) form %d element (%ld, %ld, %ld): %zu, longhand %zu", CA(c), what, l, d, st, v.form, t, row, col, got, exp); return; }
    const bool planes = v.form == kTapPlanes32 || v.form == kTapPlanes16;
    const size_t fl = planes ? v.hi + got / 2 : got, fl2 = planes ? v.lo + got / 2 : got;
    if (fl >= total_floats || fl2 >= total_floats) { FAIL(CF " %s(%d, %d, %d): element leaves the workspace", CA(c), what, l, d, st); return; }
    seen.push_back(got);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) FAIL(CF " %s(%d, %d, %d): two elements at one offset", CA(c), what, l, d, st);
}

struct Ctx { const Case* c; const EncLayout* w; int l, d, st; };

// gi(l, d)[t][row][col]
static size_t want_gi(const void* p, long t, long row, long col) {
  const Ctx& x = *(const Ctx*)p;
  const Case& c = *x.c;
  const EncLayout& w = *x.w;
  const long H3 = 3L * c.Hp, ld0 = (c.L >= 2 ? 9L : 6L) * c.Hp;
  if (x.l == 0) {
    if (c.L == 1 && x.d == 2) return lh_rows(w.g0c, H3, row, col);
    if (c.g0blk) return lh_gi_blocks(w.g0 + (size_t)(x.d * H3 * 16), ld0, c.Hp, t * c.B + row, col);      // frame-major: row t B + b, direction d's blocks 3 Hp 16 floats on
    return lh_rows(w.g0, ld0, row * c.T + t, x.d * H3 + col);                                               // batch-major: row b T + t
  }
  const StateBuf& g = x.d == 0 ? w.gf : x.d == 1 ? w.grr : w.grf;
  const size_t base = g.off + (size_t)t * w.Bs * H3;
  return c.gblk ? lh_gi_blocks(base, H3, c.Hp, row, col) : lh_rows(base, H3, row, col);
}

// h(l, d, st)[row][unit]
static size_t want_h(const void* p, long, long row, long unit) {
  const Ctx& x = *(const Ctx*)p;
  const Case& c = *x.c;
  const EncLayout& w = *x.w;
  const long Hp = c.Hp, T = c.T, Bs = (long)w.Bs;
  const bool top = x.l == c.L - 1, planes = x.l == 0 ? c.planes0 : c.planes1;
  const StateBuf* b;
  long slab = 0, c0 = 0;
  bool rows_only = false;
  if (!top) {
    b = x.d == 0 ? &w.sf[x.l & 1] : &w.sr[x.l & 1];
    slab = x.d == 1 ? T - 1 - x.st : x.st;
    c0 = x.d == 1 ? Hp : 0;
  } else if (x.d == 2) { b = &w.ytop; rows_only = true; }
  else if (x.st == T - 1) { b = x.d == 0 ? &w.pf[x.st & 1] : &w.ytop; c0 = x.d == 1 ? Hp : 0; rows_only = true; }
  else b = x.d == 0 ? &w.pf[x.st & 1] : &w.pr[x.st & 1];
  const long C = (long)b->C, R = (long)(b->T * b->Bs);
  if (c.h3 && c.gblk && !rows_only) {
    if (planes) return c.scaled ? lh_planes16(b->poff, R, slab * Bs + row, c0 + unit) : lh_planes32(b->poff, R, slab * Bs + row, c0 + unit);
    return lh_state_blocks(b->off + (size_t)(slab * Bs * C), C, row, c0 + unit);
  }
  return lh_rows(b->off + (size_t)(slab * Bs * C), C, row, c0 + unit);
}

static size_t want_tail(const void* p, long, long row, long col) {
  const Ctx& x = *(const Ctx*)p;
  const Case& c = *x.c;
  const EncLayout& w = *x.w;
  if (c.h3) return lh_planes32(0, c.B, row, col);
  if (col < c.Hp) return lh_rows(w.pf[(c.T - 1) & 1].off, c.Hp, row, col);
  return lh_rows(w.ytop.off, 2L * c.Hp, row, col - c.Hp);
}

static void check(const Case& c) {
  Carve cv;
  const EncLayout w = carve_encoder(EncShape{c.L, c.Hp, c.B, c.T, c.h3, c.scaled, c.gblk, (size_t)c.L * 96 + 160, 0}, cv);
  const size_t total = cv.cur / sizeof(float);
  const TapPlan p{c.L, c.Hp, c.B, c.T, c.h3, c.g0blk, c.planes0, c.planes1};
  TapView v;
  for (int l = -1; l <= c.L; ++l)
    for (int d = -1; d <= 3; ++d) {
      const bool real = l >= 0 && l < c.L && d >= 0 && d <= 2, top = l == c.L - 1;
      // ---- gi: layer 0 and the top layer
      const bool gi_ok = real && (l == 0 || top);
      if (tap_resolve(w, p, kTapGi, l, d, 0, &v) != gi_ok) { FAIL(CF " gi(%d, %d): accepted %d", CA(c), l, d, (int)!gi_ok); continue; }
      if (gi_ok) {
        const int slabs = top && d == 2 ? 1 : c.T;
        const int form = (l == 0 ? c.g0blk && !(c.L == 1 && d == 2) : c.gblk) ? kTapGiBlocks : kTapRows;
        if (v.slabs != slabs || v.rows != c.B || v.cols != 3 * c.Hp || v.form != form) FAIL(CF " gi(%d, %d): shape %d x %d x %d form %d", CA(c), l, d, v.slabs, v.rows, v.cols, v.form);
        const Ctx x{&c, &w, l, d, 0};
        walk(c, "gi", l, d, 0, v, total, want_gi, &x);
      }
      // ---- h
      for (int st = -1; st <= c.T; ++st) {
        const bool in = real && st >= 0 && st < c.T;
        const bool h_ok = in && (top ? (d == 2 ? st == 0 : st >= c.T - 2) : !(l + 2 < c.L - 1));
        if (tap_resolve(w, p, kTapH, l, d, st, &v) != h_ok) { FAIL(CF " h(%d, %d, %d): accepted %d", CA(c), l, d, st, (int)!h_ok); continue; }
        if (!h_ok) continue;
        if (v.slabs != 1 || v.rows != c.B || v.cols != c.Hp) FAIL(CF " h(%d, %d, %d): shape", CA(c), l, d, st);
        if ((v.form == kTapPlanes16) != (c.scaled && (v.form == kTapPlanes16 || v.form == kTapPlanes32))) FAIL(CF " h(%d, %d, %d): plane format", CA(c), l, d, st);
        if (v.form == kTapPlanes16 && (v.scale != 1.f / 16384.f || v.lo_scale != 1.f || v.hi != w.state_hi || v.lo != w.state_lo)) FAIL(CF " h: scaled planes' constants", CA(c));
        if (v.form == kTapPlanes32 && (v.scale != 1.f || v.lo_scale != 1.f / 2048.f || v.hi != w.state_hi || v.lo != w.state_lo)) FAIL(CF " h: blocked planes' constants", CA(c));
        const Ctx x{&c, &w, l, d, st};
        walk(c, "h", l, d, st, v, total, want_h, &x);
      }
    }
  if (!tap_resolve(w, p, kTapTail, 0, 0, 0, &v) || v.rows != c.B || v.cols != 3 * c.Hp || v.relu != !c.h3 || (c.h3 && (v.hi != w.tailA.hi || v.lo != w.tailA.lo || v.lo_scale != 1.f / 2048.f)))
    FAIL(CF " tail: view", CA(c));
  const Ctx x{&c, &w, 0, 0, 0};
  walk(c, "tail", 0, 0, 0, v, total, want_tail, &x);
}

int main() {
  int n = 0;
  const int Ls[] = {1, 2, 3, 4}, Hps[] = {64, 192, 320}, Bs[] = {1, 5, 16, 37}, Ts[] = {1, 2, 4};
  // plan flags as select_kernels combines them: exact | split | scaled rows | scaled + blocked (fp32 states) | + planes on layers >= 1 | + frame-major layer 0 and planes everywhere
  const bool flags[][6] = {{0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0}, {1, 1, 1, 0, 0, 0}, {1, 1, 1, 0, 0, 1}, {1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 0, 0}};
  for (int L : Ls)
    for (int Hp : Hps)
      for (int B : Bs)
        for (int T : Ts)
          for (const auto& f : flags) {
            if (f[3] && B % 16 != 0) continue;                 // g0blk: whole row tiles per frame
            check(Case{L, Hp, B, T, f[0], f[1], f[2], f[3], f[4], f[5]});
            ++n;
          }
  if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
  std::printf("ok %d\n", n);
  return 0;
}
