/* Host check of every workspace layout of forward.hip besides the encoder's own (tepose_amd/csrc/state.h: carve_regressor, carve_smpl_bwd,
 * carve_projection, carve_vibe, forward_layout, forward_bytes), compiled with the host compiler alone: tests/test_state_layout.py.  Every expectation is
 * WRITTEN OUT here -- the running sums and formulas forward.hip carried before the layouts moved into state.h, with the widths as literals -- and never
 * taken from the function under test:
 *   (a) regressor, N x {exact, h3, h3 + blend16} x L (the sync region's size): every offset and the total equal the longhand running sum in carve order,
 *       256-byte rounding included; every carved buffer starts on a 256-byte boundary and ends before the next one starts; what the shape does not have is
 *       kNoRef; the SMPL backward's five buffers follow the regressor's total in shapes.h smpl_bwd_floats order;
 *   (b) projection, M x {exact, h3}: one plane block with the lo plane as many halfs behind the hi plane as the padded rows take floats (M x 2144 for an
 *       even M; an odd M's rows are rounded up to the carve's 256 bytes first), both planes inside it, the bytes tepose_project_frames_workspace_bytes
 *       answered before -- 18176 for one row, the figure tests/golden/blob_layout.json pins;
 *   (c) VIBE, the shapes of tests/golden/make_golden_layout.py: the carve's end + 256 equals the formula tepose_vibe_workspace_bytes used to be;
 *   (d) a whole forward, the encoder shapes of state_layout_check.cpp x what the plans of B and of 2 B rows keep for the regressor: in a workspace of
 *       forward_bytes, and of 1, 255, 256 and 257 bytes more, the feature slot [feat, feat + 2 B x 2048 floats) lies inside the workspace, starts on a
 *       256-byte boundary and behind the scratch; the encoder's carve for (B, T) and the regressor's for N = B both end inside the scratch; both put
 *       the sync region at offset 0; forward_bytes is the sequential sum encoder + feature + regressor(2 B) + 256.
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure. */
#include <cstdio>
#include <algorithm>
#include <vector>

#include "state.h"

using namespace tepose;

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the running sum the carves used to be: n floats from byte `cur` on, the next buffer on the next 256-byte boundary
struct Sum {
  size_t cur = 0;
  size_t f(size_t n) { const size_t o = cur / 4; cur = up256(cur + n * 4); return o; }
};

struct Named { const char* name; size_t got, want, floats; bool have; };

static void same(const char* what, int N, int flags, int L, const std::vector<Named>& bufs, size_t got_total, size_t want_total) {
  for (const Named& b : bufs) {
    if (!b.have) { if (b.got != kNoRef) FAIL("%s N %d flags %d L %d: absent %s has offset %zu", what, N, flags, L, b.name, b.got); continue; }
    if (b.got != b.want) FAIL("%s N %d flags %d L %d: %s at %zu, longhand %zu", what, N, flags, L, b.name, b.got, b.want);
    if (b.got * 4 % 256 != 0) FAIL("%s N %d flags %d L %d: %s not on a 256-byte boundary", what, N, flags, L, b.name);
  }
  if (got_total != want_total) FAIL("%s N %d flags %d L %d: total %zu, longhand %zu", what, N, flags, L, got_total, want_total);
  std::vector<Named> s;
  for (const Named& b : bufs) if (b.have && b.got != kNoRef) s.push_back(b);
  std::sort(s.begin(), s.end(), [](const Named& a, const Named& b) { return a.got < b.got; });
  for (size_t i = 0; i < s.size(); ++i) {
    const size_t end = i + 1 < s.size() ? s[i + 1].got : got_total / 4;
    if (s[i].got + s[i].floats > end) FAIL("%s N %d flags %d L %d: %s runs into the next buffer", what, N, flags, L, s[i].name);
  }
}

// ---------------------------------------------------------------- (a)
static void check_regressor(int N, int flags, int L) {
  const bool h3 = flags >= 1, b16 = flags >= 2;
  const size_t n = (size_t)N, sync_words = (size_t)L * 96 + 32 + 96 + 32;
  // today's order: sync; hi, lo of feat, xs, h1, h2, pf; base; rows of h1, h2, xs, pf; amat, posed, vposed; scaled planes hi, lo; row scales
  Sum s;
  const size_t widths[5] = {2048, 160, 1024, 1024, 224};
  size_t hi[5], lo[5];
  const size_t sync = s.f(sync_words);
  for (int i = 0; i < 5; ++i) { hi[i] = s.f(h3 ? n * widths[i] / 2 + 64 : 0); lo[i] = s.f(h3 ? n * widths[i] / 2 + 64 : 0); }
  const size_t base = s.f(n * 1024), h1 = s.f(n * 1024), h2 = s.f(n * 1024), xs = s.f(n * 160), pf = s.f(n * 224);
  const size_t amat = s.f(n * 24 * 12), posed = s.f(n * 24 * 3), vposed = s.f(n * 20672);
  const size_t p16h = s.f(b16 ? n * 224 / 2 : 0), p16l = s.f(b16 ? n * 224 / 2 : 0), rs = s.f(b16 ? n : 0);

  const RegShape shape{N, h3, b16, sync_words};
  Carve c;
  const RegLayout w = carve_regressor(shape, c);
  const RegAct* acts[5] = {&w.feat, &w.xs, &w.h1, &w.h2, &w.pf};
  const char* hn[5] = {"feat.hi", "xs.hi", "h1.hi", "h2.hi", "pf.hi"};
  const char* ln[5] = {"feat.lo", "xs.lo", "h1.lo", "h2.lo", "pf.lo"};
  std::vector<Named> bufs{{"sync", w.sync, sync, sync_words, true}, {"base", w.base, base, n * 1024, true}, {"h1", w.h1.rows, h1, n * 1024, true},
                          {"h2", w.h2.rows, h2, n * 1024, true}, {"xs", w.xs.rows, xs, n * 160, true}, {"pf", w.pf.rows, pf, n * 224, true},
                          {"amat", w.amat, amat, n * 288, true}, {"posed", w.posed, posed, n * 72, true}, {"vposed", w.vposed, vposed, n * 20672, true},
                          {"pf16.hi", w.pf16h, p16h, n * 112, b16}, {"pf16.lo", w.pf16l, p16l, n * 112, b16}, {"pfrs", w.pfrs, rs, n, b16}};
  for (int i = 0; i < 5; ++i) {
    // (a plane of N x C halfs is N x C / 2 floats: the 64 more are the carve's slack behind it)
    bufs.push_back({hn[i], acts[i]->P.hi, hi[i], n * widths[i] / 2 + 64, h3});
    bufs.push_back({ln[i], acts[i]->P.lo, lo[i], n * widths[i] / 2 + 64, h3});
    if (acts[i]->ld != (long)widths[i] || acts[i]->P.kst != (long)N * 32) FAIL("regressor N %d flags %d: ld / kst of activation %d", N, flags, i);
  }
  if (w.feat.rows != kNoRef) FAIL("regressor N %d flags %d: feat has rows (they are the caller's)", N, flags);
  same("regressor", N, flags, L, bufs, c.cur, s.cur);

  // the backward's buffers behind it: joint sources, g_vposed, skinning partials, split-K partials, their sum
  const SmplBwdFloats f = smpl_bwd_floats(N);
  const size_t gsrc = s.f(f.gsrc), gvp = s.f(f.gvp), skin = s.f(f.skin_part), blend = s.f(f.blend_part), gf = s.f(f.gf);
  Carve cb;
  const SmplBwdLayout b = carve_smpl_bwd(shape, cb);
  if (gsrc != c.cur / 4) FAIL("backward N %d flags %d: the longhand sum does not start at the regressor's total", N, flags);
  if (b.fwd.sync != w.sync || b.fwd.base != w.base || b.fwd.vposed != w.vposed || b.fwd.pf.rows != w.pf.rows || b.fwd.pf.P.hi != w.pf.P.hi || b.fwd.pf.P.lo != w.pf.P.lo ||
      b.fwd.amat != w.amat || b.fwd.posed != w.posed || b.fwd.pf16h != w.pf16h || b.fwd.pf16l != w.pf16l || b.fwd.pfrs != w.pfrs)
    FAIL("backward N %d flags %d: the forward's buffers are not the regressor's", N, flags);
  same("backward", N, flags, L, {{"gsrc", b.gsrc, gsrc, f.gsrc, true}, {"gvp", b.gvp, gvp, f.gvp, true}, {"skin_part", b.skin_part, skin, f.skin_part, true},
                                 {"blend_part", b.blend_part, blend, f.blend_part, true}, {"gf", b.gf, gf, f.gf, true}}, cb.cur, s.cur);
}

// ---------------------------------------------------------------- (b)
static void check_projection(size_t M, bool h3) {
  Carve c;
  const ProjLayout w = carve_projection(M, h3, c);
  const size_t xbytes = up256(M * 2144 * 4);
  if (w.xp != 0) FAIL("projection M %zu: rows at %zu", M, w.xp);
  if (!h3) {
    if (w.P.hi != kNoRef || w.P.lo != kNoRef || w.rs != kNoRef || w.P.kst != 0 || c.cur != xbytes) FAIL("projection M %zu exact: planes, scales or bytes %zu", M, c.cur);
    return;
  }
  // today's: the rows; one block of xbytes / 4 + 128 floats with the lo plane xbytes / 4 halfs in; M row scales
  const size_t block = xbytes / 4, block_bytes = up256((xbytes / 4 + 128) * 4), bytes = xbytes + block_bytes + up256(M * 4);
  if (w.P.hi != block) FAIL("projection M %zu: hi plane at %zu", M, w.P.hi);
  const size_t lo_halfs = (w.P.lo - w.P.hi) * 2;
  if (w.P.lo == kNoRef || lo_halfs != xbytes / 4) FAIL("projection M %zu: lo plane %zu halfs behind hi, longhand %zu", M, lo_halfs, xbytes / 4);
  if (M % 2 == 0 && lo_halfs != M * 2144 * 4 / 4) FAIL("projection M %zu: lo plane %zu halfs behind hi, not M x 2144", M, lo_halfs);
  if (lo_halfs < M * 2144 || (lo_halfs + M * 2144) * 2 > block_bytes) FAIL("projection M %zu: the planes overlap or leave their block", M);
  if (w.rs != (xbytes + block_bytes) / 4 || w.P.kst != (long)M * 32) FAIL("projection M %zu: row scales at %zu / kst %ld", M, w.rs, w.P.kst);
  if (c.cur != bytes) FAIL("projection M %zu: %zu bytes, longhand %zu", M, c.cur, bytes);
  if (M == 1 && c.cur != 18176) FAIL("projection of one row: %zu bytes, the golden layout has 18176", c.cur);
}

// ---------------------------------------------------------------- (c)
static void check_vibe(size_t BN, size_t D, size_t Hp) {
  Carve c;
  const VibeLayout w = carve_vibe(BN, D, Hp, c);
  const size_t g = up256(BN * D * 3 * Hp * 4), st = up256(BN * D * Hp * 4);
  if (w.G != 0 || w.S[0] != g / 4 || w.S[1] != (g + st) / 4) FAIL("vibe BN %zu D %zu Hp %zu: offsets %zu %zu %zu", BN, D, Hp, w.G, w.S[0], w.S[1]);
  if (c.cur + 256 != g + 2 * st + 256) FAIL("vibe BN %zu D %zu Hp %zu: %zu bytes, formula %zu", BN, D, Hp, c.cur + 256, g + 2 * st + 256);
}

// ---------------------------------------------------------------- (d)
static void check_forward(const EncShape& e, int fb, int f2b) {
  const size_t B = (size_t)e.B, feat_floats = 2 * B * 2048;
  const RegShape rb{e.B, fb >= 1, fb >= 2, e.sync_words}, r2{2 * e.B, f2b >= 1, f2b >= 2, e.sync_words};
  Carve ce, cr, cr2;
  const EncLayout we = carve_encoder(e, ce);
  const RegLayout wr = carve_regressor(rb, cr);
  carve_regressor(r2, cr2);
  if (we.sync != 0 || wr.sync != 0) FAIL("forward B %d T %d: sync regions at %zu / %zu, not at the base", e.B, e.T, we.sync, wr.sync);
  const size_t bytes = forward_bytes(e, r2);
  if (bytes != ce.cur + up256(feat_floats * 4) + cr2.cur + 256) FAIL("forward B %d T %d L %d: %zu bytes, not the sequential sum", e.B, e.T, e.L, bytes);
  const size_t more[5] = {0, 1, 255, 256, 257};
  for (size_t k : more) {
    const size_t ws = bytes + k;
    const FwdLayout f = forward_layout(ws, e.B);
    if (f.feat * 4 + feat_floats * 4 > ws) FAIL("forward B %d T %d L %d + %zu: the feature slot leaves the workspace", e.B, e.T, e.L, k);
    if (f.feat * 4 % 256 != 0) FAIL("forward B %d T %d L %d + %zu: the feature slot starts at byte %zu", e.B, e.T, e.L, k, f.feat * 4);
    if (f.feat * 4 < f.scratch_bytes) FAIL("forward B %d T %d L %d + %zu: the feature slot overlaps the scratch", e.B, e.T, e.L, k);
    if (ce.cur > f.scratch_bytes) FAIL("forward B %d T %d L %d + %zu: the encoder (%zu bytes) leaves the scratch (%zu)", e.B, e.T, e.L, k, ce.cur, f.scratch_bytes);
    if (cr.cur > f.scratch_bytes) FAIL("forward B %d T %d L %d flags %d / %d + %zu: the regressor (%zu bytes) leaves the scratch (%zu)", e.B, e.T, e.L, fb, f2b, k, cr.cur, f.scratch_bytes);
  }
}

int main() {
  int combos = 0;
  const int Ns[] = {1, 3, 4, 5, 16, 17, 40, 130, 4096};
  for (int N : Ns)
    for (int flags = 0; flags < 3; ++flags)       // exact | h3 | h3 + blend16
      for (int L = 1; L <= 3; ++L) { check_regressor(N, flags, L); ++combos; }
  const size_t Ms[] = {1, 2, 3, 16, 17, 128, 1400, 16384};
  for (size_t M : Ms)
    for (int h3 = 0; h3 <= 1; ++h3) { check_projection(M, h3 != 0); ++combos; }
  const size_t BNs[] = {1 * 16, 64 * 16, 700 * 3, 8192 * 16}, vHp[] = {64, 128, 2048};
  for (size_t BN : BNs)
    for (size_t D = 1; D <= 2; ++D)
      for (size_t Hp : vHp) { check_vibe(BN, D, Hp); ++combos; }
  const int Ls[] = {1, 2, 3}, Hps[] = {64, 256}, Bs[] = {1, 15, 16, 17, 128}, Ts[] = {1, 2, 3, 5, 36};
  const bool eflags[4][3] = {{false, false, false}, {true, false, false}, {true, true, false}, {true, true, true}};   // exact | h3 | h3 + scaled | h3 + scaled + gblk
  for (int L : Ls)
    for (int Hp : Hps)
      for (int B : Bs)
        for (int T : Ts)
          for (const auto& f : eflags)
            for (int gran = 0; gran <= 1; ++gran)
              for (int fb = 0; fb < 3; ++fb)
                for (int f2b = 0; f2b < 3; ++f2b) {
                  check_forward(EncShape{L, Hp, B, T, f[0], f[1], f[2], (size_t)L * 96 + 32 + 96 + 32, gran ? (size_t)3 * 2 * 4 * Hp * 2 : 0}, fb, f2b);
                  ++combos;
                }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok %d\n", combos);
  return 0;
}
