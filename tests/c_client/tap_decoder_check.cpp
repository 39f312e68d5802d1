/* Host check of the decoder tap's views (tepose_amd/csrc/tap.h tap_decoder), compiled with the host compiler alone: tests/test_decoder_stages_helper.py.
 * For every N below and every combination of what the plan keeps (split planes, scaled planes, the small-N kernel, reg_seq_kernel's plane-only FC
 * activations), the layout is the regressor's own carve (state.h carve_regressor, the function tepose_decoder_tap runs) and every stage tap_decoder accepts
 * is walked element by element: tap_index against the offset WRITTEN OUT LONGHAND here for each form -- fp32 rows with the stage's own leading dimension
 * (20672 under the 20670 real columns of v_posed), blocked [K/32][R][32] planes with hi + lo / 2048, scaled [K/16][R][16] planes with hi + lo and a
 * per-row scale.  Also: what the plan never writes is refused, every offset stays inside its own buffer -- which ends where the carve's next buffer
 * begins --, and no two elements of a stage share an offset.
 * Prints one line per failure and "ok <combinations>"; exit status 1 on any failure. */
#include <cstdio>
#include <algorithm>
#include <vector>

#include "tap.h"

using namespace tepose;

static int failures = 0;
#define FAIL(...) do { if (++failures <= 40) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static size_t lh_rows(size_t base, long ld, long row, long col) { return base + (size_t)(row * ld + col); }
static size_t lh_planes32(long R, long row, long col) { return (size_t)(((col / 32) * R + row) * 32 + ((((col / 8) % 4) ^ ((row / 4) % 4)) * 8) + col % 8); }
static size_t lh_planes16(long R, long row, long col) { return (size_t)(((col / 16) * R + row) * 16 + ((((col / 8) % 2) ^ ((row / 8) % 2)) * 8) + col % 8); }

struct Buf { size_t off, floats; };

static void check(int N, bool h3, bool blend16, bool small, bool reg_seq) {
  Carve c;
  const RegLayout w = carve_regressor(RegShape{N, h3, blend16, 256}, c);
  // a buffer reaches as far as the next one the carve took (the last: the carve's end)
  std::vector<size_t> starts{w.sync, w.base, w.amat, w.posed, w.vposed, w.pf16h, w.pf16l, w.pfrs, c.cur / sizeof(float)};
  for (const RegAct* a : {&w.feat, &w.xs, &w.h1, &w.h2, &w.pf}) { starts.push_back(a->rows); starts.push_back(a->P.hi); starts.push_back(a->P.lo); }
  std::sort(starts.begin(), starts.end());
  auto buf = [&](size_t off) { return Buf{off, off == kNoRef ? 0 : *std::upper_bound(starts.begin(), starts.end(), off) - off}; };
  const Buf h1h = buf(w.h1.P.hi), h1l = buf(w.h1.P.lo), h2h = buf(w.h2.P.hi), h2l = buf(w.h2.P.lo), pfh = buf(w.pf.P.hi), pfl = buf(w.pf.P.lo);
  const Buf h1 = buf(w.h1.rows), h2 = buf(w.h2.rows), xs = buf(w.xs.rows), pf = buf(w.pf.rows);
  const Buf amat = buf(w.amat), posed = buf(w.posed), vposed = buf(w.vposed), p16h = buf(w.pf16h), p16l = buf(w.pf16l), rs = buf(w.pfrs);
  const DecPlan d{small, reg_seq, w.xs.rows};
  const int widths[kDecStages] = {160, 1024, 1024, 224, 224, 224, 288, 72, 20670};
  const Buf* rows[kDecStages] = {&xs, &h1, &h2, &pf, nullptr, nullptr, &amat, &posed, &vposed};
  const long lds[kDecStages] = {160, 1024, 1024, 224, 0, 0, 288, 72, 20672};
  TapView v;
  for (int stage = -1; stage <= kDecStages; ++stage) {
    const bool real = stage >= 0 && stage < kDecStages;
    const bool ok = real && !(small && (stage == kDecPf || stage == kDecPfPlanes || stage == kDecPf16 || stage == kDecVposed)) &&
                    !(stage == kDecPfPlanes && !h3) && !(stage == kDecPf16 && !blend16);
    if (tap_decoder(w, d, stage, N, &v) != ok) { FAIL("N=%d h3=%d b16=%d small=%d seq=%d stage %d: accepted %d", N, h3, blend16, small, reg_seq, stage, (int)!ok); continue; }
    if (!ok) continue;
    if (v.slabs != 1 || v.rows != N || v.cols != widths[stage] || v.cols != dec_cols(stage)) FAIL("N=%d stage %d: shape %d x %d x %d", N, stage, v.slabs, v.rows, v.cols);
    const bool seq_planes = reg_seq && (stage == kDecH1 || stage == kDecH2);
    const int form = stage == kDecPf16 ? kTapPlanes16 : (stage == kDecPfPlanes || seq_planes) ? kTapPlanes32 : kTapRows;
    if (v.form != form) FAIL("N=%d stage %d: form %d", N, stage, v.form);
    const Buf *hi = nullptr, *lo = nullptr;
    if (stage == kDecPfPlanes) { hi = &pfh; lo = &pfl; }
    if (stage == kDecPf16) { hi = &p16h; lo = &p16l; }
    if (seq_planes) { hi = stage == kDecH1 ? &h1h : &h2h; lo = stage == kDecH1 ? &h1l : &h2l; }
    if (form == kTapPlanes32 && (v.scale != 1.f || v.lo_scale != 1.f / 2048.f || v.rs >= 0 || v.hi != hi->off || v.lo != lo->off)) FAIL("N=%d stage %d: blocked planes' constants", N, stage);
    if (form == kTapPlanes16 && (v.scale != 1.f || v.lo_scale != 1.f || v.rs != (long)rs.off || v.hi != hi->off || v.lo != lo->off)) FAIL("N=%d stage %d: scaled planes' constants", N, stage);
    if (form == kTapRows && (size_t)N * lds[stage] > rows[stage]->floats) FAIL("N=%d stage %d: %d rows do not fit between the buffer and its neighbour", N, stage, N);
    if (form == kTapRows && (v.rs >= 0 || v.relu || v.c1 != 0)) FAIL("N=%d stage %d: row view's constants", N, stage);
    std::vector<size_t> seen;
    for (long row = 0; row < N; ++row)
      for (long col = 0; col < v.cols; ++col) {
        const size_t got = tap_index(v, 0, row, col);
        const size_t exp = form == kTapRows ? lh_rows(rows[stage]->off, lds[stage], row, col) : form == kTapPlanes32 ? lh_planes32(N, row, col) : lh_planes16(N, row, col);
        if (got != exp) { FAIL("N=%d stage %d element (%ld, %ld): %zu, longhand %zu", N, stage, row, col, got, exp); row = N; break; }
        if (form == kTapRows ? (got < rows[stage]->off || got >= rows[stage]->off + rows[stage]->floats) : (got / 2 >= hi->floats || got / 2 >= lo->floats)) { FAIL("N=%d stage %d: element leaves its buffer", N, stage); row = N; break; }
        seen.push_back(got);
      }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) FAIL("N=%d stage %d: two elements at one offset", N, stage);
    if (v.rs >= 0 && (size_t)v.rs + N > rs.off + rs.floats) FAIL("N=%d stage %d: row scales leave their buffer", N, stage);
  }
}

int main() {
  int n = 0;
  const int Ns[] = {1, 3, 4, 5, 17, 40, 130};
  // what select_kernels combines: exact | split | split + reg_seq_kernel | split + scaled pose-feature planes; the small-N kernel on either precision
  const bool flags[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 1}, {1, 1, 0, 0}, {0, 0, 1, 0}, {1, 0, 1, 0}, {1, 0, 1, 1}};
  for (int N : Ns)
    for (const auto& f : flags) {
      check(N, f[0], f[1], f[2], f[3]);
      ++n;
    }
  if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
  std::printf("ok %d\n", n);
  return 0;
}
