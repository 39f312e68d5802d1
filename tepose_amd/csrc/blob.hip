// The packed blob: where every section lives (layout pass), how the caller's tensors get there (tepose_pack_*), and the derived sections -- the hi | lo
// fp16 planes the split-precision kernels read -- which one table describes and one function writes.  The layout pass leaves one record (model.h
// Weight) per matrix; nothing else writes a geometry number, and nothing else does offset arithmetic on the blob beyond a record's views.
// Pack time only: the functions here may synchronise the stream and read back.
#include <algorithm>

#include "hmr.h"
#include "model.h"

using namespace tepose;

namespace {

constexpr size_t kAlignF = 64;   // 256-byte sections

size_t take(size_t& cur, size_t n) {
  const size_t o = cur;
  cur = align_up(cur + n, kAlignF);
  return o;
}

// the packed fp32 section of a weight, [Np][Kp], and behind it its bias of nb floats (0: none, or carved elsewhere)
void take_w(size_t& cur, Weight& w, size_t Np, size_t Kp, size_t nb = 0) {
  w.Np = (int)Np; w.Kp = (int)Kp;
  w.w = take(cur, Np * Kp);
  if (nb) w.b = take(cur, nb);
}

// a derived section -- the planes of format f of `dst`, R rows -- carved and entered into the plane table in one go, so its size and its content cannot
// disagree: filled from the first `rows` rows of dst's own fp32 matrix (src == nullptr), or its K range from k0 from another weight's
void plane(tepose_model* m, size_t& cur, Owner owner, Weight& dst, int rows, size_t R, Fmt f, const Weight* src = nullptr, int k0 = 0) {
  if (f == Fmt::scaled) { dst.s = take(cur, R * dst.Kp); dst.Rs = (int)R; }
  else if (k0 == 0) { dst.p = take(cur, R * dst.Kp); dst.Rp = (int)R; }      // (a further K range of the section carved with k0 = 0)
  m->planes.push_back(PlaneSpec{owner, src ? src : &dst, rows, &dst, k0, f});
}

void layout_tail(tepose_model* m, size_t cur) {   // regressor + SMPL sections, shared by both kinds
  take_w(cur, m->w1a, 1024, kFeat, 1024);
  take_w(cur, m->w1b, 1024, kState);
  take_w(cur, m->w2, 1024, 1024, 1024);
  take_w(cur, m->wdec, 256, 1024, kState);
  m->init = take(cur, kState);
  m->smpl.J0 = take(cur, 72);
  m->smpl.JS = take(cur, 720);
  take_w(cur, m->blend, kBlendN, kBlendK);
  m->smpl.lbsW = take(cur, (size_t)kNV * kNJ);
  m->smpl.lbs_cidx = take(cur, (size_t)kNV * 4);
  m->smpl.lbs_cval = take(cur, (size_t)kNV * 4);
  m->smpl.lbs_nnz = take(cur, 16);
  m->smpl.parents = take(cur, 32);
  m->smpl.depth = take(cur, 32);
  m->smpl.xr_ptr = take(cur, 16);
  m->smpl.xr_idx = take(cur, (size_t)9 * kNV);
  m->smpl.xr_val = take(cur, (size_t)9 * kNV);
  for (Weight* w : {&m->w1a, &m->w1b, &m->w2, &m->wdec}) plane(m, cur, Owner::regressor, *w, w->Np, w->Np, Fmt::blocked);
  plane(m, cur, Owner::smpl, m->blend, kBlendN, kBlendN, Fmt::blocked);
  plane(m, cur, Owner::smpl, m->blend, kBlendN, kBlendN, Fmt::scaled);
  m->blend.scale_at = take(cur, 16);
  take_w(cur, m->mf, 256, kFeat);
  plane(m, cur, Owner::collapsed_regressor, m->mf, 256, 256, Fmt::blocked);
  m->mf.b = take(cur, kState);
  if (m->kind == 0) {
    take_w(cur, m->mt, 256, (size_t)3 * m->Hp);
    plane(m, cur, Owner::collapsed_tail, m->mt, 256, 256, Fmt::blocked);
    m->mt.b = take(cur, kState);
  }
  m->blob_floats = cur;
}

}  // namespace

namespace tepose {

void layout_vibe(tepose_model* m) {
  const size_t Hp = m->Hp, L = m->L, D = m->vibe_bidir ? 2 : 1;
  size_t cur = 0;
  m->hdr = take(cur, 64);
  m->vibe.assign(L, DirW());
  for (size_t l = 0; l < L; ++l) {
    take_w(cur, m->vibe[l].ih, round_up(3 * (int)(D * Hp), 128), l == 0 ? (size_t)kFeat : D * Hp, D * 3 * Hp);
    take_w(cur, m->vibe[l].hh, D * 3 * Hp, Hp, D * 3 * Hp);
  }
  if (m->vibe_linear) take_w(cur, m->vlin, kFeat, D * Hp, kFeat);
  layout_tail(m, cur);
}

void layout_hmr(tepose_model* m) {
  size_t cur = 0;
  m->hdr = take(cur, 64);
  m->bb.assign(kHmrConvs, Weight());
  (void)hmr_walk(1, [&](const ConvStep& c) {
    take_w(cur, m->bb[c.idx], c.Np, c.Kp, c.l->cout);
    return 0;
  });
  for (Weight& w : m->bb) plane(m, cur, Owner::backbone, w, w.Np, w.Np, Fmt::blocked);
  layout_tail(m, cur);
}

void layout(tepose_model* m) {
  const size_t Hp = m->Hp, L = m->L;
  size_t cur = 0;
  m->hdr = take(cur, 64);
  take_w(cur, m->wih0, round_up(9 * (int)Hp, 128), kInputP, 9 * Hp);
  m->fwd.assign(L, DirW());
  m->rec_f.assign(L, DirW());
  m->rec_r.assign(L, DirW());
  const int H3 = 3 * (int)Hp;
  const size_t n128 = round_up(H3, 128);
  for (size_t l = 0; l < L; ++l) {
    DirW* const dirs[3] = {&m->fwd[l], &m->rec_f[l], &m->rec_r[l]};
    if (l > 0)      // layer >= 1 input width: gru_fwd Hp, the bi-GRU's directions 2 Hp
      for (DirW* d : dirs) take_w(cur, d->ih, n128, d == dirs[0] ? Hp : 2 * Hp, 3 * Hp);
    for (DirW* d : dirs) take_w(cur, d->hh, 3 * Hp, Hp, 3 * Hp);
  }
  take_w(cur, m->wlf, kFeat, Hp, kFeat);
  take_w(cur, m->wlr, kFeat, 2 * Hp, kFeat);
  // split-precision copies (hi plane then lo plane, fp16): same float count as an fp32 matrix of the plane's rows.  Blocked planes pad the rows to the
  // 128-row tile, scaled ones to 256 (projections) / 384 (recurrent products)
  plane(m, cur, Owner::encoder, m->wih0, m->wih0.Np, m->wih0.Np, Fmt::blocked);
  plane(m, cur, Owner::encoder, m->wih0, 3 * H3, round_up(3 * H3, 256), Fmt::scaled);
  m->wih0.scale_at = take(cur, 16);
  for (size_t l = 0; l < L; ++l) {
    DirW* const dirs[3] = {&m->fwd[l], &m->rec_f[l], &m->rec_r[l]};
    if (l > 0)
      for (DirW* d : dirs) plane(m, cur, Owner::encoder, d->ih, (int)n128, n128, Fmt::blocked);
    for (DirW* d : dirs) plane(m, cur, Owner::encoder, d->hh, H3, n128, Fmt::blocked);
    if (l > 0)
      for (DirW* d : dirs) plane(m, cur, Owner::encoder, d->ih, H3, round_up(H3, 256), Fmt::scaled);
    for (DirW* d : dirs) {
      plane(m, cur, Owner::encoder, d->hh, H3, round_up(H3, 384), Fmt::scaled);
      d->ih.scale_at = take(cur, 16);         // one slot per direction: [0] = W_ih scale, [1] = W_hh scale
      d->hh.scale_at = d->ih.scale_at + 1;
    }
  }
  plane(m, cur, Owner::encoder, m->wlf, kFeat, kFeat, Fmt::blocked);
  plane(m, cur, Owner::encoder, m->wlr, kFeat, kFeat, Fmt::blocked);
  // [W_lf | W_lr] side by side along K: K range [0, Hp) from linear_fwd, the rest from linear_rec
  m->wlfr.Np = kFeat; m->wlfr.Kp = H3;
  plane(m, cur, Owner::encoder, m->wlfr, kFeat, kFeat, Fmt::blocked, &m->wlf, 0);
  plane(m, cur, Owner::encoder, m->wlfr, kFeat, kFeat, Fmt::blocked, &m->wlr, (int)Hp);
  layout_tail(m, cur);
}

int pack(const float* src, long ld, int N, int K, float* dst, int Np, int Kp, int rowmap, int colmap,
         int H, int Hp, hipStream_t s) {
  PackArgs a{src, ld, N, K, dst, Np, Kp, rowmap, colmap, H, Hp};
  return (int)launch_pack(a, s);
}

}  // namespace tepose

namespace {

// The caller's [N][K] tensor (leading dimension ld) into the packed fp32 rows of a weight view -- `rows` of them (0: to the record's last row, padding rows
// zeroed too) -- and its [N] bias into the view's bias rows.  Destination and padded sizes come from the record, the source and the row / column maps from the call.
struct Packer {
  const tepose_model* m; hipStream_t s;
  int rows(const float* src, long ld, int N, int K, WView v, int rows, int rowmap, int colmap) const {
    return pack(src, ld, N, K, m->blob + v.w->w + (size_t)v.row0 * v.w->Kp, rows ? rows : v.w->Np - v.row0, v.w->Kp, rowmap, colmap, m->H, m->Hp, s);
  }
  int bias(const float* src, int N, WView v, int rows, int rowmap) const {
    return pack(src, 1, N, 1, m->blob + v.w->b + v.row0, rows, 1, rowmap, COL_PLAIN, m->H, m->Hp, s);
  }
};

// First 256 bytes of the blob: identifies the model the packed sections belong to, so that a blob that travelled
// (RCCL broadcast, copy) is only adopted by a handle of the same kind / size / library layout.
struct BlobHeader {
  uint32_t magic, abi, kind, L, H, Hp, sections;   // sections: bit 0 encoder, 1 regressor, 2 SMPL tables, 3 range flag, 4 / 5 collapsed regressor / tail, 6 HMR backbone
  uint32_t layout_floats_lo, layout_floats_hi;      // blob_floats of the layout that wrote it
};
constexpr uint32_t kBlobMagic = 0x54455031u;        // "TEP1"

// model kind as the header records it: a VIBE handle also carries its constructor flags
uint32_t header_kind(const tepose_model* m) {
  return (uint32_t)m->kind | (m->kind == 1 ? (m->vibe_bidir ? 0x100u : 0u) | (m->vibe_linear ? 0x200u : 0u) : 0u);
}

int write_header(tepose_model* m, hipStream_t s) {
  BlobHeader h{};
  h.magic = kBlobMagic; h.abi = TEPOSE_ABI_VERSION; h.kind = header_kind(m); h.L = (uint32_t)m->L; h.H = (uint32_t)m->H;
  h.Hp = (uint32_t)m->Hp;
  h.sections = ((m->kind == 0 ? m->enc_packed : m->vibe_packed) ? 1u : 0u) | (m->reg_packed ? 2u : 0u) |
               (m->smpl_packed ? 4u : 0u) | ((m->enc_range_ok && m->reg_range_ok && m->smpl_range_ok && m->bb_range_ok) ? 0u : 8u) |
               (m->reg_collapsed ? 16u : 0u) | (m->tail_collapsed ? 32u : 0u) | (m->bb_packed ? 64u : 0u);
  h.layout_floats_lo = (uint32_t)(m->blob_floats & 0xffffffffu); h.layout_floats_hi = (uint32_t)((uint64_t)m->blob_floats >> 32);
  CK(hipMemcpyAsync(m->blob + m->hdr, &h, sizeof(h), hipMemcpyHostToDevice, s));
  CK(hipStreamSynchronize(s));                      // h is a stack object (pack time only)
  return 0;
}

// Pack-time range guard of the split-precision path: a weight of magnitude >= 2^15 (or inf) has no fp16 hi half, so a
// handle holding one runs every product on the exact-fp32 kernels instead (as TEPOSE_EXACT_FP32=1) -- never a silent inf.
// One device reduction + read-back over the section's fp32 copy; pack time only.
int range_check(tepose_model* m, size_t first, size_t end, bool* ok, hipStream_t s) {
  float* scratch = m->blob + m->hdr + 32;
  CK(launch_absmax(m->blob + first, end - first, scratch, s));
  float wmax = 0.f;
  CK(hipMemcpyAsync(&wmax, scratch, sizeof(float), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  *ok = wmax < 32768.f;
  m->split = m->split_env && m->enc_range_ok && m->reg_range_ok && m->smpl_range_ok && m->bb_range_ok;
  return 0;
}

// Fills every derived section of `owner` from the packed fp32 matrices next to it.  Blocked planes: the pad rows are zeroed, then the real rows split.
// Scaled planes: one power-of-two scale for the matrix (largest |w| * p in [2^13, 2^14)), written to its blob slot and to the handle's host copy: one
// device reduction + read-back each.
int derive_planes(tepose_model* m, Owner owner, hipStream_t s) {
  float* B = m->blob;
  for (const PlaneSpec& p : m->planes) {
    if (p.owner != owner) continue;
    const Weight& src = *p.src;
    Weight& dst = *p.dst;
    const WPlanes q = w_planes(B, WView(dst, 0, p.k0), p.fmt);
    if (p.fmt == Fmt::blocked) {
      if (p.rows < dst.Rp) CK(launch_fill(B + dst.p, (size_t)dst.Rp * dst.Kp, 0.f, s));
      CK(launch_split_planes(B + src.w, src.Kp, p.rows, src.Kp, src.Kp, dst.Rp, (void*)q.hi, (void*)q.lo, s));
      continue;
    }
    float* scale_dev = B + dst.scale_at;
    CK(launch_absmax(B + src.w, (size_t)p.rows * src.Kp, scale_dev, s));
    float wmax = 0.f;
    CK(hipMemcpyAsync(&wmax, scale_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    float sc = 1.f;
    if (wmax > 0.f && wmax < 3e38f) {
      int ex = 0;
      (void)frexpf(wmax, &ex);              // wmax = f * 2^ex, f in [0.5, 1)
      sc = ldexpf(1.f, 14 - ex);            // wmax * sc in [2^13, 2^14)
    }
    dst.scale = sc;
    CK(hipMemcpyAsync(scale_dev, &dst.scale, sizeof(float), hipMemcpyHostToDevice, s));
    CK(launch_fill(B + dst.s, (size_t)dst.Rs * dst.Kp, 0.f, s));
    CK(launch_split_planes16(B + src.w, src.Kp, p.rows, src.Kp, src.Kp, (long)dst.Rs, sc, (void*)q.hi, (void*)q.lo, s));
    CK(hipStreamSynchronize(s));            // dst.scale is read by the async copy above
  }
  return 0;
}

// The regressor's loop (spin.py:252-261) in eval mode, with s = [pose6d | shape | cam] (157 values):
//   h1 = W1a f + W1b s + b1,  h2 = W2 h1 + b2,  s' = s + Wd h2 + bd        (no activation; Dropout is the identity)
// is affine:  s' = G s + F f + c  with  P = Wd W2,  G = I + P W1b,  F = P W1a,  c = P b1 + Wd b2 + bd,  so after three
// iterations from the model's own initial state s0:  s3 = (I + G + G^2)(F f + c) + G^3 s0 = Mf f + k0.
// All products in fp64 on the device (a few hundred MFLOP, pack time only), rounded to fp32 once.
int collapse_regressor(tepose_model* m, hipStream_t s) {
  m->reg_collapsed = false;
  m->tail_collapsed = false;
  if (!m->collapse_env || !m->reg_packed) return 0;
  constexpr int S = 157;
  float* B = m->blob;
  const size_t nP = (size_t)S * 1024, nF = (size_t)S * kFeat, nG = (size_t)S * S;
  double* d = nullptr;
  CK(hipMalloc((void**)&d, (nP + 2 * nF + 4 * nG + 5 * S) * sizeof(double)));
  double *P = d, *F = P + nP, *Mf = F + nF, *G = Mf + nF, *G2 = G + nG, *G3 = G2 + nG, *Ss = G3 + nG;
  double *t1 = Ss + nG, *c = t1 + S, *t2 = c + S, *k0 = t2 + S;
  auto run = [&]() -> int {
    CK(launch_dmm(B + m->wdec.w, 0, 1024, B + m->w2.w, 0, 1024, nullptr, 0, nullptr, 0, P, 1024, S, 1024, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->w1a.w, 0, kFeat, nullptr, 0, nullptr, 0, F, kFeat, S, kFeat, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->w1b.w, 0, kState, nullptr, 0, nullptr, 0, G, S, S, S, 1024, 1.0, 1, s));
    CK(launch_dmm(B + m->wdec.w, 0, 1024, B + m->w2.b, 0, 1, nullptr, 0, nullptr, 0, t1, 1, S, 1, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->w1a.b, 0, 1, t1, 1, B + m->wdec.b, 1, c, 1, S, 1, 1024, 1.0, 0, s));
    CK(launch_dmm(G, 1, S, G, 1, S, nullptr, 0, nullptr, 0, G2, S, S, S, S, 1.0, 0, s));
    CK(launch_dmm(G2, 1, S, G, 1, S, nullptr, 0, nullptr, 0, G3, S, S, S, S, 1.0, 0, s));
    CK(launch_dmm(G, 1, S, G, 1, S, G, S, nullptr, 0, Ss, S, S, S, S, 1.0, 1, s));                    // I + G + G^2
    CK(launch_dmm(Ss, 1, S, F, 1, kFeat, nullptr, 0, nullptr, 0, Mf, kFeat, S, kFeat, S, 1.0, 0, s));
    CK(launch_dmm(G3, 1, S, B + m->init, 0, 1, nullptr, 0, nullptr, 0, t2, 1, S, 1, S, 1.0, 0, s));
    CK(launch_dmm(Ss, 1, S, c, 1, 1, t2, 1, nullptr, 0, k0, 1, S, 1, S, 1.0, 0, s));
    CK(launch_d2f_pad(Mf, kFeat, S, kFeat, B + m->mf.w, m->mf.Np, m->mf.Kp, s));
    CK(launch_d2f_pad(k0, S, 1, S, B + m->mf.b, 1, kState, s));
    CK((hipError_t)derive_planes(m, Owner::collapsed_regressor, s));
    CK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = run();
  (void)hipFree(d);
  if (rc) return rc;
  bool ok = false;                                        // the collapsed matrix must fit the fp16 planes like any weight
  CK((hipError_t)range_check(m, m->mf.w, m->mf.p, &ok, s));
  m->reg_collapsed = ok;
  return 0;
}

// ... and through the tail linears (tepose.py:81-86, eval mode: feat = (relu(h_fwd) W_lf^T + b_lf + relu(y_rec0) W_lr^T + b_lr) / 2):
//   xs = [relu(h_fwd) | relu(y_rec0)] Mt^T + kt,   Mt = Mf [W_lf | W_lr] / 2,   kt = Mf (b_lf + b_lr) / 2 + k0
int collapse_tail(tepose_model* m, hipStream_t s) {
  m->tail_collapsed = false;
  if (m->kind != 0 || !m->collapse_env || !m->reg_collapsed || !m->enc_packed) return 0;
  constexpr int S = 157;
  const int Hp = m->Hp, K3 = 3 * Hp;
  float* B = m->blob;
  double* d = nullptr;
  CK(hipMalloc((void**)&d, ((size_t)S * K3 + 2 * S) * sizeof(double)));
  double *Mt = d, *t = Mt + (size_t)S * K3, *kt = t + S;
  auto run = [&]() -> int {
    CK(launch_dmm(B + m->mf.w, 0, kFeat, B + m->wlf.w, 0, Hp, nullptr, 0, nullptr, 0, Mt, K3, S, Hp, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf.w, 0, kFeat, B + m->wlr.w, 0, 2 * Hp, nullptr, 0, nullptr, 0, Mt + Hp, K3, S, 2 * Hp, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf.w, 0, kFeat, B + m->wlf.b, 0, 1, nullptr, 0, nullptr, 0, t, 1, S, 1, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf.w, 0, kFeat, B + m->wlr.b, 0, 1, t, 1, B + m->mf.b, 1, kt, 1, S, 1, kFeat, 0.5, 0, s));
    CK(launch_d2f_pad(Mt, K3, S, K3, B + m->mt.w, m->mt.Np, m->mt.Kp, s));
    CK(launch_d2f_pad(kt, S, 1, S, B + m->mt.b, 1, kState, s));
    CK((hipError_t)derive_planes(m, Owner::collapsed_tail, s));
    CK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = run();
  (void)hipFree(d);
  if (rc) return rc;
  bool ok = false;
  CK((hipError_t)range_check(m, m->mt.w, m->mt.p, &ok, s));
  m->tail_collapsed = ok;
  return 0;
}
}  // namespace

extern "C" {

size_t tepose_packed_bytes(const tepose_model* m) { return m ? m->blob_floats * sizeof(float) : 0; }

int tepose_set_blob(tepose_model* m, void* blob, size_t bytes) {
  if (!m || !blob) return TEPOSE_E_ARG;
  if (bytes < m->blob_floats * sizeof(float)) return TEPOSE_E_WORKSPACE;
  m->blob = (float*)blob;
  h3s16c_warm();                                 // the blob's device is current (callers run under it): its debug counter of the barrier-free kernels
  if (!m->fault) {                               // first blob = first moment a device is certain to exist
    unsigned* f = nullptr;
    if (hipHostMalloc((void**)&f, 64, hipHostMallocDefault) == hipSuccess && f) { *f = 0u; m->fault = f; }
    else (void)hipGetLastError();                // no fault word: the persistent kernels are not used (uses_persistent)
  }
  return 0;
}

int tepose_adopt_blob(tepose_model* m) {
  if (!m) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  BlobHeader h{};
  CK(hipMemcpy(&h, m->blob + m->hdr, sizeof(h), hipMemcpyDeviceToHost));                      // set-up time only
  const uint64_t lf = ((uint64_t)h.layout_floats_hi << 32) | h.layout_floats_lo;
  if (h.magic != kBlobMagic || h.abi != TEPOSE_ABI_VERSION || h.kind != header_kind(m) || (int)h.L != m->L ||
      (int)h.H != m->H || (int)h.Hp != m->Hp || lf != (uint64_t)m->blob_floats)
    return TEPOSE_E_STATE;                        // not a blob of this model kind / size / library layout
  m->enc_packed = m->kind == 0 && (h.sections & 1u);
  m->vibe_packed = m->kind == 1 && (h.sections & 1u);
  m->reg_packed = (h.sections & 2u) != 0;
  m->smpl_packed = (h.sections & 4u) != 0;
  m->bb_packed = m->kind == 2 && (h.sections & 64u) != 0;
  m->enc_range_ok = m->reg_range_ok = m->smpl_range_ok = m->bb_range_ok = !(h.sections & 8u);   // bit 3: a weight outside the fp16 range
  m->reg_collapsed = m->collapse_env && (h.sections & 16u) != 0;      // (a handle created with TEPOSE_COLLAPSE_REGRESSOR=0 keeps the loop)
  m->tail_collapsed = m->collapse_env && m->kind == 0 && (h.sections & 32u) != 0;
  m->split = m->split_env && m->enc_range_ok;
  m->maxdepth = kNJ - 1;   // upper bound; chain levels past the real depth are no-ops
  int max_nnz = kNJ;
  CK(hipMemcpy(&max_nnz, m->blob + m->smpl.lbs_nnz, sizeof(int), hipMemcpyDeviceToHost));   // set-up time only
  m->lbs_sparse = max_nnz <= 4 ? 1 : 0;
  for (const PlaneSpec& p : m->planes) {        // the host copies of the plane scales
    if (p.fmt != Fmt::scaled || (p.owner == Owner::encoder && !m->enc_packed)) continue;
    CK(hipMemcpy(&p.dst->scale, m->blob + p.dst->scale_at, sizeof(float), hipMemcpyDeviceToHost));
    if (!(p.dst->scale > 0.f)) p.dst->scale = 1.f;
  }
  return 0;
}

// ---- broadcast less (round 3): every hi / lo plane in the blob is a function of the fp32 sections next to it --------------
// The blob interleaves source-of-truth fp32 sections (packed matrices, biases, SMPL tables, the fp64-derived collapsed maps
// rounded to fp32, the header) with the plane copies the split-precision kernels read.  tepose_fp32_ranges lists the former as
// byte ranges; a rank that received only those (276 of 770 MB at L = 2 / H = 1024) rebuilds the rest with tepose_derive_planes,
// which also does what tepose_adopt_blob does.  The planes come out bit-identical to the packing rank's
// (tests/test_gpu_multirank.py::test_planes_derived_from_the_fp32_sections_are_bit_identical).
int tepose_fp32_ranges(const tepose_model* m, size_t* offsets, size_t* sizes, int cap) {
  if (!m || !offsets || !sizes) return TEPOSE_E_ARG;
  // what is derived: every plane section and every scale slot of the table, each up to the 256-byte end of its section; the rest is the answer
  std::vector<std::pair<size_t, size_t>> derived, r;
  for (const PlaneSpec& p : m->planes) {
    const Weight& w = *p.dst;
    if (p.fmt == Fmt::blocked) derived.emplace_back(w.p, align_up(w.p + (size_t)w.Rp * w.Kp, kAlignF));
    else {
      derived.emplace_back(w.s, align_up(w.s + (size_t)w.Rs * w.Kp, kAlignF));
      derived.emplace_back(w.scale_at / kAlignF * kAlignF, w.scale_at / kAlignF * kAlignF + kAlignF);      // (a slot may hold two scales)
    }
  }
  derived.emplace_back(m->blob_floats, m->blob_floats);
  std::sort(derived.begin(), derived.end());
  size_t at = 0;
  for (const auto& d : derived) {
    if (d.first > at) r.emplace_back(at, d.first);
    at = std::max(at, d.second);
  }
  if ((int)r.size() > cap) return TEPOSE_E_ARG;
  for (size_t i = 0; i < r.size(); ++i) { offsets[i] = r[i].first * sizeof(float); sizes[i] = (r[i].second - r[i].first) * sizeof(float); }
  return (int)r.size();
}

int tepose_derive_planes(tepose_model* m, void* stream) {
  if (!m) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  int rc = tepose_adopt_blob(m);                 // header check, packed / range / collapse flags
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool enc = m->kind == 0 && m->enc_packed;
  const std::pair<Owner, bool> owners[] = {{Owner::encoder, enc}, {Owner::collapsed_tail, enc && m->tail_collapsed}, {Owner::regressor, m->reg_packed},
                                           {Owner::collapsed_regressor, m->reg_packed && m->reg_collapsed}, {Owner::smpl, m->smpl_packed},
                                           {Owner::backbone, m->bb_packed}};
  for (const auto& o : owners)
    if (o.second) CK((hipError_t)derive_planes(m, o.first, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

int tepose_pack_vibe_encoder(tepose_model* m, const float* const* w, int n_w, void* stream) {
  if (!m || !w || m->kind != 1) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  const int L = m->L, H = m->H, Hp = m->Hp, D = m->vibe_bidir ? 2 : 1;
  if (n_w != 4 * L * D + (m->vibe_linear ? 2 : 0)) return TEPOSE_E_ARG;
  for (int i = 0; i < n_w; ++i)
    if (!w[i]) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const Packer pk{m, s};
  const int cmap = D == 2 ? COL_SPLIT2 : COL_PLAIN;            // layer >= 1 inputs and the linear read [fwd Hp | bwd Hp]
  for (int l = 0; l < L; ++l) {
    const int K = l == 0 ? kFeat : D * H;
    for (int d = 0; d < D; ++d) {
      const float* const* q = w + 4 * (l * D + d);              // weight_ih, weight_hh, bias_ih, bias_hh (nn.GRU's order)
      const WView ih(m->vibe[l].ih, d * 3 * Hp), hh(m->vibe[l].hh, d * 3 * Hp);
      // (the last direction also zeroes the padding rows)
      CK((hipError_t)pk.rows(q[0], K, 3 * H, K, ih, d == D - 1 ? 0 : 3 * Hp, ROW_GATES, l == 0 ? COL_PLAIN : cmap));
      CK((hipError_t)pk.bias(q[2], 3 * H, ih, 3 * Hp, ROW_GATES));
      CK((hipError_t)pk.rows(q[1], H, 3 * H, H, hh, 3 * Hp, ROW_GATES_TILED, COL_PLAIN));
      CK((hipError_t)pk.bias(q[3], 3 * H, hh, 3 * Hp, ROW_GATES));
    }
  }
  if (m->vibe_linear) {
    CK((hipError_t)pk.rows(w[4 * L * D], D * H, kFeat, D * H, m->vlin, 0, ROW_PLAIN, cmap));
    CK((hipError_t)pk.bias(w[4 * L * D + 1], kFeat, m->vlin, kFeat, ROW_PLAIN));
  }
  m->vibe_packed = true;
  CK((hipError_t)range_check(m, m->vibe[0].ih.w, m->w1a.w, &m->enc_range_ok, s));
  return write_header(m, s);
}

int tepose_pack_hmr_backbone(tepose_model* m, const float* const* w, int n_w, void* stream) {
  if (!m || !w || m->kind != 2 || n_w != 5 * kHmrConvs) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  for (int i = 0; i < n_w; ++i)
    if (!w[i]) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* B = m->blob;
  int* err = (int*)(B + m->hdr + 48);            // a word of the header section past the BlobHeader and range_check's scratch
  m->bb_packed = false;
  CK(hipMemsetAsync(err, 0, sizeof(int), s));
  int rc = hmr_walk(1, [&](const ConvStep& c) {
    const float* const* q = w + 5 * c.idx;       // weight, bn.weight, bn.bias, bn.running_mean, bn.running_var
    const Weight& bw = m->bb[c.idx];
    return (int)launch_hmr_fold_pack(q[0], q[1], q[2], q[3], q[4], c.l->cout, c.l->cin, c.l->R, B + bw.w, bw.Np, bw.Kp, B + bw.b, err, s);
  });
  if (rc) return rc;
  int bad = 0;
  CK(hipMemcpyAsync(&bad, err, sizeof(int), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));                   // pack time only
  if (bad) return TEPOSE_E_ARG;                  // running_var + eps <= 0, or a non-finite folded weight / shift
  CK((hipError_t)derive_planes(m, Owner::backbone, s));
  m->bb_packed = true;
  CK((hipError_t)range_check(m, m->bb[0].w, m->bb[0].p, &m->bb_range_ok, s));
  return write_header(m, s);
}

int tepose_pack_encoder(tepose_model* m, const float* const* w, int n_w, void* stream) {
  if (!m || !w || m->kind != 0) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  const int L = m->L, H = m->H, Hp = m->Hp;
  if (n_w != 12 * L + 4) return TEPOSE_E_ARG;
  for (int i = 0; i < n_w; ++i)
    if (!w[i]) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* B = m->blob;
  const Packer pk{m, s};
  // zero the stacked layer-0 block first (rows beyond 9Hp up to the 128 multiple)
  CK(launch_fill(B + m->wih0.w, (size_t)m->wih0.Np * m->wih0.Kp, 0.f, s));
  auto fwd_w = [&](int l, int k) { return w[4 * l + k]; };                       // ih, hh, bih, bhh
  auto rec_w = [&](int l, int rev, int k) { return w[4 * L + 8 * l + 4 * rev + k]; };
  // layer 0 input projections, stacked [fwd | rec_reverse | rec]
  const float* l0[3] = {fwd_w(0, 0), rec_w(0, 1, 0), rec_w(0, 0, 0)};
  const float* l0b[3] = {fwd_w(0, 2), rec_w(0, 1, 2), rec_w(0, 0, 2)};
  for (int d = 0; d < 3; ++d) {
    const WView v(m->wih0, d * 3 * Hp);
    CK((hipError_t)pk.rows(l0[d], kInput, 3 * H, kInput, v, 3 * Hp, ROW_GATES, COL_PLAIN));
    CK((hipError_t)pk.bias(l0b[d], 3 * H, v, 3 * Hp, ROW_GATES));
  }
  for (int l = 0; l < L; ++l) {
    struct { DirW* d; const float *ih, *hh, *bih, *bhh; bool split; } dirs[3] = {
        {&m->fwd[l], fwd_w(l, 0), fwd_w(l, 1), fwd_w(l, 2), fwd_w(l, 3), false},
        {&m->rec_f[l], rec_w(l, 0, 0), rec_w(l, 0, 1), rec_w(l, 0, 2), rec_w(l, 0, 3), true},
        {&m->rec_r[l], rec_w(l, 1, 0), rec_w(l, 1, 1), rec_w(l, 1, 2), rec_w(l, 1, 3), true}};
    for (auto& d : dirs) {
      if (l > 0) {
        const int K = d.split ? 2 * H : H;
        CK((hipError_t)pk.rows(d.ih, K, 3 * H, K, d.d->ih, 0, ROW_GATES, d.split ? COL_SPLIT2 : COL_PLAIN));
        CK((hipError_t)pk.bias(d.bih, 3 * H, d.d->ih, 3 * Hp, ROW_GATES));
      }
      CK((hipError_t)pk.rows(d.hh, H, 3 * H, H, d.d->hh, 0, ROW_GATES_TILED, COL_PLAIN));
      CK((hipError_t)pk.bias(d.bhh, 3 * H, d.d->hh, 3 * Hp, ROW_GATES));
    }
  }
  const float* const* t = w + 12 * L;
  CK((hipError_t)pk.rows(t[0], H, kFeat, H, m->wlf, 0, ROW_PLAIN, COL_PLAIN));
  CK((hipError_t)pk.bias(t[1], kFeat, m->wlf, kFeat, ROW_PLAIN));
  CK((hipError_t)pk.rows(t[2], 2 * H, kFeat, 2 * H, m->wlr, 0, ROW_PLAIN, COL_SPLIT2));
  CK((hipError_t)pk.bias(t[3], kFeat, m->wlr, kFeat, ROW_PLAIN));
  CK((hipError_t)derive_planes(m, Owner::encoder, s));
  m->enc_packed = true;
  CK((hipError_t)range_check(m, m->wih0.w, m->wih0.p, &m->enc_range_ok, s));
  CK((hipError_t)collapse_tail(m, s));
  return write_header(m, s);
}

int tepose_pack_regressor(tepose_model* m, const float* const* w, int n_w, void* stream) {
  if (!m || !w || n_w != 13) return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  for (int i = 0; i < n_w; ++i)
    if (!w[i]) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* B = m->blob;
  const Packer pk{m, s};
  const int ld1 = kFeat + kNPose + 13;   // 2205
  CK((hipError_t)pk.rows(w[0], ld1, 1024, kFeat, m->w1a, 0, ROW_PLAIN, COL_PLAIN));
  CK((hipError_t)pk.bias(w[1], 1024, m->w1a, 1024, ROW_PLAIN));
  CK((hipError_t)pk.rows(w[0] + kFeat, ld1, 1024, 157, m->w1b, 0, ROW_PLAIN, COL_PLAIN));
  CK((hipError_t)pk.rows(w[2], 1024, 1024, 1024, m->w2, 0, ROW_PLAIN, COL_PLAIN));
  CK((hipError_t)pk.bias(w[3], 1024, m->w2, 1024, ROW_PLAIN));
  // decoders stacked: rows 0..143 decpose, 144..153 decshape, 154..156 deccam, rest zero
  CK(launch_fill(B + m->wdec.w, (size_t)m->wdec.Np * m->wdec.Kp, 0.f, s));
  CK(launch_fill(B + m->wdec.b, kState, 0.f, s));
  CK(launch_fill(B + m->init, kState, 0.f, s));
  const int rows[3] = {kNPose, 10, 3}, off[3] = {0, kNPose, kNPose + 10};
  for (int i = 0; i < 3; ++i) {
    const WView v(m->wdec, off[i]);
    CK((hipError_t)pk.rows(w[4 + 2 * i], 1024, rows[i], 1024, v, rows[i], ROW_PLAIN, COL_PLAIN));
    CK((hipError_t)pk.bias(w[5 + 2 * i], rows[i], v, rows[i], ROW_PLAIN));
    CK((hipError_t)pack(w[10 + i], 1, rows[i], 1, B + m->init + off[i], rows[i], 1, 0, 0, 0, 1, s));
  }
  CK((hipError_t)derive_planes(m, Owner::regressor, s));
  m->reg_packed = true;
  CK((hipError_t)range_check(m, m->w1a.w, m->smpl.J0, &m->reg_range_ok, s));
  CK((hipError_t)collapse_regressor(m, s));
  CK((hipError_t)collapse_tail(m, s));
  return write_header(m, s);
}

int tepose_pack_smpl(tepose_model* m, const float* v_template, const float* shapedirs,
                     const float* posedirs, const float* J_regressor, const float* lbs_weights,
                     const float* J_regressor_extra, const int32_t* parents_host, void* stream) {
  if (!m || !v_template || !shapedirs || !posedirs || !J_regressor || !lbs_weights ||
      !J_regressor_extra || !parents_host)
    return TEPOSE_E_ARG;
  if (!m->blob) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  float* B = m->blob;
  int par[kNJ], dep[kNJ];
  for (int j = 0; j < kNJ; ++j) {
    par[j] = j == 0 ? -1 : parents_host[j];
    if (j > 0 && (par[j] < 0 || par[j] >= j)) return TEPOSE_E_ARG;   // parents must precede children
  }
  const int maxd = chain_depths(par, dep);      // shapes.h: the levels both chain kernels walk
  m->maxdepth = maxd;
  CK(hipMemcpyAsync(B + m->smpl.parents, par, sizeof(par), hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(B + m->smpl.depth, dep, sizeof(dep), hipMemcpyHostToDevice, s));
  CK(hipStreamSynchronize(s));   // par/dep are stack arrays (pack time only, never on the forward path)
  CK(launch_smpl_consts(v_template, shapedirs, posedirs, J_regressor, B + m->smpl.J0, B + m->smpl.JS,
                        B + m->blend.w, s));
  CK((hipError_t)pack(lbs_weights, kNJ, kNV, kNJ, B + m->smpl.lbsW, kNV, kNJ, 0, 0, 0, 1, s));
  CK(launch_lbs_compact(lbs_weights, (int*)(B + m->smpl.lbs_cidx), B + m->smpl.lbs_cval, (int*)(B + m->smpl.lbs_nnz), s));
  int max_nnz = 0;
  CK(hipMemcpyAsync(&max_nnz, B + m->smpl.lbs_nnz, sizeof(int), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));                 // pack time only
  m->lbs_sparse = max_nnz <= 4 ? 1 : 0;
  CK(launch_csr_build(J_regressor_extra, 9, kNV, (int*)(B + m->smpl.xr_ptr), (int*)(B + m->smpl.xr_idx),
                      B + m->smpl.xr_val, 9 * kNV, s));
  CK((hipError_t)derive_planes(m, Owner::smpl, s));
  m->smpl_packed = true;
  CK((hipError_t)range_check(m, m->smpl.J0, m->smpl.lbs_cidx, &m->smpl_range_ok, s));
  return write_header(m, s);
}

size_t tepose_jreg_packed_bytes(void) { return (32 + (size_t)17 * kNV * 2) * 4; }

int tepose_pack_jreg(const float* J, void* packed, void* stream) {
  if (!J || !packed) return TEPOSE_E_ARG;
  int* p = (int*)packed;
  CK(launch_csr_build(J, 17, kNV, p, p + 32, (float*)(p + 32 + 17 * kNV), 17 * kNV, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
