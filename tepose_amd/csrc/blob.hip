// The packed blob: where every section lives (layout pass), how the caller's tensors get there (tepose_pack_*), and the derived sections -- the hi | lo
// fp16 planes the split-precision kernels read -- which one table describes and one function writes.  Nothing else does offset arithmetic on the blob.
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

// a derived section: carved and entered into the plane table in one go, so its size and its content cannot disagree
size_t plane(tepose_model* m, size_t& cur, Owner owner, size_t src, int rows, int Kp, int R, const size_t* scale_slot = nullptr, int scale_i = 0,
             float* scale_host = nullptr) {
  const size_t dst = take(cur, (size_t)R * Kp);
  m->planes.push_back(PlaneSpec{owner, src, rows, Kp, dst, R, Kp, 0, scale_slot, scale_i, scale_host});
  return dst;
}

void layout_tail(tepose_model* m, size_t cur) {   // regressor + SMPL sections, shared by both kinds
  m->w1a = take(cur, 1024 * (size_t)kFeat);
  m->b1 = take(cur, 1024);
  m->w1b = take(cur, 1024 * (size_t)kState);
  m->w2 = take(cur, 1024 * 1024);
  m->b2 = take(cur, 1024);
  m->wdec = take(cur, 256 * 1024);
  m->bdec = take(cur, kState);
  m->init = take(cur, kState);
  m->smpl.J0 = take(cur, 72);
  m->smpl.JS = take(cur, 720);
  m->smpl.blendW = take(cur, (size_t)kBlendN * kBlendK);
  m->smpl.lbsW = take(cur, (size_t)kNV * kNJ);
  m->smpl.lbs_cidx = take(cur, (size_t)kNV * 4);
  m->smpl.lbs_cval = take(cur, (size_t)kNV * 4);
  m->smpl.lbs_nnz = take(cur, 16);
  m->smpl.parents = take(cur, 32);
  m->smpl.depth = take(cur, 32);
  m->smpl.xr_ptr = take(cur, 16);
  m->smpl.xr_idx = take(cur, (size_t)9 * kNV);
  m->smpl.xr_val = take(cur, (size_t)9 * kNV);
  m->w1a_p = plane(m, cur, Owner::regressor, m->w1a, 1024, kFeat, 1024);
  m->w1b_p = plane(m, cur, Owner::regressor, m->w1b, 1024, kState, 1024);
  m->w2_p = plane(m, cur, Owner::regressor, m->w2, 1024, 1024, 1024);
  m->wdec_p = plane(m, cur, Owner::regressor, m->wdec, 256, 1024, 256);
  m->blendW_p = plane(m, cur, Owner::smpl, m->smpl.blendW, kBlendN, kBlendK, kBlendN);
  m->blendW_s = plane(m, cur, Owner::smpl, m->smpl.blendW, kBlendN, kBlendK, kBlendN, &m->blend_scale, 0, &m->blend_sc);
  m->blend_scale = take(cur, 16);
  m->mf = take(cur, 256 * (size_t)kFeat);
  m->mf_p = plane(m, cur, Owner::collapsed_regressor, m->mf, 256, kFeat, 256);
  m->k0 = take(cur, kState);
  if (m->kind == 0) {
    m->mt = take(cur, 256 * (size_t)3 * m->Hp);
    m->mt_p = plane(m, cur, Owner::collapsed_tail, m->mt, 256, 3 * m->Hp, 256);
    m->kt = take(cur, kState);
  }
  m->blob_floats = cur;
}

}  // namespace

namespace tepose {

void layout_vibe(tepose_model* m) {
  const size_t Hp = m->Hp, L = m->L, D = m->vibe_bidir ? 2 : 1;
  size_t cur = 0;
  m->hdr = take(cur, 64);
  const size_t n128 = round_up(3 * (int)(D * Hp), 128);
  m->vibe.assign(L, DirW());
  for (size_t l = 0; l < L; ++l) {
    m->vibe[l].wih = take(cur, n128 * (l == 0 ? (size_t)kFeat : D * Hp));
    m->vibe[l].bih = take(cur, D * 3 * Hp);
    m->vibe[l].whh = take(cur, D * 3 * Hp * Hp);
    m->vibe[l].bhh = take(cur, D * 3 * Hp);
  }
  if (m->vibe_linear) {
    m->vlin_w = take(cur, (size_t)kFeat * D * Hp);
    m->vlin_b = take(cur, kFeat);
  }
  layout_tail(m, cur);
}

void layout_hmr(tepose_model* m) {
  size_t cur = 0;
  m->hdr = take(cur, 64);
  m->bb_w.assign(kHmrConvs, 0);
  m->bb_b.assign(kHmrConvs, 0);
  m->bb_p.assign(kHmrConvs, 0);
  (void)hmr_walk(1, [&](const ConvStep& c) {
    m->bb_w[c.idx] = take(cur, (size_t)c.Np * c.Kp);
    m->bb_b[c.idx] = take(cur, c.l->cout);
    return 0;
  });
  (void)hmr_walk(1, [&](const ConvStep& c) {
    m->bb_p[c.idx] = plane(m, cur, Owner::backbone, m->bb_w[c.idx], c.Np, c.Kp, c.Np);
    return 0;
  });
  layout_tail(m, cur);
}

void layout(tepose_model* m) {
  const size_t Hp = m->Hp, L = m->L;
  size_t cur = 0;
  m->hdr = take(cur, 64);
  m->wih0 = take(cur, (size_t)round_up(9 * (int)Hp, 128) * kInputP);
  m->bih0 = take(cur, 9 * Hp);
  m->fwd.assign(L, DirW());
  m->rec_f.assign(L, DirW());
  m->rec_r.assign(L, DirW());
  for (size_t l = 0; l < L; ++l) {
    const size_t n128 = round_up(3 * (int)Hp, 128);
    if (l > 0) {
      m->fwd[l].wih = take(cur, n128 * Hp);
      m->fwd[l].bih = take(cur, 3 * Hp);
      m->rec_f[l].wih = take(cur, n128 * 2 * Hp);
      m->rec_f[l].bih = take(cur, 3 * Hp);
      m->rec_r[l].wih = take(cur, n128 * 2 * Hp);
      m->rec_r[l].bih = take(cur, 3 * Hp);
    }
    for (DirW* d : {&m->fwd[l], &m->rec_f[l], &m->rec_r[l]}) {
      d->whh = take(cur, 3 * Hp * Hp);
      d->bhh = take(cur, 3 * Hp);
    }
  }
  m->wlf = take(cur, (size_t)kFeat * Hp);
  m->blf = take(cur, kFeat);
  m->wlr = take(cur, (size_t)kFeat * 2 * Hp);
  m->blr = take(cur, kFeat);
  // split-precision copies (hi plane then lo plane, fp16): same float count as an fp32 matrix of the plane's rows
  const int H3 = 3 * (int)Hp, n128 = round_up(H3, 128), r256 = round_up(H3, 256), r384 = round_up(H3, 384), rows0 = round_up(3 * H3, 128);
  m->wih0_p = plane(m, cur, Owner::encoder, m->wih0, rows0, kInputP, rows0);
  m->wih0_s = plane(m, cur, Owner::encoder, m->wih0, 3 * H3, kInputP, round_up(3 * H3, 256), &m->wih0_scale, 0, &m->w0_scale);
  m->wih0_scale = take(cur, 16);
  for (size_t l = 0; l < L; ++l) {
    DirW* const dirs[3] = {&m->fwd[l], &m->rec_f[l], &m->rec_r[l]};
    auto Kin = [&](const DirW* d) { return (int)(d == dirs[0] ? Hp : 2 * Hp); };      // layer >= 1 input width: gru_fwd Hp, the bi-GRU's directions 2 Hp
    if (l > 0)
      for (DirW* d : dirs) d->wih_p = plane(m, cur, Owner::encoder, d->wih, n128, Kin(d), n128);
    for (DirW* d : dirs) d->whh_p = plane(m, cur, Owner::encoder, d->whh, H3, (int)Hp, n128);
    if (l > 0)
      for (DirW* d : dirs) d->wih_s = plane(m, cur, Owner::encoder, d->wih, H3, Kin(d), r256, &d->scales, 0, &d->wih_scale);
    for (DirW* d : dirs) {
      d->whh_s = plane(m, cur, Owner::encoder, d->whh, H3, (int)Hp, r384, &d->scales, 1, &d->whh_scale);
      d->scales = take(cur, 16);
    }
  }
  m->wlf_p = plane(m, cur, Owner::encoder, m->wlf, kFeat, (int)Hp, kFeat);
  m->wlr_p = plane(m, cur, Owner::encoder, m->wlr, kFeat, 2 * (int)Hp, kFeat);
  // [W_lf | W_lr] side by side along K: K range [0, Hp) from linear_fwd, the rest from linear_rec
  m->wlfr_p = take(cur, (size_t)kFeat * H3);
  m->planes.push_back(PlaneSpec{Owner::encoder, m->wlf, kFeat, (int)Hp, m->wlfr_p, kFeat, H3, 0});
  m->planes.push_back(PlaneSpec{Owner::encoder, m->wlr, kFeat, 2 * (int)Hp, m->wlfr_p, kFeat, H3, (int)Hp});
  layout_tail(m, cur);
}

int pack(const float* src, long ld, int N, int K, float* dst, int Np, int Kp, int rowmap, int colmap,
         int H, int Hp, hipStream_t s) {
  PackArgs a{src, ld, N, K, dst, Np, Kp, rowmap, colmap, H, Hp};
  return (int)launch_pack(a, s);
}

}  // namespace tepose

namespace {

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
    half_t* hi = (half_t*)(B + p.dst);
    half_t* lo = hi + (size_t)p.R * p.Kd;
    if (!p.scale_slot) {
      if (p.rows < p.R) CK(launch_fill(B + p.dst, (size_t)p.R * p.Kd, 0.f, s));
      CK(launch_split_planes(B + p.src, p.Kp, p.rows, p.Kp, p.Kp, p.R, hi + (size_t)p.k0 * p.R, lo + (size_t)p.k0 * p.R, s));
      continue;
    }
    float* scale_dev = B + *p.scale_slot + p.scale_i;
    CK(launch_absmax(B + p.src, (size_t)p.rows * p.Kp, scale_dev, s));
    float wmax = 0.f;
    CK(hipMemcpyAsync(&wmax, scale_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    float sc = 1.f;
    if (wmax > 0.f && wmax < 3e38f) {
      int ex = 0;
      (void)frexpf(wmax, &ex);              // wmax = f * 2^ex, f in [0.5, 1)
      sc = ldexpf(1.f, 14 - ex);            // wmax * sc in [2^13, 2^14)
    }
    *p.scale_host = sc;
    CK(hipMemcpyAsync(scale_dev, p.scale_host, sizeof(float), hipMemcpyHostToDevice, s));
    CK(launch_fill(B + p.dst, (size_t)p.R * p.Kp, 0.f, s));
    CK(launch_split_planes16(B + p.src, p.Kp, p.rows, p.Kp, p.Kp, (long)p.R, sc, hi, lo, s));
    CK(hipStreamSynchronize(s));            // *scale_host is read by the async copy above
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
    CK(launch_dmm(B + m->wdec, 0, 1024, B + m->w2, 0, 1024, nullptr, 0, nullptr, 0, P, 1024, S, 1024, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->w1a, 0, kFeat, nullptr, 0, nullptr, 0, F, kFeat, S, kFeat, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->w1b, 0, kState, nullptr, 0, nullptr, 0, G, S, S, S, 1024, 1.0, 1, s));
    CK(launch_dmm(B + m->wdec, 0, 1024, B + m->b2, 0, 1, nullptr, 0, nullptr, 0, t1, 1, S, 1, 1024, 1.0, 0, s));
    CK(launch_dmm(P, 1, 1024, B + m->b1, 0, 1, t1, 1, B + m->bdec, 1, c, 1, S, 1, 1024, 1.0, 0, s));
    CK(launch_dmm(G, 1, S, G, 1, S, nullptr, 0, nullptr, 0, G2, S, S, S, S, 1.0, 0, s));
    CK(launch_dmm(G2, 1, S, G, 1, S, nullptr, 0, nullptr, 0, G3, S, S, S, S, 1.0, 0, s));
    CK(launch_dmm(G, 1, S, G, 1, S, G, S, nullptr, 0, Ss, S, S, S, S, 1.0, 1, s));                    // I + G + G^2
    CK(launch_dmm(Ss, 1, S, F, 1, kFeat, nullptr, 0, nullptr, 0, Mf, kFeat, S, kFeat, S, 1.0, 0, s));
    CK(launch_dmm(G3, 1, S, B + m->init, 0, 1, nullptr, 0, nullptr, 0, t2, 1, S, 1, S, 1.0, 0, s));
    CK(launch_dmm(Ss, 1, S, c, 1, 1, t2, 1, nullptr, 0, k0, 1, S, 1, S, 1.0, 0, s));
    CK(launch_d2f_pad(Mf, kFeat, S, kFeat, B + m->mf, 256, kFeat, s));
    CK(launch_d2f_pad(k0, S, 1, S, B + m->k0, 1, kState, s));
    CK((hipError_t)derive_planes(m, Owner::collapsed_regressor, s));
    CK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = run();
  (void)hipFree(d);
  if (rc) return rc;
  bool ok = false;                                        // the collapsed matrix must fit the fp16 planes like any weight
  CK((hipError_t)range_check(m, m->mf, m->mf_p, &ok, s));
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
    CK(launch_dmm(B + m->mf, 0, kFeat, B + m->wlf, 0, Hp, nullptr, 0, nullptr, 0, Mt, K3, S, Hp, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf, 0, kFeat, B + m->wlr, 0, 2 * Hp, nullptr, 0, nullptr, 0, Mt + Hp, K3, S, 2 * Hp, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf, 0, kFeat, B + m->blf, 0, 1, nullptr, 0, nullptr, 0, t, 1, S, 1, kFeat, 0.5, 0, s));
    CK(launch_dmm(B + m->mf, 0, kFeat, B + m->blr, 0, 1, t, 1, B + m->k0, 1, kt, 1, S, 1, kFeat, 0.5, 0, s));
    CK(launch_d2f_pad(Mt, K3, S, K3, B + m->mt, 256, K3, s));
    CK(launch_d2f_pad(kt, S, 1, S, B + m->kt, 1, kState, s));
    CK((hipError_t)derive_planes(m, Owner::collapsed_tail, s));
    CK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = run();
  (void)hipFree(d);
  if (rc) return rc;
  bool ok = false;
  CK((hipError_t)range_check(m, m->mt, m->mt_p, &ok, s));
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
    if (!p.scale_slot || (p.owner == Owner::encoder && !m->enc_packed)) continue;
    CK(hipMemcpy(p.scale_host, m->blob + *p.scale_slot + p.scale_i, sizeof(float), hipMemcpyDeviceToHost));
    if (!(*p.scale_host > 0.f)) *p.scale_host = 1.f;
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
    derived.emplace_back(p.dst, align_up(p.dst + (size_t)p.R * p.Kd, kAlignF));
    if (p.scale_slot) derived.emplace_back(*p.scale_slot, *p.scale_slot + kAlignF);
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
  float* B = m->blob;
  const int n128 = round_up(3 * D * Hp, 128);
  const int cmap = D == 2 ? COL_SPLIT2 : COL_PLAIN;            // layer >= 1 inputs and the linear read [fwd Hp | bwd Hp]
  for (int l = 0; l < L; ++l) {
    const int K = l == 0 ? kFeat : D * H, Kp = l == 0 ? kFeat : D * Hp;
    for (int d = 0; d < D; ++d) {
      const float* const* q = w + 4 * (l * D + d);              // weight_ih, weight_hh, bias_ih, bias_hh (nn.GRU's order)
      const int rows = d == D - 1 ? n128 - d * 3 * Hp : 3 * Hp; // the last direction also zeroes the padding rows
      CK((hipError_t)pack(q[0], K, 3 * H, K, B + m->vibe[l].wih + (size_t)d * 3 * Hp * Kp, rows, Kp, ROW_GATES,
                          l == 0 ? COL_PLAIN : cmap, H, Hp, s));
      CK((hipError_t)pack(q[2], 1, 3 * H, 1, B + m->vibe[l].bih + (size_t)d * 3 * Hp, 3 * Hp, 1, ROW_GATES, COL_PLAIN, H, Hp, s));
      CK((hipError_t)pack(q[1], H, 3 * H, H, B + m->vibe[l].whh + (size_t)d * 3 * Hp * Hp, 3 * Hp, Hp, ROW_GATES_TILED,
                          COL_PLAIN, H, Hp, s));
      CK((hipError_t)pack(q[3], 1, 3 * H, 1, B + m->vibe[l].bhh + (size_t)d * 3 * Hp, 3 * Hp, 1, ROW_GATES, COL_PLAIN, H, Hp, s));
    }
  }
  if (m->vibe_linear) {
    CK((hipError_t)pack(w[4 * L * D], D * H, kFeat, D * H, B + m->vlin_w, kFeat, D * Hp, ROW_PLAIN, cmap, H, Hp, s));
    CK((hipError_t)pack(w[4 * L * D + 1], 1, kFeat, 1, B + m->vlin_b, kFeat, 1, ROW_PLAIN, COL_PLAIN, H, Hp, s));
  }
  m->vibe_packed = true;
  CK((hipError_t)range_check(m, m->vibe[0].wih, m->w1a, &m->enc_range_ok, s));
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
    return (int)launch_hmr_fold_pack(q[0], q[1], q[2], q[3], q[4], c.l->cout, c.l->cin, c.l->R, B + m->bb_w[c.idx], c.Np, c.Kp, B + m->bb_b[c.idx], err, s);
  });
  if (rc) return rc;
  int bad = 0;
  CK(hipMemcpyAsync(&bad, err, sizeof(int), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));                   // pack time only
  if (bad) return TEPOSE_E_ARG;                  // running_var + eps <= 0, or a non-finite folded weight / shift
  CK((hipError_t)derive_planes(m, Owner::backbone, s));
  m->bb_packed = true;
  CK((hipError_t)range_check(m, m->bb_w[0], m->bb_p[0], &m->bb_range_ok, s));
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
  // zero the stacked layer-0 block first (rows beyond 9Hp up to the 128 multiple)
  CK(launch_fill(B + m->wih0, (size_t)round_up(9 * Hp, 128) * kInputP, 0.f, s));
  auto fwd_w = [&](int l, int k) { return w[4 * l + k]; };                       // ih, hh, bih, bhh
  auto rec_w = [&](int l, int rev, int k) { return w[4 * L + 8 * l + 4 * rev + k]; };
  const int n128 = round_up(3 * Hp, 128);
  // layer 0 input projections, stacked [fwd | rec_reverse | rec]
  const float* l0[3] = {fwd_w(0, 0), rec_w(0, 1, 0), rec_w(0, 0, 0)};
  const float* l0b[3] = {fwd_w(0, 2), rec_w(0, 1, 2), rec_w(0, 0, 2)};
  for (int d = 0; d < 3; ++d) {
    CK((hipError_t)pack(l0[d], kInput, 3 * H, kInput, B + m->wih0 + (size_t)d * 3 * Hp * kInputP, 3 * Hp,
                        kInputP, ROW_GATES, COL_PLAIN, H, Hp, s));
    CK((hipError_t)pack(l0b[d], 1, 3 * H, 1, B + m->bih0 + (size_t)d * 3 * Hp, 3 * Hp, 1, ROW_GATES,
                        COL_PLAIN, H, Hp, s));
  }
  for (int l = 0; l < L; ++l) {
    struct { DirW* d; const float *ih, *hh, *bih, *bhh; bool split; } dirs[3] = {
        {&m->fwd[l], fwd_w(l, 0), fwd_w(l, 1), fwd_w(l, 2), fwd_w(l, 3), false},
        {&m->rec_f[l], rec_w(l, 0, 0), rec_w(l, 0, 1), rec_w(l, 0, 2), rec_w(l, 0, 3), true},
        {&m->rec_r[l], rec_w(l, 1, 0), rec_w(l, 1, 1), rec_w(l, 1, 2), rec_w(l, 1, 3), true}};
    for (auto& d : dirs) {
      if (l > 0) {
        const int K = d.split ? 2 * H : H, Kp = d.split ? 2 * Hp : Hp;
        CK((hipError_t)pack(d.ih, K, 3 * H, K, B + d.d->wih, n128, Kp, ROW_GATES,
                            d.split ? COL_SPLIT2 : COL_PLAIN, H, Hp, s));
        CK((hipError_t)pack(d.bih, 1, 3 * H, 1, B + d.d->bih, 3 * Hp, 1, ROW_GATES, COL_PLAIN, H, Hp, s));
      }
      CK((hipError_t)pack(d.hh, H, 3 * H, H, B + d.d->whh, 3 * Hp, Hp, ROW_GATES_TILED, COL_PLAIN, H, Hp, s));
      CK((hipError_t)pack(d.bhh, 1, 3 * H, 1, B + d.d->bhh, 3 * Hp, 1, ROW_GATES, COL_PLAIN, H, Hp, s));
    }
  }
  const float* const* t = w + 12 * L;
  CK((hipError_t)pack(t[0], H, kFeat, H, B + m->wlf, kFeat, Hp, ROW_PLAIN, COL_PLAIN, H, Hp, s));
  CK((hipError_t)pack(t[1], 1, kFeat, 1, B + m->blf, kFeat, 1, ROW_PLAIN, COL_PLAIN, H, Hp, s));
  CK((hipError_t)pack(t[2], 2 * H, kFeat, 2 * H, B + m->wlr, kFeat, 2 * Hp, ROW_PLAIN, COL_SPLIT2, H, Hp, s));
  CK((hipError_t)pack(t[3], 1, kFeat, 1, B + m->blr, kFeat, 1, ROW_PLAIN, COL_PLAIN, H, Hp, s));
  CK((hipError_t)derive_planes(m, Owner::encoder, s));
  m->enc_packed = true;
  CK((hipError_t)range_check(m, m->wih0, m->wih0_p, &m->enc_range_ok, s));
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
  const int ld1 = kFeat + kNPose + 13;   // 2205
  CK((hipError_t)pack(w[0], ld1, 1024, kFeat, B + m->w1a, 1024, kFeat, 0, 0, 0, 1, s));
  CK((hipError_t)pack(w[1], 1, 1024, 1, B + m->b1, 1024, 1, 0, 0, 0, 1, s));
  CK((hipError_t)pack(w[0] + kFeat, ld1, 1024, 157, B + m->w1b, 1024, kState, 0, 0, 0, 1, s));
  CK((hipError_t)pack(w[2], 1024, 1024, 1024, B + m->w2, 1024, 1024, 0, 0, 0, 1, s));
  CK((hipError_t)pack(w[3], 1, 1024, 1, B + m->b2, 1024, 1, 0, 0, 0, 1, s));
  // decoders stacked: rows 0..143 decpose, 144..153 decshape, 154..156 deccam, rest zero
  CK(launch_fill(B + m->wdec, 256 * 1024, 0.f, s));
  CK(launch_fill(B + m->bdec, kState, 0.f, s));
  CK(launch_fill(B + m->init, kState, 0.f, s));
  const int rows[3] = {kNPose, 10, 3}, off[3] = {0, kNPose, kNPose + 10};
  for (int i = 0; i < 3; ++i) {
    CK((hipError_t)pack(w[4 + 2 * i], 1024, rows[i], 1024, B + m->wdec + (size_t)off[i] * 1024, rows[i], 1024,
                        0, 0, 0, 1, s));
    CK((hipError_t)pack(w[5 + 2 * i], 1, rows[i], 1, B + m->bdec + off[i], rows[i], 1, 0, 0, 0, 1, s));
    CK((hipError_t)pack(w[10 + i], 1, rows[i], 1, B + m->init + off[i], rows[i], 1, 0, 0, 0, 1, s));
  }
  CK((hipError_t)derive_planes(m, Owner::regressor, s));
  m->reg_packed = true;
  CK((hipError_t)range_check(m, m->w1a, m->smpl.J0, &m->reg_range_ok, s));
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
  int par[kNJ], dep[kNJ], maxd = 0;
  for (int j = 0; j < kNJ; ++j) {
    par[j] = parents_host[j];
    if (j == 0) { dep[j] = 0; par[j] = -1; continue; }
    if (par[j] < 0 || par[j] >= j) return TEPOSE_E_ARG;   // parents must precede children
    dep[j] = dep[par[j]] + 1;
    if (dep[j] > maxd) maxd = dep[j];
  }
  m->maxdepth = maxd;
  CK(hipMemcpyAsync(B + m->smpl.parents, par, sizeof(par), hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(B + m->smpl.depth, dep, sizeof(dep), hipMemcpyHostToDevice, s));
  CK(hipStreamSynchronize(s));   // par/dep are stack arrays (pack time only, never on the forward path)
  CK(launch_smpl_consts(v_template, shapedirs, posedirs, J_regressor, B + m->smpl.J0, B + m->smpl.JS,
                        B + m->smpl.blendW, s));
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
