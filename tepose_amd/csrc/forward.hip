// Every forward path: workspace carving and sizes, the encoder (layer-0 projection, per-layer projections and cell steps, tail linears), the regressor +
// SMPL, the cached window path, the VIBE bootstrap encoder -- and, at the end, their extern "C" entry points: argument checks, select_kernels, one call
// down.  Host code only; which kernel family runs is the plan's decision (plan.hip), where a weight lives the blob's (blob.hip).  Nothing here allocates
// device memory or synchronises the device.
#include "plan.h"
#include "state.h"
#include "tap.h"

using namespace tepose;

namespace {

// a workspace being carved: state.h's sequential carve plus the base that turns its offsets into addresses (a sizing pass needs none: plain Carve)
struct Carver : Carve {
  char* base; size_t cap;
  Carver(void* p, size_t c) : base((char*)p), cap(c) {}
  float* at(size_t off) const { return base && off != kNoRef ? (float*)base + off : nullptr; }    // kNoRef (a buffer this shape does not have): nullptr
  Planes planes(const APlanes& p) const { return Planes{(half_t*)at(p.hi), (half_t*)at(p.lo), p.kst}; }
};

// Buffers of one encoder forward (shared between sizing and execution): where they lie is state.h's EncLayout; here the offsets meet the workspace base.
// The split-precision path mirrors every state buffer as fp16 hi / lo planes inside state_hi / state_lo, in ONE format per forward (blocked, or the
// scaled one where the plan says `scaled`): every kernel of a forward agrees on it.
struct EncWs {
  EncLayout o;
  float* base = nullptr;
  float *xp, *g0, *g0c, *y1, *rs, *rs0;
  half_t *state_hi, *state_lo, *x0h, *x0l;
  unsigned long long* gran;    // {tag, hi|lo} granule buffers of the persistent kernel's B <= 16 mode
  unsigned* sync;              // persistent recurrent kernel (gru_seq.hip): per layer 3 x 32 arrival counters, then a status word
  size_t Bs = 0;               // rows per time slab of the state buffers: B, or B rounded up to 16 on the split path
  float* at(size_t off) const { return base && off != kNoRef ? base + off : nullptr; }    // kNoRef (no previous state, not blocked): nullptr
  float* rows(const StateBuf& b) const { return at(b.off); }
  Planes planes(const StateRef& r) const { return Planes{state_hi + r.p, state_lo + r.p, r.kst}; }
  // the tail linears' A planes from column k0 on: the whole [B x 3Hp] operand (0), or its K range behind relu(last forward state) (Hp)
  Planes tail(long k0) const {
    half_t *hi = (half_t*)at(o.tailA.hi), *lo = (half_t*)at(o.tailA.lo);
    return Planes{hi ? hi + o.tailA.k(k0) : nullptr, lo ? lo + o.tailA.k(k0) : nullptr, o.tailA.kst};
  }
};

// floats of the granule buffers: [3 directions][2 buffers][16 rows][Hp] uint64, only where the persistent kernel can run
inline size_t seq_gran_words(const tepose_model* m, const KernelPlan& k) { return k.gran ? (size_t)3 * 2 * kSeqGranRows * m->Hp * 2 : 0; }
inline size_t sync_zero_bytes(const tepose_model* m, const KernelPlan& k) {      // counters + granules: the block a forward clears
  return align_up(sync_words(m) * sizeof(unsigned), 256) + seq_gran_words(m, k) * sizeof(float);
}

EncShape enc_shape(const tepose_model* m, const KernelPlan& k, int B, int T) {
  return EncShape{m->L, m->Hp, B, T, k.h3, k.scaled, k.gblk, sync_words(m), seq_gran_words(m, k)};
}

void carve_encoder(const tepose_model* m, const KernelPlan& k, int B, int T, Carver& c, EncWs& w) {
  w.o = carve_encoder(enc_shape(m, k, B, T), c);
  const EncLayout& o = w.o;
  w.base = (float*)c.base; w.Bs = o.Bs;
  w.sync = (unsigned*)c.at(o.sync); w.gran = (unsigned long long*)c.at(o.gran);
  w.xp = c.at(o.xp); w.g0 = c.at(o.g0); w.g0c = c.at(o.g0c); w.y1 = c.at(o.y1); w.rs = c.at(o.rs); w.rs0 = c.at(o.rs0);
  w.state_hi = (half_t*)c.at(o.state_hi); w.state_lo = (half_t*)c.at(o.state_lo);
  w.x0h = (half_t*)c.at(o.x0h); w.x0l = (half_t*)c.at(o.x0l);
}

// ... from a workspace of `bytes`; false: it does not fit
bool carve_encoder(const tepose_model* m, const KernelPlan& k, int B, int T, void* workspace, size_t bytes, EncWs& w) {
  Carver c(workspace, bytes);
  carve_encoder(m, k, B, T, c, w);
  return c.cur <= bytes;
}

// An activation matrix of the regressor as it was carved: fp32 rows and -- split path -- the blocked planes the previous product (or a split) leaves
struct Act {
  float* rows = nullptr; long ld = 0; Planes P;
  AOperand A() const { return AOperand{rows, ld, P}; }
};

// Buffers of one regressor / SMPL call (shared between sizing and execution): where they lie is state.h's RegLayout; here the offsets meet the workspace
// base.  What the plan does not keep (operand planes without h3, the scaled pose-feature planes without blend16) is nullptr.
struct RegWs {
  RegLayout o;
  float* ws = nullptr;
  unsigned* sync;                  // see sync_words()
  Act feat, xs, h1, h2, pf;        // feat: planes only, its rows are the caller's
  float *base, *amat, *posed, *vposed;
  half_t *pf16h, *pf16l; float* pfrs;
  float* at(size_t off) const { return ws && off != kNoRef ? ws + off : nullptr; }
  Act act(const RegAct& a) const { return Act{at(a.rows), a.ld, Planes{(half_t*)at(a.P.hi), (half_t*)at(a.P.lo), a.P.kst}}; }
};

RegShape reg_shape(const tepose_model* m, const KernelPlan& k, int N) { return RegShape{N, k.h3, k.blend16, sync_words(m)}; }

void bind_regressor(const RegLayout& o, void* workspace, RegWs& w) {
  w.o = o; w.ws = (float*)workspace;
  w.sync = (unsigned*)w.at(o.sync);
  w.feat = w.act(o.feat); w.xs = w.act(o.xs); w.h1 = w.act(o.h1); w.h2 = w.act(o.h2); w.pf = w.act(o.pf);
  w.base = w.at(o.base); w.amat = w.at(o.amat); w.posed = w.at(o.posed); w.vposed = w.at(o.vposed);
  w.pf16h = (half_t*)w.at(o.pf16h); w.pf16l = (half_t*)w.at(o.pf16l); w.pfrs = w.at(o.pfrs);
}

// ... from a workspace of `bytes`; false: it does not fit
bool carve_regressor(const tepose_model* m, const KernelPlan& k, int N, void* workspace, size_t bytes, RegWs& w) {
  Carve c;
  bind_regressor(carve_regressor(reg_shape(m, k, N), c), workspace, w);
  return c.cur <= bytes;
}

hipError_t init_state(const float* init160, const float* pose, const float* shape, const float* cam, float* xs, int N,
                      hipStream_t s) {
  if (pose || shape || cam) return launch_init_state_rows(init160, pose, shape, cam, xs, N, s);
  return launch_init_state(init160, xs, N, s);
}

// the argument structs of the split families (the exact one's: model.h f32_args), from the same description of a product; Np / Kp and every plane
// address come from the weight's record
H3Args h3_args(const float* blob, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e) {
  const WPlanes wp = w_planes(blob, W, Fmt::blocked);
  H3Args p{A.p.hi, A.p.lo, A.p.kst, wp.hi, wp.lo, wp.kst, W.w->Kp, C, ldc, e.bias, M, N};
  p.addend = e.addend; p.ldadd = e.ldadd; p.scale = e.scale; p.row_scale = A.row_scale;
  if (e.out) { p.Chi = e.out->hi; p.Clo = e.out->lo; p.c_kst = e.out->kst; }
  return p;
}

// (a barrier-free kernel (gemm_h3s16c.hip) reports a give-up to the forward's status word -- the recurrent part's, or the regressor's -- and the handle's
// fault word; the test knob that provokes one (TEPOSE_TEST_FAULT bit 2) aims at the encoder's products only)
H3SArgs h3s_args(const tepose_model* m, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e) {
  const WPlanes ws = w_planes(m->blob, W, Fmt::scaled);
  H3SArgs a{A.s.hi, A.s.lo, A.s.kst, ws.hi, ws.lo, ws.kst, W.w->Kp, C, ldc, e.bias, W.w->inv_scale(A.s_scale), M, N, A.row_scale};
  if (e.sync) a.status = e.reg ? sync_reg_status(m, e.sync) : sync_gru_status(m, e.sync);
  a.fault = m->fault;
  a.inject = e.reg ? 0u : (m->test_fault >> 2) & 1u;
  a.c_blk_hp = e.c_blk_hp;
  return a;
}

}  // namespace

// The one place where a product's family becomes a launch: exact fp32 (gemm.hip / skinny.hip), split precision on blocked planes (gemm_h3.hip /
// skinny_h3.hip), scaled planes (gemm_h3s.hip, gemm_h3s16c.hip).  Plain values in, one launch out: nothing is allocated or looked up here.
int tepose::product(const tepose_model* m, Mm f, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e, hipStream_t s, bool tail_stage) {
  switch (f) {
    case Mm::f32: return (int)launch_gemm_tiles(f32_args(m->blob, A, W, C, ldc, M, N, e), s, m->opt);
    case Mm::f32_skinny: return (int)launch_skinny_gemm(f32_args(m->blob, A, W, C, ldc, M, N, e), s);
    case Mm::h3:
    case Mm::h3_skinny: {
      H3Batch b{};
      b.p[0] = h3_args(m->blob, A, W, C, ldc, M, N, e);
      // (a tail-stage product of 160 columns: always width-first -- 2 column tiles of the big kernel would use 64 CUs)
      if (f == Mm::h3_skinny || (tail_stage && N <= 256)) return (int)launch_skinny_gemm_h3(b.p[0], s, m->opt);
      b.n = 1;
      return (int)launch_gemm_h3(b, s, m->opt);
    }
    case Mm::h3s_mid: return (int)launch_gemm_h3s_mid(h3s_args(m, A, W, C, ldc, M, N, e), s);
    case Mm::h3s0:
    case Mm::h3s: return (int)launch_gemm_h3s(h3s_args(m, A, W, C, ldc, M, N, e), s, m->opt, e.tag);
  }
  return (int)hipErrorInvalidValue;
}

namespace {

// a product of the plan's tail stage, on the plan's family for it
int tail_product(const tepose_model* m, const KernelPlan& plan, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e, hipStream_t s) {
  return product(m, plan.tail, A, W, C, ldc, M, N, e, s, true);
}

// v_posed = v_template + shapedirs beta + posedirs^T pose_feature as one GEMM, K = 224
int blend_shapes(const tepose_model* m, const KernelPlan& k, const RegWs& w, int N, hipStream_t s) {
  AOperand A = w.pf.A();      // (the prep kernel wrote the pose-feature planes next to the fp32 rows)
  Epilogue e;
  if (k.smpl == Smpl::h3s) {
    // large batches: K = 224 is 7 pairs of K-tiles -- on the one-workgroup-per-tile kernel every tile pays pipeline fill, drain and a 128 KB store burst
    // (0.40 ms for 677 MB of output); the persistent barrier-free kernel streams the next tile's stages under the finished tile's stores
    CK(launch_split_rows(w.pf.rows, kBlendK, N, kBlendK, kBlendK, N, 1, w.pf16h, w.pf16l, w.pfrs, s, k.input_blend == Rows::split_few));
    A.s = Planes{w.pf16h, w.pf16l, (long)N * 16}; A.row_scale = w.pfrs;
    e.sync = w.sync; e.reg = true;
  }
  const Mm f = k.smpl == Smpl::h3s ? Mm::h3s : k.smpl == Smpl::h3 ? Mm::h3 : k.smpl == Smpl::f32_skinny ? Mm::f32_skinny : Mm::f32;
  return product(m, f, A, m->blend, w.vposed, kVertLd, N, 3 * kNV, e, s);
}

// The SMPL chain: prep (the caller's launch: from the regressor's state rows or from a pose) -> blend-shape product -> skinning
// -- or, a window or a few, all three as one launch (smpl.hip)
template <class Small, class Prep>
int smpl_chain(const tepose_model* m, const KernelPlan& k, const SmplConsts& sc, const RegWs& w, int N, float* verts, hipStream_t s, Small small, Prep prep) {
  if (k.smpl == Smpl::small) return (int)small();
  CK(prep(w.pf.P.hi, w.pf.P.lo, w.pf.P.kst));
  CK((hipError_t)blend_shapes(m, k, w, N, s));
  CK(launch_smpl_skin(sc, w.vposed, w.amat, N, verts, s));
  return 0;
}

// the optional 17-row evaluation regressor as tepose_pack_jreg laid it out
JregPacked jreg_view(const void* jreg_packed) {
  const int* p = (const int*)jreg_packed;
  return JregPacked{p, p + 32, (const float*)(p + 32 + 17 * kNV)};
}

// Where the layer-0 gate pre-activations (x W_ih^T + b_ih, 9Hp columns: fwd | rec_reverse | rec) of a
// window's frames live.  Regular forward: one buffer, frame t at base + t*frame_stride.  Cached driver:
// frame t of the window sits in slot (first + t) % ring of a per-clip ring, except the newest frame
// (theta slots still zero), which has its own buffer.
struct G0Src {
  const float* base; long frame_stride, row_stride;
  int first, ring;                 // ring == 0: no wrap
  const float* last; long last_ld; // newest frame's projections or nullptr
  const float* single; long single_ld;   // L == 1: source of the one consumed rec.l0 forward step
  long blk = 0;                    // != 0: base is in the blocked layout (formats.h gi_blk_offset), floats between 16-row tiles; frames are row_stride * B apart
};

// profiling (tepose_set_profiling) is the one thing a forward writes into its handle: the handle to write to, or nullptr while profiling is off
tepose_model* prof_of(const tepose_model* m) { return m->prof ? const_cast<tepose_model*>(m) : nullptr; }
int prof_mark(std::vector<hipEvent_t>& ev, size_t& used, hipStream_t s) {     // record the next event of an interval list, growing it on first use
  if (ev.size() < used + 1) {
    hipEvent_t e;
    CK(hipEventCreate(&e));
    ev.push_back(e);
  }
  CK(hipEventRecord(ev[used++], s));
  return 0;
}

// Gate pre-activations of one direction of a cell step (dir: 0 fwd | 1 rec_reverse | 2 rec): layers >= 1 from the workspace, layer 0 from frame d.frame
// of the G0Src (frame < 0: the one consumed rec.l0 forward step).  blk != 0: in the blocked layout, floats between 16-row tiles
struct Gi { const float* p; long ld, blk; };
Gi gate_in(const G0Src& src, const EncWs& w, int T, int H3, int l, int dir, const DirStep& d) {
  if (l > 0) return Gi{w.at(d.gi.f), d.gi.ld, d.gi.bst};
  if (d.frame < 0) return Gi{src.single, src.single_ld, 0};
  if (src.last && d.frame == T - 1) return Gi{src.last + (long)dir * H3, src.last_ld, src.blk};
  const int slot = src.ring ? (src.first + d.frame) % src.ring : d.frame;
  return Gi{src.base + (long)slot * src.frame_stride + (long)dir * H3 * (src.blk ? 16 : 1), src.row_stride, src.blk};
}

// the cell-step order of a layer's directions: gru_fwd, gru_rec reverse, gru_rec forward
struct LayerDirs { const DirW* d[3]; };
LayerDirs layer_dirs(const tepose_model* m, int l) { return LayerDirs{{&m->fwd[l], &m->rec_r[l], &m->rec_f[l]}}; }

// input projection of a layer >= 1: fp32 kernel, or the scaled-plane kernel on the mirrors of the input states
int project_l1(const tepose_model* m, const KernelPlan& plan, const EncWs& w, Mm f, const StateBuf& in, const DirW& d, const StateBuf& out, int M, hipStream_t s) {
  const int H3 = 3 * m->Hp;
  AOperand A{w.rows(in), d.ih.Kp};
  if (f == Mm::h3s) { A.s = w.planes(in.at(0)); A.s_scale = kStateScale; }
  Epilogue e{w_bias(m->blob, d.ih)};
  e.sync = w.sync; e.c_blk_hp = plan.gblk ? m->Hp : 0;
  return product(m, f, A, d.ih, w.rows(out), H3, M, H3, e, s);
}

// The three input projections of layer l >= 1 from the states of layer l - 1: gru_fwd and gru_rec's reverse direction for every slab row, gru_rec's forward
// direction for every slab row too -- or, on the top layer, for the one step it consumes.
int layer_projections(const tepose_model* m, const KernelPlan& plan, const EncWs& w, int B, int T, int l, hipStream_t s) {
  const int Hp = m->Hp, H3 = 3 * Hp;
  const float* Bl = m->blob;
  const long Bs = (long)w.Bs;
  const bool top = l == m->L - 1;
  const StateBuf &inf = w.o.sf[(l - 1) & 1], &inr = w.o.sr[(l - 1) & 1];
  const int MT = (int)(Bs * T);       // every slab row, pad rows included (their results are never read)
  const int Mf = top ? B : MT;         // the top layer's forward direction of gru_rec consumes one step only
  const Mm ff = top ? plan.proj_one : plan.proj_l1;
  if (plan.proj_l1 != Mm::h3 && plan.proj_l1 != Mm::h3_skinny) {
    CK((hipError_t)project_l1(m, plan, w, plan.proj_l1, inf, m->fwd[l], w.o.gf, MT, s));
    CK((hipError_t)project_l1(m, plan, w, plan.proj_l1, inr, m->rec_r[l], w.o.grr, MT, s));
    return project_l1(m, plan, w, ff, inr, m->rec_f[l], w.o.grf, Mf, s);
  }
  // the three products of a layer in as few launches as their shapes allow (each alone under-fills the chip:
  // 64-192 workgroups): width-first kernel for few rows, 128/256-row tiles above
  const Planes vf = w.planes(inf.at(0)), vr = w.planes(inr.at(0));
  auto mk = [&](const Planes& v, const DirW& d, float* out, int M) {
    return h3_args(Bl, AOperand{nullptr, 0, v}, d.ih, out, H3, M, H3, Epilogue{w_bias(Bl, d.ih)});
  };
  // longest K first: the blocks of a batched launch are dealt product by product, and the chip finishes a mix of
  // K = 2Hp and K = Hp tiles sooner when the long ones start first (1.5 -> 1.0 long-tile times at 1024 rows)
  H3Args pa[3] = {mk(vr, m->rec_r[l], w.rows(w.o.grr), MT), mk(vr, m->rec_f[l], w.rows(w.o.grf), Mf), mk(vf, m->fwd[l], w.rows(w.o.gf), MT)};
  const Mm fam[3] = {plan.proj_l1, ff, plan.proj_l1};
  H3ArgsBatch sk{};
  H3Batch big{};
  // width-first kernel up to 192 real rows (three 64-row passes over the weights), tiles above: with 64-row tiles (launch_gemm_h3, round 5) the tile
  // kernel is flat at ~35 us up to a round of the chip, the width-first one costs ~12-16 us per pass (222 rows: 48.7 -> 37 us; 150 rows: stays)
  for (int i = 0; i < 3; ++i) {
    H3Args& a = pa[i];
    if (fam[i] == Mm::h3_skinny) {
      // width-first kernel: only the B real rows of every 16-row-padded time slab (B = 1: 16 rows instead of 256)
      if (a.M == MT && Bs != B) { a.M = B * T; a.grp_rows = B; a.grp_stride = (int)Bs; }
      sk.p[sk.n++] = a;
    }
    else if (big.n == 0 || (big.p[0].M == a.M && big.p[0].N == a.N)) big.p[big.n++] = a;
    else {                           // a big product of another shape: its own launch
      H3Batch one{};
      one.p[0] = a; one.n = 1;
      CK(launch_gemm_h3(one, s, m->opt));
    }
  }
  if (big.n) CK(launch_gemm_h3(big, s, m->opt));
  if (sk.n) CK(launch_skinny_gemm_h3_batch(sk, s, m->opt));
  return 0;
}

// Where every direction of a cell step reads and writes is state.h's decision (cell_step, cell_top_rec_fwd: a CellStep of offsets).  The three fillers
// below turn one into the arguments of a kernel family -- base added, weights attached, nothing looked up.

// exact fp32 (gemm.hip / skinny.hip)
GruArgs gru_args(const tepose_model* m, const G0Src& src, const EncWs& w, int B, int T, int l, const CellStep& c, const LayerDirs& dw) {
  GruArgs a{};
  a.M = B; a.Hp = m->Hp; a.first = c.first; a.ndir = c.ndir;
  for (int k = 0; k < c.ndir; ++k) {
    const DirStep& q = c.d[k];
    const Gi gi = gate_in(src, w, T, 3 * m->Hp, l, k, q);
    GruDir& d = a.d[k];
    d.Whh = w_rows(m->blob, dw.d[k]->hh); d.bhh = w_bias(m->blob, dw.d[k]->hh);
    d.gi = gi.p; d.ldgi = gi.ld; d.gi_blk = gi.blk;
    d.hprev = w.at(q.hprev.f); d.ldh = q.hprev.ld;
    d.hout = w.at(q.hout.f); d.ldo = q.hout.ld;
  }
  return a;
}

// one GRU step of up to 3 directions (dw: their weights): fused fp32 kernel; or the split product with the cell update in its
// epilogue (first step: h = 0, element-wise kernel)
int launch_cell_step(const tepose_model* m, const KernelPlan& plan, const G0Src& src, const EncWs& w, Step f, int B, int T, int l, const CellStep& c,
                     const LayerDirs& dw, hipStream_t s) {
  if (f == Step::f32_skinny) return (int)launch_skinny_gru(gru_args(m, src, w, B, T, l, c, dw), s);       // (first steps too: plan.first names the same exact-fp32 kernel)
  if (f == Step::f32) return (int)launch_gru_step_tiles(gru_args(m, src, w, B, T, l, c, dw), s);
  const int Hp = m->Hp, H3 = 3 * Hp;
  const bool s16 = f == Step::s16 || f == Step::s16_planes;
  H3SBatch b16{};
  H3Batch b{};
  GateBatch gb{};
  for (int d = 0; d < c.ndir; ++d) {
    const DirStep& q = c.d[d];
    const Gi gi = gate_in(src, w, T, H3, l, d, q);
    const Planes vo = w.planes(q.hout);
    GateDir g{gi.p, gi.ld, w_bias(m->blob, dw.d[d]->hh), w.at(q.hprev.f), q.hprev.ld, w.at(q.hout.f), q.hout.ld, vo.hi, vo.lo, vo.kst};
    if (s16) {
      g.gi_blk = gi.blk;
      g.hprev_b = w.at(q.hprev.b); g.hp_blk = q.hprev.bst;
      g.hout_b = w.at(q.hout.b); g.ho_blk = q.hout.bst;
    }
    (s16 ? b16.gate[d] : b.gate[d]) = g;
    gb.d[d] = g;
    if (c.first) continue;
    // the recurrent product h_{t-1} W_hh^T: no C, no bias -- the cell update is the kernel's epilogue
    AOperand A;
    Epilogue e;
    if (s16) {
      A.s = w.planes(q.hprev); A.s_scale = kStateScale;
      e.sync = w.sync;
      b16.p[d] = h3s_args(m, A, dw.d[d]->hh, nullptr, 0, B, H3, e);
    } else {
      A.p = w.planes(q.hprev);
      b.p[d] = h3_args(m->blob, A, dw.d[d]->hh, nullptr, 0, B, H3, e);
    }
  }
  if (c.first) return (int)launch_gru_first(gb, c.ndir, B, Hp, s, s16 ? 1 : 0, s16 && plan.first == First::h3_16);
  if (s16) {
    b16.n = c.ndir; b16.Hp = Hp; b16.state_scale = kStateScale;
    // the plane-fed instantiation wants this layer's gate pre-activations blocked: layers >= 1 always are (gblk), layer 0 only where the projection
    // wrote them frame-major + blocked (g0blk; not from the driver's cache ring).  One decision per layer: every step of a layer runs the same kernel.
    // (a misaligned view or a ragged tile the plan did not foresee: the general instantiation, not an error)
    const bool planes = f == Step::s16_planes && gru_step16_planes_ok(b16);
    return (int)launch_gru_step16(b16, s, planes, m->opt.gru_gm);
  }
  b.n = c.ndir; b.Hp = Hp;
  if (f == Step::h3_skinny) return (int)launch_skinny_gru_h3(b, s);
  return (int)launch_gru_h3(b, s);
}

// persistent kernel (gru_seq.hip): all T steps of the ndir directions of layer l as one launch.  The top layer's launch also takes the one cell step of
// gru_rec's forward direction and writes relu(final states) straight into the tail product's A planes: [fwd | rec forward | rec reverse]
int launch_layer_seq(const tepose_model* m, const KernelPlan& plan, const G0Src& src, const EncWs& w, int B, int T, int l, hipStream_t s) {
  const int Hp = m->Hp, H3 = 3 * Hp;
  const bool top = l == m->L - 1;
  const LayerDirs dw = layer_dirs(m, l);
  GruSeqArgs sq{};
  sq.ndir = top ? 2 : 3;
  for (int d = 0; d < sq.ndir; ++d) {
    const WPlanes wp = w_planes(m->blob, dw.d[d]->hh, Fmt::blocked);
    sq.whi[d] = wp.hi; sq.wlo[d] = wp.lo; sq.w_kst = wp.kst; sq.bhh[d] = w_bias(m->blob, dw.d[d]->hh);
  }
  for (int st = 0; st < T; ++st) {
    const CellStep c = cell_step(w.o, m->L, T, l, st);
    for (int d = 0; d < c.ndir; ++d) {
      const DirStep& q = c.d[d];
      const Gi gi = gate_in(src, w, T, H3, l, d, q);
      GruSeqStep& e = sq.st[d][st];
      e.gi = gi.p; e.ldgi = (int)gi.ld; e.hout = w.at(q.hout.f); e.ldo = (int)q.hout.ld;
      e.poff = (unsigned)q.hout.p; e.pkst = (unsigned)q.hout.kst;
    }
  }
  sq.phi = w.state_hi; sq.plo = w.state_lo;
  sq.counters = sync_gru(w.sync, l); sq.status = sync_gru_status(m, w.sync);
  sq.fault = m->fault; sq.spin_limit = m->spin_limit; sq.inject = (m->test_fault & 1u) ? 1u : 0u;
  sq.T = T; sq.M = B; sq.Hp = Hp;
  sq.gran = (l == 0 ? plan.step0 : plan.step1) == Step::seq_gran ? w.gran : nullptr; sq.tag_base = (unsigned)l * 64u;
  const Planes tail = w.tail(0);
  sq.rhi = tail.hi; sq.rlo = tail.lo; sq.r_kst = (unsigned)tail.kst;
  sq.r_off[0] = sq.r_off[1] = sq.r_off[2] = sq.x_roff = kNoPlane;
  if (top) {
    const DirStep x = cell_top_rec_fwd(w.o, l).d[0];
    const Gi gi = gate_in(src, w, T, H3, l, 2, x);
    sq.x_gi = gi.p; sq.x_ldgi = (int)gi.ld;
    sq.x_bhh = w_bias(m->blob, m->rec_f[l].hh); sq.x_hout = w.at(x.hout.f); sq.x_ldo = (int)x.hout.ld;
    sq.x_poff = (unsigned)x.hout.p; sq.x_pkst = (unsigned)x.hout.kst;
    // the tail operand's K ranges: relu(fwd) [0, Hp), relu(rec forward) [Hp, 2 Hp), relu(rec reverse) [2 Hp, 3 Hp)
    sq.r_off[0] = (unsigned)w.o.tailA.k(0); sq.x_roff = (unsigned)w.o.tailA.k(Hp); sq.r_off[1] = (unsigned)w.o.tailA.k(2 * Hp);
  }
  return (int)launch_gru_seq(sq, s, m->opt);
}

// y_fwd = linear_fwd(relu(y[-1])), y_rec = linear_rec(relu(y_rec[0])): the feature (eval: their mean; is_train: both, side by side), or -- xs_out, eval
// mode of tail_collapsed handles -- the regressor's final state rows [B][160] = [relu(h_fwd) | relu(y_rec0)] Mt^T + kt instead: the tail linears and the
// three FC iterations as one product.  tail_planes_done: the persistent kernel of the top layer wrote relu(final states) as planes
int encoder_tail(const tepose_model* m, const KernelPlan& plan, const EncWs& w, int B, int T, int is_train, float* feat, const Planes* feat_planes,
                 float* xs_out, bool tail_planes_done, hipStream_t s) {
  const int Hp = m->Hp;
  const float* Bl = m->blob;
  const float *hlast = w.rows(w.o.pf[(T - 1) & 1]), *ytop = w.rows(w.o.ytop);
  // relu(last forward state), relu(ytop): their planes (ReLU'd when written) -- the K ranges [0, Hp) and [Hp, 3Hp) of the tail operand --, or -- exact
  // fp32 -- the rows, with the ReLU on the fly (relu_a)
  const Planes tailA = w.tail(0), tailF = tailA, tailR = w.tail(Hp);
  const AOperand Af{hlast, Hp, tailF}, Ar{ytop, 2 * Hp, tailR};
  const float *blf = w_bias(Bl, m->wlf), *blr = w_bias(Bl, m->wlr);
  if (plan.h3) {
    if (!tail_planes_done) {
      CK(launch_split_planes(hlast, Hp, B, Hp, Hp, B, tailF.hi, tailF.lo, s, 1));
      CK(launch_split_planes(ytop, 2 * Hp, B, 2 * Hp, 2 * Hp, B, tailR.hi, tailR.lo, s, 1));
    }
    const AOperand A{nullptr, 0, tailA};      // [relu(h_fwd) | relu(y_rec0)]
    if (!is_train && xs_out && plan.tail_collapsed) return tail_product(m, plan, A, m->mt, xs_out, kState, B, kState, Epilogue{w_bias(Bl, m->mt)}, s);
    // eval: (y_fwd + y_rec) / 2 = ([relu(h_fwd) | relu(y_rec0)] [W_lf | W_lr]^T + b_lf + b_lr) / 2: one product, K = 3Hp
    // (b_lr rides in as an addend row with stride 0)
    if (!is_train) return tail_product(m, plan, A, m->wlfr, feat, kFeat, B, kFeat, Epilogue{blf, blr, 0, 0.5f, 0, feat_planes}, s);
    // is_train: both, side by side
    CK((hipError_t)tail_product(m, plan, Af, m->wlf, feat, 2 * kFeat, B, kFeat, Epilogue{blf}, s));
    return tail_product(m, plan, Ar, m->wlr, feat + kFeat, 2 * kFeat, B, kFeat, Epilogue{blr}, s);
  }
  // exact fp32: eval adds y_fwd (in y1) inside the second product
  float* yf = is_train ? feat : w.y1;
  const long ld = is_train ? 2 * kFeat : kFeat;
  CK((hipError_t)tail_product(m, plan, Af, m->wlf, yf, ld, B, kFeat, Epilogue{blf, nullptr, 0, 0.f, 1}, s));
  const Epilogue er = is_train ? Epilogue{blr, nullptr, 0, 0.f, 1} : Epilogue{blr, w.y1, kFeat, 0.5f, 1};
  return tail_product(m, plan, Ar, m->wlr, is_train ? feat + kFeat : feat, ld, B, kFeat, er, s);
}

// the T cell steps of layer l (the top layer: plus the one step of gru_rec's forward direction)
int layer_cells(const tepose_model* m, const KernelPlan& plan, const G0Src& src, const EncWs& w, int B, int T, int l, bool seq, hipStream_t s) {
  if (seq) return launch_layer_seq(m, plan, src, w, B, T, l, s);      // small batches: one persistent launch
  const Step f = l == 0 ? plan.step0 : plan.step1;
  const LayerDirs dw = layer_dirs(m, l);
  for (int st = 0; st < T; ++st) CK((hipError_t)launch_cell_step(m, plan, src, w, f, B, T, l, cell_step(w.o, m->L, T, l, st), dw, s));
  if (l < m->L - 1) return 0;
  return launch_cell_step(m, plan, src, w, f, B, T, l, cell_top_rec_fwd(w.o, l), LayerDirs{{&m->rec_f[l], nullptr, nullptr}}, s);
}

// The encoder from the layer-0 gate pre-activations on: per layer the input projections (layers >= 1) and the cell steps, then the tail linears.
// small batches (seq): all T steps of a layer in one persistent launch (gru_seq.hip)
int encoder_core(const tepose_model* m, const KernelPlan& plan, const G0Src& src, int B, int T, int is_train, float* feat, EncWs& w,
                 hipStream_t s, const Planes* feat_planes = nullptr, bool sync_zeroed = false, float* xs_out = nullptr) {
  tepose_model* pm = prof_of(m);
  const int L = m->L;
  // layer >= 1 gate pre-activations in the blocked layout (formats.h gi_blk_offset): producer = the barrier-free projection kernel, consumers =
  // gru_step16_kernel / gru_first16_kernel / gru_first_kernel
  if (src.blk && !plan.gblk) return (int)hipErrorInvalidValue;   // the caller projected layer 0 into the blocked layout: every consumer here must read it
  const bool seq = plan.step0 == Step::seq || plan.step0 == Step::seq_gran;     // (every layer: the plan decides it once for the forward)
  // every forward clears its sync region -- arrival counters, granules, and the two STATUS words that tepose_forward_status
  // reads -- whether or not a persistent kernel will run (a stale or uninitialised status word would read as a give-up)
  if (!sync_zeroed && w.sync) CK(hipMemsetAsync(w.sync, 0, seq ? sync_zero_bytes(m, plan) : sync_words(m) * sizeof(unsigned), s));
  for (int l = 0; l < L; ++l) {
    const bool top = l == L - 1;
    if (l > 0) {
      CK((hipError_t)layer_projections(m, plan, w, B, T, l, s));
      if (pm) pm->prof_l1_flops += 2.0 * 3.0 * m->H * ((double)B * T * m->H + (double)B * T * 2.0 * m->H + (double)(top ? B : B * T) * 2.0 * m->H);
    }
    if (pm) CK((hipError_t)prof_mark(pm->ev_gru, pm->ev_gru_used, s));
    CK((hipError_t)layer_cells(m, plan, src, w, B, T, l, seq, s));
    if (pm) {
      CK((hipError_t)prof_mark(pm->ev_gru, pm->ev_gru_used, s));
      // consumed cell steps of this layer: fwd T + rec_reverse T + rec forward (T, or 1 on the top layer)
      pm->prof_gru_flops += 2.0 * B * 3.0 * m->H * m->H * (2.0 * T + (top ? 1 : T));
    }
  }
  return encoder_tail(m, plan, w, B, T, is_train, feat, feat_planes, xs_out, seq, s);
}

SmplConsts smpl_consts(const tepose_model* m) {
  const float* Bl = m->blob;
  SmplConsts sc{};
  sc.J0 = Bl + m->smpl.J0; sc.JS = Bl + m->smpl.JS; sc.blendW = w_rows(Bl, m->blend);
  sc.lbsW = Bl + m->smpl.lbsW; sc.lbs_cidx = (const int*)(Bl + m->smpl.lbs_cidx); sc.lbs_cval = Bl + m->smpl.lbs_cval;
  sc.lbs_sparse = m->lbs_sparse; sc.parents = (const int*)(Bl + m->smpl.parents);
  sc.depth = (const int*)(Bl + m->smpl.depth); sc.maxdepth = m->maxdepth;
  sc.xr_ptr = (const int*)(Bl + m->smpl.xr_ptr); sc.xr_idx = (const int*)(Bl + m->smpl.xr_idx);
  sc.xr_val = Bl + m->smpl.xr_val;
  return sc;
}

// feat_planes: also leave the feature as hi / lo planes there (the regressor's first A operand), when that region does
// not overlap a buffer the tail product still reads
int encoder_fwd_impl(const tepose_model* m, const KernelPlan& plan, const float* x, int B, int T, int is_train, float* feat,
                     void* workspace, size_t ws_bytes, void* stream, const Planes* feat_planes, bool* wrote_planes, float* xs_out) {
  if (wrote_planes) *wrote_planes = false;
  if (!m || m->kind != 0 || !x || !feat || !workspace || B < 1 || T < 1) return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  if ((size_t)B * T > (1u << 30) / 4) return TEPOSE_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  EncWs w;
  if (!carve_encoder(m, plan, B, T, workspace, ws_bytes, w)) return TEPOSE_E_WORKSPACE;
  const int L = m->L, Hp = m->Hp;
  const float* Bl = m->blob;
  const long BT = (long)B * T;
  const int H3 = 3 * Hp;

  // ---- layer-0 input projections: one GEMM for every direction that runs all T steps --------
  const int ld0 = (L >= 2 ? 9 : 6) * Hp;
  half_t* xh = (half_t*)w.xp;                       // hi / lo planes share the padded-input buffer
  half_t* xl = xh + (size_t)BT * kInputP;
  // h3s0: large batches of an L >= 2 model on the barrier-free scaled-plane kernel (its input planes carry scale 1: same fp16 range as the other
  // layout; elements below 2^-3 keep an absolute error <= 2^-25 instead of a relative one).  h3s_mid: mid-size batches (cfg-B: 64 windows x 16 frames =
  // 1024 rows) on 128 x 288 tiles.  g0blk: gate pre-activations FRAME-major (plane row t * B + b: a GRU step then reads B consecutive rows)
  // and 16 x 16-blocked (formats.h gi_blk_offset).
  const bool g0s = plan.projection == Mm::h3s0 || plan.projection == Mm::h3s_mid, g0blk = plan.g0blk;
  // the caller's windows -> planes with one power-of-two scale per row (any finite fp32 magnitude; DESIGN 4b "range")
  // (the forward's first kernel also clears its sync region -- arrival counters, granules, STATUS words -- so that a give-up of the
  // layer-0 projection (barrier-free kernel, gemm_h3s16c.hip) is not wiped by a clearing that comes after it)
  if (plan.input == Rows::pad) {
    CK(launch_pad_input(x, w.xp, BT, s));
    if (w.sync) CK(hipMemsetAsync(w.sync, 0, sync_zero_bytes(m, plan), s));
  } else {
    CK(launch_split_rows(x, kInput, BT, kInput, kInputP, BT, g0s ? 1 : 0, xh, xl, w.rs, s, plan.input == Rows::split_few, (void*)w.sync,
                         w.sync ? sync_zero_bytes(m, plan) : 0, g0blk ? T : 0));
  }
  {
    tepose_model* pm = prof_of(m);
    if (pm) CK((hipError_t)prof_mark(pm->ev, pm->ev_used, s));
    // A: the padded fp32 rows, or -- in the same buffer -- their planes in the family's format (blocked, or scaled with scale 1).  h3s0: 256 x 256 tiles,
    // one accumulator per tile (the barrier-free kernel loses on mid-size batches: 1024 rows are 144 of its tiles -- 0.138 against 0.119 ms,
    // profiles/r05_mid_rows_gemm.txt); h3_skinny: few rows (live stream, a handful of clips) -- the width-first kernel streams the 79 MB of W_ih planes
    // with N / 48 = 192 workgroups instead of 72 tiles of 128 rows
    const AOperand A{w.xp, kInputP, {xh, xl, BT * 32}, {xh, xl, BT * 16}, 1.f, w.rs};
    Epilogue e{w_bias(Bl, m->wih0)};
    e.sync = w.sync; e.c_blk_hp = g0blk ? Hp : 0; e.tag = 0;
    CK((hipError_t)product(m, plan.projection, A, m->wih0, w.g0, ld0, (int)BT, ld0, e, s));
    if (pm) {
      CK((hipError_t)prof_mark(pm->ev, pm->ev_used, s));
      pm->prof_flops = 2.0 * (double)BT * (double)(L >= 2 ? 9 : 6) * m->H * kInput;
    }
  }
  if (L == 1) {  // rec.l0 forward direction: only flipped index 0 (= frame T-1) is consumed
    AOperand A{w.xp + (long)(T - 1) * kInputP, (long)T * kInputP};
    if (plan.proj_one == Mm::h3) {
      // frames T-1 of every window as compact planes
      CK(launch_split_rows(x + (long)(T - 1) * kInput, (long)T * kInput, B, kInput, kInputP, B, 0, w.x0h, w.x0l, w.rs0, s,
                           plan.input_x0 == Rows::split_few));
      A.p = Planes{w.x0h, w.x0l, (long)B * 32}; A.row_scale = w.rs0;
    }
    const WView rec(m->wih0, 6 * Hp);      // W rows 6Hp.. of the stacked layer-0 block
    CK((hipError_t)product(m, plan.proj_one, A, rec, w.g0c, H3, B, H3, Epilogue{w_bias(Bl, rec)}, s));
  }

  G0Src src{w.g0, ld0, (long)T * ld0, 0, 0, nullptr, 0, w.g0c, H3};
  if (g0blk) { src.frame_stride = (long)B * ld0; src.row_stride = ld0; src.blk = (long)ld0 * 16; }
  if (feat_planes) {
    // live at tail time: the tail product's A planes and the fp32 final states; everything carved before them is dead
    const char* end = (const char*)(feat_planes->lo + (size_t)B * kFeat + 128);
    const char* first_live = (const char*)w.rows(L >= 2 ? w.o.gf : w.o.pf[0]);
    if (!plan.h3 || is_train || end > first_live) feat_planes = nullptr;
  }
  if (wrote_planes) *wrote_planes = feat_planes != nullptr;
  return encoder_core(m, plan, src, B, T, is_train, feat, w, s, feat_planes, true, xs_out);     // cleared above
}

// Buffers of one frame projection of M rows (tepose_project_frames, the pair product; shared between sizing and execution): state.h's ProjLayout on a base
struct ProjWs {
  float* xp; Planes P; float* rs; size_t bytes;
  AOperand A() const { return AOperand{xp, kInputP, P, {}, 1.f, rs}; }
};
ProjWs carve_projection(void* workspace, size_t M, bool h3) {
  Carver c(workspace, 0);
  const ProjLayout o = carve_projection(M, h3, c);
  return ProjWs{c.at(o.xp), c.planes(o.P), c.at(o.rs), c.cur};
}

int project_frames_impl(const tepose_model* m, const KernelPlan& plan, const float* feat, long feat_ld, const float* theta, long theta_ld, int B,
                        float* out, long out_ld, void* workspace, hipStream_t s) {
  const ProjWs w = carve_projection(workspace, B, plan.h3);
  CK(launch_pad_rows(feat, feat_ld, theta, theta_ld, w.xp, B, s));
  if (plan.h3)       // split-precision product, same numerics as tepose_forward's
    CK(launch_split_rows(w.xp, kInputP, B, kInputP, kInputP, B, 0, w.P.hi, w.P.lo, w.rs, s, plan.input == Rows::split_few));
  return product(m, plan.projection, w.A(), m->wih0, out, out_ld, B, 9 * m->Hp, Epilogue{w_bias(m->blob, m->wih0)}, s);
}

// Both projections of a window step of the clip driver as ONE product of 2 B rows (rows [0, B): the previous newest frame with its now-known theta ->
// its ring slot; rows [B, 2 B): the newest frame with zero theta -> the `newest` rows): the 79 MB of layer-0 W_ih planes are streamed once per
// step instead of twice, one input split (which gathers the rows itself) instead of two pads and two splits.  Same GEMM rows on the same operands as
// two tepose_project_frames calls; the width-first kernel may split K over 4 or 8 waves depending on the row count, so results agree to rounding
// (bit for bit at the published width).
// `zero` / `zero_bytes`: a region the input-split kernel clears on its way (the following forward's sync region: tepose_window_step); *zeroed says
// whether it did (the two-call form does not)
int project_frame_pair_impl(const tepose_model* m, const KernelPlan& plan, const float* feat_prev, const float* feat_new, long feat_ld,
                            const float* theta_prev, long theta_ld, int B, float* out_prev, long out_prev_ld, float* out_new, long out_new_ld,
                            void* workspace, size_t ws_bytes, void* stream, void* zero, size_t zero_bytes, bool* zeroed) {
  if (zeroed) *zeroed = false;
  if (!feat_prev || !feat_new || !theta_prev || !out_prev || !out_new || !workspace) return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  if (ws_bytes < tepose_project_frames_workspace_bytes(m, 2 * B)) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (!plan.pair) {            // exact-fp32 products / more rows than the width-first kernel takes: the two products one after the other
    CK((hipError_t)project_frames_impl(m, plan, feat_prev, feat_ld, theta_prev, theta_ld, B, out_prev, out_prev_ld, workspace, s));
    return project_frames_impl(m, plan, feat_new, feat_ld, nullptr, 0, B, out_new, out_new_ld, workspace, s);
  }
  const int M = 2 * B;
  const ProjWs w = carve_projection(workspace, M, true);
  // the split kernel gathers the 2 B rows itself (features | theta, features | zeros): no padded fp32 copy, one launch instead of three
  const RowPairSrc pr{feat_prev, theta_prev, feat_new, feat_ld, theta_ld, B};
  const bool z = zero && zero_bytes && zero_bytes % 16 == 0;
  CK(launch_split_rows(nullptr, 0, M, kInput, kInputP, M, 0, w.P.hi, w.P.lo, w.rs, s, plan.input_pair == Rows::split_few, z ? zero : nullptr,
                       z ? zero_bytes : 0, 0, &pr));
  if (zeroed) *zeroed = z;
  // (the second destination is the width-first kernel's alone: the common filler, then that launcher directly)
  H3Args p = h3_args(m->blob, w.A(), m->wih0, out_prev, out_prev_ld, M, 9 * m->Hp, Epilogue{w_bias(m->blob, m->wih0)});
  p.C2 = out_new; p.ldc2 = out_new_ld; p.c_split = B;
  CK(launch_skinny_gemm_h3(p, s, m->opt));
  return 0;
}

// feat_planes_ready: the encoder's tail product left the feature planes in the workspace; xs_ready: ... or the final state rows
int regressor_impl(const tepose_model* m, const KernelPlan& plan, const float* feat, int N, int n_iter, const float* init_pose,
                   const float* init_shape, const float* init_cam, const void* jreg_packed, float* theta, float* verts,
                   float* kp_3d, float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes, void* stream,
                   bool feat_planes_ready, bool sync_zeroed, const float* xs_ready = nullptr) {
  if (!m || !feat || !theta || !verts || !kp_3d || !kp_2d || !rotmat || !workspace || N < 1 || n_iter < 0)
    return TEPOSE_E_ARG;
  if (!m->reg_packed || !m->smpl_packed) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  RegWs w;
  if (!carve_regressor(m, plan, N, workspace, ws_bytes, w)) return TEPOSE_E_WORKSPACE;
  const float* Bl = m->blob;
  // a stand-alone regressor call clears its sync region (counters + the status words tepose_forward_status reads); inside
  // tepose_forward / tepose_forward_cached the encoder part has done it (sync_zeroed) and may have left a give-up there
  if (!sync_zeroed && w.sync) CK(hipMemsetAsync(w.sync, 0, sync_words(m) * sizeof(unsigned), s));
  // xc = cat[x, pose, shape, cam]; fc1(xc) = x W1a^T + b1 (iteration-invariant) + state W1b^T
  AOperand Afeat = w.feat.A();        // (its rows are the caller's)
  Afeat.rows = feat;
  const bool collapsed = !xs_ready && plan.reg_collapsed && n_iter == 3 && !init_pose && !init_shape && !init_cam;
  if (!xs_ready && plan.h3 && !feat_planes_ready) CK(launch_split_planes(feat, kFeat, N, kFeat, kFeat, N, w.feat.P.hi, w.feat.P.lo, s));
  Epilogue e;
  if (xs_ready) {
    // the encoder's last product already produced the final state rows (collapsed regressor + tail)
    w.xs.rows = const_cast<float*>(xs_ready);
  } else if (collapsed) {
    // the three iterations from the model's own initial state as ONE product: xs = feat Mf^T + k0
    e.bias = w_bias(Bl, m->mf);
    CK((hipError_t)tail_product(m, plan, Afeat, m->mf, w.xs.rows, kState, N, kState, e, s));
  } else if (plan.reg == Reg::seq) {
    // small batches: the whole FC loop in one persistent launch (reg_seq.hip)
    RegSeqArgs ra{};
    ra.fh = w.feat.P.hi; ra.fl = w.feat.P.lo; ra.f_kst = w.feat.P.kst;
    WPlanes p;
    p = w_planes(Bl, m->w1a, Fmt::blocked); ra.w1a_h = p.hi; ra.w1a_l = p.lo;
    p = w_planes(Bl, m->w1b, Fmt::blocked); ra.w1b_h = p.hi; ra.w1b_l = p.lo;
    p = w_planes(Bl, m->w2, Fmt::blocked); ra.w2_h = p.hi; ra.w2_l = p.lo;
    p = w_planes(Bl, m->wdec, Fmt::blocked); ra.wd_h = p.hi; ra.wd_l = p.lo;
    ra.b1 = w_bias(Bl, m->w1a); ra.b2 = w_bias(Bl, m->w2); ra.bdec = w_bias(Bl, m->wdec);
    ra.init160 = Bl + m->init; ra.ipose = init_pose; ra.ishape = init_shape; ra.icam = init_cam;
    ra.h1h = w.h1.P.hi; ra.h1l = w.h1.P.lo; ra.h2h = w.h2.P.hi; ra.h2l = w.h2.P.lo; ra.h_kst = w.h1.P.kst;
    ra.xh = w.xs.P.hi; ra.xl = w.xs.P.lo; ra.x_kst = w.xs.P.kst;
    ra.xs = w.xs.rows; ra.counters = sync_reg(m, w.sync); ra.status = sync_reg_status(m, w.sync);
    ra.fault = m->fault; ra.spin_limit = m->spin_limit; ra.inject = (m->test_fault & 2u) ? 1u : 0u;
    ra.N = N; ra.n_iter = n_iter;
    CK(launch_reg_seq(ra, s));
  } else {
    // a launch per product, either family: the split kernels also leave every result as planes, the next product's A
    e.bias = w_bias(Bl, m->w1a);
    CK((hipError_t)tail_product(m, plan, Afeat, m->w1a, w.base, 1024, N, 1024, e, s));
    CK(init_state(Bl + m->init, init_pose, init_shape, init_cam, w.xs.rows, N, s));
    if (plan.h3) CK(launch_split_planes(w.xs.rows, kState, N, kState, kState, N, w.xs.P.hi, w.xs.P.lo, s));
    Epilogue e1{nullptr, w.base, 1024}, e2{w_bias(Bl, m->w2)}, e3{w_bias(Bl, m->wdec), w.xs.rows, kState};
    e1.out = &w.h1.P; e2.out = &w.h2.P; e3.out = &w.xs.P;
    for (int it = 0; it < n_iter; ++it) {
      CK((hipError_t)tail_product(m, plan, w.xs.A(), m->w1b, w.h1.rows, 1024, N, 1024, e1, s));
      CK((hipError_t)tail_product(m, plan, w.h1.A(), m->w2, w.h2.rows, 1024, N, 1024, e2, s));
      CK((hipError_t)tail_product(m, plan, w.h2.A(), m->wdec, w.xs.rows, kState, N, kState, e3, s));
    }
  }
  const SmplConsts sc = smpl_consts(m);
  const float* xs = w.xs.rows;
  CK((hipError_t)smpl_chain(
      m, plan, sc, w, N, verts, s,
      [&] { return launch_smpl_small(sc, 0, xs, kState, xs + kNPose, kState, xs + 154, kState, N, w.amat, w.posed, rotmat, theta, verts, s); },
      [&](half_t* ph, half_t* pl, long kst) { return launch_smpl_prep(sc, xs, N, w.pf.rows, w.amat, w.posed, rotmat, theta, s, ph, pl, kst); }));
  const JregPacked jr = jreg_packed ? jreg_view(jreg_packed) : JregPacked{};
  CK(launch_smpl_joints(sc, jreg_packed ? &jr : nullptr, verts, w.posed, xs, N, kp_3d, kp_2d, s));
  return 0;
}

// A forward's workspace as [shared scratch | feature] (state.h forward_layout) on its base
struct FwdWs { void* rest; size_t rest_bytes; float* feat; };
FwdWs split_workspace(void* workspace, size_t ws_bytes, int B) {
  const FwdLayout o = forward_layout(ws_bytes, B);
  return FwdWs{workspace, o.scratch_bytes, (float*)workspace + o.feat};
}

int forward_cached_impl(const tepose_model* m, const KernelPlan& plan, const float* ring_base, int ring, int first_slot, long clip_stride,
                        const float* newest, long newest_ld, int B, int T, const void* jreg_packed, float* theta, float* verts, float* kp_3d,
                        float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes, void* stream, bool sync_zeroed) {
  if (m->kind != 0 || !ring_base || !newest || !workspace || ring < T - 1 || ring < 1 || first_slot < 0 || first_slot >= ring)
    return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  { const int rc = forward_begin(m, workspace); if (rc) return rc; }
  if (ws_bytes < tepose_workspace_bytes(m, B, T)) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const auto [rest, rest_bytes, feat] = split_workspace(workspace, ws_bytes, B);
  EncWs w;
  if (!carve_encoder(m, plan, B, T, rest, rest_bytes, w)) return TEPOSE_E_WORKSPACE;
  const int ld0 = 9 * m->Hp;
  G0Src src{ring_base, ld0, clip_stride, first_slot, ring, newest, newest_ld, newest + 6 * m->Hp, newest_ld};
  float* xs = plan.tail_collapsed ? feat : nullptr;
  int rc = encoder_core(m, plan, src, B, T, 0, feat, w, s, nullptr, sync_zeroed, xs);
  if (rc) return rc;
  return regressor_impl(m, plan, feat, B, 3, nullptr, nullptr, nullptr, jreg_packed, theta, verts, kp_3d, kp_2d, rotmat, rest,
                        rest_bytes, stream, false, true, xs);    // (encoder_core cleared the shared sync region)
}

}  // namespace

extern "C" {

size_t tepose_workspace_bytes(const tepose_model* m, int B, int T) {
  if (!m || B < 1 || T < 1) return 0;
  return forward_bytes(enc_shape(m, select_kernels(m, B, T), B, T), reg_shape(m, select_kernels(m, 2 * B, T), 2 * B));
}

size_t tepose_project_frames_workspace_bytes(const tepose_model* m, int B) {
  if (!m || B < 1) return 0;
  return carve_projection(nullptr, B, select_kernels(m, B, 1, true).h3).bytes;
}

size_t tepose_vibe_workspace_bytes(const tepose_model* m, int B, int N) {
  if (!m || m->kind != 1 || B < 1 || N < 1) return 0;
  Carve c;
  carve_vibe((size_t)B * N, m->vibe_bidir ? 2 : 1, (size_t)m->Hp, c);
  return c.cur + 256;
}

int tepose_vibe_encoder_fwd(const tepose_model* m, const float* x, int B, int N, int use_residual, float* feat,
                            void* workspace, size_t ws_bytes, void* stream) {
  if (!m || m->kind != 1 || !x || !feat || !workspace || B < 1 || N < 1) return TEPOSE_E_ARG;
  if (!m->vibe_packed) return TEPOSE_E_STATE;
  if (ws_bytes < tepose_vibe_workspace_bytes(m, B, N)) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int L = m->L, Hp = m->Hp, H3 = 3 * Hp, D = m->vibe_bidir ? 2 : 1;
  const long BN = (long)B * N;
  Carver c(workspace, ws_bytes);
  const VibeLayout o = carve_vibe((size_t)BN, (size_t)D, (size_t)Hp, c);
  float* G = c.at(o.G);
  float* S[2] = {c.at(o.S[0]), c.at(o.S[1])};
  const float* Bl = m->blob;
  // everything is batch-major (row = b*N + t), like the caller's [B,N,2048]: time steps are a
  // column offset t*ld with row stride N*ld, so no permute (vibe.py:53,62) is ever materialised; a layer's
  // output row is [forward Hp | backward Hp], the backward direction walking t = N-1 .. 0
  const float* in = x;
  int ldin = kFeat;
  for (int l = 0; l < L; ++l) {
    const Weight& ih = m->vibe[l].ih;
    CK(launch_gemm(f32_args(Bl, AOperand{in, ldin}, ih, G, (long)D * H3, (int)BN, D * H3, Epilogue{w_bias(Bl, ih)}), s, m->opt));
    float* So = S[l & 1];
    for (int t = 0; t < N; ++t) {
      GruArgs a{};
      a.M = B; a.Hp = Hp; a.first = t == 0; a.ndir = D;
      for (int d = 0; d < D; ++d) {
        const int td = d ? N - 1 - t : t, tp = d ? td + 1 : td - 1;
        GruDir& q = a.d[d];
        const WView hh(m->vibe[l].hh, d * H3);      // direction d of the stacked rows
        q.Whh = w_rows(Bl, hh); q.bhh = w_bias(Bl, hh);
        q.gi = G + (long)td * D * H3 + (long)d * H3; q.ldgi = (long)N * D * H3;
        q.hprev = So + (long)tp * D * Hp + (long)d * Hp; q.ldh = (long)N * D * Hp;
        q.hout = So + (long)td * D * Hp + (long)d * Hp; q.ldo = (long)N * D * Hp;
      }
      CK(launch_gru_step(a, s, m->opt));
    }
    in = So; ldin = D * Hp;
  }
  if (!m->vibe_linear)                                        // y = gru(x) (+ x when it is 2048 wide, vibe.py:55-61)
    return (int)launch_copy_cols(in, ldin, (use_residual && m->H == kFeat) ? x : nullptr, kFeat, feat, m->H, BN, m->H, s);
  Epilogue e{w_bias(Bl, m->vlin)};
  e.relu_a = 1;
  if (use_residual) { e.addend = x; e.ldadd = kFeat; }
  CK(launch_gemm(f32_args(Bl, AOperand{in, ldin}, m->vlin, feat, kFeat, (int)BN, kFeat, e), s, m->opt));
  return 0;
}

int tepose_smpl_fwd(const tepose_model* m, int pose2rot, const float* pose, const float* betas, int N, float* verts,
                    float* joints49, void* workspace, size_t ws_bytes, void* stream) {
  if (!m || !pose || !betas || !verts || !workspace || N < 1) return TEPOSE_E_ARG;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  const KernelPlan plan = select_kernels(m, N, 1);
  RegWs w;
  if (!carve_regressor(m, plan, N, workspace, ws_bytes, w)) return TEPOSE_E_WORKSPACE;
  SmplConsts sc = smpl_consts(m);
  const int mode = pose2rot ? 1 : 2, pose_ld = pose2rot ? 72 : 216;
  CK((hipError_t)smpl_chain(
      m, plan, sc, w, N, verts, s,
      [&] { return launch_smpl_small(sc, mode, pose, pose_ld, betas, 10, nullptr, 0, N, w.amat, w.posed, nullptr, nullptr, verts, s); },
      [&](half_t* ph, half_t* pl, long kst) { return launch_smpl_prep_pose(sc, mode, pose, pose_ld, betas, 10, N, w.pf.rows, w.amat, w.posed, s, ph, pl, kst); }));
  if (joints49) CK(launch_smpl_joints(sc, nullptr, verts, w.posed, nullptr, N, joints49, nullptr, s));
  return 0;
}

// ---- SMPL backward (smpl_bwd.hip): the forward's buffers (recomputed) and behind them the backward's own (shapes.h
// smpl_bwd_floats), carved by state.h's carve_smpl_bwd for the size query and the entry point
struct SmplBwdWs { float *gsrc, *gvp, *skin_part, *blend_part, *gf; };
// the plan of the recompute: the forward's for N persons, except that the one-launch small-N kernel (which never writes v_posed) gives way to the
// general chain on the exact-fp32 product, the arithmetic of that kernel
static KernelPlan smpl_bwd_plan(const tepose_model* m, int N) {
  KernelPlan k = select_kernels(m, N, 1);
  if (k.smpl == Smpl::small) k.smpl = N <= gemm_skinny_max_m(m->opt) ? Smpl::f32_skinny : Smpl::f32;
  return k;
}

size_t tepose_smpl_bwd_workspace_bytes(const tepose_model* m, int N) {
  if (!m || N < 1 || N > kSmplBwdMaxN) return 0;
  Carve c;
  carve_smpl_bwd(reg_shape(m, smpl_bwd_plan(m, N), N), c);
  return c.cur + 256;
}

int tepose_smpl_bwd(const tepose_model* m, int pose2rot, const float* pose, const float* betas, int N, const float* g_verts,
                    const float* g_joints49, float* g_pose, float* g_betas, void* workspace, size_t ws_bytes, void* stream) {
  if (!m || !pose || !betas || !workspace) return TEPOSE_E_ARG;
  if (!g_verts && !g_joints49 && (g_pose || g_betas)) return TEPOSE_E_ARG;
  if (N < 1 || N > kSmplBwdMaxN) return TEPOSE_E_SHAPE;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  const KernelPlan plan = smpl_bwd_plan(m, N);
  Carver c(workspace, ws_bytes);
  const SmplBwdLayout o = carve_smpl_bwd(reg_shape(m, plan, N), c);
  if (c.cur > ws_bytes) return TEPOSE_E_WORKSPACE;
  RegWs w;
  bind_regressor(o.fwd, workspace, w);
  const SmplBwdWs b{c.at(o.gsrc), c.at(o.gvp), c.at(o.skin_part), c.at(o.blend_part), c.at(o.gf)};
  if (!g_pose && !g_betas) return 0;            // nothing asked for
  SmplConsts sc = smpl_consts(m);
  const int mode = pose2rot ? 1 : 2, pose_ld = pose2rot ? 72 : 216;
  // forward values again: transforms, pose features, v_posed
  CK(launch_smpl_prep_pose(sc, mode, pose, pose_ld, betas, 10, N, w.pf.rows, w.amat, w.posed, s, w.pf.P.hi, w.pf.P.lo, w.pf.P.kst));
  CK((hipError_t)blend_shapes(m, plan, w, N, s));
  // backward, stage by stage
  CK(launch_smpl_joints_bwd(g_joints49, N, b.gsrc, s));
  CK(launch_smpl_skin_bwd(sc, w.vposed, w.amat, g_verts, b.gsrc, N, b.gvp, b.skin_part, s));
  CK(launch_smpl_blend_bwd(sc.blendW, b.gvp, N, b.blend_part, b.gf, s));
  CK(launch_smpl_chain_bwd(sc, mode, pose, betas, N, b.skin_part, b.gsrc, b.gf, g_pose, g_betas, s));
  return 0;
}

// evaluate.py:289-291 (the --filter branch): the H36M regressor applied to given vertices, 14 LSP joints per person
int tepose_joints_from_verts(const tepose_model* m, const void* jreg_packed, const float* verts, int N, float* kp_3d, void* stream) {
  if (!m || !jreg_packed || !verts || !kp_3d || N < 1) return TEPOSE_E_ARG;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  SmplConsts sc = smpl_consts(m);
  const JregPacked jr = jreg_view(jreg_packed);
  CK(launch_smpl_joints(sc, &jr, verts, nullptr, nullptr, N, kp_3d, nullptr, (hipStream_t)stream));
  return 0;
}

int tepose_smpl_fwd_per_person(const tepose_model* m, const float* pose, const float* betas, int N, float* verts,
                               void* workspace, size_t ws_bytes, void* stream) {
  if (!m || !pose || !betas || !verts || !workspace || N < 1) return TEPOSE_E_ARG;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  RegWs w;
  if (!carve_regressor(m, select_kernels(m, N, 1), N, workspace, ws_bytes, w)) return TEPOSE_E_WORKSPACE;
  SmplConsts sc = smpl_consts(m);
  CK(launch_smpl_prep_pose(sc, 1, pose, 72, betas, 10, N, w.pf.rows, w.amat, w.posed, s));
  CK(launch_smpl_person(sc, w.pf.rows, w.amat, N, verts, s));
  return 0;
}

int tepose_smpl_verts_from_theta(const tepose_model* m, const float* theta, int N, float* verts, void* workspace,
                                 size_t ws_bytes, void* stream) {
  if (!m || !theta || !verts || !workspace || N < 1) return TEPOSE_E_ARG;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  hipStream_t s = (hipStream_t)stream;
  const KernelPlan plan = select_kernels(m, N, 1);
  RegWs w;
  if (!carve_regressor(m, plan, N, workspace, ws_bytes, w)) return TEPOSE_E_WORKSPACE;
  SmplConsts sc = smpl_consts(m);
  return smpl_chain(
      m, plan, sc, w, N, verts, s,
      [&] { return launch_smpl_small(sc, 1, theta + 3, kTheta, theta + 75, kTheta, nullptr, 0, N, w.amat, nullptr, nullptr, nullptr, verts, s); },
      [&](half_t* ph, half_t* pl, long kst) { return launch_smpl_prep_pose(sc, 1, theta + 3, kTheta, theta + 75, kTheta, N, w.pf.rows, w.amat, nullptr, s, ph, pl, kst); });
}

int tepose_encoder_fwd(const tepose_model* m, const float* x, int B, int T, int is_train, float* feat,
                       void* workspace, size_t ws_bytes, void* stream) {
  if (m) { const int rc = forward_begin(m, workspace); if (rc) return rc; }   // an earlier forward on this handle gave up: say so before more work is queued
  if (!m || B < 1 || T < 1) return TEPOSE_E_ARG;
  return encoder_fwd_impl(m, select_kernels(m, B, T), x, B, T, is_train, feat, workspace, ws_bytes, stream, nullptr, nullptr, nullptr);
}

// One stage of the forward tepose_encoder_fwd(m, x, B, T, ...) left in `workspace`, as plain fp32 (tap.h says which stages survive a forward and where
// they lie): the plan and the carve are the forward's, one gather kernel is the only launch, nothing is written into the workspace.
int tepose_encoder_tap(const tepose_model* m, int B, int T, int stage, int layer, int dir, int step, float* out, size_t out_floats, int* form,
                       const void* workspace, size_t ws_bytes, void* stream) {
  if (!m || m->kind != 0 || !out || !workspace || B < 1 || T < 1 || stage < kTapGi || stage > kTapTail) return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  if ((size_t)B * T > (1u << 30) / 4) return TEPOSE_E_SHAPE;
  const KernelPlan plan = select_kernels(m, B, T);
  Carver c(const_cast<void*>(workspace), ws_bytes);
  EncWs w;
  carve_encoder(m, plan, B, T, c, w);
  const TapPlan tp{m->L, m->Hp, B, T, plan.h3, plan.g0blk, plan.step0 == Step::s16_planes, plan.step1 == Step::s16_planes};
  TapView v;
  if (!tap_resolve(w.o, tp, stage, layer, dir, step, &v) || out_floats != v.count()) return TEPOSE_E_SHAPE;
  if (c.cur > ws_bytes) return TEPOSE_E_WORKSPACE;
  if (form) *form = v.form;
  CK(launch_tap_gather(v, (const float*)workspace, out, (hipStream_t)stream));
  return 0;
}

// One stage of the decoder half -- the regressor's state row and FC activations, the pose features in each form the plan keeps, the skinning transforms,
// the posed joints, v_posed -- as the finished tepose_regressor_fwd[_init] / tepose_smpl_fwd (entry 0: N rows, T ignored) or tepose_forward (entry 1:
// N = B windows of T frames) left it in `workspace`.  Plan and carve are that call's; one gather kernel is the only launch.  What h1 / h2 / xs hold
// depends on the call (n_iter, a collapsed product writes no h1 / h2): the caller's knowledge.
int tepose_decoder_tap(const tepose_model* m, int N, int stage, float* out, size_t out_floats, int* form, int entry, int T, const void* workspace,
                       size_t ws_bytes, void* stream) {
  if (!m || !out || !workspace || N < 1 || stage < 0 || stage >= kDecStages || entry < 0 || entry > 1 || (entry == 1 && T < 1)) return TEPOSE_E_ARG;
  if (!m->smpl_packed) return TEPOSE_E_STATE;
  const KernelPlan plan = select_kernels(m, N, entry ? T : 1);
  const FwdLayout f = forward_layout(ws_bytes, N);
  Carve c;
  // (tepose_forward carves its regressor from the workspace base, too: the feature slot is cut off the END)
  const RegLayout w = carve_regressor(reg_shape(m, plan, N), c);
  const bool fits = c.cur <= (entry ? f.scratch_bytes : ws_bytes) && (!entry || ws_bytes >= tepose_workspace_bytes(m, N, T));
  const DecPlan d{plan.smpl == Smpl::small, plan.h3 && plan.reg == Reg::seq, entry && plan.tail_collapsed ? f.feat : w.xs.rows};
  TapView v;
  if (!tap_decoder(w, d, stage, N, &v) || out_floats != v.count()) return TEPOSE_E_SHAPE;
  if (!fits) return TEPOSE_E_WORKSPACE;
  if (form) *form = v.form;
  CK(launch_tap_gather(v, (const float*)workspace, out, (hipStream_t)stream));
  return 0;
}

int tepose_project_frames(const tepose_model* m, const float* feat, long feat_ld, const float* theta, long theta_ld,
                          int B, float* out, long out_ld, void* workspace, size_t ws_bytes, void* stream) {
  if (!m || m->kind != 0 || !feat || !out || !workspace || B < 1) return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  if (ws_bytes < tepose_project_frames_workspace_bytes(m, B)) return TEPOSE_E_WORKSPACE;
  return project_frames_impl(m, select_kernels(m, B, 1, true), feat, feat_ld, theta, theta_ld, B, out, out_ld, workspace, (hipStream_t)stream);
}

int tepose_project_frame_pair(const tepose_model* m, const float* feat_prev, const float* feat_new, long feat_ld, const float* theta_prev,
                              long theta_ld, int B, float* out_prev, long out_prev_ld, float* out_new, long out_new_ld, void* workspace,
                              size_t ws_bytes, void* stream) {
  if (!m || m->kind != 0 || B < 1) return TEPOSE_E_ARG;
  return project_frame_pair_impl(m, select_kernels(m, B, 1, true), feat_prev, feat_new, feat_ld, theta_prev, theta_ld, B, out_prev, out_prev_ld,
                                 out_new, out_new_ld, workspace, ws_bytes, stream, nullptr, 0, nullptr);
}

// One iteration of the reference's window loop (evaluate.py:247-269, demo.py:238-252) for B clips in lock-step, as ONE call: both layer-0 projections of
// the step (tepose_project_frame_pair: the previous newest frame with its now-known theta -> its ring slot `out_prev`, the newest frame with zero theta ->
// `newest`) and then TePose.forward of the window from the cached projections (tepose_forward_cached).  Same results as the two calls; the forward's
// sync region is cleared by the projection's input-split kernel instead of a memset node of its own, and a host loop makes one call per step.
int tepose_window_step(const tepose_model* m, const float* feat_prev, const float* feat_new, long feat_ld, const float* theta_prev, long theta_ld,
                       float* out_prev, long out_prev_ld, float* newest, long newest_ld, const float* ring_base, int ring, int first_slot,
                       long clip_stride, int B, int T, const void* jreg_packed, float* theta, float* verts, float* kp_3d, float* kp_2d, float* rotmat,
                       void* workspace, size_t ws_bytes, void* pair_workspace, size_t pair_ws_bytes, void* stream) {
  if (!m || m->kind != 0 || !workspace || B < 1 || T < 1) return TEPOSE_E_ARG;
  if (!m->enc_packed) return TEPOSE_E_STATE;
  { const int rc = forward_begin(m, workspace); if (rc) return rc; }
  if (ws_bytes < tepose_workspace_bytes(m, B, T)) return TEPOSE_E_WORKSPACE;
  const KernelPlan plan = select_kernels(m, B, T, true);
  // the forward's sync region: the first carve of its workspace (as tepose_forward_cached lays it out)
  void* zero = nullptr;
  size_t zero_bytes = 0;
  {
    const size_t rest_bytes = split_workspace(workspace, ws_bytes, B).rest_bytes;
    EncWs w;
    if (!carve_encoder(m, plan, B, T, workspace, rest_bytes, w)) return TEPOSE_E_WORKSPACE;
    if (w.sync) { zero = (void*)w.sync; zero_bytes = sync_zero_bytes(m, plan); }
  }
  bool zeroed = false;
  int rc = project_frame_pair_impl(m, plan, feat_prev, feat_new, feat_ld, theta_prev, theta_ld, B, out_prev, out_prev_ld, newest, newest_ld,
                                   pair_workspace, pair_ws_bytes, stream, zero, zero_bytes, &zeroed);
  if (rc) return rc;
  return forward_cached_impl(m, plan, ring_base, ring, first_slot, clip_stride, newest, newest_ld, B, T, jreg_packed, theta, verts, kp_3d, kp_2d,
                             rotmat, workspace, ws_bytes, stream, zeroed);
}

int tepose_forward_cached(const tepose_model* m, const float* ring_base, int ring, int first_slot, long clip_stride,
                          const float* newest, long newest_ld, int B, int T, const void* jreg_packed, float* theta,
                          float* verts, float* kp_3d, float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes,
                          void* stream) {
  if (!m || B < 1 || T < 1) return TEPOSE_E_ARG;
  return forward_cached_impl(m, select_kernels(m, B, T, true), ring_base, ring, first_slot, clip_stride, newest, newest_ld, B, T, jreg_packed, theta,
                             verts, kp_3d, kp_2d, rotmat, workspace, ws_bytes, stream, false);
}

int tepose_regressor_fwd(const tepose_model* m, const float* feat, int N, int n_iter, const void* jreg_packed,
                         float* theta, float* verts, float* kp_3d, float* kp_2d, float* rotmat,
                         void* workspace, size_t ws_bytes, void* stream) {
  return tepose_regressor_fwd_init(m, feat, N, n_iter, nullptr, nullptr, nullptr, jreg_packed, theta, verts, kp_3d, kp_2d,
                                   rotmat, workspace, ws_bytes, stream);
}

int tepose_regressor_fwd_init(const tepose_model* m, const float* feat, int N, int n_iter, const float* init_pose,
                              const float* init_shape, const float* init_cam, const void* jreg_packed, float* theta,
                              float* verts, float* kp_3d, float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes,
                              void* stream) {
  if (m) { const int rc = forward_begin(m, workspace); if (rc) return rc; }
  if (!m || N < 1) return TEPOSE_E_ARG;
  return regressor_impl(m, select_kernels(m, N, 1), feat, N, n_iter, init_pose, init_shape, init_cam, jreg_packed, theta, verts, kp_3d, kp_2d,
                        rotmat, workspace, ws_bytes, stream, false, false);
}

int tepose_forward(const tepose_model* m, const float* x, int B, int T, const void* jreg_packed, float* theta,
                   float* verts, float* kp_3d, float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes,
                   void* stream) {
  if (!m || !workspace || B < 1 || T < 1) return TEPOSE_E_ARG;
  { const int rc = forward_begin(m, workspace); if (rc) return rc; }
  if (ws_bytes < tepose_workspace_bytes(m, B, T)) return TEPOSE_E_WORKSPACE;
  const KernelPlan plan = select_kernels(m, B, T);
  const auto [rest, rest_bytes, feat] = split_workspace(workspace, ws_bytes, B);
  // the regressor's first A operand (planes of the feature) is written by the encoder's tail product
  RegWs rw;
  (void)carve_regressor(m, plan, B, rest, rest_bytes, rw);
  if (!rw.sync) return TEPOSE_E_WORKSPACE;
  // every arrival counter (and, for B <= 4, every granule) of this forward is cleared by its first kernel (the input
  // split), or by one memset node where that kernel does not run
  bool wrote = false;
  // tail_collapsed: the tail linears and the regressor's three iterations are one product on the relu(final states): the state rows land in
  // the (otherwise unused) feature buffer, and no feature planes are wanted
  float* xs = plan.tail_collapsed ? feat : nullptr;
  int rc = encoder_fwd_impl(m, plan, x, B, T, 0, feat, rest, rest_bytes, stream, plan.h3 && !xs ? &rw.feat.P : nullptr, &wrote, xs);
  if (rc) return rc;
  return regressor_impl(m, plan, feat, B, 3, nullptr, nullptr, nullptr, jreg_packed, theta, verts, kp_3d, kp_2d, rotmat, rest,
                        rest_bytes, stream, wrote, true, xs);
}

}  // extern "C"
