// Internal declarations shared by the HIP translation units of libtepose_hip.so.
// gfx950 (MI355X, CDNA4) only: 64-wide wavefronts, fp32-input MFMA, LDS-DMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "formats.h"   // the plane / blocked-scratch index functions and the row widths: HIP-free, shared with the host check of state.h
#include "shapes.h"    // options.h (struct Options) and the launch-shape rules: HIP-free, checked on the host by tests/test_launch_shapes.py

namespace tepose {

typedef _Float16 half_t;
// split-precision operands: a = hi + lo / kLoScale with hi = fp16(a), lo = fp16((a - hi) * kLoScale); the power-of-two
// scale keeps the low half out of the fp16 subnormal range for every |a| >= ~1e-7 (22 significant bits)
constexpr float kLoScale = 2048.f;
__host__ __device__ inline void split_hi_lo(float a, half_t& hi, half_t& lo) {
  hi = (half_t)a;
  lo = (half_t)((a - (float)hi) * kLoScale);
}
// the scaled format of gemm_h3s.hip (the caller has multiplied by the matrix's or row's power-of-two scale): lo = fp16(v - hi), no 2^11 factor
__host__ __device__ inline void split_hi_lo16(float v, half_t& hi, half_t& lo) {
  hi = (half_t)v;
  lo = (half_t)(v - (float)hi);
}

// ---------------------------------------------------------------- launch shapes
// The per-handle Options (their name table and the environment's view included) live in options.h; the plan's shape predicates (split_rows_few_ok,
// gru_first16_shape_ok, gru_seq_shape_ok, gru_seq_ok, gemm_skinny_max_m) and every rule that turns a shape into a kernel instantiation, grid and
// block in shapes.h -- both plain C++ that the host compiler checks alone.  A launcher launches what shapes.h returned:
inline dim3 grid_of(const Launch& l) { return dim3(l.gx, l.gy, l.gz); }
inline dim3 block_of(const Launch& l) { return dim3(l.threads); }

// ---------------------------------------------------------------- GEMM (gemm.hip)
// C[M,N] = epi( A[M,Kp] * W[Np,Kp]^T ), fp32 operands, fp32 MFMA accumulate.
struct GemmArgs {
  const float* A; long lda;      // rows 16-byte aligned, K zero-padded to Kp by the producer
  const float* W; int Kp;        // packed [Np][Kp], Np multiple of 128, Kp multiple of 32
  float* C; long ldc;
  const float* bias;             // [N] or nullptr
  const float* addend; long ldadd;  // [M,N] or nullptr
  float scale;                   // applied last
  int M, N;
  int relu_a;                    // apply max(0,.) to A on the fly
};
// launch_gemm: width-first kernel (skinny.hip) up to gemm_skinny_max_m rows, else launch_gemm_tiles (gemm_f32_kernel)
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s, const Options& o);
hipError_t launch_gemm_tiles(const GemmArgs& a, hipStream_t s, const Options& o);

// One GRU cell step for up to 3 independent directions in one launch:
//   gh = hprev * Whh^T ; r,z,n gate math ; hout = (1-z)*n + z*hprev      (torch.nn.GRU)
struct GruDir {
  const float* hprev; long ldh;  // [M][Hp]; ignored when first
  const float* Whh;              // packed, gate-interleaved tiles (see pack_whh_kernel)
  const float* bhh;              // [3*Hp], natural order g*Hp + j
  const float* gi; long ldgi;    // gi[row*ldgi + g*Hp + j] = x W_ih^T + b_ih
  float* hout; long ldo;
  long gi_blk = 0;               // != 0: gi is in the 16 x 16-blocked layout (formats.h gi_blk_offset), floats between 16-row tiles
  // != nullptr: the fp32 previous / new state in the same 16 x 16 blocks (formats.h st_blk_offset; base of the view's first row tile, floats between row tiles);
  // hprev / hout stay the row-major addresses
  const float* hprev_b = nullptr; long hp_blk = 0;
  float* hout_b = nullptr; long ho_blk = 0;
};
struct GruArgs {
  GruDir d[3];
  int ndir;
  int M, Hp;
  int first;                     // h_{-1} = 0: skip the matmul
};
// launch_gru_step: width-first kernel (skinny.hip) up to Options::skinny_max_m rows, else launch_gru_step_tiles (gru_step_kernel)
hipError_t launch_gru_step(const GruArgs& a, hipStream_t s, const Options& o);
hipError_t launch_gru_step_tiles(const GruArgs& a, hipStream_t s);
// small-M variants (skinny.hip)
hipError_t launch_skinny_gemm(const GemmArgs& a, hipStream_t s);
hipError_t launch_skinny_gru(const GruArgs& a, hipStream_t s);

// ---------------------------------------------------------------- misc.hip
// dst[np][kp] (row-major [Np][Kp]) = src[rowmap(np)][colmap(kp)] or 0.
enum RowMap { ROW_PLAIN = 0, ROW_GATES = 1, ROW_GATES_TILED = 2 };
enum ColMap { COL_PLAIN = 0, COL_SPLIT2 = 1 };
struct PackArgs {
  const float* src; long ld_src; int N, K;   // logical source [N][K] (col offset folded into src)
  float* dst; int Np, Kp;                     // fp32 destination
  int rowmap, colmap;
  int H, Hp;                                  // for the gate / split maps
};
hipError_t launch_pack(const PackArgs& a, hipStream_t s);
hipError_t launch_pad_input(const float* x, float* xp, long rows, hipStream_t s);
hipError_t launch_pad_rows(const float* feat, long feat_ld, const float* theta, long theta_ld, float* xp,
                           long rows, hipStream_t s);
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s);
hipError_t launch_dmm(const void* A, int a64, long lda, const void* B, int b64, long ldb, const double* Cadd, long ldadd,
                      const float* Cadd32, long ldadd32, double* C, long ldc, int M, int N, int K, double alpha,
                      int add_identity, hipStream_t s);
hipError_t launch_d2f_pad(const double* src, long ld, int rows, int cols, float* dst, int Rp, int Cp, hipStream_t s);
hipError_t launch_copy_cols(const float* src, long lds, const float* add, long lda, float* dst, long ldd, long rows,
                            int cols, hipStream_t s);
struct TapView;      // tap.h
hipError_t launch_tap_gather(const TapView& v, const float* ws, float* out, hipStream_t s);      // one stage of a finished forward -> [slabs][rows][cols] fp32
hipError_t launch_init_state(const float* init160, float* xs, int N, hipStream_t s);
hipError_t launch_init_state_rows(const float* init160, const float* pose, const float* shape, const float* cam,
                                  float* xs, int N, hipStream_t s);
hipError_t launch_rotmat_to_aa(const float* R, int N, float* aa, hipStream_t s);
hipError_t launch_rot6d_to_rotmat(const float* x6, int N, float* R, hipStream_t s);

// ---------------------------------------------------------------- smpl.hip
struct SmplConsts {              // device pointers into the packed blob
  const float* J0;               // [24][3]      J_regressor * v_template
  const float* JS;               // [24][3][10]  J_regressor * shapedirs
  const float* blendW;           // [kBlendN][kBlendK]  rows (v,c): [v_template | shapedirs | posedirs^T]
  const float* lbsW;             // [6890][24]
  const int* lbs_cidx;           // [6890][4] compacted skin weights (joint index)
  const float* lbs_cval;         // [6890][4]
  int lbs_sparse;                // 1: every vertex has <= 4 non-zero weights -> compact kernel
  const int* parents;            // [24]
  const int* depth;              // [24]
  int maxdepth;                  // deepest level of the tree (host-computed)
  const int* xr_ptr;             // CSR of J_regressor_extra: [10]
  const int* xr_idx;             // [nnz]
  const float* xr_val;
};
struct JregPacked {              // CSR of the optional 17-row evaluation regressor
  const int* ptr; const int* idx; const float* val;
};
// pf_hi / pf_lo: optionally also write the pose-feature rows as blocked planes (view base, pf_kst halfs between 32-column groups)
hipError_t launch_smpl_prep(const SmplConsts& c, const float* xs, int N, float* pf, float* Amat,
                            float* posed, float* rotmat, float* theta, hipStream_t s, void* pf_hi = nullptr,
                            void* pf_lo = nullptr, long pf_kst = 0);
hipError_t launch_smpl_prep_pose(const SmplConsts& c, int mode, const float* pose, int pose_ld,
                                 const float* betas, int betas_ld, int N, float* pf, float* Amat, float* posed,
                                 hipStream_t s, void* pf_hi = nullptr, void* pf_lo = nullptr, long pf_kst = 0);
// measurement only: blend shapes + skinning as one wave per person
bool smpl_small_rows_ok(int N, const Options& o);        // persons the one-launch kernel takes (it also needs <= 4 skin weights per vertex)
hipError_t launch_smpl_small(const SmplConsts& c, int mode, const float* pose, int pose_ld, const float* betas, int betas_ld,
                             const float* cam, int cam_ld, int N, float* Amat, float* posed, float* rotmat, float* theta,
                             float* verts, hipStream_t s);
hipError_t launch_smpl_person(const SmplConsts& c, const float* pf, const float* Amat, int N, float* verts, hipStream_t s);
hipError_t launch_lbs_compact(const float* lbsW, int* cidx, float* cval, int* max_nnz, hipStream_t s);
hipError_t launch_smpl_skin(const SmplConsts& c, const float* vposed, const float* Amat, int N,
                            float* verts, hipStream_t s);
hipError_t launch_smpl_joints(const SmplConsts& c, const JregPacked* jr, const float* verts,
                              const float* posed, const float* xs, int N, float* kp3d,
                              float* kp2d, hipStream_t s);
// CSR build (device): counts then fill, rows x cols dense -> ptr/idx/val
hipError_t launch_csr_build(const float* dense, int rows, int cols, int* ptr, int* idx, float* val,
                            int cap, hipStream_t s);
hipError_t launch_smpl_consts(const float* v_template, const float* shapedirs, const float* posedirs,
                              const float* J_regressor, float* J0, float* JS, float* blendW,
                              hipStream_t s);

// ---------------------------------------------------------------- smpl_bwd.hip (launch shapes and buffer sizes: shapes.h)
// g_j49 [N,49,3] or nullptr (zeros) -> gsrc [N][54][3]: the gradients of the 24 posed joints, the 21 picked vertices and the 9 regressed rows
hipError_t launch_smpl_joints_bwd(const float* g_j49, int N, float* gsrc, hipStream_t s);
// g_verts [N,6890,3] or nullptr (zeros), gsrc -> gvp [N][kVertLd] (g_vposed) and partial [N][kBwdSkinBlocks][24][12] (g_A per workgroup)
hipError_t launch_smpl_skin_bwd(const SmplConsts& c, const float* vposed, const float* Amat, const float* g_verts, const float* gsrc, int N,
                                float* gvp, float* partial, hipStream_t s);
// gvp -> part [splits][N][224] -> gf [N][224] = g_vposed x blendW (blendW: the exact fp32 table [kBlendN][kBlendK])
hipError_t launch_smpl_blend_bwd(const float* blendW, const float* gvp, int N, float* part, float* gf, hipStream_t s);
// mode 1: pose [N,72] axis-angle, g_pose [N,72]; mode 2: pose [N,24,3,3], g_pose alike.  g_pose / g_betas [N,10] may be nullptr
hipError_t launch_smpl_chain_bwd(const SmplConsts& c, int mode, const float* pose, const float* betas, int N, const float* partial,
                                 const float* gsrc, const float* gf, float* g_pose, float* g_betas, hipStream_t s);

// ---------------------------------------------------------------- metrics.hip
hipError_t launch_metrics_joints(const float* pred, const float* target, int N, int J, int pelvis_mode,
                                 float* mpjpe, float* pa, float* accel, hipStream_t s);
hipError_t launch_metrics_verts(const float* pred, const float* target, int N, float* mpvpe, hipStream_t s);

// ---------------------------------------------------------------- filters.hip
hipError_t launch_one_euro(float* x, int N, int D, float min_cutoff, float beta, float d_cutoff, hipStream_t s);
hipError_t launch_slerp_smooth(const float* in, float* out, int N, int J, double ratio, hipStream_t s);
// the one-euro step of a live session's slots (tepose_session_smooth): the step function is one_euro_kernel's
hipError_t launch_session_smooth(const float* theta, const float* hist, int S, int T, const int* ops, float* state, float* saved, float min_cutoff,
                                 float beta, float d_cutoff, float* theta_hat, float* pose_hat, float* betas_hat, hipStream_t s);

// ---------------------------------------------------------------- gemm_h3.hip (split-precision fp16x3 GEMM)
// (operand planes: K-tile-blocked and slot-swizzled, formats.h plane_index)
struct H3Args {
  const half_t *Ah, *Al; long a_kst;  // A hi / lo planes: pointer to the view's first block, halfs between K-tiles
  const half_t *Wh, *Wl; long w_kst;  // W planes: rows padded to the N-tile, zero beyond N
  int Kp;                             // multiple of 32
  float* C; long ldc;
  const float* bias;                  // [N] or nullptr
  int M, N;
  // optional epilogue extras (zero-initialised when omitted): C = (A W^T + bias + addend) * scale, and the same
  // values written as blocked hi / lo planes (the next product's A operand)
  const float* addend; long ldadd;
  float scale;                        // 0 = no scaling
  half_t *Chi, *Clo; long c_kst;      // view base (row 0, column 0), halfs between 32-column groups
  const float* row_scale;             // optional [M]: the A planes hold row m divided by row_scale[m] (launch_split_rows);
                                      // the product of row m is multiplied back before bias / addend
  // optional row grouping (width-first kernel only): logical row m lives at physical row (m / grp_rows) * grp_stride +
  // m % grp_rows of A and C -- the time slabs of the state buffers are padded to 16 rows, and at B = 1 fifteen of
  // every sixteen rows are padding that a product over the physical rows would stream W against
  int grp_rows, grp_stride;           // 0: identity
  // optional second destination (width-first kernel only; no planes out, no addend): rows >= c_split are written to C2 + (row - c_split) * ldc2 instead --
  // two row groups of ONE product land in two differently strided buffers (the clip driver's cached projections: ring slot + newest-frame row)
  float* C2; long ldc2; int c_split;  // C2 == nullptr: none
};
struct GateDir {
  const float* gi; long ldgi;         // x W_ih^T + b_ih, [row*ldgi + g*Hp + j]
  const float* bhh;                   // [3Hp]
  const float* hprev; long ldh;       // fp32 previous state (unused by the first step)
  float* hout; long ldo;              // fp32 new state
  half_t *hout_hi, *hout_lo; long okst;   // its planes: view base (row % 16 == 0), halfs between 32-column groups
  long gi_blk = 0;                    // as GruDir::gi_blk
  const float* hprev_b = nullptr; long hp_blk = 0;    // as GruDir::hprev_b / hout_b
  float* hout_b = nullptr; long ho_blk = 0;
};
struct H3Batch { H3Args p[3]; GateDir gate[3]; int n; int Hp; };
// up to 3 independent products of the same M, N, Kp in one launch
hipError_t launch_gemm_h3(const H3Batch& b, hipStream_t s, const Options& o);
// recurrent product with the GRU cell update fused into the epilogue: W planes in the gate-interleaved tile
// order (ROW_GATES_TILED), p[d].C unused, gate[d] describes the cell operands / outputs
hipError_t launch_gru_h3(const H3Batch& b, hipStream_t s);
// the same step for small M (skinny_h3.hip): width-first blocks, K split over the waves, operands streamed to VGPRs
hipError_t launch_skinny_gru_h3(const H3Batch& b, hipStream_t s);
hipError_t launch_skinny_gemm_h3(const H3Args& a, hipStream_t s, const Options& o);
struct H3ArgsBatch { H3Args p[3]; int n; };                       // independent products (own M, N, K) in one launch
hipError_t launch_skinny_gemm_h3_batch(const H3ArgsBatch& b, hipStream_t s, const Options& o);
// gru_seq.hip: all T cell steps of one layer (up to 3 directions) in one persistent launch for M <= 64 rows, W_hh
// planes stationary in registers.  Per (direction, step): where the step's gate pre-activations come from and where
// its new state goes (fp32 + the planes view, as GateDir); step t reads the planes step t-1 wrote.
struct GruSeqStep {
  const float* gi; float* hout;          // gi[row*ldgi + g*Hp + j], hout[row*ldo + j]
  int ldgi, ldo;
  unsigned poff, pkst;                   // hout's planes: view base offset inside phi / plo (halfs), halfs between 32-column groups
};
struct GruSeqArgs {
  GruSeqStep st[3][kSeqMaxT];
  const half_t* whi[3]; const half_t* wlo[3]; long w_kst;   // W_hh planes (gate-interleaved tile order), as H3Args
  const float* bhh[3];
  half_t *phi, *plo;                     // state planes (hi / lo) that every poff refers to
  unsigned* counters;                    // 3 x 32 uints, zeroed before the launch: arrivals per direction
  unsigned* status;                      // set to non-zero when a bounded wait gave up (device word, cleared per forward)
  unsigned* fault;                       // the handle's host-visible fault word (pinned host memory, sticky until
                                         // tepose_status reads it) or nullptr: written with system scope on give-up
  unsigned spin_limit;                   // polls before a wait gives up (~1 us each)
  unsigned inject;                       // test knob (TEPOSE_TEST_FAULT): added to what a wait expects, so that it cannot be met
  int ndir, T, M, Hp;
  // optional single cell step from h = 0 of one more direction (the top bi-GRU layer's forward direction consumes only
  // its first step, tepose.py:80), done by direction 0's workgroups before their loop; x_gi == nullptr: none
  const float* x_gi; const float* x_bhh; float* x_hout;
  int x_ldgi, x_ldo;
  unsigned x_poff, x_pkst;
  // optional relu(final state) planes = the A operand of the tail linears: view offsets inside rhi / rlo per
  // direction (and for the extra step), kNoPlane = none; r_kst halfs between 32-column groups
  half_t *rhi, *rlo;
  unsigned r_off[3], x_roff, r_kst;
  unsigned long long* stamps;            // diagnostic builds (-DTEPOSE_SEQ_STAMPS): per-step wall-clock stamps of one workgroup
  // M <= 16: the state travels between workgroups as 8-byte {tag, hi|lo} granules -- the data is the flag (one round trip
  // per step instead of store drain + counter + poll + load).  gran: [3 directions][2 buffers][4 rows][Hp] uint64, zeroed
  // before the forward; a step's tag = tag_base + step + 1 (tag_base separates the layers of one forward).  nullptr: counters.
  unsigned long long* gran;
  unsigned tag_base;
};
constexpr unsigned kNoPlane = 0xffffffffu;
// reg_seq.hip: the regressor's FC loop (fc1 / fc2 / decoders x n_iter) for N <= 64 rows in one persistent launch
struct RegSeqArgs {
  const half_t *fh, *fl; long f_kst;     // feature planes [N x 2048]
  const half_t *w1a_h, *w1a_l, *w1b_h, *w1b_l, *w2_h, *w2_l, *wd_h, *wd_l;   // weight planes ([1024] rows; decoders [256])
  const float *b1, *b2, *bdec;
  const float *init160, *ipose, *ishape, *icam;   // model means [160]; optional per-call rows [N,144] / [N,10] / [N,3]
  half_t *h1h, *h1l, *h2h, *h2l; long h_kst;      // exchange planes [N x 1024]
  half_t *xh, *xl; long x_kst;                    // state planes [N x 160]
  float* xs;                                      // final state [N][160]
  unsigned* counters;                             // 3 x 32 uints, zeroed before the launch
  unsigned* status;
  unsigned* fault; unsigned spin_limit; unsigned inject;      // as GruSeqArgs
  int N, n_iter;
};
hipError_t launch_reg_seq(const RegSeqArgs& a, hipStream_t s);
int device_cus(const Options& o);               // CUs of the current device (Options::assume_cus > 0: that many): the last argument of shapes.h gru_seq_ok
hipError_t launch_gru_seq(const GruSeqArgs& a, hipStream_t s, const Options& o);   // a.gran != nullptr: granule hand-off (M <= kSeqGranRows)
// first cell step of a direction (h = 0: no product), writing the same outputs
struct GateBatch { GateDir d[3]; };
// rows16: the 16-row kernel (gru_first16_kernel; scaled planes, Hp % 128 == 0), unless a view is misaligned for its vector accesses
hipError_t launch_gru_first(const GateBatch& gb, int ndir, int M, int Hp, hipStream_t s, int scaled16 = 0, bool rows16 = false);
// x[rows][2133] fp32 -> blocked hi / lo planes of [rows x 2144]
// (relu?)src[rows][ld] fp32 (K valid columns) -> blocked planes of [R x Kp], rows < R
hipError_t launch_split_planes(const float* src, long ld, long rows, int K, int Kp, long R, void* hi, void* lo,
                               hipStream_t s, int relu = 0);
// Caller-supplied rows (the [.,2133] windows) -> planes with one power-of-two scale per row: row m is stored as
// x[m] * 2^e_m with max|x[m]| * 2^e_m in [2^13, 2^14) (zero / non-finite rows: e = 0), row_scale[m] = 2^-e_m.  Any
// finite fp32 input is representable (no fp16 overflow at |x| >= 65504, no precision loss for tiny features); the
// consuming product multiplies row m's result by row_scale[m].  fmt16: the scaled [K/16][R][16] format of gemm_h3s.hip
// (hi = fp16(v), lo = fp16(v - hi)), else the blocked [K/32][R][32] format (lo = fp16((v - hi) * 2^11)).
// zero / zero_bytes (multiple of 16): the kernel also clears that block -- the forward's arrival counters and granules,
// when this is the forward's first kernel (saves the memset node).
// optional gathered source of launch_split_rows (the clip driver's two per-step projections as one product): row r < B = features f0[r] | theta th0[r],
// row r >= B = features f1[r - B] | zeros -- what two launch_pad_rows calls would have written to a padded buffer first (evaluate.py:248-252)
struct RowPairSrc { const float* f0; const float* th0; const float* f1; long fld, thld; long B; };
// few: one workgroup per row (split_rows_few_kernel, split_rows_few_ok), else 8 rows per workgroup (split_rows_kernel).
hipError_t launch_split_rows(const float* src, long ld, long rows, int K, int Kp, long R, int fmt16, void* hi, void* lo,
                             float* row_scale, hipStream_t s, bool few, void* zero = nullptr, size_t zero_bytes = 0,
                             int permT = 0, const RowPairSrc* pair = nullptr);   // permT = T: source rows [B][T] -> plane rows / row_scale frame-major (t * B + b)
hipError_t launch_gemm_h3_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C,
                              long ldc, int M, int N, int K, void* ws, hipStream_t s, const Options& o, int kind = 0);
size_t gemm_h3_ws_bytes(int M, int N, int K);
// gemm_h3s.hip: single accumulator, 256 x 256 tiles, scaled planes in the [K/16][R][16] layout (formats.h plane16_index)
constexpr float kStateScale = 16384.f;   // scale of recurrent-state planes in that format (|h| < 1)
struct H3SArgs {
  const half_t *Ah, *Al; long a_kst;     // halfs between K-tiles (R * 16)
  const half_t *Wh, *Wl; long w_kst;     // W rows padded to 256
  int Kp;                                // multiple of 16
  float* C; long ldc;
  const float* bias;                     // [N] or nullptr
  float inv_scale;                       // 1 / (pA * pW)
  int M, N;
  const float* row_scale;                // optional [M], as H3Args::row_scale (then pA = 1)
  // barrier-free kernels (gemm_h3s16c.hip): where a wave whose bounded LDS poll expired reports it -- the forward's status word
  // (workspace sync region, agent scope) and the handle's host-visible fault word (system scope); nullptr: debug counter + NaN only
  unsigned* status = nullptr;
  unsigned* fault = nullptr;
  unsigned inject = 0;                   // tests: added to every poll target (1 = no poll can ever be met)
  int c_blk_hp = 0;                      // != 0 (= Hp): C is a [rows][3 Hp] gate pre-activation matrix, written in the blocked layout (gi_blk_offset)
};
struct H3SBatch { H3SArgs p[3]; GateDir gate[3]; int n; int Hp; float state_scale; };   // state_scale: scale of the
hipError_t launch_gemm_h3s(const H3SArgs& a, hipStream_t s, const Options& o, int tag = 1);   // every plain scaled-plane product of large batches (tag 0: the layer-0 projection: own kernel symbol for profiles)
bool gemm_h3s16_ok(const H3SArgs& a);
hipError_t launch_gemm_h3s16c(const H3SArgs& a, hipStream_t s, int tag, int gm, int walk);  // gemm_h3s16c.hip: persistent, no workgroup barriers in the K loop (gm, walk: Options::s16_gm, ::s16_walk)
unsigned h3s16c_read_err();
void h3s16c_warm();                    // allocates the current device's debug error counter (tepose_set_blob: never inside a stream capture)
// gru_step16.hip: the fused GRU cell step of large batches; planes = the instantiation that takes its cell operands through the LDS-DMA stream and
// rebuilds h_{t-1} from the state planes (full tiles + blocked layouts only: gru_step16_planes_ok)
bool gru_step16_ok(const H3SBatch& b);
bool gru_step16_planes_ok(const H3SBatch& b);
hipError_t launch_gru_step16(const H3SBatch& b, hipStream_t s, bool planes, int gm);
unsigned* h3s16c_err_of_device();      // the current device's debug counter of give-ups of the barrier-free kernels (nullptr: none)
bool gemm_h3s_mid_ok(const H3SArgs& a);
hipError_t launch_gemm_h3s_mid(const H3SArgs& a, hipStream_t s);   // 128 x 288 tiles, N % 288 == 0 (shapes.h h3s_mid_cols_ok)
hipError_t launch_split_planes16(const float* src, long ld, long rows, int K, int Kp, long R, float p, void* hi,
                                 void* lo, hipStream_t s);
hipError_t launch_absmax(const float* src, size_t n, float* out, hipStream_t s);
size_t gemm_h3s_ws_bytes(int M, int N, int K);
hipError_t launch_gemm_h3s_f32(const float* A, long lda, const float* W, long ldw, float* C, long ldc, int M, int N,
                               int K, float pA, float pW, void* ws, hipStream_t s, const Options& o, const float* bias = nullptr,
                               int mid = 0);   // mid: the 128 x 288-tile kernel (N % 288 == 0) instead of the barrier-free persistent one

}  // namespace tepose
