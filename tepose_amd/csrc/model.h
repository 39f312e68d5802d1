// The model handle behind the C ABI (include/tepose_amd.h) and what every host file of the library shares: where each
// weight lives in the blob (filled by blob.hip's layout pass), the handle's knobs, the fault channel of the persistent kernels.
#pragma once
#include "../../include/tepose_amd.h"

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace tepose {

// One weight matrix of the blob: everything the layout pass (blob.hip) decided for it, in float offsets from the blob base.  take_w() and plane() there are
// the only code that writes a geometry number; packing, plane derivation, the fp32 section list and every product read them here.
struct Weight {
  size_t w = 0; int Np = 0, Kp = 0;     // packed fp32 [Np][Kp] (0: none -- a matrix that exists as planes only)
  size_t b = 0;                         // bias section (0: none)
  size_t p = 0; int Rp = 0;             // blocked hi | lo fp16 planes [Kp/32][Rp][32] (gemm_h3.hip), lo plane behind the hi plane
  size_t s = 0; int Rs = 0;             // the same as scaled [Kp/16][Rs][16] planes (gemm_h3s.hip) with one power-of-two scale per matrix ...
  size_t scale_at = 0;                  // ... the blob float that holds the scale ...
  float scale = 1.f;                    // ... and the host copy of it (derive_planes / tepose_adopt_blob)
  // what a scaled product multiplies back by: 1 / (scale of the A planes * scale of these)
  float inv_scale(float a_scale = 1.f) const { return 1.f / (a_scale * scale); }
};
enum class Fmt : unsigned char { blocked, scaled };   // which plane section of a Weight
// Rows from row0 and the K range from k0 of a weight: the whole matrix, or a sub-block that is real (the gru_rec forward rows of the stacked layer-0
// block, one direction of a VIBE layer, one half of [W_lf | W_lr]).  Kp and the plane strides stay the record's.
struct WView {
  const Weight* w; int row0, k0;
  WView(const Weight& wt, int r0 = 0, int k = 0) : w(&wt), row0(r0), k0(k) {}
};

struct DirW { Weight ih, hh; };   // one GRU layer/direction (hh: gate-tiled rows; the layer-0 ih of a TePose handle lives in the stacked block wih0)

struct SmplOff {
  size_t J0, JS, lbsW, lbs_cidx, lbs_cval, lbs_nnz, parents, depth, xr_ptr, xr_idx, xr_val;
};

// One derived section of the blob: hi | lo fp16 planes of a packed fp32 matrix that lives in the blob too.  The layout pass enters every one into
// tepose_model::planes as it carves it, so the section's size, its content (derive_planes, the only code that writes a plane section or a scale slot)
// and the complement a rank has to receive (tepose_fp32_ranges) all come from this one list.
enum class Owner : unsigned char { encoder, regressor, smpl, collapsed_regressor, collapsed_tail, backbone };   // whose packing fills the source
struct PlaneSpec {
  Owner owner;
  const Weight* src; int rows;    // source: the first `rows` rows of src's packed fp32 matrix
  Weight* dst; int k0; Fmt fmt;   // section: dst's planes of format fmt (rows beyond `rows` zero); this entry is their K range [k0, k0 + src->Kp)
};

}  // namespace tepose

struct tepose_model {
  int kind = 0;                                 // 0 = TePose, 1 = VIBE bootstrap encoder, 2 = HMR (ResNet-50 backbone + regressor + SMPL)
  // Every tepose::Weight below is filled by the layout pass at handle creation and stays where it is: the vectors are sized once, before the plane
  // table takes pointers to their elements.
  // HMR backbone (hmr.h): per convolution of the layer table, the folded weights [Np][Kp], the folded batch-norm shift [C_out] as bias, their blocked planes
  std::vector<tepose::Weight> bb;
  bool bb_packed = false, bb_range_ok = true;
  std::vector<tepose::DirW> vibe;               // VIBE: per-layer GRU weights, the rows of both directions stacked ([dir][3Hp]): direction d is the
                                                // row view from d * 3Hp
  bool vibe_bidir = false, vibe_linear = true;  // vibe.py:27-47: bidirectional GRU; Linear(D*hidden -> 2048) on relu(y)
  tepose::Weight vlin;
  bool vibe_packed = false;
  int L = 0, H = 0, Hp = 0;
  size_t hdr = 0;                               // blob header (BlobHeader): what the blob holds, checked by tepose_adopt_blob
  float* blob = nullptr;
  size_t blob_floats = 0;
  std::vector<tepose::PlaneSpec> planes;        // every derived section (the layout pass fills it)
  bool enc_packed = false, reg_packed = false, smpl_packed = false;
  // encoder weights
  tepose::Weight wih0;                          // layer-0 input projections, stacked [9Hp][2144]: fwd | rec_reverse | rec
  // kernel-family knobs (named options, read once per handle; defaults = the measured best):
  bool large_scaled = true;                     // TEPOSE_LARGE_BATCH_KERNELS=scaled|twoacc: large batches (layer-0 projection from B * T >= 8192 / mid tiles from 512 rows,
                                                // recurrent path from s_min_b windows) on the scaled-plane single-accumulator kernels (gemm_h3s16c.hip, gru_step16.hip,
                                                // gemm_h3s.hip) -- or, `twoacc`, on the two-accumulator family of gemm_h3.hip at every batch size
  bool state_planes = true;                     // TEPOSE_GRU_STATE=planes|fp32: the large-batch step kernel rebuilds h_{t-1} from the state planes and takes its cell
                                                // operands through the LDS-DMA stream (gru_step16_kernel<true>) -- or, `fp32`, keeps a separate fp32 state copy (<false>)
  std::string kinfo;                            // tepose_kernel_info(): the kernel symbols the knobs select for the dominant launches of cfg-C
  std::vector<tepose::DirW> fwd, rec_f, rec_r;  // per layer
  tepose::Weight wlf, wlr;                      // the tail linears
  tepose::Weight wlfr;                          // [W_lf | W_lr] ([2048][3Hp], planes only): eval mode's (y_fwd + y_rec)/2 as ONE product
  // regressor weights: fc1 split into its feature and state columns (w1a carries b1), fc2, the three decoders stacked; the initial state row
  tepose::Weight w1a, w1b, w2, wdec;
  size_t init = 0;
  tepose::Weight blend;                         // SMPL blend-shape matrix [3 * 6890 padded][224]; scaled planes for large batches (barrier-free persistent kernel)
  // collapsed regressor: the eval-mode FC loop is affine in (feature, initial state), so with the model's own
  // initial state and n_iter = 3 the final state is  xs = feat Mf^T + k0  and, through the (affine) tail linears,
  // xs = [relu(h_fwd) | relu(y_rec0)] Mt^T + kt.  fp64 algebra at pack time; [256][K] fp32 + planes, k0 / kt as their bias rows of 160.
  tepose::Weight mf, mt;
  bool reg_collapsed = false, tail_collapsed = false;
  bool collapse_env = true;                     // TEPOSE_COLLAPSE_REGRESSOR=0: always run the FC loop
  tepose::SmplOff smpl{};
  int maxdepth = 0;
  int lbs_sparse = 0;                           // skin-weight table has <= 4 non-zeros per vertex
  bool split = true;                            // batches of more than m->opt.split_min_m rows run their matmuls on the fp16x3 split kernels
  bool split_env = true;                        // what the environment asked for; `split` also needs every packed weight inside
  bool enc_range_ok = true, reg_range_ok = true, smpl_range_ok = true;   // the fp16 range (|w| < 2^15), checked at pack time
  int s_min_b = 640;                            // scaled-format recurrent path from this batch size
  tepose::Options opt;                          // every launch threshold (options.h Options): from the environment at tepose_create, tepose_set_option before packing
  // fault channel of the persistent kernels (gru_seq.hip, reg_seq.hip): one word of pinned host memory that a kernel
  // whose bounded wait expired writes with system scope; sticky until tepose_status() reads it
  unsigned* fault = nullptr;
  bool persist = true;                          // false: step-per-launch kernels at every batch size (tepose_set_persistent)
  unsigned spin_limit = 1u << 21;               // polls (~1 us each) before a wait gives up
  int blend16_min_n = 512;                      // TEPOSE_BLEND16_MIN_N: rows from which the blend-shape product runs on gemm_h3s_persist16c_kernel (0x7fffffff = never)
  int gi_blk = 1;                               // TEPOSE_GI_BLK: large batches keep the layer >= 1 gate pre-activations in the 16 x 16-blocked layout (common.h gi_blk_offset)
  int last_fault_code = 0;                      // the kernel code of the last fault a status call collected (tepose_fault_code)
  // The fault word is shared by every stream and thread of the handle and ANY status call clears it, so "the word is clear" says nothing about one
  // particular forward once somebody else has collected: `collected` counts the clears that found the word raised, and every forward notes the count
  // it was queued under, per workspace (its status words live there).  tepose_forward_status trusts the clear word only while the count stands still.
  mutable std::mutex q_mu;
  mutable std::unordered_map<const void*, unsigned> q_gen;
  mutable unsigned collected = 0;               // guarded by q_mu
  unsigned test_fault = 0;                      // TEPOSE_TEST_FAULT: bit 0 recurrent kernel, bit 1 regressor kernel wait for arrivals that never come
  // profiling of the dominant kernel (layer-0 input-projection GEMM)
  bool prof = false;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  double prof_flops = 0.0;
  std::vector<hipEvent_t> ev_gru;               // pairs around each layer's sequence of GRU-step launches
  size_t ev_gru_used = 0;
  double prof_gru_flops = 0.0;                  // algorithmic FLOPs of all GRU steps of one forward
  double prof_l1_flops = 0.0;                   // algorithmic FLOPs of the layer >= 1 input projections (launched between two GRU intervals)
};

namespace tepose {

#define CK(expr)                      \
  do {                                \
    hipError_t e__ = (expr);          \
    if (e__ != hipSuccess) return (int)e__; \
  } while (0)

// W operand of a split-precision product: the planes of format f of a weight (view) in `blob`; kst: halfs between K-tiles
struct WPlanes { const half_t *hi, *lo; long kst; };
inline WPlanes w_planes(const float* blob, WView v, Fmt f) {
  const Weight& w = *v.w;
  const size_t tile = f == Fmt::scaled ? 16 : 32, R = f == Fmt::scaled ? w.Rs : w.Rp;
  const half_t* hi = (const half_t*)(blob + (f == Fmt::scaled ? w.s : w.p)) + (size_t)v.row0 * tile + (size_t)v.k0 * R;
  return WPlanes{hi, hi + R * w.Kp, (long)(R * tile)};
}
// ... and the fp32 rows / the bias of the same view (nullptr: the weight has none)
inline const float* w_rows(const float* blob, WView v) { return blob + v.w->w + (size_t)v.row0 * v.w->Kp + v.k0; }
inline const float* w_bias(const float* blob, WView v) { return v.w->b ? blob + v.w->b + v.row0 : nullptr; }

// ---- one way to launch a plain product  C = (A W^T + bias + addend) * scale  (forward.hip) ----------------------------------------------------------
enum class Mm : unsigned char;     // the kernel family of one product (plan.h)
struct Planes { half_t *hi = nullptr, *lo = nullptr; long kst = 0; };   // hi / lo planes of an A operand or of a product's output: view base, halfs between K-tiles
// The A operand, as it was carved: fp32 rows and / or blocked planes and / or scaled planes -- the family reads the form it takes.
struct AOperand {
  const float* rows = nullptr; long lda = 0;
  Planes p;                              // blocked [K/32][R][32]
  Planes s; float s_scale = 1.f;         // scaled [K/16][R][16], and the scale of their values (kStateScale for recurrent states; 1 with row scales)
  const float* row_scale = nullptr;      // the planes hold row m divided by row_scale[m] (launch_split_rows)
};
struct Epilogue {
  const float* bias = nullptr;
  const float* addend = nullptr; long ldadd = 0;
  float scale = 0.f;                     // 0: none
  int relu_a = 0;                        // exact-fp32 families: max(0, .) on A on the fly (the split families are handed ReLU'd planes)
  const Planes* out = nullptr;           // Mm::h3 / h3_skinny: C also as blocked planes (the next product's A)
  int c_blk_hp = 0;                      // scaled families: != 0 (= Hp): C is a gate pre-activation matrix, written in the blocked layout (common.h gi_blk_offset)
  unsigned* sync = nullptr; bool reg = false;   // scaled families: the forward's sync region and which of its status words (regressor | recurrent part) takes a give-up
  int tag = 1;                           // scaled families: 0 = the layer-0 projection's own kernel symbol
};
// tail_stage: a product of the plan's tail stage (tail linears, FC loop, their collapsed forms), where <= 256 columns always run width-first
int product(const tepose_model* m, Mm f, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e, hipStream_t s, bool tail_stage = false);
// the exact-fp32 families' arguments of that description (also for launch_gemm, which picks between the two by the row count itself: VIBE, HMR)
inline GemmArgs f32_args(const float* blob, const AOperand& A, WView W, float* C, long ldc, int M, int N, const Epilogue& e) {
  return GemmArgs{A.rows, A.lda, w_rows(blob, W), W.w->Kp, C, ldc, e.bias, e.addend, e.ldadd, e.scale != 0.f ? e.scale : 1.f, M, N, e.relu_a};
}

// ---- fault channel of the persistent kernels: the tests every entry point and the kernel selection use
inline bool fault_pending(const tepose_model* m) { return m->fault && __atomic_load_n(m->fault, __ATOMIC_RELAXED) != 0u; }
// entry of a forward that owns status words in `workspace`: refused while the word is raised, else noted with the collection count it starts under
inline int forward_begin(const tepose_model* m, const void* workspace) {
  if (fault_pending(m)) return TEPOSE_E_TIMEOUT;
  if (workspace) {
    std::lock_guard<std::mutex> g(m->q_mu);
    if (m->q_gen.size() > 4096) m->q_gen.clear();        // callers that never reuse a workspace: an unknown workspace takes the slow path, which is always right
    m->q_gen[workspace] = m->collected;
  }
  return 0;
}
// rows up to which the persistent kernels may run (the option, capped by what the kernels hold: 64 rows)
inline int seq_rows_cap(const tepose_model* m) { return m->opt.seq_max_m > 64 ? 64 : m->opt.seq_max_m; }
inline int reg_seq_rows_cap(const tepose_model* m) { return m->opt.reg_seq_max_n > 64 ? 64 : m->opt.reg_seq_max_n; }
inline bool persist_on(const tepose_model* m) {
  return __atomic_load_n(&m->persist, __ATOMIC_RELAXED) && m->fault != nullptr;   // (tepose_set_persistent may run on another thread)
}

// Arrival counters of the persistent kernels (gru_seq.hip, reg_seq.hip), ONE block zeroed by one memset node per
// forward.  It is the first carve of the encoder's and of the regressor's workspace, so that inside tepose_forward
// (both share one region) it is the same memory: [L x 3 x 32 recurrent arrivals | 32 status | 3 x 32 regressor | 32 status].
inline size_t sync_words(const tepose_model* m) { return (size_t)m->L * 96 + 32 + 96 + 32; }
inline unsigned* sync_gru(unsigned* sy, int l) { return sy + (size_t)l * 96; }
inline unsigned* sync_gru_status(const tepose_model* m, unsigned* sy) { return sy + (size_t)m->L * 96; }
inline unsigned* sync_reg(const tepose_model* m, unsigned* sy) { return sy + (size_t)m->L * 96 + 32; }
inline unsigned* sync_reg_status(const tepose_model* m, unsigned* sy) { return sy + (size_t)m->L * 96 + 32 + 96; }

// blob.hip
void layout(tepose_model* m);          // TePose handle: every section's offset, the plane table, blob_floats
void layout_vibe(tepose_model* m);     // VIBE bootstrap handle
void layout_hmr(tepose_model* m);      // HMR handle: the backbone's sections from the layer table (hmr.h), then the shared regressor / SMPL sections
int pack(const float* src, long ld, int N, int K, float* dst, int Np, int Kp, int rowmap, int colmap, int H, int Hp, hipStream_t s);

}  // namespace tepose
