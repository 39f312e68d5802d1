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

struct DirW {                     // one GRU layer/direction inside the blob (float offsets)
  size_t wih = 0, bih = 0;        // input projection (layer-0 ones live in the stacked block)
  size_t whh = 0, bhh = 0;
  size_t wih_p = 0, whh_p = 0;    // blocked hi|lo fp16 planes of the same matrices (whh: gate-tiled rows), float offsets
  size_t wih_s = 0, whh_s = 0;    // the same as scaled [K/16][R][16] planes (gemm_h3s.hip; rows padded to 256 / 384)
  size_t scales = 0;              // blob slot: [0] = W_ih scale, [1] = W_hh scale
  float wih_scale = 1.f, whh_scale = 1.f;   // host copies
};

struct SmplOff {
  size_t J0, JS, blendW, lbsW, lbs_cidx, lbs_cval, lbs_nnz, parents, depth, xr_ptr, xr_idx, xr_val;
};

// One derived section of the blob: hi | lo fp16 planes of a packed fp32 matrix that lives in the blob too.  The layout pass enters every one into
// tepose_model::planes as it carves it, so the section's size, its content (derive_planes, the only code that writes a plane section or a scale slot)
// and the complement a rank has to receive (tepose_fp32_ranges) all come from this one list.
enum class Owner : unsigned char { encoder, regressor, smpl, collapsed_regressor, collapsed_tail, backbone };   // whose packing fills the source
struct PlaneSpec {
  Owner owner;
  size_t src; int rows, Kp;       // source: packed fp32 [rows][Kp]
  size_t dst; int R, Kd, k0;      // section: planes of an [R][Kd] matrix (lo plane behind the hi plane; rows beyond `rows` zero); this entry is its K range [k0, k0 + Kp)
  // scaled [K/16][R][16] planes (gemm_h3s.hip) with one power-of-two scale per matrix: the handle field that holds the scale's blob slot, the float inside
  // the slot, the handle's host copy.  nullptr: blocked [K/32][R][32] planes (gemm_h3.hip)
  const size_t* scale_slot = nullptr; int scale_i = 0; float* scale_host = nullptr;
};

}  // namespace tepose

struct tepose_model {
  int kind = 0;                                 // 0 = TePose, 1 = VIBE bootstrap encoder, 2 = HMR (ResNet-50 backbone + regressor + SMPL)
  // HMR backbone (hmr.h): per convolution of the layer table, the folded weights [Np][Kp], the folded batch-norm shift [C_out], their hi | lo planes
  std::vector<size_t> bb_w, bb_b, bb_p;
  bool bb_packed = false, bb_range_ok = true;
  std::vector<tepose::DirW> vibe;               // VIBE: per-layer GRU weights; wih / bih hold the stacked rows of both
                                                // directions ([dir][3Hp]), whh / bhh of direction d sit at + d * their size
  bool vibe_bidir = false, vibe_linear = true;  // vibe.py:27-47: bidirectional GRU; Linear(D*hidden -> 2048) on relu(y)
  size_t vlin_w = 0, vlin_b = 0;
  bool vibe_packed = false;
  int L = 0, H = 0, Hp = 0;
  size_t hdr = 0;                               // blob header (BlobHeader): what the blob holds, checked by tepose_adopt_blob
  float* blob = nullptr;
  size_t blob_floats = 0;
  std::vector<tepose::PlaneSpec> planes;        // every derived section (the layout pass fills it)
  bool enc_packed = false, reg_packed = false, smpl_packed = false;
  // encoder offsets
  size_t wih0 = 0, bih0 = 0;                    // stacked [9Hp][2144]: fwd | rec_reverse | rec
  size_t wih0_p = 0;                            // its hi|lo planes
  size_t wih0_s = 0, wih0_scale = 0;            // the same block as scaled [K/16][R][16] planes (gemm_h3s.hip) + its scale
  float w0_scale = 1.f;                         // host copy of blob[wih0_scale]
  // kernel-family knobs (named options, read once per handle; defaults = the measured best):
  bool large_scaled = true;                     // TEPOSE_LARGE_BATCH_KERNELS=scaled|twoacc: large batches (layer-0 projection from B * T >= 8192 / mid tiles from 512 rows,
                                                // recurrent path from s_min_b windows) on the scaled-plane single-accumulator kernels (gemm_h3s16c.hip, gru_step16.hip,
                                                // gemm_h3s.hip) -- or, `twoacc`, on the two-accumulator family of gemm_h3.hip at every batch size
  bool state_planes = true;                     // TEPOSE_GRU_STATE=planes|fp32: the large-batch step kernel rebuilds h_{t-1} from the state planes and takes its cell
                                                // operands through the LDS-DMA stream (gru_step16_kernel<true>) -- or, `fp32`, keeps a separate fp32 state copy (<false>)
  std::string kinfo;                            // tepose_kernel_info(): the kernel symbols the knobs select for the dominant launches of cfg-C
  std::vector<tepose::DirW> fwd, rec_f, rec_r;  // per layer
  size_t wlf = 0, blf = 0, wlr = 0, blr = 0;
  size_t wlf_p = 0, wlr_p = 0;                  // blocked hi|lo planes of the tail linears
  size_t wlfr_p = 0;                            // planes of [W_lf | W_lr] ([2048][3Hp]): eval mode's (y_fwd + y_rec)/2 as ONE product
  // regressor offsets
  size_t w1a = 0, b1 = 0, w1b = 0, w2 = 0, b2 = 0, wdec = 0, bdec = 0, init = 0;
  size_t w1a_p = 0, w1b_p = 0, w2_p = 0, wdec_p = 0, blendW_p = 0;   // blocked hi|lo planes (split path)
  size_t blendW_s = 0, blend_scale = 0;         // the blend-shape matrix as scaled [K/16][R][16] planes (large batches: barrier-free persistent kernel) + its scale
  float blend_sc = 1.f;                         // host copy of blob[blend_scale]
  // collapsed regressor: the eval-mode FC loop is affine in (feature, initial state), so with the model's own
  // initial state and n_iter = 3 the final state is  xs = feat Mf^T + k0  and, through the (affine) tail linears,
  // xs = [relu(h_fwd) | relu(y_rec0)] Mt^T + kt.  fp64 algebra at pack time; [256][K] fp32 + planes, bias rows of 160.
  size_t mf = 0, mf_p = 0, k0 = 0, mt = 0, mt_p = 0, kt = 0;
  bool reg_collapsed = false, tail_collapsed = false;
  bool collapse_env = true;                     // TEPOSE_COLLAPSE_REGRESSOR=0: always run the FC loop
  tepose::SmplOff smpl{};
  int maxdepth = 0;
  int lbs_sparse = 0;                           // skin-weight table has <= 4 non-zeros per vertex
  bool split = true;                            // batches of more than m->opt.split_min_m rows run their matmuls on the fp16x3 split kernels
  bool split_env = true;                        // what the environment asked for; `split` also needs every packed weight inside
  bool enc_range_ok = true, reg_range_ok = true, smpl_range_ok = true;   // the fp16 range (|w| < 2^15), checked at pack time
  int s_min_b = 640;                            // scaled-format recurrent path from this batch size
  tepose::Options opt;                          // every launch threshold (common.h Options): from the environment at tepose_create, tepose_set_option before packing
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

// W operand of a split-precision product: the plane section `dst` (PlaneSpec::dst) of an [R][K] matrix, blocked or scaled
struct WPlanes { const half_t *hi, *lo; long kst; };
inline WPlanes w_planes(const tepose_model* m, size_t dst, size_t R, size_t K, bool scaled = false) {
  const half_t* hi = (const half_t*)(m->blob + dst);
  return WPlanes{hi, hi + R * K, (long)R * (scaled ? 16 : 32)};
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
