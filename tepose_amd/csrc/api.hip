// The extern "C" boundary of libtepose_hip.so (include/tepose_amd.h): handle creation with the one read of the environment, options, the status / fault
// channel, profiling reads, and the thin metric / filter / geometry / GEMM test entries.  The packing entry points live in blob.hip, every forward entry
// point next to its launch sequence in forward.hip.  No launch sequence here.
#include <stdlib.h>
#include <string.h>

#include <new>

#include "plan.h"

using namespace tepose;

static inline void fault_collected(const tepose_model* m) {
  std::lock_guard<std::mutex> g(m->q_mu);
  ++m->collected;
}

// numerics / dispatch knobs, read once per handle at creation (both model kinds)
static void read_env_knobs(tepose_model* m) {
  m->opt = options_from_env();                      // the launch thresholds (options.h Options)
  const char* e = getenv("TEPOSE_EXACT_FP32");      // 1: keep every product on the exact-fp32 MFMA
  m->split = m->split_env = !(e && atoi(e) != 0);
  e = getenv("TEPOSE_LARGE_BATCH_KERNELS");         // scaled (default) | twoacc
  m->large_scaled = !(e && std::string(e) == "twoacc");
  e = getenv("TEPOSE_GRU_STATE");                   // planes (default) | fp32
  m->state_planes = !(e && std::string(e) == "fp32");
  e = getenv("TEPOSE_COLLAPSE_REGRESSOR");          // 0: the regressor's FC loop is always run as a loop
  m->collapse_env = !(e && atoi(e) == 0);
  e = getenv("TEPOSE_S_MIN_B");                     // batch threshold of the scaled-format recurrent path
  m->s_min_b = e ? atoi(e) : 640;                   // measured crossover against the two-accumulator recurrent path (round 4, 16x16x32 step + blocked
                                                    // operands: B = 512 2.38 vs 2.63 ms, 640 3.17 vs 2.94, 1024 4.29 vs 3.90, 1536 6.70 vs 5.91; it was 2048)
  e = getenv("TEPOSE_PERSISTENT");                  // 0: never launch the persistent small-batch kernels (the remedy for GPUs
  m->persist = !(e && atoi(e) == 0);                // that are shared or CU-masked: they need all their workgroups resident)
  e = getenv("TEPOSE_SEQ_SPIN_LIMIT");              // polls before a persistent kernel's wait gives up
  if (e && atol(e) > 0) m->spin_limit = (unsigned)atol(e);
  e = getenv("TEPOSE_TEST_FAULT");                  // tests only: make the persistent kernels' waits unmeetable
  m->test_fault = e ? (unsigned)atoi(e) : 0u;
  e = getenv("TEPOSE_BLEND16_MIN_N");
  m->blend16_min_n = e ? atoi(e) : 512;
  e = getenv("TEPOSE_GI_BLK");
  m->gi_blk = e ? atoi(e) : 1;
  refresh_kernel_info(m);
}

extern "C" {

int tepose_version(void) { return TEPOSE_ABI_VERSION; }

const char* tepose_build_info(void) {
#ifdef TEPOSE_NO_PACKED_FP32
  return "gfx950 packed_fp32=off";
#else
  return "gfx950 packed_fp32=on";
#endif
}

const char* tepose_kernel_info(const tepose_model* m) { return m ? m->kinfo.c_str() : ""; }

const char* tepose_select_kernels(const tepose_model* m, int B, int T) {
  static thread_local std::string buf;
  if (!m || B < 1 || T < 1) return "";
  buf = describe_plan(m, B, T);
  return buf.c_str();
}

const char* tepose_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case TEPOSE_E_ARG: return "tepose: bad argument";
    case TEPOSE_E_SHAPE: return "tepose: unsupported shape";
    case TEPOSE_E_WORKSPACE: return "tepose: workspace too small";
    case TEPOSE_E_STATE: return "tepose: model not packed";
    case TEPOSE_E_TIMEOUT: return "tepose: a persistent kernel's bounded wait expired (GPU shared or CU-masked?); "
                                  "outputs of that forward are NaN -- tepose_status() clears, TEPOSE_PERSISTENT=0 / "
                                  "tepose_set_persistent(m, 0) selects the step-per-launch kernels";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "tepose: unknown error";
  }
}

int tepose_create(int n_layers, int hidden, tepose_model** out) {
  if (!out || n_layers < 1 || hidden < 1) return TEPOSE_E_ARG;
  if (n_layers > 8 || hidden > 8192) return TEPOSE_E_SHAPE;
  tepose_model* m = new (std::nothrow) tepose_model();
  if (!m) return TEPOSE_E_ARG;
  m->L = n_layers; m->H = hidden; m->Hp = round_up(hidden, 64);
  read_env_knobs(m);
  layout(m);
  *out = m;
  return 0;
}

void tepose_destroy(tepose_model* m) {
  if (!m) return;
  for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->ev_gru) (void)hipEventDestroy(e);
  if (m->fault) (void)hipHostFree(m->fault);
  delete m;
}

// ---- fault channel of the persistent kernels ------------------------------------------------------------------

int tepose_status_peek(const tepose_model* m) {
  if (!m) return TEPOSE_E_ARG;
  return fault_pending(m) ? TEPOSE_E_TIMEOUT : 0;
}

int tepose_status(tepose_model* m, void* stream) {
  if (!m) return TEPOSE_E_ARG;
  CK(hipStreamSynchronize((hipStream_t)stream));
  if (!m->fault) return 0;
  const unsigned code = __atomic_exchange_n(m->fault, 0u, __ATOMIC_RELAXED);
  if (code) { m->last_fault_code = (int)code; fault_collected(m); }
  return code != 0u ? TEPOSE_E_TIMEOUT : 0;
}

int tepose_forward_status(tepose_model* m, void* workspace, void* stream) {
  if (!m || !workspace) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  CK(hipStreamSynchronize(s));
  // every give-up raises BOTH the forward's status word (workspace) and the handle's fault word (pinned host memory, system scope): with the stream
  // drained, a clear fault word means no forward of this handle gave up -- one host-memory read, no copy (the D2H copy + two null-stream
  // memsets per small-batch forward of sync mode) -- PROVIDED nobody has collected a fault since this forward was queued (another thread's
  // tepose_status / tepose_forward_status clears the shared word; this forward's own status word is then the only trace of its give-up)
  if (m->fault && __atomic_load_n(m->fault, __ATOMIC_RELAXED) == 0u) {
    std::lock_guard<std::mutex> g(m->q_mu);
    auto it = m->q_gen.find(workspace);
    if (it != m->q_gen.end() && it->second == m->collected) return 0;
  }
  // the sync region is the first carve of every workspace (carve_encoder / carve_regressor): [.. | gru status | .. | reg status]
  unsigned* sy = (unsigned*)workspace;
  // one copy of the span [recurrent status .. regressor status] (129 words: the regressor's arrival counters lie between them), on the caller's stream
  unsigned span[32 + 96 + 1];
  static_assert(sizeof(span) == (32 + 96 + 1) * sizeof(unsigned), "span");
  CK(hipMemcpyAsync(span, sync_gru_status(m, sy), sizeof(span), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  const unsigned st[2] = {span[0], span[32 + 96]};
  if ((st[0] | st[1]) == 0u) return 0;          // somebody else's forward raised the handle's word: theirs to collect
  // once per faulted forward: a later forward that launches no persistent kernel does not clear the words itself
  CK(hipMemsetAsync(sync_gru_status(m, sy), 0, sizeof(unsigned), s));
  CK(hipMemsetAsync(sync_reg_status(m, sy), 0, sizeof(unsigned), s));
  CK(hipStreamSynchronize(s));
  m->last_fault_code = (int)(st[0] ? st[0] : st[1]);
  if (m->fault && __atomic_exchange_n(m->fault, 0u, __ATOMIC_RELAXED) != 0u) fault_collected(m);   // (cleared, or every entry point would go on refusing)
  return TEPOSE_E_TIMEOUT;
}

// One named option of this handle (options.h Options + the handle's own batch thresholds), before anything is packed: workspace sizes and the packed
// planes depend on them.  name = the environment variable's, with or without the TEPOSE_ prefix.
int tepose_set_option(tepose_model* m, const char* name, long value) {
  if (!m || !name) return TEPOSE_E_ARG;
  if (m->enc_packed || m->reg_packed || m->smpl_packed || m->vibe_packed || m->bb_packed) return TEPOSE_E_STATE;
  const char* n = strncmp(name, "TEPOSE_", 7) == 0 ? name + 7 : name;
  if (int* f = option_field(m->opt, n)) *f = (int)value;
  else if (strcmp(n, "S_MIN_B") == 0) m->s_min_b = (int)value;
  else if (strcmp(n, "BLEND16_MIN_N") == 0) m->blend16_min_n = (int)value;
  else if (strcmp(n, "GI_BLK") == 0) m->gi_blk = (int)value;
  else if (strcmp(n, "SEQ_SPIN_LIMIT") == 0) { if (value <= 0) return TEPOSE_E_ARG; m->spin_limit = (unsigned)value; }
  else return TEPOSE_E_ARG;
  refresh_kernel_info(m);
  return 0;
}

long tepose_get_option(const tepose_model* m, const char* name) {
  if (!m || !name) return -1;
  const char* n = strncmp(name, "TEPOSE_", 7) == 0 ? name + 7 : name;
  Options o = m->opt;
  if (const int* f = option_field(o, n)) return *f;
  if (strcmp(n, "S_MIN_B") == 0) return m->s_min_b;
  if (strcmp(n, "BLEND16_MIN_N") == 0) return m->blend16_min_n;
  if (strcmp(n, "GI_BLK") == 0) return m->gi_blk;
  if (strcmp(n, "SEQ_SPIN_LIMIT") == 0) return (long)m->spin_limit;
  return -1;
}

int tepose_fault_code(const tepose_model* m) {
  if (!m) return TEPOSE_E_ARG;
  const unsigned live = m->fault ? __atomic_load_n(m->fault, __ATOMIC_RELAXED) : 0u;
  return live ? (int)live : m->last_fault_code;
}

int tepose_set_persistent(tepose_model* m, int on) {
  if (!m) return TEPOSE_E_ARG;
  __atomic_store_n(&m->persist, on != 0, __ATOMIC_RELAXED);
  return 0;
}

unsigned tepose_debug_kernel_errors(void) { return h3s16c_read_err(); }

int tepose_debug_set_test_fault(tepose_model* m, unsigned bits) {
  if (!m) return TEPOSE_E_ARG;
  m->test_fault = bits;
  return 0;
}

int tepose_uses_persistent(const tepose_model* m, int B, int T) {
  if (!m || B < 1) return 0;
  if (!persist_on(m) || !m->split || B <= m->opt.split_min_m) return 0;
  const int cap = seq_rows_cap(m) > reg_seq_rows_cap(m) ? seq_rows_cap(m) : reg_seq_rows_cap(m);
  (void)T;
  return B <= cap ? 1 : 0;
}

int tepose_create_vibe_ex(int n_layers, int hidden, int bidirectional, int add_linear, tepose_model** out) {
  if (!out || n_layers < 1 || hidden < 1) return TEPOSE_E_ARG;
  if (n_layers > 8 || hidden > 8192) return TEPOSE_E_SHAPE;
  tepose_model* m = new (std::nothrow) tepose_model();
  if (!m) return TEPOSE_E_ARG;
  m->kind = 1; m->L = n_layers; m->H = hidden; m->Hp = round_up(hidden, 64);
  m->vibe_bidir = bidirectional != 0;
  m->vibe_linear = bidirectional != 0 || add_linear != 0;      // vibe.py:43-47: a bidirectional encoder always has the linear
  read_env_knobs(m);        // TEPOSE_EXACT_FP32 covers the bootstrap model's regressor / blend-shape products too
  layout_vibe(m);
  *out = m;
  return 0;
}

int tepose_create_hmr(tepose_model** out) {
  if (!out) return TEPOSE_E_ARG;
  tepose_model* m = new (std::nothrow) tepose_model();
  if (!m) return TEPOSE_E_ARG;
  m->kind = 2;
  m->L = 1; m->H = m->Hp = 64;      // no recurrent encoder: a nominal shape for the workspace carve that the regressor entries share with the other kinds
  read_env_knobs(m);
  layout_hmr(m);
  *out = m;
  return 0;
}

int tepose_create_vibe(int n_layers, int hidden, tepose_model** out) {
  return tepose_create_vibe_ex(n_layers, hidden, 0, 1, out);
}

int tepose_vibe_feature_dim(const tepose_model* m) {
  if (!m || m->kind != 1) return 0;
  return m->vibe_linear ? kFeat : m->H;
}

int tepose_profile_enable(tepose_model* m, int on) {
  if (!m) return TEPOSE_E_ARG;
  m->prof = on != 0;
  m->ev_used = 0;
  m->prof_flops = 0.0;
  m->ev_gru_used = 0;
  m->prof_gru_flops = 0.0;
  m->prof_l1_flops = 0.0;
  return 0;
}

int tepose_profile_read(tepose_model* m, double* total_ms, int* n_launches, double* flops_per_launch) {
  if (!m || !total_ms || !n_launches || !flops_per_launch) return TEPOSE_E_ARG;
  double tot = 0.0;
  for (size_t i = 0; i + 1 < m->ev_used; i += 2) {
    CK(hipEventSynchronize(m->ev[i + 1]));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *n_launches = (int)(m->ev_used / 2);
  *flops_per_launch = m->prof_flops;
  m->ev_used = 0;
  return 0;
}

int tepose_profile_read_gru(tepose_model* m, double* total_ms, int* n_forwards, double* flops_per_forward) {
  if (!m || !total_ms || !n_forwards || !flops_per_forward) return TEPOSE_E_ARG;
  double tot = 0.0;
  for (size_t i = 0; i + 1 < m->ev_gru_used; i += 2) {
    CK(hipEventSynchronize(m->ev_gru[i + 1]));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, m->ev_gru[i], m->ev_gru[i + 1]));
    tot += ms;
  }
  const int nf = (int)(m->ev_gru_used / (2 * (size_t)m->L));
  *total_ms = tot;
  *n_forwards = nf;
  *flops_per_forward = nf > 0 ? m->prof_gru_flops / nf : 0.0;
  m->ev_gru_used = 0;
  m->prof_gru_flops = 0.0;
  m->prof_l1_flops = 0.0;
  return 0;
}

// the layer >= 1 input projections are what runs between the end of layer l-1's step sequence and the start of layer l's:
// the gaps of the GRU interval list.  Does not reset (tepose_profile_read_gru does): call it first.
int tepose_profile_read_l1proj(tepose_model* m, double* total_ms, int* n_forwards, double* flops_per_forward) {
  if (!m || !total_ms || !n_forwards || !flops_per_forward) return TEPOSE_E_ARG;
  const size_t per = 2 * (size_t)m->L;
  double tot = 0.0;
  for (size_t f = 0; (f + 1) * per <= m->ev_gru_used; ++f)
    for (int l = 1; l < m->L; ++l) {
      CK(hipEventSynchronize(m->ev_gru[f * per + 2 * l]));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, m->ev_gru[f * per + 2 * l - 1], m->ev_gru[f * per + 2 * l]));
      tot += ms;
    }
  const int nf = (int)(m->ev_gru_used / per);
  *total_ms = tot;
  *n_forwards = nf;
  *flops_per_forward = nf > 0 ? m->prof_l1_flops / nf : 0.0;
  return 0;
}

int tepose_metrics_joints(const float* pred, const float* target, int N, int J, int pelvis_mode, float* mpjpe,
                          float* pa_mpjpe, float* accel, void* stream) {
  if (!pred || !target || !mpjpe || !pa_mpjpe || !accel || N < 1) return TEPOSE_E_ARG;
  if (J < 4 || J > 17 || (pelvis_mode != 0 && pelvis_mode != 1)) return TEPOSE_E_SHAPE;
  CK(launch_metrics_joints(pred, target, N, J, pelvis_mode, mpjpe, pa_mpjpe, accel, (hipStream_t)stream));
  return 0;
}

int tepose_metrics_verts(const float* pred_verts, const float* target_verts, int N, float* mpvpe, void* stream) {
  if (!pred_verts || !target_verts || !mpvpe || N < 1) return TEPOSE_E_ARG;
  CK(launch_metrics_verts(pred_verts, target_verts, N, mpvpe, (hipStream_t)stream));
  return 0;
}

int tepose_filter_one_euro(float* x, int N, int D, float min_cutoff, float beta, float d_cutoff, void* stream) {
  if (!x || N < 1 || D < 1) return TEPOSE_E_ARG;
  CK(launch_one_euro(x, N, D, min_cutoff, beta, d_cutoff, (hipStream_t)stream));
  return 0;
}

int tepose_filter_slerp(const float* rotmat_in, float* rotmat_out, int N, int J, double ratio, void* stream) {
  if (!rotmat_in || !rotmat_out || N < 1 || J < 1) return TEPOSE_E_ARG;
  CK(launch_slerp_smooth(rotmat_in, rotmat_out, N, J, ratio, (hipStream_t)stream));
  return 0;
}

int tepose_rotmat_to_angle_axis(const float* R, int N, float* aa, void* stream) {
  if (!R || !aa || N < 1) return TEPOSE_E_ARG;
  CK(launch_rotmat_to_aa(R, N, aa, (hipStream_t)stream));
  return 0;
}

int tepose_rot6d_to_rotmat(const float* x6, int N, float* R, void* stream) {
  if (!x6 || !R || N < 1) return TEPOSE_E_ARG;
  CK(launch_rot6d_to_rotmat(x6, N, R, (hipStream_t)stream));
  return 0;
}

size_t tepose_gemm_h3_workspace_bytes(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  const size_t a = gemm_h3_ws_bytes(M, N, K), b = gemm_h3s_ws_bytes(M, N, K);
  return a > b ? a : b;
}

int tepose_gemm_h3_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc,
                       int M, int N, int K, void* workspace, size_t ws_bytes, void* stream) {
  if (!A || !W || !C || !workspace || M < 1 || N < 1 || K < 1) return TEPOSE_E_ARG;
  if (K % 32 != 0) return TEPOSE_E_SHAPE;
  if (ws_bytes < gemm_h3_ws_bytes(M, N, K)) return TEPOSE_E_WORKSPACE;
  // TEPOSE_H3S=1 (read per call: this is the test / bench entry): the scaled-plane barrier-free kernel of gemm_h3s16c.hip, operand scales for
  // the ranges of tools/h3_loop.py / h3_bench.py and tests/test_gpu_stress.py; TEPOSE_H3S=mid: the 128 x 288-tile kernel of gemm_h3s.hip (N % 288 == 0)
  const char* pe = getenv("TEPOSE_H3S");
  const Options opt = options_from_env();          // no handle here: the environment's thresholds, read per call (test / bench entry)
  if (pe && pe[0] && std::string(pe) != "0" && std::string(pe).rfind("skinny", 0) != 0 && ws_bytes >= gemm_h3s_ws_bytes(M, N, K)) {
    CK(launch_gemm_h3s_f32(A, lda, W, ldw, C, ldc, M, N, K, 256.f, 16384.f, workspace, (hipStream_t)stream, opt, bias, std::string(pe) == "mid" ? 1 : 0));
    return 0;
  }
  // TEPOSE_H3S=skinny: the width-first kernel of skinny_h3.hip on the same planes, at any M (tools/mid_rows_gemm_bench.py)
  CK(launch_gemm_h3_f32(A, lda, W, ldw, bias, C, ldc, M, N, K, workspace, (hipStream_t)stream, opt, pe && std::string(pe) == "skinny" ? 1 : 0));
  return 0;
}

size_t tepose_gemm_workspace_bytes(int N, int K) {
  if (N < 1 || K < 1) return 0;
  return (size_t)round_up(N, 128) * round_up(K, 32) * sizeof(float) + 256;
}

int tepose_gemm_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc,
                    int M, int N, int K, int relu_a, void* workspace, size_t ws_bytes, void* stream) {
  if (!A || !W || !C || !workspace || M < 1 || N < 1 || K < 1) return TEPOSE_E_ARG;
  if (lda % 4 != 0 || ((uintptr_t)A & 15) != 0 || K % 32 != 0) return TEPOSE_E_SHAPE;
  if (ws_bytes < tepose_gemm_workspace_bytes(N, K)) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* wp = (float*)workspace;
  CK((hipError_t)pack(W, ldw, N, K, wp, round_up(N, 128), K, 0, 0, 0, 1, s));
  const GemmArgs g{A, lda, wp, K, C, ldc, bias, nullptr, 0, 1.f, M, N, relu_a};
  CK(launch_gemm(g, s, options_from_env()));       // no handle here: the environment's thresholds, read per call (test / bench entry)
  return 0;
}

}  // extern "C"
