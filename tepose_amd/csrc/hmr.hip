// The HMR feature extractor (reference lib/models/spin.py:127-141): the launch sequence over the layer table of hmr.h -- per convolution one gather
// (conv.hip) and one product on the library's existing launchers -- plus the handle-less convolution / pooling entries the tests drive.
#include <algorithm>

#include "hmr.h"
#include "plan.h"

using namespace tepose;

namespace {

struct HmrWs {                         // one pass of n images
  float* t[kHmrTensors] = {};
  char* a = nullptr;                   // the product's A operand: hi | lo planes (split) or fp32 rows (exact)
  float* row_scale = nullptr;
  size_t bytes = 0;
};

// The same table sizes everything: every tensor is as large as the largest output written to it, the A region as the largest rows x Kp.
HmrWs carve_hmr(int n, void* base) {
  size_t fl[kHmrTensors] = {}, a_bytes = 0, rows_max = 0;
  (void)hmr_walk(n, [&](const ConvStep& c) {
    fl[c.l->out] = std::max(fl[c.l->out], (size_t)c.rows * c.l->cout);
    a_bytes = std::max(a_bytes, (size_t)c.rows * c.Kp * sizeof(float));      // 2 fp16 planes = one fp32 matrix
    rows_max = std::max(rows_max, (size_t)c.rows);
    return 0;
  });
  fl[T_J] = fl[T_C];                   // the joined value of a block has its conv3's shape (and the max-pooled stem is smaller)
  HmrWs w;
  size_t cur = 0;
  auto take = [&](size_t bytes) { const size_t o = cur; cur = align_up(cur + bytes, 256); return (char*)base + o; };
  for (int t = T_J; t < kHmrTensors; ++t) w.t[t] = (float*)take(fl[t] * sizeof(float));
  w.a = take(a_bytes);
  w.row_scale = (float*)take(rows_max * sizeof(float));
  w.bytes = cur + 256;
  return w;
}

// The A operand of one convolution's product y[rows][cout] = gather(a) * W^T + bias: split -- gathered blocked planes with row scales; exact -- gathered
// fp32 rows, or x itself (a 1 x 1 stride-1 convolution over NHWC rows IS the product: no gather, the ReLU rides in the A loads: relu_a)
int conv_operand(GatherArgs g, bool split, bool gather, char* a_buf, float* row_scale, hipStream_t s, AOperand& A, int& relu_a) {
  const long rows = (long)g.N * g.Ho * g.Wo;
  if (split) {
    g.hi = (half_t*)a_buf; g.lo = g.hi + (size_t)rows * g.Kp; g.row_scale = row_scale;
    A.p = Planes{g.hi, g.lo, rows * 32}; A.row_scale = row_scale;
  } else {
    if (gather) g.out = (float*)a_buf;
    A.rows = gather ? g.out : g.x; A.lda = g.Kp;
    relu_a = gather ? 0 : g.relu;
  }
  return gather ? (int)launch_conv_gather(g, split, s) : 0;
}

// ... and the product, W the convolution's record in the handle's blob: split on the library's product function, exact on launch_gemm (which picks
// the width-first kernel by the row count itself)
int conv_product(const tepose_model* m, const GatherArgs& g, bool gather, const Weight& W, int cout, float* y, char* a_buf, float* row_scale, hipStream_t s) {
  const int rows = g.N * g.Ho * g.Wo;
  AOperand A;
  Epilogue e{w_bias(m->blob, W)};
  CK((hipError_t)conv_operand(g, m->split, gather, a_buf, row_scale, s, A, e.relu_a));
  if (m->split) return product(m, Mm::h3, A, W, y, cout, rows, cout, e, s);
  return (int)launch_gemm(f32_args(m->blob, A, W, y, cout, rows, cout, e), s, m->opt);
}

bool needs_gather(const GatherArgs& g, bool split) {
  return split || g.R != 1 || g.stride != 1 || g.pad != 0 || g.res || g.nchw || g.K != g.Kp;
}

constexpr int kStopped = 1 << 20;      // hmr_walk's return when a pass was asked to end early: no TEPOSE_E_* (negative) and no hipError_t (CK, < 2000)

// The launches of one pass.  last < kHmrConvs - 1 (tepose_hmr_features_upto) ends it after convolution `last` (and the max pool, for the stem);
// feat == nullptr leaves the final join + average pool out.
int hmr_pass(const tepose_model* m, const float* x, int n, float* feat, const HmrWs& w, hipStream_t s, int last = kHmrConvs - 1) {
  float* const* t = w.t;
  int rc = hmr_walk(n, [&](const ConvStep& c) {
    const ConvLayer& l = *c.l;
    GatherArgs g{};
    g.x = l.in == T_IMG ? x : (l.join ? t[T_C] : t[l.in]);
    g.res = l.join == J_IDENT ? t[T_J] : (l.join == J_DOWN ? t[T_D] : nullptr);
    g.wb = l.join ? t[T_J] : nullptr;
    g.relu = (l.join || l.in == T_A || l.in == T_B) ? 1 : 0;      // T_J holds a joined (ReLU'd) value already
    g.nchw = l.in == T_IMG;
    g.N = n; g.H = g.W = c.Hin; g.C = l.cin; g.R = l.R; g.stride = l.stride; g.pad = l.pad; g.Ho = g.Wo = c.Hout; g.K = c.K; g.Kp = c.Kp;
    const int e = conv_product(m, g, needs_gather(g, m->split), m->bb[c.idx], l.cout, t[l.out], w.a, w.row_scale, s);
    if (e) return e;
    if (c.idx == 0) CK(launch_maxpool3x3s2(t[T_C], n, c.Hout, c.Hout, l.cout, t[T_J], 1, s));       // max(relu(.)) = relu(max(.))
    return c.idx == last && last < kHmrConvs - 1 ? kStopped : 0;
  });
  if (rc && rc != kStopped) return rc;
  if (rc == kStopped || !feat) return 0;
  CK(launch_avgpool7(t[T_C], kHmrTable.final_join == J_DOWN ? t[T_D] : t[T_J], 1, n, kFeat, feat, s));
  return 0;
}

}  // namespace

extern "C" {

size_t tepose_hmr_workspace_bytes(const tepose_model* m, int N) {
  if (!m || m->kind != 2 || N < 1) return 0;
  return carve_hmr(N < kHmrPass ? N : kHmrPass, nullptr).bytes;
}

int tepose_hmr_features(const tepose_model* m, const float* x, int N, float* feat, void* workspace, size_t ws_bytes, void* stream) {
  if (!m || !x || !feat || !workspace || N < 1) return TEPOSE_E_ARG;
  if (m->kind != 2 || !m->bb_packed || !m->blob) return TEPOSE_E_STATE;
  const int per = N < kHmrPass ? N : kHmrPass;
  if (ws_bytes < carve_hmr(per, nullptr).bytes) return TEPOSE_E_WORKSPACE;
  const size_t img = (size_t)3 * kHmrImage * kHmrImage;
  for (int i0 = 0; i0 < N; i0 += per) {
    const int n = N - i0 < per ? N - i0 : per;
    const int rc = hmr_pass(m, x + (size_t)i0 * img, n, feat + (size_t)i0 * kFeat, carve_hmr(n, workspace), (hipStream_t)stream);
    if (rc) return rc;
  }
  return 0;
}

// ---- building blocks for tests
// One pass of tepose_hmr_features cut short after convolution `last_conv`; what that convolution wrote (before its ReLU) and the block input T_J as
// they stand then, copied out.  The counts come from the table, so a caller that restates the network checks its restatement against hmr.h here.
int tepose_hmr_features_upto(const tepose_model* m, const float* x, int N, int last_conv, float* out, size_t out_floats, float* joined,
                             size_t joined_floats, void* workspace, size_t ws_bytes, void* stream) {
  if (!m || !x || !out || !workspace || N < 1 || N > kHmrPass || last_conv < 0 || last_conv >= kHmrConvs) return TEPOSE_E_ARG;
  if (m->kind != 2 || !m->bb_packed || !m->blob) return TEPOSE_E_STATE;
  size_t out_n = 0, joined_n = 0;
  int out_t = T_C;
  (void)hmr_walk(N, [&](const ConvStep& c) {
    const ConvLayer& l = *c.l;
    if (l.join) joined_n = (size_t)N * c.Hin * c.Hin * l.cin;                 // conv1 of a block writes back what it reads
    if (c.idx == 0) joined_n = (size_t)N * l.cout * conv_out_size(c.Hout, 3, 2, 1) * conv_out_size(c.Hout, 3, 2, 1);
    out_n = (size_t)c.rows * l.cout;
    out_t = l.out;
    return c.idx == last_conv ? kStopped : 0;
  });
  if (out_floats != out_n || (joined && joined_floats != joined_n)) return TEPOSE_E_SHAPE;
  const HmrWs w = carve_hmr(N, workspace);
  if (ws_bytes < w.bytes) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int rc = hmr_pass(m, x, N, nullptr, w, s, last_conv);
  if (rc) return rc;
  CK(hipMemcpyAsync(out, w.t[out_t], out_n * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (joined) CK(hipMemcpyAsync(joined, w.t[T_J], joined_n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

// the gather + the product on caller-supplied tensors
size_t tepose_conv2d_nhwc_workspace_bytes(int N, int H, int W, int Cin, int Cout, int R) {
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || R < 1) return 0;
  const size_t rows = (size_t)N * H * W, Kp = conv_kp(Cin, R), Np = round_up(Cout, 128);      // stride 1, 2 * pad < R: the most rows
  // packed fp32 weights | their planes | bias | error word | A operand | row scales
  return 2 * align_up(Np * Kp * sizeof(float), 256) + align_up((size_t)Cout * sizeof(float), 256) + 256 + align_up(rows * Kp * sizeof(float), 256) +
         align_up(rows * sizeof(float), 256);
}

int tepose_conv2d_nhwc_f32(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int R, int stride, int pad,
                           int relu_in, const float* residual, float* y, int exact, void* workspace, size_t ws_bytes, void* stream) {
  if (!x || !w_oihw || !y || !workspace || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return TEPOSE_E_ARG;
  if (R < 1 || R > 7 || stride < 1 || stride > 2 || pad < 0 || 2 * pad >= R || H + 2 * pad < R || W + 2 * pad < R) return TEPOSE_E_SHAPE;
  if (ws_bytes < tepose_conv2d_nhwc_workspace_bytes(N, H, W, Cin, Cout, R)) return TEPOSE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int Kp = conv_kp(Cin, R), Np = round_up(Cout, 128);
  char* p = (char*)workspace;
  auto take = [&](size_t bytes) { char* o = p; p += align_up(bytes, 256); return o; };
  float* Wf = (float*)take((size_t)Np * Kp * sizeof(float));
  half_t* Wh = (half_t*)take((size_t)Np * Kp * sizeof(float));
  float* bf = (float*)take((size_t)Cout * sizeof(float));
  int* err = (int*)take(sizeof(int));
  GatherArgs g{};
  g.x = x; g.res = residual; g.relu = relu_in ? 1 : 0;
  g.N = N; g.H = H; g.W = W; g.C = Cin; g.R = R; g.stride = stride; g.pad = pad;
  g.Ho = conv_out_size(H, R, stride, pad); g.Wo = conv_out_size(W, R, stride, pad); g.K = Cin * R * R; g.Kp = Kp;
  const long rows = (long)N * g.Ho * g.Wo;
  char* a_buf = take((size_t)rows * Kp * sizeof(float));
  float* rs = (float*)take((size_t)rows * sizeof(float));
  CK(hipMemsetAsync(err, 0, sizeof(int), s));
  CK(launch_hmr_fold_pack(w_oihw, nullptr, bias, nullptr, nullptr, Cout, Cin, R, Wf, Np, Kp, bf, err, s));
  if (!exact) CK(launch_split_planes(Wf, Kp, Np, Kp, Kp, Np, Wh, Wh + (size_t)Np * Kp, s));
  // (no handle, no blob: the caller's weights sit in the workspace, and the launchers are called with them directly)
  AOperand A;
  int relu_a = 0;
  CK((hipError_t)conv_operand(g, !exact, needs_gather(g, !exact), a_buf, rs, s, A, relu_a));
  if (exact) return (int)launch_gemm(GemmArgs{A.rows, Kp, Wf, Kp, y, Cout, bf, nullptr, 0, 1.f, (int)rows, Cout, relu_a}, s, options_from_env());
  H3Batch b{};
  b.p[0] = H3Args{A.p.hi, A.p.lo, A.p.kst, Wh, Wh + (size_t)Np * Kp, (long)Np * 32, Kp, y, Cout, bf, (int)rows, Cout};
  b.p[0].row_scale = rs; b.n = 1;
  return (int)launch_gemm_h3(b, s, options_from_env());
}

int tepose_hmr_fold_pack(const float* w_oihw, const float* gamma, const float* beta, const float* mean, const float* var, int Cout, int Cin, int R,
                         float* w_out, float* b_out, void* stream) {
  if (!w_oihw || !gamma || !beta || !mean || !var || !w_out || !b_out || Cout < 1 || Cin < 1 || R < 1) return TEPOSE_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  int* err = nullptr;
  CK(hipMalloc((void**)&err, sizeof(int)));      // test entry: may allocate and synchronise, like the pack functions
  int bad = 0;
  auto run = [&]() -> int {
    CK(hipMemsetAsync(err, 0, sizeof(int), s));
    CK(launch_hmr_fold_pack(w_oihw, gamma, beta, mean, var, Cout, Cin, R, w_out, Cout, conv_kp(Cin, R), b_out, err, s));
    CK(hipMemcpyAsync(&bad, err, sizeof(int), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = run();
  (void)hipFree(err);
  return rc ? rc : (bad ? TEPOSE_E_ARG : 0);
}

int tepose_maxpool3x3s2_nhwc(const float* x, int N, int H, int W, int C, float* y, void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1 || C < 1) return TEPOSE_E_ARG;
  if (C % 4 != 0) return TEPOSE_E_SHAPE;
  CK(launch_maxpool3x3s2(x, N, H, W, C, y, 0, (hipStream_t)stream));
  return 0;
}

int tepose_avgpool7_nhwc(const float* x, int N, int C, float* y, void* stream) {
  if (!x || !y || N < 1 || C < 1) return TEPOSE_E_ARG;
  CK(launch_avgpool7(x, nullptr, 0, N, C, y, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
