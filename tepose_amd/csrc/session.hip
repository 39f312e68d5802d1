// Window upkeep of a multi-person live session (tepose_amd.stream.MultiStreamSession): S slots, each a sliding window
// win[s] = [T][2133] fp32 (2048 features + 85 theta per frame, row T - 1 the newest frame: evaluate.py:248-252, demo.py:239-241) of one contiguous
// [S][T][2133] tensor.  A tick gives every slot one op code in a device int32[S]:
//   0 hold     the window is not touched, no theta is fed back (an idle slot; a person without a detection in this frame)
//   1 advance  rows 1 .. T-1 move to 0 .. T-2, row T-1 becomes (feat[s], 85 zeros)
//   2 join     rows 0 .. T-2 are loaded from hist[s] ([T-1][2133]: features and theta history), row T-1 as for 1
//   3 clear    the whole window becomes zero (a person left)
// any other value acts as 0 -- and so does a 2 when the call was given no hist: nothing is read through a null pointer.
//
// session_advance_kernel: one launch, no scratch.  A thread owns ONE column of ONE slot and walks t upwards, reading win[t + 1][c] before it writes
// win[t][c]: the shift is in place, no other thread ever touches that column, and adjacent lanes touch adjacent columns (coalesced dwords).  The value
// read for the shift is also what `saved` receives, so a tick reads each window element once.  Rows are 2133 floats -- 8532 bytes, not a multiple of
// 16 -- so every access is a dword, in plain C++.
// session_commit_kernel: after the forward, theta[s] -> win[s][T-1][2048:] for the slots that advanced or joined; nothing else is written.
#include "../../include/tepose_amd.h"
#include "device.h"

namespace tepose {

constexpr int kSessionRows = 8;      // rows of its column a thread has in flight

__global__ void __launch_bounds__(256) session_advance_kernel(float* __restrict__ win, float* __restrict__ saved, int S, int T,
                                                               const int* __restrict__ ops, const float* __restrict__ feat,
                                                               const float* __restrict__ hist) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;           // column of the window row
  const int s = blockIdx.y;                                      // slot
  if (c >= kInput || s >= S) return;
  int op = ops[s];
  if (op < 1 || op > 3 || (op == 2 && !hist)) op = 0;
  if (op == 0 && !saved) return;
  const size_t base = (size_t)s * T * kInput + c;
  float* w = win + base;
  float* sv = saved ? saved + base : nullptr;
  const float* h = op == 2 ? hist + (size_t)s * (T - 1) * kInput + c : nullptr;
  const float newest = (op == 1 || op == 2) && c < kFeat ? feat[(size_t)s * kFeat + c] : 0.f;
  const bool read = saved || op == 1;
  float cur = read ? w[0] : 0.f;                                 // win[t][c] as it stood before the call
  for (int t0 = 0; t0 < T; t0 += kSessionRows) {
    // the loads of kSessionRows rows first (rows t0 + 1 .. t0 + kSessionRows: none of them written yet), then the stores of rows t0 .. : one
    // memory latency per group instead of one per row (a slot alone is 9 workgroups: nothing else hides it)
    float nxt[kSessionRows], hv[kSessionRows];
#pragma unroll
    for (int u = 0; u < kSessionRows; ++u) {
      const int t = t0 + u;
      nxt[u] = read && t + 1 < T ? w[(size_t)(t + 1) * kInput] : 0.f;
      hv[u] = op == 2 && t < T - 1 ? h[(size_t)t * kInput] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kSessionRows; ++u) {
      const int t = t0 + u;
      if (t < T) {
        const size_t o = (size_t)t * kInput;
        if (sv) sv[o] = cur;
        if (op != 0) w[o] = t == T - 1 ? newest : op == 1 ? nxt[u] : hv[u];      // (op 3: hv is 0)
        cur = nxt[u];
      }
    }
  }
}

__global__ void __launch_bounds__(128) session_commit_kernel(float* __restrict__ win, int S, int T, const int* __restrict__ ops,
                                                              const float* __restrict__ theta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;           // (slot, theta column)
  if (i >= S * kTheta) return;
  const int s = i / kTheta, c = i - s * kTheta;
  const int op = ops[s];
  if (op != 1 && op != 2) return;
  win[((size_t)s * T + (T - 1)) * kInput + kFeat + c] = theta[i];
}

}  // namespace tepose

using namespace tepose;

static int session_args(const void* win, const void* ops, const void* third, int S, int T) {
  if (!win || !ops || !third) return TEPOSE_E_ARG;
  if (S < 1 || S > kSessionMaxSlots || T < 2) return TEPOSE_E_SHAPE;
  return 0;
}

extern "C" int tepose_session_advance(float* win, float* saved, int S, int T, const int* ops, const float* feat, const float* hist,
                                      void* stream) {
  if (const int rc = session_args(win, ops, feat, S, T)) return rc;
  const Launch l = session_advance_shape(S);
  hipLaunchKernelGGL(session_advance_kernel, dim3(l.gx, l.gy, l.gz), dim3(l.threads), 0, (hipStream_t)stream, win, saved, S, T, ops, feat, hist);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// The filter step of a smoothing session: the kernel lives in filters.hip, next to the whole-sequence filter whose step function it shares.
extern "C" int tepose_session_smooth(const float* theta, const float* hist, int S, int T, const int* ops, float* state, float* saved_state,
                                     float min_cutoff, float beta, float d_cutoff, float* theta_hat, float* pose_hat, float* betas_hat, void* stream) {
  if (!theta_hat || !pose_hat || !betas_hat) return TEPOSE_E_ARG;
  for (const float v : {min_cutoff, beta, d_cutoff})
    if (!(v >= 0.f && v <= 3.402823466e38f)) return TEPOSE_E_ARG;      // NaN, an infinity, a negative value
  if (const int rc = session_args(theta, ops, state, S, T)) return rc;
  const hipError_t e = launch_session_smooth(theta, hist, S, T, ops, state, saved_state, min_cutoff, beta, d_cutoff, theta_hat, pose_hat, betas_hat,
                                             (hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int tepose_session_commit(float* win, int S, int T, const int* ops, const float* theta, void* stream) {
  if (const int rc = session_args(win, ops, theta, S, T)) return rc;
  const Launch l = session_commit_shape(S);
  hipLaunchKernelGGL(session_commit_kernel, dim3(l.gx, l.gy, l.gz), dim3(l.threads), 0, (hipStream_t)stream, win, S, T, ops, theta);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
