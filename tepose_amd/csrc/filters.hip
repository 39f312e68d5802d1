// Temporal post-filters, both first-order recursions over the frames of one
// sequence: the OneEuro filter on the 72 axis-angle components (lib/utils/one_euro_filter.py,
// lib/utils/smooth_pose.py:24-67) and the MEVA-style quaternion slerp smoothing of the 24 joint
// rotations (evaluate.py:32-59 over lib/utils/slerp_filter_utils.py).  One thread per component /
// per joint walks the frames in order; neighbouring threads touch neighbouring addresses, so
// every step is one coalesced row read and one row write.
#include "common.h"

namespace tepose {

// One step of the OneEuro recursion at t_e = 1: (x_t, x^_{t-1}, dx^_{t-1}) -> (x^_t, dx^_t), for the whole-sequence kernel and for the per-tick
// kernel of a live session.  The expression is
//     rd = 2 pi d_cutoff;  a_d = rd / (rd + 1);  dx = x_t - x^_{t-1};  dx^_t = a_d dx + (1 - a_d) dx^_{t-1}
//     cutoff = min_cutoff + beta |dx^_t|;  r = 2 pi cutoff;  a = r / (r + 1);  x^_t = a x_t + (1 - a) x^_{t-1}
// and the roundings are spelled out -- contraction off, each fused multiply-add named -- exactly as one_euro_kernel has always been compiled (where
// the compiler chose them, inside its loop): left to the compiler, the same source contracts differently from one call site to the next (in a function
// of its own it fused a_d dx instead of (1 - a_d) dx^), and a session's pose_hat has to equal tepose_filter_one_euro over the same rows in every bit.
struct OneEuro { float x, dx; };
__device__ __forceinline__ OneEuro one_euro_step(float xi, float x_prev, float dx_prev, float min_cutoff, float beta, float d_cutoff) {
#pragma clang fp contract(off)
  const float two_pi = 6.283185307179586f;
  const float rd = two_pi * d_cutoff;
  const float a_d = rd / __builtin_fmaf(d_cutoff, two_pi, 1.f);
  const float dx = xi - x_prev;
  const float dx_hat = __builtin_fmaf(1.f - a_d, dx_prev, a_d * dx);
  const float cutoff = __builtin_fmaf(beta, fabsf(dx_hat), min_cutoff);
  const float r = two_pi * cutoff;
  const float a = r / __builtin_fmaf(cutoff, two_pi, 1.f);
  const float x_hat = __builtin_fmaf(xi, a, (1.f - a) * x_prev);
  return OneEuro{x_hat, dx_hat};
}

// x[N][D] in place; frame 0 passes through; timestamps are the frame indices (t_e = 1).
__global__ void __launch_bounds__(128) one_euro_kernel(float* __restrict__ x, int N, int D, float min_cutoff,
                                                       float beta, float d_cutoff) {
  const int d = blockIdx.x * 128 + threadIdx.x;
  if (d >= D) return;
  OneEuro f{x[d], 0.f};
  for (int i = 1; i < N; ++i) {
    f = one_euro_step(x[(long)i * D + d], f.x, f.dx, min_cutoff, beta, d_cutoff);
    x[(long)i * D + d] = f.x;
  }
}

hipError_t launch_one_euro(float* x, int N, int D, float min_cutoff, float beta, float d_cutoff, hipStream_t s) {
  if (N <= 1 || D <= 0) return hipSuccess;
  hipLaunchKernelGGL(one_euro_kernel, dim3((D + 127) / 128), dim3(128), 0, s, x, N, D, min_cutoff, beta, d_cutoff);
  return hipGetLastError();
}

// The same filter inside the tick of a live session (include/tepose_amd.h tepose_session_smooth): per slot a state
// (x^, dx^) of 2 x 72 floats, advanced by the slot's op code.  One thread per (slot, theta column); columns 3 .. 74 are the pose components, the other
// 13 (cam, betas) are copied.  A slot whose op is neither 1 nor 2 reads neither theta nor hist and gets zero rows (pose 0, betas 0: SMPL's rest pose).
// No LDS, no barrier; every store is a dword in plain C++.
__global__ void __launch_bounds__(128) session_smooth_kernel(const float* __restrict__ theta, const float* __restrict__ hist, int S, int T,
                                                              const int* __restrict__ ops, float* __restrict__ state, float* __restrict__ saved,
                                                              float min_cutoff, float beta, float d_cutoff, float* __restrict__ theta_hat,
                                                              float* __restrict__ pose_hat, float* __restrict__ betas_hat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;           // (slot, theta column)
  if (i >= S * kTheta) return;
  const int s = i / kTheta, c = i - s * kTheta;
  int op = ops[s];
  if (op < 1 || op > 3 || (op == 2 && !hist)) op = 0;
  const bool live = op == 1 || op == 2;
  if (c < 3 || c >= 75) {                                        // cam / betas: bit copies
    const float v = live ? theta[i] : 0.f;
    theta_hat[i] = v;
    if (c >= 75) betas_hat[s * 10 + (c - 75)] = v;
    return;
  }
  const int k = c - 3;                                           // pose component
  float* st = state + (size_t)s * 144 + k;                       // st[0] = x^, st[72] = dx^
  if (saved) {
    saved[(size_t)s * 144 + k] = st[0];
    saved[(size_t)s * 144 + 72 + k] = st[72];
  }
  float out = 0.f;
  if (live) {
    OneEuro f;
    if (op == 1) {
      f = OneEuro{st[0], st[72]};
    } else {                                                     // join: the filter starts at the first history row, as a tracklet's does
      const float* h = hist + (size_t)s * (T - 1) * kInput + kFeat + c;
      f = OneEuro{h[0], 0.f};
      for (int t = 1; t < T - 1; ++t) f = one_euro_step(h[(size_t)t * kInput], f.x, f.dx, min_cutoff, beta, d_cutoff);
    }
    f = one_euro_step(theta[i], f.x, f.dx, min_cutoff, beta, d_cutoff);
    st[0] = f.x;
    st[72] = f.dx;
    out = f.x;
  } else if (op == 3) {
    st[0] = 0.f;
    st[72] = 0.f;
  }
  theta_hat[i] = out;
  pose_hat[s * 72 + k] = out;
}

hipError_t launch_session_smooth(const float* theta, const float* hist, int S, int T, const int* ops, float* state, float* saved, float min_cutoff,
                                 float beta, float d_cutoff, float* theta_hat, float* pose_hat, float* betas_hat, hipStream_t s) {
  const Launch l = session_smooth_shape(S);
  hipLaunchKernelGGL(session_smooth_kernel, grid_of(l), block_of(l), 0, s, theta, hist, S, T, ops, state, saved, min_cutoff, beta, d_cutoff, theta_hat,
                     pose_hat, betas_hat);
  return hipGetLastError();
}

__device__ __forceinline__ void mat_to_quat(const float* R, double q[4]) {   // wxyz, Shepperd's branches
  const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7],
               m22 = R[8];
  const double tr = m00 + m11 + m22;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (m21 - m12) / s; q[2] = (m02 - m20) / s; q[3] = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = sqrt(1.0 + m00 - m11 - m22) * 2.0;
    q[0] = (m21 - m12) / s; q[1] = 0.25 * s; q[2] = (m01 + m10) / s; q[3] = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = sqrt(1.0 + m11 - m00 - m22) * 2.0;
    q[0] = (m02 - m20) / s; q[1] = (m01 + m10) / s; q[2] = 0.25 * s; q[3] = (m12 + m21) / s;
  } else {
    const double s = sqrt(1.0 + m22 - m00 - m11) * 2.0;
    q[0] = (m10 - m01) / s; q[1] = (m02 + m20) / s; q[2] = (m12 + m21) / s; q[3] = 0.25 * s;
  }
  // The reference (transformations.quaternion_from_matrix, isprecise=False) returns the dominant
  // eigenvector of the symmetric matrix K(R) -- the best-fit quaternion when R is not exactly
  // orthonormal.  K/3 has eigenvalues {1, -1/3, -1/3, -1/3} for a rotation, so K/3 + I/3 is rank one up
  // to the input's non-orthonormality and two power steps from the Shepperd start converge to it.
  double v[4] = {q[1], q[2], q[3], q[0]};                     // (x, y, z, w)
  const double K[4][4] = {
      {(m00 - m11 - m22) / 3 + 1.0 / 3, (m01 + m10) / 3, (m02 + m20) / 3, (m21 - m12) / 3},
      {(m01 + m10) / 3, (m11 - m00 - m22) / 3 + 1.0 / 3, (m12 + m21) / 3, (m02 - m20) / 3},
      {(m02 + m20) / 3, (m12 + m21) / 3, (m22 - m00 - m11) / 3 + 1.0 / 3, (m10 - m01) / 3},
      {(m21 - m12) / 3, (m02 - m20) / 3, (m10 - m01) / 3, (m00 + m11 + m22) / 3 + 1.0 / 3}};
  for (int it = 0; it < 2; ++it) {
    double u[4], n = 0.0;
    for (int a = 0; a < 4; ++a) { u[a] = K[a][0] * v[0] + K[a][1] * v[1] + K[a][2] * v[2] + K[a][3] * v[3]; n += u[a] * u[a]; }
    n = sqrt(n);
    for (int a = 0; a < 4; ++a) v[a] = u[a] / n;
  }
  q[0] = v[3]; q[1] = v[0]; q[2] = v[1]; q[3] = v[2];
}

__device__ __forceinline__ void quat_to_mat(const double qin[4], float* R) {  // quaternion_matrix()
  const double n = qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3];
  if (n < 8.881784197001252e-16) {
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.f : 0.f;
    return;
  }
  const double sc = sqrt(2.0 / n);
  const double w = qin[0] * sc, x = qin[1] * sc, y = qin[2] * sc, z = qin[3] * sc;
  R[0] = (float)(1.0 - y * y - z * z); R[1] = (float)(x * y - z * w); R[2] = (float)(x * z + y * w);
  R[3] = (float)(x * y + z * w); R[4] = (float)(1.0 - x * x - z * z); R[5] = (float)(y * z - x * w);
  R[6] = (float)(x * z - y * w); R[7] = (float)(y * z + x * w); R[8] = (float)(1.0 - x * x - y * y);
}

// in/out [N][J][3][3]; thread = joint.  c_t: sign-corrected quaternion of frame t (quat_correct),
// s_t = slerp(s_{t-1}, c_t, ratio) (quat_smooth), out_t = matrix(s_t).
__global__ void __launch_bounds__(64) slerp_smooth_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          int N, int J, double ratio) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= J) return;
  const double eps = 8.881784197001252e-16;               // numpy.finfo(float).eps * 4
  double c_prev[4], s_prev[4];
  for (int t = 0; t < N; ++t) {
    double q[4];
    mat_to_quat(in + ((long)t * J + j) * 9, q);
    if (t == 0) {
      for (int k = 0; k < 4; ++k) { c_prev[k] = q[k]; s_prev[k] = q[k]; }
    } else {
      double dm = 0.0, dp = 0.0;
      for (int k = 0; k < 4; ++k) { dm += (c_prev[k] - q[k]) * (c_prev[k] - q[k]); dp += (c_prev[k] + q[k]) * (c_prev[k] + q[k]); }
      if (dm > dp)
        for (int k = 0; k < 4; ++k) q[k] = -q[k];
      for (int k = 0; k < 4; ++k) c_prev[k] = q[k];
      // quaternion_slerp(s_prev, q, ratio), spin = 0, shortest path
      double q0[4], q1[4], n0 = 0.0, n1 = 0.0;
      for (int k = 0; k < 4; ++k) { n0 += s_prev[k] * s_prev[k]; n1 += q[k] * q[k]; }
      n0 = sqrt(n0); n1 = sqrt(n1);
      for (int k = 0; k < 4; ++k) { q0[k] = s_prev[k] / n0; q1[k] = q[k] / n1; }
      double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
      if (!(fabs(fabs(d) - 1.0) < eps) && ratio != 0.0) {
        if (ratio == 1.0) {
          for (int k = 0; k < 4; ++k) q0[k] = q1[k];
        } else {
          if (d < 0.0) { d = -d; for (int k = 0; k < 4; ++k) q1[k] = -q1[k]; }
          const double ang = acos(d);
          if (!(fabs(ang) < eps)) {
            const double isin = 1.0 / sin(ang);
            const double a = sin((1.0 - ratio) * ang) * isin, b = sin(ratio * ang) * isin;
            for (int k = 0; k < 4; ++k) q0[k] = q0[k] * a + q1[k] * b;
          }
        }
      }
      for (int k = 0; k < 4; ++k) s_prev[k] = q0[k];
    }
    quat_to_mat(s_prev, out + ((long)t * J + j) * 9);
  }
}

hipError_t launch_slerp_smooth(const float* in, float* out, int N, int J, double ratio, hipStream_t s) {
  if (N <= 0 || J <= 0) return hipSuccess;
  hipLaunchKernelGGL(slerp_smooth_kernel, dim3((J + 63) / 64), dim3(64), 0, s, in, out, N, J, ratio);
  return hipGetLastError();
}

}  // namespace tepose
