// Data movement around the convolution products of the HMR backbone (hmr.h): the im2col gather that makes a product's A operand, the two pooling
// kernels, and the pack-time fold of inference batch norm into the weights.  The products themselves are gemm_h3.hip / gemm.hip, unchanged.
#include "hmr.h"
#include "device.h"

namespace tepose {

namespace {


// Eight consecutive k of one output pixel's im2col row.  (r, s, c) order with c fastest: when C % 8 == 0 an octet is eight consecutive channels of
// one tap (two 16-byte loads per source); otherwise (the 3-channel stem) every element finds its own tap.  Taps outside the image and k >= K are zero.
template <bool NCHW>
__device__ __forceinline__ void load_octet(const GatherArgs& a, const float* x, const float* res, int relu, float* wb,
                                           int n, int ih0, int iw0, int k0, float v[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (!NCHW && (a.C & 7) == 0) {
    if (k0 >= a.K) return;
    const int tap = k0 / a.C, c0 = k0 - tap * a.C;
    const int r = tap / a.R, ih = ih0 + r, iw = iw0 + (tap - r * a.R);
    if (ih < 0 || ih >= a.H || iw < 0 || iw >= a.W) return;
    const long at = (((long)n * a.H + ih) * a.W + iw) * a.C + c0;
    const float4 p = *(const float4*)(x + at), q = *(const float4*)(x + at + 4);
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
    if (res) {
      const float4 rp = *(const float4*)(res + at), rq = *(const float4*)(res + at + 4);
      v[0] += rp.x; v[1] += rp.y; v[2] += rp.z; v[3] += rp.w; v[4] += rq.x; v[5] += rq.y; v[6] += rq.z; v[7] += rq.w;
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = v[i] > 0.f ? v[i] : (v[i] == v[i] ? 0.f : v[i]);      // NaN stays NaN
    }
    if (wb) {
      *(float4*)(wb + at) = float4{v[0], v[1], v[2], v[3]};
      *(float4*)(wb + at + 4) = float4{v[4], v[5], v[6], v[7]};
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    if (k >= a.K) continue;
    const int tap = k / a.C, c = k - tap * a.C;
    const int r = tap / a.R, ih = ih0 + r, iw = iw0 + (tap - r * a.R);
    if (ih < 0 || ih >= a.H || iw < 0 || iw >= a.W) continue;
    const long at = NCHW ? (((long)n * a.C + c) * a.H + ih) * a.W + iw : (((long)n * a.H + ih) * a.W + iw) * a.C + c;
    float t = x[at];
    if (res) t += res[at];
    if (relu) t = t > 0.f ? t : (t == t ? 0.f : t);
    if (wb) wb[at] = t;
    v[i] = t;
  }
}

// `lpr` lanes (a power of two, 8 .. 64) share one output pixel; a wave takes 64 / lpr pixels per trip.  SPLIT: first trip over the row finds its
// largest magnitude (and does the write-back), the second scales by the row's power of two and writes one 16-byte run per plane and octet; a row
// with a write-back is re-read from there (every element of a 1 x 1 stride-1 gather belongs to exactly one lane, so in-place joins are safe).
template <bool SPLIT, bool NCHW>
__global__ void __launch_bounds__(256) conv_gather_kernel(GatherArgs a, int lpr, long rows) {
  const int lane = threadIdx.x & 63, sub = lane & (lpr - 1), rpw = 64 / lpr;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const int NO = a.Kp >> 3;
  for (long row0 = wave * rpw; row0 < rows; row0 += nwaves * rpw) {           // wave-uniform trip count (the shuffles below need every lane)
    const long row = row0 + lane / lpr;
    const bool live = row < rows;
    const long pix = live ? row : rows - 1;
    const int n = (int)(pix / ((long)a.Ho * a.Wo));
    const int rem = (int)(pix - (long)n * a.Ho * a.Wo);
    const int oh = rem / a.Wo, ow = rem - oh * a.Wo;
    const int ih0 = oh * a.stride - a.pad, iw0 = ow * a.stride - a.pad;
    float v[8];
    if (!SPLIT) {
      if (!live) continue;
      for (int o = sub; o < NO; o += lpr) {
        load_octet<NCHW>(a, a.x, a.res, a.relu, a.wb, n, ih0, iw0, 8 * o, v);
        float* dst = a.out + row * a.Kp + 8 * o;
        *(float4*)dst = float4{v[0], v[1], v[2], v[3]};
        *(float4*)(dst + 4) = float4{v[4], v[5], v[6], v[7]};
      }
      continue;
    }
    float m = 0.f;
    bool bad = false;
    if (live)
      for (int o = sub; o < NO; o += lpr) {
        load_octet<NCHW>(a, a.x, a.res, a.relu, a.wb, n, ih0, iw0, 8 * o, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          m = fmaxf(m, fabsf(v[i]));                                            // fmaxf drops NaN: tracked separately
          bad |= !(fabsf(v[i]) <= 3.0e38f);
        }
      }
    int badi = bad ? 1 : 0;
    for (int off = 1; off < lpr; off <<= 1) {
      m = fmaxf(m, __shfl_xor(m, off));
      badi |= __shfl_xor(badi, off);
    }
    float sc = 1.f, inv = 1.f;
    if (m > 0.f && !badi) {
      int ex;
      (void)frexpf(m, &ex);                                                     // m = f * 2^ex, f in [0.5, 1)
      int e = 14 - ex;                                                          // m * 2^e in [2^13, 2^14)
      e = e > 100 ? 100 : (e < -100 ? -100 : e);
      sc = ldexpf(1.f, e);
      inv = ldexpf(1.f, -e);
    }
    if (!live) continue;
    if (sub == 0) a.row_scale[row] = inv;
    const float* src = a.wb ? a.wb : a.x;
    for (int o = sub; o < NO; o += lpr) {
      load_octet<NCHW>(a, src, a.wb ? nullptr : a.res, a.wb ? 0 : a.relu, nullptr, n, ih0, iw0, 8 * o, v);
      h16x8 h, l;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        half_t hh, ll;
        split_hi_lo(v[i] * sc, hh, ll);
        h[i] = hh; l[i] = ll;
      }
      const long off = plane_index(row, 8 * o, rows);
      *(h16x8*)(a.hi + off) = h;
      *(h16x8*)(a.lo + off) = l;
    }
  }
}

// padding contributes -inf; a thread takes 4 channels of one output pixel
__global__ void __launch_bounds__(256) maxpool3x3s2_kernel(const float* __restrict__ x, int N, int H, int W, int C, int Ho, int Wo,
                                                           float* __restrict__ y, int relu) {
  const int C4 = C >> 2;
  const long total = (long)N * Ho * Wo * C4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c4 = (int)(t % C4);
    long p = t / C4;
    const int ow = (int)(p % Wo); p /= Wo;
    const int oh = (int)(p % Ho);
    const int n = (int)(p / Ho);
    float4 m = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ih = 2 * oh - 1 + r;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int iw = 2 * ow - 1 + s;
        if (iw < 0 || iw >= W) continue;
        const float4 v = *(const float4*)(x + (((long)n * H + ih) * W + iw) * C + 4 * c4);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
    if (relu) { m.x = fmaxf(m.x, 0.f); m.y = fmaxf(m.y, 0.f); m.z = fmaxf(m.z, 0.f); m.w = fmaxf(m.w, 0.f); }
    *(float4*)(y + (((long)n * Ho + oh) * Wo + ow) * C + 4 * c4) = m;
  }
}

__global__ void __launch_bounds__(256) avgpool7_kernel(const float* __restrict__ x, const float* __restrict__ res, int relu, int N, int C,
                                                       float* __restrict__ y) {
  const long total = (long)N * C;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const long n = t / C;
    const int c = (int)(t - n * C);
    float acc = 0.f;
    for (int p = 0; p < 49; ++p) {
      const long at = (n * 49 + p) * C + c;
      float v = x[at];
      if (res) v += res[at];
      if (relu) v = fmaxf(v, 0.f);
      acc += v;
    }
    y[t] = acc * (1.f / 49.f);
  }
}

__global__ void __launch_bounds__(256) hmr_fold_pack_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ var, int cout, int cin, int R,
                                                            float* __restrict__ dst, int Np, int Kp, float* __restrict__ bias_out, int* err) {
  const int K = cin * R * R;
  const long total = (long)Np * Kp;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int co = (int)(t / Kp), k = (int)(t - (long)co * Kp);
    if (co >= cout) { dst[t] = 0.f; continue; }
    double sc = 1.0;
    bool bad = false;
    if (gamma) {
      const double d = (double)var[co] + kBnEps;
      bad = !(d > 0.0);
      sc = bad ? 0.0 : (double)gamma[co] / sqrt(d);
    }
    float o = 0.f;
    if (k < K) {
      const int tap = k / cin, c = k - tap * cin, r = tap / R, s = tap - r * R;
      o = (float)((double)w[(((long)co * cin + c) * R + r) * R + s] * sc);
    }
    if (k == 0) {
      const float b = (float)((beta ? (double)beta[co] : 0.0) - (gamma ? (double)mean[co] * sc : 0.0));
      bias_out[co] = b;
      bad |= !(fabsf(b) <= 3.0e38f);
    }
    bad |= !(fabsf(o) <= 3.0e38f);
    if (bad) atomicOr(err, 1);
    dst[t] = o;
  }
}

inline int grid_for(long items, int per_block) {
  const long want = (items + per_block - 1) / per_block;
  return (int)(want < 1 ? 1 : (want < 16384 ? want : 16384));
}

}  // namespace

hipError_t launch_conv_gather(const GatherArgs& a, bool split, hipStream_t s) {
  const long rows = (long)a.N * a.Ho * a.Wo;
  if (rows <= 0) return hipSuccess;
  if ((a.Kp & 31) || a.K > a.Kp || a.K != a.C * a.R * a.R) return hipErrorInvalidValue;
  if (a.wb && (a.R != 1 || a.stride != 1 || a.pad != 0 || a.nchw)) return hipErrorInvalidValue;   // an element must belong to one lane
  if (a.nchw && a.res) return hipErrorInvalidValue;
  int lpr = 8;
  while (lpr < 64 && 2 * lpr <= a.Kp / 8) lpr *= 2;
  const dim3 grid(grid_for(rows, 4 * (64 / lpr))), block(256);
  if (split) {
    if (a.nchw) hipLaunchKernelGGL((conv_gather_kernel<true, true>), grid, block, 0, s, a, lpr, rows);
    else hipLaunchKernelGGL((conv_gather_kernel<true, false>), grid, block, 0, s, a, lpr, rows);
  } else {
    if (a.nchw) hipLaunchKernelGGL((conv_gather_kernel<false, true>), grid, block, 0, s, a, lpr, rows);
    else hipLaunchKernelGGL((conv_gather_kernel<false, false>), grid, block, 0, s, a, lpr, rows);
  }
  return hipGetLastError();
}

hipError_t launch_maxpool3x3s2(const float* x, int N, int H, int W, int C, float* y, int relu, hipStream_t s) {
  if (C & 3) return hipErrorInvalidValue;
  const int Ho = conv_out_size(H, 3, 2, 1), Wo = conv_out_size(W, 3, 2, 1);
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid_for((long)N * Ho * Wo * (C / 4), 256)), dim3(256), 0, s, x, N, H, W, C, Ho, Wo, y, relu);
  return hipGetLastError();
}

hipError_t launch_avgpool7(const float* x, const float* res, int relu, int N, int C, float* y, hipStream_t s) {
  hipLaunchKernelGGL(avgpool7_kernel, dim3(grid_for((long)N * C, 256)), dim3(256), 0, s, x, res, relu, N, C, y);
  return hipGetLastError();
}

hipError_t launch_hmr_fold_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int cout, int cin, int R,
                                float* dst, int Np, int Kp, float* bias_out, int* err, hipStream_t s) {
  hipLaunchKernelGGL(hmr_fold_pack_kernel, dim3(grid_for((long)Np * Kp, 256)), dim3(256), 0, s, w, gamma, beta, mean, var, cout, cin, R, dst, Np, Kp,
                     bias_out, err);
  return hipGetLastError();
}

}  // namespace tepose
