// Person crops of video frames, on the device: what the reference's CropDataset does per frame on CPU workers
// (lib/dataset/inference.py:58-74 over lib/data_utils/_img_utils.py:53-101,219-252,322-330) -- cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT)
// of the uint8 RGB frame by the bounding box's affine, ToTensor, ImageNet Normalize -- for all crops of a call in one launch.  The frames
// stay uint8 on the device; no image exists on the host in float.
//
// Semantics (the definition the tests pin, tests/_crop_ref.py):
//   crop pixel (u, v), integer coordinates at pixel centres, samples the frame at  x = m0 u + m1 v + m2,  y = m3 u + m4 v + m5  (minv row);
//   the coordinates, their floors and the fractions fx = x - floor(x), fy = y - floor(y) are fp64 -- an fp32 coordinate near x = 1900 is off
//   by ~1e-4 px, 0.03 grey levels on a steep edge; everything after that is fp32;
//   each of the four taps outside [0, W) x [0, H) contributes 0 on its own (BORDER_CONSTANT 0; no clamping);
//   raw = floor(bilinear + 0.5) as uint8 (the network sees 8-bit values in the reference: quantise, then normalise);
//   out[c] = (raw / 255 - mean[c]) / std[c] in fp32.
// One thread per crop pixel handles its three channels: 2 x 6 adjacent source bytes in, three planes out, coalesced along u.  Frame rows are
// W * 3 bytes -- generally not dword-aligned -- so the taps are byte loads.
#include "../../include/tepose_amd.h"
#include "common.h"

namespace tepose {

constexpr int kCropBlock = 256;
constexpr int kCropMaxSide = 32768;   // S * S stays below 2^31; blocks per crop below 2^22

__global__ void __launch_bounds__(kCropBlock) crop_frames_u8_kernel(const uint8_t* __restrict__ frames, int F, int H, int W,
                                                                     const int* __restrict__ frame_index, const double* __restrict__ minv,
                                                                     int n, int S, float* __restrict__ out, uint8_t* __restrict__ raw) {
  const int p = blockIdx.x * kCropBlock + threadIdx.x;          // pixel of the crop, row-major
  if (p >= S * S) return;
  const int v = p / S, u = p - v * S;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const double* m = minv + (size_t)i * 6;
    const double x = fma(m[0], (double)u, fma(m[1], (double)v, m[2]));
    const double y = fma(m[3], (double)u, fma(m[4], (double)v, m[5]));
    const int fi = frame_index[i];
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    // a tap column / row can be inside only for -1 < x < W, -1 < y < H (also false for NaN); a frame index outside [0, F) reads nothing
    if (fi >= 0 && fi < F && x > -1.0 && x < (double)W && y > -1.0 && y < (double)H) {
      const double xf = floor(x), yf = floor(y);
      const int x0 = (int)xf, y0 = (int)yf;                      // in [-1, W - 1] x [-1, H - 1]
      const float fx = (float)(x - xf), fy = (float)(y - yf);
      const uint8_t* fr = frames + (size_t)fi * H * W * 3;
      const bool cx0 = x0 >= 0, cx1 = x0 + 1 < W, ry0 = y0 >= 0, ry1 = y0 + 1 < H;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
      if (ry0) {
        const uint8_t* q = fr + ((long)y0 * W + x0) * 3;       // q + 0..2 is only read when cx0, q + 3..5 only when cx1
        if (cx0) { a0 = q[0]; a1 = q[1]; a2 = q[2]; }
        if (cx1) { b0 = q[3]; b1 = q[4]; b2 = q[5]; }
      }
      if (ry1) {
        const uint8_t* q = fr + ((long)(y0 + 1) * W + x0) * 3;
        if (cx0) { c0 = q[0]; c1 = q[1]; c2 = q[2]; }
        if (cx1) { d0 = q[3]; d1 = q[4]; d2 = q[5]; }
      }
      const float t0 = a0 + fx * (b0 - a0), t1 = a1 + fx * (b1 - a1), t2 = a2 + fx * (b2 - a2);
      const float s0 = c0 + fx * (d0 - c0), s1 = c1 + fx * (d1 - c1), s2 = c2 + fx * (d2 - c2);
      r0 = fminf(floorf(t0 + fy * (s0 - t0) + 0.5f), 255.f);
      r1 = fminf(floorf(t1 + fy * (s1 - t1) + 0.5f), 255.f);
      r2 = fminf(floorf(t2 + fy * (s2 - t2) + 0.5f), 255.f);
    }
    if (raw) {
      uint8_t* q = raw + ((size_t)i * S * S + p) * 3;
      q[0] = (uint8_t)r0; q[1] = (uint8_t)r1; q[2] = (uint8_t)r2;
    }
    if (out) {
      float* q = out + (size_t)i * 3 * S * S + p;
      const size_t plane = (size_t)S * S;
      q[0] = (r0 / 255.f - 0.485f) / 0.229f;                     // _img_utils.py:322-330
      q[plane] = (r1 / 255.f - 0.456f) / 0.224f;
      q[2 * plane] = (r2 / 255.f - 0.406f) / 0.225f;
    }
  }
}

}  // namespace tepose

using namespace tepose;

extern "C" int tepose_crop_frames_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const double* minv, int n, int S,
                                     float* out_nchw, uint8_t* raw_nhwc, void* stream) {
  if (n < 0 || S < 1 || H < 1 || W < 1 || F < 1 || (!out_nchw && !raw_nhwc)) return TEPOSE_E_ARG;
  if (n > 0 && (!frames || !frame_index || !minv)) return TEPOSE_E_ARG;
  if (S > kCropMaxSide) return TEPOSE_E_SHAPE;
  if (n == 0) return 0;
  const dim3 grid((unsigned)(((long)S * S + kCropBlock - 1) / kCropBlock), (unsigned)(n < 65535 ? n : 65535));
  hipLaunchKernelGGL(crop_frames_u8_kernel, grid, dim3(kCropBlock), 0, (hipStream_t)stream, frames, F, H, W, frame_index, minv, n, S, out_nchw,
                     raw_nhwc);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
