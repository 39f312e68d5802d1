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
// Two kernels share that pixel: crop_frames_u8_kernel takes each crop's map (minv, made on the host), crop_boxes_u8_kernel takes each crop's BOX and
// forms the map itself (boxes are per-tick data of a live session whose graph never changes).
#include "../../include/tepose_amd.h"
#include "common.h"

namespace tepose {

// One crop pixel: p = v * S + u of crop i, sampled from frame fi through the map m (six fp64 entries, in registers), quantised, normalised and stored.
// The body both kernels share: a crop cut from a box equals, bit for bit, the crop cut from that box's host-made map.
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ frames, int F, int H, int W, int fi, const double (&m)[6], int i, int p, int u, int v,
                                           int S, float* __restrict__ out, uint8_t* __restrict__ raw) {
  const double x = fma(m[0], (double)u, fma(m[1], (double)v, m[2]));
  const double y = fma(m[3], (double)u, fma(m[4], (double)v, m[5]));
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

__global__ void __launch_bounds__(kCropBlock) crop_frames_u8_kernel(const uint8_t* __restrict__ frames, int F, int H, int W,
                                                                     const int* __restrict__ frame_index, const double* __restrict__ minv,
                                                                     int n, int S, float* __restrict__ out, uint8_t* __restrict__ raw) {
  const int p = blockIdx.x * kCropBlock + threadIdx.x;          // pixel of the crop, row-major
  if (p >= S * S) return;
  const int v = p / S, u = p - v * S;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const double* mi = minv + (size_t)i * 6;
    const double m[6] = {mi[0], mi[1], mi[2], mi[3], mi[4], mi[5]};
    crop_pixel(frames, F, H, W, frame_index[i], m, i, p, u, v, S, out, raw);
  }
}

// The box -> map rule of tepose_amd.crop.crop_transform followed by invert_affine, operation for operation in fp64: every product, sum and
// quotient is rounded on its own (no contraction; `/` is IEEE division under the project's flags), the three source points go through float32
// as the reference stores them.  b = (c_x, c_y, w, h).  A degenerate box (w = 0, NaN) yields non-finite entries; nothing here tests for it.
__device__ __forceinline__ void box_to_minv(const double* __restrict__ b, double scale, int S, double (&m)[6]) {
#pragma clang fp contract(off)
  const double cx = b[0], cy = b[1], w = b[2], h = b[3];
  const double sx = (double)(float)cx, sy = (double)(float)cy;
  const double dx = (double)(float)(cx + (double)(float)((w * scale) * 0.5)) - sx;
  const double dy = (double)(float)(cy + (double)(float)((h * scale) * 0.5)) - sy;
  const double dc = (double)(float)((double)S * 0.5);
  const double dd = (double)(float)(dc + dc) - dc;
  // M = [[a, 0, dc - a sx], [0, d, dc - d sy]]
  const double M00 = dd / dx, M11 = dd / dy, M01 = 0.0, M10 = 0.0;
  const double M02 = dc - M00 * sx, M12 = dc - M11 * sy;
  // cv2.warpAffine's inversion: determinant, adjugate, translation
  const double det = M00 * M11 - M01 * M10;
  const double D = det != 0.0 ? 1.0 / det : 0.0;
  m[0] = M11 * D;
  m[4] = M00 * D;
  m[1] = M01 * -D;
  m[3] = M10 * -D;
  m[2] = -m[0] * M02 - m[1] * M12;
  m[5] = -m[3] * M02 - m[4] * M12;
}

// Crops from boxes: as crop_frames_u8_kernel, but every thread forms its crop's map from the box in registers (three fp64
// divisions per thread: nothing next to 12 byte loads), and with `ops` a row whose code is neither 1 nor 2 reads neither box nor frame index nor
// frame and stores the all-zero crop.  minv_out (tests): the first thread of a crop stores the map it used, six zeros for a gated-off row.
__global__ void __launch_bounds__(kCropBlock) crop_boxes_u8_kernel(const uint8_t* __restrict__ frames, int F, int H, int W,
                                                                    const int* __restrict__ frame_index, const double* __restrict__ boxes,
                                                                    double scale, const int* __restrict__ ops, int n, int S,
                                                                    float* __restrict__ out, uint8_t* __restrict__ raw, double* __restrict__ minv_out) {
  const int p = blockIdx.x * kCropBlock + threadIdx.x;          // pixel of the crop, row-major
  if (p >= S * S) return;
  const int v = p / S, u = p - v * S;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    double m[6] = {0., 0., 0., 0., 0., 0.};
    int fi = -1;                                                 // outside [0, F): the all-zero crop, nothing read
    bool on = true;
    if (ops) {
      const int op = ops[i];
      on = op == 1 || op == 2;
    }
    if (on) {
      box_to_minv(boxes + (size_t)i * 4, scale, S, m);
      fi = frame_index[i];
    }
    if (minv_out && p == 0)
      for (int k = 0; k < 6; ++k) minv_out[(size_t)i * 6 + k] = m[k];
    crop_pixel(frames, F, H, W, fi, m, i, p, u, v, S, out, raw);
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
  const Launch l = crop_shape(S, n);
  hipLaunchKernelGGL(crop_frames_u8_kernel, dim3(l.gx, l.gy, l.gz), dim3(l.threads), 0, (hipStream_t)stream, frames, F, H, W, frame_index, minv, n, S,
                     out_nchw, raw_nhwc);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int tepose_crop_boxes_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const double* boxes, double scale,
                                    const int* ops, int n, int S, float* out_nchw, uint8_t* raw_nhwc, double* minv_out, void* stream) {
  if (n < 0 || S < 1 || H < 1 || W < 1 || F < 1 || (!out_nchw && !raw_nhwc)) return TEPOSE_E_ARG;
  if (n > 0 && (!frames || !frame_index || !boxes)) return TEPOSE_E_ARG;
  if (!(scale > 0.0) || scale > 1.7976931348623157e308) return TEPOSE_E_ARG;      // NaN, <= 0, +inf
  if (S > kCropMaxSide || n > kSessionMaxSlots) return TEPOSE_E_SHAPE;
  if (n == 0) return 0;
  const Launch l = crop_shape(S, n);
  hipLaunchKernelGGL(crop_boxes_u8_kernel, dim3(l.gx, l.gy, l.gz), dim3(l.threads), 0, (hipStream_t)stream, frames, F, H, W, frame_index, boxes, scale,
                     ops, n, S, out_nchw, raw_nhwc, minv_out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
