// SMPL overlay rasteriser, on the device: what the reference's Renderer.render does per person and frame with pyrender,
// trimesh and an OpenGL context (lib/utils/renderer.py:36-121, called from demo.py:390-417) -- here three passes of plain HIP over uint8 frames
// that already sit on the device.  No pyrender output exists to compare with: the kernels are pinned to the definition below
// (tests/_render_ref.py restates it in numpy fp64); the distance to pyrender's own fragment shader is not measured.
//
// Semantics:
//   vertex (x, y, z), camera (sx, sy, tx, ty), rotation R (row-major 3 x 3, identity when absent), all fp64, no contraction into fma:
//     flip (x, -y, -z) (renderer.py:68-69); rotate: xr = (R0 x + R1 y') + R2 z' and so on; X = sx (xr + tx), Y = sy (yr - ty), d = -zr (:26-33);
//     px = (X + 1) (W / 2), py = (1 - Y) (H / 2), row 0 on top, the centre of pixel (c, r) at (c + 1/2, r + 1/2);
//     snap: ix = floor(256 px + 1/2), iy alike, int32; d is stored in fp32.  A vertex that is not finite or beyond +-2^20 px is invalid.
//   triangle (v0, v1, v2) on snapped coordinates, int64: A = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0); kept only for A < 0 (counter-clockwise in
//     NDC: front-facing), with three valid vertices and three indices in [0, V).
//   coverage of a pixel centre p: E_i = the edge function of the edge opposite vertex i (walked v1->v2, v2->v0, v0->v1), E_0 + E_1 + E_2 = A;
//     inside when every E_i < 0, or E_i == 0 on an edge that owns its points: dy > 0 (a left edge), or dy == 0 and dx < 0 (a top edge).
//   depth: b_i = (float)(-E_i) / (float)(-A), d = (b_0 d_0 + b_1 d_1) + b_2 d_2 in fp32 (no fma), kept for -1 <= d < 1; inside one instance the
//     smallest d wins, the smaller face index on equal d; a later instance of the call overwrites an earlier one whatever the depths.
//   shading: vertex normal = the sum over the vertex' faces (ascending face index, from the caller's adjacency) of (p1 - p0) x (p2 - p0) on the
//     flipped and rotated positions, summed and normalised in fp64 (more than the definition's fp32 asks; no atomics: bit-reproducible), stored
//     fp32; a zero sum stays zero.  Fragment: n = sum b_i n_i, normalised, lambda = max(0, n_z); colour = clamp(base (0.3 + (2.4 / pi) lambda)
//     + 0.1, 0, 1) (three directional lights of 0.8 along the view axis, ambient 0.3, Lambert base / pi, emissive 0.1: renderer.py:50-63,91-99);
//     out = floor(255 colour + 1/2) as uint8.  An uncovered pixel keeps the frame's value (:114-115).
//
// Mapping: (a) one thread per (instance, vertex): transform, snap, normal -> 24-byte record in the workspace; (b) one thread per (instance, face):
// small clamped boxes are walked by that thread, larger ones are handed through LDS to the whole workgroup; every covered centre does one 64-bit
// atomicMin on the pixel's key  (4095 - instance) << 52 | monotone(d) << 20 | face,  so the plane's final content does not depend on scheduling;
// (c) one thread per pixel decodes the key, recomputes the barycentrics from the stored records, shades and writes three bytes (rows are W * 3
// bytes, not dword-aligned in general).  The rate of 64-bit atomicMin on this chip is not measured; profiles/render_frames.txt times the pass.
#include "../../include/tepose_amd.h"
#include "common.h"

namespace tepose {

constexpr int kRenderBlock = 256;
constexpr int kRenderMaxSide = 16384;          // H * W <= 2^28: pixel indices of one frame fit an int
constexpr int kRenderFaceBits = 20;
constexpr int kRenderMaxFaces = 1 << kRenderFaceBits;
constexpr int kRenderMaxVerts = 1 << 20;
constexpr int kRenderMaxInstances = 4096;      // 12 key bits
constexpr int kRenderSmallBox = 64;            // pixels of a clamped box one thread walks alone; larger boxes go to the workgroup
constexpr int kRenderInvalid = 0x7fffffff;
constexpr unsigned long long kRenderEmpty = ~0ull;

struct RenderVertex {
  int ix, iy;          // 1/256 px; ix == kRenderInvalid: not drawable
  float d, nx, ny, nz;
};

struct RenderTri {
  int x0, y0, x1, y1, x2, y2;
  float d0, d1, d2;
  int c0, c1, r0, r1;  // clamped pixel box, inclusive
  unsigned long long key_hi;   // instance and face parts of the key
  size_t plane;        // first key of the frame
};

__device__ inline unsigned monotone_u32(float d) {          // order-preserving image of a finite float
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float monotone_inverse(unsigned m) { return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m); }

__device__ inline bool edge_owns(int dx, int dy) { return dy > 0 || (dy == 0 && dx < 0); }

// -E_i >= 0 inside, for the centre of pixel (c, r); false when the centre is outside or on an edge that does not own it
__device__ inline bool cover(const RenderTri& t, int c, int r, long long& w0, long long& w1, long long& w2) {
  const long long px = (long long)c * 256 + 128, py = (long long)r * 256 + 128;
  const long long e0 = (long long)(t.x2 - t.x1) * (py - t.y1) - (long long)(t.y2 - t.y1) * (px - t.x1);
  const long long e1 = (long long)(t.x0 - t.x2) * (py - t.y2) - (long long)(t.y0 - t.y2) * (px - t.x2);
  const long long e2 = (long long)(t.x1 - t.x0) * (py - t.y0) - (long long)(t.y1 - t.y0) * (px - t.x0);
  if (e0 > 0 || e1 > 0 || e2 > 0) return false;
  if (e0 == 0 && !edge_owns(t.x2 - t.x1, t.y2 - t.y1)) return false;
  if (e1 == 0 && !edge_owns(t.x0 - t.x2, t.y0 - t.y2)) return false;
  if (e2 == 0 && !edge_owns(t.x1 - t.x0, t.y1 - t.y0)) return false;
  w0 = -e0; w1 = -e1; w2 = -e2;
  return true;
}

__device__ inline void barycentrics(long long w0, long long w1, long long w2, float& b0, float& b1, float& b2) {
  const float a = (float)(w0 + w1 + w2);                 // -A > 0
  b0 = (float)w0 / a; b1 = (float)w1 / a; b2 = (float)w2 / a;
}

__device__ inline void draw_pixel(const RenderTri& t, int c, int r, int W, unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
  long long w0, w1, w2;
  if (!cover(t, c, r, w0, w1, w2)) return;
  float b0, b1, b2;
  barycentrics(w0, w1, w2, b0, b1, b2);
  float d = (b0 * t.d0 + b1 * t.d1) + b2 * t.d2;
  d += 0.0f;                                              // -0 -> +0: one image per value
  if (!(d >= -1.0f && d < 1.0f)) return;                 // the clip planes of an orthographic projection; also false for NaN
  atomicMin(keys + t.plane + (size_t)r * W + c, t.key_hi | ((unsigned long long)monotone_u32(d) << kRenderFaceBits));
}

// (a) ------------------------------------------------------------------------------------------------------------------------------------------
__device__ inline void place(const float* __restrict__ P, int u, const double* R, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  const double a = (double)P[3 * (size_t)u], b = -(double)P[3 * (size_t)u + 1], c = -(double)P[3 * (size_t)u + 2];
  x = (R[0] * a + R[1] * b) + R[2] * c;
  y = (R[3] * a + R[4] * b) + R[5] * c;
  z = (R[6] * a + R[7] * b) + R[8] * c;
}

__global__ void __launch_bounds__(kRenderBlock) render_vertex_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                                      const int* __restrict__ vf_off, const int* __restrict__ vf_list, int n_adj,
                                                                      const double* __restrict__ cams, const double* __restrict__ rot, int n, int V,
                                                                      int Fc, int H, int W, RenderVertex* __restrict__ vout) {
#pragma clang fp contract(off)
  const size_t t = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (t >= (size_t)n * V) return;
  const int i = (int)(t / V), v = (int)(t - (size_t)i * V);
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (rot)
    for (int k = 0; k < 9; ++k) R[k] = rot[(size_t)i * 9 + k];
  const float* P = verts + (size_t)i * V * 3;
  double xr, yr, zr;
  place(P, v, R, xr, yr, zr);
  const double* cam = cams + (size_t)i * 4;
  const double X = cam[0] * (xr + cam[2]), Y = cam[1] * (yr - cam[3]), d = -zr;
  const double px = (X + 1.0) * (0.5 * W), py = (1.0 - Y) * (0.5 * H);
  const double lim = 1048576.0;
  RenderVertex o;
  if (px >= -lim && px <= lim && py >= -lim && py <= lim && d >= -3.0e38 && d <= 3.0e38) {   // false for NaN and infinities
    o.ix = (int)floor(256.0 * px + 0.5);
    o.iy = (int)floor(256.0 * py + 0.5);
    o.d = (float)d;
  } else {
    o.ix = kRenderInvalid; o.iy = 0; o.d = 0.f;
  }
  // the normal: incident faces in the adjacency's (ascending) order; ranges are clamped to the list, entries outside [0, Fc) and faces with a
  // vertex index outside [0, V) contribute nothing
  double sx = 0, sy = 0, sz = 0;
  int k0 = vf_off[v], k1 = vf_off[v + 1];
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > n_adj ? n_adj : k1;
  for (int k = k0; k < k1; ++k) {
    const int f = vf_list[k];
    if (f < 0 || f >= Fc) continue;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;
    double ax, ay, az, bx, by, bz, cx, cy, cz;
    place(P, a, R, ax, ay, az); place(P, b, R, bx, by, bz); place(P, c, R, cx, cy, cz);
    const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
    sx += uy * wz - uz * wy; sy += uz * wx - ux * wz; sz += ux * wy - uy * wx;
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  if (len > 0) { sx /= len; sy /= len; sz /= len; }
  o.nx = (float)sx; o.ny = (float)sy; o.nz = (float)sz;
  vout[t] = o;
}

// (b) ------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRenderBlock) render_triangle_kernel(const RenderVertex* __restrict__ vin, const int* __restrict__ faces,
                                                                        const int* __restrict__ frame_index, int n, int V, int Fc, int F, int H, int W,
                                                                        unsigned long long* __restrict__ keys) {
  __shared__ RenderTri big[kRenderBlock];
  __shared__ int n_big;
  if (threadIdx.x == 0) n_big = 0;
  __syncthreads();
  const size_t t = (size_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (t < (size_t)n * Fc) {
    const int i = (int)(t / Fc), f = (int)(t - (size_t)i * Fc);
    const int fi = frame_index[i];
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (fi >= 0 && fi < F && a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V) {
      const RenderVertex* base = vin + (size_t)i * V;
      const RenderVertex p0 = base[a], p1 = base[b], p2 = base[c];
      if (p0.ix != kRenderInvalid && p1.ix != kRenderInvalid && p2.ix != kRenderInvalid) {
        const long long A = (long long)(p1.ix - p0.ix) * (p2.iy - p0.iy) - (long long)(p2.ix - p0.ix) * (p1.iy - p0.iy);
        if (A < 0) {
          RenderTri tr;
          tr.x0 = p0.ix; tr.y0 = p0.iy; tr.x1 = p1.ix; tr.y1 = p1.iy; tr.x2 = p2.ix; tr.y2 = p2.iy;
          tr.d0 = p0.d; tr.d1 = p1.d; tr.d2 = p2.d;
          const int xmin = min(p0.ix, min(p1.ix, p2.ix)), xmax = max(p0.ix, max(p1.ix, p2.ix));
          const int ymin = min(p0.iy, min(p1.iy, p2.iy)), ymax = max(p0.iy, max(p1.iy, p2.iy));
          // centres 256 c + 128 inside [xmin, xmax]; >> floors for negative values; |coordinates| <= 2^28 + 1: no overflow
          tr.c0 = max((xmin + 127) >> 8, 0); tr.c1 = min((xmax - 128) >> 8, W - 1);
          tr.r0 = max((ymin + 127) >> 8, 0); tr.r1 = min((ymax - 128) >> 8, H - 1);
          if (tr.c0 <= tr.c1 && tr.r0 <= tr.r1) {
            tr.key_hi = ((unsigned long long)(kRenderMaxInstances - 1 - i) << 52) | (unsigned long long)f;
            tr.plane = (size_t)fi * H * W;
            const int bw = tr.c1 - tr.c0 + 1, bh = tr.r1 - tr.r0 + 1;            // bw * bh <= H * W <= 2^28
            if (bw * bh <= kRenderSmallBox) {
              for (int r = tr.r0; r <= tr.r1; ++r)
                for (int c2 = tr.c0; c2 <= tr.c1; ++c2) draw_pixel(tr, c2, r, W, keys);
            } else {
              big[atomicAdd(&n_big, 1)] = tr;                                    // at most one per thread: the list cannot overflow
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const int nb = n_big;
  for (int j = 0; j < nb; ++j) {                                                  // list order varies from run to run; the key plane does not
    const RenderTri& tr = big[j];
    const int bw = tr.c1 - tr.c0 + 1, np = bw * (tr.r1 - tr.r0 + 1);
    for (int p = threadIdx.x; p < np; p += kRenderBlock) {
      const int r = p / bw;
      draw_pixel(tr, tr.c0 + (p - r * bw), tr.r0 + r, W, keys);
    }
  }
}

// (c) ------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRenderBlock) render_resolve_kernel(const uint8_t* frames, int F, int H, int W,
                                                                       const unsigned long long* __restrict__ keys,
                                                                       const RenderVertex* __restrict__ vin, const int* __restrict__ faces, int n, int V,
                                                                       int Fc, const float* __restrict__ colors, uint8_t* out, int* __restrict__ winner,
                                                                       float* __restrict__ depth) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * kRenderBlock + threadIdx.x;
  if (p >= H * W) return;
  const int r = p / W, c = p - r * W;
  for (int fr = blockIdx.y; fr < F; fr += gridDim.y) {
    const size_t q = (size_t)fr * H * W + p;
    const unsigned long long key = keys[q];
    int inst = -1, face = -1;
    float dd = INFINITY;
    uint8_t o0, o1, o2;
    bool drawn = false;
    if (key != kRenderEmpty) {
      inst = kRenderMaxInstances - 1 - (int)(key >> 52);
      face = (int)(key & (unsigned long long)(kRenderMaxFaces - 1));
      dd = monotone_inverse((unsigned)(key >> kRenderFaceBits));
      if (inst >= 0 && inst < n && face < Fc) {                                  // always true for keys this call wrote
        const int a = faces[3 * (size_t)face], b = faces[3 * (size_t)face + 1], c3 = faces[3 * (size_t)face + 2];
        const RenderVertex* base = vin + (size_t)inst * V;
        const RenderVertex p0 = base[a], p1 = base[b], p2 = base[c3];
        RenderTri tr;
        tr.x0 = p0.ix; tr.y0 = p0.iy; tr.x1 = p1.ix; tr.y1 = p1.iy; tr.x2 = p2.ix; tr.y2 = p2.iy;
        long long w0, w1, w2;
        if (cover(tr, c, r, w0, w1, w2)) {
          float b0, b1, b2;
          barycentrics(w0, w1, w2, b0, b1, b2);
          const float nx = (b0 * p0.nx + b1 * p1.nx) + b2 * p2.nx, ny = (b0 * p0.ny + b1 * p1.ny) + b2 * p2.ny,
                      nz = (b0 * p0.nz + b1 * p1.nz) + b2 * p2.nz;
          const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
          const float lam = len > 0.f ? fmaxf(0.f, nz / len) : 0.f;
          const float light = 0.3f + 0.76394373f * lam;                          // 2.4 / pi
          const float* col = colors + (size_t)inst * 3;
          const float v0 = fminf(fmaxf(col[0] * light + 0.1f, 0.f), 1.f), v1 = fminf(fmaxf(col[1] * light + 0.1f, 0.f), 1.f),
                      v2 = fminf(fmaxf(col[2] * light + 0.1f, 0.f), 1.f);
          o0 = (uint8_t)floorf(255.f * v0 + 0.5f); o1 = (uint8_t)floorf(255.f * v1 + 0.5f); o2 = (uint8_t)floorf(255.f * v2 + 0.5f);
          drawn = true;
        }
      }
    }
    if (!drawn) {
      const uint8_t* s = frames + q * 3;
      o0 = s[0]; o1 = s[1]; o2 = s[2];
      if (key != kRenderEmpty) { inst = -1; face = -1; dd = INFINITY; }
    }
    uint8_t* w = out + q * 3;                                                    // may be the frame itself: this thread alone reads and writes the pixel
    w[0] = o0; w[1] = o1; w[2] = o2;
    if (winner) { winner[2 * q] = inst; winner[2 * q + 1] = face; }
    if (depth) depth[q] = dd;
  }
}

inline size_t render_key_bytes(int H, int W, int n_frames) { return align_up((size_t)n_frames * H * W * sizeof(unsigned long long), 256); }

}  // namespace tepose

using namespace tepose;

extern "C" size_t tepose_render_workspace_bytes(int H, int W, int n_frames, int n_instances, int V, int Fc) {
  if (H < 1 || W < 1 || n_frames < 1 || n_instances < 0 || V < 1 || Fc < 0) return 0;
  if (H > kRenderMaxSide || W > kRenderMaxSide || n_instances > kRenderMaxInstances || V > kRenderMaxVerts || Fc > kRenderMaxFaces) return 0;
  return render_key_bytes(H, W, n_frames) + align_up((size_t)n_instances * V * sizeof(RenderVertex), 256);
}

extern "C" int tepose_render_meshes_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const float* verts, int n, int V,
                                       const int* faces, int Fc, const int* vert_face_offsets, const int* vert_face_list, int n_adj,
                                       const double* cams, const double* rot, const float* colors, uint8_t* out, int* winner, float* depth,
                                       void* workspace, size_t ws_bytes, void* stream) {
  if (F < 1 || H < 1 || W < 1 || n < 0 || V < 1 || Fc < 0 || n_adj < 0 || !frames || !out) return TEPOSE_E_ARG;
  if (n > 0 && (!frame_index || !verts || !cams || !colors || !vert_face_offsets || (Fc > 0 && !faces) || (n_adj > 0 && !vert_face_list)))
    return TEPOSE_E_ARG;
  if ((n > 0 || winner || depth) && (!workspace || ((uintptr_t)workspace & 7))) return TEPOSE_E_ARG;
  if (H > kRenderMaxSide || W > kRenderMaxSide || n > kRenderMaxInstances || V > kRenderMaxVerts || Fc > kRenderMaxFaces) return TEPOSE_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const size_t px = (size_t)H * W;
  if (n == 0 && !winner && !depth) {                                             // nothing to draw: the frames, copied
    if (out != frames) {
      const hipError_t e = hipMemcpyAsync(out, frames, (size_t)F * px * 3, hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
  if (ws_bytes < tepose_render_workspace_bytes(H, W, F, n, V, Fc)) return TEPOSE_E_WORKSPACE;
  unsigned long long* keys = (unsigned long long*)workspace;
  RenderVertex* rv = (RenderVertex*)((char*)workspace + render_key_bytes(H, W, F));
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)F * px * sizeof(unsigned long long), s);
  if (e != hipSuccess) return (int)e;
  if (n > 0) {
    const size_t nv = (size_t)n * V, nt = (size_t)n * Fc;
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((nv + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, s, verts, faces,
                       vert_face_offsets, vert_face_list, n_adj, cams, rot, n, V, Fc, H, W, rv);
    if (nt > 0)
      hipLaunchKernelGGL(render_triangle_kernel, dim3((unsigned)((nt + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, s, rv, faces,
                         frame_index, n, V, Fc, F, H, W, keys);
  }
  const dim3 grid((unsigned)((px + kRenderBlock - 1) / kRenderBlock), (unsigned)(F < 65535 ? F : 65535));
  hipLaunchKernelGGL(render_resolve_kernel, grid, dim3(kRenderBlock), 0, s, frames, F, H, W, keys, rv, faces, n, V, Fc, colors, out, winner, depth);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
