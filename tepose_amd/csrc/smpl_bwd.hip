// SMPL backward for N persons: gradients of (vertices, 49 joints) with respect to (pose, betas), DESIGN.md section 19.
//
// The gradient is autograd's through oracle/tepose_ref.py (batch_rodrigues -> lbs -> smpl_joints49), stage by stage in reverse:
//   joints  (smpl_joints_bwd_kernel)  g_joints49 -> the 54 joint sources (24 posed joints | 21 picked vertices | 9 regressed rows), repeats of the
//                                     joint map added in ascending joint order
//   skin    (smpl_skin_bwd_kernel)    g_verts + the picked / regressed sources -> g_vposed = T^T g_v per vertex, and per workgroup one partial
//                                     of g_A[24][12] = sum_v w_vj (g_v x [v_posed, 1])
//   blend   (smpl_blend_bwd_kernel)   g_f[N,224] = g_vposed[N,20670] x blendW[20670,224], K split over workgroups; smpl_blend_bwd_sum_kernel adds
//                                     the splits in ascending order
//   chain   (smpl_chain_bwd_kernel)   one wave per person, lane = joint: sums the skinning partials in ascending workgroup order, walks the
//                                     kinematic tree from the leaves to the root, g_R -> Rodrigues -> g_pose, g_J -> JS^T -> g_betas
// The forward values these need (transforms, pose features, v_posed) are recomputed by the forward's own prep kernel and blend product before the
// first kernel here (forward.hip tepose_smpl_bwd): nothing is carried over from a forward call.  No atomics: every sum has a fixed order, so two calls
// on the same inputs agree bit for bit.
#include "device.h"

namespace tepose {

// ------------------------------------------------------------------ (a) 49 joints -> 54 sources
// block = person, thread = (source, coordinate).  g_joints49 == nullptr: zeros.
__global__ void __launch_bounds__(192) smpl_joints_bwd_kernel(const float* __restrict__ g_j49, int N, float* __restrict__ gsrc) {
  const int p = blockIdx.x, t = threadIdx.x;
  if (p >= N || t >= kBwdSrc * 3) return;
  const int s = t / 3, c = t % 3;
  float acc = 0.f;
  if (g_j49) {
    const float* g = g_j49 + (long)p * 49 * 3;
    for (int k = 0; k < 49; ++k)
      if (kJointMap49[k] == s) acc += g[k * 3 + c];
  }
  gsrc[(long)p * kBwdSrc * 3 + t] = acc;
}

// ------------------------------------------------------------------ (b) skinning backward
// thread = vertex (512 per workgroup), persons looped as the forward's skinning kernels do.  Per person a thread forms g_v (the caller's vertex gradient
// plus what the joints send to this vertex: its column of J_regressor_extra, held in 9 registers, and -- for the 21 picked vertices -- the joint's own
// gradient), the blended transform T of the vertex (SPARSE: its <= 4 (joint, weight) pairs; else the 24 dense weights), writes g_vposed = T^T g_v and
// leaves [g_v | v_posed, 1] in LDS.  The 24 x 12 transform gradient of the workgroup's vertices is then summed without atomics: thread (slice, joint)
// adds the 25 vertices of its slice in ascending order, its 25 skin weights for that joint in registers (loaded once per workgroup), and 288 threads add
// the 21 slices in ascending order.  partial[p][workgroup][24][12].
template <bool SPARSE>
__global__ void __launch_bounds__(kBwdSkinVB, SPARSE ? 4 : 2) smpl_skin_bwd_kernel(SmplConsts c, const float* __restrict__ vposed, const float* __restrict__ Amat,
                                                                   const float* __restrict__ g_verts, const float* __restrict__ gsrc, int N, int pg,
                                                                   float* __restrict__ gvp, float* __restrict__ partial) {
  constexpr int VB = kBwdSkinVB, SL = kBwdSkinSlice, NS = kBwdSkinSlices;
  __shared__ __attribute__((aligned(16))) float sO[NS * SL * 8];       // per vertex [g0 g1 g2 0 | x y z 1]; rows past the 512 vertices stay zero
  __shared__ __attribute__((aligned(16))) float sR[NS * kNJ * 12];     // per (slice, joint) the 12 sums; at set-up the 512 x 9 regressor columns
  __shared__ __attribute__((aligned(16))) float sA[kNJ * 12];
  __shared__ float sG[(kBwdSrc - kNJ) * 3];                            // this person's gradients of the 21 picked vertices and the 9 regressed rows
  static_assert(NS * kNJ * 12 >= VB * 9, "the regressor columns fit the slice sums' buffer");
  const int tid = threadIdx.x, v0 = blockIdx.x * VB, v = v0 + tid;
  const bool ok = v < kNV;
  // ---- set-up, once per workgroup: this vertex's column of J_regressor_extra from the row CSR (a vertex occurs at most once per row)
  for (int i = tid; i < VB * 9; i += VB) sR[i] = 0.f;
  for (int i = tid; i < (NS * SL - VB) * 8; i += VB) sO[VB * 8 + i] = 0.f;
  __syncthreads();
  for (int r = 0; r < 9; ++r) {
    const int e1 = c.xr_ptr[r + 1];
    for (int e = c.xr_ptr[r] + tid; e < e1; e += VB) {
      const int col = c.xr_idx[e] - v0;
      if (col >= 0 && col < VB) sR[col * 9 + r] = c.xr_val[e];
    }
  }
  __syncthreads();
  float xv[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) xv[r] = sR[tid * 9 + r];
  int pick = -1;                                     // index among the 21 picked vertices, or none
#pragma unroll
  for (int i = 0; i < 21; ++i)
    if (ok && kExtraVerts[i] == v) pick = i;
  // skin weights of this vertex (the transform it is skinned with) ...
  int jx[4];
  float wv[SPARSE ? 4 : kNJ];
  if (SPARSE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { jx[k] = ok ? c.lbs_cidx[v * 4 + k] * 12 : 0; wv[k] = ok ? c.lbs_cval[v * 4 + k] : 0.f; }
  } else {
#pragma unroll
    for (int j = 0; j < kNJ; ++j) wv[j] = ok ? c.lbsW[(long)v * kNJ + j] : 0.f;
  }
  // ... and, as reducing thread (slice, joint), the weights of the slice's vertices for that joint
  const int rs = tid / kNJ, rj = tid % kNJ;
  const bool red = rs < NS;
  float wr[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const int lv = rs * SL + i, gv = v0 + lv;
    wr[i] = red && lv < VB && gv < kNV ? c.lbsW[(long)gv * kNJ + rj] : 0.f;
  }
  __syncthreads();                                   // the regressor columns are read: sR is free for the sums

  const int p0 = blockIdx.y * pg, p1 = min(p0 + pg, N);
  for (int p = p0; p < p1; ++p) {
    if (tid < kNJ * 12) sA[tid] = Amat[(long)p * kNJ * 12 + tid];
    if (tid >= 320 && tid < 320 + (kBwdSrc - kNJ) * 3) sG[tid - 320] = gsrc[(long)p * kBwdSrc * 3 + kNJ * 3 + (tid - 320)];
    __syncthreads();
    {
      float g[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f};
      if (ok) {
        const float* vp = vposed + (long)p * kVertLd + 3 * v;
        x[0] = vp[0]; x[1] = vp[1]; x[2] = vp[2];
        if (g_verts) { const float* gp = g_verts + ((long)p * kNV + v) * 3; g[0] = gp[0]; g[1] = gp[1]; g[2] = gp[2]; }
        if (pick >= 0) { g[0] += sG[pick * 3]; g[1] += sG[pick * 3 + 1]; g[2] += sG[pick * 3 + 2]; }
#pragma unroll
        for (int r = 0; r < 9; ++r) { g[0] += xv[r] * sG[(21 + r) * 3]; g[1] += xv[r] * sG[(21 + r) * 3 + 1]; g[2] += xv[r] * sG[(21 + r) * 3 + 2]; }
        float t[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) t[e] = 0.f;
        if (SPARSE) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const f32x4 r0 = *(const f32x4*)(sA + jx[k]), r1 = *(const f32x4*)(sA + jx[k] + 4), r2 = *(const f32x4*)(sA + jx[k] + 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { t[e] += wv[k] * r0[e]; t[4 + e] += wv[k] * r1[e]; t[8 + e] += wv[k] * r2[e]; }
          }
        } else {
#pragma unroll
          for (int j = 0; j < kNJ; ++j)
#pragma unroll
            for (int e = 0; e < 12; ++e) t[e] += wv[j] * sA[j * 12 + e];
        }
        float* o = gvp + (long)p * kVertLd + 3 * v;                // g_vposed = T[:3,:3]^T g_v
        o[0] = t[0] * g[0] + t[4] * g[1] + t[8] * g[2];
        o[1] = t[1] * g[0] + t[5] * g[1] + t[9] * g[2];
        o[2] = t[2] * g[0] + t[6] * g[1] + t[10] * g[2];
      } else if (v == kNV) {                                       // the row padding (kVertLd - 3 * 6890 floats): the blend kernel reads whole groups of 8 rows
#pragma unroll
        for (int e = 0; e < kVertLd - 3 * kNV; ++e) gvp[(long)p * kVertLd + 3 * kNV + e] = 0.f;
      }
      *(f32x4*)(sO + tid * 8) = f32x4{g[0], g[1], g[2], 0.f};     // (a thread past the last vertex: zeros, with weight zero)
      *(f32x4*)(sO + tid * 8 + 4) = f32x4{x[0], x[1], x[2], ok ? 1.f : 0.f};
    }
    __syncthreads();
    if (red) {
      float a[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) a[e] = 0.f;
#pragma unroll
      for (int i = 0; i < SL; ++i) {
        const f32x4 gq = *(const f32x4*)(sO + (rs * SL + i) * 8), xq = *(const f32x4*)(sO + (rs * SL + i) * 8 + 4);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float wg = wr[i] * gq[r];
#pragma unroll
          for (int e = 0; e < 4; ++e) a[r * 4 + e] += wg * xq[e];
        }
      }
      float* o = sR + (rs * kNJ + rj) * 12;
#pragma unroll
      for (int r = 0; r < 3; ++r) *(f32x4*)(o + 4 * r) = f32x4{a[4 * r], a[4 * r + 1], a[4 * r + 2], a[4 * r + 3]};
    }
    __syncthreads();
    if (tid < kNJ * 12) {
      float acc = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) acc += sR[s * kNJ * 12 + tid];
      partial[((long)p * kBwdSkinBlocks + blockIdx.x) * (kNJ * 12) + tid] = acc;
    }
  }
}

hipError_t launch_smpl_skin_bwd(const SmplConsts& c, const float* vposed, const float* Amat, const float* g_verts, const float* gsrc, int N,
                                float* gvp, float* partial, hipStream_t s) {
  const Launch l = skin_bwd_shape(N);      // a1: persons per block
  if (c.lbs_sparse)
    hipLaunchKernelGGL(smpl_skin_bwd_kernel<true>, grid_of(l), block_of(l), 0, s, c, vposed, Amat, g_verts, gsrc, N, l.a1, gvp, partial);
  else
    hipLaunchKernelGGL(smpl_skin_bwd_kernel<false>, grid_of(l), block_of(l), 0, s, c, vposed, Amat, g_verts, gsrc, N, l.a1, gvp, partial);
  return hipGetLastError();
}

hipError_t launch_smpl_joints_bwd(const float* g_j49, int N, float* gsrc, hipStream_t s) {
  const Launch l = joints_bwd_shape(N);
  hipLaunchKernelGGL(smpl_joints_bwd_kernel, grid_of(l), block_of(l), 0, s, g_j49, N, gsrc);
  return hipGetLastError();
}

// ------------------------------------------------------------------ (c) blend shapes backward
// part[split][p][k] = sum over the split's table rows r of g_vposed[p][r] * blendW[r][k], rows ascending, fp32 FMA on the exact fp32 table (the one the
// forward's small-N kernel and TEPOSE_EXACT_FP32 read).  The product's K axis is the table's ROW axis, so a workgroup streams whole rows (896 bytes,
// coalesced, 8 bytes per thread: thread = 2 adjacent columns) and needs no transposed copy of the table.  A person's gradients are the same for
// every thread: their addresses are formed from the block index and loop counters alone, so they arrive through the scalar cache, eight consecutive rows
// per load, and enter the FMAs as scalar operands -- no LDS, no barrier.  2 x PT accumulators per thread.  Persons past N repeat person N - 1 (never
// stored); the last chunk's rows past 20670 meet table rows that are zero and the zeros the skinning kernel leaves in g_vposed's row padding.
template <int PT>
__global__ void __launch_bounds__(128) smpl_blend_bwd_kernel(const float* __restrict__ blendW, const float* __restrict__ gvp, int N, int per,
                                                             float* __restrict__ part) {
  static_assert(kBwdChunk % 8 == 0 && kBwdChunks * kBwdChunk <= kBlendN && kVertLd % 8 == 0, "whole groups of 8 rows inside the table and inside a g_vposed row");
  const int tid = threadIdx.x, split = blockIdx.x, p0 = blockIdx.y * PT;
  if (tid >= kBlendK / 2) return;                    // (no barrier below)
  float acc0[PT], acc1[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  const int r_begin = split * per * kBwdChunk, r_end = min((split + 1) * per, kBwdChunks) * kBwdChunk;
  const float* w = blendW + 2 * tid;
  for (int r = r_begin; r < r_end; r += 8) {
    float w0[8], w1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { w0[i] = w[(long)(r + i) * kBlendK]; w1[i] = w[(long)(r + i) * kBlendK + 1]; }
#pragma unroll
    for (int pp = 0; pp < PT; ++pp) {
      const f32x4* g = (const f32x4*)(gvp + (long)min(p0 + pp, N - 1) * kVertLd + r);       // wave-uniform, 32-byte aligned
      const f32x4 ga = g[0], gb = g[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc0[pp] += ga[i] * w0[i]; acc1[pp] += ga[i] * w1[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc0[pp] += gb[i] * w0[4 + i]; acc1[pp] += gb[i] * w1[4 + i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PT; ++i)
    if (p0 + i < N) {
      float* o = part + ((long)split * N + p0 + i) * kBlendK + 2 * tid;
      o[0] = acc0[i]; o[1] = acc1[i];
    }
}

// gf[p][k] = sum over the splits, ascending within each quarter of them, the four quarters then added in order: 64 elements x 4 quarters per block,
// eight independent loads in flight per thread (323 splits at N <= 32)
__global__ void __launch_bounds__(256) smpl_blend_bwd_sum_kernel(const float* __restrict__ part, int N, int splits, float* __restrict__ gf) {
  __shared__ float sq[4][64];
  const int q = threadIdx.x >> 6, e = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 64 + e, n = (long)N * kBlendK;
  const int per = (splits + 3) / 4, s0 = q * per, s1 = min(s0 + per, splits);
  float acc = 0.f;
  if (i < n) {
#pragma unroll 8
    for (int s = s0; s < s1; ++s) acc += part[(long)s * n + i];
  }
  sq[q][e] = acc;
  __syncthreads();
  if (q == 0 && i < n) gf[i] = ((sq[0][e] + sq[1][e]) + sq[2][e]) + sq[3][e];
}

hipError_t launch_smpl_blend_bwd(const float* blendW, const float* gvp, int N, float* part, float* gf, hipStream_t s) {
  const Launch l = blend_bwd_shape(N);     // a0: chunks per split
  if (l.kernel == kBlendBwd8)
    hipLaunchKernelGGL(smpl_blend_bwd_kernel<8>, grid_of(l), block_of(l), 0, s, blendW, gvp, N, l.a0, part);
  else
    hipLaunchKernelGGL(smpl_blend_bwd_kernel<32>, grid_of(l), block_of(l), 0, s, blendW, gvp, N, l.a0, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const Launch r = blend_bwd_sum_shape(N);
  hipLaunchKernelGGL(smpl_blend_bwd_sum_kernel, grid_of(r), block_of(r), 0, s, part, N, (int)l.gx, gf);
  return hipGetLastError();
}

// ------------------------------------------------------------------ (d) chain backward
// R(aa) = I + a K + b K^2 with K = skew(aa), a = sin(t) / t, b = (1 - cos t) / t^2, t = |aa + 1e-8| -- smplx's batch_rodrigues
// (I + sin K(aa / t) + (1 - cos) K(aa / t)^2) with the division by t moved into the coefficients, so that nothing is divided by a small number twice.
// b through sin^2(t / 2) (1 - cos t cancels below t ~ 1e-3); da/dt and db/dt as series below t = 0.5 (their closed forms cancel there).
__device__ __forceinline__ void rodrigues_bwd(const float aa[3], const float gR[3][3], float g_aa[3]) {
  const float ex = aa[0] + 1e-8f, ey = aa[1] + 1e-8f, ez = aa[2] + 1e-8f;
  const float t = sqrtf(ex * ex + ey * ey + ez * ez), t2 = t * t;
  const float sn = sinf(t), cs = cosf(t), sh = sinf(0.5f * t);
  const float a = sn / t, b = 2.f * (sh / t) * (sh / t);
  float da, db;
  if (t < 0.5f) {
    da = t * (-1.f / 3.f + t2 * (1.f / 30.f + t2 * (-1.f / 840.f + t2 * (1.f / 45360.f))));
    db = t * (-1.f / 12.f + t2 * (1.f / 180.f + t2 * (-1.f / 6720.f + t2 * (1.f / 453600.f))));
  } else {
    da = (cs * t - sn) / t2;
    db = (sn * t - 4.f * sh * sh) / (t2 * t);
  }
  const float K[3][3] = {{0.f, -aa[2], aa[1]}, {aa[2], 0.f, -aa[0]}, {-aa[1], aa[0], 0.f}};
  float ga = 0.f, gb = 0.f, gK[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const float kk = K[r][0] * K[0][cc] + K[r][1] * K[1][cc] + K[r][2] * K[2][cc];
      ga += gR[r][cc] * K[r][cc];
      gb += gR[r][cc] * kk;
      // d/dK of <gR, K^2> = gR K^T + K^T gR
      const float m = gR[r][0] * K[cc][0] + gR[r][1] * K[cc][1] + gR[r][2] * K[cc][2] + K[0][r] * gR[0][cc] + K[1][r] * gR[1][cc] + K[2][r] * gR[2][cc];
      gK[r][cc] = a * gR[r][cc] + b * m;
    }
  const float gt = (ga * da + gb * db) / t;          // through t = |aa + 1e-8|: dt / d aa_i = (aa_i + 1e-8) / t
  g_aa[0] = gK[2][1] - gK[1][2] + gt * ex;
  g_aa[1] = gK[0][2] - gK[2][0] + gt * ey;
  g_aa[2] = gK[1][0] - gK[0][1] + gt * ez;
}

// One wave per person, lane = joint.  Forward values again as smpl_prep_person forms them (R, rest joints, G level by level), then
//   g_G_j = [g_A_j[:, :3] - g_A_j[:, 3] x J_j | g_A_j[:, 3] + g_posed_j],   g_J_j = -G_j[:, :3]^T g_A_j[:, 3]
// and from the deepest level up (G_j = G_parent [R_j | rel_j]):
//   g_R_j = P^T g_G_j[:, :3],  g_rel_j = P^T g_G_j[:, 3],  g_G_parent += [g_G_j[:, :3] R_j^T + g_G_j[:, 3] x rel_j | g_G_j[:, 3]]
// A parent takes its children's contributions from LDS in ascending joint index.  mode 1: pose = axis-angle, g_pose [N,72]; mode 2: rotation matrices,
// g_pose [N,24,3,3].
__global__ void __launch_bounds__(256) smpl_chain_bwd_kernel(SmplConsts c, int maxdepth, int mode, const float* __restrict__ pose,
                                                             const float* __restrict__ betas, int N, const float* __restrict__ partial,
                                                             const float* __restrict__ gsrc, const float* __restrict__ gf,
                                                             float* __restrict__ g_pose, float* __restrict__ g_betas) {
  __shared__ float sC[4][kNJ][16];
  __shared__ float sJ[4][kNJ * 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * 4 + wave;
  if (p >= N) return;                       // wave-uniform; only wave-level synchronisation below
  const int j = lane < kNJ ? lane : 0;
  const bool act = lane < kNJ;
  const float* x = pose + (long)p * (mode == 1 ? 72 : 216);
  float R[3][3], aa[3] = {0.f, 0.f, 0.f};
  if (mode == 1) {
    // smplx.lbs.batch_rodrigues as the forward's prep forms it
    aa[0] = x[3 * j]; aa[1] = x[3 * j + 1]; aa[2] = x[3 * j + 2];
    const float ex = aa[0] + 1e-8f, ey = aa[1] + 1e-8f, ez = aa[2] + 1e-8f;
    const float ang = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = aa[0] / ang, ry = aa[1] / ang, rz = aa[2] / ang;
    const float sn = sinf(ang), cs = 1.f - cosf(ang);
    const float K[3][3] = {{0.f, -rz, ry}, {rz, 0.f, -rx}, {-ry, rx, 0.f}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        const float kk = K[r][0] * K[0][cc] + K[r][1] * K[1][cc] + K[r][2] * K[2][cc];
        R[r][cc] = (r == cc ? 1.f : 0.f) + sn * K[r][cc] + cs * kk;
      }
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) R[r][cc] = x[9 * j + 3 * r + cc];
  }
  float Jr[3];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    float v = c.J0[j * 3 + cc];
#pragma unroll
    for (int l = 0; l < 10; ++l) v += c.JS[(j * 3 + cc) * 10 + l] * betas[(long)p * 10 + l];
    Jr[cc] = v;
  }
  const int par = act ? c.parents[j] : -1;
  const int dep = act ? c.depth[j] : 0;
  const int src = par < 0 ? 0 : par;
  float rel[3];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    const float pj = __shfl(Jr[cc], src);
    rel[cc] = par < 0 ? Jr[cc] : Jr[cc] - pj;
  }
  float G[3][4], P[3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r) { G[r][0] = R[r][0]; G[r][1] = R[r][1]; G[r][2] = R[r][2]; G[r][3] = rel[r]; }
  for (int lvl = 1; lvl <= maxdepth; ++lvl) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) P[r][cc] = __shfl(G[r][cc], src);
    if (dep == lvl) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) G[r][cc] = P[r][0] * R[0][cc] + P[r][1] * R[1][cc] + P[r][2] * R[2][cc];
        G[r][3] = P[r][0] * rel[0] + P[r][1] * rel[1] + P[r][2] * rel[2] + P[r][3];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) P[r][cc] = __shfl(G[r][cc], src);      // the parent's finished transform

  // ---- g_A: the skinning partials in ascending workgroup order; g_posed
  float gA[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) gA[e] = 0.f;
  if (act) {
    for (int b = 0; b < kBwdSkinBlocks; ++b) {
      const float* q = partial + ((long)p * kBwdSkinBlocks + b) * (kNJ * 12) + j * 12;
#pragma unroll
      for (int e = 0; e < 12; ++e) gA[e] += q[e];
    }
  }
  float gGR[3][3], gGt[3], gJ[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float gp = act ? gsrc[(long)p * kBwdSrc * 3 + j * 3 + r] : 0.f;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      gGR[r][cc] = gA[r * 4 + cc] - gA[r * 4 + 3] * Jr[cc];
      gJ[cc] -= G[r][cc] * gA[r * 4 + 3];
    }
    gGt[r] = gA[r * 4 + 3] + gp;
  }
  // ---- leaves to root
  float gR[3][3], grel[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { grel[r] = 0.f; gR[r][0] = gR[r][1] = gR[r][2] = 0.f; }
  float* mine = sC[wave][j];
  for (int lvl = maxdepth; lvl >= 1; --lvl) {
    if (act && dep == lvl) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          gR[r][cc] = P[0][r] * gGR[0][cc] + P[1][r] * gGR[1][cc] + P[2][r] * gGR[2][cc];
          mine[r * 4 + cc] = gGR[r][0] * R[cc][0] + gGR[r][1] * R[cc][1] + gGR[r][2] * R[cc][2] + gGt[r] * rel[cc];
        }
        grel[r] = P[0][r] * gGt[0] + P[1][r] * gGt[1] + P[2][r] * gGt[2];
        mine[r * 4 + 3] = gGt[r];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int ch = 1; ch < kNJ; ++ch) {
      const int pc = __shfl(par, ch), dc = __shfl(dep, ch);
      if (act && pc == j && dc == lvl) {
        const float* q = sC[wave][ch];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          gGR[r][0] += q[r * 4]; gGR[r][1] += q[r * 4 + 1]; gGR[r][2] += q[r * 4 + 2];
          gGt[r] += q[r * 4 + 3];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (act && dep == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { gR[r][0] = gGR[r][0]; gR[r][1] = gGR[r][1]; gR[r][2] = gGR[r][2]; grel[r] = gGt[r]; }
  }
  // ---- rel_j = J_j - J_parent: g_J_j += g_rel_j, g_J_parent -= g_rel_child (children in ascending joint index)
  if (act) { mine[12] = grel[0]; mine[13] = grel[1]; mine[14] = grel[2]; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) gJ[cc] += grel[cc];
  for (int ch = 1; ch < kNJ; ++ch) {
    const int pc = __shfl(par, ch);
    if (act && pc == j) {
      const float* q = sC[wave][ch];
      gJ[0] -= q[12]; gJ[1] -= q[13]; gJ[2] -= q[14];
    }
  }
  // ---- g_betas = the blend product's columns 1..10 + JS^T g_J (72 terms, ascending)
  if (act) { sJ[wave][j * 3] = gJ[0]; sJ[wave][j * 3 + 1] = gJ[1]; sJ[wave][j * 3 + 2] = gJ[2]; }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (g_betas && lane < 10) {
    float acc = gf[(long)p * kBlendK + 1 + lane];
    for (int i = 0; i < kNJ * 3; ++i) acc += c.JS[i * 10 + lane] * sJ[wave][i];
    g_betas[(long)p * 10 + lane] = acc;
  }
  // ---- the pose feature's R[1:] - I, then the pose
  if (g_pose && act) {
    if (j >= 1) {
      const float* q = gf + (long)p * kBlendK + 11 + 9 * (j - 1);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) gR[r][cc] += q[3 * r + cc];
    }
    if (mode == 1) {
      float g_aa[3];
      rodrigues_bwd(aa, gR, g_aa);
      float* o = g_pose + (long)p * 72 + 3 * j;
      o[0] = g_aa[0]; o[1] = g_aa[1]; o[2] = g_aa[2];
    } else {
      float* o = g_pose + (long)p * 216 + 9 * j;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) o[3 * r + cc] = gR[r][cc];
    }
  }
}

hipError_t launch_smpl_chain_bwd(const SmplConsts& c, int mode, const float* pose, const float* betas, int N, const float* partial,
                                 const float* gsrc, const float* gf, float* g_pose, float* g_betas, hipStream_t s) {
  const Launch l = chain_bwd_shape(N);
  hipLaunchKernelGGL(smpl_chain_bwd_kernel, grid_of(l), block_of(l), 0, s, c, c.maxdepth, mode, pose, betas, N, partial, gsrc, gf, g_pose, g_betas);
  return hipGetLastError();
}

}  // namespace tepose
