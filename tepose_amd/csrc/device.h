// Device-side primitives shared by the kernel files: MFMA vector types, the GRU gate math and cell update, vmcnt waits, the LDS-DMA
// request in its builtin and its M0 form, and the two-value plane stores.  One definition each -- a kernel file states what is its own
// (tiling, K loop, epilogue store pattern) and takes the rest from here.  The data formats (plane_index, plane_slot, split_hi_lo,
// split_hi_lo16) are in common.h because the host packs them too; the block -> tile map is in walk.h (walk_block_tile).
#pragma once
#include "common.h"

namespace tepose {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- SMPL joint tables (smpl.hip forward, smpl_bwd.hip backward)
// the 49 joints of lib/models/smpl.py:72-84 as indices into [24 posed joints | 21 picked vertices | 9 regressed rows], the 14 LSP joints of the 17 H36M
// rows, and the picked vertices (smplx vertex_joint_selector)
static __device__ const int kJointMap49[49] = {24, 12, 17, 19, 21, 16, 18, 20, 0,  2,  5,  8,  1,  4,  7,  25, 26,
                                        27, 28, 29, 30, 31, 32, 33, 34, 8,  5,  45, 46, 4,  7,  21, 19, 17,
                                        16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27};
static __device__ const int kH36mToJ14[14] = {6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10};
static __device__ const int kExtraVerts[21] = {332,  6260, 2800, 4071, 583,  3216, 3226, 3387, 6617, 6624, 6787,
                                        2746, 2319, 2445, 2556, 2673, 6191, 5782, 5905, 6016, 6133};

// ---------------------------------------------------------------- GRU gate math
// sigma(x) = 1/(1+2^(-x log2 e)), tanh(x) = 2 sigma(2x) - 1 on the hardware exp2 / rcp units
// (v_exp_f32, v_rcp_f32: ~1 ulp each).  Absolute error of a gate value < 3e-7, far inside the
// 1e-4 parity budget (tests/test_gpu_parity.py::test_encoder_vs_oracle runs 32-step recurrences).
// -DTEPOSE_FAST_GATES=0 switches every kernel of the library to expf / tanhf.
#ifndef TEPOSE_FAST_GATES
#define TEPOSE_FAST_GATES 1
#endif
__device__ __forceinline__ float gate_sigmoid(float x) {
#if TEPOSE_FAST_GATES
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
#else
  return 1.f / (1.f + expf(-x));
#endif
}
__device__ __forceinline__ float gate_tanh(float x) {
#if TEPOSE_FAST_GATES
  return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.88539008177792681f * x)) - 1.f;
#else
  return tanhf(x);
#endif
}
// torch.nn.GRU's cell: gi_x = x W_ih^T + b_ih, gh_x = h W_hh^T + b_hh (the caller adds the bias), gates r, z, n
__device__ __forceinline__ float gru_cell(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float hprev) {
  const float r = gate_sigmoid(gi_r + gh_r);
  const float z = gate_sigmoid(gi_z + gh_z);
  const float n = gate_tanh(gi_n + r * gh_n);
  return (1.f - z) * n + z * hprev;
}
// the step from h = 0 (gh_x = b_x).  Not gru_cell(..., 0.f): that adds z * 0, which turns a -0 result into +0
__device__ __forceinline__ float gru_cell_first(float gi_r, float gi_z, float gi_n, float b_r, float b_z, float b_n) {
  const float r = gate_sigmoid(gi_r + b_r);
  const float z = gate_sigmoid(gi_z + b_z);
  const float n = gate_tanh(gi_n + r * b_n);
  return (1.f - z) * n;
}

// ---------------------------------------------------------------- waits and LDS-DMA
template <int N>
__device__ __forceinline__ void wait_vm() {          // s_waitcnt vmcnt(N) with a literal count
  static_assert(N >= 0 && N <= 63, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// 16 bytes per lane from global memory straight into LDS (wave-uniform LDS base + 16 * lane)
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
// the same request with the LDS destination written to M0 by hand: scalar base + one 32-bit lane offset, no address VGPR pair
__device__ __forceinline__ void glds16_m0(unsigned voff, const char* sbase, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_dst) : "m0", "memory");
}

__device__ __forceinline__ h16x8 as_h8(u32x4 v) {
  union { u32x4 u; h16x8 h; } c;
  c.u = v;
  return c.h;
}

// ---------------------------------------------------------------- two consecutive values of one row as hi / lo plane pairs (4 bytes each)
struct PlanePair2 { h16x2 hi, lo; };
__device__ __forceinline__ PlanePair2 split_pack2(float v0, float v1) {
  half_t h0, l0, h1, l1;
  split_hi_lo(v0, h0, l0);
  split_hi_lo(v1, h1, l1);
  return PlanePair2{h16x2{h0, h1}, h16x2{l0, l1}};
}
// plain stores: for a reader in a LATER kernel (or the same workgroup behind a barrier)
__device__ __forceinline__ void store_planes2(half_t* hi, half_t* lo, float v0, float v1) {
  const PlanePair2 p = split_pack2(v0, v1);
  *(h16x2*)hi = p.hi;
  *(h16x2*)lo = p.lo;
}
// write-through stores (relaxed, agent scope): what a hand-off to ANOTHER workgroup of the SAME launch needs -- the storing wave then
// drains (wait_vm<0>) and the workgroup arrives at its counter; the reader loads with sc1 (gru_seq.hip's header has the protocol)
__device__ __forceinline__ void publish_planes2(half_t* hi, half_t* lo, float v0, float v1) {
  const PlanePair2 p = split_pack2(v0, v1);
  __hip_atomic_store((unsigned*)hi, __builtin_bit_cast(unsigned, p.hi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store((unsigned*)lo, __builtin_bit_cast(unsigned, p.lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace tepose
