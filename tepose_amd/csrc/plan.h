// The kernel plan and its selection (plan.hip): pure host code -- calls no launcher, makes no device call.
#pragma once
#include "model.h"

namespace tepose {

// ---- the kernel plan: one kernel family per stage of a forward ------------------------------------------------------------------------------------
// select_kernels (plan.hip) is the only function that reads a handle's family knobs (split, large_scaled, state_planes, gi_blk, s_min_b, blend16_min_n,
// the collapse flags, lbs_sparse, persist) and the Options thresholds that pick between kernel symbols.  Every entry point that launches TePose work
// builds ONE plan after its argument checks and passes it down; launch sites switch on its values and pass the family to the launchers.  What is left
// below the family -- which instantiation of it, the grid, the block, the group size of the walk -- is decided by the pure functions of shapes.h, which
// select_kernels calls too (its shape predicates, the rounds comparison of the 128 x 288 tiles): a launcher keeps its empty-shape return, its argument
// and alignment checks with their fall-backs for misaligned views (gru_step16_planes_ok, launch_gru_first), and one switch over what shapes.h returned.
// describe_plan renders the plan as the symbols a rocprofv3 trace prints (tepose_select_kernels; pinned by tests/test_dispatch.py without a GPU).
enum class Rows : unsigned char { pad, split_few, split };                              // how caller rows become the A operand
enum class Mm : unsigned char { f32, f32_skinny, h3, h3_skinny, h3s_mid, h3s0, h3s };    // one product
enum class Step : unsigned char { f32, f32_skinny, h3, h3_skinny, seq, seq_gran, s16, s16_planes };   // one layer's cell steps
enum class First : unsigned char { f32, f32_skinny, h3, h3_16, in_seq };                 // a first step (h = 0)
enum class Reg : unsigned char { loop, seq };                                            // the regressor's FC loop: a launch per product | reg_seq_kernel
enum class Smpl : unsigned char { small, f32, f32_skinny, h3, h3s };                     // SMPL: one launch | prep + blend-shape product (as Mm) + skinning

struct KernelPlan {
  // carving and operand formats
  bool h3 = false;            // split-precision planes (split-mode handle, B > TEPOSE_SPLIT_MIN_M); else the exact-fp32 kernels of gemm.hip / skinny.hip
  bool scaled = false;        // large batch: recurrent-state planes in the scaled format of gemm_h3s.hip
  bool gblk = false;          // ... with the layer >= 1 gate pre-activations and the fp32 states between steps in the 16 x 16-blocked layout
  bool g0blk = false;         // layer-0 gate pre-activations frame-major + blocked (gi0_layout)
  bool gran = false;          // granule buffers of the persistent recurrent kernel carved (its B <= 4 mode)
  bool blend16 = false;       // pose-feature rows as scaled planes for the blend-shape product on gemm_h3s_persist16c_kernel<1>
  bool reg_collapsed = false; // the regressor's three FC iterations as one product, where a call asks for exactly that
  bool tail_collapsed = false;   // ... together with the tail linears, from the encoder's final states
  bool pair = false;          // window path: both layer-0 products of a step as one width-first launch
  // one kernel family per stage; window plans (select_kernels(.., window = true)) describe the cached window path instead of the layer-0 input + product
  Rows input = Rows::pad;     // the windows (window plan: the B frame rows of tepose_project_frames)
  Rows input_x0 = Rows::pad;  // L = 1: frame T - 1 of every window, for the one-step product
  Rows input_pair = Rows::pad;   // window plan: the 2 B rows of the pair product
  Rows input_blend = Rows::pad;  // blend16: the pose-feature rows
  Mm projection = Mm::f32;    // layer 0 (window plan: one B-row frame product)
  Mm proj_l1 = Mm::f32;       // layers >= 1, every slab row
  Mm proj_one = Mm::f32;      // the top gru_rec layer's forward direction, which consumes one step: B rows (L = 1: layer 0, frame T - 1)
  First first = First::f32;
  Step step0 = Step::f32, step1 = Step::f32;   // layer 0 | layers >= 1
  Mm tail = Mm::f32;          // the B-row products of >= 1024 columns of the tail linears and of the FC loop (the 160-column ones are always width-first)
  Reg reg = Reg::loop;
  Smpl smpl = Smpl::f32;
};

KernelPlan select_kernels(const tepose_model* m, int B, int T, bool window = false, bool assume_ready = false);
std::string describe_plan(const tepose_model* m, int B, int T);      // what tepose_select_kernels returns
void refresh_kernel_info(tepose_model* m);                           // tepose_kernel_info's string, after a knob changed

}  // namespace tepose
