/* tepose_amd.h -- C ABI of libtepose_hip.so: the MI355X (gfx950) implementation of the
 * TePose per-window inference hot path.
 *
 * The reference (ostadabbas/TePose) is pure Python/PyTorch and has no FFI layer; its
 * boundary for this path is the Python module API of lib/models.  The
 * entry points below are what the Python drop-in (tepose_amd/tepose.py, spin.py, smpl.py)
 * binds through ctypes; each one names the reference code it replaces (paths relative to
 * the reference repo root).
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t, or a negative
 *     TEPOSE_E_* error; nothing throws or aborts; no forward entry point synchronises
 *     (tepose_status does, on the stream it is given: that is its purpose; the pack /
 *     adopt / derive functions synchronise at set-up time);
 *   - all `const float*` / `float*` arguments are DEVICE pointers owned by the caller
 *     (fp32, contiguous unless a stride is given); the library never frees them and keeps
 *     none beyond the call, except the packed-weight blob registered in a model handle;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - a handle is host memory only (plus one word of pinned host memory, the fault word
 *     below); calls on one handle are re-entrant across streams as long as each call gets
 *     its own workspace;
 *   - a `workspace` needs no initialisation: a forward's results depend only on its inputs
 *     and the packed weights, not on what the workspace held before (every counter, tag,
 *     status word and padding a kernel reads is cleared or written earlier in the same
 *     call's stream order; DESIGN.md section 3 lists them);
 *   - a forward writes only inside [workspace, workspace + tepose_*_workspace_bytes(...))
 *     and inside the first B (N) rows of each output, and never its inputs: a caller may
 *     hand in row slices of larger tensors (tests/test_gpu_buffers.py holds both);
 *   - tepose_workspace_bytes() must be queried again after every tepose_pack_* / tepose_adopt_blob
 *     call: what was packed (e.g. a weight outside the fp16 range) can change the kernels a
 *     forward uses and with them the workspace it needs.
 */
#ifndef TEPOSE_AMD_H
#define TEPOSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEPOSE_ABI_VERSION 1

#define TEPOSE_E_ARG (-1)       /* null pointer / non-positive size / bad enum           */
#define TEPOSE_E_SHAPE (-2)     /* dimension not supported (see each function)           */
#define TEPOSE_E_WORKSPACE (-3) /* workspace smaller than tepose_*_workspace_bytes()     */
#define TEPOSE_E_STATE (-4)     /* handle not packed yet / blob of another model         */
#define TEPOSE_E_TIMEOUT (-5)   /* a persistent small-batch kernel gave up waiting: that forward's outputs are NaN */

#define TEPOSE_FEAT 2048        /* ResNet feature width (lib/models/tepose.py:68)         */
#define TEPOSE_THETA 85         /* cam3 + pose72 + shape10 (lib/models/spin.py:285)       */
#define TEPOSE_INPUT 2133       /* GRU input_size (lib/models/tepose.py:54,60)            */
#define TEPOSE_NVERT 6890
#define TEPOSE_NJOINT 24

typedef struct tepose_model tepose_model; /* opaque */

int tepose_version(void);
/* How the library was built: "gfx950 packed_fp32=off" for the supported build (hipcc ... -Xclang -target-feature -Xclang
 * -packed-fp32-ops -DTEPOSE_NO_PACKED_FP32=1, see __graft_entry__.py).  gfx950 erratum (reproducer
 * tools/micro/pk_chain_mfma.hip): v_pk_fma_f32 with op_sel[1] = 1 returns a wrong low result in lanes 48..63 next to LDS + MFMA
 * workgroups on the same CU; a build with packed fp32 VALU instructions gave wrong SMPL vertices in 1-3 % of the launches when a
 * GEMM of another process / stream shared the GPU.  Bindings should refuse or warn on "packed_fp32=on".                        */
const char* tepose_build_info(void);
const char* tepose_error_string(int code);

/* ---- model handle ------------------------------------------------------------------
 * Replaces TePose.__init__ / TemporalEncoder.__init__ / Regressor.__init__
 * (lib/models/tepose.py:44-69,90-118; lib/models/spin.py:209-238).
 * n_layers >= 1, hidden >= 1 (padded internally to a multiple of 64).               */
int tepose_create(int n_layers, int hidden, tepose_model** out);
void tepose_destroy(tepose_model* m);
/* "projection=<kernel symbol>;gru_step=<kernel symbol>": the kernels this handle's knobs (environment at creation) select for
 * the two dominant launch families of a large-batch forward, as a rocprofv3 kernel trace spells them.  A committed profile
 * (profiles/rNN_traffic_*.json) describes the running binary only if it names the same symbols; bench.py marks it stale
 * otherwise.  The string lives as long as the handle.                                                                    */
const char* tepose_kernel_info(const tepose_model* m);
/* Options are PER HANDLE (no global mutable state).  tepose_create reads the environment ONCE into the handle: the numerics / family
 * knobs (TEPOSE_EXACT_FP32, TEPOSE_LARGE_BATCH_KERNELS, TEPOSE_GRU_STATE, TEPOSE_COLLAPSE_REGRESSOR, TEPOSE_PERSISTENT, ...) and every launch
 * threshold (csrc/common.h `Options`: SKINNY_MAX_M, SKINNY_H3_MAX_M, SPLIT_MIN_M, SPLIT_FEW_MAX_ROWS, SEQ_MAX_M, SEQ_GRAN_MAX_M, REG_SEQ_MAX_N,
 * SMPL_SMALL_MAX_N, L1_SKINNY_MAX_ROWS, G0_MID_MIN_ROWS, G0_SKINNY_MAX_M, S16_GM, S16_WALK, GRU_GM, H3_TILE64, ASSUME_CUS, ...; plus S_MIN_B,
 * BLEND16_MIN_N, GI_BLK, SEQ_SPIN_LIMIT).  Nothing in the library reads a threshold from the environment afterwards, and no launcher keeps
 * process-wide state: two handles of one process may differ.  tepose_set_option changes one integer option of THIS handle by name (with or
 * without the TEPOSE_ prefix); it is refused with TEPOSE_E_STATE once anything has been packed (workspace sizes and packed planes depend on
 * the options) and with TEPOSE_E_ARG for an unknown name.  tepose_get_option returns the current value (-1: unknown name).  The handle-less
 * test entry points (tepose_gemm_f32, tepose_gemm_h3_f32) take the environment's values at each call.                                   */
int tepose_set_option(tepose_model* m, const char* name, long value);
long tepose_get_option(const tepose_model* m, const char* name);
/* The whole kernel selection of an eval forward of B windows x T frames on this handle, family by family ("input=...;projection=...;gi0_layout=...;
 * gru_step=...;gru_first=...;projection_l1=...;gi1_layout=...;tail_regressor=...;smpl=..."), as the launch code itself decides it (csrc/plan.hip
 * select_kernels: the ONE place where batch classes are told apart).  A pure host function of the handle's knobs (environment at creation: TEPOSE_EXACT_FP32,
 * TEPOSE_LARGE_BATCH_KERNELS=scaled|twoacc, TEPOSE_GRU_STATE=planes|fp32, TEPOSE_S_MIN_B, ...), L, hidden, B, T -- no device needed (the persistent
 * small-batch kernels plan with the device's CU count, or TEPOSE_ASSUME_CUS where none is visible).  The string belongs to the calling thread and is
 * valid until its next call.                                                                                                  */
const char* tepose_select_kernels(const tepose_model* m, int B, int T);

/* Bytes of the single device blob that holds every packed constant of the model
 * (encoder + regressor + SMPL tables).  The caller allocates it; it is what gets
 * broadcast to the other ranks of a node.                                            */
size_t tepose_packed_bytes(const tepose_model* m);
int tepose_set_blob(tepose_model* m, void* blob, size_t bytes);
/* Declare that the registered blob already holds a fully packed model (it was filled by
 * tepose_pack_* on another handle of the same n_layers/hidden and copied or broadcast
 * here, e.g. rank 0 -> all ranks over RCCL).                                          */
int tepose_adopt_blob(tepose_model* m);

/* Broadcast less: the blob interleaves the fp32 sections (packed matrices, biases, SMPL tables, the collapsed maps, the
 * header) with the fp16 hi / lo plane copies the split-precision kernels read, and every plane is a function of the fp32
 * section next to it.  tepose_fp32_ranges fills offsets[] / sizes[] (bytes, at most `cap` entries, returns the count or a
 * negative error) with the ranges a sender has to transmit -- 276 of 770 MB at n_layers = 2 / hidden = 1024; the receiver
 * copies them into a zeroed blob of tepose_packed_bytes(), registers it with tepose_set_blob and calls tepose_derive_planes,
 * which rebuilds every plane (bit-identical to the sender's) and then adopts the blob as tepose_adopt_blob does.            */
int tepose_fp32_ranges(const tepose_model* m, size_t* offsets, size_t* sizes, int cap);
int tepose_derive_planes(tepose_model* m, void* stream);

/* Pack encoder weights.  `w` = HOST array of DEVICE pointers in the reference's
 * state-dict order, n_w = 8*L + 16*L... precisely:
 *   for l in 0..L-1:  gru_fwd.{weight_ih,weight_hh,bias_ih,bias_hh}_l{l}
 *   for l in 0..L-1, sfx in ("", "_reverse"): gru_rec.{weight_ih,weight_hh,bias_ih,bias_hh}_l{l}{sfx}
 *   linear_fwd.weight, linear_fwd.bias, linear_rec.weight, linear_rec.bias
 * i.e. n_w = 12*L + 4.  Shapes as torch.nn.GRU / nn.Linear make them
 * (lib/models/tepose.py:53-69).                                                      */
int tepose_pack_encoder(tepose_model* m, const float* const* w, int n_w, void* stream);

/* Pack regressor weights: w = { fc1.weight[1024,2205], fc1.bias, fc2.weight[1024,1024],
 * fc2.bias, decpose.weight[144,1024], decpose.bias, decshape.weight[10,1024],
 * decshape.bias, deccam.weight[3,1024], deccam.bias, init_pose[144], init_shape[10],
 * init_cam[3] }  (lib/models/spin.py:215-238), n_w = 13.                             */
int tepose_pack_regressor(tepose_model* m, const float* const* w, int n_w, void* stream);

/* Pack SMPL tables (the buffers smplx.SMPL registers + lib/models/smpl.py:67-68):
 * v_template[6890,3], shapedirs[6890,3,10], posedirs[207,20670], J_regressor[24,6890],
 * lbs_weights[6890,24], J_regressor_extra[9,6890]; `parents` is a HOST int32[24].
 * Re-callable: evaluate.py:130-135 swaps model.regressor.smpl per gender.            */
int tepose_pack_smpl(tepose_model* m, const float* v_template, const float* shapedirs,
                     const float* posedirs, const float* J_regressor, const float* lbs_weights,
                     const float* J_regressor_extra, const int32_t* parents_host, void* stream);

/* Optional evaluation joint regressor (J_regressor_h36m[17,6890], evaluate.py:109,
 * lib/models/spin.py:275-278).  Packed into a caller-provided device buffer of
 * tepose_jreg_packed_bytes() so several regressors can coexist.                       */
size_t tepose_jreg_packed_bytes(void);
int tepose_pack_jreg(const float* J_regressor_17x6890, void* packed, void* stream);

/* ---- forward ------------------------------------------------------------------------ */
size_t tepose_workspace_bytes(const tepose_model* m, int B, int T);

/* TemporalEncoder.forward (lib/models/tepose.py:71-87).
 * x[B,T,2133] -> feat: eval mode [B,2048] = (y_fwd + y_rec)/2 ; is_train != 0 writes
 * [B,2,2048] = stack(y_fwd, y_rec).                                                  */
int tepose_encoder_fwd(const tepose_model* m, const float* x, int B, int T, int is_train,
                       float* feat, void* workspace, size_t ws_bytes, void* stream);

/* Regressor.forward (lib/models/spin.py:240-291) incl. rot6d_to_rotmat
 * (lib/utils/geometry.py:330-344), SMPL wrapper (lib/models/smpl.py:72-84 over
 * smplx.lbs), projection (spin.py:307-351), rotation_matrix_to_angle_axis
 * (geometry.py:68-233).  feat[N,2048] -> theta[N,85], verts[N,6890,3], kp_3d[N,J,3],
 * kp_2d[N,J,2], rotmat[N,24,3,3]; J = 14 when jreg_packed != NULL (H36M_TO_J14 path),
 * else 49.  n_iter = 3 in the reference.  With n_iter = 3 and the model's own initial state a split-mode handle runs the
 * loop as ONE product: the loop has no activation and Dropout is the identity in eval mode, so it is an affine map of the
 * feature, formed in fp64 by tepose_pack_regressor (TEPOSE_COLLAPSE_REGRESSOR=0 or TEPOSE_EXACT_FP32=1 at
 * tepose_create keep the loop).  Same results to ~2e-6.                                                              */
int tepose_regressor_fwd(const tepose_model* m, const float* feat, int N, int n_iter,
                         const void* jreg_packed, float* theta, float* verts, float* kp_3d,
                         float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes,
                         void* stream);

/* Same with the caller's initial state (Regressor.forward(x, init_pose=, init_shape=, init_cam=, n_iter=),
 * lib/models/spin.py:240-251): init_pose[N,144] (6D), init_shape[N,10], init_cam[N,3] device rows, each may be NULL
 * = the model's mean-parameter buffer.  n_iter = 0 returns SMPL(init state) -- rot6d_to_rotmat and
 * rotation_matrix_to_angle_axis of the given pose, which is how the geometry edge cases are tested.           */
int tepose_regressor_fwd_init(const tepose_model* m, const float* feat, int N, int n_iter, const float* init_pose,
                              const float* init_shape, const float* init_cam, const void* jreg_packed,
                              float* theta, float* verts, float* kp_3d, float* kp_2d, float* rotmat,
                              void* workspace, size_t ws_bytes, void* stream);

/* TePose.forward, eval mode (lib/models/tepose.py:121-136) = the two calls above.     */
int tepose_forward(const tepose_model* m, const float* x, int B, int T, const void* jreg_packed,
                   float* theta, float* verts, float* kp_3d, float* kp_2d, float* rotmat,
                   void* workspace, size_t ws_bytes, void* stream);

/* ---- failure channel of the persistent small-batch kernels ------------------------------------
 * Batches of <= 64 windows run each GRU layer (and an iterating regressor) as ONE persistent launch whose
 * workgroups hand the recurrent state to each other through L2; that needs all of them resident at once (<= 192
 * of the 256 CUs).  On a GPU that is shared with another process or CU-masked they may not be; every wait is
 * therefore bounded (~2 s), and a launch that gives up poisons that forward's outputs with NaN AND raises the
 * handle's fault word (pinned host memory, written by the kernel).  The reference has no silent-garbage mode
 * (an exception ends evaluate.py:255); neither has this boundary:
 *   - tepose_forward_status(m, workspace, stream): synchronises `stream` and answers for ONE forward -- the last one that ran
 *     with this workspace: TEPOSE_E_TIMEOUT (once; the workspace's status words and the handle's word are cleared) if one of
 *     its persistent launches gave up, else 0.  The status words live in the workspace, which concurrent forwards never
 *     share, so this is the call for a handle that several streams / threads drive at once.
 *   - tepose_status(m, stream): synchronises `stream`, returns TEPOSE_E_TIMEOUT if ANY forward on `m` gave up since the last
 *     call (and clears the handle's word), else 0.  Handle-wide: with one handle on several streams the caller that polls
 *     first collects the fault, whichever forward raised it -- use it only with one stream per handle, or use
 *     tepose_forward_status.  Call one of the two wherever the outputs are about to be trusted.
 *   - tepose_status_peek(m): the handle-wide test without synchronising or clearing.
 *   - every forward entry point (tepose_forward, tepose_forward_cached, tepose_encoder_fwd,
 *     tepose_regressor_fwd[_init]) returns TEPOSE_E_TIMEOUT up front while the word is raised.
 *   - tepose_set_persistent(m, 0) (or TEPOSE_PERSISTENT=0 at tepose_create): the step-per-launch HIP kernels at
 *     every batch size -- same results, no residency requirement; the remedy after a TEPOSE_E_TIMEOUT.  The switch is one
 *     atomic flag: it may be flipped while other threads run forwards on the handle (each forward reads it once).
 *   - tepose_uses_persistent(m, B, T): 1 if a forward of B windows may launch a persistent kernel.
 * The large-batch projection kernel (csrc/gemm_h3s16c.hip) has no workgroup barriers; its waves wait on LDS arrival counters with
 * bounded polls.  No wait there depends on another workgroup, so only a kernel bug or a hardware fault can expire one -- but if one
 * does, it is reported the same way (NaN in the output, status word of the forward's workspace = 4, the handle's fault word), never
 * as a plausible result with rc 0.  Large batches are not synchronised by the library: the next entry point on the handle refuses
 * with TEPOSE_E_TIMEOUT, tepose_forward_status / tepose_status answer after their synchronisation.  tepose_set_persistent does not
 * affect this kernel.                                                                                          */
int tepose_forward_status(tepose_model* m, void* workspace, void* stream);
int tepose_status(tepose_model* m, void* stream);
int tepose_status_peek(const tepose_model* m);
/* Which kernel raised the fault: the handle's fault word while it is raised, else the code of the last fault a status call collected (0 = none yet).
 * 1, 3 = the persistent recurrent kernel (gru_seq.hip; 3: a peer workgroup not resident after half the bound), 2 = the persistent regressor kernel
 * (reg_seq.hip) -- residency problems: tepose_set_persistent(m, 0) is the remedy; 4 = a bounded LDS poll of the barrier-free projection kernel
 * (gemm_h3s16c.hip) expired -- no wait there depends on another workgroup, so this is a kernel bug or a hardware fault, NOT a residency problem: switching
 * the persistent kernels off does not help, report it.                                                                                        */
int tepose_fault_code(const tepose_model* m);
int tepose_set_persistent(tepose_model* m, int on);
int tepose_uses_persistent(const tepose_model* m, int B, int T);
/* Tests only: what TEPOSE_TEST_FAULT sets at tepose_create (bit 2: every poll of the barrier-free projection kernel; bit 0 / 1: the waits of the persistent recurrent / regressor
 * kernels launched from now on expect an arrival that never comes), changeable on a live handle -- e.g. between the warm-up
 * and the capture of a hipGraph, so that the give-up happens inside a replay (tests/test_gpu_stream.py).                  */
int tepose_debug_set_test_fault(tepose_model* m, unsigned bits);
/* Tests / monitoring: how many waves of the barrier-free GEMM kernels (gemm_h3s16c.hip) ever gave up a bounded poll in this
 * process (they cannot unless the kernel has a bug: a wave only waits for waves of its own workgroup); 0 = never.         */
unsigned tepose_debug_kernel_errors(void);

/* ---- sliding-window driver with cached layer-0 projections ---------------
 * Consecutive windows of a clip share T-1 frames, and a frame's layer-0 gate pre-activations
 * x W_ih^T + b_ih (all three directions, 9*Hp floats) do not change once its theta is known
 * (evaluate.py:248-269).  The caller keeps, per clip, a ring of `ring` >= T-1 frame slots
 * (slot = frame % ring) plus one row for the newest frame (theta = 0).
 * tepose_project_frames: one frame per clip: feat row b at feat + b*feat_ld (2048 floats),
 * theta row at theta + b*theta_ld (85 floats) or theta == NULL for zeros  ->  out + b*out_ld.
 * workspace >= tepose_project_frames_workspace_bytes(m, B) (the padded rows, plus their fp16 planes when
 * the product runs on the split-precision kernel, i.e. with the numerics tepose_forward uses at that B). */
size_t tepose_project_frames_workspace_bytes(const tepose_model* m, int B);
int tepose_project_frames(const tepose_model* m, const float* feat, long feat_ld, const float* theta,
                          long theta_ld, int B, float* out, long out_ld, void* workspace,
                          size_t ws_bytes, void* stream);
/* Both projections of one window step in one call (the previous newest frame with its now-known theta -> out_prev rows, the newest frame with zero
 * theta -> out_new rows): ONE product of 2 B rows, so the layer-0 weights are streamed once per step.  The same GEMM rows on the same operands as two
 * tepose_project_frames calls (equal to rounding: the width-first kernel may group the K partial sums differently at another row count; bit for bit at
 * the published width); B <= 4 and 2 B > 768 run as those two calls.  workspace >= tepose_project_frames_workspace_bytes(m, 2 * B).     */
int tepose_project_frame_pair(const tepose_model* m, const float* feat_prev, const float* feat_new, long feat_ld, const float* theta_prev,
                              long theta_ld, int B, float* out_prev, long out_prev_ld, float* out_new, long out_new_ld, void* workspace,
                              size_t ws_bytes, void* stream);
/* One iteration of the reference's window loop (evaluate.py:247-269, demo.py:238-252) for B clips in lock-step as ONE call: tepose_project_frame_pair
 * (previous newest frame with its now-known theta -> `out_prev`, normally its ring slot; newest frame with zero theta -> `newest`) followed by
 * tepose_forward_cached on the window starting at ring slot `first_slot`.  Same arguments and results as those two calls (workspace >=
 * tepose_workspace_bytes(m, B, T), pair_workspace >= tepose_project_frames_workspace_bytes(m, 2 * B)); the forward's sync region is cleared by the
 * projection's input-split kernel instead of a memset node of its own.                                                                        */
int tepose_window_step(const tepose_model* m, const float* feat_prev, const float* feat_new, long feat_ld, const float* theta_prev, long theta_ld,
                       float* out_prev, long out_prev_ld, float* newest, long newest_ld, const float* ring_base, int ring, int first_slot,
                       long clip_stride, int B, int T, const void* jreg_packed, float* theta, float* verts, float* kp_3d, float* kp_2d, float* rotmat,
                       void* workspace, size_t ws_bytes, void* pair_workspace, size_t pair_ws_bytes, void* stream);
/* TePose.forward for the window whose first frame sits in ring slot `first_slot`; clip b's ring
 * starts at ring_base + b*clip_stride; newest frame's row at newest + b*newest_ld.  Outputs and
 * workspace as tepose_forward.  Saves the T-fold re-projection (42 % of the FLOPs at T = 16).  */
int tepose_forward_cached(const tepose_model* m, const float* ring_base, int ring, int first_slot,
                          long clip_stride, const float* newest, long newest_ld, int B, int T,
                          const void* jreg_packed, float* theta, float* verts, float* kp_3d,
                          float* kp_2d, float* rotmat, void* workspace, size_t ws_bytes, void* stream);

/* ---- VIBE bootstrap encoder (lib/models/vibe.py:27-117; used by evaluate.py:89-107,233-245
 * and demo.py:104-130,229-237 to predict the first seqlen-1 frames) ----------------------
 * A handle made by tepose_create_vibe_ex holds: GRU(2048 -> hidden, n_layers, bidirectional),
 * Linear(D*hidden -> 2048) on relu(y) when bidirectional or add_linear (vibe.py:43-47; D = 2 when
 * bidirectional), residual add when the output is 2048 wide, plus the same regressor / SMPL sections
 * as a TePose handle (tepose_pack_regressor / tepose_pack_smpl / tepose_regressor_fwd work
 * on it).  w = { for l, for direction (forward, then reverse): gru.weight_ih, weight_hh, bias_ih,
 * bias_hh ; then linear.weight, linear.bias when present }, n_w = 4*L*D (+ 2) -- nn.GRU's parameter order.
 * tepose_create_vibe(n_layers, hidden) = tepose_create_vibe_ex(n_layers, hidden, 0, 1): the configuration
 * both reference callers build (evaluate.py:93-101).                                            */
int tepose_create_vibe(int n_layers, int hidden, tepose_model** out);
int tepose_create_vibe_ex(int n_layers, int hidden, int bidirectional, int add_linear, tepose_model** out);
int tepose_pack_vibe_encoder(tepose_model* m, const float* const* w, int n_w, void* stream);
size_t tepose_vibe_workspace_bytes(const tepose_model* m, int B, int N);
/* width F of the encoder's output rows: 2048 with the linear, hidden without (0: not a VIBE handle) */
int tepose_vibe_feature_dim(const tepose_model* m);
/* x[B,N,2048] -> feat[B*N,F] (row b*N+t) = linear(relu(gru(x))) or gru(x), + x when use_residual and F = 2048. */
int tepose_vibe_encoder_fwd(const tepose_model* m, const float* x, int B, int N, int use_residual,
                            float* feat, void* workspace, size_t ws_bytes, void* stream);

/* ---- HMR feature extractor (lib/models/spin.py:59-141: the ResNet-50 backbone that demo.py:116-121,193 and
 * lib/data_utils/_feature_extractor.py run on 224 x 224 crops) -------------------------------------------------
 * A handle made by tepose_create_hmr holds the backbone's 53 convolutions with their inference batch norms folded in
 * (w' = w * gamma / sqrt(var + 1e-5), b' = beta - mean * gamma / sqrt(var + 1e-5), in fp64 at pack time), plus the same
 * regressor / SMPL sections as the other kinds: tepose_pack_regressor, tepose_pack_smpl, tepose_regressor_fwd[_init] (the HMR
 * head, spin.py:167-201), tepose_set_blob, tepose_adopt_blob, tepose_fp32_ranges, tepose_derive_planes and the option calls work on it.
 * tepose_pack_hmr_backbone: w = HOST array of DEVICE pointers in state-dict order, per convolution
 *   { conv.weight[C_out,C_in,R,R], bn.weight, bn.bias, bn.running_mean, bn.running_var }   (num_batches_tracked is not passed)
 * for conv1/bn1, then per block conv1/bn1, conv2/bn2, conv3/bn3 and, in a stage's first block, downsample.0/.1: n_w = 5 * 53 = 265.
 * TEPOSE_E_ARG for another count, a null entry, running_var + 1e-5 <= 0 or a non-finite folded value.  A folded |w'| >= 2^15 puts
 * the handle on the exact-fp32 kernels, as for the other sections.
 * tepose_hmr_features: x[N,3,224,224] (NCHW fp32, as the callers hand it over) -> feat[N,2048].  Asynchronous on `stream`, no
 * allocation, no synchronisation, capturable.  Images are processed in passes of at most 64; workspace >=
 * tepose_hmr_workspace_bytes(m, N) (that of min(N, 64) images).  TEPOSE_E_STATE on a handle of another kind or before the
 * backbone is packed.  Every convolution is a gather (im2col rows as the product's A operand) and one product on the kernels
 * of tepose_gemm_h3_f32 (default) or tepose_gemm_f32 (TEPOSE_EXACT_FP32=1 at creation).                                    */
int tepose_create_hmr(tepose_model** out);
int tepose_pack_hmr_backbone(tepose_model* m, const float* const* w, int n_w, void* stream);
size_t tepose_hmr_workspace_bytes(const tepose_model* m, int N);
int tepose_hmr_features(const tepose_model* m, const float* x, int N, float* feat, void* workspace, size_t ws_bytes, void* stream);

/* ---- evaluation metrics on the device (evaluate.py:413-457, lib/utils/eval_utils.py) -------
 * Joint metrics per frame, in mm: pred/target [N,J,3] (J <= 17) are pelvis-aligned inside
 * (pelvis_mode 0: mean of joints 2,3 -- 3DPW / H36M 14-joint order, evaluate.py:424-425;
 * 1: joint J-3 -- mpii3d_test order, evaluate.py:420-422).  mpjpe[N], pa_mpjpe[N]
 * (batch_compute_similarity_transform_torch, eval_utils.py:287-337), accel[N] (second
 * difference, eval_utils.py:110-138; 0 for the first and last frame of the sequence).     */
int tepose_metrics_joints(const float* pred, const float* target, int N, int J, int pelvis_mode,
                          float* mpjpe, float* pa_mpjpe, float* accel, void* stream);
/* Vertices of the ground-truth mesh from theta[N,85] = cam3 | axis-angle 72 | betas 10 with
 * pose2rot=True (eval_utils.py:155-169).  Workspace >= tepose_workspace_bytes(m, ceil(N/2), 1). */
int tepose_smpl_verts_from_theta(const tepose_model* m, const float* theta, int N, float* verts,
                                 void* workspace, size_t ws_bytes, void* stream);
/* Standalone SMPL forward as callers use the class directly (lib/utils/smooth_pose.py:35-64 with
 * axis-angle, evaluate.py:279-286 with rotation matrices; lib/models/smpl.py:72-84):
 * pose2rot != 0: pose[N,72] axis-angle (global orient first); == 0: pose[N,24,3,3].  betas[N,10].
 * verts[N,6890,3]; joints49[N,49,3] (may be NULL).  Needs tepose_pack_smpl only.          */
int tepose_smpl_fwd(const tepose_model* m, int pose2rot, const float* pose, const float* betas, int N,
                    float* verts, float* joints49, void* workspace, size_t ws_bytes, void* stream);
/* Backward of tepose_smpl_fwd: the gradients of a scalar loss with respect to pose and betas, given its gradients with respect to
 * the vertices and / or the 49 joints -- autograd's through smplx's batch_rodrigues (angle = |aa + 1e-8|), LBS and the joint map
 * (DESIGN.md section 19).  pose / betas / pose2rot as in the forward call; g_verts [N,6890,3] or NULL (= zeros); g_joints49 [N,49,3]
 * or NULL (= zeros); g_pose: pose2rot != 0: [N,72], == 0: [N,24,3,3] (the gradient of every matrix entry, no orthogonality
 * constraint), may be NULL; g_betas [N,10], may be NULL.  Stateless: what the backward needs of the forward (transforms, v_posed) is
 * recomputed from (pose, betas); nothing is kept between calls.  No allocation, no synchronisation (capturable in a graph); no
 * atomics: two calls on the same inputs agree bit for bit.  Workspace >= tepose_smpl_bwd_workspace_bytes(m, N) (0 for N outside
 * [1, 65536]).  Before any device call: TEPOSE_E_ARG for a NULL pose / betas / workspace, then for both gradients-in NULL while a
 * gradient-out is asked for; TEPOSE_E_SHAPE for N outside [1, 65536]; TEPOSE_E_STATE before tepose_pack_smpl;
 * TEPOSE_E_WORKSPACE.  Needs tepose_pack_smpl only.                                                                              */
int tepose_smpl_bwd(const tepose_model* m, int pose2rot, const float* pose, const float* betas, int N, const float* g_verts,
                    const float* g_joints49, float* g_pose, float* g_betas, void* workspace, size_t ws_bytes, void* stream);
size_t tepose_smpl_bwd_workspace_bytes(const tepose_model* m, int N);
/* kp_3d[N,14,3] = (J_regressor_h36m verts[N,6890,3])[H36M_TO_J14]: the joints of given meshes as evaluate.py:289-291 regresses them in its
 * --filter branch (slerp-smoothed rotations -> SMPL -> vertices -> these joints).  jreg_packed from tepose_pack_jreg; needs tepose_pack_smpl only. */
int tepose_joints_from_verts(const tepose_model* m, const void* jreg_packed, const float* verts, int N, float* kp_3d, void* stream);
/* MEASUREMENT ONLY (tools/smpl_per_person_bench.py): the same vertices as tepose_smpl_fwd(pose2rot=1)
 * with blend shapes + skinning done by one wavefront per person (BASELINE.json's sketch of the SMPL stage) instead of a
 * GEMM over 128-person tiles + a skinning kernel.  Never called by the product path.                                   */
int tepose_smpl_fwd_per_person(const tepose_model* m, const float* pose, const float* betas, int N, float* verts,
                               void* workspace, size_t ws_bytes, void* stream);
/* mpvpe[N] = mean_v |pred_verts - target_verts| in mm (eval_utils.py:173-175).             */
int tepose_metrics_verts(const float* pred_verts, const float* target_verts, int N, float* mpvpe,
                         void* stream);

/* ---- temporal post-filters over one sequence (evaluate.py --filter, demo smoothing) ----------
 * OneEuro filter (lib/utils/one_euro_filter.py as lib/utils/smooth_pose.py:24-67 drives it:
 * timestamps = frame indices, x0 = first frame, dx0 = 0): x[N,D] filtered in place.        */
int tepose_filter_one_euro(float* x, int N, int D, float min_cutoff, float beta, float d_cutoff,
                           void* stream);
/* Quaternion slerp smoothing of joint rotations (evaluate.py:32-59): rotmat_in[N,J,3,3] ->
 * rotmat_out (may alias): sign-continuous quaternions, q_t = slerp(q_{t-1}, q_t, ratio).    */
int tepose_filter_slerp(const float* rotmat_in, float* rotmat_out, int N, int J, double ratio,
                        void* stream);

/* ---- geometry helpers as callers use them on their own (lib/utils/demo_utils.py:112,
 * lib/data_utils/threedpw_utils.py:98); the device functions are the ones the regressor kernel inlines ----
 * rotation_matrix_to_angle_axis (lib/utils/geometry.py:68-233): R[N,3,3] -> aa[N,3], NaN -> 0.         */
int tepose_rotmat_to_angle_axis(const float* R, int N, float* aa, void* stream);
/* rot6d_to_rotmat (lib/utils/geometry.py:330-344): x6[N,6] (x.view(-1,3,2)) -> R[N,3,3].                */
int tepose_rot6d_to_rotmat(const float* x6, int N, float* R, void* stream);

/* ---- person crops of video frames (the reference's CropDataset: lib/dataset/inference.py:58-74 over
 * lib/data_utils/_img_utils.py:53-101,219-252,322-330 -- warpAffine(INTER_LINEAR, BORDER_CONSTANT), ToTensor, Normalize) ----
 * frames[F,H,W,3]: uint8 RGB, contiguous, device.  frame_index[n] (device): the frame each crop is cut from.  minv[n,6] (device,
 * fp64): row-major 2 x 3 map from crop pixel (u, v) to frame coordinates, x = m0 u + m1 v + m2, y = m3 u + m4 v + m5, integer
 * coordinates at pixel centres; evaluated in fp64.  S: crop side (224 for HMR; any S in [1, 32768], TEPOSE_E_SHAPE above).
 * Bilinear over four taps, each tap outside the frame contributing 0 on its own; raw = floor(value + 0.5) as uint8;
 * out = (raw / 255 - mean[c]) / std[c] with the ImageNet constants.  out_nchw[n,3,S,S] (fp32) and raw_nhwc[n,S,S,3] (uint8): either
 * may be NULL, not both.  A frame_index outside [0, F) gives the all-zero 8-bit crop and reads nothing.  One launch for all n crops;
 * n == 0 returns 0 without a launch.  Handle-less; never allocates or synchronises.  TEPOSE_E_ARG (before any device call): n < 0,
 * S / H / W / F < 1, a NULL frames / frame_index / minv with n > 0, both outputs NULL.  DESIGN.md section 14.               */
int tepose_crop_frames_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const double* minv, int n, int S,
                          float* out_nchw, uint8_t* raw_nhwc, void* stream);

/* The same crops from BOXES: the map of each row is formed on the device, in fp64, by the rule of tepose_amd.crop.crop_transform followed by
 * invert_affine (the reference's gen_trans_from_patch_cv at rot = 0 and cv2.warpAffine's inversion) -- bit for bit the map the host forms, so
 * a crop equals tepose_crop_frames_u8's on that map.  boxes[n,4] (device, fp64): c_x, c_y, w, h in frame pixels; scale: the box scale
 * (demo.py's bbox_scale).  ops (device, int32[n], or NULL): with it, a row is cropped only when its code is 1 or 2 (the codes of
 * tepose_session_advance under which a slot consumes a feature); any other code gives the all-zero 8-bit crop and reads neither box, frame
 * index nor frame.  A box whose map is not finite (w = 0, NaN) gives the all-zero crop as well.  minv_out (device, fp64 [n,6], or NULL): a
 * test output, the map each row used (six zeros for a row its op switched off).  Everything else -- frames, frame_index, S, the two outputs,
 * one launch, n == 0, handle-less, never allocates or synchronises (graph-capturable) -- as tepose_crop_frames_u8.  TEPOSE_E_ARG (before any
 * device call): that entry's conditions with boxes in place of minv, and a scale that is not finite or <= 0; then TEPOSE_E_SHAPE for
 * S > 32768 or n > 4096.  DESIGN.md section 18.                                                                                          */
int tepose_crop_boxes_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const double* boxes, double scale,
                         const int* ops, int n, int S, float* out_nchw, uint8_t* raw_nhwc, double* minv_out, void* stream);

/* ---- SMPL overlay on video frames (the reference's Renderer.render, lib/utils/renderer.py:36-121, once per person and frame:
 * demo.py:390-417) -- a rasteriser pinned to the definition in csrc/render.hip and DESIGN.md section 15, not to pyrender's shader ----
 * frames[F,H,W,3] -> out[F,H,W,3]: uint8 RGB, contiguous, device; `out` may be `frames` itself.  n instances, drawn in the order given: a
 * later instance overwrites an earlier one wherever it covers, whatever the depths (instances of one frame should be contiguous in draw
 * order; the result depends on their relative order only).  Per instance: frame_index[n] (device, int32; an index outside [0, F) draws
 * nothing), verts[n,V,3] fp32, cams[n,4] fp64 (sx, sy, tx, ty), rot[n,9] fp64 row-major or NULL (identity), colors[n,3] fp32 base colour
 * in [0, 1].  Shared: faces[Fc,3] int32 (a face with an index outside [0, V) draws nothing) and the vertex -> face adjacency in CSR form,
 * vert_face_offsets[V + 1] / vert_face_list[n_adj], faces of a vertex in ascending order (ranges are clamped to the list, entries outside
 * [0, Fc) skipped: the vertex normals are summed in that order, without atomics, bit-reproducibly).
 * Test outputs, NULL in production: winner[F,H,W,2] int32 (instance, face; -1, -1 where uncovered), depth[F,H,W] fp32 (+inf where uncovered).
 * Limits (TEPOSE_E_SHAPE): H, W <= 16384; Fc <= 2^20 and n <= 4096 (the 64-bit pixel key holds 12 bits of draw order, 32 of depth, 20 of
 * face index); V <= 2^20.  workspace: 8-byte aligned, at least the size the workspace function below returns for (H, W, F, n, V, Fc)
 * -- 8 bytes per pixel of every frame plus 24 per vertex and instance; 0 for arguments outside the limits.
 * Handle-less; never allocates or synchronises: a memset, three launches.  n == 0 copies the frames.  TEPOSE_E_ARG (before any
 * device call): F / H / W / V < 1, n / Fc / n_adj < 0, NULL frames / out, with n > 0 a NULL input other than rot (faces only with Fc > 0,
 * vert_face_list only with n_adj > 0), a NULL or misaligned workspace when n > 0 or a test output is asked for.  Order: ARG, SHAPE, WORKSPACE. */
size_t tepose_render_workspace_bytes(int H, int W, int n_frames, int n_instances, int V, int Fc);
int tepose_render_meshes_u8(const uint8_t* frames, int F, int H, int W, const int* frame_index, const float* verts, int n, int V,
                            const int* faces, int Fc, const int* vert_face_offsets, const int* vert_face_list, int n_adj, const double* cams,
                            const double* rot, const float* colors, uint8_t* out, int* winner, float* depth, void* workspace,
                            size_t ws_bytes, void* stream);

/* ---- windows of a multi-person live session (tepose_amd.stream.MultiStreamSession) ----
 * win[S,T,2133] (device, fp32, contiguous): one sliding window per slot, row T - 1 the newest frame.  ops[S] (device, int32), one code per
 * slot and tick: 0 hold (window untouched, no theta fed back), 1 advance (rows 1 .. T-1 -> 0 .. T-2, row T-1 = (feat[s], 85 zeros)),
 * 2 join (rows 0 .. T-2 = hist[s], row T-1 as for 1), 3 clear (window = 0); any other value acts as 0.
 * tepose_session_advance: `saved` (NULL or [S,T,2133]) first receives the window of EVERY slot as it stood before the call, then the ops
 *   are applied: one launch, in place, no scratch.  feat[S,2048]; hist[S,T-1,2133] may be NULL when no op is 2 (a 2 then acts as 0).
 * tepose_session_commit: theta[s] ([S,85]) -> win[s][T-1][2048:] for the slots whose op is 1 or 2; nothing else is written.
 * Handle-less; neither allocates or synchronises (graph-capturable).  Before any device call: TEPOSE_E_ARG for a NULL win / ops / feat /
 * theta, then TEPOSE_E_SHAPE for S < 1, S > 4096 or T < 2.                                                                            */
int tepose_session_advance(float* win, float* saved, int S, int T, const int* ops, const float* feat, const float* hist, void* stream);
int tepose_session_commit(float* win, int S, int T, const int* ops, const float* theta, void* stream);
/* One-euro smoothing of the pose inside the tick (the reference's --smooth, lib/utils/smooth_pose.py:24-67, which is causal: x^_t depends on
 * x^_{t-1}, dx^_{t-1} and x_t only, at t_e = 1 per tracklet row).  state[S,2,72] (device, fp32): per slot (x^, dx^) of the 72 axis-angle components.
 * theta[S,85]: the model's output of this tick; hist as above.  By the slot's op code:
 *   1 advance  one filter step on theta[s][3:75] from state[s]; the new state is stored
 *   2 join     the filter has seen nothing yet: x^ = hist[s][0][2048+3 : 2048+75], dx^ = 0, then a step per history row 1 .. T-2 in order, then
 *              the step on theta[s] (T = 2: no history step).  hist may be NULL when no op is 2 (a 2 then acts as 0)
 *   3 clear    state[s] = 0
 *   0, other   hold: the state is untouched (a held tick is not a tracklet row: t_e stays 1 at the next advance)
 * saved_state (NULL or [S,2,72]) first receives the state of EVERY slot as it stood before the call (as `saved` of tepose_session_advance).
 * Outputs, rows with op 1 or 2: theta_hat[s] = (cam | pose_hat | betas) with cam and betas copied bit for bit, pose_hat[S,72] and betas_hat[S,10]
 * the same values contiguous (the operands of tepose_smpl_fwd(pose2rot = 1)).  Every other row of the three is written as zeros (a valid rest pose for
 * the SMPL launch that follows) and neither theta[s] nor hist[s] is read for it.  The step is the one of tepose_filter_one_euro -- one device function,
 * fp32, the same operation order: pose_hat equals that filter run over (history rows, advanced theta rows) in every bit.
 * One launch, one thread per (slot, theta column); handle-less; neither allocates nor synchronises (graph-capturable).  Before any device call:
 * TEPOSE_E_ARG for a NULL theta / ops / state / theta_hat / pose_hat / betas_hat or a min_cutoff / beta / d_cutoff that is not finite or is negative,
 * then TEPOSE_E_SHAPE for S < 1, S > 4096 or T < 2.                                                                                          */
int tepose_session_smooth(const float* theta, const float* hist, int S, int T, const int* ops, float* state, float* saved_state,
                          float min_cutoff, float beta, float d_cutoff, float* theta_hat, float* pose_hat, float* betas_hat, void* stream);

/* ---- building blocks exported for tests and bench.py --------------------------------- */
/* C[M,N] = (relu_a ? relu(A) : A)[M,K] * W[N,K]^T (+ bias[N]) with the library's own
 * fp32-MFMA kernel.  A rows must be 16-byte aligned (lda % 4 == 0); W is packed on the
 * fly into `workspace` (>= tepose_gemm_workspace_bytes(N,K)).                          */
size_t tepose_gemm_workspace_bytes(int N, int K);
int tepose_gemm_f32(const float* A, long lda, const float* W, long ldw, const float* bias,
                    float* C, long ldc, int M, int N, int K, int relu_a, void* workspace,
                    size_t ws_bytes, void* stream);

/* Same product on the split-precision kernel (fp16 hi/lo planes, three fp16 MFMAs per k-step, fp32
 * accumulate; csrc/gemm_h3.hip).  K % 32 == 0.  workspace >= tepose_gemm_h3_workspace_bytes(M,N,K).  */
size_t tepose_gemm_h3_workspace_bytes(int M, int N, int K);
int tepose_gemm_h3_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C,
                       long ldc, int M, int N, int K, void* workspace, size_t ws_bytes, void* stream);

/* One convolution of the HMR backbone on caller-supplied tensors: x[N,H,W,Cin] (NHWC), w[Cout,Cin,R,R] (OIHW), bias[Cout] or NULL ->
 * y[N,Ho,Wo,Cout] = conv(relu_in ? relu(x + residual) : x + residual) + bias; residual (x's shape) may be NULL; zero padding.
 * R <= 7, stride 1 or 2, 2 * pad < R.  exact != 0: the fp32-MFMA product (a 1 x 1 stride-1 convolution then runs without a gather),
 * else the split-precision product with one power-of-two scale per gathered row (any finite input).
 * workspace >= tepose_conv2d_nhwc_workspace_bytes(N,H,W,Cin,Cout,R).                                                      */
size_t tepose_conv2d_nhwc_workspace_bytes(int N, int H, int W, int Cin, int Cout, int R);
int tepose_conv2d_nhwc_f32(const float* x, int N, int H, int W, int Cin, const float* w_oihw, const float* bias, int Cout, int R,
                           int stride, int pad, int relu_in, const float* residual, float* y, int exact, void* workspace,
                           size_t ws_bytes, void* stream);
/* MaxPool2d(3, stride 2, padding 1) over NHWC (C % 4 == 0; padding contributes -inf): y[N,(H-1)/2+1,(W-1)/2+1,C].      */
int tepose_maxpool3x3s2_nhwc(const float* x, int N, int H, int W, int C, float* y, void* stream);
/* AvgPool2d(7) over x[N,7,7,C] -> y[N,C].                                                                             */
int tepose_avgpool7_nhwc(const float* x, int N, int C, float* y, void* stream);
/* The pack-time fold of tepose_pack_hmr_backbone for one convolution: w_out[Cout][Kp] in (r, s, c) order, Kp = Cin * R * R rounded
 * up to 32 (zero beyond), b_out[Cout].  Synchronises; TEPOSE_E_ARG as above.                                            */
int tepose_hmr_fold_pack(const float* w_oihw, const float* gamma, const float* beta, const float* mean, const float* var, int Cout,
                         int Cin, int R, float* w_out, float* b_out, void* stream);
/* One pass of tepose_hmr_features (1 <= N <= 64 images) that ends after convolution `last_conv` (0 .. 52, state-dict order; the max pool
 * belongs to convolution 0): the same launches with the same arguments, then two asynchronous device-to-device copies on `stream`:
 *   out    [N,Ho,Wo,C_out] (NHWC fp32) what convolution `last_conv` wrote, BEFORE its ReLU
 *   joined (may be NULL) the block input as it stands then: the max-pooled stem, or relu(conv3 + identity) of the block before, as the
 *          most recent conv1 of a block wrote it back.
 * out_floats / joined_floats (ignored without `joined`) must equal the element counts the library's layer table gives these tensors:
 * TEPOSE_E_SHAPE before any launch otherwise.  Checks in the order ARG, STATE (as tepose_hmr_features), SHAPE, WORKSPACE (tepose_hmr_workspace_bytes(m, N)).  */
int tepose_hmr_features_upto(const tepose_model* m, const float* x, int N, int last_conv, float* out, size_t out_floats, float* joined,
                             size_t joined_floats, void* workspace, size_t ws_bytes, void* stream);

/* A read-only tap of a finished encoder forward: after tepose_encoder_fwd(m, x, B, T, ..., workspace, ...) has run, called with the same m, B, T and
 * workspace, copies ONE stage out of that workspace as plain row-major fp32 -- from whichever form the plan's producer wrote and its consumer reads
 * (fp32 rows, fp32 16 x 16 blocks, or hi + lo planes where gru_step16_kernel<true> writes no fp32 state).  One gather launch on `stream`; the workspace
 * is not written.  Directions: 0 gru_fwd, 1 gru_rec reverse, 2 gru_rec forward.
 *   stage 0  gi(layer, dir)        gate pre-activations [T][B][3 Hp]; the top layer's dir 2: [1][B][3 Hp].  Layer 0 in frame order; layers >= 1 in the
 *                                  order of their input states' slabs (dir 1: slab T - 1 - step feeds cell step `step`).  Of layers >= 1 only the top
 *                                  layer's survive a forward.
 *   stage 1  h(layer, dir, step)   the state [B][Hp] that cell step wrote: every step below the top layer (not a layer that a layer two above it
 *                                  overwrote); on the top layer steps T - 1 and T - 2 of dir 0 / 1 and step 0 of dir 2.
 *   stage 2  tail                  the tail product's A operand [B][3 Hp] = relu[gru_fwd's last state | dir 2's state | dir 1's last state]
 * out_floats must equal the stage's element count; *form (may be NULL) receives the form read: 0 rows, 1 / 2 blocks, 3 / 4 planes (22 bits).
 * Checks in the order ARG, STATE, SHAPE (a stage that does not exist or did not survive, a wrong count), WORKSPACE, all before the launch.              */
int tepose_encoder_tap(const tepose_model* m, int B, int T, int stage, int layer, int dir, int step, float* out, size_t out_floats, int* form,
                       const void* workspace, size_t ws_bytes, void* stream);

/* The same for the decoder half: after tepose_regressor_fwd[_init] / tepose_smpl_fwd(m, ..., N, ..., workspace, ws_bytes) (entry 0; T ignored) or
 * tepose_forward(m, x, B = N, T, ..., workspace, ws_bytes) (entry 1) has run, copies ONE stage of it out of that workspace as fp32 [N][cols].  The
 * addresses are the call's own carve and plan; one gather launch on `stream`, the workspace is not written, nothing is allocated or synchronised.
 *   stage 0 xs         [N][160]    the regressor's final state row (pose6d 144 | shape 10 | cam 3 | pad 3); after a tail-collapsed tepose_forward it
 *                                  is read from the feature slot at the end of the workspace
 *         1 h1, 2 h2   [N][1024]   the FC activations of the last iteration (a collapsed product writes none: what they hold is the caller's knowledge);
 *                                  where the plan runs the FC loop as reg_seq_kernel they exist as hi + lo planes only, and are read from those
 *         3 pf         [N][224]    pose-feature rows [1 | betas | R - I | 0 x 6]
 *         4 pf_planes  [N][224]    ... as the blocked hi + lo / 2048 planes             only on a split-precision plan
 *         5 pf16       [N][224]    ... as the scaled planes, (hi + lo) x row scale       only where the plan runs the blend-shape product on them
 *         6 amat       [N][288]    skinning transforms [24][3][4]
 *         7 posed      [N][72]     posed joints
 *         8 vposed     [N][20670]  v_posed (the real columns of its 20672-wide rows)
 * Stages 3, 4, 5 and 8 do not exist where the one-launch small-N SMPL kernel runs.  out_floats must equal N x cols; *form (may be NULL) receives the
 * form read (0 rows, 3 / 4 planes).  Checks in the order ARG (null pointers, N < 1, unknown stage or entry), STATE (SMPL not packed), SHAPE (a wrong
 * count, a stage the plan never writes), WORKSPACE (shorter than the call's carve), all before the launch.                                              */
int tepose_decoder_tap(const tepose_model* m, int N, int stage, float* out, size_t out_floats, int* form, int entry, int T, const void* workspace,
                       size_t ws_bytes, void* stream);

/* Per-launch timing of the dominant kernel (the layer-0 input-projection GEMM) with
 * hipEvents on the launch stream: enable, run forwards, then read back.  Reading
 * synchronises on the recorded events only.  Used by bench.py for the `roofline`
 * object; off by default.                                                            */
int tepose_profile_enable(tepose_model* m, int on);
int tepose_profile_read(tepose_model* m, double* total_ms, int* n_launches, double* flops_per_launch);
/* Same switch, second kernel class: total time of the GRU-step launch sequences (one interval per layer
 * per forward) and the algorithmic FLOPs of the consumed cell steps of one forward.          */
int tepose_profile_read_gru(tepose_model* m, double* total_ms, int* n_forwards, double* flops_per_forward);
/* Third class: the layer >= 1 input projections of the encoder (tepose.py:53-64 layers 1..L-1), i.e. what runs between
 * the step sequences of two consecutive layers -- the gaps of the interval list above.  Does not reset the list
 * (tepose_profile_read_gru does): call it first.                                              */
int tepose_profile_read_l1proj(tepose_model* m, double* total_ms, int* n_forwards, double* flops_per_forward);

#ifdef __cplusplus
}
#endif
#endif /* TEPOSE_AMD_H */
