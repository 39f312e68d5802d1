// select_kernels and its description: pure host functions of a handle's knobs and a shape.
#include "plan.h"

namespace tepose {

// ---- select_kernels: every kernel-family decision of a forward of B windows x T frames ------------------------------------------------------------
// Pure host function of (handle knobs, Options, L, Hp, B, T): no device call, so tests/test_dispatch.py pins every class boundary on a machine without a
// GPU (tepose_select_kernels).  window: the plan of the cached window path (tepose_window_step / tepose_forward_cached / tepose_project_frame[s|_pair]).
// assume_ready: plan as if the fault word existed (description of a handle that has no blob yet).
KernelPlan select_kernels(const tepose_model* m, int B, int T, bool window, bool assume_ready) {
  KernelPlan k;
  const Options& o = m->opt;
  const int L = m->L, Hp = m->Hp;
  const long BT = (long)B * T;
  const bool persist = assume_ready ? m->persist : persist_on(m);
  auto split = [&](long rows, int Kp, int permT) { return split_rows_few_ok(rows, Kp, permT, o) ? Rows::split_few : Rows::split; };
  auto f32 = [&](long rows) { return rows <= gemm_skinny_max_m(o) ? Mm::f32_skinny : Mm::f32; };
  auto h3 = [&](long rows) { return rows <= o.skinny_max_m ? Mm::h3_skinny : Mm::h3; };      // few rows: the width-first kernel streams W once
  k.h3 = m->split && B > o.split_min_m;
  k.scaled = k.h3 && m->large_scaled && B >= m->s_min_b;
  k.gblk = k.scaled && m->gi_blk && Hp % 32 == 0;
  const bool planes_state = k.gblk && m->state_planes && B % 128 == 0;   // the step kernel's PLANES instantiation needs full row tiles
  k.gran = m->split && B <= gru_seq_gran_rows(o) && gru_seq_shape_ok(Hp);
  // layer-0 projection.  g0big: large batches of an L >= 2 model on the barrier-free scaled-plane kernel.  g0mid: mid-size batches (cfg-B: 1024 rows)
  // on 128 x 288 tiles, which cut the 9 Hp columns into whole rounds of the chip, where that needs less time in whole rounds of the chip
  // than 128 x 128 tiles (shapes.h g0_mid_fewer_rounds).  g0blk: gate pre-activations frame-major + blocked, whole row tiles per frame.
  const bool g0big = k.h3 && m->large_scaled && L >= 2 && BT >= 8192;
  const bool g0mid = k.h3 && m->large_scaled && L >= 2 && !g0big && BT >= o.g0_mid_min_rows && BT > 128 && h3s_mid_cols_ok(9 * Hp) && g0_mid_fewer_rounds(BT, Hp);
  if (window) {      // layer 0 from the clip's cached projections (row-major): B frame rows per product, the two of a step as one launch where it fits
    k.pair = k.h3 && 2 * B <= o.skinny_max_m;
    k.input = k.h3 ? split(B, kInputP, 0) : Rows::pad;
    k.input_pair = split(2L * B, kInputP, 0);
    k.projection = k.h3 ? h3(B) : f32(B);
  } else {
    k.g0blk = g0big && k.gblk && B % 16 == 0;
    k.input = k.h3 ? split(BT, kInputP, k.g0blk ? T : 0) : Rows::pad;
    k.projection = !k.h3 ? f32(BT) : g0big ? Mm::h3s0 : g0mid ? Mm::h3s_mid : BT <= o.g0_skinny_max_m ? Mm::h3_skinny : Mm::h3;
  }
  // layers >= 1 (the width-first kernel up to 192 real rows: three 64-row passes over the weights) and the one-step product
  const long Bs = k.h3 ? round_up(B, 16) : B;
  k.input_x0 = split(B, kInputP, 0);
  if (!k.h3) { k.proj_l1 = f32(BT); k.proj_one = f32(B); }
  else if (L == 1) k.proj_l1 = k.proj_one = Mm::h3;
  else if (k.scaled) k.proj_l1 = k.proj_one = Mm::h3s;
  else {
    k.proj_l1 = Bs * T <= o.skinny_max_m && BT <= o.l1_skinny_max_rows ? Mm::h3_skinny : Mm::h3;
    k.proj_one = B <= o.skinny_max_m && B <= o.l1_skinny_max_rows ? Mm::h3_skinny : Mm::h3;
  }
  // recurrent part: small batches run every layer's T steps as one persistent launch (2 directions on the top layer, 3 below)
  const bool seq = k.h3 && !k.scaled && persist && gru_seq_ok(L == 1 ? 2 : 3, B, Hp, T, o, device_cus(o));
  auto step = [&](bool gi_blocked) {
    if (!k.h3) return B <= o.skinny_max_m ? Step::f32_skinny : Step::f32;
    if (k.scaled) return planes_state && gi_blocked ? Step::s16_planes : Step::s16;
    if (seq) return k.gran ? Step::seq_gran : Step::seq;
    return B <= o.skinny_h3_max_m ? Step::h3_skinny : Step::h3;
  };
  k.step0 = step(k.g0blk);
  k.step1 = step(k.gblk);
  k.first = !k.h3 ? (B <= o.skinny_max_m ? First::f32_skinny : First::f32) : seq ? First::in_seq
            : k.scaled && gru_first16_shape_ok(Hp) ? First::h3_16 : First::h3;
  // tail + regressor + SMPL at N = B persons (a handle whose weights are not packed yet is described as it will be once they are)
  k.reg_collapsed = k.h3 && m->collapse_env && (m->reg_collapsed || !m->reg_packed);
  k.tail_collapsed = k.reg_collapsed && (m->tail_collapsed || !m->enc_packed);
  k.reg = k.h3 && B <= reg_seq_rows_cap(m) && persist ? Reg::seq : Reg::loop;
  k.tail = k.h3 ? h3(B) : f32(B);
  k.blend16 = k.h3 && m->large_scaled && B >= m->blend16_min_n;
  k.input_blend = split(B, kBlendK, 0);
  k.smpl = smpl_small_rows_ok(B, o) && (m->lbs_sparse || !m->smpl_packed) ? Smpl::small : k.blend16 ? Smpl::h3s : k.h3 ? Smpl::h3
           : B <= gemm_skinny_max_m(o) ? Smpl::f32_skinny : Smpl::f32;
  return k;
}

namespace {
const char* name(Rows v) { return v == Rows::pad ? "pad_input_kernel" : v == Rows::split_few ? "split_rows_few_kernel" : "split_rows_kernel"; }
const char* name(Mm v) {
  static const char* const n[] = {"gemm_f32_kernel", "skinny_gemm_kernel", "gemm_h3_kernel", "skinny_gemm_h3_kernel", "gemm_h3s_kernel<1, 3, 4, 3, 4>",
                                  "gemm_h3s_persist16c_kernel<0>", "gemm_h3s_persist16c_kernel<1>"};
  return n[(int)v];
}
const char* name(Step v) {
  static const char* const n[] = {"gru_step_kernel", "skinny_gru_kernel", "gemm_h3_kernel<GRU>", "skinny_gru_h3_kernel", "gru_seq_kernel",
                                  "gru_seq_kernel(granules)", "gru_step16_kernel<false>", "gru_step16_kernel<true>"};
  return n[(int)v];
}
const char* name(First v) {
  static const char* const n[] = {"gru_step_kernel", "skinny_gru_kernel", "gru_first_kernel", "gru_first16_kernel", "(in gru_seq_kernel)"};
  return n[(int)v];
}
const char* name(Smpl v) {
  static const char* const n[] = {"smpl_small_kernel", "smpl_prep_kernel+gemm_f32_kernel+smpl_skin4_kernel", "smpl_prep_kernel+skinny_gemm_kernel+smpl_skin4_kernel",
                                  "smpl_prep_kernel+gemm_h3_kernel+smpl_skin4_kernel", "smpl_prep_kernel+gemm_h3s_persist16c_kernel<1>+smpl_skin4_kernel"};
  return n[(int)v];
}
std::string tail_name(const KernelPlan& k) {
  if (k.tail_collapsed) return "collapsed: one product (skinny_gemm_h3_kernel)";
  const std::string tail = name(k.tail);
  if (k.reg_collapsed) return tail + " + collapsed regressor (skinny_gemm_h3_kernel)";
  if (k.reg == Reg::seq) return "reg_seq_kernel";
  return tail + (k.h3 ? " loop" : " x (2 + 1 + 9)");
}
}  // namespace

std::string describe_plan(const tepose_model* m, int B, int T) {
  const KernelPlan k = select_kernels(m, B, T, false, true), w = select_kernels(m, B, T, true, true);
  std::string s = std::string("input=") + name(k.input) + ";projection=" + name(k.projection) +
                  ";gi0_layout=" + (k.g0blk ? "frame_major_blocked" : "row_major") + ";gru_step=" + name(k.step0) + ";gru_first=" + name(k.first);
  if (m->L >= 2)
    s += std::string(";projection_l1=") + name(k.proj_l1) + ";gi1_layout=" + (k.gblk ? "blocked" : "row_major") + ";gru_step_l1=" + name(k.step1);
  s += std::string(";projection_one_step=") + name(k.proj_one) + ";tail_regressor=" + tail_name(k) + ";smpl=" + name(k.smpl);
  s += std::string(";projection_window=") + (w.pair ? "skinny_gemm_h3_kernel (pair)" : std::string(name(w.projection)) + " x 2") +
       ";gru_step_window=" + name(w.step0);
  return s;
}

void refresh_kernel_info(tepose_model* m) {
  // the symbols a rocprofv3 kernel trace of cfg-C (B = 8192, T = 16) lists for the two dominant launch families -- what a committed profile must
  // name to describe THIS binary with THESE knobs (bench.py checks)
  const std::string d = describe_plan(m, 8192, 16);
  auto field = [&](const char* key) {      // a whole key: the first one or one after a ';' (projection_window= does not match projection=)
    const std::string kk = std::string(";") + key + "=", dd = ";" + d;
    const size_t i = dd.find(kk);
    if (i == std::string::npos) return std::string("?");
    const size_t j = dd.find(';', i + 1);
    return dd.substr(i + kk.size(), j == std::string::npos ? std::string::npos : j - i - kk.size());
  };
  m->kinfo = "projection=" + field("projection") + ";gru_step=" + field("gru_step");
}

}  // namespace tepose
