// The HMR backbone (reference lib/models/spin.py:59-141: ResNet-50 up to the 7 x 7 average pool) as ONE table of its 53 convolutions, in state-dict
// order.  The blob layout, the pack order, the workspace carve and the forward all walk this table; nothing else lists a shape.
#pragma once
#include "common.h"

namespace tepose {

// Activation tensors of one pass (NHWC fp32, except the caller's NCHW image).  Every convolution output is stored BEFORE its ReLU; readers apply it.
//   T_J: the block input = the joined value relu(conv3 + identity) of the block before (or the max-pooled stem), already ReLU'd
//   T_A / T_B / T_C: outputs of a block's conv1 / conv2 / conv3 (the stem also writes T_C: it is dead once max-pooled);  T_D: the downsample branch
enum HmrTensor : unsigned char { T_IMG, T_J, T_A, T_B, T_C, T_D, kHmrTensors };
// conv1 of every block but the first reads relu(T_C + identity) instead of a stored tensor and writes that value to T_J once (conv.hip GatherArgs)
enum HmrJoin : unsigned char { J_NONE, J_IDENT /* identity = T_J */, J_DOWN /* identity = T_D */ };

struct ConvLayer { short cin, cout; unsigned char R, stride, pad, in, out, join; };
constexpr int kHmrConvs = 53;
constexpr int kHmrImage = 224;          // AvgPool2d(7) + view + fc1 fix the input size (spin.py:76,139-140)
constexpr int kHmrPass = 64;            // images per pass of tepose_hmr_features
constexpr double kBnEps = 1e-5;
struct ConvTable { ConvLayer l[kHmrConvs]; unsigned char final_join; };

constexpr ConvTable make_hmr_table() {
  ConvTable t{};
  int i = 0;
  t.l[i++] = ConvLayer{3, 64, 7, 2, 3, T_IMG, T_C, J_NONE};
  constexpr int blocks[4] = {3, 4, 6, 3};
  short inplanes = 64;
  unsigned char join = J_NONE;
  for (int s = 0; s < 4; ++s) {
    const short planes = (short)(64 << s);
    for (int b = 0; b < blocks[s]; ++b) {
      const unsigned char stride = (b == 0 && s > 0) ? 2 : 1;
      t.l[i++] = ConvLayer{inplanes, planes, 1, 1, 0, T_J, T_A, join};
      t.l[i++] = ConvLayer{planes, planes, 3, stride, 1, T_A, T_B, J_NONE};
      t.l[i++] = ConvLayer{planes, (short)(planes * 4), 1, 1, 0, T_B, T_C, J_NONE};
      join = J_IDENT;
      if (b == 0) {
        t.l[i++] = ConvLayer{inplanes, (short)(planes * 4), 1, stride, 0, T_J, T_D, J_NONE};
        join = J_DOWN;
      }
      inplanes = (short)(planes * 4);
    }
  }
  t.final_join = join;                  // what the average pool joins
  return t;
}
constexpr ConvTable kHmrTable = make_hmr_table();
static_assert(kHmrTable.l[kHmrConvs - 1].cout == kFeat && kHmrTable.l[kHmrConvs - 1].out == T_C, "53 convolutions ending in layer4.2.conv3");

inline int conv_out_size(int in, int R, int stride, int pad) { return (in + 2 * pad - R) / stride + 1; }

// One convolution as the walk sees it: geometry for `n` images and the product's shape  [rows x Kp] * [Np x Kp]^T
struct ConvStep {
  const ConvLayer* l; int idx;
  int Hin, Hout;                        // square maps
  long rows; int K, Kp, Np;
};
inline int conv_kp(int cin, int R) { return round_up(cin * R * R, 32); }
// f(step) for the 53 convolutions in order; hw[] tracks every tensor's spatial size (the max pool after the stem, the joins)
template <class F>
inline int hmr_walk(int n, F&& f) {
  int hw[kHmrTensors] = {kHmrImage, 0, 0, 0, 0, 0};
  for (int i = 0; i < kHmrConvs; ++i) {
    const ConvLayer& l = kHmrTable.l[i];
    if (l.join) hw[T_J] = hw[T_C];
    ConvStep st{&l, i, hw[l.in], conv_out_size(hw[l.in], l.R, l.stride, l.pad), 0, l.cin * l.R * l.R, conv_kp(l.cin, l.R), round_up(l.cout, 128)};
    st.rows = (long)n * st.Hout * st.Hout;
    hw[l.out] = st.Hout;
    const int rc = f(st);
    if (rc) return rc;
    if (i == 0) hw[T_J] = conv_out_size(hw[T_C], 3, 2, 1);      // maxpool3x3s2 of the stem
  }
  return 0;
}

// ---------------------------------------------------------------- conv.hip
// A operand of a convolution-as-product: row = output pixel (n, oh, ow), K order (r, s, c) with c fastest, columns [K, Kp) zero.
struct GatherArgs {
  const float* x;                       // [N,H,W,C] fp32 (nchw: [N,C,H,W])
  const float* res;                     // optional, same shape: the value gathered is x + res
  float* wb;                            // optional, same shape (1 x 1 stride 1 only; may alias x or res): the value after res / relu, written once
  int relu, nchw;
  int N, H, W, C, R, stride, pad, Ho, Wo, K, Kp;
  // split form: blocked hi / lo planes [Kp/32][rows][32] of row m * 2^e_m + row_scale[m] = 2^-e_m (as launch_split_rows); exact form: fp32 [rows][Kp]
  half_t *hi, *lo; float* row_scale;
  float* out;
};
hipError_t launch_conv_gather(const GatherArgs& a, bool split, hipStream_t s);
hipError_t launch_maxpool3x3s2(const float* x, int N, int H, int W, int C, float* y, int relu, hipStream_t s);
// y[n][c] = mean over the 49 pixels of (relu?)(x + res?)
hipError_t launch_avgpool7(const float* x, const float* res, int relu, int N, int C, float* y, hipStream_t s);
// OIHW weights (* gamma / sqrt(var + eps), in fp64) -> dst[Np][Kp] in (r, s, c) order, zero beyond (cout, K); bias_out = beta - mean * gamma / sqrt(var + eps).
// gamma == nullptr: no batch norm (bias_out = beta or 0).  *err |= 1 on var + eps <= 0 or a non-finite result.
hipError_t launch_hmr_fold_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int cout, int cin, int R,
                                float* dst, int Np, int Kp, float* bias_out, int* err, hipStream_t s);

}  // namespace tepose
