// Convolution entry points for gfx950: descriptor checks, the argument blocks of the gather-GEMM kernels, and the decision which kernel family
// (each in a unit of its own) takes a forward or a data gradient; of kernels only the two small passes behind routes decided here.
//
// Reference arithmetic: nn.ReflectionPad2d + nn.Conv2d (+bias) + LeakyReLU/ReLU/tanh and autograd's
// convolution_backward (models.py:80-84, 92-98, 161-166, 173-178; torchvision VGG conv3x3 + ReLU).
//
// Data layout: activations NHWC (channel contiguous), packed weights [rows][Kp] with the GEMM reduction
// index k = (kh, kw, c) contiguous -- both MFMA operands are "row-major with K contiguous", so a lane's
// fragment is one 16-byte LDS read.  The weight matrix is the MFMA A operand and the pixel tile the B
// operand: D[channel][pixel], so each lane ends up with 4 consecutive channels of one pixel and the
// NHWC store is a single 8/16-byte vector store per fragment.
#include "conv_stream.h"

namespace uegan {

int check_desc(const uegan_conv_desc* d) {
  UEGAN_CHECK_ARG(d != nullptr, "conv desc is null");
  UEGAN_CHECK_ARG(d->dtype == UEGAN_F32 || d->dtype == UEGAN_BF16, "bad dtype %d", d->dtype);
  UEGAN_CHECK_ARG(d->B > 0 && d->H > 0 && d->W > 0 && d->C1 > 0 && d->C2 >= 0 && d->Cout > 0, "bad conv dims");
  UEGAN_CHECK_ARG(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "bad conv kernel/stride/pad");
  UEGAN_CHECK_ARG(d->Ho == (d->H + 2 * d->pad - d->KH) / d->stride + 1 && d->Wo == (d->W + 2 * d->pad - d->KW) / d->stride + 1,
                  "Ho/Wo inconsistent with H,W,pad,K,stride");
  if (d->pad_mode == UEGAN_PAD_REFLECT)
    UEGAN_CHECK_ARG(d->pad < d->H && d->pad < d->W, "reflection pad %d must be smaller than the input (%d x %d)", d->pad, d->H, d->W);
  else
    UEGAN_CHECK_ARG(d->pad_mode == UEGAN_PAD_ZERO, "bad pad mode");
  const int epc = d->dtype == UEGAN_F32 ? 4 : 8;
  UEGAN_CHECK_ARG(d->C1 % epc == 0 && d->C2 % epc == 0 && d->Cout % epc == 0,
                  "tensor channel counts must be multiples of %d (one 16-byte chunk): pad them (C1=%d C2=%d Cout=%d)", epc, d->C1, d->C2, d->Cout);
  UEGAN_CHECK_ARG(d->Cin_w >= 0 && d->Cin_w <= d->C1 + d->C2 && d->Cout_w >= 0 && d->Cout_w <= d->Cout, "bad true weight dims");
  UEGAN_CHECK_ARG(d->stride <= 2, "stride > 2 is not built");
  UEGAN_CHECK_ARG(d->scale_group >= 0, "bad scale_group");
  UEGAN_CHECK_ARG(d->Cin_total == 0 || d->Cin_total >= (d->Cin_w ? d->Cin_w : d->C1 + d->C2), "Cin_total must cover the input channels used");
  return UEGAN_OK;
}

ConvGeom fwd_geom(const uegan_conv_desc* d) {
  ConvGeom g;
  g.B = d->B; g.IH = d->H; g.IW = d->W; g.C1 = d->C1; g.C2 = d->C2; g.C = d->C1 + d->C2;
  g.OH = d->Ho; g.OW = d->Wo; g.KH = d->KH; g.KW = d->KW; g.stride = d->stride; g.pad = d->pad; g.pad_mode = d->pad_mode;
  g.mode = 0;
  return g;
}

}  // namespace uegan

using namespace uegan;

static size_t esize(int dtype) { return dtype == UEGAN_F32 ? 4 : 2; }
// the result of an optional kernel (a *_run's 1 = not taken, nothing launched): *flag = value when it ran
static int report_taken(int rc, int* flag, int value) {
  if (rc == UEGAN_OK) *flag = value;
  return rc == 1 ? UEGAN_OK : rc;
}

// ---- argument blocks: one builder per direction
static void fwd_args(const uegan_conv_desc* d, ConvArgs& a, const void* x1, const void* x2, const void* w_ohwi, const float* bias, const float* scale, void* y) {
  a.g = fwd_geom(d);
  a.in1 = x1; a.in2 = d->C2 ? x2 : x1; a.w = w_ohwi; a.bias = bias; a.scale = scale; a.scale_group = d->scale_group; a.out = y; a.out2 = nullptr; a.n_out1 = 0;
  a.N = d->Cout; a.nbias = cout_w(d); a.Kp = (int)uegan_packed_k((int64_t)d->KH * d->KW * a.g.C); a.act = d->act;
  a.frame = 0; a.fy0 = a.fy1 = a.fx0 = a.fx1 = 0; a.mask = nullptr; a.mask_act = UEGAN_ACT_NONE;
}
// data gradient: rows = the conv's input pixels, source = dz on its output grid; out2 (C2 != 0): the virtual concat's second destination, one
// launch.  padded_grid: dz -> d(pad(x)) over the (H + 2 pad) x (W + 2 pad) grid, a pad-0 transposed conv without mirrored images
static void dgrad_args(const uegan_conv_desc* d, ConvArgs& a, const void* dz, const void* w_ihwo, const float* scale, void* out1, void* out2, bool padded_grid) {
  ConvGeom& g = a.g;
  const int grow = padded_grid ? 2 * d->pad : 0;
  g.B = d->B; g.IH = d->Ho; g.IW = d->Wo; g.C1 = d->Cout; g.C2 = 0; g.C = d->Cout;
  g.OH = d->H + grow; g.OW = d->W + grow; g.KH = d->KH; g.KW = d->KW; g.stride = d->stride;
  g.pad = padded_grid ? 0 : d->pad; g.pad_mode = padded_grid ? UEGAN_PAD_ZERO : d->pad_mode;
  g.mode = 1;
  a.in1 = dz; a.in2 = dz; a.bias = nullptr; a.nbias = 0; a.scale = scale; a.scale_group = d->scale_group; a.act = UEGAN_ACT_NONE;
  a.Kp = (int)uegan_packed_k((int64_t)d->KH * d->KW * d->Cout);
  a.w = w_ihwo; a.N = d->C1 + d->C2;
  a.out = out1; a.out2 = d->C2 ? out2 : nullptr; a.n_out1 = d->C1;
  a.frame = 0; a.fy0 = a.fy1 = a.fx0 = a.fx1 = 0; a.mask = nullptr; a.mask_act = UEGAN_ACT_NONE;
}
static size_t padded_grid_bytes(const uegan_conv_desc* d) {
  return (size_t)d->B * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * (d->C1 + d->C2) * esize(d->dtype);
}

// ---- routes: each "would kernel X take this problem" is answered by ONE function, for the dispatcher, the size queries and the fused entry points
// what takes a gather-GEMM problem ahead of the tile-per-block MFMA kernels (sp: the plan, for ROUTE_STREAM)
enum GatherRoute { ROUTE_DIRECT, ROUTE_TOEP, ROUTE_STREAM, ROUTE_MFMA };
static GatherRoute gather_route(const ConvArgs& a, int dtype, ConvStreamPlan& sp) {
  if (g_impl.impl == UEGAN_IMPL_DIRECT) return ROUTE_DIRECT;
  if (g_impl.glds && g_impl.stream && conv_toep_takes(a, dtype)) return ROUTE_TOEP;      // <= 4 output channels on 32 k input channels: Toeplitz kernel
  if (g_impl.glds && conv_stream_plan(a, dtype, sp)) return ROUTE_STREAM;                // thin full-resolution layers: persistent streaming kernel
  return ROUTE_MFMA;
}
// patch-resident kernel family: every 64-wide (bf16) K step fully populated; thin-channel layers (3-channel images, 1/3-channel heads,
// 32-channel full-resolution layers) pack several taps per K step in the generic kernel
static bool patch_family(const ConvGeom& g, int dtype) { return g_impl.patch && g_impl.glds && g.KH == g.KW && g.C % (CONV_ROWB / (int)esize(dtype)) == 0; }
// ... and its taps per axis (the KS of conv_patch_kernel); 0: a shape the family has no kernel for
static int patch_ks(const ConvGeom& g, int dtype) {
  if (!patch_family(g, dtype)) return 0;
  if (g.stride == 1) {
    // 1x1 convs (the attention modules' fuse conv, the decoder's upsample convs; pad 0): plain GEMMs -- the patch is the tile itself
    if (g.KH == 1 && g.pad == 0) return 1;
    if (g.KH == 3 || g.KH == 5 || g.KH == 7) return g.KH;
  } else if (g.stride == 2 && g.mode == 1) {     // stride-2 dgrad: per parity class a stride-1 problem with (K+1)/2 taps
    if (g.KH == 3 || g.KH == 5 || g.KH == 7) return (g.KH + 1) / 2;
  }
  return 0;
}
// the stride-1 3x3 layers: conv_tall / conv_wide / conv_interior are asked, in this order, before the patch kernel
static bool wide_first(const ConvGeom& g, int dtype) { return g.stride == 1 && patch_ks(g, dtype) == 3; }

static bool fwd_on_heads(const uegan_conv_desc* d) { return g_impl.impl != UEGAN_IMPL_DIRECT && g_impl.heads && heads_applicable(d); }
static bool dgrad_on_heads(const uegan_conv_desc* d) { return g_impl.impl != UEGAN_IMPL_DIRECT && g_impl.heads && heads_dgrad_applicable(d); }

static int patch_run(ConvArgs& a, int dtype, hipStream_t s, int ks) {
  if (dtype == UEGAN_F32) return ks <= 3 ? conv_patch_f32_a(a, s, ks) : conv_patch_f32_b(a, s, ks);
  return ks <= 3 ? conv_patch_bf16_a(a, s, ks) : conv_patch_bf16_b(a, s, ks);
}

static int dispatch_conv_gemm(ConvArgs& a, int dtype, hipStream_t s) {
  const ConvGeom& g = a.g;
  if (g_impl.patch && g_impl.glds && g.KH == g.KW && g.stride == 2 && g.mode == 0 && dtype != UEGAN_F32 && g.C == 32) {
    const int rc = conv_s2fwd_run(a, dtype, s);      // 32-channel stride-2 forwards (D.d2, G.enc2): pixel-pair rows
    if (rc != 1) return rc;
  }
  if (patch_family(g, dtype)) {
    if (wide_first(g, dtype)) {                      // wide layers on maps that fill 256 x 256 tiles
      int rc = conv_tall_run(a, dtype, s);
      if (rc != 1) return rc;
      rc = conv_wide_run(a, dtype, s);
      if (rc != 1) return rc;
      rc = conv_interior_run(a, dtype, s);      // (sets a.border_only: the patch launch below takes the frame with the mirrored images)
      if (rc != 1 && rc != UEGAN_OK) return rc;
    }
    const int ks = patch_ks(g, dtype);
    if (ks) return patch_run(a, dtype, s, ks);
    const int rc = conv_s2fwd_run(a, dtype, s);
    if (rc != 1) return rc;
  }
  return conv_gemm_run(a, dtype, s);      // (nothing else took it: the generic MFMA kernel, GLDS or register staged)
}

// *mask_applied (when asked for): whether the route taken multiplied by act'(a.mask) in its epilogue -- only the streaming kernel
// and the patch kernel's zero-padded 3x3 dgrads do, otherwise the caller runs act_bwd in place
static int run_gather_gemm(ConvArgs& a, int dtype, hipStream_t s, bool* mask_applied = nullptr) {
  if (mask_applied) *mask_applied = false;
  ConvStreamPlan sp;
  switch (gather_route(a, dtype, sp)) {
    case ROUTE_DIRECT: return conv_gemm_run(a, dtype, s);      // (under UEGAN_IMPL_DIRECT that is the scalar direct kernel)
    case ROUTE_TOEP: return conv_toep_run(a, dtype, s);
    case ROUTE_STREAM:
      if (mask_applied) *mask_applied = a.mask != nullptr;
      {
        ProfScope prof = conv_stream_prof(sp, a.g.mode, s);
        conv_stream_launch(sp, s);
        UEGAN_CHECK_LAUNCH();
      }
      return sp.fixup ? launch_dgrad_images(a, dtype, s, sp.a.xmir != 0) : UEGAN_OK;
    case ROUTE_MFMA: break;
  }
  // the masked epilogue exists for the patch kernel's zero-padded stride-1 3x3 data gradients (the VGG chain) and its 1x1 ones
  // (the generator's upsample / attention convs)
  const int ks = a.g.stride == 1 ? patch_ks(a.g, dtype) : 0;
  if (!(a.g.mode == 1 && ((ks == 3 && a.g.pad_mode != UEGAN_PAD_REFLECT) || ks == 1))) a.mask = nullptr;
  if (mask_applied) *mask_applied = a.mask != nullptr;
  return dispatch_conv_gemm(a, dtype, s);
}

extern "C" int uegan_conv2d_fwd(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias,
                                const float* scale, void* y, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(x1 && w_ohwi && y && (d->C2 == 0 || x2), "null pointer");
  ConvArgs a;
  fwd_args(d, a, x1, x2, w_ohwi, bias, scale, y);
  hipStream_t s = (hipStream_t)stream;
  if (fwd_on_heads(d)) {
    // (<= 4 output channels: the Toeplitz MFMA kernel where it applies -- 32 k input channels, bf16 -- or the streaming kernel, else the vector-ALU head kernel)
    ConvStreamPlan sp;
    if (d->act == UEGAN_ACT_SIGMOID || gather_route(a, d->dtype, sp) == ROUTE_MFMA) return heads_fwd(d, x1, w_ohwi, bias, scale, y, s);
  }
  // (the MFMA kernels' epilogues evaluate NONE / LRELU / RELU / TANH; the sigmoid exists for the prediction heads, above, and in the direct kernel)
  UEGAN_CHECK_ARG(d->act <= UEGAN_ACT_TANH || (d->act == UEGAN_ACT_SIGMOID && g_impl.impl == UEGAN_IMPL_DIRECT),
                  "activation %d is not available in this convolution's epilogue (sigmoid: prediction heads only; Swish / SELU: uegan_affine_act_fwd)", d->act);
  return run_gather_gemm(a, d->dtype, s);
}

// ----------------------------------------------------------------------------------------------------
// Split-K forward: see ConvArgs::kws.  The reduce pass adds the parts in order (deterministic) and applies scale, bias and activation.
// ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* ws, int parts, size_t part_stride, const float* bias, int nbias, const float* scale,
                                                            int scale_group, int act, bf16_t* out, size_t quads, int N, int hw) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const size_t e = q * 4;
  const int n = (int)(e % N);
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + e);
  for (int p = 1; p < parts; ++p) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(ws + (size_t)p * part_stride + e);
    v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
  }
  const int b = (int)((e / N) / hw);
  const float sc = scale ? scale[scale_group ? b / scale_group : 0] : 1.f;
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = apply_act(v[k] * sc + ((bias && n + k < nbias) ? bias[n + k] : 0.f), act);
  store4(out + e, r[0], r[1], r[2], r[3]);
}
int uegan::splitk_reduce_launch(const ConvArgs& a, hipStream_t s) {
  const size_t elems = (size_t)a.g.B * a.g.OH * a.g.OW * a.N, quads = elems / 4;      // (channel counts are multiples of 4)
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, a.kws, a.kparts, elems, a.bias, a.nbias, a.scale,
                     a.scale_group, a.act, static_cast<bf16_t*>(a.out), quads, a.N, a.g.OH * a.g.OW);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// upper bound of what a split-K forward of this layer would use (0: no kernel would split it -- call uegan_conv2d_fwd)
extern "C" size_t uegan_conv2d_fwd_splitk_workspace_bytes(const uegan_conv_desc* d) {
  if (check_desc(d) || d->dtype == UEGAN_F32 || !g_impl.patch || !g_impl.glds) return 0;
  const ConvGeom g = fwd_geom(d);
  if (g.KH != g.KW || g.C % 64 || g.C < 128 || d->Cout < 64) return 0;
  int blocks;
  if (g.stride == 1 && g.KH == 3 && g.pad == 1 && d->Cout > 64 && g.OH >= 16) blocks = g.B * ((g.OH + 15) / 16) * ((g.OW + CONV_TW - 1) / CONV_TW) * ((d->Cout + 63) / 64);
  else if (g.stride == 2 && (g.KH == 3 || g.KH == 5 || g.KH == 7) && g.C2 == 0 && g.OH >= 8 && g.OW >= 16) blocks = g.B * ((g.OH + 7) / 8) * ((g.OW + CONV_TW - 1) / CONV_TW) * ((d->Cout + 63) / 64);
  else return 0;
  int parts = 1;
  while (parts * 2 <= g.C / 64 && blocks * parts * 2 <= 256) parts *= 2;
  return parts < 2 ? 0 : (size_t)parts * g.B * g.OH * g.OW * d->Cout * sizeof(float);
}

// uegan_conv2d_fwd with a workspace the kernels may use for a split-K launch (see include/uegan_hip.h)
extern "C" int uegan_conv2d_fwd_splitk(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias, const float* scale,
                                       void* y, void* workspace, size_t workspace_bytes, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!workspace || !workspace_bytes || d->dtype == UEGAN_F32 || g_impl.impl == UEGAN_IMPL_DIRECT || fwd_on_heads(d))
    return uegan_conv2d_fwd(d, x1, x2, w_ohwi, bias, scale, y, stream);
  UEGAN_CHECK_ARG(x1 && w_ohwi && y && (d->C2 == 0 || x2), "null pointer");
  UEGAN_CHECK_ARG(d->act <= UEGAN_ACT_TANH, "activation %d is not available in this convolution's epilogue", d->act);
  ConvArgs a;
  fwd_args(d, a, x1, x2, w_ohwi, bias, scale, y);
  a.kws = static_cast<float*>(workspace); a.kws_bytes = workspace_bytes;
  return run_gather_gemm(a, UEGAN_BF16, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------------------------
// Forward + the per-(image, channel) moments of its result (InstanceNorm behind a conv: the generator's attention modules, models.py:227,
// 230-237): where the streaming kernel takes the layer the sums ride along with the forward (conv_stream.hip) -- the moments pass over the
// tensor is gone.
// *produced = 0: no such kernel for this layer, y is computed as by uegan_conv2d_fwd and mean / rstd are untouched (the caller runs uegan_moments).
// ----------------------------------------------------------------------------------------------------
static bool fwd_stats_plan(const uegan_conv_desc* d, ConvArgs& a, ConvStreamPlan& sp) {
  if (d->dtype != UEGAN_BF16 || g_impl.impl == UEGAN_IMPL_DIRECT || !g_impl.glds || g_tuning[UEGAN_TUNE_FWD_STATS] == 0) return false;
  if (d->act > UEGAN_ACT_TANH) return false;
  // (64 output channels on 16-row tiles sit at the 256-register limit without the 32 sum registers: 8-row tiles there -- VGG conv1_1 609 -> 462 us; 420 without the sums)
  if (!conv_stream_plan(a, d->dtype, sp, a.N > 32 ? 2 : 4) || !conv_stream_stats_ok(sp)) return false;
  return true;
}
extern "C" size_t uegan_conv2d_fwd_stats_workspace_bytes(const uegan_conv_desc* d) {
  if (check_desc(d)) return 0;
  ConvArgs a;
  ConvStreamPlan sp;
  fwd_args(d, a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return fwd_stats_plan(d, a, sp) ? conv_stream_stats_bytes(sp) : 0;
}
extern "C" int uegan_conv2d_fwd_stats(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias, const float* scale,
                                      void* y, float* mean, float* rstd, float eps, void* workspace, size_t workspace_bytes, int* produced,
                                      uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(x1 && w_ohwi && y && produced && (d->C2 == 0 || x2), "null pointer");
  *produced = 0;
  ConvArgs a;
  ConvStreamPlan sp;
  fwd_args(d, a, x1, x2, w_ohwi, bias, scale, y);
  if (!fwd_stats_plan(d, a, sp)) return uegan_conv2d_fwd(d, x1, x2, w_ohwi, bias, scale, y, stream);
  UEGAN_CHECK_ARG(mean && rstd && workspace && workspace_bytes >= uegan_conv2d_fwd_stats_workspace_bytes(d), "conv2d_fwd_stats: mean / rstd / workspace");
  hipStream_t s = (hipStream_t)stream;
  conv_stream_stats_arm(sp, workspace);
  {
    ProfScope prof = conv_stream_prof(sp, a.g.mode, s);
    conv_stream_launch(sp, s);
    UEGAN_CHECK_LAUNCH();
  }
  rc = conv_stream_stats_finalize(sp, mean, rstd, eps, s);
  if (rc == UEGAN_OK) *produced = 1;
  return rc;
}

// ----------------------------------------------------------------------------------------------------
// Forward with extras (round 6): hi + lo pairs, the product epilogue, the generator's final residual + clamp, the moments (include/uegan_hip.h).
// ----------------------------------------------------------------------------------------------------
static bool ex_plan(const uegan_conv_desc* d, const uegan_conv_ex* ex, ConvArgs& a, ConvStreamPlan& sp, bool* toep) {
  *toep = false;
  if (d->dtype != UEGAN_BF16 || g_impl.impl == UEGAN_IMPL_DIRECT || !g_impl.glds || !g_impl.stream || d->act > UEGAN_ACT_TANH) return false;
  a.in1_lo = ex->x1_lo; a.in2_lo = d->C2 ? ex->x2_lo : nullptr; a.w_lo = ex->w_lo; a.out_lo = ex->y_lo;
  a.mul = ex->mul; a.mul_lo = ex->mul_lo; a.out_mul = ex->y_mul; a.out_mul_lo = ex->y_mul_lo;
  a.res_x = ex->res_x; a.res_x2 = ex->res_x2; a.res_out = ex->res_out; a.res_out2 = ex->res_out2; a.res_split = ex->res_split > 0 ? ex->res_split : (1 << 30);
  if (ex->w_interleaved) {               // a stride-2 forward against a [hi | lo] weight matrix: the source's channels read twice (ConvArgs::src_wrap)
    if (d->stride != 2 || d->C2 || (d->C1 != 32 && d->C1 != 64) || a.in1_lo || a.w_lo || a.out_lo || a.mul || a.res_out) return false;
    a.g.C = 2 * d->C1;
    a.src_wrap = d->C1 - 1;
    a.Kp = (int)uegan_packed_k((int64_t)d->KH * d->KW * a.g.C);
    *toep = false;
    return true;
  }
  if (a.res_out || cout_w(d) <= 4) {      // dec5.1: the Toeplitz kernel
    *toep = conv_toep_takes(a, d->dtype) && !(a.res_out && a.res_split < d->B && !(a.res_x2 && a.res_out2));
    return *toep;
  }
  return conv_stream_plan(a, d->dtype, sp);
}
extern "C" size_t uegan_conv2d_fwd_ex_workspace_bytes(const uegan_conv_desc* d, const uegan_conv_ex* ex) {
  if (check_desc(d) || !ex) return 0;
  ConvArgs a;
  ConvStreamPlan sp;
  bool toep;
  fwd_args(d, a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (!ex_plan(d, ex, a, sp, &toep) || toep || a.src_wrap || g_tuning[UEGAN_TUNE_FWD_STATS] == 0 || !conv_stream_stats_ok(sp)) return 0;
  sp.stats = true;
  return conv_stream_ex_available(sp) ? conv_stream_stats_bytes(sp) : 0;
}
extern "C" int uegan_conv2d_fwd_ex(const uegan_conv_desc* d, const uegan_conv_ex* ex, const void* x1, const void* x2, const void* w_ohwi, const float* bias,
                                   const float* scale, void* y, int* taken, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(ex && taken && x1 && w_ohwi && y && (d->C2 == 0 || x2), "null pointer");
  *taken = 0;
  ConvArgs a;
  ConvStreamPlan sp;
  bool toep;
  fwd_args(d, a, x1, x2, w_ohwi, bias, scale, y);
  if (!ex_plan(d, ex, a, sp, &toep)) return UEGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  if (toep) return report_taken(conv_toep_run(a, d->dtype, s), taken, 1);
  if (a.src_wrap) return report_taken(conv_s2fwd_run(a, d->dtype, s), taken, 1);
  const size_t wsb = ex->mean ? uegan_conv2d_fwd_ex_workspace_bytes(d, ex) : 0;
  const bool stats = wsb != 0 && ex->rstd && ex->stats_workspace && ex->stats_workspace_bytes >= wsb;
  if (stats) conv_stream_stats_arm(sp, ex->stats_workspace);
  {
    ProfScope prof = conv_stream_prof(sp, 8 + sp.pr, s);
    if (!conv_stream_launch_ex(sp, s)) return UEGAN_OK;
    UEGAN_CHECK_LAUNCH();
  }
  *taken = 1;
  if (stats) {
    rc = conv_stream_stats_finalize(sp, ex->mean, ex->rstd, ex->eps, s);
    if (rc) return rc;
    *taken |= 2;
  }
  return UEGAN_OK;
}

// forward + 2x2 max-pool of the result (the VGG chain, losses.py:74-104: conv, ReLU, MaxPool2d(2)): y as uegan_conv2d_fwd, y_pool =
// maxpool2x2(y) written by the convolution's epilogue where the kernel that takes the layer can, else by the pooling kernel
extern "C" int uegan_conv2d_fwd_pool(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias,
                                     const float* scale, void* y, void* y_pool, uegan_stream_t stream) {
  return uegan_conv2d_fwd_pool_part(d, x1, x2, w_ohwi, bias, scale, y, y_pool, d ? d->B : 0, stream);
}

// ... where only the first n_full images need y itself: y[n_full:] is UNDEFINED afterwards (a kernel with a pooling epilogue does not store
// those rows -- the store-bound half of its epilogue; the fallback writes them).  The fidelity loss's reference images (losses.py:29-30: no
// gradient reaches them) and every no-grad VGG pass: the outputs of conv1_2 / conv2_2 / conv3_4 / conv4_4 feed nothing but their pool.
extern "C" int uegan_conv2d_fwd_pool_part(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias,
                                          const float* scale, void* y, void* y_pool, int n_full, uegan_stream_t stream) {
  return uegan_conv2d_fwd_pool_idx(d, x1, x2, w_ohwi, bias, scale, y, y_pool, nullptr, n_full, 0, stream);
}

// ... and with the window position of each maximum (one byte per pooled element, first maximum in (row, column) order as ATen's
// max_pool2d_with_indices picks it) for the first n_idx images: uegan_maxpool2x2_bwd_idx routes the gradient with them and the pooled
// tensor alone, so an image that needs a gradient does not need its full-resolution y either (n_full = 0, n_idx = B: the fidelity loss's
// enhanced batch -- y is then neither written by the forward nor read by the backward).  idx[n_idx:] is undefined afterwards.
extern "C" int uegan_conv2d_fwd_pool_idx(const uegan_conv_desc* d, const void* x1, const void* x2, const void* w_ohwi, const float* bias,
                                         const float* scale, void* y, void* y_pool, void* idx, int n_full, int n_idx, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(n_full >= 0 && n_full <= d->B && n_idx >= 0 && n_idx <= d->B && (idx || n_idx == 0), "conv2d_fwd_pool: n_full / n_idx outside [0, B], or positions wanted without a buffer");
  UEGAN_CHECK_ARG(x1 && w_ohwi && y && y_pool && (d->C2 == 0 || x2), "null pointer");
  UEGAN_CHECK_ARG(d->Ho % 2 == 0 && d->Wo % 2 == 0, "conv2d_fwd_pool needs an even output map");
  UEGAN_CHECK_ARG(d->act <= UEGAN_ACT_TANH, "activation %d is not available in this convolution's epilogue", d->act);
  ConvArgs a;
  fwd_args(d, a, x1, x2, w_ohwi, bias, scale, y);
  a.pool_out = y_pool;
  a.n_full = n_full;
  a.pool_idx = n_idx > 0 ? idx : nullptr;
  a.n_idx = n_idx;
  rc = run_gather_gemm(a, d->dtype, (hipStream_t)stream);
  if (rc || a.pool_done) return rc;
  // (no kernel with a pooling epilogue took the layer: y is complete -- the plain kernels ignore n_full -- and is pooled here)
  if (a.pool_idx) return uegan_maxpool2x2_fwd_idx(d->dtype, y, y_pool, idx, d->B, d->Ho, d->Wo, d->Cout, stream);
  return uegan_maxpool2x2_fwd(d->dtype, y, y_pool, d->B, d->Ho, d->Wo, d->Cout, stream);
}

extern "C" int uegan_conv2d_dgrad(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx1,
                                  void* dx2, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(dz && w_ihwo && dx1 && (d->C2 == 0 || dx2), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (dgrad_on_heads(d)) return heads_dgrad(d, dz, w_ihwo, scale, dx1, s);
  ConvArgs a;
  dgrad_args(d, a, dz, w_ihwo, scale, dx1, dx2, false);
  return run_gather_gemm(a, d->dtype, s);
}

// ----------------------------------------------------------------------------------------------------
// Reflection-padded dgrad on small maps: "pad-grid dgrad + fold".  On a map of a few tiles every tile touches the border,
// so the mirrored-image passes of the MODE 2 kernels (a full MFMA pass per left / right image) cost 2-3x the direct
// work.  Instead the dgrad runs image-free over the PADDED grid (a zero-pad, pad = 0 problem of (H+2p) x (W+2p) pixels)
// into a workspace and fold_reflect_kernel adds each pixel's up to 3 x 3 mirror sources (the adjoint of
// nn.ReflectionPad2d, models.py:80) while copying the interior out.  The workspace is ~(1 + 2p/H)^2 x the size of dx,
// which is why large maps keep the interior / frame split.
// ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) fold_reflect_kernel(const T* __restrict__ ws, T* __restrict__ dx1, T* __restrict__ dx2,
                                                           int B, int H, int W, int p, int Ct, int C1) {
  constexpr int E = 16 / (int)sizeof(T);
  const int cch = Ct / E;
  const size_t total = (size_t)B * H * W * cch;
  const int Hp = H + 2 * p, Wp = W + 2 * p;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cc = (int)(i % cch);
    size_t r = i / cch;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int b = (int)(r / H);
    int ys[3], xs[3], ny = 1, nx = 1;
    ys[0] = y + p; xs[0] = x + p;
    if (y >= 1 && y <= p) ys[ny++] = p - y;                                  // mirrored across row 0
    if (y <= H - 2 && y >= H - 1 - p) ys[ny++] = p + 2 * (H - 1) - y;        // mirrored across row H-1
    if (x >= 1 && x <= p) xs[nx++] = p - x;
    if (x <= W - 2 && x >= W - 1 - p) xs[nx++] = p + 2 * (W - 1) - x;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int iy = 0; iy < ny; ++iy)
      for (int ix = 0; ix < nx; ++ix) {
        float v[E];
        Vec<T, E>::ld(ws + (((size_t)b * Hp + ys[iy]) * Wp + xs[ix]) * Ct + cc * E, v);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += v[e];
      }
    const int c = cc * E;
    const size_t pix = ((size_t)b * H + y) * W + x;
    T* o = (dx2 && c >= C1) ? dx2 + pix * (Ct - C1) + (c - C1) : dx1 + pix * (dx2 ? C1 : Ct) + c;
    Vec<T, E>::st(o, acc);
  }
}

// Which reflection-padded dgrads take the pad-grid + fold route.  Measured on the model's layers (bf16, batch 16; direct -> fold):
// 5x5s2 256->512 @32^2 0.313 -> 0.141 ms, 7x7s2 64->128 @128^2 0.270 -> 0.168, the 5x5 / 7x7 prediction heads @<=128^2
// 1.3-2.1x faster; every 3x3 (pad 1: one mirrored row, cheap images) equal or slower, maps >= 256^2 slower (workspace
// traffic), and 5x5s2 128->256 @64^2 slower (0.105 -> 0.133: its 32^2 parity-class grids are exactly 2 x 2 tiles, the
// padded 34^2 ones 3 x 3).  uegan_set_tuning(UEGAN_TUNE_FOLD_MAX, n) (full-resolution pixels; the tests flip it) overrides the map
// limit, n = 0 disables the route, -1 (default) is this rule.
static bool dgrad_folds(const uegan_conv_desc* d) {
  if (d->pad_mode != UEGAN_PAD_REFLECT || d->pad == 0 || g_impl.impl == UEGAN_IMPL_DIRECT) return false;
  if (dgrad_on_heads(d)) return false;                             // (the one-channel heads: uegan_conv2d_dgrad's VALU kernel, no workspace)
  if (g_impl.glds && conv_flat_applicable(d)) return true;         // stride-2 layers: conv_flat_kernel computes the padded grid in one launch
  if (g_tuning[UEGAN_TUNE_FOLD_MAX] >= 0) return (long)d->H * d->W <= (long)g_tuning[UEGAN_TUNE_FOLD_MAX];
  if (d->pad < 2 || (long)d->H * d->W > 128L * 128L) return false;
  if (d->Cout <= 8) return true;      // prediction heads (gather-GEMM dgrad, no tile quantisation): always faster folded
  auto tiles = [&](int h, int w) { return (((h + d->stride - 1) / d->stride + 15) / 16) * (((w + d->stride - 1) / d->stride + 15) / 16); };
  const int direct = tiles(d->H, d->W), padded = tiles(d->H + 2 * d->pad, d->W + 2 * d->pad);
  return direct == 1 || padded <= 2 * direct;
}

extern "C" size_t uegan_conv2d_dgrad_workspace_bytes(const uegan_conv_desc* d) { return check_desc(d) || !dgrad_folds(d) ? 0 : padded_grid_bytes(d); }

extern "C" int uegan_conv2d_dgrad_ws(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx1,
                                     void* dx2, void* workspace, size_t workspace_bytes, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!dgrad_folds(d)) return uegan_conv2d_dgrad(d, dz, w_ihwo, scale, dx1, dx2, stream);
  UEGAN_CHECK_ARG(dz && w_ihwo && dx1 && (d->C2 == 0 || dx2), "null pointer");
  UEGAN_CHECK_ARG(workspace && workspace_bytes >= uegan_conv2d_dgrad_workspace_bytes(d), "dgrad workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ConvArgs a;
  dgrad_args(d, a, dz, w_ihwo, scale, workspace, nullptr, true);      // (one destination: the fold writes the two)
  rc = g_impl.glds ? conv_flat_run(d, dz, w_ihwo, scale, workspace, s) : 1;
  if (rc == 1) rc = run_gather_gemm(a, d->dtype, s);
  if (rc) return rc;
  const int Ct = d->C1 + d->C2;
  const size_t total = (size_t)d->B * d->H * d->W * (Ct * esize(d->dtype) / 16);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (d->dtype == UEGAN_F32)
    hipLaunchKernelGGL((fold_reflect_kernel<float>), dim3(blocks), dim3(256), 0, s, (const float*)workspace, (float*)dx1, d->C2 ? (float*)dx2 : nullptr, d->B, d->H, d->W, d->pad, Ct, d->C1);
  else
    hipLaunchKernelGGL((fold_reflect_kernel<bf16_t>), dim3(blocks), dim3(256), 0, s, (const bf16_t*)workspace, (bf16_t*)dx1, d->C2 ? (bf16_t*)dx2 : nullptr, d->B, d->H, d->W, d->pad, Ct, d->C1);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// The data gradient with respect to the PADDED input, for a caller whose next kernel can add the mirror images itself (uegan_sn_act_bwd_p,
// uegan_act_bwd_p): workspace = [B][H + 2 pad][W + 2 pad][C1], *pad_out = pad.  Only where a kernel computes the padded grid in one launch --
// stride-2 layers on conv_flat_kernel (w_ihwo), the one-channel prediction heads on head_dgrad_mfma_kernel (w_ohwi: the FORWARD pack) --
// else *pad_out = -1, nothing is launched and the caller takes uegan_conv2d_dgrad_ws.
// who computes that padded grid: decided once, for the launcher and for its size query
enum PaddedRoute { PADDED_NONE, PADDED_HEADS, PADDED_FLAT };
static PaddedRoute padded_route(const uegan_conv_desc* d, bool can_heads, bool can_flat) {
  if (d->C2 || d->pad_mode != UEGAN_PAD_REFLECT || d->pad == 0 || g_impl.impl == UEGAN_IMPL_DIRECT || !g_impl.glds) return PADDED_NONE;
  if (can_heads && g_impl.heads && heads_dgrad_mfma_applicable(d)) return PADDED_HEADS;
  if (can_flat && conv_flat_applicable(d)) return PADDED_FLAT;
  return PADDED_NONE;
}
extern "C" int uegan_conv2d_dgrad_padded(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const void* w_ohwi, const float* scale,
                                         void* workspace, size_t workspace_bytes, int* pad_out, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(dz && pad_out, "null pointer");
  *pad_out = -1;
  const PaddedRoute route = padded_route(d, w_ohwi && !scale, w_ihwo != nullptr);
  if (route == PADDED_NONE) return UEGAN_OK;
  UEGAN_CHECK_ARG(workspace && workspace_bytes >= padded_grid_bytes(d), "dgrad_padded: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (route == PADDED_FLAT) return report_taken(conv_flat_run(d, dz, w_ihwo, scale, workspace, s), pad_out, d->pad);
  rc = heads_dgrad_mfma(d, dz, w_ohwi, workspace, s);      // (not a *_run: it takes every layer heads_dgrad_mfma_applicable names)
  if (rc == UEGAN_OK) *pad_out = d->pad;
  return rc;
}
// (0 where uegan_conv2d_dgrad_padded would decline the layer whatever packs it is handed: the caller then does not allocate the padded grid at all)
extern "C" size_t uegan_conv2d_dgrad_padded_bytes(const uegan_conv_desc* d) {
  return check_desc(d) || padded_route(d, true, true) == PADDED_NONE ? 0 : padded_grid_bytes(d);
}

// dx = dgrad(dz) * act'(x_act): the data gradient with the activation gradient of the layer that PRODUCED the conv input folded
// into the epilogue (act' is a function of the activated output, which is this conv's saved input).  The producer then skips its
// own act_bwd pass -- valid when every consumer of that tensor applies the factor (uegan_amd/losses.py VGG19_relu).
extern "C" int uegan_conv2d_dgrad_act(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx1,
                                      void* workspace, size_t workspace_bytes, int in_act, const void* x_act, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(d->C2 == 0, "dgrad_act takes one destination");
  if (in_act == UEGAN_ACT_NONE) return uegan_conv2d_dgrad_ws(d, dz, w_ihwo, scale, dx1, nullptr, workspace, workspace_bytes, stream);
  UEGAN_CHECK_ARG(dz && w_ihwo && dx1 && x_act, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  bool applied = false;
  if (dgrad_folds(d)) {
    rc = uegan_conv2d_dgrad_ws(d, dz, w_ihwo, scale, dx1, nullptr, workspace, workspace_bytes, stream);
  } else {
    ConvArgs a;
    dgrad_args(d, a, dz, w_ihwo, scale, dx1, nullptr, false);
    a.mask = x_act; a.mask_act = in_act;
    rc = run_gather_gemm(a, d->dtype, s, &applied);
  }
  if (rc || applied) return rc;
  return uegan_act_bwd(d->dtype, in_act, dx1, x_act, dx1, (int64_t)d->B * d->H * d->W * d->C1, stream);
}

// ---- the fidelity loss's backward: a data gradient with the next elementwise pass in conv_tall_kernel's epilogue (ConvArgs::epi)
// Only where the unfused route (uegan_conv2d_dgrad_act -> run_gather_gemm -> dispatch_conv_gemm) hands the SAME problem to conv_tall_kernel: the
// accumulation is then the same and the fused result is bit-identical to the two passes.  Asked of the very predicates those functions branch on.
static bool dgrad_takes_tall(const uegan_conv_desc* d, const ConvArgs& a) {
  if (d->dtype != UEGAN_BF16 || d->C2 || g_tuning[UEGAN_TUNE_VGG_EPI] == 0 || a.g.pad_mode == UEGAN_PAD_REFLECT) return false;      // (what the epilogues exist for)
  if (dgrad_folds(d) || dgrad_on_heads(d)) return false;
  ConvStreamPlan sp;
  return gather_route(a, d->dtype, sp) == ROUTE_MFMA && wide_first(a.g, d->dtype);
}

extern "C" int uegan_conv2d_dgrad_act_tap(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx1, int in_act,
                                          const void* x_act, const void* y, float weight, const float* gscale, const float* tmp, int* applied,
                                          uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(dz && w_ihwo && dx1 && x_act && y && tmp && applied, "null pointer");
  *applied = 0;
  ConvArgs a;
  dgrad_args(d, a, dz, w_ihwo, scale, dx1, nullptr, false);
  a.mask = x_act; a.mask_act = in_act;              // (the unfused route: uegan_conv2d_dgrad_act's masked data gradient)
  if (in_act != UEGAN_ACT_RELU || !dgrad_takes_tall(d, a)) return UEGAN_OK;
  a.epi = 1;
  a.epi_y = y; a.epi_weight = weight; a.epi_gscale = gscale;
  percep_tap_consts(d->dtype, tmp, d->B, d->H * d->W, d->C1, &a.epi_st, &a.epi_tot);
  return report_taken(conv_tall_run(a, d->dtype, (hipStream_t)stream), applied, 1);
}

extern "C" int uegan_conv2d_dgrad_unpool(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx_full, int in_act,
                                         const void* y_pool, const void* idx, int* applied, uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(dz && w_ihwo && dx_full && y_pool && idx && applied, "null pointer");
  *applied = 0;
  ConvArgs a;
  dgrad_args(d, a, dz, w_ihwo, scale, dx_full, nullptr, false);      // (the unfused route: uegan_conv2d_dgrad, no mask)
  if (in_act != UEGAN_ACT_RELU || !dgrad_takes_tall(d, a)) return UEGAN_OK;
  a.mask = y_pool; a.mask_act = in_act;
  a.epi = 2;
  a.epi_idx = static_cast<const unsigned char*>(idx);
  return report_taken(conv_tall_run(a, d->dtype, (hipStream_t)stream), applied, 1);
}

// Every build compiles each csrc/*.hip on its own (tests/emu/build_emu.sh says so with -DUEGAN_EMU_UNITS).  Only an emulator build script from
// before the split of this file, with its fixed unit list, gets the units split out of it as part of this one, as they were then.
#if defined(UEGAN_EMU) && !defined(UEGAN_EMU_UNITS)
#include "conv_gemm.hip"
#include "conv_stream.hip"
#include "wgrad.hip"
#include "act_bwd.hip"
#include "pack_weights.hip"
#include "runtime.hip"
#endif
