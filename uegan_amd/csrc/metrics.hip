// Image-level helpers around the generator: the history pool's gather/scatter (utils.py:23-50) and the evaluation metrics of
// the inference configuration -- 8-bit quantisation (torchvision save_image as called at tester.py:70-71), PSNR
// (metrics/CalcPSNR.py:85-92 with the 4-pixel border crop of :24,56) and SSIM with skimage's defaults as called at
// metrics/CalcSSIM.py:63 (7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, data_range 255, mean over the three
// channels) -- all on the device, so validation never copies images to the host.
#include "common.h"
#include "nima.h"      // the NIMA scorer's kernels (MobileNetV2 trunk + head), entry points at the end of this file

namespace uegan {

// ---- copy whole images between two stacks by index table (the tables travel by value: no host-to-device copy) ----
constexpr int COPY_MAX_IMAGES = 64;
struct CopyTable {
  int dst[COPY_MAX_IMAGES];
  int src[COPY_MAX_IMAGES];      // >= 0: image of stack A, < 0: image ~src of stack B
};

template <int V>
__global__ void copy_images_kernel(float* dst, const float* src_a, const float* src_b, CopyTable t, size_t elems) {
  const int img = blockIdx.y;
  const int si = t.src[img];
  const float* s = si >= 0 ? src_a + (size_t)si * elems : src_b + (size_t)(~si) * elems;
  float* d = dst + (size_t)t.dst[img] * elems;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i < elems; i += (size_t)gridDim.x * blockDim.x * V) {
    if (V == 4) *reinterpret_cast<f32x4*>(d + i) = *reinterpret_cast<const f32x4*>(s + i);
    else d[i] = s[i];
  }
}

// ---- [-1,1] NCHW fp32 -> uint8 NHWC: denorm (utils.py:128-130) then save_image's mul(255).add(0.5).clamp(0,255).to(uint8) ----
__global__ void quantize_u8_kernel(const float* x, uint8_t* y, int B, int C, int HW) {
  const size_t total = (size_t)B * HW * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int b = (int)(p / HW);
    const size_t hw = p - (size_t)b * HW;
    float v = (x[((size_t)b * C + c) * HW + hw] + 1.f) / 2.f;
    v = fminf(fmaxf(v, 0.f), 1.f);
    v = v * 255.f + 0.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    y[i] = (uint8_t)v;                       // truncation, like Tensor.to(torch.uint8)
  }
}

// ---- up to four [-1,1] NCHW fp32 images side by side -> ONE uint8 NHWC image [B][H][n*W][C], panel k in columns [k*W, (k+1)*W): what
// save_image(torch.cat([denorm(a), denorm(b), ...], 3)) writes (trainer.py:182-183,244-245, tester.py:73-74), with quantize_u8_kernel's
// arithmetic.  The source pointers travel by value, like CopyTable.  HBM-bound: 4 B read + 1 B written per element, each exactly once.
// The sources are [B][C][Hs][Ws] planes of which the H x W window at (sy, sx) is taken; panel k goes to rows [dy, dy + H) and columns
// [dx + k*Wp, dx + k*Wp + W) of a [B][Hd][Wd][C] image of which nothing else is written (MontageGeom).  uegan_montage_place_u8 sets all of it (tiled
// inference writes each tile's core into the full-size result); uegan_montage_crop_u8: window and destination at the origin, Hd = H, Wd = n*W, Wp = W;
// uegan_montage_u8: also Hs = H, Ws = W. ----
constexpr int MONTAGE_MAX_SRCS = 4;
constexpr int MONTAGE_THREADS = 256;
constexpr int MONTAGE_MAX_BLOCKS = 1024;      // grid cap: 4 blocks (16 waves) per CU on 256 CUs, the rest by grid stride
constexpr int MONTAGE_VEC = 4;                // pixels per thread of the vector path (uegan_amd/tester.py mirrors these three numbers)
struct MontageSrcs {
  const float* p[MONTAGE_MAX_SRCS];
};
struct MontageGeom {
  int Hs, Ws, sy, sx;      // source planes, window origin
  int H, W;                // window
  int Hd, Wd, dy, dx, Wp;  // destination image, origin of panel 0, panel pitch in columns
};

__device__ __forceinline__ uint32_t quantize_u8(float x) {
  float v = (x + 1.f) / 2.f;
  v = fminf(fmaxf(v, 0.f), 1.f);
  v = v * 255.f + 0.5f;
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (uint32_t)(uint8_t)v;                 // truncation, like Tensor.to(torch.uint8)
}

// vector path (W, Ws, sx, and for C = 3 also Wd, dx, Wp multiples of 4; sources 16-byte and y 4-byte aligned): one thread = 4 neighbouring pixels of one panel row: one 16-byte load per
// plane (a wave reads 1 KiB of a plane row in one instruction), C whole dwords stored (4 * C bytes: the 4 pixels' bytes are contiguous in NHWC)
template <int C>
__global__ void montage_u8_vec_kernel(MontageSrcs s, int n, uint8_t* y, size_t rows, MontageGeom g) {
  const int Hs = g.Hs, Ws = g.Ws, H = g.H, W = g.W;
  const int wq = W / MONTAGE_VEC;
  const size_t items = rows * n * wq;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % wq);
    const size_t t = i / wq;
    const int k = (int)(t % n);
    const size_t row = t / n;                  // b * H + h
    const size_t b = row / H, h = row - b * H;
    const float* src = s.p[k] + ((b * C) * Hs + g.sy + h) * Ws + g.sx + (size_t)q * MONTAGE_VEC;
    uint32_t by[MONTAGE_VEC * C];              // byte j of the 4 * C output bytes = pixel j / C, channel j % C
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * Hs * Ws);
      by[0 * C + c] = quantize_u8(v[0]);
      by[1 * C + c] = quantize_u8(v[1]);
      by[2 * C + c] = quantize_u8(v[2]);
      by[3 * C + c] = quantize_u8(v[3]);
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(y + (((b * g.Hd + g.dy + h) * g.Wd) + g.dx + (size_t)k * g.Wp + (size_t)q * MONTAGE_VEC) * C);
#pragma unroll
    for (int d = 0; d < C; ++d) dst[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
  }
}

// scalar path (any width, any alignment, any C): one thread = one output pixel
__global__ void montage_u8_kernel(MontageSrcs s, int n, uint8_t* y, size_t rows, int C, MontageGeom g) {
  const int Hs = g.Hs, Ws = g.Ws, H = g.H, W = g.W;
  const size_t items = rows * n * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    const size_t t = i / W;
    const int k = (int)(t % n);
    const size_t row = t / n;
    const size_t b = row / H, h = row - b * H;
    const float* src = s.p[k] + ((b * C) * Hs + g.sy + h) * Ws + g.sx + w;
    uint8_t* dst = y + (((b * g.Hd + g.dy + h) * g.Wd) + g.dx + (size_t)k * g.Wp + w) * C;
    for (int c = 0; c < C; ++c) dst[c] = (uint8_t)quantize_u8(src[(size_t)c * Hs * Ws]);
  }
}

// ---- sum of squared differences over the cropped region, per image (double accumulation; the terms are integers and the sums stay
// below 2^53, so the double atomicAdd per block is exact and the result does not depend on the order of the blocks) ----
__global__ void sqdiff_u8_kernel(const uint8_t* a, const uint8_t* b, double* out, int H, int W, int C, int crop) {
  const int img = blockIdx.y;
  const int h = H - 2 * crop, w = W - 2 * crop;
  const size_t n = (size_t)h * w * C;
  const uint8_t* pa = a + (size_t)img * H * W * C;
  const uint8_t* pb = b + (size_t)img * H * W * C;
  double sd = 0.0;      // (terms are integers <= 65025: fp32 sums would lose bits after ~258 of them)
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int x = (int)(p % w), y = (int)(p / w);
    const size_t o = ((size_t)(y + crop) * W + (x + crop)) * C + c;
    const float d = (float)pa[o] - (float)pb[o];
    sd += (double)(d * d);
  }
  for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
  __shared__ double dred[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) dred[wv] = sd;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)((blockDim.x + 63) >> 6); ++i) t += dred[i];
    atomicAdd(out + img, t);
  }
}

// ---- SSIM (skimage.metrics.structural_similarity defaults, channel_axis = -1, data_range = 255) ----
// One thread per (valid window position, channel): the 7x7 window sums in double-free fp32 are exact for 8-bit data
// (49 * 255^2 < 2^24).  S is accumulated per image in double.
__global__ void ssim_u8_kernel(const uint8_t* a, const uint8_t* b, double* out, int H, int W, int C, int crop) {
  constexpr int WIN = 7;
  const int img = blockIdx.y;
  const int h = H - 2 * crop, w = W - 2 * crop;          // the cropped image skimage sees
  const int vh = h - (WIN - 1), vw = w - (WIN - 1);      // window centres left after skimage's own (WIN-1)/2 border crop
  const size_t n = (size_t)vh * vw * C;
  const uint8_t* pa = a + (size_t)img * H * W * C;
  const uint8_t* pb = b + (size_t)img * H * W * C;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double NP = WIN * WIN, cov_norm = NP / (NP - 1.0);
  double sd = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int x = (int)(p % vw), y = (int)(p / vw);
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
    for (int dy = 0; dy < WIN; ++dy)
      for (int dx = 0; dx < WIN; ++dx) {
        const size_t o = ((size_t)(y + dy + crop) * W + (x + dx + crop)) * C + c;
        const float u = (float)pa[o], v = (float)pb[o];
        sx += u; sy += v; sxx += u * u; syy += v * v; sxy += u * v;
      }
    const double ux = sx / NP, uy = sy / NP, uxx = sxx / NP, uyy = syy / NP, uxy = sxy / NP;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    sd += (A1 * A2) / (B1 * B2);
  }
  for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
  __shared__ double dred[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) dred[wv] = sd;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)((blockDim.x + 63) >> 6); ++i) t += dred[i];
    // order-independent accumulation: the block sum as 2^-32 fixed point in a 64-bit integer (|S| <= 1 per window: no overflow below
    // 2^31 windows per image); ssim_fix_kernel turns the slot into the double the caller reads
    atomicAdd(reinterpret_cast<unsigned long long*>(out) + img, (unsigned long long)(long long)llrint(t * 4294967296.0));
  }
}
__global__ void ssim_fix_kernel(double* out, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) out[i] = (double)(long long)reinterpret_cast<unsigned long long*>(out)[i] * (1.0 / 4294967296.0);
}

// total = sum_i w_i * t_i (accumulated left to right, like `a*x + b*y + c*z` in the reference's trainer.py:104-115), scaled[i] = w_i * t_i
struct ScalarSumArgs {
  const float* t[8];
  float w[8];
  int n;
};
__global__ void scalar_wsum_kernel(ScalarSumArgs a, float* total, float* scaled) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float acc = 0.f;
    for (int i = 0; i < a.n; ++i) {
      const float v = a.w[i] * a.t[i][0];
      if (scaled) scaled[i] = v;
      acc = i == 0 ? v : acc + v;
    }
    *total = acc;
  }
}
// gout[i] = w_i * g
__global__ void scalar_wsum_bwd_kernel(ScalarSumArgs a, const float* g, float* gout) {
  if (blockIdx.x == 0 && (int)threadIdx.x < a.n) gout[threadIdx.x] = a.w[threadIdx.x] * g[0];
}

// out[i] = t_i[0]
__global__ void gather_scalars_kernel(ScalarSumArgs a, float* out) {
  if (blockIdx.x == 0 && (int)threadIdx.x < a.n) out[threadIdx.x] = a.t[threadIdx.x][0];
}

}  // namespace uegan

using namespace uegan;

extern "C" int uegan_gather_scalars(int n, const float* const* src, float* out, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(n >= 1 && n <= 8 && src && out, "gather_scalars: 1..8 scalars");
  ScalarSumArgs a;
  a.n = n;
  for (int i = 0; i < 8; ++i) { a.t[i] = i < n ? src[i] : nullptr; a.w[i] = 0.f; }
  for (int i = 0; i < n; ++i) UEGAN_CHECK_ARG(src[i], "null scalar %d", i);
  hipLaunchKernelGGL(gather_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, out);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_fill_zero(void* p, size_t bytes, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(p || bytes == 0, "null pointer");
  if (bytes == 0) return UEGAN_OK;
  hipError_t e = hipMemsetAsync(p, 0, bytes, (hipStream_t)stream);
  if (e != hipSuccess) { set_error("hipMemsetAsync failed: %s", hipGetErrorString(e)); return UEGAN_E_HIP; }
  return UEGAN_OK;
}

extern "C" int uegan_scalar_wsum(int n, const float* const* terms, const float* weights, float* total, float* scaled, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(n >= 1 && n <= 8 && terms && weights && total, "scalar_wsum: 1..8 terms");
  ScalarSumArgs a;
  a.n = n;
  for (int i = 0; i < 8; ++i) { a.t[i] = i < n ? terms[i] : nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
  for (int i = 0; i < n; ++i) UEGAN_CHECK_ARG(terms[i], "null term %d", i);
  hipLaunchKernelGGL(scalar_wsum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, total, scaled);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_scalar_wsum_bwd(int n, const float* weights, const float* g, float* gout, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(n >= 1 && n <= 8 && weights && g && gout, "scalar_wsum_bwd: 1..8 terms");
  ScalarSumArgs a;
  a.n = n;
  for (int i = 0; i < 8; ++i) { a.t[i] = nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
  hipLaunchKernelGGL(scalar_wsum_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, g, gout);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_copy_images(float* dst, const float* src_a, const float* src_b, const int32_t* dst_idx, const int32_t* src_idx,
                                 int n_images, int64_t image_elems, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(dst && src_a && src_b && dst_idx && src_idx && image_elems > 0, "bad copy_images args");
  UEGAN_CHECK_ARG(n_images >= 0 && n_images <= COPY_MAX_IMAGES, "copy_images takes at most %d images per call (got %d)", COPY_MAX_IMAGES, n_images);
  if (n_images == 0) return UEGAN_OK;
  CopyTable t;
  for (int i = 0; i < n_images; ++i) {
    UEGAN_CHECK_ARG(dst_idx[i] >= 0, "negative destination index");
    t.dst[i] = dst_idx[i];
    t.src[i] = src_idx[i];
  }
  const bool vec = image_elems % 4 == 0 && ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src_a % 16 == 0) && ((uintptr_t)src_b % 16 == 0);
  const size_t work = vec ? (size_t)image_elems / 4 : (size_t)image_elems;
  const int bx = (int)((work + 255) / 256 < 256 ? (work + 255) / 256 : 256);
  if (vec) hipLaunchKernelGGL((copy_images_kernel<4>), dim3(bx, n_images), dim3(256), 0, (hipStream_t)stream, dst, src_a, src_b, t, (size_t)image_elems);
  else hipLaunchKernelGGL((copy_images_kernel<1>), dim3(bx, n_images), dim3(256), 0, (hipStream_t)stream, dst, src_a, src_b, t, (size_t)image_elems);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_quantize_u8(const float* x_nchw, uint8_t* y_nhwc, int B, int C, int H, int W, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x_nchw && y_nhwc && B > 0 && C > 0 && H > 0 && W > 0, "bad quantize_u8 args");
  const size_t n = (size_t)B * C * H * W;
  const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(quantize_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_nchw, y_nhwc, B, C, H * W);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

static int montage_launch(const char* who, const float* const* srcs_nchw, int n, uint8_t* y_nhwc, int B, int C, const MontageGeom& g, uegan_stream_t stream) {
  const int Hs = g.Hs, Ws = g.Ws, H = g.H, W = g.W;
  UEGAN_CHECK_ARG(srcs_nchw && y_nhwc && B > 0 && C > 0 && H > 0 && W > 0, "bad %s args", who);
  UEGAN_CHECK_ARG(n >= 1 && n <= MONTAGE_MAX_SRCS, "%s takes 1..%d images (got %d)", who, MONTAGE_MAX_SRCS, n);
  UEGAN_CHECK_ARG(g.sy >= 0 && g.sx >= 0 && (long long)g.sy + H <= Hs && (long long)g.sx + W <= Ws, "%s: the %d x %d window at (%d, %d) does not fit its %d x %d source",
                  who, H, W, g.sy, g.sx, Hs, Ws);
  UEGAN_CHECK_ARG(g.dy >= 0 && g.dx >= 0 && g.Wp >= W && (long long)g.dy + H <= g.Hd && (long long)g.dx + (long long)(n - 1) * g.Wp + W <= g.Wd,
                  "%s: %d panels of %d x %d (pitch %d) at (%d, %d) do not fit the %d x %d destination", who, n, H, W, g.Wp, g.dy, g.dx, g.Hd, g.Wd);
  MontageSrcs s;
  bool vec = W % MONTAGE_VEC == 0 && Ws % MONTAGE_VEC == 0 && g.sx % MONTAGE_VEC == 0 && (uintptr_t)y_nhwc % 4 == 0 && (C == 1 || C == 3 || C == 4);
  // (every panel row starts on a dword of y: (Wd, dx, Wp) * C bytes are multiples of 4)
  vec = vec && ((size_t)g.Wd * C) % 4 == 0 && ((size_t)g.dx * C) % 4 == 0 && (n == 1 || ((size_t)g.Wp * C) % 4 == 0);
  for (int k = 0; k < MONTAGE_MAX_SRCS; ++k) {
    s.p[k] = k < n ? srcs_nchw[k] : nullptr;
    if (k < n) {
      UEGAN_CHECK_ARG(srcs_nchw[k], "%s: null image %d", who, k);
      vec = vec && (uintptr_t)srcs_nchw[k] % 16 == 0;
    }
  }
  const size_t rows = (size_t)B * H;
  const size_t items = rows * n * (vec ? W / MONTAGE_VEC : W);
  const size_t want = (items + MONTAGE_THREADS - 1) / MONTAGE_THREADS;
  const dim3 grid((unsigned)(want < (size_t)MONTAGE_MAX_BLOCKS ? want : (size_t)MONTAGE_MAX_BLOCKS)), block(MONTAGE_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (!vec) hipLaunchKernelGGL(montage_u8_kernel, grid, block, 0, st, s, n, y_nhwc, rows, C, g);
  else if (C == 3) hipLaunchKernelGGL((montage_u8_vec_kernel<3>), grid, block, 0, st, s, n, y_nhwc, rows, g);
  else if (C == 1) hipLaunchKernelGGL((montage_u8_vec_kernel<1>), grid, block, 0, st, s, n, y_nhwc, rows, g);
  else hipLaunchKernelGGL((montage_u8_vec_kernel<4>), grid, block, 0, st, s, n, y_nhwc, rows, g);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_montage_u8(const float* const* srcs_nchw, int n, uint8_t* y_nhwc, int B, int C, int H, int W, uegan_stream_t stream) {
  return montage_launch("montage_u8", srcs_nchw, n, y_nhwc, B, C, MontageGeom{H, W, 0, 0, H, W, H, n * W, 0, 0, W}, stream);
}

extern "C" int uegan_montage_crop_u8(const float* const* srcs_nchw, int n, uint8_t* y_nhwc, int B, int C, int Hs, int Ws, int H, int W,
                                     uegan_stream_t stream) {
  return montage_launch("montage_crop_u8", srcs_nchw, n, y_nhwc, B, C, MontageGeom{Hs, Ws, 0, 0, H, W, H, n * W, 0, 0, W}, stream);
}

extern "C" int uegan_montage_place_u8(const float* const* srcs_nchw, int n, uint8_t* y_nhwc, int B, int C, int Hs, int Ws, int sy, int sx, int H, int W,
                                      int Hd, int Wd, int dy, int dx, int Wpanel, uegan_stream_t stream) {
  return montage_launch("montage_place_u8", srcs_nchw, n, y_nhwc, B, C, MontageGeom{Hs, Ws, sy, sx, H, W, Hd, Wd, dy, dx, Wpanel}, stream);
}

extern "C" int uegan_image_metrics_u8(const uint8_t* a_nhwc, const uint8_t* b_nhwc, double* sqdiff_sum, double* ssim_sum, int B, int H, int W,
                                      int C, int crop_border, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(a_nhwc && b_nhwc && (sqdiff_sum || ssim_sum) && B > 0 && C > 0 && crop_border >= 0, "bad image_metrics args");
  UEGAN_CHECK_ARG(H - 2 * crop_border >= 7 && W - 2 * crop_border >= 7, "image too small for a 7x7 SSIM window after the border crop");
  hipStream_t s = (hipStream_t)stream;
  const int h = H - 2 * crop_border, w = W - 2 * crop_border;
  if (sqdiff_sum) {
    UEGAN_CHECK_ARG(hipMemsetAsync(sqdiff_sum, 0, sizeof(double) * B, s) == hipSuccess, "memset failed");
    const size_t n = (size_t)h * w * C;
    const int bx = (int)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512);
    hipLaunchKernelGGL(sqdiff_u8_kernel, dim3(bx, B), dim3(256), 0, s, a_nhwc, b_nhwc, sqdiff_sum, H, W, C, crop_border);
    UEGAN_CHECK_LAUNCH();
  }
  if (ssim_sum) {
    UEGAN_CHECK_ARG(hipMemsetAsync(ssim_sum, 0, sizeof(double) * B, s) == hipSuccess, "memset failed");
    const size_t n = (size_t)(h - 6) * (w - 6) * C;
    const int bx = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(ssim_u8_kernel, dim3(bx, B), dim3(256), 0, s, a_nhwc, b_nhwc, ssim_sum, H, W, C, crop_border);
    UEGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_fix_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ssim_sum, B);
    UEGAN_CHECK_LAUNCH();
  }
  return UEGAN_OK;
}

// ---- NIMA scorer (nima.h): fp32 NHWC tensors whose channel counts are multiples of 16 ----
static bool nima_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int uegan_nima_conv3x3_first(const float* x, int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x, const float* w_kc,
                                        const float* scale, const float* shift, float* y_nhwc, int B, int H, int W, int Cout_pad, int stride,
                                        float lo, float hi, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && w_kc && scale && shift && y_nhwc, "nima_conv3x3_first: null pointer");
  UEGAN_CHECK_ARG(B > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2), "nima_conv3x3_first: bad geometry");
  UEGAN_CHECK_ARG(Cout_pad > 0 && Cout_pad % NIMA_CPAD == 0, "nima_conv3x3_first: Cout_pad must be a multiple of %d (got %d)", NIMA_CPAD, Cout_pad);
  UEGAN_CHECK_ARG(stride_b >= 0 && stride_c > 0 && stride_y > 0 && stride_x > 0, "nima_conv3x3_first: bad input strides");
  UEGAN_CHECK_ARG(nima_aligned(w_kc) && nima_aligned(scale) && nima_aligned(shift) && nima_aligned(y_nhwc), "nima_conv3x3_first: 16-byte alignment");
  nima_first_launch(x, stride_b, stride_c, stride_y, stride_x, w_kc, scale, shift, y_nhwc, B, H, W, Cout_pad, stride, lo, hi, (hipStream_t)stream);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_nima_dwconv3x3(const float* x_nhwc, const float* w_9c, const float* scale, const float* shift, float* y_nhwc, int B, int H, int W,
                                    int C_pad, int stride, float lo, float hi, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x_nhwc && w_9c && scale && shift && y_nhwc, "nima_dwconv3x3: null pointer");
  UEGAN_CHECK_ARG(B > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2), "nima_dwconv3x3: bad geometry");
  UEGAN_CHECK_ARG(C_pad > 0 && C_pad % NIMA_CPAD == 0, "nima_dwconv3x3: C_pad must be a multiple of %d (got %d)", NIMA_CPAD, C_pad);
  UEGAN_CHECK_ARG(nima_aligned(x_nhwc) && nima_aligned(w_9c) && nima_aligned(scale) && nima_aligned(shift) && nima_aligned(y_nhwc),
                  "nima_dwconv3x3: 16-byte alignment");
  UEGAN_CHECK_ARG((size_t)B * H * W * (C_pad / 4) < ((size_t)1 << 31) * 256, "nima_dwconv3x3: tensor too large");
  nima_dw_launch(x_nhwc, w_9c, scale, shift, y_nhwc, B, H, W, C_pad, stride, lo, hi, (hipStream_t)stream);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_nima_pwconv(const float* x_mk, const float* w_nk, const float* scale, const float* shift, const float* residual, float* y_mn,
                                 int64_t M, int Cin_pad, int Cout_pad, float lo, float hi, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x_mk && w_nk && scale && shift && y_mn, "nima_pwconv: null pointer");
  UEGAN_CHECK_ARG(M > 0 && M <= (int64_t)65535 * 16, "nima_pwconv: 1..%d rows per call (got %lld)", 65535 * 16, (long long)M);
  UEGAN_CHECK_ARG(Cin_pad > 0 && Cin_pad % NIMA_CPAD == 0 && Cout_pad > 0 && Cout_pad % NIMA_CPAD == 0,
                  "nima_pwconv: channel counts must be multiples of %d (got %d -> %d)", NIMA_CPAD, Cin_pad, Cout_pad);
  UEGAN_CHECK_ARG(nima_aligned(x_mk) && nima_aligned(w_nk) && nima_aligned(scale) && nima_aligned(shift) && nima_aligned(y_mn) && nima_aligned(residual),
                  "nima_pwconv: 16-byte alignment");
  nima_pw_launch(x_mk, w_nk, scale, shift, residual, y_mn, (int)M, Cin_pad, Cout_pad, lo, hi, (hipStream_t)stream);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_nima_head(const float* x_nhwc, const float* w, const float* bias, float* pooled, float* probs, float* mean, float* std, int B,
                               int HW, int C_pad, int C, int n_classes, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x_nhwc && w && bias && probs && mean && std, "nima_head: null pointer");
  UEGAN_CHECK_ARG(B > 0 && HW > 0 && C > 0 && C <= C_pad && C <= NIMA_HEAD_MAX_C, "nima_head: 1..%d channels (got %d of %d)", NIMA_HEAD_MAX_C, C, C_pad);
  UEGAN_CHECK_ARG(n_classes >= 1 && n_classes <= NIMA_HEAD_MAX_CLS, "nima_head: 1..%d classes (got %d)", NIMA_HEAD_MAX_CLS, n_classes);
  hipLaunchKernelGGL(nima_head_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x_nhwc, w, bias, pooled, probs, mean, std, HW, C_pad, C, n_classes);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
