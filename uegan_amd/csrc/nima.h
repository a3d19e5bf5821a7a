// NIMA aesthetic scorer (metrics/NIMA/CalcNIMA.py: a MobileNetV2 trunk + ReLU -> Linear(1280, 10) -> Softmax head) in eval mode, fp32
// storage and fp32 accumulation (a metric is a measuring instrument; the whole network is 0.3 GFLOP per image).  All activations are
// NHWC with the channel count padded to a multiple of 16 (one MFMA tile of output channels); padded channels carry zero weights and a
// zero shift, so they stay exactly zero through every layer.  Eval-mode BatchNorm is folded by the caller into a per-channel
// (scale, shift) pair that every convolution applies in its epilogue, followed by clamp(lo, hi): (0, 6) is ReLU6, (0, +inf) ReLU,
// (-inf, +inf) none.  Four kernels:
//   nima_first_kernel   3x3 zero-padded strided convolution from 3 input channels read through arbitrary strides (NCHW or NHWC)
//   nima_dw_kernel      depthwise 3x3, stride 1 or 2: memory-bound, one 16-byte chunk of channels per lane, weights in registers,
//                       input rows kept in registers while the lane walks down a strip of output rows
//   nima_pw_kernel      1x1 convolution = GEMM on v_mfma_f32_16x16x4_f32, optional residual added after the affine
//   nima_head_kernel    global average pool + ReLU + Linear + softmax + mean / standard deviation of the score distribution
#pragma once
#include "common.h"

namespace uegan {

constexpr int NIMA_CPAD = 16;             // channel padding of every NHWC tensor of the scorer
constexpr int NIMA_HEAD_MAX_C = 2048;     // pooled vector kept in LDS
constexpr int NIMA_HEAD_MAX_CLS = 16;

__device__ __forceinline__ float nima_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- first layer: y[b][yo][xo][co] = clamp(scale[co] * sum_{ky,kx,ci} x[b][ci][yo*s-1+ky][xo*s-1+kx] * w[(ky*3+kx)*3+ci][co] + shift[co]) ----
// One thread per pixel and NIMA_FIRST_CT output channels: blockIdx.y picks the channel group, whose 27 x NIMA_FIRST_CT weights sit in LDS
// (every lane reads the same address: a broadcast), the 27 inputs of a pixel are loaded once per group and each lane stores
// NIMA_FIRST_CT contiguous floats.
constexpr int NIMA_FIRST_CT = 16;
__global__ void __launch_bounds__(256) nima_first_kernel(const float* x, long long sb, long long sc, long long sy, long long sx, const float* w, const float* scale,
                                  const float* shift, float* y, int B, int H, int W, int Ho, int Wo, int Cp, int stride, float lo, float hi) {
  const int c0 = blockIdx.y * NIMA_FIRST_CT;
  __shared__ float ws[27 * NIMA_FIRST_CT];
  for (int t = threadIdx.x; t < 27 * NIMA_FIRST_CT; t += blockDim.x) ws[t] = w[(size_t)(t / NIMA_FIRST_CT) * Cp + c0 + t % NIMA_FIRST_CT];
  __syncthreads();
  const size_t total = (size_t)B * Ho * Wo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    const size_t r = i / Wo;
    const int yo = (int)(r % Ho), b = (int)(r / Ho);
    float acc[NIMA_FIRST_CT];
#pragma unroll
    for (int e = 0; e < NIMA_FIRST_CT; ++e) acc[e] = 0.f;
    const float* xb = x + (size_t)b * sb;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {      // (one tap at a time: unrolled, the compiler fetches all 432 weights first and spills)
      const int ky = k / 3, kx = k - 3 * ky;
      const int iy = yo * stride - 1 + ky, ix = xo * stride - 1 + kx;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float* px = xb + (size_t)(in ? iy : 0) * sy + (size_t)(in ? ix : 0) * sx;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float v = in ? px[(size_t)ci * sc] : 0.f;          // zero padding: a zero term leaves the sum unchanged
        const float* wk = ws + (k * 3 + ci) * NIMA_FIRST_CT;
#pragma unroll
        for (int e = 0; e < NIMA_FIRST_CT; ++e) acc[e] = fmaf(v, wk[e], acc[e]);
      }
    }
    float* yp = y + i * Cp + c0;
#pragma unroll
    for (int q = 0; q < NIMA_FIRST_CT / 4; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = nima_clamp(fmaf(acc[4 * q + e], scale[c0 + 4 * q + e], shift[c0 + 4 * q + e]), lo, hi);
      *reinterpret_cast<f32x4*>(yp + 4 * q) = o;
    }
  }
}

// ---- depthwise 3x3, zero padding 1: w is [9][C] (tap-major), x [B][H][W][C], y [B][Ho][Wo][C], C % 4 == 0 ----
// A lane owns 4 channels of one output column and walks down R output rows.  Its 36 weights and a 3 x 3 window of 16-byte input chunks
// live in registers; moving down one output row loads STRIDE new input rows (3 chunks each) and keeps the rest.
__device__ __forceinline__ void nima_dw_load_row(const float* xb, int iy, int ix0, int H, int W, int C, f32x4 (&row)[3]) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ix = ix0 + k;
    row[k] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? *reinterpret_cast<const f32x4*>(xb + ((size_t)iy * W + ix) * C) : z;
  }
}

template <int STRIDE>
__global__ void nima_dw_kernel(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int H, int W, int C,
                               int Ho, int Wo, int R, float lo, float hi) {
  const int C4 = C >> 2;
  const int strips = (Ho + R - 1) / R;
  const size_t total = (size_t)B * strips * Wo * C4;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  size_t p = i / C4;
  const int xo = (int)(p % Wo);
  p /= Wo;
  const int strip = (int)(p % strips), b = (int)(p / strips);
  const int y0 = strip * R, y1 = (y0 + R < Ho) ? y0 + R : Ho;
  const float* xb = x + (size_t)b * H * W * C + c4 * 4;
  float* yb = y + (size_t)b * Ho * Wo * C + c4 * 4;
  f32x4 wr[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wr[k] = *reinterpret_cast<const f32x4*>(w + (size_t)k * C + c4 * 4);
  const f32x4 sv = *reinterpret_cast<const f32x4*>(scale + c4 * 4), tv = *reinterpret_cast<const f32x4*>(shift + c4 * 4);
  const int ix0 = xo * STRIDE - 1;
  f32x4 r0[3], r1[3], r2[3];
  // rows of the first output row; afterwards the window slides by STRIDE rows
  nima_dw_load_row(xb, y0 * STRIDE - 1, ix0, H, W, C, r0);
  nima_dw_load_row(xb, y0 * STRIDE, ix0, H, W, C, r1);
  nima_dw_load_row(xb, y0 * STRIDE + 1, ix0, H, W, C, r2);
  for (int yo = y0; yo < y1; ++yo) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] = fmaf(r0[k][e], wr[k][e], acc[e]);
        acc[e] = fmaf(r1[k][e], wr[3 + k][e], acc[e]);
        acc[e] = fmaf(r2[k][e], wr[6 + k][e], acc[e]);
      }
    }
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = nima_clamp(fmaf(acc[e], sv[e], tv[e]), lo, hi);
    *reinterpret_cast<f32x4*>(yb + ((size_t)yo * Wo + xo) * C) = o;
    if (yo + 1 < y1) {
      const int iy = (yo + 1) * STRIDE - 1;        // first input row of the next output row
      if (STRIDE == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { r0[k] = r1[k]; r1[k] = r2[k]; }
        nima_dw_load_row(xb, iy + 2, ix0, H, W, C, r2);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) r0[k] = r2[k];
        nima_dw_load_row(xb, iy + 1, ix0, H, W, C, r1);
        nima_dw_load_row(xb, iy + 2, ix0, H, W, C, r2);
      }
    }
  }
}

// ---- pointwise 1x1 = GEMM: y[m][n] = clamp(scale[n] * sum_k x[m][k] * w[n][k] + shift[n]) (+ res[m][n]) ----
// x [M][K], w [N][K] (the convolution's own [Cout][Cin] layout, zero-padded), y / res [M][N]; K % 16 == 0, N % 16 == 0.
// One wave per workgroup computes NT tiles of 16 output channels x MT tiles of 16 pixels with v_mfma_f32_16x16x4_f32, channels as the
// MFMA's row index: the A operand is the weight (lane l: channel l & 15), the B operand the pixel (lane l: pixel l & 15), and lane l
// ends up with channels 4 * (l >> 4) .. + 3 of pixel l & 15 -- one 16-byte store, one 16-byte scale / shift / residual load.
// Operands come straight from global memory as 16-byte chunks: lane l loads k = kk + 4 * (l >> 4) .. + 3 of its row, and the four MFMAs
// of a 16-wide k step take element s of both chunks (the k order inside the step is permuted identically on both sides).
// blockIdx.x runs over the channel tiles (fastest), so the waves that share a strip of pixels run together and re-read it from the cache.
template <int NT, int MT>
__global__ void __launch_bounds__(64) nima_pw_kernel(const float* x, const float* w, const float* scale, const float* shift, const float* res,
                                                     float* y, int M, int K, int N, float lo, float hi) {
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int m0 = blockIdx.y * (16 * MT);
  const float* wp[NT];
  const float* xp[MT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wp[t] = w + (size_t)(n0 + 16 * t + l15) * K + 4 * lg;       // n0 + 16 * NT <= N by the launch
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    int m = m0 + 16 * t + l15;
    m = m < M ? m : M - 1;                                   // rows past the end read the last row and are never stored
    xp[t] = x + (size_t)m * K + 4 * lg;
  }
  f32x4 acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int c = 0; c < MT; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < K; kk += 16) {
    f32x4 wa[NT], xa[MT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wa[t] = *reinterpret_cast<const f32x4*>(wp[t] + kk);
#pragma unroll
    for (int t = 0; t < MT; ++t) xa[t] = *reinterpret_cast<const f32x4*>(xp[t] + kk);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int c = 0; c < MT; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[a][s], xa[c][s], acc[a][c], 0, 0, 0);
  }
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const int n = n0 + 16 * a + 4 * lg;
    const f32x4 sv = *reinterpret_cast<const f32x4*>(scale + n), tv = *reinterpret_cast<const f32x4*>(shift + n);
#pragma unroll
    for (int c = 0; c < MT; ++c) {
      const int m = m0 + 16 * c + l15;
      if (m >= M) continue;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = nima_clamp(fmaf(acc[a][c][e], sv[e], tv[e]), lo, hi);
      if (res) {
        const f32x4 rv = *reinterpret_cast<const f32x4*>(res + (size_t)m * N + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += rv[e];
      }
      *reinterpret_cast<f32x4*>(y + (size_t)m * N + n) = o;
    }
  }
}

// ---- head: AvgPool over HW -> ReLU -> Linear(C -> ncls) + bias -> softmax -> mean = sum j p_j, std = sqrt(sum p_j (j - mean)^2), j = 1.. ----
// One workgroup of 1024 threads per image.  pooled (optional) receives the pooled vector BEFORE the ReLU (what the trunk hands the head).
__global__ void __launch_bounds__(1024) nima_head_kernel(const float* x, const float* w, const float* bias, float* pooled, float* probs, float* mean,
                                                        float* stdv, int HW, int Cp, int C, int ncls) {
  __shared__ float feat[NIMA_HEAD_MAX_C];
  __shared__ float logit[NIMA_HEAD_MAX_CLS];
  const int b = blockIdx.x;
  const float* xb = x + (size_t)b * HW * Cp;
  const float inv = 1.f / (float)HW;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
#pragma unroll 7
    for (int p = 0; p < HW; ++p) s += xb[(size_t)p * Cp + c];      // (unrolled: the loads of a group are in flight together)
    const float v = s * inv;
    if (pooled) pooled[(size_t)b * C + c] = v;
    feat[c] = fmaxf(v, 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int j = wv; j < ncls; j += nw) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(feat[c], w[(size_t)j * C + c], s);
    s = wave_sum(s);
    if (lane == 0) logit[j] = s + bias[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mx = logit[0];
    for (int j = 1; j < ncls; ++j) mx = fmaxf(mx, logit[j]);
    float e[NIMA_HEAD_MAX_CLS];
    float den = 0.f;
    for (int j = 0; j < ncls; ++j) { e[j] = expf(logit[j] - mx); den += e[j]; }
    float mu = 0.f;
    for (int j = 0; j < ncls; ++j) {
      e[j] = e[j] / den;
      probs[(size_t)b * ncls + j] = e[j];
      mu += (float)(j + 1) * e[j];
    }
    float var = 0.f;
    for (int j = 0; j < ncls; ++j) { const float d = (float)(j + 1) - mu; var += e[j] * d * d; }
    mean[b] = mu;
    stdv[b] = sqrtf(var);
  }
}

// ---- host side ----
inline int nima_first_launch(const float* x, long long sb, long long sc, long long sy, long long sx, const float* w, const float* scale,
                             const float* shift, float* y, int B, int H, int W, int Cp, int stride, float lo, float hi, hipStream_t s) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t total = (size_t)B * Ho * Wo;
  const size_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(nima_first_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536), Cp / NIMA_FIRST_CT), dim3(256), 0, s, x, sb, sc, sy, sx, w,
                     scale, shift, y, B, H, W, Ho, Wo, Cp, stride, lo, hi);
  return 0;
}

inline int nima_dw_launch(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int H, int W, int C, int stride,
                          float lo, float hi, hipStream_t s) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  // rows per lane: as many as keep at least ~64k lanes in flight (row reuse saves loads only while the device stays full)
  int R = 8;
  while (R > 1 && (size_t)B * ((Ho + R - 1) / R) * Wo * (C / 4) < 65536) R >>= 1;
  const size_t total = (size_t)B * ((Ho + R - 1) / R) * Wo * (C / 4);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (stride == 1) hipLaunchKernelGGL((nima_dw_kernel<1>), grid, dim3(256), 0, s, x, w, scale, shift, y, B, H, W, C, Ho, Wo, R, lo, hi);
  else hipLaunchKernelGGL((nima_dw_kernel<2>), grid, dim3(256), 0, s, x, w, scale, shift, y, B, H, W, C, Ho, Wo, R, lo, hi);
  return 0;
}

template <int NT>
inline void nima_pw_launch_nt(const float* x, const float* w, const float* scale, const float* shift, const float* res, float* y, int M, int K, int N,
                              float lo, float hi, hipStream_t s) {
  // 32 pixels per wave while that still gives every CU several waves, 16 otherwise (the 7x7 layers: 49 rows per image)
  const int ntiles = N / (16 * NT);
  if ((size_t)((M + 31) / 32) * ntiles >= 1024) {
    hipLaunchKernelGGL((nima_pw_kernel<NT, 2>), dim3(ntiles, (M + 31) / 32), dim3(64), 0, s, x, w, scale, shift, res, y, M, K, N, lo, hi);
  } else {
    hipLaunchKernelGGL((nima_pw_kernel<NT, 1>), dim3(ntiles, (M + 15) / 16), dim3(64), 0, s, x, w, scale, shift, res, y, M, K, N, lo, hi);
  }
}

inline int nima_pw_launch(const float* x, const float* w, const float* scale, const float* shift, const float* res, float* y, int M, int K, int N,
                          float lo, float hi, hipStream_t s) {
  // channel tiles per wave: the largest of 4, 3, 2, 1 that divides N / 16 -- fewer when the grid would leave CUs idle
  const int t = N / 16;
  int nt = t % 4 == 0 ? 4 : (t % 3 == 0 ? 3 : (t % 2 == 0 ? 2 : 1));
  while (nt > 1 && (size_t)((M + 15) / 16) * (t / nt) < 1024) nt = (nt == 4) ? 2 : 1;
  if (t % nt != 0) nt = 1;
  switch (nt) {
    case 4: nima_pw_launch_nt<4>(x, w, scale, shift, res, y, M, K, N, lo, hi, s); break;
    case 3: nima_pw_launch_nt<3>(x, w, scale, shift, res, y, M, K, N, lo, hi, s); break;
    case 2: nima_pw_launch_nt<2>(x, w, scale, shift, res, y, M, K, N, lo, hi, s); break;
    default: nima_pw_launch_nt<1>(x, w, scale, shift, res, y, M, K, N, lo, hi, s); break;
  }
  return 0;
}

}  // namespace uegan
