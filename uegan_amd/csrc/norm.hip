// The per-(image, channel) reductions over the pixels of an NHWC tensor, all on one work decomposition (RedPlan): moments, InstanceNorm
// (non-affine) forward and backward, affine normalisation + activation on explicit coefficients, and the fidelity-loss tap
// weight * MSE(IN(x), IN(y)) with its gradient.  All HBM-bound: per-thread fp32 accumulation, an LDS tree over the block's pixel lanes,
// fp32 partials per pixel split combined by a finalize kernel -- moments with Chan's formula (means / M2), so the variance never suffers
// E[x^2]-E[x]^2 cancellation.  The adversarial and reconstruction losses are in loss.hip.  Tiled inference adds the moments over a WINDOW of a map,
// accumulated in double across calls (WinPlan, further down).
//
// Reference arithmetic: nn.InstanceNorm2d(affine=False) (models.py:227,236; losses.py:18,30-34), the norm_fun / act_fun variants of ConvBlock
// (models.py:88-101, 249-281), PerceptualLoss tap term (losses.py:30-34).
#include "common.h"
#include "conv_internal.h"
#include "launch.h"

namespace uegan {

// ----------------------------------------------------------------------------------------------------
// work decomposition for per-(b,c) reductions over HW pixels of an NHWC tensor.
// A thread owns V consecutive channels (V = one 16-byte chunk when C allows it, else 1) of a strided set of pixels;
// a block = CG channel lanes x PL pixel lanes over one pixel split; partials are combined by the consumer kernels.
// ----------------------------------------------------------------------------------------------------
struct RedPlan {
  int B, HW, C;
  int V;       // channels per thread
  int CG;      // channel lanes per block (power of two <= 64)
  int PL;      // pixel lanes per block = 256 / CG
  int ncg;     // channel groups
  int S;       // pixel splits
  int chunk;   // pixels per split
  dim3 grid() const { return dim3(S, ncg, B); }      // of every <T, V> kernel below, 256 threads per block
};

static RedPlan make_plan(int B, int HW, int C, int dtype) {
  const int epc = epc_of(dtype);
  RedPlan p;
  p.B = B; p.HW = HW; p.C = C;
  p.V = (C % epc == 0) ? epc : 1;
  const int lanes = C / p.V;
  int cg = 1;
  while (cg < lanes && cg < 64) cg <<= 1;
  p.CG = cg;
  p.PL = 256 / cg;
  p.ncg = (lanes + cg - 1) / cg;
  int s = (HW + 1023) / 1024;
  int cap = 64;
  while ((long)B * p.ncg * cap < 512 && cap < 512) cap *= 2;      // few images (inference: B = 1): more splits, so that the grid still covers the chip
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  // ... and SHORTER splits (down to 128 pixels) while the grid is under ~4 blocks per CU: at B = 1 a 512 x 512 x 32 map was 256 blocks of
  // 4 waves -- 53 us for a 33 MB pass (the streaming kernels need many more waves in flight than that to reach HBM speed)
#if defined(UEGAN_EMU)
  constexpr long kGridTarget = 64;      // (CPU emulator: every block is 256 fibers -- same code path, CI-sized grids)
#else
  constexpr long kGridTarget = 1024;
#endif
  while ((long)B * p.ncg * s < kGridTarget && s < 2048 && HW / (2 * s) >= 128) s *= 2;
  // ... and, on the small maps of the attention modules (<= 64 x 64: ga4 / ga5 of a 512^2 input), down to 16 pixels while ONE image's blocks are a fraction
  // of the chip: at batch 1 these were 8 / 32 blocks whose threads walked 32 / 16 dependent loads (moments 9.7 / 8.5 us, apply 8.7 / 5.4 us for 1 MB).
  // Per image, not per batch: on these maps (at most 4096 pixels; fewer than 8 channel groups, i.e. every layer of the model -- with more, the loop above
  // can outrun this one) the split count does not depend on how many images share the launch, so a pair pass and two single passes are bit-identical there
  // (Generator.forward_pair, tests/test_fused.py; tests/test_reduction_kernels.py pins the range).  Above 4096 pixels S follows B * ncg (the loop above
  // and `cap`): a batch and its images alone then sum in different orders and agree to rounding only.
  while (HW <= 4096 && (long)p.ncg * s < 128 && s < 2048 && HW / (2 * s) >= 16) s *= 2;
  p.chunk = (HW + s - 1) / s;
  p.S = (HW + p.chunk - 1) / p.chunk;
  return p;
}

#define RED_THREAD_SETUP()                                           \
  const int s = blockIdx.x, cg = blockIdx.y, b = blockIdx.z;         \
  const int cl = threadIdx.x % p.CG, pl = threadIdx.x / p.CG;        \
  const int c0 = (cg * p.CG + cl) * V;                               \
  const bool cvalid = c0 < p.C;                                      \
  const int p0 = s * p.chunk;                                        \
  int p1 = p0 + p.chunk;                                             \
  if (p1 > p.HW) p1 = p.HW;                                          \
  const size_t base = (size_t)b * p.HW * p.C + c0;

// partial moments of one tensor: part[((b*S + s)*C + c)*3 + {0,1,2}] = {count, mean, M2}
template <typename T, int V>
__global__ void moments_partial_kernel(const T* x, float* part, RedPlan p) {
  __shared__ float sh[3][V][256];
  RED_THREAD_SETUP();
  float n = 0.f, s1[V], s2[V], K[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { s1[e] = 0.f; s2[e] = 0.f; K[e] = 0.f; }
  if (cvalid) {
    if (p0 + pl < p1) Vec<T, V>::ld(x + base + (size_t)(p0 + pl) * p.C, K);     // shift: first sample of this thread
    _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
      float v[V];
      Vec<T, V>::ld(x + base + (size_t)q * p.C, v);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = v[e] - K[e];
        s1[e] += d;
        s2[e] += d * d;
      }
      n += 1.f;
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    sh[0][e][threadIdx.x] = n;
    sh[1][e][threadIdx.x] = n > 0.f ? K[e] + s1[e] / n : 0.f;
    sh[2][e][threadIdx.x] = n > 0.f ? s2[e] - s1[e] * s1[e] / n : 0.f;
  }
  __syncthreads();
  // pairwise (Chan) merge over the pixel lanes, all threads working: log2(PL) steps instead of a PL-long serial chain on
  // the CG threads of pixel lane 0 (that tail used to cost as much as the streaming loop)
  for (int half = p.PL >> 1; half > 0; half >>= 1) {
    if (pl < half) {
      const int o = threadIdx.x + half * p.CG;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float na = sh[0][e][threadIdx.x], nb = sh[0][e][o];
        if (nb > 0.f) {
          const float nt = na + nb, d = sh[1][e][o] - sh[1][e][threadIdx.x], r = nb / nt;
          sh[1][e][threadIdx.x] += d * r;
          sh[2][e][threadIdx.x] += sh[2][e][o] + d * d * na * r;
          sh[0][e][threadIdx.x] = nt;
        }
      }
    }
    __syncthreads();
  }
  if (pl == 0 && cvalid) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float* o = part + (((size_t)b * p.S + s) * p.C + c0 + e) * 3;
      o[0] = sh[0][e][threadIdx.x]; o[1] = sh[1][e][threadIdx.x]; o[2] = sh[2][e][threadIdx.x];
    }
  }
}

// one WAVE per (b,c): combine the split partials once (consumers then read 2 floats per channel).  Lane l merges partials
// l, l+64, ..., then a butterfly of pairwise Chan merges (fixed order: deterministic); a serial loop over the splits by one thread
// per channel used to take 13-26 us -- more than the streaming pass it follows on small tensors.
__global__ void moments_finalize_kernel(const float* part, float* mean_out, float* rstd_out, RedPlan p, float eps) {
  const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (w >= p.B * p.C) return;
  const int b = w / p.C, c = w - b * p.C;
  float N = 0.f, M = 0.f, Q = 0.f;
  for (int sp = lane; sp < p.S; sp += 64) {
    const float* o = part + (((size_t)b * p.S + sp) * p.C + c) * 3;
    const float nb = o[0], mb = o[1], qb = o[2];
    if (nb > 0.f) {
      const float nt = N + nb, d = mb - M;
      M += d * nb / nt;
      Q += qb + d * d * N * nb / nt;
      N = nt;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float nb = __shfl_xor(N, o, 64), mb = __shfl_xor(M, o, 64), qb = __shfl_xor(Q, o, 64);
    const float nt = N + nb;
    if (nt > 0.f) {
      // symmetric form: both partners compute the same merged triple
      const float wa = N / nt, wb = nb / nt, d = mb - M;
      Q = Q + qb + d * d * N * wb;
      M = M * wa + mb * wb;
      N = nt;
    }
  }
  if (lane == 0) {
    const float var = N > 0.f ? Q / N : 0.f;
    mean_out[w] = M;
    rstd_out[w] = eps < 0.f ? var : 1.f / sqrtf(var + eps);      // (eps < 0: the caller wants the biased variance itself)
  }
}
// out[(b*C + c)*K + k] = sum_s part[((b*S + s)*C + c)*K + k]: one wave per output element
__global__ void sums_finalize_kernel(const float* part, float* out, RedPlan p, int K) {
  const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (w >= p.B * p.C * K) return;
  const int k = w % K, bc = w / K, b = bc / p.C, c = bc % p.C;
  float t = 0.f;
  for (int sp = lane; sp < p.S; sp += 64) t += part[(((size_t)b * p.S + sp) * p.C + c) * K + k];
  t = wave_sum(t);
  if (lane == 0) out[w] = t;
}

template <typename T, int V>
__global__ void instnorm_apply_kernel(const T* x, T* y, const float* mean_in, const float* rstd_in, RedPlan p) {
  RED_THREAD_SETUP();
  if (!cvalid) return;
  float mean[V], rstd[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    mean[e] = mean_in[(size_t)b * p.C + c0 + e];
    rstd[e] = rstd_in[(size_t)b * p.C + c0 + e];
  }
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float v[V];
    Vec<T, V>::ld(x + base + (size_t)q * p.C, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = (v[e] - mean[e]) * rstd[e];
    Vec<T, V>::st(y + base + (size_t)q * p.C, v);
  }
}

// the same on a hi + lo pair of 16-bit planes (value = hi + lo), result as a pair: the attention module's InstanceNorm in the `precise` mode
template <typename T, int V>
__global__ void instnorm_apply_pair_kernel(const T* x, const T* xl, T* y, T* yl, const float* mean_in, const float* rstd_in, RedPlan p) {
  RED_THREAD_SETUP();
  if (!cvalid) return;
  float mean[V], rstd[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    mean[e] = mean_in[(size_t)b * p.C + c0 + e];
    rstd[e] = rstd_in[(size_t)b * p.C + c0 + e];
  }
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float v[V], l[V], h[V];
    Vec<T, V>::ld(x + base + (size_t)q * p.C, v);
    Vec<T, V>::ld(xl + base + (size_t)q * p.C, l);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = ((v[e] - mean[e]) + l[e]) * rstd[e];
    Vec<T, V>::st(y + base + (size_t)q * p.C, v);
#pragma unroll
    for (int e = 0; e < V; ++e) {                      // (what the store rounded to: the lo plane takes the rest)
      T r;
      DT<T>::st(&r, v[e]);
      h[e] = DT<T>::ld(&r);
      l[e] = v[e] - h[e];
    }
    Vec<T, V>::st(yl + base + (size_t)q * p.C, l);
  }
}

// backward partial sums: part[((b*S+s)*C + c)*2 + {0,1}] = {sum dy, sum dy*y}
template <typename T, int V>
__global__ void instnorm_bwd_partial_kernel(const T* dy, const T* y, float* part, RedPlan p) {
  __shared__ float sh[2][V][256];
  RED_THREAD_SETUP();
  float a0[V], a1[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { a0[e] = 0.f; a1[e] = 0.f; }
  if (cvalid) {
    _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
      float gv[V], yv[V];
      Vec<T, V>::ld(dy + base + (size_t)q * p.C, gv);
      Vec<T, V>::ld(y + base + (size_t)q * p.C, yv);
#pragma unroll
      for (int e = 0; e < V; ++e) { a0[e] += gv[e]; a1[e] += gv[e] * yv[e]; }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] = a0[e]; sh[1][e][threadIdx.x] = a1[e]; }
  __syncthreads();
  for (int half = p.PL >> 1; half > 0; half >>= 1) {        // tree over the pixel lanes (PL is a power of two)
    if (pl < half) {
      const int o = threadIdx.x + half * p.CG;
#pragma unroll
      for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] += sh[0][e][o]; sh[1][e][threadIdx.x] += sh[1][e][o]; }
    }
    __syncthreads();
  }
  if (pl == 0 && cvalid) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float* o = part + (((size_t)b * p.S + s) * p.C + c0 + e) * 2;
      o[0] = sh[0][e][threadIdx.x]; o[1] = sh[1][e][threadIdx.x];
    }
  }
}

template <typename T, int V>
__global__ void instnorm_bwd_apply_kernel(const T* dy, const T* y, const float* rstd, const float* tot, T* dx, RedPlan p) {
  RED_THREAD_SETUP();
  if (!cvalid) return;
  float m0[V], m1[V], r[V];
  const float inv_n = 1.f / (float)p.HW;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float* o = tot + ((size_t)b * p.C + c0 + e) * 2;
    m0[e] = o[0] * inv_n; m1[e] = o[1] * inv_n; r[e] = rstd[(size_t)b * p.C + c0 + e];
  }
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float gv[V], yv[V];
    Vec<T, V>::ld(dy + base + (size_t)q * p.C, gv);
    Vec<T, V>::ld(y + base + (size_t)q * p.C, yv);
#pragma unroll
    for (int e = 0; e < V; ++e) gv[e] = r[e] * (gv[e] - m0[e] - yv[e] * m1[e]);
    Vec<T, V>::st(dx + base + (size_t)q * p.C, gv);
  }
}

// ----------------------------------------------------------------------------------------------------
// Affine normalisation + activation on explicit per-(b,c) coefficients: the norm_fun / act_fun variants of ConvBlock
// (models.py:88-101, 249-281: BatchNorm2d / InstanceNorm2d(affine, running statistics) followed by LeakyReLU | ReLU | Swish | SELU).
//   forward   y = act(x * scale[b,c] + shift[b,c])           (scale = gamma * rstd, shift = beta - mean * gamma * rstd; NULL = 1 / 0)
//   backward  g = gy * act'(x * scale + shift);   sums[b,c] = {sum g, sum g * x}    (-> d beta, d gamma, the mean terms of dx)
//             gx = g * ca[b,c] + x * cb[b,c] + cc[b,c]
// Which statistics feed the coefficients (per sample / per batch / running) is the caller's arithmetic on [B,C] arrays
// (uegan_amd/ops.py: NormAct); the pre-activation is recomputed from x, never stored.
// ----------------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void affine_act_fwd_kernel(const T* x, T* y, const float* scale, const float* shift, int act, RedPlan p) {
  RED_THREAD_SETUP();
  if (!cvalid) return;
  float sc[V], sf[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    sc[e] = scale ? scale[(size_t)b * p.C + c0 + e] : 1.f;
    sf[e] = shift ? shift[(size_t)b * p.C + c0 + e] : 0.f;
  }
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float v[V];
    Vec<T, V>::ld(x + base + (size_t)q * p.C, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = act_of_pre(v[e] * sc[e] + sf[e], act);
    Vec<T, V>::st(y + base + (size_t)q * p.C, v);
  }
}

template <typename T, int V>
__global__ void affine_act_bwd_partial_kernel(const T* gy, const T* x, const float* scale, const float* shift, int act, float* part, RedPlan p) {
  __shared__ float sh[2][V][256];
  RED_THREAD_SETUP();
  float a0[V], a1[V], sc[V], sf[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    a0[e] = 0.f; a1[e] = 0.f;
    sc[e] = (scale && cvalid) ? scale[(size_t)b * p.C + c0 + e] : 1.f;
    sf[e] = (shift && cvalid) ? shift[(size_t)b * p.C + c0 + e] : 0.f;
  }
  if (cvalid) {
    _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
      float gv[V], xv[V];
      Vec<T, V>::ld(gy + base + (size_t)q * p.C, gv);
      Vec<T, V>::ld(x + base + (size_t)q * p.C, xv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float g = gv[e] * act_grad_of_pre(xv[e] * sc[e] + sf[e], act);
        a0[e] += g; a1[e] += g * xv[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] = a0[e]; sh[1][e][threadIdx.x] = a1[e]; }
  __syncthreads();
  for (int half = p.PL >> 1; half > 0; half >>= 1) {
    if (pl < half) {
      const int o = threadIdx.x + half * p.CG;
#pragma unroll
      for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] += sh[0][e][o]; sh[1][e][threadIdx.x] += sh[1][e][o]; }
    }
    __syncthreads();
  }
  if (pl == 0 && cvalid) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float* o = part + (((size_t)b * p.S + s) * p.C + c0 + e) * 2;
      o[0] = sh[0][e][threadIdx.x]; o[1] = sh[1][e][threadIdx.x];
    }
  }
}

template <typename T, int V>
__global__ void affine_act_bwd_apply_kernel(const T* gy, const T* x, const float* scale, const float* shift, int act, const float* ca,
                                            const float* cb, const float* cc, T* gx, RedPlan p) {
  RED_THREAD_SETUP();
  if (!cvalid) return;
  float sc[V], sf[V], ka[V], kb[V], kc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const size_t i = (size_t)b * p.C + c0 + e;
    sc[e] = scale ? scale[i] : 1.f; sf[e] = shift ? shift[i] : 0.f;
    ka[e] = ca ? ca[i] : 1.f; kb[e] = cb ? cb[i] : 0.f; kc[e] = cc ? cc[i] : 0.f;
  }
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float gv[V], xv[V];
    Vec<T, V>::ld(gy + base + (size_t)q * p.C, gv);
    Vec<T, V>::ld(x + base + (size_t)q * p.C, xv);
#pragma unroll
    for (int e = 0; e < V; ++e) gv[e] = gv[e] * act_grad_of_pre(xv[e] * sc[e] + sf[e], act) * ka[e] + xv[e] * kb[e] + kc[e];
    Vec<T, V>::st(gx + base + (size_t)q * p.C, gv);
  }
}

// ----------------------------------------------------------------------------------------------------
// perceptual tap: weight * MSE(IN(x), IN(y)) and its gradient w.r.t. x
// ----------------------------------------------------------------------------------------------------
// sums over the block's pixel range, per (b,c): {sum (xh-yh)^2, sum (xh-yh), sum (xh-yh)*xh}
template <typename T, int V>
__global__ void percep_sums_kernel(const T* x, const T* y, const float* st, float* sums, RedPlan p) {
  __shared__ float sh[3][V][256];
  RED_THREAD_SETUP();
  float a0[V], a1[V], a2[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { a0[e] = 0.f; a1[e] = 0.f; a2[e] = 0.f; }
  if (cvalid) {
    // st = [mean_x | rstd_x | mean_y | rstd_y], each B*C
    const size_t bc = (size_t)p.B * p.C, o0 = (size_t)b * p.C + c0;
    float mx[V], rx[V], my[V], ry[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      mx[e] = st[o0 + e]; rx[e] = st[bc + o0 + e]; my[e] = st[2 * bc + o0 + e]; ry[e] = st[3 * bc + o0 + e];
    }
    _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
      float xv[V], yv[V];
      Vec<T, V>::ld(x + base + (size_t)q * p.C, xv);
      Vec<T, V>::ld(y + base + (size_t)q * p.C, yv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xh = (xv[e] - mx[e]) * rx[e], yh = (yv[e] - my[e]) * ry[e];
        const float d = xh - yh;
        a0[e] += d * d;
        a1[e] += d;
        a2[e] += d * xh;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] = a0[e]; sh[1][e][threadIdx.x] = a1[e]; sh[2][e][threadIdx.x] = a2[e]; }
  __syncthreads();
  for (int half = p.PL >> 1; half > 0; half >>= 1) {        // tree over the pixel lanes
    if (pl < half) {
      const int o = threadIdx.x + half * p.CG;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        sh[0][e][threadIdx.x] += sh[0][e][o]; sh[1][e][threadIdx.x] += sh[1][e][o]; sh[2][e][threadIdx.x] += sh[2][e][o];
      }
    }
    __syncthreads();
  }
  if (pl == 0 && cvalid) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float* o = sums + (((size_t)b * p.S + s) * p.C + c0 + e) * 3;
      o[0] = sh[0][e][threadIdx.x]; o[1] = sh[1][e][threadIdx.x]; o[2] = sh[2][e][threadIdx.x];
    }
  }
}

// loss += weight * sum_{b,c} sum (xh-yh)^2 / nel   (ONE block: a fixed summation order; the taps add up in launch order)
__global__ void percep_loss_kernel(const float* tot, float weight, float* loss, RedPlan p) {
  __shared__ float red[16];
  const int total = p.B * p.C;
  float acc = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) acc += tot[(size_t)i * 3];
  acc = block_sum(acc, red);
  const float nel = (float)p.B * (float)p.HW * (float)p.C;
  if (threadIdx.x == 0) *loss += weight * acc / nel;
}

// gx = gscale * d(weight * MSE(IN(x), IN(y)))/dx
template <typename T, int V, bool RELU, bool ACC = false>      // RELU: the act argument is UEGAN_ACT_RELU (the only one the model uses), resolved at compile time
__global__ void percep_grad_kernel(const T* x, const T* y, const float* st, const float* tot, float weight, const float* gscale, T* gx,
                                   RedPlan p, int act) {       // ACC: gx += ... (the tap has a second consumer whose gradient is already in gx)
  RED_THREAD_SETUP();
  if (!cvalid) return;
  // (the formula lives in common.h: conv_tall_kernel's tap epilogue evaluates the same one, bit for bit)
  float k, inv_n;
  percep_scalars(weight, gscale, p.B, p.HW, p.C, k, inv_n);
  const size_t bc = (size_t)p.B * p.C, o0 = (size_t)b * p.C + c0;
  float mx[V], rx[V], my[V], ry[V], mg[V], mgx[V];
#pragma unroll
  for (int e = 0; e < V; ++e) percep_consts(st, tot, bc, o0 + e, k, inv_n, mx[e], rx[e], my[e], ry[e], mg[e], mgx[e]);
  _Pragma("unroll 4") for (int q = p0 + pl; q < p1; q += p.PL) {
    float xv[V], yv[V];
    Vec<T, V>::ld(x + base + (size_t)q * p.C, xv);
    Vec<T, V>::ld(y + base + (size_t)q * p.C, yv);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float gv = percep_tap_grad(xv[e], yv[e], mx[e], rx[e], my[e], ry[e], k, mg[e], mgx[e]);
      xv[e] = RELU ? (xv[e] > 0.f ? gv : 0.f) : gv * act_grad_from_out(xv[e], act);      // (act: x's producer's deferred act')
    }
    if (ACC) {
      float pv[V];
      Vec<T, V>::ld(gx + base + (size_t)q * p.C, pv);
#pragma unroll
      for (int e = 0; e < V; ++e) xv[e] += pv[e];
    }
    Vec<T, V>::st(gx + base + (size_t)q * p.C, xv);
  }
}

// ----------------------------------------------------------------------------------------------------
// Moments over a WINDOW of an NHWC map, accumulated across calls: tiled inference collects the attention modules' whole-image moments tile by tile
// (each tile contributes the window it owns).  Per (image, channel) the running sum z and sum z^2 live in DOUBLE: z and z^2 are exact there (24-bit
// significands), so the sums carry ~n * 2^-53 relative error and E[z^2] - E[z]^2 loses nothing that matters against the fp32 one-pass moments above.
// Same thread layout as RedPlan (CG channel lanes x PL pixel lanes, V channels per thread); a block owns one of S splits of the window's pixels,
// which it reads in place through the map's row pitch.  No atomics: window_fold_kernel adds the S partials of a (b, c) in split order.
// ----------------------------------------------------------------------------------------------------
constexpr int WINDOW_MAX_SPLITS = 512;      // grid cap in x; the workspace is sized by it (uegan_moments_window_workspace_bytes)
constexpr int WINDOW_PIX_PER_LANE = 4;      // a split is at least this many pixels per pixel lane
struct WinPlan {
  int B, H, W, C;
  int y0, x0, wh, ww;      // window origin and extent
  int V, CG, PL, ncg;      // as RedPlan
  int S, chunk;            // pixel splits of the wh * ww window pixels, pixels per split
  dim3 grid() const { return dim3(S, ncg, B); }
};
static WinPlan make_win_plan(int B, int H, int W, int C, int y0, int y1, int x0, int x1, int dtype, bool aligned) {
  const int epc = epc_of(dtype);
  WinPlan p;
  p.B = B; p.H = H; p.W = W; p.C = C; p.y0 = y0; p.x0 = x0; p.wh = y1 - y0; p.ww = x1 - x0;
  p.V = (C % epc == 0 && aligned) ? epc : 1;
  const int lanes = C / p.V;
  int cg = 1;
  while (cg < lanes && cg < 64) cg <<= 1;
  p.CG = cg;
  p.PL = 256 / cg;
  p.ncg = (lanes + cg - 1) / cg;
  const size_t n = (size_t)p.wh * p.ww;
  const int s = blocks_for(n, WINDOW_PIX_PER_LANE * p.PL, WINDOW_MAX_SPLITS);
  p.chunk = (int)((n + s - 1) / s);
  p.S = (int)((n + p.chunk - 1) / p.chunk);
  return p;
}

// part[((b*S + s)*C + c)*2 + {0,1}] = {sum z, sum z^2} over split s of the window;  PAIR: z = x + x_lo (a hi + lo pair of 16-bit planes)
template <typename T, int V, bool PAIR>
__global__ void window_partial_kernel(const T* x, const T* xl, double* part, WinPlan p) {
  __shared__ double sh[2][V][256];
  const int s = blockIdx.x, cg = blockIdx.y, b = blockIdx.z;
  const int cl = threadIdx.x % p.CG, pl = threadIdx.x / p.CG;
  const int c0 = (cg * p.CG + cl) * V;
  const bool cvalid = c0 < p.C;
  const int n = p.wh * p.ww, q0 = s * p.chunk;
  const int q1 = q0 + p.chunk < n ? q0 + p.chunk : n;
  double a0[V], a1[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { a0[e] = 0.0; a1[e] = 0.0; }
  if (cvalid) {
    for (int q = q0 + pl; q < q1; q += p.PL) {
      const int r = q / p.ww, col = q - r * p.ww;
      const size_t o = (((size_t)b * p.H + p.y0 + r) * p.W + p.x0 + col) * p.C + c0;
      float v[V];
      Vec<T, V>::ld(x + o, v);
      if (PAIR) {
        float l[V];
        Vec<T, V>::ld(xl + o, l);
#pragma unroll
        for (int e = 0; e < V; ++e) { const double z = (double)v[e] + (double)l[e]; a0[e] += z; a1[e] += z * z; }
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) { const double z = (double)v[e]; a0[e] += z; a1[e] += z * z; }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] = a0[e]; sh[1][e][threadIdx.x] = a1[e]; }
  __syncthreads();
  for (int half = p.PL >> 1; half > 0; half >>= 1) {        // tree over the pixel lanes (PL is a power of two): a fixed order
    if (pl < half) {
      const int o = threadIdx.x + half * p.CG;
#pragma unroll
      for (int e = 0; e < V; ++e) { sh[0][e][threadIdx.x] += sh[0][e][o]; sh[1][e][threadIdx.x] += sh[1][e][o]; }
    }
    __syncthreads();
  }
  if (pl == 0 && cvalid) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      double* o = part + (((size_t)b * p.S + s) * p.C + c0 + e) * 2;
      o[0] = sh[0][e][threadIdx.x]; o[1] = sh[1][e][threadIdx.x];
    }
  }
}
// sum[b*C + c] += the S partials of (b, c) in split order, sumsq likewise: one thread per (b, c)
__global__ void window_fold_kernel(const double* part, double* sum, double* sumsq, int B, int S, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  double t0 = 0.0, t1 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* o = part + (((size_t)b * S + s) * C + c) * 2;
    t0 += o[0];
    t1 += o[1];
  }
  sum[i] += t0;
  sumsq[i] += t1;
}
// accumulators -> mean, rstd = 1 / sqrt(var + eps) (biased variance; eps < 0: the variance itself), evaluated in double and rounded once
__global__ void window_finish_kernel(const double* sum, const double* sumsq, double count, float eps, float* mean, float* rstd, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m = sum[i] / count;
  double var = sumsq[i] / count - m * m;
  if (var < 0.0) var = 0.0;
  mean[i] = (float)m;
  rstd[i] = eps < 0.f ? (float)var : (float)(1.0 / sqrt(var + (double)eps));
}

}  // namespace uegan

using namespace uegan;

// launches a RedPlan kernel -- KERNEL names the instance in terms of T and V, e.g. (moments_partial_kernel<T, V>) -- on the plan's grid and
// checks the launch, so that an entry point reads as its sequence of passes
#define RED_LAUNCH(KERNEL, dtype, PLAN, stream, ...)                                                                      \
  do {                                                                                                                    \
    UEGAN_DISPATCH_TV(dtype, (PLAN).V != 1, hipLaunchKernelGGL(KERNEL, (PLAN).grid(), dim3(256), 0, stream, __VA_ARGS__)); \
    UEGAN_CHECK_LAUNCH();                                                                                                 \
  } while (0)

// the finalize passes over the split partials: one wave per (b, c, k), 4 per 256-thread block
static inline int bc_blocks(const RedPlan& p, int K) { return (p.B * p.C * K + 3) / 4; }
static int finalize_moments(const RedPlan& p, const float* part, float* mean, float* rstd, float eps, hipStream_t s) {
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(bc_blocks(p, 1)), dim3(256), 0, s, part, mean, rstd, p, eps);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
static int finalize_sums(const RedPlan& p, const float* part, float* out, int K, hipStream_t s) {
  hipLaunchKernelGGL(sums_finalize_kernel, dim3(bc_blocks(p, K)), dim3(256), 0, s, part, out, p, K);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// scratch per reduction pass: split partials (3 per (b,s,c)) + 8 floats per (b,c) for finalized statistics / totals
extern "C" size_t uegan_reduce_workspace_floats(int B, int HW, int C) {
  const RedPlan p4 = make_plan(B, HW, C, UEGAN_F32), p8 = make_plan(B, HW, C, UEGAN_BF16);      // (the split count depends on the storage type's chunk width)
  const int S = p4.S > p8.S ? p4.S : p8.S;
  return (size_t)B * S * C * 3 + (size_t)B * C * 8;
}

extern "C" int uegan_instnorm_fwd(int dtype, const void* x, void* y, float* mean, float* rstd, float* tmp, int B, int HW, int C, float eps,
                                  uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && mean && rstd && tmp && B > 0 && HW > 0 && C > 0, "bad instnorm args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  hipStream_t s = (hipStream_t)stream;
  RED_LAUNCH((moments_partial_kernel<T, V>), dtype, p, s, (const T*)x, tmp, p);
  if (int rc = finalize_moments(p, tmp, mean, rstd, eps, s)) return rc;
  RED_LAUNCH((instnorm_apply_kernel<T, V>), dtype, p, s, (const T*)x, (T*)y, mean, rstd, p);
  return UEGAN_OK;
}

extern "C" int uegan_instnorm_apply(int dtype, const void* x, void* y, const float* mean, const float* rstd, int B, int HW, int C, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && mean && rstd && B > 0 && HW > 0 && C > 0, "bad instnorm args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  RED_LAUNCH((instnorm_apply_kernel<T, V>), dtype, p, (hipStream_t)stream, (const T*)x, (T*)y, mean, rstd, p);
  return UEGAN_OK;
}

extern "C" int uegan_instnorm_apply_pair(int dtype, const void* x, const void* x_lo, void* y, void* y_lo, const float* mean, const float* rstd, int B, int HW,
                                         int C, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && x_lo && y && y_lo && mean && rstd && B > 0 && HW > 0 && C > 0, "bad instnorm args");
  UEGAN_CHECK_ARG(dtype == UEGAN_BF16, "hi + lo pairs exist for the 16-bit storage format");
  const RedPlan p = make_plan(B, HW, C, dtype);
  using T = bf16_t;      // (the only storage type the pair kernel is built for)
  UEGAN_DISPATCH_BOOL(p.V != 1, VEC, hipLaunchKernelGGL((instnorm_apply_pair_kernel<T, VEC ? 8 : 1>), p.grid(), dim3(256), 0, (hipStream_t)stream,
                                                        (const T*)x, (const T*)x_lo, (T*)y, (T*)y_lo, mean, rstd, p));
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// the two sums of the InstanceNorm backward, {sum dy, sum dy*y} per (image, channel): tot[(b*C + c)*2 + {0,1}] inside tmp (gam_bwd.hip's first two launches too)
int uegan::instnorm_bwd_sums(int dtype, const void* dy, const void* y, float* tmp, int B, int HW, int C, hipStream_t s, const float** tot_out) {
  const RedPlan p = make_plan(B, HW, C, dtype);
  float* tot = tmp + (size_t)B * p.S * C * 3;
  RED_LAUNCH((instnorm_bwd_partial_kernel<T, V>), dtype, p, s, (const T*)dy, (const T*)y, tmp, p);
  if (int rc = finalize_sums(p, tmp, tot, 2, s)) return rc;
  *tot_out = tot;
  return UEGAN_OK;
}

extern "C" int uegan_instnorm_bwd(int dtype, const void* dy, const void* y, const float* rstd, void* dx, float* tmp, int B, int HW, int C,
                                  uegan_stream_t stream) {
  UEGAN_CHECK_ARG(dy && y && rstd && dx && tmp && B > 0 && HW > 0 && C > 0, "bad instnorm args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  hipStream_t s = (hipStream_t)stream;
  const float* tot = nullptr;
  if (int rc = instnorm_bwd_sums(dtype, dy, y, tmp, B, HW, C, s, &tot)) return rc;
  RED_LAUNCH((instnorm_bwd_apply_kernel<T, V>), dtype, p, s, (const T*)dy, (const T*)y, rstd, tot, (T*)dx, p);
  return UEGAN_OK;
}

extern "C" int uegan_moments(int dtype, const void* x, float* mean, float* var, float* tmp, int B, int HW, int C, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && mean && var && tmp && B > 0 && HW > 0 && C > 0, "bad moments args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  hipStream_t s = (hipStream_t)stream;
  RED_LAUNCH((moments_partial_kernel<T, V>), dtype, p, s, (const T*)x, tmp, p);
  return finalize_moments(p, tmp, mean, var, -1.f, s);
}

extern "C" size_t uegan_moments_window_workspace_bytes(int B, int C) {
  return (size_t)(B > 0 ? B : 0) * (size_t)(C > 0 ? C : 0) * WINDOW_MAX_SPLITS * 2 * sizeof(double);
}

extern "C" int uegan_moments_window_acc(int dtype, const void* x, const void* x_lo, int B, int H, int W, int C, int y0, int y1, int x0, int x1,
                                        double* sum, double* sumsq, void* tmp, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && sum && sumsq && tmp && B > 0 && H > 0 && W > 0 && C > 0, "bad moments_window args");
  UEGAN_CHECK_ARG(0 <= y0 && y0 < y1 && y1 <= H && 0 <= x0 && x0 < x1 && x1 <= W, "moments_window: rows [%d, %d) x columns [%d, %d) is no window of a %d x %d map",
                  y0, y1, x0, x1, H, W);
  UEGAN_CHECK_ARG((long long)(y1 - y0) * (x1 - x0) < (1LL << 31) - 1024 && B <= 65535, "moments_window: window too large");
  UEGAN_CHECK_ARG(!x_lo || dtype == UEGAN_BF16, "hi + lo pairs exist for the 16-bit storage format");
  UEGAN_CHECK_ARG((uintptr_t)tmp % 8 == 0 && (uintptr_t)sum % 8 == 0 && (uintptr_t)sumsq % 8 == 0, "moments_window: 8-byte alignment");
  const bool aligned = (uintptr_t)x % 16 == 0 && (uintptr_t)x_lo % 16 == 0;
  const WinPlan p = make_win_plan(B, H, W, C, y0, y1, x0, x1, dtype, aligned);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)tmp;
  UEGAN_DISPATCH_BOOL(x_lo != nullptr, PAIR, UEGAN_DISPATCH_TV(dtype, p.V != 1,
      hipLaunchKernelGGL((window_partial_kernel<T, V, PAIR>), p.grid(), dim3(256), 0, s, (const T*)x, (const T*)x_lo, part, p)));
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(window_fold_kernel, dim3(grid_for((size_t)B * C)), dim3(256), 0, s, part, sum, sumsq, B, p.S, C);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_moments_finish(const double* sum, const double* sumsq, double count, float eps, float* mean, float* rstd, int n, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(sum && sumsq && mean && rstd && n > 0 && count >= 1.0, "bad moments_finish args");
  hipLaunchKernelGGL(window_finish_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, sum, sumsq, count, eps, mean, rstd, n);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_affine_act_fwd(int dtype, int act, const void* x, const float* scale, const float* shift, void* y, int B, int HW, int C,
                                    uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && B > 0 && HW > 0 && C > 0 && act >= UEGAN_ACT_NONE && act <= UEGAN_ACT_SELU, "bad affine_act args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  RED_LAUNCH((affine_act_fwd_kernel<T, V>), dtype, p, (hipStream_t)stream, (const T*)x, (T*)y, scale, shift, act, p);
  return UEGAN_OK;
}

extern "C" int uegan_affine_act_bwd_sums(int dtype, int act, const void* gy, const void* x, const float* scale, const float* shift, float* sums,
                                         float* tmp, int B, int HW, int C, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(gy && x && sums && tmp && B > 0 && HW > 0 && C > 0 && act >= UEGAN_ACT_NONE && act <= UEGAN_ACT_SELU, "bad affine_act args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  hipStream_t s = (hipStream_t)stream;
  RED_LAUNCH((affine_act_bwd_partial_kernel<T, V>), dtype, p, s, (const T*)gy, (const T*)x, scale, shift, act, tmp, p);
  return finalize_sums(p, tmp, sums, 2, s);
}

extern "C" int uegan_affine_act_bwd_apply(int dtype, int act, const void* gy, const void* x, const float* scale, const float* shift,
                                          const float* ca, const float* cb, const float* cc, void* gx, int B, int HW, int C, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(gy && x && gx && B > 0 && HW > 0 && C > 0 && act >= UEGAN_ACT_NONE && act <= UEGAN_ACT_SELU, "bad affine_act args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  RED_LAUNCH((affine_act_bwd_apply_kernel<T, V>), dtype, p, (hipStream_t)stream, (const T*)gy, (const T*)x, scale, shift, act, ca, cb, cc, (T*)gx, p);
  return UEGAN_OK;
}

// percep scratch (3 reduction workspaces): region 0 = x partials + [mean_x|rstd_x|mean_y|rstd_y] (4*B*C in its 8*B*C tail),
// region 1 = y partials, region 2 = sum partials + totals (3*B*C in its tail)
struct PercepScratch {
  float *px, *py, *sums, *st, *tot;
};
static PercepScratch percep_layout(const RedPlan& p, float* tmp) {
  const size_t part = (size_t)p.B * p.S * p.C * 3, region = part + (size_t)p.B * p.C * 8;
  return {tmp, tmp + region, tmp + 2 * region, tmp + part, tmp + 2 * region + part};
}
// where the backward's constants sit in a tap's scratch (conv.hip: uegan_conv2d_dgrad_act_tap hands them to conv_tall_kernel's tap epilogue)
void uegan::percep_tap_consts(int dtype, const float* tmp, int B, int HW, int C, const float** st, const float** tot) {
  const PercepScratch w = percep_layout(make_plan(B, HW, C, dtype), const_cast<float*>(tmp));
  *st = w.st;
  *tot = w.tot;
}

// the tail of both forward forms, from the statistics in w.st: the three sums per (image, channel), their totals, the loss term
static int percep_finish(int dtype, const RedPlan& p, const PercepScratch& w, const void* x, const void* y, float weight, float* loss, hipStream_t s) {
  RED_LAUNCH((percep_sums_kernel<T, V>), dtype, p, s, (const T*)x, (const T*)y, w.st, w.sums, p);
  if (int rc = finalize_sums(p, w.sums, w.tot, 3, s)) return rc;
  hipLaunchKernelGGL(percep_loss_kernel, dim3(1), dim3(1024), 0, s, w.tot, weight, loss, p);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_percep_tap_fwd(int dtype, const void* x, const void* y, float weight, float* loss, float* tmp, int B, int HW, int C,
                                    float eps, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && loss && tmp && B > 0 && HW > 0 && C > 0, "bad percep args");
  const RedPlan p = make_plan(B, HW, C, dtype);
  const PercepScratch w = percep_layout(p, tmp);
  hipStream_t s = (hipStream_t)stream;
  const size_t bc = (size_t)B * C;
  RED_LAUNCH((moments_partial_kernel<T, V>), dtype, p, s, (const T*)x, w.px, p);
  RED_LAUNCH((moments_partial_kernel<T, V>), dtype, p, s, (const T*)y, w.py, p);
  if (int rc = finalize_moments(p, w.px, w.st, w.st + bc, eps, s)) return rc;
  if (int rc = finalize_moments(p, w.py, w.st + 2 * bc, w.st + 3 * bc, eps, s)) return rc;
  return percep_finish(dtype, p, w, x, y, weight, loss, s);
}

// ... with the InstanceNorm moments of both taps GIVEN (uegan_conv2d_fwd_stats emitted them from the tap conv's epilogue: VGG conv1_1, the 1-GB
// tap): the four moment launches become one copy of [mean_x | rstd_x | mean_y | rstd_y] into the scratch the backward reads them from
__global__ void percep_stats_copy_kernel(const float* mx, const float* rx, const float* my, const float* ry, float* st, int bc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * bc) return;
  const int k = i / bc, j = i - k * bc;
  st[i] = k == 0 ? mx[j] : (k == 1 ? rx[j] : (k == 2 ? my[j] : ry[j]));
}
extern "C" int uegan_percep_tap_fwd_given(int dtype, const void* x, const void* y, float weight, float* loss, float* tmp, int B, int HW, int C,
                                          const float* mean_x, const float* rstd_x, const float* mean_y, const float* rstd_y, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && loss && tmp && mean_x && rstd_x && mean_y && rstd_y && B > 0 && HW > 0 && C > 0, "bad percep args");
  UEGAN_CHECK_ARG(dtype == UEGAN_F32 || dtype == UEGAN_BF16, "bad dtype %d", dtype);      // (before the copy, which no dispatch guards)
  const RedPlan p = make_plan(B, HW, C, dtype);
  const PercepScratch w = percep_layout(p, tmp);
  hipStream_t s = (hipStream_t)stream;
  const int bc = B * C;
  hipLaunchKernelGGL(percep_stats_copy_kernel, dim3((4 * bc + 255) / 256), dim3(256), 0, s, mean_x, rstd_x, mean_y, rstd_y, w.st, bc);
  UEGAN_CHECK_LAUNCH();
  return percep_finish(dtype, p, w, x, y, weight, loss, s);
}

extern "C" int uegan_percep_tap_bwd(int dtype, const void* x, const void* y, float weight, const float* gscale, void* gx, const float* tmp,
                                    int B, int HW, int C, float eps, uegan_stream_t stream) {
  return uegan_percep_tap_bwd_act(dtype, UEGAN_ACT_NONE, x, y, weight, gscale, gx, tmp, B, HW, C, eps, stream);
}
extern "C" int uegan_percep_tap_bwd_act(int dtype, int act, const void* x, const void* y, float weight, const float* gscale, void* gx,
                                        const float* tmp, int B, int HW, int C, float eps, uegan_stream_t stream) {
  return uegan_percep_tap_bwd_acc(dtype, act, x, y, weight, gscale, gx, tmp, B, HW, C, eps, 0, stream);
}
extern "C" int uegan_percep_tap_bwd_acc(int dtype, int act, const void* x, const void* y, float weight, const float* gscale, void* gx,
                                        const float* tmp, int B, int HW, int C, float eps, int accumulate, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(x && y && gx && tmp && B > 0 && HW > 0 && C > 0, "bad percep args");
  (void)eps;
  const RedPlan p = make_plan(B, HW, C, dtype);
  const PercepScratch w = percep_layout(p, const_cast<float*>(tmp));
  UEGAN_DISPATCH_BOOL(act == UEGAN_ACT_RELU, RELU, UEGAN_DISPATCH_BOOL(accumulate != 0, ACC,
      RED_LAUNCH((percep_grad_kernel<T, V, RELU, ACC>), dtype, p, (hipStream_t)stream, (const T*)x, (const T*)y, w.st, w.tot, weight, gscale, (T*)gx, p, act)));
  return UEGAN_OK;
}
