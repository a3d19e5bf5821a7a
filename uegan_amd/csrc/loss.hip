// The adversarial and reconstruction losses, on flat prediction lists and on the prediction-head maps of a batched discriminator pass:
// relativistic average hinge / least squares (rahinge, rals), the one-list terms of the other GANLoss modes (pred_loss), the head-map form
// of the relativistic hinge (rahinge_heads) and the multiscale reconstruction loss (msrec).  Every multi-block reduction stores one fp32
// partial per block and its consumer adds the partials in a fixed order, so a result is a function of the block count alone; the caps
// on the block counts (RB, MSREC_MAXB, 256, 1024) size the workspaces.  The per-(image, channel) reductions are in norm.hip.
//
// Reference arithmetic: GANLoss 'rahinge' (losses.py:348-362, 393-409) and its other modes (losses.py:312-392),
// MultiscaleRecLoss (losses.py:202-231).
#include "common.h"
#include "launch.h"

namespace uegan {

// ----------------------------------------------------------------------------------------------------
// relativistic average hinge (losses.py:348-362), all scales in one launch per stage
// ----------------------------------------------------------------------------------------------------
// Deterministic reductions: a multi-block reduction stage stores ONE partial sum per block and quantity (grid.x <= RB) and its consumer --
// the next kernel of the chain -- adds the partials in a fixed order (a 64-lane butterfly), so the result does not depend on the order
// in which the blocks ran (a float atomicAdd per block did, at rounding level, and the relativistic means feed the gradient).
constexpr int RB = 64;
// sum of the nb (<= 64) block partials of one quantity: call from ONE whole wave, result in every lane
__device__ __forceinline__ float fold_partials(const float* part, int nb) {
  const int lane = threadIdx.x & 63;
  return wave_sum(lane < nb ? part[lane] : 0.f);
}

struct RaArgs {
  const float* real[8];
  const float* fake[8];
  float* greal[8];
  float* gfake[8];
  long long n[8];
  float* tmp;     // [nscales][8]: {sum r, sum f, sum A, sum B, cnt A, cnt B, -, -}, then the block partials [nscales][6][RB]
  float* loss;
  int nscales, nbx;      // nbx: blocks (partials) per scale of the reduction stages
  float sgn;      // +1 discriminator, -1 generator
};
__device__ __forceinline__ float* ra_part(const RaArgs& a, int sc, int q) { return a.tmp + 8 * a.nscales + (sc * 6 + q) * RB; }
// the two means of a scale from the partials of rahinge_means_kernel (waves 0 / 1 fold one each); block x == 0 also files them in the slots
__device__ __forceinline__ void ra_fold_means(const RaArgs& a, int sc, float* sh, float& rsum, float& fsum) {
  const int wv = threadIdx.x >> 6;
  if (wv < 2) {
    const float v = fold_partials(ra_part(a, sc, wv), a.nbx);
    if ((threadIdx.x & 63) == 0) {
      sh[wv] = v;
      if (blockIdx.x == 0) a.tmp[sc * 8 + wv] = v;
    }
  }
  __syncthreads();
  rsum = sh[0]; fsum = sh[1];
  __syncthreads();
}

__global__ void rahinge_means_kernel(RaArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  float sr = 0.f, sf = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    sr += a.real[sc][i];
    sf += a.fake[sc][i];
  }
  sr = block_sum(sr, red);
  sf = block_sum(sf, red);
  if (threadIdx.x == 0) {
    ra_part(a, sc, 0)[blockIdx.x] = sr;
    ra_part(a, sc, 1)[blockIdx.x] = sf;
  }
}

__global__ void rahinge_terms_kernel(RaArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  float rsum, fsum;
  ra_fold_means(a, sc, red, rsum, fsum);
  const float rbar = rsum / (float)n, fbar = fsum / (float)n;
  float sa = 0.f, sb = 0.f, ca = 0.f, cb = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float A = 1.f - a.sgn * (a.real[sc][i] - fbar);
    const float Bv = 1.f + a.sgn * (a.fake[sc][i] - rbar);
    if (A > 0.f) { sa += A; ca += 1.f; }
    if (Bv > 0.f) { sb += Bv; cb += 1.f; }
  }
  sa = block_sum(sa, red);
  sb = block_sum(sb, red);
  ca = block_sum(ca, red);
  cb = block_sum(cb, red);
  if (threadIdx.x == 0) {
    ra_part(a, sc, 2)[blockIdx.x] = sa;
    ra_part(a, sc, 3)[blockIdx.x] = sb;
    ra_part(a, sc, 4)[blockIdx.x] = ca;
    ra_part(a, sc, 5)[blockIdx.x] = cb;
  }
}

// one wave: folds the term partials of every scale into the slots (the gradient kernels read them there) and adds up the loss
__global__ void rahinge_loss_kernel(RaArgs a) {
  float L = 0.f;
  for (int k = 0; k < a.nscales; ++k) {
    const float nk = (float)a.n[k];
    float t[4];
    for (int q = 0; q < 4; ++q) {
      t[q] = fold_partials(ra_part(a, k, 2 + q), a.nbx);
      if (threadIdx.x == 0) a.tmp[k * 8 + 2 + q] = t[q];
    }
    L += 0.5f * (t[0] / nk + t[1] / nk);
  }
  if (threadIdx.x == 0) *a.loss = L;
}

// d loss / d real_i = -(sgn/2n) (1[A_i>0] + cntB/n) ; d loss / d fake_j = (sgn/2n) (1[B_j>0] + cntA/n), times gscale
__global__ void rahinge_grad_kernel(RaArgs a, const float* gscale) {
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  const float fn = (float)n;
  const float rbar = a.tmp[sc * 8 + 0] / fn, fbar = a.tmp[sc * 8 + 1] / fn;
  const float ca = a.tmp[sc * 8 + 4] / fn, cb = a.tmp[sc * 8 + 5] / fn;
  const float k = a.sgn * 0.5f / fn * (gscale ? *gscale : 1.f);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (a.greal[sc]) {
      const float A = 1.f - a.sgn * (a.real[sc][i] - fbar);
      a.greal[sc][i] = -k * ((A > 0.f ? 1.f : 0.f) + cb);
    }
    if (a.gfake[sc]) {
      const float Bv = 1.f + a.sgn * (a.fake[sc][i] - rbar);
      a.gfake[sc][i] = k * ((Bv > 0.f ? 1.f : 0.f) + ca);
    }
  }
}

// ----------------------------------------------------------------------------------------------------
// The other adversarial losses of GANLoss.loss (losses.py:312-392).  'rals' (relativistic average least squares, :363-376) shares
// the two-stage shape of 'rahinge' (means, then terms); the non-relativistic modes ('original' :313-323, 'ls' :324-332, 'hinge'
// :333-347, the wgan fallback :378-392) are a mean of an elementwise function of ONE prediction list.
// ----------------------------------------------------------------------------------------------------
// A_i = (r_i - fbar) - sgn, B_j = (f_j - rbar) + sgn; loss = sum_scales (mean A^2 + mean B^2) / 2
__global__ void rals_terms_kernel(RaArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  float rsum, fsum;
  ra_fold_means(a, sc, red, rsum, fsum);
  const float rbar = rsum / (float)n, fbar = fsum / (float)n;
  float sa = 0.f, sb = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float A = a.real[sc][i] - fbar - a.sgn;
    const float Bv = a.fake[sc][i] - rbar + a.sgn;
    sa += A * A;
    sb += Bv * Bv;
  }
  sa = block_sum(sa, red);
  sb = block_sum(sb, red);
  if (threadIdx.x == 0) {
    ra_part(a, sc, 2)[blockIdx.x] = sa;
    ra_part(a, sc, 3)[blockIdx.x] = sb;
    ra_part(a, sc, 4)[blockIdx.x] = 0.f;      // (the shared loss kernel folds four quantities)
    ra_part(a, sc, 5)[blockIdx.x] = 0.f;
  }
}
// d loss / d r_i = (A_i - mean B) / n,  d loss / d f_j = (B_j - mean A) / n   (mean A = rbar - fbar - sgn, mean B = fbar - rbar + sgn)
__global__ void rals_grad_kernel(RaArgs a, const float* gscale) {
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  const float fn = (float)n;
  const float rbar = a.tmp[sc * 8 + 0] / fn, fbar = a.tmp[sc * 8 + 1] / fn;
  const float ma = rbar - fbar - a.sgn, mb = fbar - rbar + a.sgn;
  const float k = (gscale ? *gscale : 1.f) / fn;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (a.greal[sc]) a.greal[sc][i] = k * ((a.real[sc][i] - fbar - a.sgn) - mb);
    if (a.gfake[sc]) a.gfake[sc][i] = k * ((a.fake[sc][i] - rbar + a.sgn) - ma);
  }
}

struct PredArgs {
  const float* p[8];
  float* g[8];
  long long n[8];
  float* tmp;      // [nscales][RB] block partials
  float* loss;
  int nscales, fid, nbx;
  float target;
};
__device__ __forceinline__ float pred_term(float p, int fid, float t) {
  switch (fid) {
    case UEGAN_PRED_BCE: return fmaxf(p, 0.f) - p * t + log1pf(expf(-fabsf(p)));      // binary_cross_entropy_with_logits
    case UEGAN_PRED_LS: return (p - t) * (p - t);
    case UEGAN_PRED_HINGE_REAL: return -fminf(p - 1.f, 0.f);
    case UEGAN_PRED_HINGE_FAKE: return -fminf(-p - 1.f, 0.f);
    case UEGAN_PRED_NEG_MEAN: return -p;
    default: return p;
  }
}
__device__ __forceinline__ float pred_term_grad(float p, int fid, float t) {
  switch (fid) {
    case UEGAN_PRED_BCE: return 1.f / (1.f + expf(-p)) - t;
    case UEGAN_PRED_LS: return 2.f * (p - t);
    // torch.min(x, 0) hands half of the gradient to each argument where the two are equal (p exactly on the threshold)
    case UEGAN_PRED_HINGE_REAL: return p - 1.f < 0.f ? -1.f : (p - 1.f == 0.f ? -0.5f : 0.f);
    case UEGAN_PRED_HINGE_FAKE: return -p - 1.f < 0.f ? 1.f : (-p - 1.f == 0.f ? 0.5f : 0.f);
    case UEGAN_PRED_NEG_MEAN: return -1.f;
    default: return 1.f;
  }
}
__global__ void pred_terms_kernel(PredArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  float sa = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) sa += pred_term(a.p[sc][i], a.fid, a.target);
  sa = block_sum(sa, red);
  if (threadIdx.x == 0) a.tmp[sc * RB + blockIdx.x] = sa;
}
__global__ void pred_loss_kernel(PredArgs a) {      // one wave
  float L = 0.f;
  for (int k = 0; k < a.nscales; ++k) L += fold_partials(a.tmp + k * RB, a.nbx) / (float)a.n[k];
  if (threadIdx.x == 0) *a.loss = L;
}
__global__ void pred_grad_kernel(PredArgs a, const float* gscale) {
  const int sc = blockIdx.y;
  const long long n = a.n[sc];
  const float k = (gscale ? *gscale : 1.f) / (float)n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    a.g[sc][i] = k * pred_term_grad(a.p[sc][i], a.fid, a.target);
}

// ----------------------------------------------------------------------------------------------------
// The same loss read straight off the prediction-head maps of a BATCHED discriminator pass (uegan_amd/fused.py): the maps are
// NHWC with channel 0 = tanh output (the other channels of the 16-byte chunk are padding), image groups of nb images lie one
// after the other in the batch, and the loss is a sum over (real group, fake group) pairs -- trainer.py:92+95 is
// {(exp, fake_store), (exp, raw)}, :104 is {(exp, fake)}.  The gradient comes back in the same layout already multiplied by
// tanh'(P) = 1 - P^2, i.e. it IS the head convolution's pre-activation gradient.
// ----------------------------------------------------------------------------------------------------
constexpr int RH_MAXG = 4, RH_MAXP = 4;
struct RaHeadArgs {
  const void* maps[8];
  void* gmaps[8];
  long long npg[8];       // prediction pixels per group (nb * h * w) of each scale
  int pr[RH_MAXP], pf[RH_MAXP];
  float* tmp;             // [nscales][RH_MAXG] group sums, then [nscales][RH_MAXP][4] {sum A, sum B, cnt A, cnt B}, then the block
                          // partials of both: [nscales][RH_MAXG][RB], [nscales][RH_MAXP][4][RB]
  float* loss;
  int nscales, ngroups, npairs, cp, nbx;
  unsigned gmask;         // groups whose gradient is wanted
  float sgn;
};

__device__ __forceinline__ float* rh_gpart(const RaHeadArgs& a, int sc, int g) {
  return a.tmp + a.nscales * (RH_MAXG + RH_MAXP * 4) + (sc * RH_MAXG + g) * RB;
}
__device__ __forceinline__ float* rh_ppart(const RaHeadArgs& a, int sc, int pi, int q) {
  return a.tmp + a.nscales * (RH_MAXG + RH_MAXP * 4) + a.nscales * RH_MAXG * RB + ((sc * RH_MAXP + pi) * 4 + q) * RB;
}

template <typename T>
__global__ void rahead_means_kernel(RaHeadArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y, g = blockIdx.z;
  const long long n = a.npg[sc];
  const T* p = static_cast<const T*>(a.maps[sc]) + (size_t)g * n * a.cp;
  float sm = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) sm += DT<T>::ld(p + i * a.cp);
  sm = block_sum(sm, red);
  if (threadIdx.x == 0) rh_gpart(a, sc, g)[blockIdx.x] = sm;
}

template <typename T>
__global__ void rahead_terms_kernel(RaHeadArgs a) {
  __shared__ float red[16];
  const int sc = blockIdx.y, pi = blockIdx.z;
  const long long n = a.npg[sc];
  const int gr = a.pr[pi], gf = a.pf[pi];
  const T* pr = static_cast<const T*>(a.maps[sc]) + (size_t)gr * n * a.cp;
  const T* pf = static_cast<const T*>(a.maps[sc]) + (size_t)gf * n * a.cp;
  {      // the two group sums from the partials of rahead_means_kernel (waves 0 / 1); block x == 0 files them in the slots
    const int wv = threadIdx.x >> 6;
    if (wv < 2) {
      const int g = wv == 0 ? gr : gf;
      const float v = fold_partials(rh_gpart(a, sc, g), a.nbx);
      if ((threadIdx.x & 63) == 0) {
        red[wv] = v;
        if (blockIdx.x == 0) a.tmp[sc * RH_MAXG + g] = v;      // (pairs sharing a group store the same value)
      }
    }
    __syncthreads();
  }
  const float rbar = red[0] / (float)n, fbar = red[1] / (float)n;
  __syncthreads();
  float sa = 0.f, sb = 0.f, ca = 0.f, cb = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float A = 1.f - a.sgn * (DT<T>::ld(pr + i * a.cp) - fbar);
    const float Bv = 1.f + a.sgn * (DT<T>::ld(pf + i * a.cp) - rbar);
    if (A > 0.f) { sa += A; ca += 1.f; }
    if (Bv > 0.f) { sb += Bv; cb += 1.f; }
  }
  sa = block_sum(sa, red);
  sb = block_sum(sb, red);
  ca = block_sum(ca, red);
  cb = block_sum(cb, red);
  if (threadIdx.x == 0) {
    rh_ppart(a, sc, pi, 0)[blockIdx.x] = sa; rh_ppart(a, sc, pi, 1)[blockIdx.x] = sb;
    rh_ppart(a, sc, pi, 2)[blockIdx.x] = ca; rh_ppart(a, sc, pi, 3)[blockIdx.x] = cb;
  }
}

// one wave: folds the pair-term partials into the slots (the gradient kernel reads them there) and adds up the loss
__global__ void rahead_loss_kernel(RaHeadArgs a) {
  float Ltot = 0.f;
  for (int pi = 0; pi < a.npairs; ++pi)        // pair-major, scale-minor: the order trainer.py:92,95 adds the two GANLoss calls
    for (int k = 0; k < a.nscales; ++k) {
      float* o = a.tmp + a.nscales * RH_MAXG + (k * RH_MAXP + pi) * 4;
      float t[4];
      for (int q = 0; q < 4; ++q) {
        t[q] = fold_partials(rh_ppart(a, k, pi, q), a.nbx);
        if (threadIdx.x == 0) o[q] = t[q];
      }
      const float nk = (float)a.npg[k];
      Ltot += 0.5f * (t[0] / nk + t[1] / nk);
    }
  if (threadIdx.x == 0) *a.loss = Ltot;
}

// one thread per prediction pixel: dP summed over the pairs the pixel's group takes part in, times tanh'(P); one 16-byte (bf16) /
// two-chunk (fp32, cp = 4: one chunk) store with zeros in the padding channels
template <typename T>
__global__ void rahead_grad_kernel(RaHeadArgs a, const float* gscale) {
  const int sc = blockIdx.y, g = blockIdx.z;
  if (!((a.gmask >> g) & 1u)) return;
  const long long n = a.npg[sc];
  const float fn = (float)n;
  const T* p = static_cast<const T*>(a.maps[sc]) + (size_t)g * n * a.cp;
  T* o = static_cast<T*>(a.gmaps[sc]) + (size_t)g * n * a.cp;
  const float gs = a.sgn * 0.5f / fn * (gscale ? *gscale : 1.f);
  // per pair this group is in: threshold mean and the count term
  float bar[RH_MAXP], cnt[RH_MAXP];
  int role[RH_MAXP];       // 0: not in the pair, 1: real, 2: fake
#pragma unroll
  for (int pi = 0; pi < RH_MAXP; ++pi) {
    role[pi] = 0; bar[pi] = 0.f; cnt[pi] = 0.f;
    if (pi < a.npairs) {
      const float* t = a.tmp + a.nscales * RH_MAXG + (sc * RH_MAXP + pi) * 4;
      if (a.pr[pi] == g) { role[pi] = 1; bar[pi] = a.tmp[sc * RH_MAXG + a.pf[pi]] / fn; cnt[pi] = t[3] / fn; }
      else if (a.pf[pi] == g) { role[pi] = 2; bar[pi] = a.tmp[sc * RH_MAXG + a.pr[pi]] / fn; cnt[pi] = t[2] / fn; }
    }
  }
  constexpr int EPC = DT<T>::EPC;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float P = DT<T>::ld(p + i * a.cp);
    float d = 0.f;
#pragma unroll
    for (int pi = 0; pi < RH_MAXP; ++pi) {
      if (role[pi] == 1) {
        const float A = 1.f - a.sgn * (P - bar[pi]);
        d -= gs * ((A > 0.f ? 1.f : 0.f) + cnt[pi]);
      } else if (role[pi] == 2) {
        const float Bv = 1.f + a.sgn * (P - bar[pi]);
        d += gs * ((Bv > 0.f ? 1.f : 0.f) + cnt[pi]);
      }
    }
    float v[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[e] = 0.f;
    v[0] = d * (1.f - P * P);
    for (int c0 = 0; c0 < a.cp; c0 += EPC) {
      Vec<T, EPC>::st(o + i * a.cp + c0, v);
      v[0] = 0.f;
    }
  }
}

// ----------------------------------------------------------------------------------------------------
// MultiscaleRecLoss (losses.py:202-231): criterion at `nscales` scales with AvgPool2d(2,2) between, weights 1, 1/2, 1/4.
// KIND 0 L1Loss, 1 SmoothL1Loss (beta = 1), 2 MSELoss.  One thread per 4x4 block of one channel plane; per-block partial sums, added up
// in a fixed order by msrec_final_kernel (deterministic).
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
template <int KIND> __device__ __forceinline__ float rec_term(float d) {
  if (KIND == 0) return fabsf(d);
  if (KIND == 1) { const float ad = fabsf(d); return ad < 1.f ? 0.5f * d * d : ad - 0.5f; }
  return d * d;
}
template <int KIND> __device__ __forceinline__ float rec_grad(float d) {
  if (KIND == 0) return sgnf(d);
  if (KIND == 1) return fabsf(d) < 1.f ? d : sgnf(d);
  return 2.f * d;
}

template <int KIND>
__global__ void msrec_kernel(const float* pred, const float* gt, float* part, float* gpred, const float* gscale, int planes, int H, int W, int nscales) {
  __shared__ float red[16];
  const int bw = W / 4, bh = H / 4;
  const size_t total = (size_t)planes * bh * bw;
  const float n0 = (float)planes * (float)H * (float)W;
  const float c0 = 1.f / n0, c1 = nscales > 1 ? 0.5f / (n0 / 4.f) : 0.f, c2 = nscales > 2 ? 0.25f / (n0 / 16.f) : 0.f;
  const float gs = (gpred && gscale) ? *gscale : 1.f;
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int bx = (int)(i % bw);
    size_t t = i / bw;
    const int by = (int)(t % bh);
    const size_t pl = t / bh;
    const size_t base = (pl * H + (size_t)by * 4) * W + (size_t)bx * 4;
    float d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pred + base + (size_t)r * W);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gt + base + (size_t)r * W);
      d[r][0] = pv.x - gv.x; d[r][1] = pv.y - gv.y; d[r][2] = pv.z - gv.z; d[r][3] = pv.w - gv.w;
    }
    float d1[2][2], l0 = 0.f, l1 = 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        d1[r][c] = 0.25f * (d[2 * r][2 * c] + d[2 * r][2 * c + 1] + d[2 * r + 1][2 * c] + d[2 * r + 1][2 * c + 1]);
        l1 += rec_term<KIND>(d1[r][c]);
      }
    const float d2 = 0.25f * (d1[0][0] + d1[0][1] + d1[1][0] + d1[1][1]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) l0 += rec_term<KIND>(d[r][c]);
    acc += c0 * l0 + c1 * l1 + c2 * rec_term<KIND>(d2);
    if (gpred) {
      const float g2 = gs * c2 * rec_grad<KIND>(d2) * (1.f / 16.f);
      const float g0 = gs * c0, g1 = gs * c1 * 0.25f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x4 o;
        o.x = g0 * rec_grad<KIND>(d[r][0]) + g1 * rec_grad<KIND>(d1[r / 2][0]) + g2;
        o.y = g0 * rec_grad<KIND>(d[r][1]) + g1 * rec_grad<KIND>(d1[r / 2][0]) + g2;
        o.z = g0 * rec_grad<KIND>(d[r][2]) + g1 * rec_grad<KIND>(d1[r / 2][1]) + g2;
        o.w = g0 * rec_grad<KIND>(d[r][3]) + g1 * rec_grad<KIND>(d1[r / 2][1]) + g2;
        *reinterpret_cast<f32x4*>(gpred + base + (size_t)r * W) = o;
      }
    }
  }
  acc = block_sum(acc, red);
  if (part && threadIdx.x == 0) part[blockIdx.x] = acc;
}

// any H x W (AvgPool2d(2, 2) floors: a last odd row / column does not reach the next scale, losses.py:225-227): one thread per 4 x 4
// block of the ceil grid, scalar accesses, per-element validity.  The denominators are the element counts of the floored maps.
template <int KIND>
__global__ void msrec_ragged_kernel(const float* pred, const float* gt, float* part, float* gpred, const float* gscale, int planes, int H, int W,
                                    int nscales) {
  __shared__ float red[16];
  const int bw = (W + 3) / 4, bh = (H + 3) / 4;
  const int H1 = H / 2, W1 = W / 2, H2 = H1 / 2, W2 = W1 / 2;
  const size_t total = (size_t)planes * bh * bw;
  const float c0 = 1.f / ((float)planes * (float)H * (float)W);
  const float c1 = nscales > 1 ? 0.5f / ((float)planes * (float)H1 * (float)W1) : 0.f;
  const float c2 = nscales > 2 ? 0.25f / ((float)planes * (float)H2 * (float)W2) : 0.f;
  const float gs = (gpred && gscale) ? *gscale : 1.f;
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int bx = (int)(i % bw);
    size_t t = i / bw;
    const int by = (int)(t % bh);
    const size_t pl = t / bh;
    const size_t base = (pl * H + (size_t)by * 4) * W + (size_t)bx * 4;
    float d[4][4];
    float l0 = 0.f, l1 = 0.f, l2 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool ok = by * 4 + r < H && bx * 4 + c < W;
        d[r][c] = ok ? pred[base + (size_t)r * W + c] - gt[base + (size_t)r * W + c] : 0.f;
        l0 += ok ? rec_term<KIND>(d[r][c]) : 0.f;
      }
    float d1[2][2];
    bool ok1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        ok1[r][c] = nscales > 1 && by * 2 + r < H1 && bx * 2 + c < W1;
        d1[r][c] = 0.25f * (d[2 * r][2 * c] + d[2 * r][2 * c + 1] + d[2 * r + 1][2 * c] + d[2 * r + 1][2 * c + 1]);
        l1 += ok1[r][c] ? rec_term<KIND>(d1[r][c]) : 0.f;
      }
    const bool ok2 = nscales > 2 && by < H2 && bx < W2;
    const float d2 = 0.25f * (d1[0][0] + d1[0][1] + d1[1][0] + d1[1][1]);
    l2 = ok2 ? rec_term<KIND>(d2) : 0.f;
    acc += c0 * l0 + c1 * l1 + c2 * l2;
    if (gpred) {
      const float g2 = ok2 ? gs * c2 * rec_grad<KIND>(d2) * (1.f / 16.f) : 0.f;
      const float g0 = gs * c0, g1 = gs * c1 * 0.25f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (by * 4 + r < H && bx * 4 + c < W)
            gpred[base + (size_t)r * W + c] = g0 * rec_grad<KIND>(d[r][c]) + (ok1[r / 2][c / 2] ? g1 * rec_grad<KIND>(d1[r / 2][c / 2]) : 0.f) + g2;
    }
  }
  acc = block_sum(acc, red);
  if (part && threadIdx.x == 0) part[blockIdx.x] = acc;
}

// single scale (multiscale=False, or scale=1), any H x W: mean criterion(pred - gt)
template <int KIND>
__global__ void rec_flat_kernel(const float* pred, const float* gt, float* part, float* gpred, const float* gscale, size_t n) {
  __shared__ float red[16];
  const float c0 = 1.f / (float)n, gs = (gpred && gscale) ? *gscale : 1.f;
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = pred[i] - gt[i];
    acc += c0 * rec_term<KIND>(d);
    if (gpred) gpred[i] = gs * c0 * rec_grad<KIND>(d);
  }
  acc = block_sum(acc, red);
  if (part && threadIdx.x == 0) part[blockIdx.x] = acc;
}

constexpr int MSREC_MAXB = 2048;
__global__ void msrec_final_kernel(const float* part, int nb, float* loss) {      // one block: fixed summation order
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) acc += part[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = acc;
}

}  // namespace uegan

using namespace uegan;

// Block counts per scale.  A reduction stage leaves one partial per block for a single wave to fold (<= RB blocks of 256 threads x 4 elements);
// the gradient stages are elementwise and only bound their grids.
static inline int red_blocks(long long maxn) { return blocks_for((size_t)maxn, 1024, RB); }
static inline int grad_blocks(long long maxn) { return blocks_for((size_t)maxn, 1024, 256); }

static int ra_fill(RaArgs& a, int nscales, const float* const* real, const float* const* fake, const int64_t* n, int for_discriminator,
                   float* const* greal, float* const* gfake, float* tmp, long long& maxn) {
  UEGAN_CHECK_ARG(nscales >= 1 && nscales <= 8 && real && fake && n && tmp, "bad rahinge args");
  maxn = 0;
  for (int i = 0; i < 8; ++i) {
    a.real[i] = i < nscales ? real[i] : nullptr;
    a.fake[i] = i < nscales ? fake[i] : nullptr;
    a.greal[i] = (i < nscales && greal) ? greal[i] : nullptr;
    a.gfake[i] = (i < nscales && gfake) ? gfake[i] : nullptr;
    a.n[i] = i < nscales ? (long long)n[i] : 0;
    if (i < nscales) {
      UEGAN_CHECK_ARG(real[i] && fake[i] && n[i] > 0, "bad rahinge scale %d", i);
      if (a.n[i] > maxn) maxn = a.n[i];
    }
  }
  a.tmp = tmp; a.loss = nullptr; a.nscales = nscales; a.sgn = for_discriminator ? 1.f : -1.f;
  a.nbx = red_blocks(maxn);
  return UEGAN_OK;
}

extern "C" size_t uegan_rahinge_workspace_floats(int nscales) { return (size_t)nscales * (8 + 6 * RB); }
extern "C" size_t uegan_pred_loss_workspace_floats(int nscales) { return (size_t)nscales * RB; }

// the relativistic pair: means, then the terms of 'rahinge' or 'rals', then one combination (sum_k (tmp2 / n + tmp3 / n) / 2 for both)
static int ra_fwd(void (*terms_kernel)(RaArgs), int nscales, const float* const* real, const float* const* fake, const int64_t* n,
                  int for_discriminator, float* loss, float* tmp, uegan_stream_t stream) {
  RaArgs a;
  long long maxn;
  int rc = ra_fill(a, nscales, real, fake, n, for_discriminator, nullptr, nullptr, tmp, maxn);
  if (rc) return rc;
  UEGAN_CHECK_ARG(loss, "null loss");
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(a.nbx, nscales);
  hipLaunchKernelGGL(rahinge_means_kernel, grid, dim3(256), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(terms_kernel, grid, dim3(256), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(rahinge_loss_kernel, dim3(1), dim3(64), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
static int ra_bwd(void (*grad_kernel)(RaArgs, const float*), int nscales, const float* const* real, const float* const* fake, const int64_t* n,
                  int for_discriminator, const float* tmp, const float* gscale, float* const* greal, float* const* gfake, uegan_stream_t stream) {
  RaArgs a;
  long long maxn;
  int rc = ra_fill(a, nscales, real, fake, n, for_discriminator, greal, gfake, const_cast<float*>(tmp), maxn);
  if (rc) return rc;
  hipLaunchKernelGGL(grad_kernel, dim3(grad_blocks(maxn), nscales), dim3(256), 0, (hipStream_t)stream, a, gscale);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_rahinge_fwd(int nscales, const float* const* real, const float* const* fake, const int64_t* n, int for_discriminator,
                                 float* loss, float* tmp, uegan_stream_t stream) {
  return ra_fwd(rahinge_terms_kernel, nscales, real, fake, n, for_discriminator, loss, tmp, stream);
}
extern "C" int uegan_rahinge_bwd(int nscales, const float* const* real, const float* const* fake, const int64_t* n, int for_discriminator,
                                 const float* tmp, const float* gscale, float* const* greal, float* const* gfake, uegan_stream_t stream) {
  return ra_bwd(rahinge_grad_kernel, nscales, real, fake, n, for_discriminator, tmp, gscale, greal, gfake, stream);
}
extern "C" int uegan_rals_fwd(int nscales, const float* const* real, const float* const* fake, const int64_t* n, int for_discriminator,
                              float* loss, float* tmp, uegan_stream_t stream) {
  return ra_fwd(rals_terms_kernel, nscales, real, fake, n, for_discriminator, loss, tmp, stream);
}
extern "C" int uegan_rals_bwd(int nscales, const float* const* real, const float* const* fake, const int64_t* n, int for_discriminator,
                              const float* tmp, const float* gscale, float* const* greal, float* const* gfake, uegan_stream_t stream) {
  return ra_bwd(rals_grad_kernel, nscales, real, fake, n, for_discriminator, tmp, gscale, greal, gfake, stream);
}

static int pred_fill(PredArgs& a, int fid, float target, int nscales, const float* const* preds, const int64_t* n, float* const* gpreds, float* tmp,
                     long long& maxn) {
  UEGAN_CHECK_ARG(nscales >= 1 && nscales <= 8 && preds && n && tmp, "bad pred_loss args");
  UEGAN_CHECK_ARG(fid >= UEGAN_PRED_BCE && fid <= UEGAN_PRED_POS_MEAN, "bad pred_loss term %d", fid);
  maxn = 0;
  for (int i = 0; i < 8; ++i) {
    a.p[i] = i < nscales ? preds[i] : nullptr;
    a.g[i] = (i < nscales && gpreds) ? gpreds[i] : nullptr;
    a.n[i] = i < nscales ? (long long)n[i] : 0;
    if (i < nscales) {
      UEGAN_CHECK_ARG(preds[i] && n[i] > 0 && (!gpreds || gpreds[i]), "bad pred_loss scale %d", i);
      if (a.n[i] > maxn) maxn = a.n[i];
    }
  }
  a.tmp = tmp; a.loss = nullptr; a.nscales = nscales; a.fid = fid; a.target = target;
  a.nbx = red_blocks(maxn);
  return UEGAN_OK;
}

extern "C" int uegan_pred_loss_fwd(int term, float target, int nscales, const float* const* preds, const int64_t* n, float* loss, float* tmp,
                                   uegan_stream_t stream) {
  PredArgs a;
  long long maxn;
  int rc = pred_fill(a, term, target, nscales, preds, n, nullptr, tmp, maxn);
  if (rc) return rc;
  UEGAN_CHECK_ARG(loss, "null loss");
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pred_terms_kernel, dim3(a.nbx, nscales), dim3(256), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(pred_loss_kernel, dim3(1), dim3(64), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_pred_loss_bwd(int term, float target, int nscales, const float* const* preds, const int64_t* n, const float* gscale,
                                   float* const* gpreds, uegan_stream_t stream) {
  PredArgs a;
  long long maxn;
  float dummy;
  UEGAN_CHECK_ARG(gpreds, "null gradient table");
  int rc = pred_fill(a, term, target, nscales, preds, n, gpreds, &dummy, maxn);
  if (rc) return rc;
  hipLaunchKernelGGL(pred_grad_kernel, dim3(grad_blocks(maxn), nscales), dim3(256), 0, (hipStream_t)stream, a, gscale);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

static int rahead_fill(RaHeadArgs& a, int nscales, const void* const* maps, const int64_t* pix_per_image, int nb, int cp, int ngroups,
                       int npairs, const int32_t* pairs, int for_discriminator, float* tmp, long long& maxn) {
  UEGAN_CHECK_ARG(nscales >= 1 && nscales <= 8 && maps && pix_per_image && tmp && nb > 0 && cp > 0, "bad rahinge_heads args");
  UEGAN_CHECK_ARG(ngroups >= 2 && ngroups <= RH_MAXG && npairs >= 1 && npairs <= RH_MAXP && pairs, "rahinge_heads: 2..%d groups, 1..%d pairs", RH_MAXG, RH_MAXP);
  maxn = 0;
  for (int i = 0; i < 8; ++i) {
    a.maps[i] = i < nscales ? maps[i] : nullptr;
    a.gmaps[i] = nullptr;
    a.npg[i] = i < nscales ? (long long)nb * pix_per_image[i] : 0;
    if (i < nscales) {
      UEGAN_CHECK_ARG(maps[i] && pix_per_image[i] > 0, "bad rahinge_heads scale %d", i);
      if (a.npg[i] > maxn) maxn = a.npg[i];
    }
  }
  for (int i = 0; i < RH_MAXP; ++i) {
    a.pr[i] = i < npairs ? pairs[2 * i] : -1;
    a.pf[i] = i < npairs ? pairs[2 * i + 1] : -1;
    if (i < npairs) UEGAN_CHECK_ARG(a.pr[i] >= 0 && a.pr[i] < ngroups && a.pf[i] >= 0 && a.pf[i] < ngroups && a.pr[i] != a.pf[i], "bad pair %d", i);
  }
  a.tmp = tmp; a.loss = nullptr; a.nscales = nscales; a.ngroups = ngroups; a.npairs = npairs; a.cp = cp; a.gmask = 0;
  a.sgn = for_discriminator ? 1.f : -1.f;
  a.nbx = red_blocks(maxn);
  return UEGAN_OK;
}

extern "C" size_t uegan_rahinge_heads_workspace_floats(int nscales) { return (size_t)nscales * (RH_MAXG + RH_MAXP * 4) * (1 + RB); }

extern "C" int uegan_rahinge_heads_fwd(int dtype, int nscales, const void* const* maps, const int64_t* pix_per_image, int nb, int cp,
                                       int ngroups, int npairs, const int32_t* pairs, int for_discriminator, float* loss, float* tmp,
                                       uegan_stream_t stream) {
  RaHeadArgs a;
  long long maxn;
  int rc = rahead_fill(a, nscales, maps, pix_per_image, nb, cp, ngroups, npairs, pairs, for_discriminator, tmp, maxn);
  if (rc) return rc;
  UEGAN_CHECK_ARG(loss, "null loss");
  UEGAN_CHECK_ARG(cp % epc_of(dtype) == 0, "head maps must carry whole 16-byte chunks per pixel");
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  UEGAN_DISPATCH_T(dtype, hipLaunchKernelGGL((rahead_means_kernel<T>), dim3(a.nbx, nscales, ngroups), dim3(256), 0, s, a));
  UEGAN_CHECK_LAUNCH();
  UEGAN_DISPATCH_T(dtype, hipLaunchKernelGGL((rahead_terms_kernel<T>), dim3(a.nbx, nscales, npairs), dim3(256), 0, s, a));
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(rahead_loss_kernel, dim3(1), dim3(64), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_rahinge_heads_bwd(int dtype, int nscales, const void* const* maps, const int64_t* pix_per_image, int nb, int cp,
                                       int ngroups, int npairs, const int32_t* pairs, int for_discriminator, const float* tmp,
                                       const float* gscale, void* const* gmaps, uint32_t group_mask, uegan_stream_t stream) {
  RaHeadArgs a;
  long long maxn;
  int rc = rahead_fill(a, nscales, maps, pix_per_image, nb, cp, ngroups, npairs, pairs, for_discriminator, const_cast<float*>(tmp), maxn);
  if (rc) return rc;
  UEGAN_CHECK_ARG(gmaps && group_mask, "rahinge_heads_bwd: no gradient requested");
  for (int i = 0; i < nscales; ++i) {
    UEGAN_CHECK_ARG(gmaps[i], "null gradient map %d", i);
    a.gmaps[i] = gmaps[i];
  }
  a.gmask = group_mask;
  const int bx = blocks_for((size_t)maxn, 256, 1024);      // one thread per prediction pixel
  UEGAN_DISPATCH_T(dtype, hipLaunchKernelGGL((rahead_grad_kernel<T>), dim3(bx, nscales, ngroups), dim3(256), 0, (hipStream_t)stream, a, gscale));
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

static int msrec_launch(const float* pred, const float* gt, float* loss, float* scratch, float* gpred, const float* gscale, int B, int C,
                        int H, int W, int kind, int nscales, hipStream_t s) {
  UEGAN_CHECK_ARG(pred && gt && B > 0 && C > 0 && H > 0 && W > 0, "bad multiscale-rec args");
  UEGAN_CHECK_ARG(kind >= 0 && kind <= 2 && nscales >= 1 && nscales <= 3, "multiscale rec: kind 0..2 (l1 / smoothl1 / l2), 1..3 scales");
  // (like AvgPool2d, which raises "Output size is too small" when a pooled map would be empty)
  UEGAN_CHECK_ARG(nscales == 1 || ((H >> (nscales - 1)) > 0 && (W >> (nscales - 1)) > 0), "multiscale rec loss: %dx%d is too small for %d scales", H, W,
                  nscales);
  const bool ragged = nscales > 1 && (H % 4 != 0 || W % 4 != 0);
  const size_t total = nscales == 1 ? (size_t)B * C * H * W : (size_t)B * C * ((H + 3) / 4) * ((W + 3) / 4);
  const int blocks = blocks_for(total, 256, MSREC_MAXB);      // one partial per block in `scratch`
#define UEGAN_MSREC(K)                                                                                                              \
  do {                                                                                                                              \
    if (nscales == 1) hipLaunchKernelGGL((rec_flat_kernel<K>), dim3(blocks), dim3(256), 0, s, pred, gt, scratch, gpred, gscale, total); \
    else if (ragged) hipLaunchKernelGGL((msrec_ragged_kernel<K>), dim3(blocks), dim3(256), 0, s, pred, gt, scratch, gpred, gscale, B * C, H, W, nscales); \
    else hipLaunchKernelGGL((msrec_kernel<K>), dim3(blocks), dim3(256), 0, s, pred, gt, scratch, gpred, gscale, B * C, H, W, nscales); \
  } while (0)
  if (kind == 0) UEGAN_MSREC(0); else if (kind == 1) UEGAN_MSREC(1); else UEGAN_MSREC(2);
#undef UEGAN_MSREC
  UEGAN_CHECK_LAUNCH();
  if (loss) {
    hipLaunchKernelGGL(msrec_final_kernel, dim3(1), dim3(1024), 0, s, scratch, blocks, loss);
    UEGAN_CHECK_LAUNCH();
  }
  return UEGAN_OK;
}

extern "C" size_t uegan_msrec_scratch_floats(void) { return MSREC_MAXB; }

extern "C" int uegan_msrec_fwd(const float* pred, const float* gt, float* loss, float* scratch, int B, int C, int H, int W, int kind, int nscales,
                               uegan_stream_t stream) {
  UEGAN_CHECK_ARG(loss && scratch, "null loss / scratch");
  return msrec_launch(pred, gt, loss, scratch, nullptr, nullptr, B, C, H, W, kind, nscales, (hipStream_t)stream);
}

extern "C" int uegan_msrec_bwd(const float* pred, const float* gt, const float* gscale, float* gpred, int B, int C, int H, int W, int kind,
                               int nscales, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(gpred, "null gpred");
  return msrec_launch(pred, gt, nullptr, nullptr, gpred, gscale, B, C, H, W, kind, nscales, (hipStream_t)stream);
}

// the round-1/2 entry points of the default identity loss (three-scale L1): kept as aliases of uegan_msrec_* (kind 0, 3 scales)
extern "C" size_t uegan_msl1_scratch_floats(void) { return MSREC_MAXB; }
extern "C" int uegan_msl1_fwd(const float* pred, const float* gt, float* loss, float* scratch, int B, int C, int H, int W, uegan_stream_t stream) {
  return uegan_msrec_fwd(pred, gt, loss, scratch, B, C, H, W, 0, 3, stream);
}
extern "C" int uegan_msl1_bwd(const float* pred, const float* gt, const float* gscale, float* gpred, int B, int C, int H, int W,
                              uegan_stream_t stream) {
  return uegan_msrec_bwd(pred, gt, gscale, gpred, B, C, H, W, 0, 3, stream);
}
