// Weight gradients: the transpose-read kernel (wgrad_tr.h, bf16) and the older register-transpose kernel, their split-K reduce, the bias
// gradient, the scalar direct kernel (cross-checks only) and the uegan_conv2d_wgrad* entry points.
#include "conv_core.h"

namespace uegan {

// ----------------------------------------------------------------------------------------------------
// wgrad: dW[co][kk] = sum_pixels dz[pix][co] * gather(pix, kk), split over pixel ranges (split-K), partials
// to workspace, then a reduce kernel that sums the splits, scales and permutes to OIHW fp32.
// ----------------------------------------------------------------------------------------------------
struct WgradArgs {
  ConvGeom g;          // forward gather geometry (mode 0): rows = conv outputs, source = conv input
  const void* in1;
  const void* in2;
  const void* dz;      // [B][OH][OW][zC]
  float* ws;           // [nsplit][N][ktot]
  int N, zC, ktot;     // N = rows computed (true Cout), zC = channel stride of dz (padded Cout), ktot = KH*KW*C (padded C)
  int WS, WSlog, R;    // pixel strip: WS columns (power of two) x R rows = 32 slots
  int nxb, nyb;        // strips per row / per image
  int steps_total, steps_per_split;
};

constexpr int WG_BK = 128;   // kk columns per block

// In-register transpose of an E x E block of 16-bit (E=8) or 32-bit (E=4) elements held as E 16-byte rows.
__device__ __forceinline__ void transpose_chunks(const u32x4 (&in)[4], u32x4 (&out)[4]) {   // fp32: 4x4
  out[0] = u32x4{in[0].x, in[1].x, in[2].x, in[3].x};
  out[1] = u32x4{in[0].y, in[1].y, in[2].y, in[3].y};
  out[2] = u32x4{in[0].z, in[1].z, in[2].z, in[3].z};
  out[3] = u32x4{in[0].w, in[1].w, in[2].w, in[3].w};
}
__device__ __forceinline__ void transpose_chunks(const u32x4 (&in)[8], u32x4 (&out)[8]) {   // bf16: 8x8
  // in[p] = 8 channels of pixel p (dword d holds channels 2d, 2d+1); out[c] = 8 pixels of channel c
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const uint32_t a = in[2 * pp][d], b = in[2 * pp + 1][d];
      lo[pp] = (a & 0xffffu) | (b << 16);            // channel 2d   of pixels 2pp, 2pp+1
      hi[pp] = (a >> 16) | (b & 0xffff0000u);        // channel 2d+1
    }
    out[2 * d] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    out[2 * d + 1] = u32x4{hi[0], hi[1], hi[2], hi[3]};
  }
}

// wgrad block: BN output-channel rows x 128 kk columns, reduction over a range of pixel strips (split-K).
// One K step = 128 bytes of pixels per row (64 bf16 / 32 fp32 pixel slots).  Both operands arrive pixel-major from HBM
// (NHWC) but MFMA wants the reduction index contiguous per lane, so each thread loads an E x E block (E pixels x one
// 16-byte channel chunk), transposes it in registers and writes E 16-byte rows [channel][E pixels] into the swizzled
// LDS tile.  Lane mapping: the 8 lanes of a ds_write_b128 lane group hold 8 different pixel groups of one channel chunk,
// which makes the transposed writes bank-conflict free.  Two LDS buffers, one barrier per step.
template <typename T, int BN>
__global__ void __launch_bounds__(256) conv_wgrad_kernel(WgradArgs a) {
  constexpr int EPC = DT<T>::EPC;
  constexpr int ROWB = CONV_ROWB;
  constexpr int NPIX = ROWB / (int)sizeof(T);                 // pixel slots per step (64 / 32)
  constexpr int NCHUNK = Mma<T>::NCHUNK;
  constexpr int NSUB = NPIX / 32;
  constexpr int ZCH = BN / EPC, XCH = WG_BK / EPC;            // channel chunks of the two tiles
  constexpr int NUNIT = 8 * (ZCH + XCH);                      // 8 pixel groups x chunks
  constexpr int NU = (NUNIT + 255) / 256;
  constexpr int WZ = BN >= 64 ? 2 : 1, WX = 4 / WZ;           // wave grid (co x kk)
  constexpr int TN = BN / WZ / 16, TM = WG_BK / WX / 16;
  constexpr int BUFB = (BN + WG_BK) * ROWB;
  static_assert(TN >= 1 && TM >= 1 && NPIX / EPC == 8, "tile");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUFB];

  const ConvGeom& g = a.g;
  const T* in1 = static_cast<const T*>(a.in1);
  const T* in2 = static_cast<const T*>(a.in2);
  const T* dz = static_cast<const T*>(a.dz);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wz = wave / WX, wx = wave % WX;
  const int kk_base = blockIdx.x * WG_BK, n_base = blockIdx.y * BN, split = blockIdx.z;
  int s_begin = split * a.steps_per_split;
  int s_end = s_begin + a.steps_per_split;
  if (s_end > a.steps_total) s_end = a.steps_total;

  // my units: unit id = u*256 + tid -> pixel group pq = id & 7, chunk index ch = id >> 3 (dz chunks first, then x chunks)
  int u_kind[NU], u_pq[NU], u_row0[NU], u_ty[NU], u_tx[NU], u_c[NU];    // kind: 0 dz, 1 x, 2 idle
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int id = u * 256 + tid;
    u_pq[u] = id & 7;
    const int ch = id >> 3;
    u_kind[u] = ch < ZCH ? 0 : (ch < ZCH + XCH ? 1 : 2);
    const int lc = ch < ZCH ? ch : ch - ZCH;
    u_row0[u] = (ch < ZCH ? 0 : BN) + lc * EPC;               // first LDS row (channel) of the unit
    u_c[u] = -1; u_ty[u] = 0; u_tx[u] = 0;
    if (u_kind[u] == 0) {
      u_c[u] = n_base + lc * EPC;                              // dz channel
      if (u_c[u] >= a.zC) u_c[u] = -1;
    } else if (u_kind[u] == 1) {
      const int kk = kk_base + lc * EPC;
      if (kk < a.ktot) {
        const int tap = kk / g.C;
        u_c[u] = kk - tap * g.C;
        u_ty[u] = tap / g.KW;
        u_tx[u] = tap - u_ty[u] * g.KW;
      }
    }
  }

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 regs[NU][EPC];

  auto load_units = [&](int s) {
    const int xb = s % a.nxb;
    const int t = s / a.nxb;
    const int yb = t % a.nyb;
    const int b = t / a.nyb;
    const int oy0 = yb * a.R, ox0 = xb * a.WS;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int p = 0; p < EPC; ++p) {
        const int slot = u_pq[u] * EPC + p;
        const int oy = oy0 + (slot >> a.WSlog), ox = ox0 + (slot & (a.WS - 1));
        const bool pv = oy < g.OH && ox < g.OW && u_c[u] >= 0;
        const void* src = g_zero16;
        if (pv) {
          if (u_kind[u] == 0) {
            src = dz + (((size_t)b * g.OH + oy) * g.OW + ox) * a.zC + u_c[u];
          } else if (u_kind[u] == 1) {
            const int sy = src_coord(g, oy, u_ty[u], 0, g.IH, g.OH);
            const int sx = src_coord(g, ox, u_tx[u], 0, g.IW, g.OW);
            if (sy >= 0 && sx >= 0) {
              const size_t pix = ((size_t)b * g.IH + sy) * g.IW + sx;
              const int c = u_c[u];
              src = (c < g.C1) ? (const void*)(in1 + pix * g.C1 + c) : (const void*)(in2 + pix * g.C2 + (c - g.C1));
            }
          }
        }
        regs[u][p] = *reinterpret_cast<const u32x4*>(src);
      }
    }
  };
  auto commit = [&](unsigned char* buf) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (u_kind[u] == 2) continue;
      u32x4 tr[EPC];
      transpose_chunks(regs[u], tr);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        const int row = u_row0[u] + e;
        *reinterpret_cast<u32x4*>(buf + row * ROWB + ((u_pq[u] ^ ((row >> 1) & 7)) << 4)) = tr[e];
      }
    }
  };

  if (s_begin < s_end) {
    load_units(s_begin);
    commit(lds);
  }
  const int fr = lane & 15, fg = lane >> 4;
  for (int s = s_begin; s < s_end; ++s) {
    unsigned char* cur = lds + ((s - s_begin) & 1) * BUFB;
    unsigned char* nxt = lds + ((s - s_begin + 1) & 1) * BUFB;
    __syncthreads();
    if (s + 1 < s_end) load_units(s + 1);
#pragma unroll
    for (int ksub = 0; ksub < NSUB; ++ksub) {
      u32x4 zf[TN][NCHUNK], xf[TM][NCHUNK];
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int row = wz * (BN / WZ) + i * 16 + fr;
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
          const int q = ksub * 4 + c * 4 * (NCHUNK - 1) + fg;
          zf[i][c] = *reinterpret_cast<const u32x4*>(cur + row * ROWB + ((q ^ ((row >> 1) & 7)) << 4));
        }
      }
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int row = BN + wx * (WG_BK / WX) + j * 16 + fr;
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
          const int q = ksub * 4 + c * 4 * (NCHUNK - 1) + fg;
          xf[j][c] = *reinterpret_cast<const u32x4*>(cur + row * ROWB + ((q ^ ((row >> 1) & 7)) << 4));
        }
      }
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) Mma<T>::step(zf[i], xf[j], acc[i][j]);
    }
    if (s + 1 < s_end) commit(nxt);
  }

  // partial tile -> workspace [split][N][ktot]; D rows = co, cols = kk
  float* ws = a.ws + (size_t)split * a.N * a.ktot;
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int kk = kk_base + wx * (WG_BK / WX) + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n_base + wz * (BN / WZ) + i * 16 + (lane >> 4) * 4 + r;
        if (n < a.N && kk < a.ktot) ws[(size_t)n * a.ktot + kk] = acc[i][j][r];
      }
    }
}

// sum splits, scale, permute [co][(ty,tx,c_padded)] -> OIHW [co][ci][ty][tx] (padding channels dropped).  Partials are
// [nsplit][pstride] with the N*ktot weight sums first; when dbias is given, N bias sums follow (unscaled).
// Block = 32 consecutive elements x 8 split lanes (fixed summation order: deterministic).
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* ws, float* dw, float* dbias, const float* scale, int nsplit, int N,
                                                            int C, int Cin_w, int KH, int KW, size_t pstride, int acc, int accb, int Cin_row) {
  // Cin_row: input channels per row of the OIHW destination (>= Cin_w: the convolution may use a column slice of a wider master weight)
  __shared__ float red[8][32];
  const int ktot = KH * KW * C;
  const size_t nw = (size_t)N * ktot, total = nw + (dbias ? (size_t)N : 0);
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const size_t i = (size_t)blockIdx.x * 32 + e;
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    int k = sl;
    for (; k + 24 < nsplit; k += 32) {
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] += ws[(size_t)(k + 8 * u) * pstride + i];
    }
    for (; k < nsplit; k += 8) p[0] += ws[(size_t)k * pstride + i];
  }
  red[sl][e] = (p[0] + p[1]) + (p[2] + p[3]);
  __syncthreads();
  if (sl == 0 && i < total) {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += red[u][e];
    if (i >= nw) {
      dbias[i - nw] = s + (accb ? dbias[i - nw] : 0.f);
    } else {
      const int n = (int)(i / ktot), kk = (int)(i - (size_t)n * ktot);
      const int tap = kk / C, c = kk - tap * C;
      if (c < Cin_w) {
        float* o = dw + ((size_t)n * Cin_row + c) * (KH * KW) + tap;
        *o = s * (scale ? *scale : 1.f) + (acc ? *o : 0.f);      // acc: gradient accumulation into a live bucket (beta = 1)
      }
    }
  }
}

#include "wgrad_tr.h"

// dbias[c] = sum over pixels of dz[pix][c] for c < C (dz channel stride zC, a multiple of one 16-byte chunk).
// Two stages (same-address fp32 atomics from ~1000 blocks serialise in L2): per-block partial sums -> part[block][zC],
// then one small kernel sums the <= BIAS_BLOCKS partials per channel.
constexpr int BIAS_BLOCKS = 512;
template <typename T>
__global__ void bias_grad_partial_kernel(const T* dz, float* part, size_t npix, int zC) {
  constexpr int V = DT<T>::EPC;
  __shared__ float red[V][256];
  const int nch = zC / V;                    // channel chunks per pixel
  int cp = 1;
  while (cp < nch && cp < 64) cp <<= 1;      // chunk lanes per block
  const int rows = 256 / cp;
  const int c_lane = threadIdx.x % cp, r_lane = threadIdx.x / cp;
  for (int ch0 = 0; ch0 < nch; ch0 += cp) {
    const int ch = ch0 + c_lane;
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    if (ch < nch)
      for (size_t p = (size_t)blockIdx.x * rows + r_lane; p < npix; p += (size_t)gridDim.x * rows) {
        float v[V];
        Vec<T, V>::ld(dz + p * zC + ch * V, v);
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += v[e];
      }
#pragma unroll
    for (int e = 0; e < V; ++e) red[e][threadIdx.x] = s[e];
    __syncthreads();
    for (int half = rows >> 1; half > 0; half >>= 1) {      // tree over the pixel lanes (rows is a power of two)
      if (r_lane < half) {
#pragma unroll
        for (int e = 0; e < V; ++e) red[e][threadIdx.x] += red[e][threadIdx.x + half * cp];
      }
      __syncthreads();
    }
    if (r_lane == 0 && ch < nch) {
#pragma unroll
      for (int e = 0; e < V; ++e) part[(size_t)blockIdx.x * zC + ch * V + e] = red[e][c_lane];
    }
    __syncthreads();
  }
}
// one block per channel: 256 threads split the partials
__global__ void bias_grad_final_kernel(const float* part, float* dbias, int nblocks, int C, int zC, int acc) {
  __shared__ float red[16];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < nblocks; k += blockDim.x) s += part[(size_t)k * zC + c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) dbias[c] = s + (acc ? dbias[c] : 0.f);
}

// one thread per (co, kk): loops over all pixels (slow; tests only)
template <typename T>
__global__ void wgrad_direct_kernel(WgradArgs a, float* dw, const float* scale_p, int Cin_w, int accum, int Cin_row) {
  const ConvGeom& g = a.g;
  const T* in1 = static_cast<const T*>(a.in1);
  const T* in2 = static_cast<const T*>(a.in2);
  const T* dz = static_cast<const T*>(a.dz);
  const size_t total = (size_t)a.N * a.ktot;
  const float scale = scale_p ? *scale_p : 1.f;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(idx / a.ktot), kk = (int)(idx - (size_t)n * a.ktot);
    const int tap = kk / g.C, c = kk - tap * g.C, ty = tap / g.KW, tx = tap - ty * g.KW;
    if (c >= Cin_w) continue;
    float acc = 0.f;
    for (int b = 0; b < g.B; ++b)
      for (int oy = 0; oy < g.OH; ++oy) {
        const int sy = src_coord(g, oy, ty, 0, g.IH, g.OH);
        if (sy < 0) continue;
        for (int ox = 0; ox < g.OW; ++ox) {
          const int sx = src_coord(g, ox, tx, 0, g.IW, g.OW);
          if (sx < 0) continue;
          const size_t pix = ((size_t)b * g.IH + sy) * g.IW + sx;
          const float xv = (c < g.C1) ? DT<T>::ld(in1 + pix * g.C1 + c) : DT<T>::ld(in2 + pix * g.C2 + (c - g.C1));
          acc += xv * DT<T>::ld(dz + (((size_t)b * g.OH + oy) * g.OW + ox) * a.zC + n);
        }
      }
    float* o = dw + ((size_t)n * Cin_row + c) * (g.KH * g.KW) + tap;
    *o = acc * scale + (accum ? *o : 0.f);
  }
}

}  // namespace uegan

using namespace uegan;

int uegan::wgrad_reduce_1x1(const float* ws, float* dw, int nsplit, int N, int C, int Cin_w, int Cin_row, size_t pstride, int acc, hipStream_t s) {
  const size_t total = (size_t)N * C;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, s, ws, dw, (float*)nullptr, (const float*)nullptr, nsplit, N, C,
                     Cin_w, 1, 1, pstride, acc, 0, Cin_row);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// everything a weight-gradient launch needs, decided once: the size query and the launcher both read it from here
struct WgradPlan {
  WgradArgs a;
  WgradTrPlan tr;
  int nsplit, bn;      // bn: block rows of conv_wgrad_kernel; -1: the transpose-read kernel, 0: the VALU head kernel
  dim3 grid;
  size_t ws_bytes;     // workspace: [nsplit][N * ktot weight partials + N bias partials], then the bias-gradient kernels' partials
};

static void wgrad_plan(const uegan_conv_desc* d, WgradPlan& p) {
  WgradArgs& a = p.a;
  a.g = fwd_geom(d);
  a.N = cout_w(d);
  a.zC = d->Cout;
  a.ktot = d->KH * d->KW * (d->C1 + d->C2);
  auto done = [&](int bn, int nsplit, dim3 grid) {
    p.bn = bn; p.nsplit = nsplit; p.grid = grid;
    p.ws_bytes = ((size_t)nsplit * ((size_t)a.N * a.ktot + a.N) + (size_t)BIAS_BLOCKS * d->Cout) * sizeof(float);
  };
  if (g_impl.impl != UEGAN_IMPL_DIRECT && wgtr_plan(d, a.g, p.tr)) return done(-1, p.tr.nsplit_eff, p.tr.grid);      // bf16 transpose-read kernel
  const int npix = d->dtype == UEGAN_BF16 ? 64 : 32;     // pixel slots per K step (128-byte LDS rows)
  int ws = 1, wl = 0;
  while (ws < d->Wo && ws < npix) { ws <<= 1; ++wl; }
  a.WS = ws; a.WSlog = wl; a.R = npix / ws;
  a.nxb = (d->Wo + ws - 1) / ws;
  a.nyb = (d->Ho + a.R - 1) / a.R;
  a.steps_total = d->B * a.nyb * a.nxb;
  if (g_impl.impl != UEGAN_IMPL_DIRECT && g_impl.heads && heads_applicable(d)) {     // VALU head kernel: one partial per block
    const int nb = heads_wgrad_blocks(d);
    return done(0, nb, dim3(nb));
  }
  const int bn = a.N <= 16 ? 16 : (a.N <= 32 ? 32 : (a.N <= 64 ? 64 : 128));
  const int tiles = ((a.ktot + WG_BK - 1) / WG_BK) * ((a.N + bn - 1) / bn);
  int want = (1536 + tiles - 1) / tiles;
  if (want < 1) want = 1;
  if (want > a.steps_total) want = a.steps_total;
  a.steps_per_split = (a.steps_total + want - 1) / want;
  const int nsplit = (a.steps_total + a.steps_per_split - 1) / a.steps_per_split;
  done(bn, nsplit, dim3((a.ktot + WG_BK - 1) / WG_BK, (a.N + bn - 1) / bn, nsplit));
}

extern "C" size_t uegan_conv2d_wgrad_workspace_bytes(const uegan_conv_desc* d) {
  if (check_desc(d)) return 0;
  WgradPlan p;
  wgrad_plan(d, p);
  return p.ws_bytes;
}

template <typename T>
static int run_wgrad(const uegan_conv_desc* d, WgradPlan& p, const float* scale, float* dw, float* dbias, int accmask, hipStream_t s) {
  WgradArgs& a = p.a;
  const int acc = accmask & 1, accb = (accmask >> 1) & 1;      // accumulate into dw / into dbias
  // the profiler's figures: 2 x MACs; elements of the two tensors read
  const double flops = 2.0 * (double)d->B * d->Ho * d->Wo * a.N * (double)a.ktot, elems = (double)d->B * d->H * d->W * (d->C1 + d->C2) + (double)d->B * d->Ho * d->Wo * d->Cout;
  // sum the splits of a.ws, scale, permute to OIHW; bias_too: N bias sums follow each split's weight sums (the transpose-read kernel's)
  auto reduce = [&](bool bias_too) {
    const size_t nw = (size_t)a.N * a.ktot, total = nw + (bias_too ? a.N : 0);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, s, a.ws, dw, bias_too ? dbias : (float*)nullptr, scale, p.nsplit,
                       a.N, a.g.C, cin_w(d), a.g.KH, a.g.KW, p.bn == -1 ? (size_t)p.tr.a.pstride : nw, acc, accb, cin_row(d));
  };
  if (g_impl.impl == UEGAN_IMPL_DIRECT) {
    const size_t total = (size_t)a.N * a.ktot;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL((wgrad_direct_kernel<T>), dim3(blocks), dim3(256), 0, s, a, dw, scale, cin_w(d), acc, cin_row(d));
  } else if (p.bn == -1) {
    WgradTrPlan& tr = p.tr;
    tr.a.in1 = a.in1; tr.a.in2 = a.in2; tr.a.dz = a.dz; tr.a.ws = a.ws;
    tr.a.want_bias = dbias ? 1 : 0;
    {
      ProfScope prof(prof_key(3, true, tr.tn, tr.tm, 0, 8, tr.big), flops, s, 2.0 * elems);
      wgtr_launch(tr, s);
      UEGAN_CHECK_LAUNCH();
    }
    reduce(dbias != nullptr);      // (the bias gradient rode along)
    UEGAN_CHECK_LAUNCH();
    return UEGAN_OK;
  } else if (p.bn == 0) {
    int rc = heads_wgrad(d, a.in1, a.dz, a.ws, s);
    if (rc) return rc;
    reduce(false);
  } else {
    {
      ProfScope prof(prof_key(2, DT<T>::kDtype == UEGAN_BF16, p.bn, 0, 0, 8, false), flops, s, sizeof(T) * elems);
      if (p.bn == 128) hipLaunchKernelGGL((conv_wgrad_kernel<T, 128>), p.grid, dim3(256), 0, s, a);
      else if (p.bn == 64) hipLaunchKernelGGL((conv_wgrad_kernel<T, 64>), p.grid, dim3(256), 0, s, a);
      else if (p.bn == 32) hipLaunchKernelGGL((conv_wgrad_kernel<T, 32>), p.grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((conv_wgrad_kernel<T, 16>), p.grid, dim3(256), 0, s, a);
      UEGAN_CHECK_LAUNCH();
    }
    reduce(false);
  }
  UEGAN_CHECK_LAUNCH();
  if (dbias) {
    const size_t npix = (size_t)d->B * d->Ho * d->Wo;
    const int nch = a.zC / DT<T>::EPC;
    int cp = 1;
    while (cp < nch && cp < 64) cp <<= 1;
    const size_t rows = 256 / cp;
    size_t blocks = (npix + rows * 8 - 1) / (rows * 8);
    if (blocks > BIAS_BLOCKS) blocks = BIAS_BLOCKS;
    if (blocks < 1) blocks = 1;
    float* part = a.ws + (size_t)p.nsplit * a.N * a.ktot;      // tail of the wgrad workspace
    hipLaunchKernelGGL((bias_grad_partial_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const T*>(a.dz), part, npix, a.zC);
    UEGAN_CHECK_LAUNCH();
    hipLaunchKernelGGL(bias_grad_final_kernel, dim3(a.N), dim3(256), 0, s, part, dbias, (int)blocks, a.N, a.zC, accb);
    UEGAN_CHECK_LAUNCH();
  }
  return UEGAN_OK;
}

extern "C" int uegan_conv2d_wgrad(const uegan_conv_desc* d, const void* x1, const void* x2, const void* dz, const float* scale,
                                  float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, uegan_stream_t stream) {
  return uegan_conv2d_wgrad_acc(d, x1, x2, dz, scale, dw_oihw, dbias, workspace, workspace_bytes, 0, stream);
}

extern "C" int uegan_conv2d_wgrad_acc(const uegan_conv_desc* d, const void* x1, const void* x2, const void* dz, const float* scale,
                                      float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, int accumulate,
                                      uegan_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  UEGAN_CHECK_ARG(x1 && dz && dw_oihw && (d->C2 == 0 || x2), "null pointer");
  WgradPlan p;
  wgrad_plan(d, p);
  UEGAN_CHECK_ARG(workspace && workspace_bytes >= p.ws_bytes, "wgrad workspace too small: %zu < %zu", workspace_bytes, p.ws_bytes);
  p.a.in1 = x1; p.a.in2 = d->C2 ? x2 : x1; p.a.dz = dz; p.a.ws = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  UEGAN_CHECK_ARG(accumulate >= 0 && accumulate <= 3, "accumulate is a bit mask: 1 = dw, 2 = dbias");
  return d->dtype == UEGAN_F32 ? run_wgrad<float>(d, p, scale, dw_oihw, dbias, accumulate, s) : run_wgrad<bf16_t>(d, p, scale, dw_oihw, dbias, accumulate, s);
}
