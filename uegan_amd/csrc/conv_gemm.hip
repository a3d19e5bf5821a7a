// The generic gather-GEMM kernel (any kernel size, stride 1 / 2, forward and data gradient: the layers no specialised kernel takes) and the
// scalar direct kernel used only for on-GPU cross-checks.  conv.hip decides the route; this unit is reached through conv_gemm_run.
#include "conv_core.h"

namespace uegan {

template <typename T, int BN, int WARPS_M, int WARPS_N, bool GLDS>
__global__ void __launch_bounds__(256) conv_gemm_kernel(ConvArgs a) {
  constexpr int BM = CONV_BM, ROWB = CONV_ROWB;
  constexpr int EPC = DT<T>::EPC;
  constexpr int BK = ROWB / (int)sizeof(T);          // reduction elements per K step
  constexpr int NI_X = BM / 32;                      // staging instructions per thread for the pixel tile (8 rows each)
  constexpr int WROWG = BN / 8;                      // 8-row groups of the weight tile
  constexpr int NI_W = (WROWG + 3) / 4;
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int NCHUNK = Mma<T>::NCHUNK;
  constexpr int NSUB = BK / 32;                      // 32-wide MFMA K sub-steps per K step (bf16: 2, fp32: 1)
  constexpr int BUFB = (BM + BN) * ROWB;
  static_assert(WARPS_M * WARPS_N == 4 && TM >= 1 && TN >= 1, "tile");

  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUFB];

  const ConvGeom& g = a.g;
  const T* in1 = static_cast<const T*>(a.in1);
  const T* in2 = static_cast<const T*>(a.in2);
  const T* w = static_cast<const T*>(a.w);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int n0 = blockIdx.y * BN;

  // ---- tile decode: (image b, parity class, tile_y, tile_x)
  const int sub = (g.mode == 1) ? g.stride : 1;      // pixel stride inside the tile (dgrad parity classes)
  int t = blockIdx.x;
  int tile_x, tile_y, pcls = 0, b;
  tile_x = t % a.ntx; t /= a.ntx;
  tile_y = t % a.nty; t /= a.nty;
  pcls = t % (sub * sub);
  b = t / (sub * sub);
  const int py = pcls / sub, px = pcls - py * sub;
  // taps this tile iterates: dgrad keeps ty with (py + pad - ty) % stride == 0
  const int ty0 = (g.mode == 1) ? (py + g.pad) % sub : 0;
  const int tx0 = (g.mode == 1) ? (px + g.pad) % sub : 0;
  const int nty_t = ty0 < g.KH ? (g.KH - ty0 + sub - 1) / sub : 0;
  const int ntx_t = tx0 < g.KW ? (g.KW - tx0 + sub - 1) / sub : 0;
  const int kvalid = nty_t * ntx_t * g.C;            // flattened (tap, channel) reduction length of this tile
  const int nk = (kvalid + BK - 1) / BK;

  // ---- staging role of this thread: LDS (row, pos) per instruction i -> row = (i*4 + wave)*8 + (lane>>3), pos = lane&7
  const int srow = lane >> 3;
  const int spos = lane & 7;
  const int sdc = spos ^ (((lane >> 4) + 4 * (wave & 1)) & 7);     // data chunk held at that position (same for every i)
  // initial (tap, channel) of my chunk: flattened offset sdc*EPC
  int tyi0, txi0, c0;
  {
    const int q = sdc * EPC;
    const int ti = q / g.C;
    c0 = q - ti * g.C;
    tyi0 = ntx_t > 0 ? ti / ntx_t : 0;
    txi0 = ntx_t > 0 ? ti - tyi0 * ntx_t : 0;
  }
  // my pixel rows
  int roy[NI_X], rox[NI_X];
  bool rv[NI_X];
#pragma unroll
  for (int i = 0; i < NI_X; ++i) {
    const int r = (i * 4 + wave) * 8 + srow;
    roy[i] = py + sub * (tile_y * CONV_TH + (r >> 4));
    rox[i] = px + sub * (tile_x * CONV_TW + (r & 15));
    rv[i] = roy[i] < g.OH && rox[i] < g.OW;
  }
  // block-uniform list of padded-space images (4 bits per entry), from the tile's coordinate range: an image is
  // listed when some row of the tile MAY have it (rows that do not simply gather nothing for it)
  unsigned long long imgs = 0;
  int nimg = 0;
  if (g.mode == 1 && g.pad_mode == UEGAN_PAD_REFLECT) {
    const int y_lo = py + sub * tile_y * CONV_TH, y_hi = py + sub * (tile_y * CONV_TH + CONV_TH - 1);
    const int x_lo = px + sub * tile_x * CONV_TW, x_hi = px + sub * (tile_x * CONV_TW + CONV_TW - 1);
    bool hy[3], hx[3];
    hy[0] = hx[0] = true;
    hy[1] = y_lo <= g.pad && y_hi >= 1;
    hy[2] = y_lo <= g.OH - 2 && y_hi >= g.OH - 1 - g.pad;
    hx[1] = x_lo <= g.pad && x_hi >= 1;
    hx[2] = x_lo <= g.OW - 2 && x_hi >= g.OW - 1 - g.pad;
    for (int q = 0; q < 9; ++q)
      if (hy[q / 3] && hx[q % 3]) {
        imgs |= (unsigned long long)q << (4 * nimg);
        ++nimg;
      }
  } else {
    nimg = 1;
  }
  const int nsteps = nimg * nk;

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // running decode state of my chunk
  int tyi = tyi0, txi = txi0, cc = c0, ks_in_img = 0, img_i = 0;
  u32x4 xreg[NI_X], wreg[NI_W];

  // gathered source pixel of my NI_X rows for the current (image, tap): recomputed only when the tap changes -- with >= 128
  // channels several consecutive K steps (1x1 convs: all of them) read the same pixels at different channel offsets
  int pixoff[NI_X];
  const T* pbase[NI_X];          // single-source tensors: in1 + pixel * C1 of the cached pixel (a K step only adds the channel offset)
  const T* wrow[NI_W];           // start of my weight rows (null: row beyond N)
#pragma unroll
  for (int i = 0; i < NI_X; ++i) pbase[i] = nullptr;
#pragma unroll
  for (int i = 0; i < NI_W; ++i) {
    const int rg = i * 4 + wave;
    const int n = n0 + rg * 8 + srow;
    wrow[i] = (rg < WROWG && n < a.N) ? w + (size_t)n * a.Kp : nullptr;
  }
  const bool one_src = g.C2 == 0;
  int pix_key = -1;
  auto stage = [&](unsigned char* buf) {
    // addresses for the current step, then advance the state by one K step
    const bool kv = tyi < nty_t;
    const int key = (img_i * 16 + tyi) * 16 + txi;
    if (key != pix_key) {
      pix_key = key;
      const int q = (int)((imgs >> (4 * img_i)) & 15ull);
      const int iy = q / 3, ix = q - iy * 3;
      const int ty = ty0 + sub * tyi, tx = tx0 + sub * txi;
#pragma unroll
      for (int i = 0; i < NI_X; ++i) {
        int off = -1;
        if (kv && rv[i]) {
          const int sy = src_coord(g, roy[i], ty, iy, g.IH, g.OH);
          const int sx = src_coord(g, rox[i], tx, ix, g.IW, g.OW);
          if (sy >= 0 && sx >= 0) off = (b * g.IH + sy) * g.IW + sx;
        }
        pixoff[i] = off;
        pbase[i] = off >= 0 ? in1 + (size_t)off * g.C1 : nullptr;
      }
    }
    const int ty = ty0 + sub * tyi, tx = tx0 + sub * txi;
#pragma unroll
    for (int i = 0; i < NI_X; ++i) {
      const void* src = g_zero16;
      if (pixoff[i] >= 0) {
        if (one_src) {
          src = pbase[i] + cc;
        } else {
          const size_t pix = (size_t)pixoff[i];
          src = (cc < g.C1) ? (const void*)(in1 + pix * g.C1 + cc) : (const void*)(in2 + pix * g.C2 + (cc - g.C1));
        }
      }
      if (GLDS) glds16(src, buf + ((i * 4 + wave) * 8) * ROWB);
      else xreg[i] = *reinterpret_cast<const u32x4*>(src);
    }
#pragma unroll
    for (int i = 0; i < NI_W; ++i) {
      const int rg = i * 4 + wave;
      if (rg < WROWG) {
        const void* src = g_zero16;
        if (kv && wrow[i]) src = wrow[i] + ((ty * g.KW + tx) * g.C + cc);
        if (GLDS) glds16(src, buf + (BM + rg * 8) * ROWB);
        else wreg[i] = *reinterpret_cast<const u32x4*>(src);
      }
    }
    // advance
    ++ks_in_img;
    if (ks_in_img == nk) {
      ks_in_img = 0; ++img_i; tyi = tyi0; txi = txi0; cc = c0;
    } else {
      cc += BK;
      while (cc >= g.C) {
        cc -= g.C;
        if (++txi == ntx_t) { txi = 0; ++tyi; }
      }
    }
  };
  auto commit = [&](unsigned char* buf) {   // register-staged mode: VGPRs -> LDS
#pragma unroll
    for (int i = 0; i < NI_X; ++i)
      *reinterpret_cast<u32x4*>(buf + ((i * 4 + wave) * 8 + srow) * ROWB + spos * 16) = xreg[i];
#pragma unroll
    for (int i = 0; i < NI_W; ++i) {
      const int rg = i * 4 + wave;
      if (rg < WROWG) *reinterpret_cast<u32x4*>(buf + (BM + rg * 8 + srow) * ROWB + spos * 16) = wreg[i];
    }
  };

  if (nsteps > 0) {
    stage(lds);
    if (!GLDS) commit(lds);
  }
  const int fr = lane & 15, fg = lane >> 4;
  for (int s = 0; s < nsteps; ++s) {
    unsigned char* cur = lds + (s & 1) * BUFB;
    unsigned char* nxt = lds + ((s + 1) & 1) * BUFB;
    __syncthreads();                       // step s staged (the compiler drains vmcnt here); buffer nxt is free again
    if (s + 1 < nsteps) stage(nxt);
#pragma unroll
    for (int ksub = 0; ksub < NSUB; ++ksub) {
      u32x4 xf[TM][NCHUNK], wf[TN][NCHUNK];
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int row = wm * WTM + j * 16 + fr;
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
          const int q = ksub * 4 + c * 4 * (NCHUNK - 1) + fg;      // data chunk index within the 128-byte row
          xf[j][c] = *reinterpret_cast<const u32x4*>(cur + row * ROWB + ((q ^ ((row >> 1) & 7)) << 4));
        }
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int row = wn * WTN + i * 16 + fr;
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
          const int q = ksub * 4 + c * 4 * (NCHUNK - 1) + fg;
          wf[i][c] = *reinterpret_cast<const u32x4*>(cur + (BM + row) * ROWB + ((q ^ ((row >> 1) & 7)) << 4));
        }
      }
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) Mma<T>::step(wf[i], xf[j], acc[i][j]);
    }
    if (!GLDS && s + 1 < nsteps) commit(nxt);
  }

  // ---- epilogue: lane holds channels n..n+3 of pixel (tile row m)
  const float scale = a.scale ? a.scale[a.scale_group ? b / a.scale_group : 0] : 1.f;
  T* out = static_cast<T*>(a.out);
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int n = n0 + wn * WTN + i * 16 + (lane >> 4) * 4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (n + r < a.nbias) bv[r] = a.bias[n + r];
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = wm * WTM + j * 16 + (lane & 15);
      const int oy = py + sub * (tile_y * CONV_TH + (m >> 4));
      const int ox = px + sub * (tile_x * CONV_TW + (m & 15));
      if (oy >= g.OH || ox >= g.OW || n >= a.N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = apply_act(acc[i][j][r] * scale + bv[r], a.act);
      const size_t pixo = ((size_t)b * g.OH + oy) * g.OW + ox;
      T* p = (a.out2 && n >= a.n_out1) ? static_cast<T*>(a.out2) + pixo * (a.N - a.n_out1) + (n - a.n_out1)
                                       : out + pixo * (a.out2 ? a.n_out1 : a.N) + n;
      store4(p, v[0], v[1], v[2], v[3]);      // channel counts are multiples of 4 (padded tensors)
    }
  }
}

template <typename T, bool GLDS>
static int launch_conv_gemm(ConvArgs& a, hipStream_t s) {
  const ConvGeom& g = a.g;
  const int sub = g.mode == 1 ? g.stride : 1;
  const int sh = (g.OH + sub - 1) / sub, sw = (g.OW + sub - 1) / sub;
  a.nty = (sh + CONV_TH - 1) / CONV_TH;
  a.ntx = (sw + CONV_TW - 1) / CONV_TW;
  const int gm = g.B * sub * sub * a.nty * a.ntx;
  if (gm == 0) return UEGAN_OK;
  dim3 block(256);
  const int bn_idx = a.N > 64 ? 3 : (a.N > 32 ? 2 : (a.N > 16 ? 1 : 0));
  const double rows = g.mode == 0 ? (double)g.B * g.OH * g.OW : (double)g.B * g.IH * g.IW;   // algorithmic MACs: conv-output pixels
  static const int kBn[4] = {16, 32, 64, 128};
  ProfScope prof(prof_key(0, DT<T>::kDtype == UEGAN_BF16, kBn[bn_idx], 0, 0, 8, GLDS), 2.0 * rows * a.N * (double)(g.KH * g.KW * g.C), s,
                 sizeof(T) * (rows * a.N + (double)g.B * g.IH * g.IW * g.C));
  const int small_grid = g_tuning[UEGAN_TUNE_SMALL_GRID];
  if (a.N > 64 && gm * ((a.N + 127) / 128) < small_grid) {         // small maps: 64-channel blocks so the grid covers the chip
    dim3 grid(gm, (a.N + 63) / 64);
    hipLaunchKernelGGL((conv_gemm_kernel<T, 64, 2, 2, GLDS>), grid, block, 0, s, a);
  } else if (a.N > 64) {
    dim3 grid(gm, (a.N + 127) / 128);
    hipLaunchKernelGGL((conv_gemm_kernel<T, 128, 2, 2, GLDS>), grid, block, 0, s, a);
  } else if (a.N > 32) {
    dim3 grid(gm, 1);
    hipLaunchKernelGGL((conv_gemm_kernel<T, 64, 2, 2, GLDS>), grid, block, 0, s, a);
  } else if (a.N > 16) {
    dim3 grid(gm, 1);
    hipLaunchKernelGGL((conv_gemm_kernel<T, 32, 4, 1, GLDS>), grid, block, 0, s, a);
  } else {
    dim3 grid(gm, 1);
    hipLaunchKernelGGL((conv_gemm_kernel<T, 16, 4, 1, GLDS>), grid, block, 0, s, a);
  }
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

// ----------------------------------------------------------------------------------------------------
// Direct (scalar) kernels: ground truth on the GPU for the MFMA path; never the default.
// ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void conv_direct_kernel(ConvArgs a) {
  const ConvGeom& g = a.g;
  const T* in1 = static_cast<const T*>(a.in1);
  const T* in2 = static_cast<const T*>(a.in2);
  const T* w = static_cast<const T*>(a.w);
  T* out = static_cast<T*>(a.out);
  const size_t total = (size_t)g.B * g.OH * g.OW * a.N;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(idx / a.N), n = (int)(idx - (size_t)m * a.N);
    const int ohw = g.OH * g.OW;
    const int b = m / ohw, r = m - b * ohw, oy = r / g.OW, ox = r - oy * g.OW;
    const float scale = a.scale ? a.scale[a.scale_group ? b / a.scale_group : 0] : 1.f;
    float acc = 0.f;
    const int nimg = (g.mode == 1 && g.pad_mode == UEGAN_PAD_REFLECT) ? 3 : 1;
    for (int iy = 0; iy < nimg; ++iy)
      for (int ix = 0; ix < nimg; ++ix)
        for (int ty = 0; ty < g.KH; ++ty) {
          const int sy = src_coord(g, oy, ty, iy, g.IH, g.OH);
          if (sy < 0) continue;
          for (int tx = 0; tx < g.KW; ++tx) {
            const int sx = src_coord(g, ox, tx, ix, g.IW, g.OW);
            if (sx < 0) continue;
            const size_t pix = ((size_t)b * g.IH + sy) * g.IW + sx;
            const T* wp = w + (size_t)n * a.Kp + (size_t)(ty * g.KW + tx) * g.C;
            for (int c = 0; c < g.C; ++c) {
              const float xv = (c < g.C1) ? DT<T>::ld(in1 + pix * g.C1 + c) : DT<T>::ld(in2 + pix * g.C2 + (c - g.C1));
              acc += xv * DT<T>::ld(wp + c);
            }
          }
        }
    float v = acc * scale + ((a.bias && n < a.nbias) ? a.bias[n] : 0.f);
    T* p = (a.out2 && n >= a.n_out1) ? static_cast<T*>(a.out2) + (size_t)m * (a.N - a.n_out1) + (n - a.n_out1)
                                     : out + (size_t)m * (a.out2 ? a.n_out1 : a.N) + n;
    DT<T>::st(p, apply_act_ext(v, a.act));
  }
}
template <typename T>
static int conv_gemm_run_t(ConvArgs& a, hipStream_t s) {
  if (g_impl.impl == UEGAN_IMPL_DIRECT) {
    const size_t total = (size_t)a.g.B * a.g.OH * a.g.OW * a.N;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL((conv_direct_kernel<T>), dim3(blocks), dim3(256), 0, s, a);
    UEGAN_CHECK_LAUNCH();
    return UEGAN_OK;
  }
  return g_impl.glds ? launch_conv_gemm<T, true>(a, s) : launch_conv_gemm<T, false>(a, s);
}
int conv_gemm_run(ConvArgs& a, int dtype, hipStream_t s) {
  return dtype == UEGAN_F32 ? conv_gemm_run_t<float>(a, s) : conv_gemm_run_t<bf16_t>(a, s);
}

}  // namespace uegan
