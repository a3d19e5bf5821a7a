// The streaming kernel's plain instantiations with their planner and launcher (conv_stream.h holds the kernel template), the fold of its
// per-channel moments, and the mirrored-image pass behind its reflection-padded data gradients.
#include "conv_stream.h"

namespace uegan {

bool conv_stream_plan(const ConvArgs& c, int dtype, ConvStreamPlan& p, int max_pf) {
  const ConvGeom& g = c.g;
  if (!g_impl.stream || dtype != UEGAN_BF16 || g.KH != g.KW || !(g.KH & 1) || g.pad != (g.KH - 1) / 2) return false;
  // hi + lo pairs / epilogue extras (uegan_conv2d_fwd_ex): plain stride-1 forwards, weights always as a pair when anything is
  int pr = 0;
  if (c.w_lo) pr = (c.in1_lo && g.C2 == 0) ? 2 : ((c.in2_lo && !c.in1_lo && g.C1 == 32 && g.C2 == 32) ? 3 : ((c.in1_lo || c.in2_lo) ? -1 : 1));
  else if (c.in1_lo || c.in2_lo) pr = -1;
  const int epx = c.mul ? 2 : (c.out_lo ? 1 : 0);
  if (c.mul && c.out_lo) return false;                                      // (no instantiation writes both)
  if (pr >= 2 && !epx) return false;                                        // (the source-pair instantiations all carry an epilogue extra)
  if (pr < 0 || ((pr || epx) && (g.mode != 0 || g.stride != 1 || c.mask || c.out2))) return false;
  if (pr >= 2 && g.pad_mode != UEGAN_PAD_REFLECT && g.pad != 0) return false;      // (the zero-filling staging path knows no lo plane)
  if (c.mul && !c.out_mul) return false;
  p.pr = pr; p.epx = epx;
  const int sx = g.stride;
  const bool cls = sx == 2 && g.mode == 1;      // data gradient of a stride-2 conv: four parity classes per tile
  if (cls) {
    if (!(g.C == 32 || g.C == 64) || g.OH != 2 * g.IH || g.OW != 2 * g.IW || g.pad_mode != UEGAN_PAD_REFLECT || g.C2 != 0) return false;
  } else if (sx == 2) {
    if (g.mode != 0 || g.OH != (g.IH + 2 * g.pad - g.KH) / 2 + 1 || g.OW != (g.IW + 2 * g.pad - g.KW) / 2 + 1) return false;
  } else if (sx != 1 || g.IH != g.OH || g.IW != g.OW) {
    return false;
  }
  if (!(g.C == 8 || g.C == 16 || g.C == 32 || g.C == 64) || c.N > 64 || c.N % 8 || (c.out2 && c.n_out1 % 8)) return false;
  if (g.C1 % 8 || g.C2 % 8) return false;
  if ((cls ? g.IH : g.OH) < 16 || (cls ? g.IW : g.OW) < 32) return false;
  ConvStreamArgs& a = p.a;
  a.c = c;
  a.abl = UEGAN_ABL_BITS(g_abl_stream);
  a.sx = cls ? 1 : sx;
  a.cls = cls ? 1 : 0;
  a.flip = g.mode == 1;
  a.org = g.mode == 1 ? g.pad - (g.KH - 1) : -g.pad;
  a.zero_fill = (g.mode == 1 || g.pad_mode != UEGAN_PAD_REFLECT) ? 1 : 0;
  a.taps = g.KH * g.KW;
  a.Clog = g.C == 8 ? 3 : (g.C == 16 ? 4 : (g.C == 32 ? 5 : 6));
  a.rb = g.C * 2;
  a.rblog = a.Clog + 1;
  a.ksteps = (a.taps * g.C + 31) / 32;
  a.KWmagic = 65536 / g.KW + 1;
  for (int tap = 0; tap < a.taps; ++tap)
    if (((tap * a.KWmagic) >> 16) != tap / g.KW) return false;
  a.wrow = a.ksteps * 64;
  // rows 64 B apart modulo the 256-byte bank row: conflict-free A reads (192 = -64 serves as well -- slot 12 n mod 16 is the same permutation of n & 3 --
  // and is what lets dec4's weight PAIR fit the LDS beside its patches; the plain launches keep the layout they were measured with)
  while (a.wrow % 256 != 64 && !(pr && a.wrow % 256 == 192)) a.wrow += 64;
  p.tn = c.N <= 16 ? 1 : (c.N <= 32 ? 2 : 4);
  a.wrows = (c.N + 7) / 8 * 8;
  if (a.wrows > p.tn * 16) a.wrows = p.tn * 16;
  a.wbytes = (a.wrows * a.wrow + 15) / 16 * 16;
  a.wlo_off = a.wbytes;
  if (pr) a.wbytes *= 2;                                             // (the lo part of the weights behind the hi matrix)
  a.tbytes = a.ksteps * 256 + (a.ksteps * 4 + 255) / 256 * 256;      // lane offsets + weight-slice offsets per K step
  // reflection-padded stride-1 data gradient on a map whose width is whole tiles: x-mirrored images inside the kernel (two more tables)
  a.xmir = (!cls && g.mode == 1 && g.pad_mode == UEGAN_PAD_REFLECT && g.pad > 0 && g.pad < 8 && g.OW % 16 == 0 && g.KW == 2 * g.pad + 1) ? 1 : 0;
  a.mtab_off = a.tbytes;
  if (a.xmir) a.tbytes += 2 * a.ksteps * 256 + (2 * a.ksteps * 4 + 255) / 256 * 256;
  if (pr && (a.xmir || cls)) return false;
  a.tlo_off = a.tbytes;
  if (pr == 3) a.tbytes += a.taps * 256;                             // the lo plane's per-tap lane offsets
  a.c_lo = pr == 2 ? g.C : (pr == 3 ? g.C2 : 0);
  a.rb_lo = a.c_lo * 2;
  a.rblog_lo = a.c_lo == 8 ? 4 : (a.c_lo == 16 ? 5 : (a.c_lo == 32 ? 6 : 7));
  a.lo_xoff = 0;
  a.PW = sx * 15 + g.KW;
  a.ymin = 0;
  int cspan = 0;
  for (int c = 0; c < 5; ++c) a.kstart[c] = 0;
  if (cls) {
    // source = i + (py + pad - t) / 2 over the taps t of class py: from (py - pad)/2 (t = K-1) up to (py + pad - t0)/2
    const int ymin = (g.pad & 1) ? (1 - g.pad) / 2 : -(g.pad / 2);
    int ymax = 0;
    for (int py = 0; py < 2; ++py) {
      const int t0 = (py + g.pad) & 1, v = (py + g.pad - t0) / 2;
      if (v > ymax) ymax = v;
    }
    a.ymin = ymin;
    cspan = ymax - ymin;
    a.PW = 16 + cspan;
    const int spt = g.C / 32;
    for (int c = 0; c < 4; ++c) {
      const int py = c >> 1, px = c & 1;
      const int nty = (g.KH - ((py + g.pad) & 1) + 1) / 2, ntx = (g.KW - ((px + g.pad) & 1) + 1) / 2;
      a.kstart[c + 1] = a.kstart[c] + nty * ntx * spt;
    }
    if (a.kstart[4] != a.ksteps) return false;
  }
  a.PWmagic = 65536 / a.PW + 1;
  p.pf = 0;
  p.lc = 1;
  for (int pass = 1; pass < (pr == 3 ? 4 : 3) && !p.pf; ++pass) {      // 80 KB (two blocks per CU) if it fits, else 152 KB (PR 3: else all 160)
    const int kb = CS_LDS_KB[pass], maxix = pass >= 2 ? 16 : 10;
    for (int pf : {4, 2}) {
      if (pf > max_pf) continue;
      const int th = 4 * pf, ph = cls ? th + cspan : sx * (th - 1) + g.KH;
      // (PR >= 2: both planes packed exactly, lanes without a chunk masked; else whole staging rounds: every lane of a round writes)
      const int xbh = pr >= 2 ? ph * a.PW * a.rb : (ph * a.PW * a.rb + 4095) / 4096 * 4096;
      const int xb = xbh + (pr >= 2 ? ph * a.PW * a.rb_lo : 0);
      if (a.wbytes + a.tbytes + 2 * xb > kb * 1024 || (xb + 4095) / 4096 > maxix) continue;
      bool ok = true;
      for (int r = 0; r < ph * a.PW && ok; ++r) ok = ((r * a.PWmagic) >> 16) == r / a.PW;
      if (!ok) continue;
      p.pf = pf; a.TH = th; a.PH = ph; a.xbytes = xb; p.lc = pass;
      if (pr >= 2) a.lo_xoff = xbh;
      break;
    }
  }
  if (!p.pf) return false;
  p.nw = 4;
  if (p.pf == 4 && (!cls || p.lc == 2) && p.lc == 2 && p.tn <= 2 && !a.xmir && !pr) {
    // the same 16-row tile on 8 waves of 2 rows each (staging rounds of 512 lanes)
    const int xb8 = (a.PH * a.PW * a.rb + 8191) / 8192 * 8192;
    if (a.wbytes + a.tbytes + 2 * xb8 <= CS_LDS_KB[p.lc] * 1024 && xb8 / 8192 <= (p.lc == 2 ? 8 : 5)) { p.nw = 8; p.pf = 2; a.xbytes = xb8; }
  }
  // pairs on one block per CU: 8 waves as well (the same tile, half the rows per wave; the planes are packed exactly, so only the round count changes):
  // dec5.0 0.96 -> 0.74 ms, dec4 2.09 -> 1.51 ms per 32 images
  if (pr >= 2 && p.lc >= 2 && p.tn <= 2 && (a.xbytes + 8191) / 8192 <= 8) { p.nw = 8; p.pf /= 2; }
  // one block per CU only pays for the thin layers: with 64 output channels (VGG conv1_2) or four parity classes per tile the
  // patch kernel measured faster
  if (p.lc == 2 && ((p.tn == 4 && sx == 1) || (cls && p.nw != 8))) return false;
  // Every tile of the map.  The data gradient of a reflection-padded conv is computed as if the padding were zeros (the direct
  // image of every pixel); the few pixels within `pad` of a border that also receive MIRRORED images get those added afterwards
  // by dgrad_images_kernel (below) -- 0.8 % of a 512^2 map for pad 1, instead of a second MFMA launch over every border tile.
  p.fixup = g.mode == 1 && g.pad_mode == UEGAN_PAD_REFLECT && g.pad > 0;
  if (p.fixup && (g.OH <= 2 * g.pad + 2 || g.OW <= 2 * g.pad + 2)) return false;
  a.ty0 = 0; a.tx0 = 0;
  a.ty1 = ((cls ? g.IH : g.OH) + a.TH - 1) / a.TH;
  a.tx1 = ((cls ? g.IW : g.OW) + 15) / 16;
  a.tiles_total = g.B * (a.ty1 - a.ty0) * (a.tx1 - a.tx0);
  const int maxb = p.lc == 2 ? 256 : 512;
  int blocks = a.tiles_total < maxb ? a.tiles_total : maxb;
  a.tiles_per_block = (a.tiles_total + blocks - 1) / blocks;
  p.blocks = (a.tiles_total + a.tiles_per_block - 1) / a.tiles_per_block;
  if ((pr || epx) && !conv_stream_ex_available(p)) return false;      // (a handful of instantiations: the generator's full-resolution layers)
  return true;
}

template <int TN, int PF>
static void conv_stream_launch2(const ConvStreamPlan& p, hipStream_t s) {
  const int blocks = p.blocks;
  if (p.a.cls) {        // parity-class data gradient: own instantiation, so the plain kernel keeps its straight-line K loop
    if constexpr (PF == 2 && TN <= 2) {
      if (p.nw == 8) {
        hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 2, true, false, 8>), dim3(blocks), dim3(512), 0, s, p.a);
        return;
      }
    }
    if (p.lc == 2) hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 2, true>), dim3(blocks), dim3(256), 0, s, p.a);
    else hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, true>), dim3(blocks), dim3(256), 0, s, p.a);
    return;
  }
  if constexpr (PF == 2 && TN <= 2) {
    if (p.nw == 8) {
      if (p.a.xmir) hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, false, true, 8>), dim3(blocks), dim3(512), 0, s, p.a);
      else if (p.lc == 2) hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 2, false, false, 8>), dim3(blocks), dim3(512), 0, s, p.a);
      else hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, false, false, 8>), dim3(blocks), dim3(512), 0, s, p.a);
      return;
    }
  }
  if (p.stats) {        // (forward with per-channel sums; conv_stream_stats_ok: 4 waves, 80-KB class, no mirrors, >= 32 output channels)
    if constexpr (TN >= 2) {
      hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, false, false, 4, true>), dim3(blocks), dim3(256), 0, s, p.a);
      return;
    }
  }
  if (p.a.xmir) {       // (own instantiation: the forward kernels keep their register budget)
    if (p.lc == 2) hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 2, false, true>), dim3(blocks), dim3(256), 0, s, p.a);
    else hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, false, true>), dim3(blocks), dim3(256), 0, s, p.a);
    return;
  }
  if (p.lc == 2) hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 2, false>), dim3(blocks), dim3(256), 0, s, p.a);
  else hipLaunchKernelGGL((conv_stream_kernel<TN, PF, 1, false>), dim3(blocks), dim3(256), 0, s, p.a);
}
// can this planned launch carry the per-channel sums?  (a block's tile range must span at most two images)
bool conv_stream_stats_ok(const ConvStreamPlan& p) {
  const ConvGeom& g = p.a.c.g;
  const int tpi = (p.a.ty1 - p.a.ty0) * (p.a.tx1 - p.a.tx0);
  return g.mode == 0 && !p.a.cls && !p.a.xmir && p.nw == 4 && p.lc == 1 && !p.a.c.out2 && !p.a.c.mask && p.a.tiles_per_block <= tpi && p.tn >= 2;
}
void conv_stream_launch(const ConvStreamPlan& p, hipStream_t s) {
  if (p.pr || p.epx) {
    (void)conv_stream_launch_ex(p, s);      // (the planner's caller checked conv_stream_ex_available)
    return;
  }
  if (p.tn == 1 && p.pf == 4) conv_stream_launch2<1, 4>(p, s);
  else if (p.tn == 1) conv_stream_launch2<1, 2>(p, s);
  else if (p.tn == 2 && p.pf == 4) conv_stream_launch2<2, 4>(p, s);
  else if (p.tn == 2) conv_stream_launch2<2, 2>(p, s);
  else if (p.pf == 4) conv_stream_launch2<4, 4>(p, s);
  else conv_stream_launch2<4, 2>(p, s);
}
}  // namespace uegan

using namespace uegan;

// The moments of a forward's result (uegan_conv2d_fwd_stats, uegan_conv2d_fwd_ex): conv_stream_kernel<..., STATS> accumulates sum / sum of
// squares of its fp32 results on the way out and stream_stats_finalize_kernel folds the per-(block, image, wave) partials in a fixed order into
// mean[b][c] and rstd[b][c] = 1 / sqrt(biased variance + eps) (eps < 0: the variance itself).
__global__ void __launch_bounds__(256) stream_stats_finalize_kernel(const float* part, float* mean_out, float* rstd_out, int B, int C, int Cs, int HW,
                                                                    int tpi, int tpb, int NW, float eps) {
  // one BLOCK per (b, c): at batch 1 an image is spread over all 512 blocks of the forward (2048 partials per channel); fixed summation order
  __shared__ float red[16];
  const int w = blockIdx.x;
  const int b = w / C, c = w - b * C;
  const int k0 = (b * tpi) / tpb, k1 = ((b + 1) * tpi - 1) / tpb;      // blocks whose tile range touches image b
  const int n = (k1 - k0 + 1) * NW;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += 256) {
    const int k = k0 + i / NW, wv = i - (i / NW) * NW;
    const int j = b - (k * tpb) / tpi;                                 // image index inside block k's range (0 or 1)
    const float* o = part + ((size_t)((k * 2 + j) * NW + wv) * Cs + c) * 2;
    s1 += o[0]; s2 += o[1];
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    const float m = s1 / (float)HW;
    float var = s2 / (float)HW - m * m;
    var = var > 0.f ? var : 0.f;
    mean_out[w] = m;
    rstd_out[w] = eps < 0.f ? var : 1.f / sqrtf(var + eps);
  }
}

static int stream_tpi(const ConvStreamPlan& p) { return (p.a.ty1 - p.a.ty0) * (p.a.tx1 - p.a.tx0); }      // tiles per image
size_t uegan::conv_stream_stats_bytes(const ConvStreamPlan& p) { return (size_t)p.blocks * 2 * p.nw * (p.tn * 16) * 2 * sizeof(float); }
void uegan::conv_stream_stats_arm(ConvStreamPlan& p, void* workspace) {
  p.a.c.stats_part = static_cast<float*>(workspace);
  p.a.c.stats_tpi = stream_tpi(p);
  p.stats = true;
}
int uegan::conv_stream_stats_finalize(const ConvStreamPlan& p, float* mean, float* rstd, float eps, hipStream_t s) {
  const ConvArgs& c = p.a.c;      // (padding channels: exact zeros in y, mean 0 and rstd 1 / sqrt(eps): what uegan_moments reports for them)
  hipLaunchKernelGGL(stream_stats_finalize_kernel, dim3(c.g.B * c.N), dim3(256), 0, s, (const float*)c.stats_part, mean, rstd, c.g.B, c.N, p.tn * 16,
                     c.g.OH * c.g.OW, stream_tpi(p), p.a.tiles_per_block, p.nw, eps);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

ProfScope uegan::conv_stream_prof(const ConvStreamPlan& p, int mode, hipStream_t s) {
  const ConvArgs& c = p.a.c;
  const ConvGeom& g = c.g;
  const int npl = 1 + (c.in1_lo || c.in2_lo ? 1 : 0) + (c.w_lo ? 1 : 0);      // MFMA passes per operand pair
  return ProfScope(prof_key(4, true, p.tn, p.pf, mode, 8, p.lc >= 2), 2.0 * npl * (double)p.a.tiles_total * p.a.TH * 16 * c.N * (double)(g.KH * g.KW * g.C), s,
                   2.0 * ((double)g.B * g.OH * g.OW * c.N * (1 + (c.out_lo ? 1 : 0) + (c.mul ? 2 : 0) + (c.out_mul_lo ? 1 : 0) + (c.mul_lo ? 1 : 0)) +
                          (double)g.B * g.IH * g.IW * (g.C + p.a.c_lo)));
}

// ----------------------------------------------------------------------------------------------------
// Mirrored images of a reflection-padded data gradient, for the pixels that have any (the adjoint of nn.ReflectionPad2d,
// models.py:80): dx[o] += sum over the image pairs (iy, ix) != (0, 0) of sum_{taps, c} dz[src] * w.  Only pixels in rows
// 1..pad / OH-1-pad..OH-2 or the same columns have images -- 4 lines of a map for pad 1.  The streaming kernel has already
// written the direct image of EVERY pixel; this kernel reads, adds and writes back the affected ones (VALU: a few thousand MACs
// per pixel, <= 1 % of the pixels).  One thread = one affected pixel x one 16-byte chunk of output channels.
// ----------------------------------------------------------------------------------------------------
// per axis: the taps of output coordinate o that reach its direct image (img 0) and its (at most one) mirrored image -- see
// src_coord: t = t0, t0 + stride, ... (n of them), source (q - t) / stride.  A mirrored image only sees the <= pad taps that
// cross the border.
struct AxisTaps {
  int n0, t00, q0;     // direct image
  int n1, t01, q1;     // mirrored image (n1 = 0: none)
};
__device__ __forceinline__ void axis_range(const ConvGeom& g, int pp, int in_n, int K, int& n, int& t0, int& q) {
  q = pp + g.pad;                                   // t2 = q - t >= 0, (q - t) % stride == 0, (q - t) / stride <= in_n - 1
  int t1 = q < K - 1 ? q : K - 1;
  t0 = q - g.stride * (in_n - 1);
  if (t0 < 0) t0 = 0;
  if (g.stride == 2 && ((q - t0) & 1)) ++t0;
  n = t1 >= t0 ? (t1 - t0) / g.stride + 1 : 0;
}
__device__ __forceinline__ AxisTaps axis_taps(const ConvGeom& g, int o, int in_n, int out_n, int K) {
  AxisTaps r;
  axis_range(g, o, in_n, K, r.n0, r.t00, r.q0);
  r.n1 = 0; r.t01 = 0; r.q1 = 0;
  if (o >= 1 && o <= g.pad) axis_range(g, -o, in_n, K, r.n1, r.t01, r.q1);
  else if (o >= out_n - 1 - g.pad && o <= out_n - 2) axis_range(g, 2 * (out_n - 1) - o, in_n, K, r.n1, r.t01, r.q1);
  return r;
}
// j-th (tap, source) of an axis: direct taps first, then the mirrored image's
__device__ __forceinline__ void axis_pick(const ConvGeom& g, const AxisTaps& r, int j, int& t, int& src) {
  if (j < r.n0) { t = r.t00 + j * g.stride; src = (r.q0 - t) / g.stride; }
  else { t = r.t01 + (j - r.n0) * g.stride; src = (r.q1 - t) / g.stride; }
}

// ONE WAVE per affected pixel.  Work units = (tap pair with at least one mirrored axis) x (16-byte chunk of dz channels); lane =
// (chunk of output channels) + NCH * part: the 64 / NCH parts share the units round-robin, partial sums meet through shuffles, the
// part-0 lanes add them into dx.  (A thread-per-pixel loop was a chain of dependent HBM round trips: 170-280 us per launch.)
// rows_only: the x-mirrored images of the direct rows were added inside the streaming kernel (conv_stream.h XMIR); what is left are
// the y-mirrored images (with any x image) of rows 1..pad / OH-1-pad..OH-2 -- whole, contiguous rows.
template <typename T>
__global__ void __launch_bounds__(256) dgrad_images_kernel(ConvArgs a, int n_aff, int nch_log, int rows_only, int multi) {
  constexpr int E = DT<T>::EPC;
  const ConvGeom& g = a.g;
  const int lane = threadIdx.x & 63;
  // multi: a wave takes 64 / nch pixels, every lane the whole unit list of its pixel (no partial sums to shuffle) -- the thin layers' units are
  // so few (3-21 taps x 1-4 dz chunks) that one wave per pixel was bound by wave launches (10^5 waves of a few loads each)
  const size_t wv = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t wid = multi ? wv * (size_t)(64 >> nch_log) + (size_t)(lane >> nch_log) : wv;
  if (wid >= (size_t)g.B * n_aff) return;              // (wave-uniform unless multi; nothing below needs the whole wave then)
  const int q = (int)(wid % n_aff), b = (int)(wid / n_aff);
  const int nyr = 2 * g.pad, nxc = 2 * g.pad;
  int y, x;
  if (q < nyr * g.OW) {                                // whole rows 1..pad and OH-1-pad..OH-2
    const int ri = q / g.OW;
    x = q - ri * g.OW;
    y = ri < g.pad ? 1 + ri : g.OH - 1 - g.pad + (ri - g.pad);
  } else {                                             // the remaining rows: columns 1..pad and OW-1-pad..OW-2
    const int q2 = q - nyr * g.OW;
    const int rr = q2 / nxc, ci = q2 - rr * nxc;
    const int nrest = g.OH - nyr;
    y = rr == 0 ? 0 : (rr == nrest - 1 ? g.OH - 1 : g.pad + rr);
    x = ci < g.pad ? 1 + ci : g.OW - 1 - g.pad + (ci - g.pad);
  }
  const AxisTaps ay = axis_taps(g, y, g.IH, g.OH, g.KH), ax = axis_taps(g, x, g.IW, g.OW, g.KW);
  const int nx = ax.n0 + ax.n1;
  const int items = ay.n1 * nx + (rows_only ? 0 : ay.n0 * ax.n1);        // (mirrored y) x (all x)  +  (direct y) x (mirrored x)
  const int kc = g.C / E;
  const int nch = 1 << nch_log, nparts = multi ? 1 : 64 >> nch_log;
  const int mych = lane & (nch - 1), part = multi ? 0 : lane >> nch_log;
  const int n0 = mych * E;
  const T* dz = static_cast<const T*>(a.in1);
  const T* w = static_cast<const T*>(a.w);
  float acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = 0.f;
  const bool nvalid = n0 < a.N;
  // the value to add to (and the deferred-activation mask): loaded up front by the lanes that will write, so that this round trip
  // overlaps the gathers below (a wave lives for a handful of dependent memory round trips: their number is its run time)
  const size_t pixo = ((size_t)b * g.OH + y) * g.OW + x;
  T* p = (a.out2 && n0 >= a.n_out1) ? static_cast<T*>(a.out2) + pixo * (a.N - a.n_out1) + (n0 - a.n_out1)
                                    : static_cast<T*>(a.out) + pixo * (a.out2 ? a.n_out1 : a.N) + n0;
  const bool writer = part == 0 && nvalid;
  typedef typename std::conditional<sizeof(T) == 2, u32x4, f32x4>::type chunk_t;      // one 16-byte chunk, still packed
  chunk_t curp = {}, mkp = {};
  if (writer) {
    curp = *reinterpret_cast<const chunk_t*>(p);
    if (a.mask) mkp = *reinterpret_cast<const chunk_t*>(static_cast<const T*>(a.mask) + pixo * a.N + n0);
  }
  for (int u = part; u < items * kc; u += nparts) {
    const int it = u / kc, c = (u - it * kc) * E;
    int jy, jx;
    if (it < ay.n1 * nx) { jy = ay.n0 + it / nx; jx = it % nx; }
    else { const int i2 = it - ay.n1 * nx; jy = i2 / ax.n1; jx = ax.n0 + i2 % ax.n1; }
    int ty, sy, tx, sx;
    axis_pick(g, ay, jy, ty, sy);
    axis_pick(g, ax, jx, tx, sx);
    const T* zp = dz + (((size_t)b * g.IH + sy) * g.IW + sx) * g.C + c;
    const T* wp = w + (size_t)(nvalid ? n0 : 0) * a.Kp + (size_t)(ty * g.KW + tx) * g.C + c;
    // E + 1 unconditional 16-byte loads in flight together, kept packed until used (registers = resident waves = throughput here)
    chunk_t zq = *reinterpret_cast<const chunk_t*>(zp), wq[E];
#pragma unroll
    for (int e = 0; e < E; ++e) wq[e] = *reinterpret_cast<const chunk_t*>(wp + (size_t)e * a.Kp);
    float zv[E];
    Vec<T, E>::ld(reinterpret_cast<const T*>(&zq), zv);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float wv[E];
      Vec<T, E>::ld(reinterpret_cast<const T*>(&wq[e]), wv);
#pragma unroll
      for (int k = 0; k < E; ++k) acc[e] = fmaf(zv[k], wv[k], acc[e]);
    }
  }
  if (!multi)
    for (int o = 32; o >= nch; o >>= 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    }
  if (!writer) return;
  const float scale = a.scale ? a.scale[a.scale_group ? b / a.scale_group : 0] : 1.f;
  float cur[E];
  Vec<T, E>::ld(reinterpret_cast<const T*>(&curp), cur);
  if (a.mask) {
    float mv[E];
    Vec<T, E>::ld(reinterpret_cast<const T*>(&mkp), mv);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] *= act_grad_from_out(mv[e], a.mask_act);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) cur[e] += acc[e] * scale;
  Vec<T, E>::st(p, cur);
}

template <typename T>
static int launch_dgrad_images_t(ConvArgs& a, hipStream_t s, bool rows_only) {
  const ConvGeom& g = a.g;
  const int n_aff = 2 * g.pad * g.OW + (rows_only ? 0 : (g.OH - 2 * g.pad) * 2 * g.pad);
  const int chunks = a.N / DT<T>::EPC;               // <= 8 for the layers the streaming kernel takes (N <= 64)
  int nch_log = 0;
  while ((1 << nch_log) < chunks) ++nch_log;
  UEGAN_CHECK_ARG(nch_log <= 6 && g.C % DT<T>::EPC == 0, "dgrad_images: unsupported channel counts");
  const int multi = nch_log <= 3 ? 1 : 0;      // (<= 8 output chunks: >= 8 pixels per wave)
  const size_t waves = multi ? ((size_t)g.B * n_aff + (64 >> nch_log) - 1) / (64 >> nch_log) : (size_t)g.B * n_aff;
  hipLaunchKernelGGL((dgrad_images_kernel<T>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a, n_aff, nch_log, rows_only ? 1 : 0, multi);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
int uegan::launch_dgrad_images(ConvArgs& a, int dtype, hipStream_t s, bool rows_only) {
  return dtype == UEGAN_F32 ? launch_dgrad_images_t<float>(a, s, rows_only) : launch_dgrad_images_t<bf16_t>(a, s, rows_only);
}
