// One-pass backward of a full-resolution attention module y = IN(W x) (models.py:230-237 after the exact shortcut of uegan_amd/models.py: GAM)
// together with the activation backward of x's producer.  x is [B][HW][C] with C = 32 or 64 in the 16-bit storage format; at the generator's
// 512^2 / 256^2 maps nothing survives in the last-level cache between kernels, so every stand-alone pass is an HBM pass.  The passes replaced:
//
//   instnorm_bwd_apply (g, y -> dz)    1x1 data gradient (dz -> dx)    1x1 weight gradient (dz, x -> dW)    act_bwd (dx, add1, add2, x -> out)
//
// After the two sums of the InstanceNorm backward (instnorm_bwd_partial_kernel + sums_finalize_kernel, unchanged: the means must exist before dz
// does) everything is work on one pixel at a time with a C x C matrix, so ONE streaming kernel reads g, y, x, add1, add2 once and writes
//
//   dz  = rstd (g - mean g - y mean(g y))           fp32, rounded to the storage format: the value instnorm_bwd_apply_kernel stores, so both
//                                                    MFMA products see the operands the separate kernels see
//   out = (add1 + add2 + W^T dz) act'(x)            W^T dz rounded to the storage format before the fp32 sum, as the stand-alone data gradient stores it:
//                                                    out is then the value the separate passes give (same roundings, same order of the sum)
//   dW  = sum_pixels dz x^T                         per-block fp32 partials in registers over the block's whole tile range -> wgrad_reduce_kernel
//
// Block = 256 threads, tile = 512 sixteen-byte chunks (128 pixels at C = 32, 64 at C = 64): a thread owns the same channel chunk of two pixels, so
// its 24 per-(image, channel) constants are re-fetched (into LDS) only when the block's tile range crosses into the next image.
//   * every global access is a whole contiguous NHWC row, 16 bytes per lane (the pattern of the project's 5+ TB/s elementwise passes)
//   * the operands of tile t+1 are loaded into registers before tile t is multiplied; nothing is loaded in the epilogue (add1, add2 and x wait
//     in registers from the tile's one load)
//   * dz and x tiles sit pixel-major in LDS (rows XOR-swizzled like wgrad_tr.h's).  Data gradient: D[ci][pixel] = W^T[ci][co] dz[pixel][co], W^T
//     fragments (the IHWO pack's rows) in registers for the whole kernel, dz fragments are plain 16-byte row reads; the D layout gives a lane 4
//     consecutive channels of one pixel, which go through a padded fp32 LDS tile back to the row owners.  Weight gradient: contraction over
//     pixels, both fragments by the LDS transpose read
//   * deterministic: the grid follows from the shape (and the workspace the caller was told to bring), blocks take contiguous tile ranges in
//     image order, a wave owns whole 16 x 16 tiles of dW (no fold inside the block), the partials are summed by wgrad_reduce_kernel in a fixed
//     order; no float atomics
#include "conv_core.h"

namespace uegan {

struct GamBwdArgs {
  const bf16_t *g, *y, *x, *add1, *add2, *w;      // w: IHWO [ci][co], row length C
  const float* rstd;                              // [B * C]
  const float* tot;                               // [B * C][2]: {sum g, sum g y}
  bf16_t* out;
  float* ws;                                      // [blocks][C * C] weight-gradient partials, [co][ci]
  int HW, act;
  int tiles_per_img, tiles_total, tiles_per_block;
  float inv_n;
};

template <int C>
__global__ void __launch_bounds__(256, C == 64 ? 2 : 3) gam_bwd_kernel(GamBwdArgs a) {
  constexpr int CH = C / 8;                   // 16-byte chunks per pixel row
  constexpr int TP = 512 / CH;                // pixels per tile
  constexpr int PPI = 256 / CH;               // pixels per 256-lane round: a thread owns pixels prow and prow + PPI of the tile
  constexpr int RB = 2 * C;                   // LDS bytes per pixel row of the dz / x tiles
  constexpr int DRB = 4 * C + 16;             // ... of the fp32 data-gradient tile (padded: the 16 pixels a store instruction covers hit distinct banks)
  constexpr int MT = C / 16, KD = C / 32;     // data gradient: 16-channel output tiles, 32-channel k-steps
  constexpr int NPT = TP / 64;                // ... 16-pixel tiles per wave
  constexpr int TM = C == 64 ? 4 : 1;         // weight gradient: 16 x 16 tiles per wave (C = 64: dz tile `wave` x all x tiles; C = 32: one of the four)
  constexpr int KW = TP / 32;                 // ... 32-pixel k-steps per tile
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * TP * RB + TP * DRB];
  unsigned char* const zs = lds;
  unsigned char* const xs = lds + TP * RB;
  unsigned char* const ds = lds + 2 * TP * RB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cq = tid % CH, prow = tid / CH;

  // ---- per-lane fragment addresses (tile independent) ----
  // weight gradient, supplier role of the transpose read: pixel pk (+ 8 for the second half) of a 32-pixel k-step, 4 channels from 4 * seg
  const int g4 = lane >> 4, sj = (lane & 15) >> 2, seg = lane & 3;
  const int pk = sj + 4 * (g4 & 1) + 16 * (g4 >> 1);
  auto tr_addr = [&](int ch) { return pk * RB + ((((ch >> 3) ^ wgtr_swz(RB, pk))) << 4) + ((ch >> 2) & 1) * 8; };
  const int co_t = C == 64 ? wave : (wave >> 1), ci_t0 = C == 64 ? 0 : (wave & 1);
  const int zaddr = tr_addr(co_t * 16 + 4 * seg);
  int xaddr[TM];
#pragma unroll
  for (int m = 0; m < TM; ++m) xaddr[m] = tr_addr((ci_t0 + m) * 16 + 4 * seg);
  // data gradient: W^T fragments A[ci = 16 mt + (lane & 15)][co = 32 ks + 8 (lane >> 4) + e]
  u32x4 wf[MT][KD];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ks = 0; ks < KD; ++ks) wf[mt][ks] = *reinterpret_cast<const u32x4*>(a.w + (mt * 16 + (lane & 15)) * C + ks * 32 + 8 * g4);

  f32x4 accw[TM];
#pragma unroll
  for (int m = 0; m < TM; ++m) accw[m] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int t_begin = blockIdx.x * a.tiles_per_block;
  int t_end = t_begin + a.tiles_per_block;
  if (t_end > a.tiles_total) t_end = a.tiles_total;

  struct Operands { u32x4 g[2], y[2], x[2], a1[2], a2[2]; };
  const u32x4 zero4 = u32x4{0u, 0u, 0u, 0u};
  auto load = [&](int t, Operands& o) {
    const int b = t / a.tiles_per_img, p0 = (t - b * a.tiles_per_img) * TP;
    const size_t base = ((size_t)b * a.HW + p0) * C + cq * 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int p = it * PPI + prow;
      const size_t off = base + (size_t)p * C;
      const bool valid = p0 + p < a.HW;
      o.g[it] = o.y[it] = o.x[it] = o.a1[it] = o.a2[it] = zero4;
      if (valid) {
        o.g[it] = *reinterpret_cast<const u32x4*>(a.g + off);
        o.y[it] = *reinterpret_cast<const u32x4*>(a.y + off);
        o.x[it] = *reinterpret_cast<const u32x4*>(a.x + off);
        if (a.add1) o.a1[it] = *reinterpret_cast<const u32x4*>(a.add1 + off);
        if (a.add2) o.a2[it] = *reinterpret_cast<const u32x4*>(a.add2 + off);
      }
    }
  };

  Operands cur;
  if (t_begin < t_end) load(t_begin, cur);
  __shared__ __attribute__((aligned(16))) float cst[3][C];      // mean g, mean(g y), rstd of the current image (24 registers per thread otherwise)
  int b_have = -1;
  for (int t = t_begin; t < t_end; ++t) {
    const int b = t / a.tiles_per_img, p0 = (t - b * a.tiles_per_img) * TP;
    if (b != b_have) {      // the range crossed into the next image: its means and rstd (every wave is past the previous tile's reads of them)
      b_have = b;
      if (tid < C) {
        const size_t i = (size_t)b * C + tid;
        cst[0][tid] = a.tot[i * 2] * a.inv_n; cst[1][tid] = a.tot[i * 2 + 1] * a.inv_n; cst[2][tid] = a.rstd[i];
      }
      __syncthreads();
    }
    float m0[8], m1[8], rs[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(&cst[0][cq * 8 + 4 * h]), v1 = *reinterpret_cast<const f32x4*>(&cst[1][cq * 8 + 4 * h]);
      const f32x4 v2 = *reinterpret_cast<const f32x4*>(&cst[2][cq * 8 + 4 * h]);
#pragma unroll
      for (int e = 0; e < 4; ++e) { m0[4 * h + e] = v0[e]; m1[4 * h + e] = v1[e]; rs[4 * h + e] = v2[e]; }
    }
    // ---- dz in registers, dz and x tiles to LDS ----
    u32x4 xk[2], a1k[2], a2k[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int p = it * PPI + prow;
      u32x4 dz = zero4;
      if (p0 + p < a.HW) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const float g0 = half_lo_to_f32(cur.g[it][d]), g1 = half_hi_to_f32(cur.g[it][d]);
          const float y0 = half_lo_to_f32(cur.y[it][d]), y1 = half_hi_to_f32(cur.y[it][d]);
          dz[d] = pack_bf16x2(rs[2 * d] * (g0 - m0[2 * d] - y0 * m1[2 * d]), rs[2 * d + 1] * (g1 - m0[2 * d + 1] - y1 * m1[2 * d + 1]));
        }
      }
      const int la = p * RB + ((cq ^ wgtr_swz(RB, p)) << 4);
      *reinterpret_cast<u32x4*>(zs + la) = dz;
      *reinterpret_cast<u32x4*>(xs + la) = cur.x[it];      // (pixels beyond the image: zeros, so they add nothing to dW)
      xk[it] = cur.x[it]; a1k[it] = cur.a1[it]; a2k[it] = cur.a2[it];
    }
    if (t + 1 < t_end) load(t + 1, cur);      // in flight while this tile is multiplied
    __syncthreads();
    // ---- weight gradient: accw[m] += dz^T[co tile][32 pixels] x[32 pixels][ci tile] ----
    // (every 32-pixel k-step is summed from zero and the k-steps are added pairwise before they join the running sums: an addend is rounded at the
    // magnitude of a k-step's sum, not the total's, and the chain of dependent additions stays short)
    u32x4 af[KW];
#pragma unroll
    for (int ks = 0; ks < KW; ++ks) {
      const u32x2 zl = lds_read_tr16(zs + ks * 32 * RB + zaddr), zh = lds_read_tr16(zs + ks * 32 * RB + zaddr + 8 * RB);
      af[ks] = u32x4{zl.x, zl.y, zh.x, zh.y};
    }
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      f32x4 part[KW];
#pragma unroll
      for (int ks = 0; ks < KW; ++ks) {
        const u32x2 xl = lds_read_tr16(xs + ks * 32 * RB + xaddr[m]), xh = lds_read_tr16(xs + ks * 32 * RB + xaddr[m] + 8 * RB);
        part[ks] = mfma_bf16(af[ks], u32x4{xl.x, xl.y, xh.x, xh.y}, f32x4{0.f, 0.f, 0.f, 0.f});
      }
      if constexpr (KW == 4) accw[m] += (part[0] + part[1]) + (part[2] + part[3]);
      else accw[m] += part[0] + part[1];
    }
    // ---- data gradient: D[ci][pixel] = sum_co W^T[ci][co] dz[pixel][co] -> fp32 tile [pixel][ci] ----
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int px = (wave + 4 * j) * 16 + (lane & 15);
      f32x4 accd[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) accd[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KD; ++ks) {
        const u32x4 bf = *reinterpret_cast<const u32x4*>(zs + px * RB + (((ks * 4 + g4) ^ wgtr_swz(RB, px)) << 4));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) accd[mt] = mfma_bf16(wf[mt][ks], bf, accd[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4*>(ds + px * DRB + (mt * 16 + 4 * g4) * 4) = accd[mt];
    }
    __syncthreads();
    // ---- epilogue: back to the row owners, + add1 + add2, act'(x), one 16-byte store per chunk ----
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int p = it * PPI + prow;
      if (p0 + p >= a.HW) continue;
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(ds + p * DRB + cq * 32), d1 = *reinterpret_cast<const f32x4*>(ds + p * DRB + cq * 32 + 16);
      float v[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
      u32x4 o;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        // (W^T dz rounded to the storage format first, then + add1 + add2 in that order: what the stand-alone data gradient stores and act_bwd_kernel
        // sums, so dz_enc is the value the separate passes give, not merely one close to it)
        const unsigned int vr = pack_bf16x2(v[2 * d], v[2 * d + 1]);
        float lo = half_lo_to_f32(vr), hi = half_hi_to_f32(vr);
        if (a.add1) { lo += half_lo_to_f32(a1k[it][d]); hi += half_hi_to_f32(a1k[it][d]); }
        if (a.add2) { lo += half_lo_to_f32(a2k[it][d]); hi += half_hi_to_f32(a2k[it][d]); }
        if (a.act == UEGAN_ACT_LRELU) {
          lo = half_lo_to_f32(xk[it][d]) > 0.f ? lo : 0.2f * lo;
          hi = half_hi_to_f32(xk[it][d]) > 0.f ? hi : 0.2f * hi;
        }
        o[d] = pack_bf16x2(lo, hi);
      }
      *reinterpret_cast<u32x4*>(a.out + ((size_t)b * a.HW + p0 + p) * C + cq * 8) = o;
    }
    // (the next tile's dz / x writes need no barrier: every wave finished its fragment reads before the second barrier above; its D writes come
    // after that tile's first barrier, which every wave reaches only after this epilogue)
  }
  // ---- weight-gradient partial of this block: [co][ci] ----
  float* ws = a.ws + (size_t)blockIdx.x * C * C;
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) ws[(co_t * 16 + g4 * 4 + r) * C + (ci_t0 + m) * 16 + (lane & 15)] = accw[m][r];
}

// the persistent grid: as many blocks as stay resident on the MI355X's 256 CUs (three per CU at C = 32, two at C = 64, where the kernel needs more than
// 168 registers).  It depends on the shape only, never on the device
static int gam_blocks(int C) {
#if defined(UEGAN_EMU)
  return 8;        // (CPU emulator: every block is 256 fibers -- same code path, CI-sized grids)
#else
  return C == 64 ? 512 : 768;
#endif
}

struct GamPlan {
  int tiles_per_img, tiles_total, blocks;      // blocks: the default grid
  size_t red_floats;                           // the scratch of the InstanceNorm sums in front of the weight-gradient partials
};

static bool gam_plan(int dtype, int B, int HW, int C, int act, GamPlan& p) {
  if (dtype != UEGAN_BF16 || (C != 32 && C != 64) || B <= 0 || HW <= 0) return false;
  if (act != UEGAN_ACT_NONE && act != UEGAN_ACT_LRELU) return false;
  const int tp = 512 / (C / 8);
  p.tiles_per_img = (HW + tp - 1) / tp;
  if ((long long)B * p.tiles_per_img > (1 << 30)) return false;
  p.tiles_total = B * p.tiles_per_img;
  p.blocks = p.tiles_total < gam_blocks(C) ? p.tiles_total : gam_blocks(C);
  p.red_floats = (uegan_reduce_workspace_floats(B, HW, C) + 3) / 4 * 4;
  return true;
}
// the grid for a block cap: contiguous ranges of equal length, no empty block
static void gam_grid(const GamPlan& p, int cap, int& blocks, int& per_block) {
  if (cap > p.blocks) cap = p.blocks;
  if (cap < 1) cap = 1;
  per_block = (p.tiles_total + cap - 1) / cap;
  blocks = (p.tiles_total + per_block - 1) / per_block;
}

}  // namespace uegan

using namespace uegan;

extern "C" size_t uegan_gam_bwd_ws_bytes(int dtype, int B, int HW, int C, int act) {
  const int knob = g_tuning[UEGAN_TUNE_GAM_BWD];
  GamPlan p;
  if (knob == 0 || !gam_plan(dtype, B, HW, C, act, p)) return 0;
  int blocks, per_block;
  gam_grid(p, knob >= 2 ? knob : p.blocks, blocks, per_block);
  return (p.red_floats + (size_t)blocks * C * C) * sizeof(float);
}

extern "C" int uegan_gam_bwd(int dtype, const void* g, const void* y, const void* x, const float* rstd, const void* w_ihwo, const void* add1,
                             const void* add2, int act, void* dz_enc, float* dw, int Cin_row, int Cin_w, int accumulate, void* workspace,
                             size_t workspace_bytes, int B, int HW, int C, uegan_stream_t stream) {
  GamPlan p;
  UEGAN_CHECK_ARG(gam_plan(dtype, B, HW, C, act, p), "uegan_gam_bwd: 16-bit storage, C = 32 or 64, activation none or LeakyReLU (ask uegan_gam_bwd_ws_bytes first)");
  UEGAN_CHECK_ARG(g && y && x && rstd && w_ihwo && dz_enc && dw && workspace, "uegan_gam_bwd: null argument");
  UEGAN_CHECK_ARG(Cin_w == C && Cin_row >= C, "uegan_gam_bwd: the weight gradient is a [C][Cin_row] matrix whose first C columns are written");
  // the grid is the one the size query planned: read back from the workspace the caller brought (the tuning knob is not consulted here)
  const size_t floats = workspace_bytes / sizeof(float);
  UEGAN_CHECK_ARG(floats >= p.red_floats + (size_t)C * C, "uegan_gam_bwd: workspace too small (uegan_gam_bwd_ws_bytes)");
  const size_t room = (floats - p.red_floats) / ((size_t)C * C);
  int blocks, per_block;
  gam_grid(p, room < (size_t)p.blocks ? (int)room : p.blocks, blocks, per_block);
  hipStream_t s = (hipStream_t)stream;
  float* tmp = static_cast<float*>(workspace);
  const float* tot = nullptr;
  int rc = instnorm_bwd_sums(dtype, g, y, tmp, B, HW, C, s, &tot);
  if (rc) return rc;
  GamBwdArgs a;
  a.g = static_cast<const bf16_t*>(g); a.y = static_cast<const bf16_t*>(y); a.x = static_cast<const bf16_t*>(x);
  a.add1 = static_cast<const bf16_t*>(add1); a.add2 = static_cast<const bf16_t*>(add2); a.w = static_cast<const bf16_t*>(w_ihwo);
  a.rstd = rstd; a.tot = tot; a.out = static_cast<bf16_t*>(dz_enc); a.ws = tmp + p.red_floats;
  a.HW = HW; a.act = act;
  a.tiles_per_img = p.tiles_per_img; a.tiles_total = p.tiles_total; a.tiles_per_block = per_block;
  a.inv_n = 1.f / (float)HW;
  if (C == 32) hipLaunchKernelGGL((gam_bwd_kernel<32>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gam_bwd_kernel<64>), dim3(blocks), dim3(256), 0, s, a);
  UEGAN_CHECK_LAUNCH();
  return wgrad_reduce_1x1(a.ws, dw, blocks, C, C, Cin_w, Cin_row, (size_t)C * C, accumulate ? 1 : 0, s);
}
