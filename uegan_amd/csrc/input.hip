// Input pipeline on the device (data_loader.py:74-82 train, :95-100 test): what torchvision's
//     RandomCrop -> Resize -> RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize(0.5, 0.5)
// does to a decoded 8-bit RGB image, as two kernels over a batch of crop windows that were copied to the device as raw bytes.
//
// Resize on a PIL image is Pillow's two-pass resampler (horizontal, then vertical, an 8-bit intermediate image between the
// passes) with 22-bit fixed-point coefficients of the triangle filter stretched by the scale factor.  The coefficient tables
// are built on the host in double precision exactly as Pillow builds them (uegan_amd/data.py: resample_table) and the device
// does the integer arithmetic -- so the result is BIT-identical to the reference's loader, not "a bilinear resize".
//   pass 1   tmp[b][y][xo][c]  = clip8((2^21 + sum_k pix[b][y][xmin(xo) + k][c] * hc[xo][k]) >> 22)
//   pass 2   v                 = clip8((2^21 + sum_k tmp[b][ymin(yo) + k][xo][c] * vc[yo][k]) >> 22)
//            out[b][c][yo'][xo'] = (v / 255 - 0.5) / 0.5      (fp32, ToTensor's division then Normalize's two operations)
//            with (yo', xo') = (yo, xo) mirrored per image by the flip bits (a flip after the resize, as in the reference).
#include "common.h"

namespace uegan {

constexpr int INPUT_MAX_IMAGES = 64;
constexpr int RESAMPLE_PRECISION_BITS = 32 - 8 - 2;      // Pillow's PRECISION_BITS for 8-bit channels
struct FlipTable { int32_t bits[INPUT_MAX_IMAGES]; };     // bit 0: horizontal flip, bit 1: vertical flip (by value: no copy)

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// table row of output index o: [first input index, number of taps n <= K, K coefficients]
__global__ void resample_h_kernel(const uint8_t* pix, uint8_t* tmp, const int32_t* tab, int K, int B, int H, int W, int OW) {
  const size_t total = (size_t)B * H * OW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % OW);
    const size_t row = i / OW;                                   // (b, y)
    const int32_t* t = tab + (size_t)xo * (K + 2);
    const int x0 = t[0], n = t[1];
    const uint8_t* p = pix + (row * W + x0) * 3;
    int s0 = 1 << (RESAMPLE_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int k = 0; k < n; ++k) {
      const int c = t[2 + k];
      s0 += p[3 * k] * c; s1 += p[3 * k + 1] * c; s2 += p[3 * k + 2] * c;
    }
    uint8_t* q = tmp + i * 3;
    q[0] = (uint8_t)clip8(s0 >> RESAMPLE_PRECISION_BITS);
    q[1] = (uint8_t)clip8(s1 >> RESAMPLE_PRECISION_BITS);
    q[2] = (uint8_t)clip8(s2 >> RESAMPLE_PRECISION_BITS);
  }
}

// pass 1 over windows of RESIDENT images (uegan_input_transform_windows): the same sums, the source addressed per image.  origin[b] points at the
// window's first pixel (image + (top * pitch + left) * 3, computed and bounds-checked by the launcher), row y of the window lies y * pitch pixels
// further.  The table goes by value like FlipTable (768 bytes of kernel arguments, no copy); tmp is written as resample_h_kernel writes it, so
// pass 2 is resample_v_norm_kernel itself.  Byte loads only: a window's origin has no alignment.  One image per blockIdx.y: origin and pitch are
// uniform in a block (scalar loads of the arguments), and an item's (y, xo) comes from one 32-bit division.
struct WindowTable { const uint8_t* origin[INPUT_MAX_IMAGES]; int32_t pitch[INPUT_MAX_IMAGES]; };
constexpr int WINDOWS_BLOCKS_PER_IMAGE = 512;      // grid cap of pass 1 per image: 512 x 256 threads are one per item at 512 -> 256; above, grid stride

__global__ void resample_h_windows_kernel(WindowTable wt, uint8_t* tmp, const int32_t* tab, int K, int H, int OW) {
  const int b = blockIdx.y;
  const uint8_t* origin = wt.origin[b];
  const size_t pitch = (size_t)wt.pitch[b];
  uint8_t* dst = tmp + (size_t)b * H * OW * 3;
  const uint32_t total = (uint32_t)H * (uint32_t)OW;                  // (the launcher checked that it fits)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t y = i / (uint32_t)OW, xo = i - y * (uint32_t)OW;
    const int32_t* t = tab + (size_t)xo * (K + 2);
    const int x0 = t[0], n = t[1];
    const uint8_t* p = origin + (y * pitch + x0) * 3;
    int s0 = 1 << (RESAMPLE_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int k = 0; k < n; ++k) {
      const int c = t[2 + k];
      s0 += p[3 * k] * c; s1 += p[3 * k + 1] * c; s2 += p[3 * k + 2] * c;
    }
    uint8_t* q = dst + (size_t)i * 3;
    q[0] = (uint8_t)clip8(s0 >> RESAMPLE_PRECISION_BITS);
    q[1] = (uint8_t)clip8(s1 >> RESAMPLE_PRECISION_BITS);
    q[2] = (uint8_t)clip8(s2 >> RESAMPLE_PRECISION_BITS);
  }
}

__global__ void resample_v_norm_kernel(const uint8_t* tmp, float* out, const int32_t* tab, int K, FlipTable flips, int B, int H, int OH, int OW) {
  const size_t total = (size_t)B * OH * OW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % OW);
    const size_t r = i / OW;
    const int yo = (int)(r % OH), b = (int)(r / OH);
    const int32_t* t = tab + (size_t)yo * (K + 2);
    const int y0 = t[0], n = t[1];
    const uint8_t* p = tmp + (((size_t)b * H + y0) * OW + xo) * 3;
    int s0 = 1 << (RESAMPLE_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int k = 0; k < n; ++k) {
      const int c = t[2 + k];
      const uint8_t* pk = p + (size_t)k * OW * 3;
      s0 += pk[0] * c; s1 += pk[1] * c; s2 += pk[2] * c;
    }
    const int fb = flips.bits[b];
    const int xd = (fb & 1) ? OW - 1 - xo : xo, yd = (fb & 2) ? OH - 1 - yo : yo;
    float* o = out + (((size_t)b * 3) * OH + yd) * OW + xd;
    const size_t plane = (size_t)OH * OW;
    const int v[3] = {clip8(s0 >> RESAMPLE_PRECISION_BITS), clip8(s1 >> RESAMPLE_PRECISION_BITS), clip8(s2 >> RESAMPLE_PRECISION_BITS)};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v[c], 255.f), 0.5f), 0.5f);
  }
}

// pass 2 of the NIMA preparation (CalcNIMA.py:45-55: Resize(256) -> CenterCrop(224) -> ToTensor): the crop is an offset into the two tables
// (the caller passes the rows of the kept output indices only), the value is ToTensor's v / 255 alone.  cpad == 0: NCHW planes;
// cpad >= 3: NHWC with cpad channels per pixel, the extra ones zero.
__global__ void resample_v_unit_kernel(const uint8_t* tmp, float* out, const int32_t* tab, int K, int B, int H, int OH, int OW, int cpad) {
  const size_t total = (size_t)B * OH * OW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % OW);
    const size_t r = i / OW;
    const int yo = (int)(r % OH), b = (int)(r / OH);
    const int32_t* t = tab + (size_t)yo * (K + 2);
    const int y0 = t[0], n = t[1];
    const uint8_t* p = tmp + (((size_t)b * H + y0) * OW + xo) * 3;
    int s0 = 1 << (RESAMPLE_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int k = 0; k < n; ++k) {
      const int c = t[2 + k];
      const uint8_t* pk = p + (size_t)k * OW * 3;
      s0 += pk[0] * c; s1 += pk[1] * c; s2 += pk[2] * c;
    }
    const int v[3] = {clip8(s0 >> RESAMPLE_PRECISION_BITS), clip8(s1 >> RESAMPLE_PRECISION_BITS), clip8(s2 >> RESAMPLE_PRECISION_BITS)};
    if (cpad == 0) {
      const size_t plane = (size_t)OH * OW;
      float* o = out + (((size_t)b * 3) * OH + yo) * OW + xo;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = __fdiv_rn((float)v[c], 255.f);
    } else {
      float* o = out + i * cpad;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = __fdiv_rn((float)v[c], 255.f);
      for (int c = 3; c < cpad; ++c) o[c] = 0.f;
    }
  }
}

// ---- native-size input: ToTensor + Normalize of the image as it is, extended by reflection at the bottom and right to [hp][wp] (multiples of 16
// for the generator) in the same pass.  HBM-bound: 3 B read + 12 B written per output pixel.  One thread = 4 neighbouring output pixels of one row:
// one 16-byte store per plane (wp % 4 == 0 and out 16-byte aligned: the launcher checks both).  DW: w % 4 == 0 and pixels 4-byte aligned, so a
// group inside the image is 12 contiguous bytes at a multiple of 12 from an aligned base -> 3 whole dwords; groups in the extension (their source
// columns run backwards) and every group of the other case read byte by byte. ----
constexpr int NATIVE_THREADS = 256;
constexpr int NATIVE_MAX_BLOCKS = 2048;       // grid cap: 8 blocks (32 waves) per CU on 256 CUs, the rest by grid stride
constexpr int NATIVE_VEC = 4;                 // output pixels per thread (uegan_amd/data.py mirrors these three numbers)

__device__ __forceinline__ float norm_u8(uint32_t v) { return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), 0.5f), 0.5f); }

template <bool DW>
__global__ void native_input_kernel(const uint8_t* pix, float* out, size_t rows, int h, int w, int hp, int wp) {
  const int wq = wp / NATIVE_VEC;
  const size_t items = rows * wq;               // rows = B * hp
  const size_t plane = (size_t)hp * wp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
    const int x0 = (int)(i % wq) * NATIVE_VEC;
    const size_t row = i / wq;                  // b * hp + y
    const size_t b = row / hp;
    const int y = (int)(row - b * hp);
    const int sy = y < h ? y : 2 * (h - 1) - y;
    const uint8_t* src = pix + (b * h + sy) * (size_t)w * 3;
    uint32_t v[NATIVE_VEC * 3];                  // v[3 * j + c]: pixel x0 + j, channel c
    if (DW && x0 + NATIVE_VEC <= w) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (size_t)x0 * 3);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const uint32_t u = p[d];
        v[4 * d] = u & 255u; v[4 * d + 1] = (u >> 8) & 255u; v[4 * d + 2] = (u >> 16) & 255u; v[4 * d + 3] = u >> 24;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NATIVE_VEC; ++j) {
        const int x = x0 + j;
        const uint8_t* p = src + (size_t)(x < w ? x : 2 * (w - 1) - x) * 3;
        v[3 * j] = p[0]; v[3 * j + 1] = p[1]; v[3 * j + 2] = p[2];
      }
    }
    float* o = out + (b * 3 * hp + y) * (size_t)wp + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{norm_u8(v[c]), norm_u8(v[3 + c]), norm_u8(v[6 + c]), norm_u8(v[9 + c])};
  }
}

}  // namespace uegan

using namespace uegan;

extern "C" int uegan_native_input(const uint8_t* pixels, int B, int h, int w, int hp, int wp, float* out_nchw, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(pixels && out_nchw, "native_input: null pointer");
  UEGAN_CHECK_ARG(B >= 1 && h >= 1 && w >= 1, "native_input: bad geometry (B %d, %d x %d)", B, h, w);
  // a reflected index 2(n-1) - i stays inside [0, n) only while the extension is shorter than the image
  UEGAN_CHECK_ARG(hp >= h && hp - h < h && wp >= w && wp - w < w, "native_input: %d x %d cannot be extended by reflection to %d x %d", h, w, hp, wp);
  UEGAN_CHECK_ARG(wp % NATIVE_VEC == 0 && (uintptr_t)out_nchw % 16 == 0, "native_input: the padded width (%d) must be a multiple of %d and the output 16-byte aligned",
                  wp, NATIVE_VEC);
  const size_t rows = (size_t)B * hp;
  const size_t items = rows * (wp / NATIVE_VEC);
  const size_t want = (items + NATIVE_THREADS - 1) / NATIVE_THREADS;
  const dim3 grid((unsigned)(want < (size_t)NATIVE_MAX_BLOCKS ? want : (size_t)NATIVE_MAX_BLOCKS)), block(NATIVE_THREADS);
  const bool dw = w % 4 == 0 && (uintptr_t)pixels % 4 == 0;
  if (dw) hipLaunchKernelGGL((native_input_kernel<true>), grid, block, 0, (hipStream_t)stream, pixels, out_nchw, rows, h, w, hp, wp);
  else hipLaunchKernelGGL((native_input_kernel<false>), grid, block, 0, (hipStream_t)stream, pixels, out_nchw, rows, h, w, hp, wp);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_nima_prepare(const uint8_t* pixels, int B, int in_h, int in_w, int out_h, int out_w, const int32_t* htab, int hk,
                                  const int32_t* vtab, int vk, uint8_t* tmp, float* out, int cpad, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(pixels && htab && vtab && tmp && out, "nima_prepare: null pointer");
  UEGAN_CHECK_ARG(B >= 1 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && hk >= 1 && vk >= 1, "nima_prepare: bad geometry");
  UEGAN_CHECK_ARG(cpad == 0 || cpad >= 3, "nima_prepare: cpad is 0 (NCHW) or the NHWC channel count >= 3 (got %d)", cpad);
  hipStream_t s = (hipStream_t)stream;
  const size_t n1 = (size_t)B * in_h * out_w, n2 = (size_t)B * out_h * out_w;
  const int b1 = (int)((n1 + 255) / 256 < 16384 ? (n1 + 255) / 256 : 16384), b2 = (int)((n2 + 255) / 256 < 16384 ? (n2 + 255) / 256 : 16384);
  hipLaunchKernelGGL(resample_h_kernel, dim3(b1), dim3(256), 0, s, pixels, tmp, htab, hk, B, in_h, in_w, out_w);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(resample_v_unit_kernel, dim3(b2), dim3(256), 0, s, (const uint8_t*)tmp, out, vtab, vk, B, in_h, out_h, out_w, cpad);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_input_transform(const uint8_t* pixels, int B, int in_h, int in_w, int out_h, int out_w, const int32_t* htab, int hk,
                                     const int32_t* vtab, int vk, const int32_t* flips, uint8_t* tmp, float* out_nchw, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(pixels && htab && vtab && tmp && out_nchw, "input_transform: null pointer");
  UEGAN_CHECK_ARG(B >= 1 && B <= INPUT_MAX_IMAGES, "input_transform takes 1..%d images per call (got %d)", INPUT_MAX_IMAGES, B);
  UEGAN_CHECK_ARG(in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && hk >= 1 && vk >= 1, "input_transform: bad geometry");
  FlipTable ft;
  for (int i = 0; i < INPUT_MAX_IMAGES; ++i) ft.bits[i] = (flips && i < B) ? flips[i] : 0;
  hipStream_t s = (hipStream_t)stream;
  const size_t n1 = (size_t)B * in_h * out_w, n2 = (size_t)B * out_h * out_w;
  const int b1 = (int)((n1 + 255) / 256 < 16384 ? (n1 + 255) / 256 : 16384), b2 = (int)((n2 + 255) / 256 < 16384 ? (n2 + 255) / 256 : 16384);
  hipLaunchKernelGGL(resample_h_kernel, dim3(b1), dim3(256), 0, s, pixels, tmp, htab, hk, B, in_h, in_w, out_w);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(resample_v_norm_kernel, dim3(b2), dim3(256), 0, s, (const uint8_t*)tmp, out_nchw, vtab, vk, ft, B, in_h, out_h, out_w);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_input_transform_windows(const uegan_window* windows, int B, int win_h, int win_w, int out_h, int out_w, const int32_t* htab, int hk,
                                             const int32_t* vtab, int vk, uint8_t* tmp, float* out_nchw, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(windows && htab && vtab && tmp && out_nchw, "input_transform_windows: null pointer");
  UEGAN_CHECK_ARG(B >= 1 && B <= INPUT_MAX_IMAGES, "input_transform_windows takes 1..%d windows per call (got %d)", INPUT_MAX_IMAGES, B);
  UEGAN_CHECK_ARG(win_h > 0 && win_w > 0 && out_h > 0 && out_w > 0 && hk >= 1 && vk >= 1, "input_transform_windows: bad geometry");
  UEGAN_CHECK_ARG((int64_t)win_h * out_w < ((int64_t)1 << 31), "input_transform_windows: %d rows x %d output columns do not fit a 32-bit index", win_h, out_w);
  WindowTable wt;
  FlipTable ft;
  for (int i = 0; i < INPUT_MAX_IMAGES; ++i) { wt.origin[i] = nullptr; wt.pitch[i] = 0; ft.bits[i] = 0; }
  for (int i = 0; i < B; ++i) {      // every window inside its image, before anything is launched (64-bit sums: no wrap-around passes the test)
    const uegan_window& w = windows[i];
    UEGAN_CHECK_ARG(w.image, "input_transform_windows: window %d has no image", i);
    UEGAN_CHECK_ARG(w.height >= 1 && w.width >= 1 && w.pitch_px >= w.width, "input_transform_windows: window %d: bad image (%d x %d, pitch %d pixels)", i,
                    w.height, w.width, w.pitch_px);
    UEGAN_CHECK_ARG(w.top >= 0 && w.left >= 0 && (int64_t)w.top + win_h <= w.height && (int64_t)w.left + win_w <= w.width,
                    "input_transform_windows: window %d (%d x %d at row %d, column %d) leaves its %d x %d image", i, win_h, win_w, w.top, w.left, w.height,
                    w.width);
    wt.origin[i] = w.image + ((size_t)w.top * w.pitch_px + w.left) * 3;
    wt.pitch[i] = w.pitch_px;
    ft.bits[i] = w.flip_bits;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t n1 = (size_t)win_h * out_w, n2 = (size_t)B * out_h * out_w;      // pass 1: items per image
  const int b1 = (int)((n1 + 255) / 256 < (size_t)WINDOWS_BLOCKS_PER_IMAGE ? (n1 + 255) / 256 : (size_t)WINDOWS_BLOCKS_PER_IMAGE);
  const int b2 = (int)((n2 + 255) / 256 < 16384 ? (n2 + 255) / 256 : 16384);
  hipLaunchKernelGGL(resample_h_windows_kernel, dim3(b1, B), dim3(256), 0, s, wt, tmp, htab, hk, win_h, out_w);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(resample_v_norm_kernel, dim3(b2), dim3(256), 0, s, (const uint8_t*)tmp, out_nchw, vtab, vk, ft, B, win_h, out_h, out_w);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
