// Baseline JPEG files encoded on the device (include/uegan_hip.h: uegan_jpeg_encode, uegan_jpeg_coeffs, uegan_jpeg_qtables).  Five launches per batch:
//   1. jpeg_tables_kernel        the host-built 629 header bytes into the workspace; the four code tables (symbol -> length, code) from their DHT
//   2. jpeg_coeffs_kernel        pixels -> YCbCr (edges replicated, 4:2:0 chroma = mean of 2 x 2) -> fp32 8 x 8 DCT -> quantised int16, zigzag order
//   3. jpeg_pack_kernel<false>   per restart interval (one MCU row): the code words bit-packed through an LDS window, bytes and FF bytes counted
//   4. jpeg_offsets_kernel       per image: scan of the interval sizes -> offsets, file size
//   5. jpeg_pack_kernel<true>    the same packing again, the window's bytes stuffed (FF -> FF 00) straight to their place, RSTm / EOI, header
// Packing twice costs less than an unstuffed copy of the stream in global memory would, and needs no scratch whose size depends on the data.
// An interval is an independent byte-aligned stream whose DC prediction starts at 0, so nothing is serial beyond one MCU row.
//
// OPTIMISED TABLES (uegan_jpeg_encode_ex, flags bit 0).  Two more launches between 2 and 3 give every image its own four Huffman tables:
//   2a. jpeg_stats_kernel        per restart interval: the symbols encode_block would emit, counted in LDS, added to the image's [4][256] histogram
//   2b. jpeg_build_kernel        one wave per (table, image): Annex K.2 (libjpeg's jpeg_gen_optimal_table) -> BITS, HUFFVAL, the code table
// The packer then reads the image's own code tables, jpeg_offsets_kernel puts the image's header together from its four DHT (its length depends on
// how many symbols occur) and starts the offsets behind it.  An own table may give a DC category a 16-bit code: JPEG_BLOCK_BITS_OPT = 16 + 11 + 63 * 26.
//
// CAPACITY.  A block takes at most JPEG_BLOCK_BITS = 11 + 11 (the longest DC code of the Annex K.3 tables, chroma category 11, and its 11 magnitude
// bits) + 63 * (16 + 10) (the longest AC code and the 10 magnitude bits of a baseline coefficient) = 1660 bits: a ZRL stands for 16 zeros in 11 bits,
// and EOB only appears when the last coefficient is zero, so neither adds to it.  Stage 1 clamps DC to [-1024, 1023] and AC to +-1023, which an 8-bit
// input cannot exceed anyway, so the categories hold.  An interval of n blocks is ceil(1660 n / 8) bytes (the padding included), each stuffed at worst,
// + its 2-byte marker; a file is that per interval + the 629 header bytes.  The packing window holds a piece of PACK_PIECE blocks + 31 carried bits.
#include "common.h"
#include "conv_core.h"      // ProfScope: the per-launch event timing tools/bench_jpeg.py reads
#include "launch.h"

#include <string.h>

namespace uegan {
namespace {

constexpr int JPEG_THREADS = 128;
constexpr int JPEG_MCUS = JPEG_THREADS / 8;                    // stage 1: 8 lanes per MCU, so a wave holds 8 MCUs = 24 or 48 blocks
constexpr int JPEG_HDR = 629;                                  // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
constexpr int JPEG_HDR_PAD = 640;
constexpr int JPEG_BLOCK_BITS = 11 + 11 + 63 * (16 + 10);
constexpr int PACK_PIECE = JPEG_THREADS;                       // blocks per piece of the packer: one per thread
constexpr int PACK_WIN = ((31 + PACK_PIECE * JPEG_BLOCK_BITS + 31) / 32 + 1 + 3) & ~3;      // window words: carry + the longest piece, + one spare
constexpr int CST_PITCH = 33;                                  // words per staged block: 32 + 1, so the threads' blocks start in different banks
static_assert((31 + PACK_PIECE * JPEG_BLOCK_BITS + 31) / 32 < PACK_WIN, "the window holds the longest piece and its carry");
constexpr int JPEG_BLOCK_BITS_OPT = 16 + 11 + 63 * (16 + 10);  // an image's own DC table may hold a 16-bit code
constexpr int PACK_WIN_OPT = ((31 + PACK_PIECE * JPEG_BLOCK_BITS_OPT + 31) / 32 + 1 + 3) & ~3;
static_assert((31 + PACK_PIECE * JPEG_BLOCK_BITS_OPT + 31) / 32 < PACK_WIN_OPT, "the window holds the longest piece and its carry");
constexpr int JPEG_HDR_FRONT = 2 + 18 + 2 * 69 + 19;           // SOI .. SOF0: what stands before the first DHT
constexpr int JPEG_HDR_BACK = 6 + 14;                          // DRI, SOS: what stands behind the last
constexpr int JPEG_DHT_PITCH = 16 + 256;                       // a built table: BITS, HUFFVAL (zero-filled)
constexpr int HUFF_WAVE = 64;
constexpr int HUFF_PER_LANE = 5;                               // jpeg_build_kernel: 257 frequencies over 64 lanes
static_assert(JPEG_HDR_FRONT + 4 * 5 + 2 * (16 + 12) + 2 * (16 + 162) + JPEG_HDR_BACK == JPEG_HDR, "the header's parts");
static_assert(HUFF_WAVE * HUFF_PER_LANE >= 257, "every frequency has a lane");

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ void lds_or_u32(uint32_t* p, uint32_t v) {      // (png.hip: the emulator's fibers only switch at barriers)
#ifdef UEGAN_EMU
  *p |= v;
#else
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}
__device__ __forceinline__ void lds_add_u32(uint32_t* p, uint32_t v) {
#ifdef UEGAN_EMU
  *p += v;
#else
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}

// An image's coefficients: component planes one after the other, [block row][block col][64].  4:4:4: three planes of mcuy x mcux blocks;
// 4:2:0: Y has 2 mcuy x 2 mcux, Cb and Cr mcuy x mcux.
struct JpegGeom {
  int H, W, ss;                 // ss 0: 4:4:4 (MCU 8 x 8, 3 blocks), 1: 4:2:0 (MCU 16 x 16, 6 blocks: Y00 Y01 Y10 Y11 Cb Cr)
  int mcux, mcuy, nblk;
  int ycols;                    // block columns of the Y plane
  long long plane[3];           // first block of each component's plane
  long long img_blocks;
};

// block j (scan order) of MCU row iy -> its block index inside the image's coefficients
__device__ __forceinline__ long long scan_block(const JpegGeom& g, int iy, int j) {
  const int mx = j / g.nblk, k = j - mx * g.nblk;
  if (g.ss == 0) return (long long)k * g.plane[1] + (long long)iy * g.mcux + mx;
  if (k < 4) return (long long)(2 * iy + (k >> 1)) * g.ycols + 2 * mx + (k & 1);
  return (k == 4 ? g.plane[1] : g.plane[2]) + (long long)iy * g.mcux + mx;
}

// ---- 1. header + code tables --------------------------------------------------------------------------------------------------------
struct JpegHeader {
  uint8_t bytes[JPEG_HDR_PAD];
  int dht[4];                   // where each table's 16 counts start: DC luma, DC chroma, AC luma, AC chroma
  int nvals[4];
};

// huff[t * 256 + symbol] = length << 16 | code (0: no such symbol), t as in JpegHeader::dht
__global__ __launch_bounds__(256) void jpeg_tables_kernel(JpegHeader h, uint8_t* __restrict__ hdr, uint32_t* __restrict__ huff) {
  const int tid = threadIdx.x;
  for (int i = tid; i < JPEG_HDR_PAD; i += 256) hdr[i] = h.bytes[i];
  for (int i = tid; i < 4 * 256; i += 256) huff[i] = 0;
  __syncthreads();
  if (tid < 4) {
    const uint8_t* bits = h.bytes + h.dht[tid];
    const uint8_t* vals = bits + 16;
    const int nv = h.nvals[tid] < 256 ? h.nvals[tid] : 256;
    int l = 1, left = bits[0];
    uint32_t code = 0;
    for (int i = 0; i < nv; ++i) {
      for (int q = 0; q < 15 && left == 0 && l < 16; ++q) { ++l; code <<= 1; left = bits[l - 1]; }
      huff[tid * 256 + vals[i]] = ((uint32_t)l << 16) | (code & 0xffffu);
      ++code;
      --left;
    }
  }
}

// ---- 2. pixels -> coefficients ------------------------------------------------------------------------------------------------------
struct JpegQuant {
  uint8_t q[128];               // zigzag order, luma then chroma
  uint8_t zz[64];               // natural index (8 u + v) -> zigzag position
};

// 8-point DCT-II with the JPEG normalisation, X_k = a_k / 2 * sum x_n cos((2n + 1) k pi / 16), a_0 = 1 / sqrt 2: even / odd halves, c_k = cos(k pi / 16) / 2
__device__ __forceinline__ void dct8(const float (&x)[8], float (&X)[8]) {
  constexpr float c1 = 0.49039264020161522f, c2 = 0.46193976625564337f, c3 = 0.41573480615127262f, c4 = 0.35355339059327379f, c5 = 0.27778511650980111f,
                  c6 = 0.19134171618254489f, c7 = 0.09754516100806413f;
  const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
  const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
  X[0] = c4 * ((s0 + s3) + (s1 + s2));
  X[4] = c4 * ((s0 + s3) - (s1 + s2));
  X[2] = c2 * (s0 - s3) + c6 * (s1 - s2);
  X[6] = c6 * (s0 - s3) - c2 * (s1 - s2);
  X[1] = c1 * d0 + c3 * d1 + c5 * d2 + c7 * d3;
  X[3] = c3 * d0 - c7 * d1 - c1 * d2 - c5 * d3;
  X[5] = c5 * d0 - c1 * d1 + c7 * d2 + c3 * d3;
  X[7] = c7 * d0 - c5 * d1 + c3 * d2 - c1 * d3;
}

// JFIF full range, level shift -128 on Y (Cb, Cr: +128 - 128)
__device__ __forceinline__ void rgb_to_ycc(const uint8_t* p, float& y, float& cb, float& cr) {
  const float r = (float)p[0], g = (float)p[1], b = (float)p[2];
  y = 0.299f * r + 0.587f * g + 0.114f * b - 128.f;
  cb = -0.168735892f * r - 0.331264108f * g + 0.5f * b;
  cr = 0.5f * r - 0.418687589f * g - 0.081312411f * b;
}

// One block per JPEG_MCUS MCUs of one MCU row; 8 lanes per MCU.  The block's threads read the pixels side by side (a wave's loads are contiguous
// along the row) and leave the samples in the MCU's tile; lane r of an MCU then transforms row r of each of its blocks in place, after the barrier
// column r, quantises, and the block's 64 int16 go to the tile's front in zigzag order, from where each lane stores 16 bytes.
template <int SS>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_coeffs_kernel(const uint8_t* __restrict__ images, int16_t* __restrict__ coefs, JpegGeom g, JpegQuant jq) {
  constexpr int NBLK = SS ? 6 : 3, MCU = SS ? 16 : 8;
  __shared__ __attribute__((aligned(16))) float tile[JPEG_MCUS][NBLK][8][9];
  __shared__ float qf[128];      // natural order
  __shared__ uint8_t zz[64];
  const int tid = threadIdx.x, iy = blockIdx.y, b = blockIdx.z, mx0 = blockIdx.x * JPEG_MCUS;
  qf[tid] = (float)jq.q[(tid & 64) + jq.zz[tid & 63]];
  if (tid < 64) zz[tid] = jq.zz[tid];
  const uint8_t* img = images + (size_t)b * g.H * g.W * 3;
  const int xlast = g.W - 1, ylast = g.H - 1;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int i = it * JPEG_THREADS + tid, ry = i >> 7, rx = i & 127, m = rx >> 3, c = rx & 7;      // 8 rows of 128 pixels (4:2:0: of 2 x 2 quads)
    if constexpr (SS == 0) {
      const int px = imin(mx0 * 8 + rx, xlast), py = imin(iy * 8 + ry, ylast);
      float y, cb, cr;
      rgb_to_ycc(img + ((size_t)py * g.W + px) * 3, y, cb, cr);
      tile[m][0][ry][c] = y;
      tile[m][1][ry][c] = cb;
      tile[m][2][ry][c] = cr;
    } else {
      float sb = 0.f, sr = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int lx = 2 * c + (d & 1), ly = 2 * ry + (d >> 1);
        const int px = imin((mx0 + m) * MCU + lx, xlast), py = imin(iy * MCU + ly, ylast);
        float y, cb, cr;
        rgb_to_ycc(img + ((size_t)py * g.W + px) * 3, y, cb, cr);
        tile[m][(ly >> 3) * 2 + (lx >> 3)][ly & 7][lx & 7] = y;
        sb += cb;
        sr += cr;
      }
      tile[m][4][ry][c] = 0.25f * sb;
      tile[m][5][ry][c] = 0.25f * sr;
    }
  }
  __syncthreads();
  const int m = tid >> 3, r = tid & 7;
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {
    float x[8], X[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = tile[m][k][r][c];
    dct8(x, X);
#pragma unroll
    for (int c = 0; c < 8; ++c) tile[m][k][r][c] = X[c];
  }
  __syncthreads();
  int res[NBLK][8];
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {
    const float* q = qf + ((SS ? k >= 4 : k >= 1) ? 64 : 0);
    float x[8], X[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = tile[m][k][u][r];
    dct8(x, X);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float v = X[u] / q[u * 8 + r];
      const int iv = (int)(v + (v < 0.f ? -0.5f : 0.5f));          // round half away from zero
      res[k][u] = imax(u + r == 0 ? -1024 : -1023, imin(iv, 1023));
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {
    int16_t* o = reinterpret_cast<int16_t*>(&tile[m][k][0][0]);
#pragma unroll
    for (int u = 0; u < 8; ++u) o[zz[u * 8 + r]] = (int16_t)res[k][u];
  }
  __syncthreads();
  if (mx0 + m >= g.mcux) return;
  int16_t* cimg = coefs + (size_t)b * g.img_blocks * 64;
#pragma unroll
  for (int k = 0; k < NBLK; ++k) {
    const long long blk = scan_block(g, iy, (mx0 + m) * NBLK + k);
    *reinterpret_cast<u32x4*>(cimg + blk * 64 + r * 8) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const int16_t*>(&tile[m][k][0][0]) + r * 8);
  }
}

// ---- 3. / 5. entropy coding ----------------------------------------------------------------------------------------------------------
struct BitSink {
  uint32_t* win;
  uint32_t word;                // the window word the accumulator continues
  int nacc;                     // bits of that word already taken, by this thread's accumulator or by the neighbour before it
  unsigned long long acc;
  uint32_t bits;
};
// MSB first: a window word holds stream bits 32 w .. 32 w + 31 from its bit 31 down
template <bool EMIT>
__device__ __forceinline__ void sink_put(BitSink& s, uint32_t val, int len) {      // len <= 27
  s.bits += (uint32_t)len;
  if (EMIT) {
    s.acc = (s.acc << len) | val;
    s.nacc += len;
    if (s.nacc >= 32) {
      s.nacc -= 32;
      lds_or_u32(&s.win[s.word++], (uint32_t)(s.acc >> s.nacc));
      s.acc &= (1ull << s.nacc) - 1ull;
    }
  }
}
__device__ __forceinline__ int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

// What encode_block hands a block's symbols to.  CodeSink looks them up in the block's code tables and measures (EMIT: packs) the code words;
// CountSink (jpeg_stats_kernel) counts them in the block's two LDS histograms.  One walk feeds both, so every symbol that is emitted was counted.
template <bool EMIT>
struct CodeSink {
  BitSink s;
  const uint32_t *dc, *ac;
  uint32_t e_zrl, e_eob;
  __device__ __forceinline__ CodeSink(const BitSink& s_, const uint32_t* dc_, const uint32_t* ac_) : s(s_), dc(dc_), ac(ac_), e_zrl(ac_[0xF0]), e_eob(ac_[0]) {}
  __device__ __forceinline__ void code(uint32_t e, int sz, uint32_t extra) { sink_put<EMIT>(s, ((e & 0xffffu) << sz) | extra, (int)(e >> 16) + sz); }
  __device__ __forceinline__ void dc_symbol(int sz, uint32_t extra) { code(dc[sz], sz, extra); }
  __device__ __forceinline__ void ac_symbol(int run, int sz, uint32_t extra) { code(ac[(run << 4) | sz], sz, extra); }
  __device__ __forceinline__ void zrl() { code(e_zrl, 0, 0u); }
  __device__ __forceinline__ void eob() { code(e_eob, 0, 0u); }
};
struct CountSink {
  uint32_t *dc, *ac;            // [256] each, in LDS
  __device__ __forceinline__ void dc_symbol(int sz, uint32_t) { lds_add_u32(dc + sz, 1u); }
  __device__ __forceinline__ void ac_symbol(int run, int sz, uint32_t) { lds_add_u32(ac + ((run << 4) | sz), 1u); }
  __device__ __forceinline__ void zrl() { lds_add_u32(ac + 0xF0, 1u); }
  __device__ __forceinline__ void eob() { lds_add_u32(ac, 1u); }
};

// One block: the DC difference, then run/size symbols with ZRL for runs of 16 and EOB.  blk: the block's 32 words in LDS.
template <class Sink>
__device__ __forceinline__ void encode_block(Sink& s, const uint32_t* blk, int diff) {
  {
    const int sz = bit_size(imin(abs(diff), 2047));
    s.dc_symbol(sz, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << sz) - 1u));
  }
  int run = 0;
  for (int i = 1; i < 64; ++i) {
    const uint32_t w = blk[i >> 1];
    const int c = (int)(int16_t)((i & 1) ? (w >> 16) : (w & 0xffffu));
    if (c == 0) { ++run; continue; }
#pragma unroll
    for (int q = 0; q < 3; ++q)                                    // run <= 62: at most three ZRL
      if (q < (run >> 4)) s.zrl();
    const int sz = bit_size(imin(abs(c), 1023));
    s.ac_symbol(run & 15, sz, (uint32_t)(c < 0 ? c - 1 : c) & ((1u << sz) - 1u));
    run = 0;
  }
  if (run) s.eob();
}

// Piece p0 of interval k: its blocks staged from their planes into cst, CST_PITCH words each (a barrier must follow)
__device__ __forceinline__ void stage_piece(uint32_t* cst, const int16_t* cimg, const JpegGeom& g, int k, int p0, int n) {
  for (int c = threadIdx.x; c < PACK_PIECE * 8; c += JPEG_THREADS) {
    const int jb = c >> 3, part = c & 7;
    if (p0 + jb < n) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(cimg + scan_block(g, k, p0 + jb) * 64 + part * 8);
      uint32_t* d = cst + jb * CST_PITCH + part * 4;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  }
}

// Block j (scan order) of interval k, staged at blk: its DC difference; chroma: whether it takes the chroma tables
__device__ __forceinline__ int block_diff(const int16_t* cimg, const JpegGeom& g, int k, int j, const uint32_t* blk, bool& chroma) {
  const int mx = j / g.nblk, kk = j - mx * g.nblk;
  chroma = g.ss ? kk >= 4 : kk >= 1;
  // the block before it of the same component: 4:4:4 and 4:2:0 Y00 three back, Y01 Y10 Y11 one back, 4:2:0 chroma six back
  const int back = g.ss == 0 ? 3 : (kk >= 4 ? 6 : (kk == 0 ? 3 : 1));
  const bool first = g.ss && kk >= 1 && kk < 4 ? false : mx == 0;
  const int pred = first ? 0 : (int)cimg[scan_block(g, k, j - back) * 64];
  return (int)(int16_t)(blk[0] & 0xffffu) - pred;
}

// exclusive prefix of v over the block's threads, the block's total in `total`
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
  const int tid = threadIdx.x;
  uint32_t pre = 0, tot = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t other = __shfl_xor(tot, o, 64);
    if (tid & o) pre += other;
    tot += other;
  }
  __syncthreads();
  if ((tid & 63) == 0) wsum[tid >> 6] = tot;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < JPEG_THREADS / 64; ++w) {
    if (w < (tid >> 6)) pre += wsum[w];
    total += wsum[w];
  }
  return pre;
}

__device__ __forceinline__ uint32_t count_ff(uint32_t w) {
  return ((w >> 24) == 0xffu) + (((w >> 16) & 0xffu) == 0xffu) + (((w >> 8) & 0xffu) == 0xffu) + ((w & 0xffu) == 0xffu);
}

// One block per interval k (MCU row) of image b, pieces of PACK_PIECE blocks in scan order.  A thread owns one block of the piece: staged from its
// plane into LDS, measured, placed by the block scan of the lengths, and ORed into the window (neighbours share their boundary words there).  The
// window's whole words are then counted (WRITE: stuffed and stored by contiguous per-thread runs, placed by a scan of their FF counts), the rest
// is carried to the front.  !WRITE leaves the interval's size, marker included, in meta; WRITE writes at off[].
// OPT (an image's own tables): image b's code tables at huff + 1024 b, its header of hlen[b] bytes at hdr + JPEG_HDR_PAD b, and the wider window.
template <bool WRITE, bool OPT>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pack_kernel(const int16_t* __restrict__ coefs, const uint32_t* __restrict__ huff, uint32_t* __restrict__ meta,
                                                                 const unsigned long long* __restrict__ off, const long long* __restrict__ sizes,
                                                                 const uint8_t* __restrict__ hdr, const int* __restrict__ hlen, uint8_t* __restrict__ out,
                                                                 long long out_stride, JpegGeom g) {
  constexpr int WIN = OPT ? PACK_WIN_OPT : PACK_WIN;
  __shared__ uint32_t hf[4 * 256];
  __shared__ uint32_t cst[PACK_PIECE * CST_PITCH];
  __shared__ uint32_t win[WIN];
  __shared__ uint32_t wsum[JPEG_THREADS / 64];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (WRITE && sizes[b] > out_stride) return;                    // the file does not fit its slot: nothing of it is written
  const int n = g.mcux * g.nblk;                                 // blocks of the interval
  const size_t interval = (size_t)b * g.mcuy + k;
  const int16_t* cimg = coefs + (size_t)b * g.img_blocks * 64;
  uint8_t* file = WRITE ? out + (size_t)b * (size_t)out_stride : nullptr;
  uint8_t* dst = WRITE ? file + off[interval] : nullptr;
  if (OPT) { huff += (size_t)b * 1024; hdr += (size_t)b * JPEG_HDR_PAD; }
  for (int i = tid; i < 4 * 256; i += JPEG_THREADS) hf[i] = huff[i];
  for (int i = tid; i < WIN; i += JPEG_THREADS) win[i] = 0;
  if (WRITE && k == 0) {
    const int nh = OPT ? imin(hlen[b], JPEG_HDR) : JPEG_HDR;
    for (int i = tid; i < nh; i += JPEG_THREADS) file[i] = hdr[i];
  }
  uint32_t carry_bits = 0;                                       // < 32, in win[0]
  unsigned long long done = 0;                                   // bytes of the interval so far, stuffing included
  for (int p0 = 0; p0 < n; p0 += PACK_PIECE) {
    stage_piece(cst, cimg, g, k, p0, n);
    __syncthreads();
    const int j = p0 + tid;
    const bool have = j < n;
    const uint32_t* blk = cst + tid * CST_PITCH;
    const uint32_t *dc = hf, *ac = hf + 512;
    int diff = 0;
    if (have) {
      bool chroma;
      diff = block_diff(cimg, g, k, j, blk, chroma);
      if (chroma) { dc = hf + 256; ac = hf + 768; }
    }
    CodeSink<false> measure(BitSink{win, 0, 0, 0ull, 0}, dc, ac);
    if (have) encode_block(measure, blk, diff);
    uint32_t piece_bits;
    const uint32_t pos = carry_bits + block_scan_excl(measure.s.bits, wsum, piece_bits);
    if (have) {
      CodeSink<true> emit(BitSink{win, pos >> 5, (int)(pos & 31u), 0ull, 0}, dc, ac);
      encode_block(emit, blk, diff);
      if (emit.s.nacc) lds_or_u32(&win[emit.s.word], (uint32_t)(emit.s.acc << (32 - emit.s.nacc)));
    }
    __syncthreads();
    const uint32_t total_bits = carry_bits + piece_bits, nw = total_bits >> 5;
    const uint32_t per = (nw + JPEG_THREADS - 1) / JPEG_THREADS;
    const uint32_t lo = (uint32_t)tid * per < nw ? (uint32_t)tid * per : nw, hi = lo + per < nw ? lo + per : nw;
    uint32_t ff = 0;
    for (uint32_t i = lo; i < hi; ++i) ff += count_ff(win[i]);
    uint32_t piece_ff;
    const uint32_t ff_before = block_scan_excl(ff, wsum, piece_ff);
    if (WRITE) {
      uint8_t* p = dst + done + 4ull * lo + ff_before;
      for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t w = win[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint8_t v = (uint8_t)(w >> (24 - 8 * q));
          *p++ = v;
          if (v == 0xffu) *p++ = 0;
        }
      }
    }
    done += 4ull * nw + piece_ff;
    const uint32_t cw = win[nw];
    __syncthreads();
    for (uint32_t i = tid; i <= nw; i += JPEG_THREADS) win[i] = 0;
    __syncthreads();
    if (tid == 0) win[0] = cw;
    carry_bits = total_bits & 31u;
  }
  __syncthreads();
  if (tid == 0) {                                                // the last 0..4 bytes, padded with 1-bits, and the marker
    const uint32_t nb = (carry_bits + 7) >> 3, pad = nb * 8 - carry_bits;
    uint32_t w = win[0];
    if (pad) w |= ((1u << pad) - 1u) << (32 - nb * 8);
    uint8_t* p = WRITE ? dst + done : nullptr;
    uint32_t extra = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (q < nb) {
        const uint8_t v = (uint8_t)(w >> (24 - 8 * q));
        const bool stuff = v == 0xffu;
        if (WRITE) { *p++ = v; if (stuff) *p++ = 0; }
        extra += stuff ? 2u : 1u;
      }
    }
    if (WRITE) {
      p[0] = 0xff;
      p[1] = k == g.mcuy - 1 ? 0xd9 : (uint8_t)(0xd0 + (k & 7));
    } else {
      meta[interval] = (uint32_t)(done + extra + 2u);
    }
  }
}

// ---- 2a. symbol statistics -------------------------------------------------------------------------------------------------------------
// One block per interval k of image b, pieces staged as the packer stages them; a thread walks its block with the counting sink.  The block's
// counts gather in LDS and its non-zero counters are added to the image's histogram hist[b][4][256] (tables in the order of JpegHeader::dht), which
// the caller zeroed.  Integer sums: the result does not depend on the order of the blocks.
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_stats_kernel(const int16_t* __restrict__ coefs, unsigned long long* __restrict__ hist, JpegGeom g) {
  __shared__ uint32_t cst[PACK_PIECE * CST_PITCH];
  __shared__ uint32_t cnt[4 * 256];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = g.mcux * g.nblk;
  const int16_t* cimg = coefs + (size_t)b * g.img_blocks * 64;
  for (int i = tid; i < 4 * 256; i += JPEG_THREADS) cnt[i] = 0;
  for (int p0 = 0; p0 < n; p0 += PACK_PIECE) {
    stage_piece(cst, cimg, g, k, p0, n);
    __syncthreads();
    const int j = p0 + tid;
    if (j < n) {
      const uint32_t* blk = cst + tid * CST_PITCH;
      bool chroma;
      const int diff = block_diff(cimg, g, k, j, blk, chroma);
      CountSink s{cnt + (chroma ? 256 : 0), cnt + 512 + (chroma ? 256 : 0)};
      encode_block(s, blk, diff);
    }
    __syncthreads();
  }
  unsigned long long* h = hist + (size_t)b * 4 * 256;
  for (int i = tid; i < 4 * 256; i += JPEG_THREADS)
    if (cnt[i]) atomicAdd(h + i, (unsigned long long)cnt[i]);
}

// ---- 2b. code construction -------------------------------------------------------------------------------------------------------------
// a (frequency, index) comes before b in the search for the least frequency: ties go to the LARGEST index; index < 0: no candidate
__device__ __forceinline__ bool huff_before(unsigned long long fa, int ia, unsigned long long fb, int ib) {
  return ia >= 0 && (ib < 0 || fa < fb || (fa == fb && ia > ib));
}
// the first candidate of the wave, in every lane (the indices differ, so the order is total and all lanes agree)
__device__ __forceinline__ void wave_least(unsigned long long& f, int& i) {
#pragma unroll
  for (int o = 1; o < HUFF_WAVE; o <<= 1) {
    const unsigned long long of = __shfl_xor(f, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (huff_before(of, oi, f, i)) { f = of; i = oi; }
  }
}

// One wave per table: block (t, i) builds table t of histogram set i.  Annex K.2 as libjpeg's jpeg_gen_optimal_table states it: frequency 1 for the
// reserved index 256; merge the two least frequencies (ties to the largest index) until one is left, every merge lengthening the codes of both
// trees by one; move the symbols of lengths above 16 up pairwise; drop the reserved code; HUFFVAL by (length of the unlimited code, symbol).
// Lane l keeps indices 5 l .. 5 l + 4 in registers: frequency, code length, and the tree (the index its merges ended in) instead of libjpeg's
// `others` chain -- a merge adds one to every member of two trees, which the lanes do side by side with no chain to walk.  Bounds: 256 merges,
// 256 levels, per level at most 129 moves (each takes two of at most 257 symbols).  The serial rest (lane 0) runs over levels, not symbols.
__global__ __launch_bounds__(HUFF_WAVE) void jpeg_build_kernel(const unsigned long long* __restrict__ hist, uint8_t* __restrict__ dht, uint32_t* __restrict__ codes) {
  __shared__ int size_of[HUFF_WAVE * HUFF_PER_LANE];
  __shared__ int bits[260];                                      // [length], 0 .. 257
  __shared__ int start[260];                                     // [length of the unlimited code] -> its first place in HUFFVAL
  __shared__ int first[18], cum[18];                             // [length <= 16] -> its first code, its first place
  __shared__ uint32_t vals[256], code_of[256];
  __shared__ int nvals_s;
  const int lane = threadIdx.x;
  const size_t tab = (size_t)blockIdx.y * 4 + blockIdx.x;
  const unsigned long long* h = hist + tab * 256;
  unsigned long long fr[HUFF_PER_LANE];
  int cs[HUFF_PER_LANE], tree[HUFF_PER_LANE];
#pragma unroll
  for (int k = 0; k < HUFF_PER_LANE; ++k) {
    const int idx = lane * HUFF_PER_LANE + k;
    fr[k] = idx < 256 ? h[idx] : (idx == 256 ? 1ull : 0ull);
    cs[k] = 0;
    tree[k] = idx;
  }
  for (int merge = 0; merge < 256; ++merge) {
    unsigned long long f1 = 0, f2 = 0;
    int c1 = -1, c2 = -1;
#pragma unroll
    for (int k = 0; k < HUFF_PER_LANE; ++k)
      if (fr[k] && huff_before(fr[k], lane * HUFF_PER_LANE + k, f1, c1)) { f1 = fr[k]; c1 = lane * HUFF_PER_LANE + k; }
    wave_least(f1, c1);
#pragma unroll
    for (int k = 0; k < HUFF_PER_LANE; ++k)
      if (fr[k] && lane * HUFF_PER_LANE + k != c1 && huff_before(fr[k], lane * HUFF_PER_LANE + k, f2, c2)) { f2 = fr[k]; c2 = lane * HUFF_PER_LANE + k; }
    wave_least(f2, c2);
    if (c2 < 0) break;                                           // (the same in every lane)
#pragma unroll
    for (int k = 0; k < HUFF_PER_LANE; ++k) {
      const int idx = lane * HUFF_PER_LANE + k;
      if (idx == c1) fr[k] = f1 + f2;
      if (idx == c2) fr[k] = 0;
      if (tree[k] == c1 || tree[k] == c2) { ++cs[k]; tree[k] = c1; }
    }
  }
  for (int i = lane; i < 260; i += HUFF_WAVE) { bits[i] = 0; start[i] = 0; }
  for (int i = lane; i < 256; i += HUFF_WAVE) { vals[i] = 0; code_of[i] = 0; }
#pragma unroll
  for (int k = 0; k < HUFF_PER_LANE; ++k) size_of[lane * HUFF_PER_LANE + k] = cs[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < HUFF_PER_LANE; ++k)
    if (cs[k] > 0) lds_add_u32(reinterpret_cast<uint32_t*>(&bits[imin(cs[k], 257)]), 1u);
  __syncthreads();
  if (lane == 0) {
    const int reserved = size_of[256];
    int deep = 0, nv = 0;
    for (int l = 1; l <= 256; ++l) {
      const int c = bits[l];
      if (c) deep = l;
      start[l] = nv;
      nv += c - (l == reserved ? 1 : 0);
    }
    for (int i = deep; i > 16; --i)
      for (int move = 0; move < 129 && bits[i] > 0; ++move) {
        int j = i - 2;
        while (j > 0 && bits[j] == 0) --j;
        if (j == 0) break;
        bits[i] -= 2;
        bits[i - 1] += 1;
        bits[j + 1] += 2;
        bits[j] -= 1;
      }
    int last = 16;
    while (last > 0 && bits[last] == 0) --last;
    if (last > 0) --bits[last];                                  // the reserved code: the longest, all ones
    int code = 0, place = 0;
    for (int l = 1; l <= 16; ++l) {
      first[l] = code;
      cum[l] = place;
      place += bits[l];
      code = (code + bits[l]) << 1;
    }
    cum[17] = place;
    nvals_s = nv;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < HUFF_PER_LANE; ++k) {
    const int idx = lane * HUFF_PER_LANE + k;
    if (idx < 256 && cs[k] > 0) {
      int rank = 0;
      for (int s = 0; s < idx; ++s) rank += size_of[s] == cs[k];
      vals[(start[imin(cs[k], 257)] + rank) & 255] = (uint32_t)idx;
    }
  }
  __syncthreads();
  const int nv = imin(nvals_s, 256);
  for (int p = lane; p < nv; p += HUFF_WAVE) {
    int l = 1;
    while (l < 16 && p >= cum[l + 1]) ++l;
    code_of[vals[p]] = ((uint32_t)l << 16) | ((uint32_t)(first[l] + p - cum[l]) & 0xffffu);
  }
  __syncthreads();
  uint8_t* d = dht + tab * JPEG_DHT_PITCH;
  uint32_t* c = codes + tab * 256;
  if (lane < 16) d[lane] = (uint8_t)bits[lane + 1];
  for (int p = lane; p < 256; p += HUFF_WAVE) {
    d[16 + p] = p < nv ? (uint8_t)vals[p] : (uint8_t)0;
    c[p] = code_of[p];
  }
}

// ---- 4. offsets, file size ------------------------------------------------------------------------------------------------------------
// dht (an image's own tables, else null): image b's four built tables, [4][JPEG_DHT_PITCH] in the order of JpegHeader::dht.  Its header goes to
// hdrs + JPEG_HDR_PAD b: the front and the back of the standard header `hdr`, between them the four DHT segments at their real lengths in file
// order (DC luma, AC luma, DC chroma, AC chroma); its length to hlen[b], and the offsets start there.
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const uint32_t* __restrict__ meta, unsigned long long* __restrict__ off, long long* __restrict__ sizes, int nint,
                                                           const uint8_t* __restrict__ dht, const uint8_t* __restrict__ hdr, uint8_t* __restrict__ hdrs,
                                                           int* __restrict__ hlen) {
  __shared__ unsigned long long tsz[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int nhdr = JPEG_HDR;
  if (dht) {
    const uint8_t* tabs = dht + (size_t)b * 4 * JPEG_DHT_PITCH;
    int at[5];                                                     // where each segment starts, file order
    at[0] = JPEG_HDR_FRONT;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const uint8_t* bits = tabs + ((f & 1) * 2 + (f >> 1)) * JPEG_DHT_PITCH;
      int nv = 0;
      for (int l = 0; l < 16; ++l) nv += bits[l];
      at[f + 1] = at[f] + 5 + 16 + imin(nv, 162);                  // (12 DC categories and 162 AC symbols exist: never more than the standard header)
    }
    nhdr = imin(at[4] + JPEG_HDR_BACK, JPEG_HDR);
    uint8_t* o = hdrs + (size_t)b * JPEG_HDR_PAD;
    for (int i = tid; i < nhdr; i += 256) {
      uint8_t v;
      if (i < JPEG_HDR_FRONT) v = hdr[i];
      else if (i >= at[4]) v = hdr[JPEG_HDR - JPEG_HDR_BACK + (i - at[4])];
      else {
        const int f = (i >= at[1]) + (i >= at[2]) + (i >= at[3]), r = i - at[f], len = at[f + 1] - at[f] - 2;
        v = r == 0 ? 0xff : r == 1 ? 0xc4 : r == 2 ? (uint8_t)(len >> 8) : r == 3 ? (uint8_t)len : r == 4 ? (uint8_t)(((f & 1) << 4) | (f >> 1))
                                                                                                        : tabs[((f & 1) * 2 + (f >> 1)) * JPEG_DHT_PITCH + r - 5];
      }
      o[i] = v;
    }
    if (tid == 0) hlen[b] = nhdr;
  }
  const int per = (nint + 255) / 256;
  const int k0 = tid * per < nint ? tid * per : nint, k1 = k0 + per < nint ? k0 + per : nint;
  unsigned long long sz = 0;
  for (int k = k0; k < k1; ++k) sz += meta[(size_t)b * nint + k];
  tsz[tid] = sz;
  __syncthreads();
  if (tid == 0) {                      // exclusive scan of the 256 per-thread totals
    unsigned long long a = 0;
    for (int t = 0; t < 256; ++t) {
      const unsigned long long v = tsz[t];
      tsz[t] = a;
      a += v;
    }
  }
  __syncthreads();
  unsigned long long pos = (unsigned long long)nhdr + tsz[tid];
  for (int k = k0; k < k1; ++k) {
    off[(size_t)b * nint + k] = pos;
    pos += meta[(size_t)b * nint + k];
  }
  if (tid == 255) sizes[b] = (long long)pos;      // (its range ends the image, or is empty behind it)
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 / K.2, natural order
const uint8_t QBASE[2][64] = {{16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
                              {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: the 16 counts per code length, then the symbols
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// libjpeg's quality rule; zigzag order, luma then chroma
bool jpeg_qtables(int quality, uint8_t* out128) {
  if (quality < 1 || quality > 100) return false;
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = ((int)QBASE[t][ZIGZAG[i]] * s + 50) / 100;
      out128[t * 64 + i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return true;
}

struct JpegPlan {
  JpegGeom g;
  size_t o_coefs, o_meta, o_off, o_huff, o_hdr, ws_bytes, capacity;
  size_t o_hist, o_dht, o_huffs, o_hdrs, o_hlen;      // optimised tables only: per image
};

constexpr int JPEG_FLAG_OPTIMIZE = 1;

// subsampling: 0 (4:4:4) or 2 (4:2:0); flags: JPEG_FLAG_OPTIMIZE or 0.  false: refused.
bool jpeg_plan(int B, int H, int W, int subsampling, int flags, JpegPlan& p) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535 || (subsampling != 0 && subsampling != 2) || (flags & ~JPEG_FLAG_OPTIMIZE)) return false;
  JpegGeom& g = p.g;
  g.H = H; g.W = W; g.ss = subsampling == 2;
  const int mcu = g.ss ? 16 : 8;
  g.mcux = (W + mcu - 1) / mcu;
  g.mcuy = (H + mcu - 1) / mcu;
  g.nblk = g.ss ? 6 : 3;
  const long long cblocks = (long long)g.mcux * g.mcuy, yblocks = g.ss ? 4 * cblocks : cblocks;
  g.ycols = g.ss ? 2 * g.mcux : g.mcux;
  g.plane[0] = 0; g.plane[1] = yblocks; g.plane[2] = yblocks + cblocks;
  g.img_blocks = yblocks + 2 * cblocks;
  const size_t nint = (size_t)B * g.mcuy;
  size_t o = 0;
  p.o_coefs = o;  o += up256((size_t)B * g.img_blocks * 128);
  p.o_meta = o;   o += up256(nint * 4);
  p.o_off = o;    o += up256(nint * 8);
  p.o_huff = o;   o += up256(4 * 256 * 4);
  p.o_hdr = o;    o += up256(JPEG_HDR_PAD);
  p.o_hist = p.o_dht = p.o_huffs = p.o_hdrs = p.o_hlen = 0;
  if (flags & JPEG_FLAG_OPTIMIZE) {
    p.o_hist = o;   o += up256((size_t)B * 4 * 256 * 8);
    p.o_dht = o;    o += up256((size_t)B * 4 * JPEG_DHT_PITCH);
    p.o_huffs = o;  o += up256((size_t)B * 4 * 256 * 4);
    p.o_hdrs = o;   o += up256((size_t)B * JPEG_HDR_PAD);
    p.o_hlen = o;   o += up256((size_t)B * 4);
  }
  p.ws_bytes = o;
  const size_t interval = ((size_t)g.mcux * g.nblk * ((flags & JPEG_FLAG_OPTIMIZE) ? JPEG_BLOCK_BITS_OPT : JPEG_BLOCK_BITS) + 7) / 8;
  p.capacity = JPEG_HDR + (size_t)g.mcuy * (2 * interval + 2);
  return true;
}

void put_be16(uint8_t*& p, int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; }

void jpeg_header(const JpegGeom& g, const uint8_t* q128, JpegHeader& h) {
  memset(&h, 0, sizeof(h));
  uint8_t* p = h.bytes;
  put_be16(p, 0xffd8);
  put_be16(p, 0xffe0); put_be16(p, 16);
  const uint8_t jfif[12] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};      // 1.01, no units (aspect ratio) 1 : 1
  memcpy(p, jfif, 12); p += 12;
  *p++ = 0; *p++ = 0;                                                          // no thumbnail
  for (int t = 0; t < 2; ++t) {
    put_be16(p, 0xffdb); put_be16(p, 67);
    *p++ = (uint8_t)t;
    memcpy(p, q128 + t * 64, 64); p += 64;
  }
  put_be16(p, 0xffc0); put_be16(p, 17);
  *p++ = 8; put_be16(p, g.H); put_be16(p, g.W); *p++ = 3;
  *p++ = 1; *p++ = g.ss ? 0x22 : 0x11; *p++ = 0;
  *p++ = 2; *p++ = 0x11; *p++ = 1;
  *p++ = 3; *p++ = 0x11; *p++ = 1;
  for (int t = 0; t < 2; ++t) {                                                // DC, AC of luma, then of chroma
    put_be16(p, 0xffc4); put_be16(p, 2 + 1 + 16 + 12);
    *p++ = (uint8_t)t;
    h.dht[t] = (int)(p - h.bytes); h.nvals[t] = 12;
    memcpy(p, DC_BITS[t], 16); p += 16;
    for (int i = 0; i < 12; ++i) *p++ = (uint8_t)i;
    put_be16(p, 0xffc4); put_be16(p, 2 + 1 + 16 + 162);
    *p++ = (uint8_t)(0x10 | t);
    h.dht[2 + t] = (int)(p - h.bytes); h.nvals[2 + t] = 162;
    memcpy(p, AC_BITS[t], 16); p += 16;
    memcpy(p, AC_VALS[t], 162); p += 162;
  }
  put_be16(p, 0xffdd); put_be16(p, 4); put_be16(p, g.mcux);
  put_be16(p, 0xffda); put_be16(p, 12);
  *p++ = 3; *p++ = 1; *p++ = 0x00; *p++ = 2; *p++ = 0x11; *p++ = 3; *p++ = 0x11;
  *p++ = 0; *p++ = 63; *p++ = 0;
}

int jpeg_coeffs_run(const JpegGeom& g, int B, const uint8_t* images, const uint8_t* q128, int16_t* coefs, hipStream_t s) {
  JpegQuant jq;
  memcpy(jq.q, q128, 128);
  for (int i = 0; i < 64; ++i) jq.zz[ZIGZAG[i]] = (uint8_t)i;
  const dim3 grid(blocks_for((size_t)g.mcux, JPEG_MCUS, 1 << 30), g.mcuy, B);
  ProfScope prof(PROF_JPEG | 1, 0.0, s, (double)B * (3.0 * g.H * g.W + 128.0 * g.img_blocks));
  if (g.ss) hipLaunchKernelGGL((jpeg_coeffs_kernel<1>), grid, dim3(JPEG_THREADS), 0, s, images, coefs, g, jq);
  else hipLaunchKernelGGL((jpeg_coeffs_kernel<0>), grid, dim3(JPEG_THREADS), 0, s, images, coefs, g, jq);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

}  // namespace
}  // namespace uegan

using namespace uegan;

extern "C" int uegan_jpeg_qtables(int quality, uint8_t* out128) {
  UEGAN_CHECK_ARG(out128 && jpeg_qtables(quality, out128), "jpeg_qtables: quality %d is not in [1, 100]", quality);
  return UEGAN_OK;
}

extern "C" size_t uegan_jpeg_capacity_bytes_ex(int H, int W, int subsampling, int flags) {
  JpegPlan p;
  return jpeg_plan(1, H, W, subsampling, flags, p) ? p.capacity : 0;
}

extern "C" size_t uegan_jpeg_workspace_bytes_ex(int B, int H, int W, int subsampling, int flags) {
  JpegPlan p;
  return jpeg_plan(B, H, W, subsampling, flags, p) ? p.ws_bytes : 0;
}

extern "C" size_t uegan_jpeg_capacity_bytes(int H, int W, int subsampling) { return uegan_jpeg_capacity_bytes_ex(H, W, subsampling, 0); }

extern "C" size_t uegan_jpeg_workspace_bytes(int B, int H, int W, int subsampling) { return uegan_jpeg_workspace_bytes_ex(B, H, W, subsampling, 0); }

extern "C" int uegan_jpeg_coeffs(const uint8_t* images, int B, int H, int W, int quality, int subsampling, int16_t* coeffs, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(images && coeffs, "bad jpeg_coeffs args");
  JpegPlan p;
  UEGAN_CHECK_ARG(jpeg_plan(B, H, W, subsampling, 0, p), "jpeg_coeffs: B %d, H %d, W %d (1..65535 each) or subsampling %d (0: 4:4:4, 2: 4:2:0) is refused", B, H, W, subsampling);
  uint8_t q[128];
  UEGAN_CHECK_ARG(jpeg_qtables(quality, q), "jpeg_coeffs: quality %d is not in [1, 100]", quality);
  UEGAN_CHECK_ARG((uintptr_t)coeffs % 16 == 0, "jpeg_coeffs: the coefficients must be 16-byte aligned");
  return jpeg_coeffs_run(p.g, B, images, q, coeffs, (hipStream_t)stream);
}

static int jpeg_stats_run(const JpegGeom& g, int B, const int16_t* coefs, unsigned long long* hist, hipStream_t s) {
  UEGAN_CHECK_ARG(hipMemsetAsync(hist, 0, (size_t)B * 4 * 256 * 8, s) == hipSuccess, "jpeg: clearing the histograms failed");
  ProfScope prof(PROF_JPEG | 5, 0.0, s, (double)B * 128.0 * g.img_blocks);
  hipLaunchKernelGGL(jpeg_stats_kernel, dim3(g.mcuy, B), dim3(JPEG_THREADS), 0, s, coefs, hist, g);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

static int jpeg_build_run(const unsigned long long* hist, int n, uint8_t* dht, uint32_t* codes, hipStream_t s) {
  ProfScope prof(PROF_JPEG | 6, 0.0, s, (double)n * 4 * (256 * 12 + JPEG_DHT_PITCH));
  hipLaunchKernelGGL(jpeg_build_kernel, dim3(4, n), dim3(HUFF_WAVE), 0, s, hist, dht, codes);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_jpeg_histogram(const int16_t* coeffs, int B, int H, int W, int subsampling, uint64_t* hist, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(coeffs && hist, "bad jpeg_histogram args");
  JpegPlan p;
  UEGAN_CHECK_ARG(jpeg_plan(B, H, W, subsampling, 0, p), "jpeg_histogram: B %d, H %d, W %d (1..65535 each) or subsampling %d (0: 4:4:4, 2: 4:2:0) is refused", B, H, W,
                  subsampling);
  UEGAN_CHECK_ARG((uintptr_t)coeffs % 16 == 0 && (uintptr_t)hist % 8 == 0, "jpeg_histogram: the coefficients must be 16-byte, the histograms 8-byte aligned");
  return jpeg_stats_run(p.g, B, coeffs, reinterpret_cast<unsigned long long*>(hist), (hipStream_t)stream);
}

extern "C" int uegan_jpeg_build_tables(const uint64_t* hist, int n, uint8_t* dht, uint32_t* codes, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(hist && dht && codes, "bad jpeg_build_tables args");
  UEGAN_CHECK_ARG(n >= 1 && n <= 65535, "jpeg_build_tables: n %d is not in [1, 65535]", n);
  UEGAN_CHECK_ARG((uintptr_t)hist % 8 == 0 && (uintptr_t)codes % 4 == 0, "jpeg_build_tables: the histograms must be 8-byte, the codes 4-byte aligned");
  return jpeg_build_run(reinterpret_cast<const unsigned long long*>(hist), n, dht, codes, (hipStream_t)stream);
}

extern "C" int uegan_jpeg_encode_ex(const uint8_t* images, int B, int H, int W, int quality, int subsampling, int flags, uint8_t* out, int64_t out_stride,
                                    int64_t* sizes, void* workspace, uegan_stream_t stream) {
  UEGAN_CHECK_ARG((images || out) && sizes && workspace, "bad jpeg_encode args");
  UEGAN_CHECK_ARG((flags & ~JPEG_FLAG_OPTIMIZE) == 0, "jpeg_encode: flags %d holds an unknown bit (bit 0: optimised Huffman tables)", flags);
  JpegPlan p;
  UEGAN_CHECK_ARG(jpeg_plan(B, H, W, subsampling, flags, p), "jpeg_encode: B %d, H %d, W %d (1..65535 each; the restart interval of one MCU row must fit DRI) or "
                  "subsampling %d (0: 4:4:4, 2: 4:2:0) is refused", B, H, W, subsampling);
  uint8_t q[128];
  UEGAN_CHECK_ARG(jpeg_qtables(quality, q), "jpeg_encode: quality %d is not in [1, 100]", quality);
  UEGAN_CHECK_ARG(!out || out_stride >= JPEG_HDR, "jpeg_encode: out_stride %lld is below the header's %d bytes", (long long)out_stride, JPEG_HDR);
  UEGAN_CHECK_ARG((uintptr_t)workspace % 16 == 0, "jpeg_encode: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const JpegGeom& g = p.g;
  const bool opt = (flags & JPEG_FLAG_OPTIMIZE) != 0;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int16_t* coefs = reinterpret_cast<int16_t*>(ws + p.o_coefs);
  uint32_t* meta = reinterpret_cast<uint32_t*>(ws + p.o_meta);
  unsigned long long* off = reinterpret_cast<unsigned long long*>(ws + p.o_off);
  uint32_t* huff = reinterpret_cast<uint32_t*>(ws + p.o_huff);
  uint8_t* hdr = ws + p.o_hdr;
  // an image's own tables: its histograms, built tables, code tables, header and the header's length
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(ws + p.o_hist);
  uint8_t* dht = ws + p.o_dht;
  uint32_t* huffs = reinterpret_cast<uint32_t*>(ws + p.o_huffs);
  uint8_t* hdrs = ws + p.o_hdrs;
  int* hlen = reinterpret_cast<int*>(ws + p.o_hlen);
  long long* sz = reinterpret_cast<long long*>(sizes);
  const dim3 grid(g.mcuy, B), block(JPEG_THREADS);
  const double cbytes = (double)B * 128.0 * g.img_blocks;
  if (images) {
    {
      JpegHeader h;
      jpeg_header(g, q, h);
      ProfScope prof(PROF_JPEG | 0, 0.0, s, 0.0);
      hipLaunchKernelGGL(jpeg_tables_kernel, dim3(1), dim3(256), 0, s, h, hdr, huff);
      UEGAN_CHECK_LAUNCH();
    }
    int rc = jpeg_coeffs_run(g, B, images, q, coefs, s);
    if (rc != UEGAN_OK) return rc;
    if (opt) {
      rc = jpeg_stats_run(g, B, coefs, hist, s);
      if (rc != UEGAN_OK) return rc;
      rc = jpeg_build_run(hist, B, dht, huffs, s);
      if (rc != UEGAN_OK) return rc;
    }
    {
      ProfScope prof(PROF_JPEG | 2, 0.0, s, cbytes);
      if (opt) hipLaunchKernelGGL((jpeg_pack_kernel<false, true>), grid, block, 0, s, coefs, huffs, meta, off, sz, hdrs, hlen, (uint8_t*)nullptr, (long long)0, g);
      else hipLaunchKernelGGL((jpeg_pack_kernel<false, false>), grid, block, 0, s, coefs, huff, meta, off, sz, hdr, (const int*)nullptr, (uint8_t*)nullptr, (long long)0, g);
      UEGAN_CHECK_LAUNCH();
    }
    {
      ProfScope prof(PROF_JPEG | 3, 0.0, s, (double)B * g.mcuy * 12);
      hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(B), dim3(256), 0, s, meta, off, sz, g.mcuy, opt ? dht : (const uint8_t*)nullptr, hdr, hdrs, hlen);
      UEGAN_CHECK_LAUNCH();
    }
  }
  if (out) {
    ProfScope prof(PROF_JPEG | 4, 0.0, s, cbytes);
    if (opt) hipLaunchKernelGGL((jpeg_pack_kernel<true, true>), grid, block, 0, s, coefs, huffs, meta, off, sz, hdrs, hlen, out, (long long)out_stride, g);
    else hipLaunchKernelGGL((jpeg_pack_kernel<true, false>), grid, block, 0, s, coefs, huff, meta, off, sz, hdr, (const int*)nullptr, out, (long long)out_stride, g);
    UEGAN_CHECK_LAUNCH();
  }
  return UEGAN_OK;
}

extern "C" int uegan_jpeg_encode(const uint8_t* images, int B, int H, int W, int quality, int subsampling, uint8_t* out, int64_t out_stride, int64_t* sizes,
                                 void* workspace, uegan_stream_t stream) {
  return uegan_jpeg_encode_ex(images, B, H, W, quality, subsampling, 0, out, out_stride, sizes, workspace, stream);
}

