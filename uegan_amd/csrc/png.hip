// PNG files encoded on the device (include/uegan_hip.h: uegan_png_encode, uegan_deflate_bands).  Five launches per batch, (band, image) on the grid:
//   1. png_filter_hist_kernel   pixels -> Paeth-filtered bytes; per band the 256 literal counts (LDS) and the Adler partials S, T
//   2. png_code_kernel          per band: the length-limited, complete canonical Huffman code, the coded size, coded / stored
//   3. png_offsets_kernel       per image: scan of the band sizes -> chunk offsets, file size; Adler-32 from the partials
//   4. png_pack_kernel          per band: the block header and the code words, bit-packed through an LDS window into the band's scratch slot
//   5. png_layout_kernel        per band: the slot copied behind its chunk framing, the chunk CRC-32; band 0 also writes signature, IHDR, IEND
// Photographic residuals leave LZ77 almost nothing to find, so a band is ONE dynamic-Huffman block of literals.
#include "common.h"
#include "conv_core.h"      // ProfScope: the per-launch event timing tools/bench_png.py reads

namespace uegan {
namespace {

constexpr int PNG_THREADS = 256;
constexpr int PNG_MAX_BAND = 65535;          // a stored block holds at most this, so a band never takes more than n + 5 bytes
constexpr int PNG_SYMS = 257;                // 256 literals + end of block
constexpr int PNG_TAB = 260;                 // pitch (uint32) of the per-band count and code tables
constexpr int PNG_MAX_BITS = 15;
// BFINAL + BTYPE, HLIT, HDIST, HCLEN, 19 code-length code lengths of 3 bits, then 257 + 2 code lengths in the fixed 4-bit code
constexpr int PNG_HDR_LENS = 3 + 5 + 5 + 4 + 19 * 3;
constexpr int PNG_HDR_BITS = PNG_HDR_LENS + (PNG_SYMS + 2) * 4;
constexpr int PACK_RUN = 16;                                        // input bytes a thread owns per piece
constexpr int PACK_PIECE = PNG_THREADS * PACK_RUN;
constexpr int PACK_WIN = 1968;               // window words: 127 carried bits + the header + PACK_PIECE * 15 bits = 62677 bits -> 1959 words, + the carry group
static_assert(PACK_WIN % 4 == 0 && (127 + PNG_HDR_BITS + PACK_PIECE * PNG_MAX_BITS + 31) / 32 + 4 <= PACK_WIN, "the window holds the longest piece and its carry");
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t ADLER_MOD = 65521u;

// 32-bit add / or on an LDS word.  The emulator's fibers of one block share an OS thread and only switch at barriers: a plain update is atomic there.
__device__ __forceinline__ void lds_add_u32(uint32_t* p, uint32_t v) {
#ifdef UEGAN_EMU
  *p += v;
#else
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}
__device__ __forceinline__ void lds_or_u32(uint32_t* p, uint32_t v) {
#ifdef UEGAN_EMU
  *p |= v;
#else
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}

// Band k of an image covers bytes [k * band_n, k * band_n + n_k) of its `total` filtered (or raw) bytes; only the last band is short.
struct BandGeom {
  long long total;
  int band_n, nb;
  int row;            // 3W + 1; 0: raw bytes, no filter
  int H, W;
};
__device__ __forceinline__ int band_len(const BandGeom& g, int k) {
  const long long left = g.total - (long long)k * g.band_n;
  return left < (long long)g.band_n ? (int)left : g.band_n;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- 1. filter + histogram + Adler partials ------------------------------------------------------------------------------------------
// S = sum d_i, T = sum (n - i) d_i over the band's bytes (i from 0): from (a, b) a band leads to (a + S, b + n a + T) mod 65521.
template <bool FILTER>
__global__ __launch_bounds__(PNG_THREADS) void png_filter_hist_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ filt, uint32_t* __restrict__ hist,
                                                                      unsigned long long* __restrict__ st, BandGeom g) {
  __shared__ uint32_t h[4][PNG_TAB];             // one copy per wave: residuals crowd around 0, and same-address LDS adds serialise
  __shared__ unsigned long long red[2][4];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < 4 * PNG_TAB; i += PNG_THREADS) (&h[0][0])[i] = 0;
  __syncthreads();
  const long long off = (long long)k * g.band_n;
  const int n = band_len(g, k);
  uint32_t* hw = h[tid >> 6];
  unsigned long long S = 0, T = 0;
  if (FILTER) {
    const size_t pitch = (size_t)g.W * 3;
    const uint8_t* img = src + (size_t)b * g.H * pitch;
    uint8_t* dst = filt + (size_t)b * g.total + off;
    const int y0 = k * (g.band_n / g.row);
    for (int j = tid; j < n; j += PNG_THREADS) {
      const int r = j / g.row, c = j - r * g.row;
      int d = 4;                                  // the row's filter type: Paeth
      if (c > 0) {
        const int i = c - 1, y = y0 + r;
        const uint8_t* cur = img + (size_t)y * pitch;
        const int x = cur[i], left = i >= 3 ? cur[i - 3] : 0;
        int up = 0, ul = 0;                       // the row above comes from the pixels: bands do not depend on each other
        if (y > 0) {
          up = cur[(long long)i - (long long)pitch];
          ul = i >= 3 ? cur[(long long)i - 3 - (long long)pitch] : 0;
        }
        const int p = left + up - ul;
        const int pa = abs(p - left), pb = abs(p - up), pc = abs(p - ul);
        const int pred = (pa <= pb && pa <= pc) ? left : (pb <= pc ? up : ul);
        d = (x - pred) & 255;
      }
      dst[j] = (uint8_t)d;
      lds_add_u32(&hw[d], 1u);
      S += (unsigned)d;
      T += (unsigned long long)(n - j) * (unsigned)d;
    }
  } else {
    const uint8_t* p = src + (size_t)b * g.total + off;
    for (int j = tid; j < n; j += PNG_THREADS) {
      const unsigned d = p[j];
      lds_add_u32(&hw[d], 1u);
      S += d;
      T += (unsigned long long)(n - j) * d;
    }
  }
  S = wave_sum_u64(S);
  T = wave_sum_u64(T);
  if ((tid & 63) == 0) { red[0][tid >> 6] = S; red[1][tid >> 6] = T; }
  __syncthreads();
  const size_t band = (size_t)b * g.nb + k;
  for (int s = tid; s < 256; s += PNG_THREADS) hist[band * PNG_TAB + s] = h[0][s] + h[1][s] + h[2][s] + h[3][s];
  if (tid == 0) {
    st[band * 2] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    st[band * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// ---- 2. code build --------------------------------------------------------------------------------------------------------------------
// One wave per band.  The lanes rank-sort the used symbols by (count, symbol); lane 0 builds the Huffman tree from the sorted leaves with two
// queues, counts the leaves per depth, folds depths above 15 into 15 and repairs the Kraft sum back to exactly 1 (one step: drop a 15-bit
// code, split the deepest shorter code into two), then hands the lengths out in sorted order, longest to the rarest.  table[s] = len << 16 |
// the canonical code, bit-reversed for the LSB-first stream.  meta[2 band] = the band's byte count in the stream, meta[2 band + 1] = stored.
__global__ __launch_bounds__(64) void png_code_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ table, uint32_t* __restrict__ meta, BandGeom g) {
  __shared__ uint32_t cnt[PNG_TAB], wt[PNG_TAB];
  __shared__ uint16_t order[PNG_TAB], par_leaf[PNG_TAB], par_int[PNG_TAB], dep[PNG_TAB];
  __shared__ uint8_t len[PNG_TAB];
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const size_t band = (size_t)b * g.nb + k;
  for (int s = lane; s < PNG_SYMS; s += 64) {
    cnt[s] = s < 256 ? hist[band * PNG_TAB + s] : 1u;          // the end-of-block symbol occurs once
    len[s] = 0;
  }
  __syncthreads();
  for (int s = lane; s < PNG_SYMS; s += 64) {
    const uint32_t c = cnt[s];
    if (c == 0) continue;
    int rank = 0;
    for (int t = 0; t < PNG_SYMS; ++t) {
      const uint32_t ct = cnt[t];
      rank += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
    }
    order[rank] = (uint16_t)s;
  }
  __syncthreads();
  if (lane == 0) {
    int nu = 0;
    for (int s = 0; s < PNG_SYMS; ++s) nu += cnt[s] != 0;      // >= 2: a band holds a byte, and the end of block
    int li = 0, ii = 0;
    for (int ni = 0; ni < nu - 1; ++ni) {                        // internal node ni = the two lightest roots; both queues are ascending
      uint32_t w = 0;
      for (int q = 0; q < 2; ++q) {
        if (li < nu && (ii >= ni || cnt[order[li]] <= wt[ii])) { w += cnt[order[li]]; par_leaf[li++] = (uint16_t)ni; }
        else { w += wt[ii]; par_int[ii++] = (uint16_t)ni; }
      }
      wt[ni] = w;
    }
    int bl[PNG_MAX_BITS + 2];
    for (int l = 0; l <= PNG_MAX_BITS + 1; ++l) bl[l] = 0;
    dep[nu - 2] = 0;
    for (int i = nu - 3; i >= 0; --i) dep[i] = dep[par_int[i]] + 1;
    for (int i = 0; i < nu; ++i) {
      const int d = dep[par_leaf[i]] + 1;
      ++bl[d < PNG_MAX_BITS ? d : PNG_MAX_BITS];
    }
    uint32_t kraft = 0;                                          // in units of 2^-15
    for (int l = 1; l <= PNG_MAX_BITS; ++l) kraft += (uint32_t)bl[l] << (PNG_MAX_BITS - l);
    while (kraft > (1u << PNG_MAX_BITS) && bl[PNG_MAX_BITS] > 0) {      // (every excess unit came from a code folded into 15 bits)
      --bl[PNG_MAX_BITS];
      for (int l = PNG_MAX_BITS - 1; l >= 1; --l)
        if (bl[l]) { --bl[l]; bl[l + 1] += 2; break; }
      --kraft;
    }
    int i = 0;
    for (int l = PNG_MAX_BITS; l >= 1; --l)
      for (int c = 0; c < bl[l]; ++c) len[order[i++]] = (uint8_t)l;
    uint32_t next[PNG_MAX_BITS + 1], code = 0;
    for (int l = 1; l <= PNG_MAX_BITS; ++l) { code = (code + (uint32_t)bl[l - 1]) << 1; next[l] = code; }
    uint32_t bits = PNG_HDR_BITS;
    for (int s = 0; s < PNG_SYMS; ++s) {
      const uint32_t l = len[s];
      uint32_t e = 0;
      if (l) {
        e = (l << 16) | (__builtin_bitreverse32(next[l]++) >> (32 - l));
        bits += cnt[s] * l;
      }
      table[band * PNG_TAB + s] = e;
    }
    const bool last = k == g.nb - 1;
    const uint32_t n = (uint32_t)band_len(g, k);
    const uint32_t coded = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;      // non-final: an empty stored block byte-aligns the next band
    const bool stored = coded >= n + 5 || kraft != (1u << PNG_MAX_BITS);      // (an incomplete code never reaches the stream)
    meta[band * 2] = stored ? n + 5 : coded;
    meta[band * 2 + 1] = stored ? 1u : 0u;
  }
}

// ---- 3. offsets, file size, Adler-32 --------------------------------------------------------------------------------------------------
// One block per image.  Band k's chunk (PNG: length, "IDAT", [78 01], bytes, [Adler], CRC; raw: [78 01], bytes, [Adler]) starts at off[k].
__global__ __launch_bounds__(PNG_THREADS) void png_offsets_kernel(const uint32_t* __restrict__ meta, const unsigned long long* __restrict__ st,
                                                                  unsigned long long* __restrict__ off, uint32_t* __restrict__ adler, long long* __restrict__ sizes,
                                                                  BandGeom g, int png) {
  __shared__ unsigned long long tsz[PNG_THREADS], ts[PNG_THREADS], tb[PNG_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = (g.nb + PNG_THREADS - 1) / PNG_THREADS;
  const int k0 = tid * per < g.nb ? tid * per : g.nb, k1 = k0 + per < g.nb ? k0 + per : g.nb;
  const unsigned frame = png ? 12u : 0u;
  unsigned long long sz = 0, s = 0;
  for (int k = k0; k < k1; ++k) {
    const size_t band = (size_t)b * g.nb + k;
    sz += meta[band * 2] + frame;
    s += st[band * 2];
  }
  tsz[tid] = sz;
  ts[tid] = s;
  __syncthreads();
  if (tid == 0) {                      // exclusive scans of the 256 per-thread totals
    unsigned long long a = 0, c = 0;
    for (int t = 0; t < PNG_THREADS; ++t) {
      const unsigned long long va = tsz[t], vc = ts[t];
      tsz[t] = a; ts[t] = c;
      a += va; c += vc;
    }
  }
  __syncthreads();
  unsigned long long pos = (png ? 33u : 0u) + tsz[tid], a = 1 + ts[tid], bsum = 0;
  for (int k = k0; k < k1; ++k) {
    const size_t band = (size_t)b * g.nb + k;
    off[band] = pos + (k > 0 ? 2u : 0u);
    pos += meta[band * 2] + frame;
    const unsigned long long n = (unsigned long long)band_len(g, k);
    bsum = (bsum + n * (a % ADLER_MOD) + st[band * 2 + 1] % ADLER_MOD) % ADLER_MOD;
    a += st[band * 2];
  }
  tb[tid] = bsum;
  __syncthreads();
  if (tid == PNG_THREADS - 1) {        // (this thread's running values are the image's totals)
    unsigned long long bt = 0;
    for (int t = 0; t < PNG_THREADS; ++t) bt += tb[t];
    adler[b] = (uint32_t)((bt % ADLER_MOD) << 16 | (a % ADLER_MOD));
    sizes[b] = (long long)(pos + 6u + frame);                    // zlib header + Adler; PNG: + IEND
  }
}

// ---- 4. bit packing -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_bits(uint32_t* win, uint32_t pos, uint32_t val) {
  const unsigned long long v = (unsigned long long)val << (pos & 31);
  lds_or_u32(&win[pos >> 5], (uint32_t)v);
  if (v >> 32) lds_or_u32(&win[(pos >> 5) + 1], (uint32_t)(v >> 32));
}

// One block per band, pieces of PACK_PIECE bytes.  A thread owns PACK_RUN consecutive bytes of the piece; its bit offset is the block scan of the runs'
// code lengths; it ORs its words into the LDS window (neighbours share their boundary words there), and the block flushes the window's whole 16-byte
// groups to the band's slot, carrying the rest to the front.  Stored bands are copied behind their 5-byte block header.
__global__ __launch_bounds__(PNG_THREADS) void png_pack_kernel(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ table, const uint32_t* __restrict__ meta,
                                                               uint8_t* __restrict__ tmp, size_t tstride, BandGeom g) {
  __shared__ uint32_t tab[PNG_TAB];
  __shared__ uint32_t stage[PACK_PIECE / 4];
  __shared__ __attribute__((aligned(16))) uint32_t win[PACK_WIN];
  __shared__ uint32_t wsum[4];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t band = (size_t)b * g.nb + k;
  const int n = band_len(g, k);
  const bool last = k == g.nb - 1;
  const uint8_t* src = bytes + (size_t)b * g.total + (size_t)k * g.band_n;
  uint8_t* out = tmp + band * tstride;
  if (meta[band * 2 + 1]) {
    if (tid == 0) {
      out[0] = last ? 1 : 0;
      out[1] = (uint8_t)(n & 255); out[2] = (uint8_t)(n >> 8);
      out[3] = (uint8_t)(~n & 255); out[4] = (uint8_t)((~n >> 8) & 255);
    }
    for (int j = tid; j < n; j += PNG_THREADS) out[5 + j] = src[j];
    return;
  }
  for (int s = tid; s < PNG_TAB; s += PNG_THREADS) tab[s] = s < PNG_SYMS ? table[band * PNG_TAB + s] : 0u;
  for (int i = tid; i < PACK_WIN; i += PNG_THREADS) win[i] = 0;
  __syncthreads();
  if (tid == 0) {
    put_bits(win, 0, (last ? 1u : 0u) | (2u << 1));          // BFINAL, BTYPE = dynamic
    put_bits(win, 3, 0);                                      // HLIT: 257 codes
    put_bits(win, 8, 1);                                      // HDIST: 2 codes
    put_bits(win, 13, 15);                                    // HCLEN: all 19, in the order 16 17 18 0 8 7 9 ... 15
    for (int i = 3; i < 19; ++i) put_bits(win, 17 + 3 * i, 4);      // 16, 17, 18 unused; 0..15 at 4 bits: symbol v has code v
  }
  for (int i = tid; i < PNG_SYMS + 2; i += PNG_THREADS) {
    const uint32_t l = i < PNG_SYMS ? tab[i] >> 16 : 1u;        // ... and two distance codes of length 1
    put_bits(win, PNG_HDR_LENS + 4 * i, __builtin_bitreverse32(l) >> 28);
  }
  uint32_t carry_bits = PNG_HDR_BITS;
  size_t groups = 0;                                            // 16-byte groups flushed so far
  uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
  for (int p0 = 0; p0 < n; p0 += PACK_PIECE) {
    for (int i = tid; i < PACK_PIECE; i += PNG_THREADS) sb[i] = p0 + i < n ? src[p0 + i] : (uint8_t)0;
    __syncthreads();
    const int have = n - p0 - tid * PACK_RUN;
    uint32_t e[PACK_RUN], bits = 0;
#pragma unroll
    for (int q = 0; q < PACK_RUN; ++q) {
      e[q] = q < have ? tab[sb[tid * PACK_RUN + q]] : 0u;
      bits += e[q] >> 16;
    }
    uint32_t pre = 0, tot = bits;                               // exclusive prefix inside the wave by butterflies
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t other = __shfl_xor(tot, o, 64);
      if (tid & o) pre += other;
      tot += other;
    }
    if ((tid & 63) == 0) wsum[tid >> 6] = tot;
    __syncthreads();
    uint32_t piece_bits = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < (tid >> 6)) pre += wsum[w];
      piece_bits += wsum[w];
    }
    uint32_t pos = carry_bits + pre, word = pos >> 5;
    int nacc = (int)(pos & 31);
    unsigned long long acc = 0;
#pragma unroll
    for (int q = 0; q < PACK_RUN; ++q) {
      acc |= (unsigned long long)(e[q] & 0xffffu) << nacc;
      nacc += (int)(e[q] >> 16);
      if (nacc >= 32) {
        lds_or_u32(&win[word++], (uint32_t)acc);
        acc >>= 32;
        nacc -= 32;
      }
    }
    if (nacc) lds_or_u32(&win[word], (uint32_t)acc);
    __syncthreads();
    const uint32_t total_bits = carry_bits + piece_bits, ng = total_bits >> 7;
    for (uint32_t gi = tid; gi < ng; gi += PNG_THREADS)
      *reinterpret_cast<u32x4*>(out + (groups + gi) * 16) = *reinterpret_cast<const u32x4*>(&win[4 * gi]);
    const uint32_t cw = tid < 4 ? win[4 * ng + tid] : 0u;
    __syncthreads();
    for (int i = tid; i < PACK_WIN; i += PNG_THREADS) win[i] = 0;
    __syncthreads();
    if (tid < 4) win[tid] = cw;
    groups += ng;
    carry_bits = total_bits & 127u;
  }
  __syncthreads();
  const uint32_t eob = tab[256];
  if (tid == 0) put_bits(win, carry_bits, eob & 0xffffu);
  carry_bits += eob >> 16;
  if (!last) {                                                   // empty stored block: 000, pad to the byte, LEN 0000, NLEN FFFF
    carry_bits = (carry_bits + 3 + 7) & ~7u;
    if (tid == 0) put_bits(win, carry_bits + 16, 0xffffu);
    carry_bits += 32;
  } else {
    carry_bits = (carry_bits + 7) & ~7u;
  }
  __syncthreads();
  const uint32_t nwords = (carry_bits + 31) >> 5;               // (the slot has 16 spare bytes for the last word's tail)
  if ((uint32_t)tid < nwords) reinterpret_cast<uint32_t*>(out + groups * 16)[tid] = win[tid];
}

// ---- 5. layout + CRC ------------------------------------------------------------------------------------------------------------------
// CRC-32 register arithmetic (reflected, x^0 at bit 31): a zero byte multiplies the register by x^8 mod P, and the register after a message is
// affine in its start value, so per-thread slices started from 0 join as XOR of (slice register) * x^(8 * bytes that follow).
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
__device__ __forceinline__ uint32_t crc_shift(uint32_t c, uint32_t nbytes) {
  uint32_t pw = 0x00800000u;                                     // x^8
  while (nbytes && c) {
    if (nbytes & 1u) c = gf_mul(pw, c);
    pw = gf_mul(pw, pw);
    nbytes >>= 1;
  }
  return c;
}
__device__ __forceinline__ uint32_t crc_byte(const uint32_t* crct, uint32_t c, uint32_t v) { return crct[(c ^ v) & 255u] ^ (c >> 8); }
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

__global__ __launch_bounds__(PNG_THREADS) void png_layout_kernel(const uint8_t* __restrict__ tmp, size_t tstride, const uint32_t* __restrict__ meta,
                                                                 const unsigned long long* __restrict__ off, const uint32_t* __restrict__ adler,
                                                                 const long long* __restrict__ sizes, uint8_t* __restrict__ out, long long out_stride, BandGeom g, int png) {
  __shared__ uint32_t crct[256];
  __shared__ uint32_t red[4];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t band = (size_t)b * g.nb + k;
  const bool first = k == 0, last = k == g.nb - 1;
  const uint32_t size = meta[band * 2];
  const uint8_t* src = tmp + band * tstride;
  uint8_t* file = out + (size_t)b * (size_t)out_stride;
  uint8_t* dst = file + off[band];
  {
    uint32_t c = (uint32_t)tid;
    for (int i = 0; i < 8; ++i) c = (c & 1u) ? CRC_POLY ^ (c >> 1) : c >> 1;
    crct[tid] = c;
  }
  __syncthreads();
  const uint32_t hdr = png ? 8u : 0u, pre = first ? 2u : 0u;
  const uint32_t ad = adler[b];
  uint8_t* body = dst + hdr + pre;
  if (tid == 0) {
    if (png) {
      put_be32(dst, size + pre + (last ? 4u : 0u));
      dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    }
    if (first) { dst[hdr] = 0x78; dst[hdr + 1] = 0x01; }        // zlib header: deflate, 32 KiB window, no dictionary, check bits
    if (last) put_be32(body + size, ad);
  }
  for (uint32_t j = tid; j < size; j += PNG_THREADS) body[j] = src[j];
  if (!png) return;
  if (first && tid == 64) {                                      // the fixed chunks, by another wave's first lane
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int i = 0; i < 8; ++i) file[i] = sig[i];
    uint8_t* ih = file + 8;
    put_be32(ih, 13);
    ih[4] = 'I'; ih[5] = 'H'; ih[6] = 'D'; ih[7] = 'R';
    put_be32(ih + 8, (uint32_t)g.W);
    put_be32(ih + 12, (uint32_t)g.H);
    ih[16] = 8; ih[17] = 2; ih[18] = 0; ih[19] = 0; ih[20] = 0;   // 8 bits, RGB, deflate, adaptive filtering, no interlace
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 4; i < 21; ++i) c = crc_byte(crct, c, ih[i]);
    put_be32(ih + 21, ~c);
    uint8_t* ie = file + sizes[b] - 12;
    put_be32(ie, 0);
    ie[4] = 'I'; ie[5] = 'E'; ie[6] = 'N'; ie[7] = 'D';
    put_be32(ie + 8, 0xAE426082u);
  }
  // the chunk's CRC: type, [zlib header], the band's bytes in 256 contiguous slices (whole 16-byte groups of the aligned slot), [Adler]
  const uint32_t slice = ((size + PNG_THREADS - 1) / PNG_THREADS + 15u) & ~15u;
  const uint32_t lo = (uint32_t)tid * slice < size ? (uint32_t)tid * slice : size, hi = lo + slice < size ? lo + slice : size;
  uint32_t c = 0;
  if (tid == 0) {
    c = 0xFFFFFFFFu;
    c = crc_byte(crct, c, 'I'); c = crc_byte(crct, c, 'D'); c = crc_byte(crct, c, 'A'); c = crc_byte(crct, c, 'T');
    if (first) { c = crc_byte(crct, c, 0x78); c = crc_byte(crct, c, 0x01); }
  }
  for (uint32_t j = lo; j < hi; j += 16) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(src + j);
    const uint32_t m = hi - j < 16u ? hi - j : 16u;
    for (uint32_t q = 0; q < m; ++q) c = crc_byte(crct, c, (v[q >> 2] >> (8 * (q & 3))) & 255u);
  }
  c = crc_shift(c, size - hi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    c = red[0] ^ red[1] ^ red[2] ^ red[3];
    if (last)
      for (int i = 0; i < 4; ++i) c = crc_byte(crct, c, (ad >> (24 - 8 * i)) & 255u);
    put_be32(body + size + (last ? 4u : 0u), ~c);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct PngPlan {
  BandGeom g;
  size_t tstride;                                               // a band's slot: its n + 5 bytes in whole 16-byte groups, + one for the packer's last word
  size_t o_filt, o_tmp, o_hist, o_table, o_st, o_meta, o_off, o_adler, ws_bytes, capacity;
};

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// W > 0: H x W RGB images; W == 0: H raw bytes.  false: refused.
bool png_plan(int B, long long H, int W, int band_bytes, PngPlan& p) {
  if (B < 1 || B > 65535 || H < 1 || W < 0 || band_bytes < 0 || band_bytes > PNG_MAX_BAND) return false;
  const int bb = band_bytes == 0 ? PNG_MAX_BAND : band_bytes;
  BandGeom& g = p.g;
  long long nb;
  if (W > 0) {
    if (H > 0x7fffffffLL || (long long)W * 3 + 1 > bb) return false;
    g.row = 3 * W + 1;
    const int rows = bb / g.row;
    g.band_n = rows * g.row;
    nb = (H + rows - 1) / rows;
    g.total = H * g.row;
    g.H = (int)H;
  } else {
    g.row = 0;
    g.band_n = bb;
    nb = (H + bb - 1) / bb;
    g.total = H;
    g.H = 0;
  }
  if (nb > 0x7fffffffLL / 2) return false;
  g.W = W;
  g.nb = (int)nb;
  const size_t NB = (size_t)B * g.nb;
  p.tstride = (((size_t)g.band_n + 5 + 15) & ~(size_t)15) + 16;
  size_t o = 0;
  p.o_filt = o;   o += up256(W > 0 ? (size_t)B * g.total : 0);
  p.o_tmp = o;    o += up256(NB * p.tstride);
  p.o_hist = o;   o += up256(NB * PNG_TAB * 4);
  p.o_table = o;  o += up256(NB * PNG_TAB * 4);
  p.o_st = o;     o += up256(NB * 16);
  p.o_meta = o;   o += up256(NB * 8);
  p.o_off = o;    o += up256(NB * 8);
  p.o_adler = o;  o += up256((size_t)B * 4);
  p.ws_bytes = o;
  p.capacity = (size_t)g.total + (size_t)g.nb * (W > 0 ? 17 : 5) + 6 + (W > 0 ? 8 + 25 + 12 : 0);
  return true;
}

int png_run(const PngPlan& p, int B, const uint8_t* src, uint8_t* out, long long out_stride, long long* sizes, void* workspace, hipStream_t s) {
  const BandGeom& g = p.g;
  const int png = g.row > 0;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint8_t* filt = ws + p.o_filt;
  uint8_t* tmp = ws + p.o_tmp;
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + p.o_hist);
  uint32_t* table = reinterpret_cast<uint32_t*>(ws + p.o_table);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(ws + p.o_st);
  uint32_t* meta = reinterpret_cast<uint32_t*>(ws + p.o_meta);
  unsigned long long* off = reinterpret_cast<unsigned long long*>(ws + p.o_off);
  uint32_t* adler = reinterpret_cast<uint32_t*>(ws + p.o_adler);
  const dim3 grid(g.nb, B), block(PNG_THREADS);
  const double NB = (double)B * g.nb, filtered = (double)B * (double)g.total;      // (the records' bytes: what is known before the launch)
  {
    ProfScope prof(PROF_PNG | 0, 0.0, s, png ? filtered + 3.0 * B * g.H * g.W : filtered);
    if (png) hipLaunchKernelGGL((png_filter_hist_kernel<true>), grid, block, 0, s, src, filt, hist, st, g);
    else hipLaunchKernelGGL((png_filter_hist_kernel<false>), grid, block, 0, s, src, filt, hist, st, g);
    UEGAN_CHECK_LAUNCH();
  }
  {
    ProfScope prof(PROF_PNG | 1, 0.0, s, NB * PNG_TAB * 8);
    hipLaunchKernelGGL(png_code_kernel, grid, dim3(64), 0, s, hist, table, meta, g);
    UEGAN_CHECK_LAUNCH();
  }
  {
    ProfScope prof(PROF_PNG | 2, 0.0, s, NB * 32);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(B), block, 0, s, meta, st, off, adler, sizes, g, png);
    UEGAN_CHECK_LAUNCH();
  }
  {
    ProfScope prof(PROF_PNG | 3, 0.0, s, filtered);
    hipLaunchKernelGGL(png_pack_kernel, grid, block, 0, s, png ? (const uint8_t*)filt : src, table, meta, tmp, p.tstride, g);
    UEGAN_CHECK_LAUNCH();
  }
  {
    ProfScope prof(PROF_PNG | 4, 0.0, s, 0.0);
    hipLaunchKernelGGL(png_layout_kernel, grid, block, 0, s, tmp, p.tstride, meta, off, adler, sizes, out, out_stride, g, png);
    UEGAN_CHECK_LAUNCH();
  }
  return UEGAN_OK;
}

}  // namespace
}  // namespace uegan

using namespace uegan;

extern "C" size_t uegan_png_capacity_bytes(int64_t H, int W, int band_bytes) {
  PngPlan p;
  return png_plan(1, H, W, band_bytes, p) ? p.capacity : 0;
}

extern "C" size_t uegan_png_workspace_bytes(int B, int64_t H, int W, int band_bytes) {
  PngPlan p;
  return png_plan(B, H, W, band_bytes, p) ? p.ws_bytes : 0;
}

extern "C" int uegan_png_encode(const uint8_t* images, int B, int H, int W, int band_bytes, uint8_t* out, int64_t out_stride, int64_t* sizes, void* workspace,
                                uegan_stream_t stream) {
  UEGAN_CHECK_ARG(images && out && sizes && workspace && B > 0 && H > 0 && W > 0, "bad png_encode args");
  UEGAN_CHECK_ARG((long long)W * 3 + 1 <= PNG_MAX_BAND, "png_encode: a filtered row of %d pixels does not fit a %d-byte band", W, PNG_MAX_BAND);
  PngPlan p;
  UEGAN_CHECK_ARG(png_plan(B, H, W, band_bytes, p), "png_encode: band_bytes %d is not in [3W + 1 = %d, %d] (or B = %d is out of range)", band_bytes, 3 * W + 1,
                  PNG_MAX_BAND, B);
  UEGAN_CHECK_ARG(out_stride >= (int64_t)p.capacity, "png_encode: out_stride %lld is below the capacity %zu", (long long)out_stride, p.capacity);
  UEGAN_CHECK_ARG((uintptr_t)workspace % 16 == 0, "png_encode: the workspace must be 16-byte aligned");
  return png_run(p, B, images, out, out_stride, reinterpret_cast<long long*>(sizes), workspace, (hipStream_t)stream);
}

extern "C" int uegan_deflate_bands(const uint8_t* data, int64_t n, int band_bytes, uint8_t* out, int64_t* size, void* workspace, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(data && out && size && workspace && n > 0, "bad deflate_bands args");
  PngPlan p;
  UEGAN_CHECK_ARG(png_plan(1, n, 0, band_bytes, p), "deflate_bands: band_bytes %d is not in [1, %d] (or too many bands)", band_bytes, PNG_MAX_BAND);
  UEGAN_CHECK_ARG((uintptr_t)workspace % 16 == 0, "deflate_bands: the workspace must be 16-byte aligned");
  return png_run(p, 1, data, out, (long long)p.capacity, reinterpret_cast<long long*>(size), workspace, (hipStream_t)stream);
}
