// Baseline JPEG files decoded on the device (include/uegan_hip.h: uegan_jpeg_decode).  The host parses the header (uegan_amd/codecs.py:
// jpeg_info) and hands over a descriptor; nothing on the host touches the entropy-coded bytes.
//
//   1. unstuff      jd_count_kernel / jd_offsets_kernel / jd_scatter_kernel: FF 00 -> FF, FF FF.. fill dropped, RSTm ends a restart
//                   interval (count and m = k mod 8 checked), the first other marker ends the scan.  Out: the plain stream and every
//                   interval's first byte.
//   2. entropy      an interval is cut into sub-sequences of `s` bits.  f_i(state) decodes from state = (bit position, block of the
//                   MCU, zigzag index) until the position passes the end of sub-sequence i.  jd_decode_kernel<true> computes
//                   E[i] = f_i(blind start) (E[0] from the true start); jd_decode_kernel<false> repeats E[i] = f_i(E[i-1]) for every i whose
//                   predecessor changed, until a launch changes nothing: then every E[i] is the serial decoder's state (induction from 0).
//                   jd_write_kernel decodes each sub-sequence once more from E[i-1] into int16 [block][64]; jd_dc_kernel sums the DC
//                   differences per component and interval.  With s = 0 an interval is one sub-sequence: one thread per interval.
//   3. pixels       jd_idct_kernel: dequantisation + libjpeg's integer "islow" inverse DCT into uint8 component planes;
//                   jd_colour_kernel: "fancy" chroma up-sampling and the fixed-point YCbCr -> RGB of libjpeg, uint8 [H][W][3].
//
// Termination: no kernel waits on another block; every loop is bounded by a size known at launch (a symbol takes at least one bit, so a
// sub-sequence decodes in at most its bit count + 1 steps; the rounds inside a block stop after `rmax`); the host bounds the launches by
// max_rounds and by N + JD_ROUNDS * (blocks - 1) + 1, which the iteration cannot exceed: with the first entry of a block reading its
// predecessor once per launch, entry i is final after at most i + JD_ROUNDS * (its block's index) rounds.  Every read of the stream is
// checked against the interval's end (zero bits behind it), every coefficient index against 64, every block index against the interval's
// expected count.
#include "common.h"

#include <string.h>

namespace uegan {
namespace {

constexpr int JD_THREADS = 256;
constexpr int JD_CHUNK = 16;                       // bytes per thread of the unstuff kernels
constexpr int JD_BLOCK_BYTES = JD_THREADS * JD_CHUNK;
constexpr int JD_SCAN_THREADS = 1024;
constexpr int JD_ROUNDS = 8;                       // rounds inside a block per launch: what one read of the control words covers
constexpr uint32_t JD_NONE = 0xffffffffu;

// control words (uint32) at the head of the workspace
enum { CTL_STATUS = 0, CTL_TERM = 1, CTL_BYTES = 2, CTL_RST = 3, CTL_NSUB = 4, CTL_HITS = 8, CTL_WORDS = 64 };
enum { ST_OK = 0, ST_MARKERS = 1, ST_CODE = 2, ST_BLOCKS = 3 };

struct HuffDec {
  uint16_t look[256];      // the next 8 bits -> length << 8 | symbol; 0: the code is longer than 8 bits
  int32_t maxcode[17];     // [l]: the largest code of length l, -1 without one
  int32_t valoff[17];      // [l]: index of the first symbol of length l minus its code
  uint8_t vals[256];
};
static_assert(sizeof(HuffDec) % 4 == 0, "copied by words");

struct JdTables { uint8_t counts[8][16]; uint8_t vals[8][256]; };      // DC 0..3, then AC 0..3

struct JdGeom {
  int H, W, ncomp, hmax, vmax, mcux, mcuy, bpm, ri, nint, s;
  int h[3], v[3], dc[3], ac[3];
  int blk_comp[6], blk_by[6], blk_bx[6];
  long long plane[4];          // first block of each component's plane; [ncomp]: all blocks
  long long pix[4];            // first byte of each component's sample plane
  uint8_t q[3][64];            // per component, zigzag order
};

struct JdPlan {
  JdGeom g;
  uint32_t len, nblocks, nmax;
  size_t o_ctl, o_huff, o_bb, o_br, o_bt, o_stream, o_istart, o_sfirst, o_e, o_in, o_cnt, o_cbase, o_subk, o_coefs, o_planes, ws_bytes;
};

size_t jd_up(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------------------
// block scans
// ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ uint32_t block_incl_scan(uint32_t v, uint32_t* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const uint32_t x = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  return sh[t];
}

template <int NT>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if (t < off) { const uint32_t o = sh[t + off]; if (o < sh[t]) sh[t] = o; }
    __syncthreads();
  }
  const uint32_t r = sh[0];
  __syncthreads();
  return r;
}

// exclusive scan of in[0 .. n) by one block, n = n_max or, with n_word >= 0, min(ctl[n_word], n_max); out[n] and, with total_word >= 0,
// ctl[total_word] receive the sum
__global__ __launch_bounds__(JD_SCAN_THREADS) void jd_scan_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ ctl, int n_word,
                                                                  uint32_t n_max, int total_word) {
  __shared__ uint32_t sh[JD_SCAN_THREADS];
  if (ctl[CTL_STATUS] != ST_OK) return;
  uint32_t n = n_word >= 0 ? ctl[n_word] : n_max;
  if (n > n_max) n = n_max;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_max; base += JD_SCAN_THREADS) {
    if (base >= n) break;
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n ? in[i] : 0u;
    const uint32_t incl = block_incl_scan<JD_SCAN_THREADS>(v, sh);
    if (i < n) out[i] = carry + incl - v;
    carry += sh[JD_SCAN_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[n] = carry;
    if (total_word >= 0) ctl[total_word] = carry;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. unstuff
// ---------------------------------------------------------------------------------------------------------------------
enum { K_NONE = 0, K_BYTE = 1, K_FF = 2, K_RST = 3, K_TERM = 4 };

// what position i of the scan contributes: a byte decides by itself and its predecessor alone (an FF contributes nothing; the byte behind a
// run of FFs says what the run was)
__device__ __forceinline__ int jd_classify(const uint8_t* __restrict__ d, uint32_t i) {
  const uint8_t b = d[i];
  if (b == 0xff) return K_NONE;
  if (i == 0 || d[i - 1] != 0xff) return K_BYTE;
  if (b == 0) return K_FF;
  if (b >= 0xd0 && b <= 0xd7) return K_RST;
  return K_TERM;
}

__global__ __launch_bounds__(JD_THREADS) void jd_count_kernel(const uint8_t* __restrict__ d, uint32_t len, uint32_t* __restrict__ bb, uint32_t* __restrict__ br,
                                                              uint32_t* __restrict__ bt) {
  __shared__ uint32_t sh[JD_THREADS];
  const uint32_t first = blockIdx.x * (uint32_t)JD_BLOCK_BYTES + threadIdx.x * (uint32_t)JD_CHUNK;
  uint32_t term = JD_NONE;
  for (int k = 0; k < JD_CHUNK; ++k) {
    const uint32_t i = first + k;
    if (i < len && term == JD_NONE && jd_classify(d, i) == K_TERM) term = i;
  }
  term = block_min<JD_THREADS>(term, sh);
  uint32_t nb = 0, nr = 0;
  for (int k = 0; k < JD_CHUNK; ++k) {
    const uint32_t i = first + k;
    if (i < len && i < term) {
      const int c = jd_classify(d, i);
      nb += (c == K_BYTE || c == K_FF);
      nr += (c == K_RST);
    }
  }
  const uint32_t tb = block_incl_scan<JD_THREADS>(nb, sh);
  __syncthreads();
  const uint32_t tr = block_incl_scan<JD_THREADS>(nr, sh);
  if (threadIdx.x == JD_THREADS - 1) {
    bb[blockIdx.x] = tb;
    br[blockIdx.x] = tr;
    bt[blockIdx.x] = term;
  }
}

// one block: where the scan ends, the blocks' first output byte and first marker index (in place), the totals, the first and last interval start
__global__ __launch_bounds__(JD_SCAN_THREADS) void jd_offsets_kernel(uint32_t* __restrict__ bb, uint32_t* __restrict__ br, const uint32_t* __restrict__ bt, uint32_t nblocks,
                                                                     uint32_t len, uint32_t nint, uint32_t* __restrict__ ctl, uint32_t* __restrict__ istart) {
  __shared__ uint32_t sh[JD_SCAN_THREADS];
  uint32_t term = JD_NONE;
  for (uint32_t base = 0; base < nblocks; base += JD_SCAN_THREADS) {
    const uint32_t i = base + threadIdx.x;
    if (i < nblocks && bt[i] < term) term = bt[i];
  }
  term = block_min<JD_SCAN_THREADS>(term, sh);
  if (term > len) term = len;
  const uint32_t last = term / JD_BLOCK_BYTES;          // blocks behind it hold nothing of the scan
  uint32_t cb = 0, cr = 0;
  for (uint32_t base = 0; base < nblocks; base += JD_SCAN_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const bool in = i < nblocks && i <= last;
    const uint32_t vb = in ? bb[i] : 0u, vr = in ? br[i] : 0u;
    const uint32_t ib = block_incl_scan<JD_SCAN_THREADS>(vb, sh);
    const uint32_t tb = sh[JD_SCAN_THREADS - 1];
    __syncthreads();
    const uint32_t ir = block_incl_scan<JD_SCAN_THREADS>(vr, sh);
    const uint32_t tr = sh[JD_SCAN_THREADS - 1];
    __syncthreads();
    if (i < nblocks) {
      bb[i] = cb + ib - vb;
      br[i] = cr + ir - vr;
    }
    cb += tb;
    cr += tr;
  }
  if (threadIdx.x == 0) {
    ctl[CTL_TERM] = term;
    ctl[CTL_BYTES] = cb;
    ctl[CTL_RST] = cr;
    istart[0] = 0;
    istart[nint] = cb;
    if (cr != nint - 1) ctl[CTL_STATUS] = ST_MARKERS;
  }
}

__global__ __launch_bounds__(JD_THREADS) void jd_scatter_kernel(const uint8_t* __restrict__ d, const uint32_t* __restrict__ bb, const uint32_t* __restrict__ br,
                                                                uint32_t nint, uint32_t* __restrict__ ctl, uint8_t* __restrict__ out, uint32_t* __restrict__ istart) {
  __shared__ uint32_t sh[JD_THREADS];
  const uint32_t term = ctl[CTL_TERM], total = ctl[CTL_BYTES];
  const uint32_t first = blockIdx.x * (uint32_t)JD_BLOCK_BYTES + threadIdx.x * (uint32_t)JD_CHUNK;
  uint32_t nb = 0, nr = 0;
  for (int k = 0; k < JD_CHUNK; ++k) {
    const uint32_t i = first + k;
    if (i < term) {
      const int c = jd_classify(d, i);
      nb += (c == K_BYTE || c == K_FF);
      nr += (c == K_RST);
    }
  }
  const uint32_t ib = block_incl_scan<JD_THREADS>(nb, sh);
  __syncthreads();
  const uint32_t ir = block_incl_scan<JD_THREADS>(nr, sh);
  uint32_t ob = bb[blockIdx.x] + ib - nb, orst = br[blockIdx.x] + ir - nr;
  bool bad = false;
  for (int k = 0; k < JD_CHUNK; ++k) {
    const uint32_t i = first + k;
    if (i >= term) break;
    const int c = jd_classify(d, i);
    if (c == K_BYTE || c == K_FF) {
      if (ob < total) out[ob] = c == K_FF ? (uint8_t)0xff : d[i];
      ++ob;
    } else if (c == K_RST) {
      if (orst + 1 < nint && (uint32_t)(d[i] - 0xd0) == (orst & 7u)) istart[orst + 1] = ob;
      else bad = true;
      ++orst;
    }
  }
  if (bad) ctl[CTL_STATUS] = ST_MARKERS;
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. entropy decoding
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jd_tables_kernel(JdTables t, HuffDec* __restrict__ huff) {
  if (threadIdx.x != 0) return;
  const int id = blockIdx.x;
  HuffDec& h = huff[id];
  for (int i = 0; i < 256; ++i) { h.look[i] = 0; h.vals[i] = t.vals[id][i]; }
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = t.counts[id][l - 1];
    h.valoff[l] = k - code;
    h.maxcode[l] = n ? code + n - 1 : -1;
    if (code + n > (1 << l)) h.maxcode[l] = n ? (1 << l) - 1 : -1;          // (an oversubscribed table is refused on the host; the bound holds regardless)
    if (l <= 8)
      for (int c = code; c < code + n && c < (1 << l); ++c)
        for (int f = 0; f < (1 << (8 - l)); ++f) h.look[((c << (8 - l)) | f) & 255] = (uint16_t)(l << 8 | t.vals[id][(k + c - code) & 255]);
    code = (code + n) << 1;
    k += n;
  }
  h.maxcode[0] = -1;
  h.valoff[0] = 0;
}

// per interval: its sub-sequence count (scanned into sfirst by jd_scan_kernel)
__global__ __launch_bounds__(JD_THREADS) void jd_plan_kernel(const uint32_t* __restrict__ istart, uint32_t nint, uint32_t s, const uint32_t* __restrict__ ctl,
                                                             uint32_t* __restrict__ nsub) {
  const uint32_t k = blockIdx.x * (uint32_t)JD_THREADS + threadIdx.x;
  if (k >= nint || ctl[CTL_STATUS] != ST_OK) return;
  const uint32_t a = istart[k], b = istart[k + 1];
  const unsigned long long bits = b > a ? 8ull * (b - a) : 0ull;
  uint32_t n = 1;
  if (s && bits > s) n = (uint32_t)((bits + s - 1) / s);
  nsub[k] = n;
}

struct JdState { uint32_t p, b, z; };
__device__ __forceinline__ unsigned long long jd_pack(uint32_t p, uint32_t b, uint32_t z) { return (unsigned long long)p | (unsigned long long)b << 32 | (unsigned long long)z << 40; }

// 32 bits from bit position p of an interval of nbytes bytes; zero bits behind its end
__device__ __forceinline__ uint32_t jd_peek32(const uint8_t* __restrict__ s, uint32_t nbytes, uint32_t p) {
  const uint32_t i = p >> 3;
  unsigned long long w = 0;
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) w = w << 8 | (i + k < nbytes ? s[i + k] : 0u);
  return (uint32_t)(w >> (8 - (p & 7)));
}

__device__ __forceinline__ bool jd_symbol(const HuffDec& h, uint32_t w, uint32_t& len, uint32_t& sym) {
  const uint32_t l = h.look[w >> 24];
  if (l) { len = l >> 8; sym = l & 255; return true; }
  for (uint32_t n = 9; n <= 16; ++n) {
    const int32_t c = (int32_t)(w >> (32 - n));
    if (c <= h.maxcode[n]) { len = n; sym = h.vals[(h.valoff[n] + c) & 255]; return true; }
  }
  len = 1; sym = 0;          // an undefined code: one bit is skipped (the write pass reports it)
  return false;
}

// f_i: decode from `st` until the position passes `end`.  WRITE: into the coefficient planes, blocks first .. limit of the scan's order; returns
// false after a code or run no valid stream holds inside those blocks.
template <bool WRITE>
__device__ __forceinline__ bool jd_run(const JdGeom& g, const HuffDec* __restrict__ huff, const uint8_t* __restrict__ s, uint32_t nbytes, uint32_t end, JdState& st,
                                       uint32_t& nblk, int16_t* __restrict__ coefs, long long blk, long long limit) {
  uint32_t p = st.p, b = st.b, z = st.z;
  bool ok = true;
  const uint32_t steps = end > p ? end - p : 0u;          // a symbol takes at least one bit
  int16_t* dst = nullptr;
  if (WRITE && blk < limit) {
    const long long mcu = blk / g.bpm;
    const int c = g.blk_comp[b], my = (int)(mcu / g.mcux), mx = (int)(mcu % g.mcux);
    dst = coefs + (g.plane[c] + (long long)(my * g.v[c] + g.blk_by[b]) * (g.mcux * g.h[c]) + mx * g.h[c] + g.blk_bx[b]) * 64;
  }
  for (uint32_t it = 0; it < steps && p < end; ++it) {
    if (WRITE && blk >= limit) break;
    const uint32_t w = jd_peek32(s, nbytes, p);
    const int c = g.blk_comp[b];
    uint32_t len, sym;
    if (z == 0) {
      bool good = jd_symbol(huff[g.dc[c]], w, len, sym);
      if (sym > 15) { good = false; sym &= 15; }
      const uint32_t extra = sym ? (w << len) >> (32 - sym) : 0u;
      if (WRITE) {
        ok = ok && good;
        dst[0] = (int16_t)(sym && extra < (1u << (sym - 1)) ? (int)extra - (1 << sym) + 1 : (int)extra);
      }
      p += len + sym;
      z = 1;
    } else {
      bool good = jd_symbol(huff[4 + g.ac[c]], w, len, sym);
      const uint32_t run = sym >> 4, size = sym & 15;
      if (size == 0) {
        if (run == 15) z += 16;
        else { good = good && run == 0; z = 64; }
        p += len;
        if (z > 64) { good = false; z = 64; }
      } else {
        z += run;
        const uint32_t extra = (w << len) >> (32 - size);
        if (z > 63) { good = false; z = 64; }
        else {
          if (WRITE) dst[z] = (int16_t)(extra < (1u << (size - 1)) ? (int)extra - (1 << size) + 1 : (int)extra);
          ++z;
        }
        p += len + size;
      }
      if (WRITE) ok = ok && good;
    }
    if (z >= 64) {
      z = 0;
      b = b + 1 < (uint32_t)g.bpm ? b + 1 : 0u;
      ++nblk;
      if (WRITE) {
        ++blk;
        if (blk < limit) {
          const long long mcu = blk / g.bpm;
          const int c2 = g.blk_comp[b], my = (int)(mcu / g.mcux), mx = (int)(mcu % g.mcux);
          dst = coefs + (g.plane[c2] + (long long)(my * g.v[c2] + g.blk_by[b]) * (g.mcux * g.h[c2]) + mx * g.h[c2] + g.blk_bx[b]) * 64;
        }
      }
    }
  }
  st.p = p; st.b = b; st.z = z;
  return ok;
}

__device__ __forceinline__ void jd_load_tables(const HuffDec* __restrict__ huff, HuffDec* sh) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(huff);
  uint32_t* dst = reinterpret_cast<uint32_t*>(sh);
  for (uint32_t i = threadIdx.x; i < 8 * sizeof(HuffDec) / 4; i += JD_THREADS) dst[i] = src[i];
  __syncthreads();
}

// the interval of sub-sequence gi: the last k with sfirst[k] <= gi
__device__ __forceinline__ uint32_t jd_interval_of(const uint32_t* __restrict__ sfirst, uint32_t nint, uint32_t gi) {
  uint32_t lo = 0, hi = nint;
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (sfirst[mid] <= gi) lo = mid; else hi = mid;
  }
  return lo;
}

struct JdSub { uint32_t k, j, a, nbytes, end; };
__device__ __forceinline__ JdSub jd_sub(const JdGeom& g, const uint32_t* __restrict__ istart, const uint32_t* __restrict__ sfirst, uint32_t k, uint32_t gi) {
  JdSub u;
  u.k = k;
  u.j = gi - sfirst[k];
  u.a = istart[k];
  const uint32_t b = istart[k + 1];
  u.nbytes = b > u.a ? b - u.a : 0u;
  const unsigned long long bits = 8ull * u.nbytes, e = g.s ? (unsigned long long)(u.j + 1) * (unsigned long long)g.s : bits;
  u.end = (uint32_t)(e < bits ? e : bits);
  return u;
}

// INIT: round 0, every sub-sequence from its blind start (the first of an interval from the true one).  Otherwise up to rmax rounds inside the
// block: a thread whose predecessor's exit state is not the state it last started from decodes again; the block's first thread reads its
// predecessor, another block's, once per launch.  hits[r] is set when round r changed a state anywhere.
template <bool INIT>
__global__ __launch_bounds__(JD_THREADS) void jd_decode_kernel(JdGeom g, const HuffDec* __restrict__ huff, const uint8_t* __restrict__ stream, const uint32_t* __restrict__ istart,
                                                               const uint32_t* __restrict__ sfirst, uint32_t* __restrict__ ctl, unsigned long long* __restrict__ E,
                                                               unsigned long long* __restrict__ in, uint32_t* __restrict__ cnt, uint32_t* __restrict__ subk, int rmax) {
  __shared__ HuffDec tabs[8];
  __shared__ unsigned long long sE[JD_THREADS];
  if (ctl[CTL_STATUS] != ST_OK) return;
  jd_load_tables(huff, tabs);
  const uint32_t n = ctl[CTL_NSUB];
  const uint32_t t = threadIdx.x, gi = blockIdx.x * (uint32_t)JD_THREADS + t;
  const bool active = gi < n;
  if (INIT) {
    if (!active) return;
    const uint32_t k = jd_interval_of(sfirst, (uint32_t)g.nint, gi);
    const JdSub u = jd_sub(g, istart, sfirst, k, gi);
    JdState st = {u.j * (uint32_t)g.s, 0u, 0u};
    const unsigned long long from = jd_pack(st.p, 0, 0);
    uint32_t nb = 0;
    jd_run<false>(g, tabs, stream + u.a, u.nbytes, u.end, st, nb, nullptr, 0, 0);
    E[gi] = jd_pack(st.p, st.b, st.z);
    in[gi] = from;
    cnt[gi] = nb;
    subk[gi] = k;
    return;
  }
  JdSub u = {0, 0, 0, 0, 0};
  unsigned long long myE = 0, myin = 0, predG = 0;
  uint32_t mycnt = 0;
  bool moving = false;
  if (active) {
    u = jd_sub(g, istart, sfirst, subk[gi], gi);
    moving = u.j > 0;
    myE = E[gi]; myin = in[gi]; mycnt = cnt[gi];
    if (moving && t == 0) predG = E[gi - 1];
  }
  sE[t] = myE;
  __syncthreads();
  bool touched = false;
  for (int r = 0; r < rmax; ++r) {
    int ch = 0;
    if (moving) {
      const unsigned long long pred = t == 0 ? predG : sE[t - 1];
      if (pred != myin) {
        JdState st = {(uint32_t)pred, (uint32_t)(pred >> 32) & 255u, (uint32_t)(pred >> 40) & 255u};
        if (st.b >= (uint32_t)g.bpm) st.b = 0;
        uint32_t nb = 0;
        jd_run<false>(g, tabs, stream + u.a, u.nbytes, u.end, st, nb, nullptr, 0, 0);
        myE = jd_pack(st.p, st.b, st.z);
        myin = pred;
        mycnt = nb;
        ch = 1;
        touched = true;
      }
    }
    __syncthreads();
    if (ch) sE[t] = myE;
    if (!__syncthreads_or(ch)) break;
    if (t == 0) ctl[CTL_HITS + r] = 1;
  }
  if (touched) { E[gi] = myE; in[gi] = myin; cnt[gi] = mycnt; }
}

// every sub-sequence once more, from its verified start state, into the (zeroed) coefficients: DC as a difference
__global__ __launch_bounds__(JD_THREADS) void jd_write_kernel(JdGeom g, const HuffDec* __restrict__ huff, const uint8_t* __restrict__ stream, const uint32_t* __restrict__ istart,
                                                              const uint32_t* __restrict__ sfirst, uint32_t* __restrict__ ctl, const unsigned long long* __restrict__ E,
                                                              const uint32_t* __restrict__ cbase, const uint32_t* __restrict__ subk, int16_t* __restrict__ coefs) {
  __shared__ HuffDec tabs[8];
  if (ctl[CTL_STATUS] != ST_OK) return;
  jd_load_tables(huff, tabs);
  const uint32_t n = ctl[CTL_NSUB];
  const uint32_t gi = blockIdx.x * (uint32_t)JD_THREADS + threadIdx.x;
  if (gi >= n) return;
  const uint32_t k = subk[gi];
  if (k >= (uint32_t)g.nint) return;
  const JdSub u = jd_sub(g, istart, sfirst, k, gi);
  JdState st = {0u, 0u, 0u};
  if (u.j > 0) {
    const unsigned long long pred = E[gi - 1];
    st.p = (uint32_t)pred; st.b = (uint32_t)(pred >> 32) & 255u; st.z = (uint32_t)(pred >> 40) & 255u;
    if (st.b >= (uint32_t)g.bpm || st.z > 63) { ctl[CTL_STATUS] = ST_CODE; return; }
  }
  const long long mcus = (long long)g.mcux * g.mcuy, m0 = (long long)k * g.ri, m1 = m0 + g.ri < mcus ? m0 + g.ri : mcus;
  const long long blk = m0 * g.bpm + (long long)(cbase[gi] - cbase[sfirst[k]]), limit = m1 * g.bpm;
  uint32_t nb = 0;
  if (!jd_run<true>(g, tabs, stream + u.a, u.nbytes, u.end, st, nb, coefs, blk, limit)) ctl[CTL_STATUS] = ST_CODE;
}

// per (interval, component): the block count of the interval is checked, the DC differences become DC values (a chunked block scan in scan order)
__global__ __launch_bounds__(JD_THREADS) void jd_dc_kernel(JdGeom g, const uint32_t* __restrict__ sfirst, const uint32_t* __restrict__ cbase, const uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ ctl, int16_t* __restrict__ coefs) {
  __shared__ uint32_t sh[JD_THREADS];
  if (ctl[CTL_STATUS] != ST_OK) return;
  const uint32_t k = blockIdx.x;
  const int c = blockIdx.y;
  const long long mcus = (long long)g.mcux * g.mcuy, m0 = (long long)k * g.ri, m1 = m0 + g.ri < mcus ? m0 + g.ri : mcus;
  const uint32_t lastsub = sfirst[k + 1] - 1;
  const long long have = (long long)(cbase[lastsub] + cnt[lastsub] - cbase[sfirst[k]]);
  if (have < (m1 - m0) * g.bpm) {          // (uniform over the block)
    if (threadIdx.x == 0) ctl[CTL_STATUS] = ST_BLOCKS;
    return;
  }
  const int hv = g.h[c] * g.v[c];
  const long long count = (m1 - m0) * hv;
  uint32_t carry = 0;
  for (long long base = 0; base < count; base += JD_THREADS) {
    const long long qi = base + threadIdx.x;
    int16_t* at = nullptr;
    uint32_t v = 0;
    if (qi < count) {
      const long long mcu = m0 + qi / hv;
      const int sub = (int)(qi % hv), my = (int)(mcu / g.mcux), mx = (int)(mcu % g.mcux);
      at = coefs + (g.plane[c] + (long long)(my * g.v[c] + sub / g.h[c]) * (g.mcux * g.h[c]) + mx * g.h[c] + sub % g.h[c]) * 64;
      v = (uint32_t)(int)*at;
    }
    const uint32_t incl = block_incl_scan<JD_THREADS>(v, sh);
    if (at) *at = (int16_t)(carry + incl);
    carry += sh[JD_THREADS - 1];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. pixels
// ---------------------------------------------------------------------------------------------------------------------
// libjpeg's jpeg_idct_islow (13-bit constants, PASS1_BITS 2) on one vector of 8: products in 64 bits
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(const long long* x, long long* y) {
  long long z2 = x[2], z3 = x[6];
  long long z1 = (z2 + z3) * 4433;
  long long tmp2 = z1 - z3 * 15137, tmp3 = z1 + z2 * 6270;
  long long tmp0 = (x[0] + x[4]) * 8192, tmp1 = (x[0] - x[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const long long half = 1ll << (SHIFT - 1);
  y[0] = (tmp10 + tmp3 + half) >> SHIFT; y[7] = (tmp10 - tmp3 + half) >> SHIFT;
  y[1] = (tmp11 + tmp2 + half) >> SHIFT; y[6] = (tmp11 - tmp2 + half) >> SHIFT;
  y[2] = (tmp12 + tmp1 + half) >> SHIFT; y[5] = (tmp12 - tmp1 + half) >> SHIFT;
  y[3] = (tmp13 + tmp0 + half) >> SHIFT; y[4] = (tmp13 - tmp0 + half) >> SHIFT;
}

// one thread per block: dequantise, columns then rows, + 128, clamp -> 8 x 8 samples of the component's plane (whole MCUs wide)
__global__ __launch_bounds__(JD_THREADS) void jd_idct_kernel(JdGeom g, const int16_t* __restrict__ coefs, const uint32_t* __restrict__ ctl, uint8_t* __restrict__ planes) {
  const long long bi = (long long)blockIdx.x * JD_THREADS + threadIdx.x;
  if (bi >= g.plane[g.ncomp] || ctl[CTL_STATUS] != ST_OK) return;
  int c = 0;
  if (g.ncomp > 1 && bi >= g.plane[1]) c = bi >= g.plane[2] ? 2 : 1;
  const long long local = bi - g.plane[c];
  const int cols = g.mcux * g.h[c], row = (int)(local / cols), col = (int)(local % cols);
  const int16_t* src = coefs + bi * 64;
  constexpr uint8_t zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  long long blk[64], ws[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) blk[zigzag[i]] = (long long)src[i] * g.q[c][i];
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    long long in[8], out[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = blk[y * 8 + x];
    jd_idct8<11>(in, out);
#pragma unroll
    for (int y = 0; y < 8; ++y) ws[y * 8 + x] = out[y];
  }
  uint8_t* dst = planes + g.pix[c] + ((long long)row * 8) * (cols * 8) + col * 8;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    long long out[8];
    jd_idct8<18>(ws + y * 8, out);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      long long v = out[x] + 128;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      if (x < 4) lo |= (uint32_t)v << (8 * x); else hi |= (uint32_t)v << (8 * (x - 4));
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(dst + (long long)y * (cols * 8));
    o[0] = lo; o[1] = hi;
  }
}

// a chroma sample at full resolution: libjpeg's h2v1 / h2v2 "fancy" up-sampling on the plane cropped to ch x cw (neighbours outside it are the
// edge sample); a plane of at most two columns is replicated instead, as libjpeg does
__device__ __forceinline__ int jd_chroma(const JdGeom& g, const uint8_t* __restrict__ p, int pitch, int cw, int ch, int y, int x) {
  if (g.hmax == 1) return p[(long long)y * pitch + x];
  const int i = x >> 1;
  if (g.vmax == 1) {
    const uint8_t* r = p + (long long)y * pitch;
    if (cw <= 2) return r[i];
    const int o = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    return (3 * r[i] + r[o] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int j = y >> 1;
  if (cw <= 2) return p[(long long)j * pitch + i];
  const int jo = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
  const int o = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
  const uint8_t *r0 = p + (long long)j * pitch, *r1 = p + (long long)jo * pitch;
  const int a = 3 * r0[i] + r1[i], b = 3 * r0[o] + r1[o];
  return (3 * a + b + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ uint32_t jd_clamp8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// four pixels of the flat [H * W] order per thread: 12 bytes = three aligned words
__global__ __launch_bounds__(JD_THREADS) void jd_colour_kernel(JdGeom g, const uint8_t* __restrict__ planes, const uint32_t* __restrict__ ctl, uint8_t* __restrict__ out) {
  const long long npix = (long long)g.H * g.W, first = ((long long)blockIdx.x * JD_THREADS + threadIdx.x) * 4;
  if (first >= npix || ctl[CTL_STATUS] != ST_OK) return;
  const int ypitch = g.mcux * g.h[0] * 8;
  const int cpitch = g.ncomp == 3 ? g.mcux * 8 : 0;
  const int cw = (g.W + g.hmax - 1) / g.hmax, ch = (g.H + g.vmax - 1) / g.vmax;
  uint8_t px[12];
  int y = (int)(first / g.W), x = (int)(first % g.W);
  const int n = npix - first < 4 ? (int)(npix - first) : 4;
  for (int k = 0; k < n; ++k) {
    const int Y = planes[g.pix[0] + (long long)y * ypitch + x];
    if (g.ncomp == 1) {
      px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (uint8_t)Y;
    } else {
      const int cb = jd_chroma(g, planes + g.pix[1], cpitch, cw, ch, y, x) - 128, cr = jd_chroma(g, planes + g.pix[2], cpitch, cw, ch, y, x) - 128;
      px[3 * k] = (uint8_t)jd_clamp8(Y + ((91881 * cr + 32768) >> 16));
      px[3 * k + 1] = (uint8_t)jd_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      px[3 * k + 2] = (uint8_t)jd_clamp8(Y + ((116130 * cb + 32768) >> 16));
    }
    if (++x == g.W) { x = 0; ++y; }
  }
  uint8_t* o = out + first * 3;
  if (n == 4) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k) o4[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
  } else {
    for (int k = 0; k < 3 * n; ++k) o[k] = px[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
constexpr long long JD_MAX_SCAN = 1ll << 28;          // bytes behind SOS: bit positions stay inside 32 bits

const char* jd_plan(const uegan_jpeg_desc* d, int subseq_bits, bool with_coefs, JdPlan& p) {
  if (!d) return "no descriptor";
  if (d->H < 1 || d->W < 1 || d->H > 65535 || d->W > 65535) return "a side is outside 1..65535";
  if (d->ncomp != 1 && d->ncomp != 3) return "not one or three components";
  if (subseq_bits != 0 && (subseq_bits < 128 || subseq_bits % 32 || subseq_bits > (1 << 20))) return "subseq_bits is not 0 (off) or a multiple of 32 in [128, 2^20]";
  if (d->scan_offset < 0 || d->scan_length < 1 || d->scan_length > JD_MAX_SCAN) return "the scan's length is outside 1..2^28";
  if (d->restart_interval < 0 || d->restart_interval > 65535) return "the restart interval is outside 0..65535";
  JdGeom& g = p.g;
  memset(&g, 0, sizeof(g));
  g.H = d->H; g.W = d->W; g.ncomp = d->ncomp; g.s = subseq_bits;
  if (g.ncomp == 1) {
    g.hmax = g.vmax = 1;
    g.h[0] = g.v[0] = 1;
  } else {
    g.hmax = d->h[0]; g.vmax = d->v[0];
    if (!((g.hmax == 1 && g.vmax == 1) || (g.hmax == 2 && g.vmax == 1) || (g.hmax == 2 && g.vmax == 2)) || d->h[1] != 1 || d->v[1] != 1 || d->h[2] != 1 || d->v[2] != 1)
      return "the sampling is not 4:4:4, 4:2:2 or 4:2:0";
    for (int c = 0; c < 3; ++c) { g.h[c] = d->h[c]; g.v[c] = d->v[c]; }
  }
  g.mcux = (g.W + 8 * g.hmax - 1) / (8 * g.hmax);
  g.mcuy = (g.H + 8 * g.vmax - 1) / (8 * g.vmax);
  const long long mcus = (long long)g.mcux * g.mcuy;
  if (mcus * g.hmax * g.vmax * 64 > (1ll << 28)) return "the padded area is above 2^28 pixels";
  g.ri = d->restart_interval ? d->restart_interval : (int)(mcus < 0x7fffffff ? mcus : 0x7fffffff);
  g.nint = (int)((mcus + g.ri - 1) / g.ri);
  long long blocks = 0, bytes = 0;
  for (int c = 0; c < g.ncomp; ++c) {
    if (d->tq[c] < 0 || d->tq[c] > 3 || d->td[c] < 0 || d->td[c] > 3 || d->ta[c] < 0 || d->ta[c] > 3) return "a table id is outside 0..3";
    g.dc[c] = d->td[c]; g.ac[c] = d->ta[c];
    memcpy(g.q[c], d->quant[d->tq[c]], 64);
    g.plane[c] = blocks; g.pix[c] = bytes;
    for (int by = 0; by < g.v[c]; ++by)
      for (int bx = 0; bx < g.h[c]; ++bx) { g.blk_comp[g.bpm] = c; g.blk_by[g.bpm] = by; g.blk_bx[g.bpm] = bx; ++g.bpm; }
    blocks += mcus * g.h[c] * g.v[c];
    bytes += (mcus * g.h[c] * g.v[c] * 64 + 255) & ~255ll;
  }
  g.plane[g.ncomp] = blocks;
  for (int t = 0; t < 4; ++t) {
    int ndc = 0, nac = 0;
    for (int i = 0; i < 16; ++i) { ndc += d->dc[t].counts[i]; nac += d->ac[t].counts[i]; }
    if (ndc > 256 || nac > 256) return "a Huffman table holds more than 256 symbols";
  }
  p.len = (uint32_t)d->scan_length;
  p.nblocks = (p.len + JD_BLOCK_BYTES - 1) / JD_BLOCK_BYTES;
  const unsigned long long nmax = (subseq_bits ? (8ull * p.len + subseq_bits - 1) / subseq_bits : 0ull) + (unsigned long long)g.nint;
  if (nmax > 0x7fffffffull) return "too many sub-sequences";
  p.nmax = (uint32_t)nmax;
  size_t o = 0;
  p.o_ctl = o;     o += jd_up(CTL_WORDS * 4);
  p.o_huff = o;    o += jd_up(8 * sizeof(HuffDec));
  p.o_bb = o;      o += jd_up((size_t)p.nblocks * 4);
  p.o_br = o;      o += jd_up((size_t)p.nblocks * 4);
  p.o_bt = o;      o += jd_up((size_t)p.nblocks * 4);
  p.o_stream = o;  o += jd_up((size_t)p.len + 16);
  p.o_istart = o;  o += jd_up(((size_t)g.nint + 1) * 4);
  p.o_sfirst = o;  o += jd_up(((size_t)g.nint + 1) * 4);
  p.o_e = o;       o += jd_up((size_t)p.nmax * 8);
  p.o_in = o;      o += jd_up((size_t)p.nmax * 8);
  p.o_cnt = o;     o += jd_up((size_t)p.nmax * 4);
  p.o_cbase = o;   o += jd_up(((size_t)p.nmax + 1) * 4);
  p.o_subk = o;    o += jd_up((size_t)p.nmax * 4);
  p.o_coefs = o;   o += with_coefs ? jd_up((size_t)blocks * 128) : 0;
  p.o_planes = o;  o += jd_up((size_t)bytes);
  p.ws_bytes = o;
  return nullptr;
}

int jd_read_ctl(const uint32_t* ctl, uint32_t* host, hipStream_t s) {
#ifdef UEGAN_EMU
  (void)s;
  if (hipMemcpy(host, ctl, CTL_WORDS * 4, hipMemcpyDeviceToHost) != hipSuccess) { set_error("jpeg_decode: reading the control words failed"); return UEGAN_E_HIP; }
#else
  if (hipMemcpyAsync(host, ctl, CTL_WORDS * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("jpeg_decode: reading the control words failed");
    return UEGAN_E_HIP;
  }
#endif
  return UEGAN_OK;
}

int jd_status(uint32_t st) {
  if (st == ST_OK) return UEGAN_OK;
  set_error(st == ST_MARKERS ? "jpeg_decode: the restart markers are not the %s"
            : st == ST_CODE  ? "jpeg_decode: the stream holds a code or a run that %s"
                             : "jpeg_decode: a restart interval holds fewer blocks than %s",
            st == ST_MARKERS ? "count and sequence the header sets" : st == ST_CODE ? "its tables do not define" : "the header sets");
  return UEGAN_E_JPEG_STREAM;
}

hipEvent_t* jd_events() {
  static hipEvent_t ev[5];
  static bool made = false;
  if (!made) {
    for (int i = 0; i < 5; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) return nullptr;
    made = true;
  }
  return ev;
}

// stats (host, optional): [0] rounds used, [1] sub-sequences, [2] restart intervals, [3] bytes of the plain stream;
// stage_ms (host, optional): unstuff, rounds, write pass + DC, pixels
int jd_run_all(const uint8_t* file, const uegan_jpeg_desc* d, int subseq_bits, int max_rounds, int16_t* coeffs_out, uint8_t* pixels, int32_t* stats, float* stage_ms,
               void* workspace, hipStream_t s) {
  UEGAN_CHECK_ARG(file && d && workspace && (coeffs_out || pixels), "bad jpeg_decode args");
  UEGAN_CHECK_ARG(max_rounds >= 1, "jpeg_decode: max_rounds %d is below 1", max_rounds);
  JdPlan p;
  const char* why = jd_plan(d, subseq_bits, coeffs_out == nullptr, p);
  UEGAN_CHECK_ARG(!why, "jpeg_decode: %s", why);
  UEGAN_CHECK_ARG((uintptr_t)workspace % 16 == 0 && (!pixels || (uintptr_t)pixels % 16 == 0) && (!coeffs_out || (uintptr_t)coeffs_out % 16 == 0),
                  "jpeg_decode: the workspace, the pixels and the coefficients must be 16-byte aligned");
  const JdGeom& g = p.g;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* ctl = reinterpret_cast<uint32_t*>(ws + p.o_ctl);
  HuffDec* huff = reinterpret_cast<HuffDec*>(ws + p.o_huff);
  uint32_t *bb = reinterpret_cast<uint32_t*>(ws + p.o_bb), *br = reinterpret_cast<uint32_t*>(ws + p.o_br), *bt = reinterpret_cast<uint32_t*>(ws + p.o_bt);
  uint8_t* stream = ws + p.o_stream;
  uint32_t *istart = reinterpret_cast<uint32_t*>(ws + p.o_istart), *sfirst = reinterpret_cast<uint32_t*>(ws + p.o_sfirst);
  unsigned long long *E = reinterpret_cast<unsigned long long*>(ws + p.o_e), *in = reinterpret_cast<unsigned long long*>(ws + p.o_in);
  uint32_t *cnt = reinterpret_cast<uint32_t*>(ws + p.o_cnt), *cbase = reinterpret_cast<uint32_t*>(ws + p.o_cbase), *subk = reinterpret_cast<uint32_t*>(ws + p.o_subk);
  int16_t* coefs = coeffs_out ? coeffs_out : reinterpret_cast<int16_t*>(ws + p.o_coefs);
  uint8_t* planes = ws + p.o_planes;
  const uint8_t* data = file + d->scan_offset;
  hipEvent_t* ev = stage_ms ? jd_events() : nullptr;
  UEGAN_CHECK_ARG(!stage_ms || ev, "jpeg_decode: creating the timing events failed");
  if (ev) (void)hipEventRecord(ev[0], s);

  // 1. unstuff
  UEGAN_CHECK_ARG(hipMemsetAsync(ctl, 0, CTL_WORDS * 4, s) == hipSuccess && hipMemsetAsync(istart, 0, ((size_t)g.nint + 1) * 4, s) == hipSuccess &&
                  hipMemsetAsync(subk, 0xff, (size_t)p.nmax * 4, s) == hipSuccess, "jpeg_decode: clearing the workspace failed");
  {
    JdTables t;
    for (int i = 0; i < 4; ++i) {
      memcpy(t.counts[i], d->dc[i].counts, 16); memcpy(t.vals[i], d->dc[i].symbols, 256);
      memcpy(t.counts[4 + i], d->ac[i].counts, 16); memcpy(t.vals[4 + i], d->ac[i].symbols, 256);
    }
    hipLaunchKernelGGL(jd_tables_kernel, dim3(8), dim3(64), 0, s, t, huff);
    UEGAN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(jd_count_kernel, dim3(p.nblocks), dim3(JD_THREADS), 0, s, data, p.len, bb, br, bt);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_offsets_kernel, dim3(1), dim3(JD_SCAN_THREADS), 0, s, bb, br, bt, p.nblocks, p.len, (uint32_t)g.nint, ctl, istart);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_scatter_kernel, dim3(p.nblocks), dim3(JD_THREADS), 0, s, data, bb, br, (uint32_t)g.nint, ctl, stream, istart);
  UEGAN_CHECK_LAUNCH();
  if (ev) (void)hipEventRecord(ev[1], s);

  // 2. the sub-sequences of every interval, round 0
  const uint32_t iblocks = ((uint32_t)g.nint + JD_THREADS - 1) / JD_THREADS, sblocks = (p.nmax + JD_THREADS - 1) / JD_THREADS;
  hipLaunchKernelGGL(jd_plan_kernel, dim3(iblocks), dim3(JD_THREADS), 0, s, istart, (uint32_t)g.nint, (uint32_t)g.s, ctl, cbase);      // (cbase: scratch for the counts)
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_scan_kernel, dim3(1), dim3(JD_SCAN_THREADS), 0, s, cbase, sfirst, ctl, -1, (uint32_t)g.nint, (int)CTL_NSUB);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL((jd_decode_kernel<true>), dim3(sblocks), dim3(JD_THREADS), 0, s, g, huff, stream, istart, sfirst, ctl, E, in, cnt, subk, 0);
  UEGAN_CHECK_LAUNCH();
  uint32_t host[CTL_WORDS];
  int rc = jd_read_ctl(ctl, host, s);
  if (rc != UEGAN_OK) return rc;
  if (stats) { stats[0] = 0; stats[1] = (int32_t)host[CTL_NSUB]; stats[2] = g.nint; stats[3] = (int32_t)host[CTL_BYTES]; }
  if (host[CTL_STATUS] != ST_OK) return jd_status(host[CTL_STATUS]);
  const uint32_t nsub = host[CTL_NSUB];
  UEGAN_CHECK_ARG(nsub >= (uint32_t)g.nint && nsub <= p.nmax, "jpeg_decode: %u sub-sequences for %d intervals and a bound of %u", nsub, g.nint, p.nmax);
  long long rounds = 1;
  if (nsub > (uint32_t)g.nint) {          // an interval longer than a sub-sequence: iterate to the fixed point
    const uint32_t used = (nsub + JD_THREADS - 1) / JD_THREADS;
    const long long hard = (long long)nsub + (long long)JD_ROUNDS * (used - 1) + 1;
    const long long most = max_rounds < hard ? max_rounds : hard;
    bool fixed = false;
    for (long long launch = 0; launch <= hard && !fixed; ++launch) {
      const long long left = most - rounds;
      const int rmax = left >= JD_ROUNDS ? JD_ROUNDS : (left > 0 ? (int)left : 1);      // (left == 0: one round more tells whether the last one reached the fixed point)
      UEGAN_CHECK_ARG(hipMemsetAsync(ctl + CTL_HITS, 0, JD_ROUNDS * 4, s) == hipSuccess, "jpeg_decode: clearing the control words failed");
      hipLaunchKernelGGL((jd_decode_kernel<false>), dim3(used), dim3(JD_THREADS), 0, s, g, huff, stream, istart, sfirst, ctl, E, in, cnt, subk, rmax);
      UEGAN_CHECK_LAUNCH();
      rc = jd_read_ctl(ctl, host, s);
      if (rc != UEGAN_OK) return rc;
      int hits = 0;
      for (int r = 0; r < JD_ROUNDS; ++r) hits += host[CTL_HITS + r] != 0;
      if (hits == 0) { fixed = true; break; }
      if (left <= 0) break;
      rounds += hits;
    }
    if (stats) stats[0] = (int32_t)rounds;
    if (!fixed) {
      set_error("jpeg_decode: the sub-sequences are not synchronised after %lld rounds (max_rounds %d, %u sub-sequences of %d bits)", rounds, max_rounds, nsub, g.s);
      return UEGAN_E_JPEG_DESYNC;
    }
  }
  if (stats) stats[0] = (int32_t)rounds;
  if (ev) (void)hipEventRecord(ev[2], s);

  // the write pass from the verified states, then the DC sums
  hipLaunchKernelGGL(jd_scan_kernel, dim3(1), dim3(JD_SCAN_THREADS), 0, s, cnt, cbase, ctl, (int)CTL_NSUB, p.nmax, -1);
  UEGAN_CHECK_LAUNCH();
  UEGAN_CHECK_ARG(hipMemsetAsync(coefs, 0, (size_t)g.plane[g.ncomp] * 128, s) == hipSuccess, "jpeg_decode: clearing the coefficients failed");
  hipLaunchKernelGGL(jd_write_kernel, dim3((nsub + JD_THREADS - 1) / JD_THREADS), dim3(JD_THREADS), 0, s, g, huff, stream, istart, sfirst, ctl, E, cbase, subk, coefs);
  UEGAN_CHECK_LAUNCH();
  hipLaunchKernelGGL(jd_dc_kernel, dim3(g.nint, g.ncomp), dim3(JD_THREADS), 0, s, g, sfirst, cbase, cnt, ctl, coefs);
  UEGAN_CHECK_LAUNCH();
  if (ev) (void)hipEventRecord(ev[3], s);

  // 3. pixels
  if (pixels) {
    hipLaunchKernelGGL(jd_idct_kernel, dim3((unsigned)((g.plane[g.ncomp] + JD_THREADS - 1) / JD_THREADS)), dim3(JD_THREADS), 0, s, g, coefs, ctl, planes);
    UEGAN_CHECK_LAUNCH();
    const long long groups = ((long long)g.H * g.W + 3) / 4;
    hipLaunchKernelGGL(jd_colour_kernel, dim3((unsigned)((groups + JD_THREADS - 1) / JD_THREADS)), dim3(JD_THREADS), 0, s, g, planes, ctl, pixels);
    UEGAN_CHECK_LAUNCH();
  }
  if (ev) (void)hipEventRecord(ev[4], s);
  rc = jd_read_ctl(ctl, host, s);
  if (rc != UEGAN_OK) return rc;
  if (ev) {
    for (int i = 0; i < 4; ++i) {
      (void)hipEventSynchronize(ev[i + 1]);
      if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) stage_ms[i] = -1.0f;
    }
  }
  return jd_status(host[CTL_STATUS]);
}

}  // namespace
}  // namespace uegan

using namespace uegan;

extern "C" size_t uegan_jpeg_decode_workspace_bytes(const uegan_jpeg_desc* desc, int subseq_bits) {
  JdPlan p;
  return jd_plan(desc, subseq_bits, true, p) ? 0 : p.ws_bytes;
}

extern "C" int uegan_jpeg_decode_coeffs(const uint8_t* file, const uegan_jpeg_desc* desc, int subseq_bits, int max_rounds, int16_t* coeffs, int32_t* stats, void* workspace,
                                        uegan_stream_t stream) {
  UEGAN_CHECK_ARG(coeffs, "jpeg_decode_coeffs: no coefficient buffer");
  return jd_run_all(file, desc, subseq_bits, max_rounds, coeffs, nullptr, stats, nullptr, workspace, (hipStream_t)stream);
}

extern "C" int uegan_jpeg_decode(const uint8_t* file, const uegan_jpeg_desc* desc, int subseq_bits, int max_rounds, uint8_t* pixels, int32_t* stats, float* stage_ms,
                                 void* workspace, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(pixels, "jpeg_decode: no pixel buffer");
  return jd_run_all(file, desc, subseq_bits, max_rounds, nullptr, pixels, stats, stage_ms, workspace, (hipStream_t)stream);
}
