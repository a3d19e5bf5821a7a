// Weight packing: OIHW fp32 master weights -> the OHWI / IHWO matrices of the storage format that the convolution kernels read.
#include "conv_core.h"
#include "launch.h"

namespace uegan {

// ----------------------------------------------------------------------------------------------------
// weight packing: OIHW fp32 [Cout][Cin][KH][KW] -> ohwi [Cout_p][Kp] (k = (kh,kw,ci_padded)) and
//                                                  ihwo [Cin_p ][Kp2] (k = (kh,kw,co_padded)), zero padded
// ----------------------------------------------------------------------------------------------------
// ohwi_lo (optional): what the rounding of each OHWI element left, rn(w - rn(w)) -- the weights as a hi + lo pair (uegan_conv2d_fwd_ex);
// dup 1: input channels [Cin, 2 Cin) of the OHWI copies repeat [0, Cin) (a source that carries ITS lo plane in those channels, uegan_nchw_to_nhwc_pair);
// dup 2: they hold the LO part of [0, Cin) instead (the pair inside ONE matrix: a kernel that reads the source's channels twice multiplies by both)
template <typename T>
__device__ __forceinline__ void st_pair(T* hi, T* lo, size_t i, float v, bool as_lo = false) {
  if (as_lo) {
    T h;
    DT<T>::st(&h, v);
    v -= DT<T>::ld(&h);
  }
  DT<T>::st(hi + i, v);
  if (lo) DT<T>::st(lo + i, v - DT<T>::ld(hi + i));
}
template <typename T>
__global__ void pack_weights_kernel(const float* w, T* ohwi, T* ihwo, int Cout, int Cin, int KH, int KW, int Cout_p, int Cin_p, int Kp,
                                    int Kp2, int Cin_row, T* ohwi_lo = nullptr, int dup = 0) {
  const int taps = KH * KW;
  const size_t n1 = (size_t)Cout_p * Kp, n2 = ihwo ? (size_t)Cin_p * Kp2 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (size_t)gridDim.x * blockDim.x) {
    if (i < n1) {
      const int co = (int)(i / Kp), kk = (int)(i - (size_t)co * Kp);
      float v = 0.f;
      bool as_lo = false;
      if (co < Cout && kk < taps * Cin_p) {
        const int tap = kk / Cin_p;
        int ci = kk - tap * Cin_p;
        if (dup && ci >= Cin && ci < 2 * Cin) { ci -= Cin; as_lo = dup == 2; }
        if (ci < Cin) v = w[((size_t)co * Cin_row + ci) * taps + tap];
      }
      st_pair<T>(ohwi, ohwi_lo, i, v, as_lo);
    } else {
      const size_t j = i - n1;
      const int ci = (int)(j / Kp2), kk = (int)(j - (size_t)ci * Kp2);
      float v = 0.f;
      if (ci < Cin && kk < taps * Cout_p) {
        const int tap = kk / Cout_p, co = kk - tap * Cout_p;
        if (co < Cout) v = w[((size_t)co * Cin_row + ci) * taps + tap];
      }
      DT<T>::st(ihwo + j, v);
    }
  }
}

// All conv weights of one optimizer in ONE launch (uegan_pack_weights_multi): entry e owns the element range [start, start + n1 + n2) of
// the concatenated (OHWI, IHWO) destinations; a thread finds its entry by bisection over the (<= a few hundred) range starts.
template <typename T>
__global__ void pack_weights_multi_kernel(const uegan_pack_entry* __restrict__ tab, int n_entries, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = n_entries - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].start <= i) lo = mid; else hi = mid - 1;
    }
    const uegan_pack_entry& e = tab[lo];
    const long long r = i - e.start;
    const int taps = e.KH * e.KW;
    const long long n1 = (long long)e.Cout_pad * e.Kp;
    const float* w = e.w_oihw;
    if (r < n1) {
      const int co = (int)(r / e.Kp), kk = (int)(r - (long long)co * e.Kp);
      float v = 0.f;
      bool as_lo = false;
      if (co < e.Cout && kk < taps * e.Cin_pad) {
        const int tap = kk / e.Cin_pad;
        int ci = kk - tap * e.Cin_pad;
        if ((e.flags & 3) && ci >= e.Cin && ci < 2 * e.Cin) { ci -= e.Cin; as_lo = (e.flags & 3) == 2; }
        if (ci < e.Cin) v = w[((size_t)co * e.Cin_total + ci) * taps + tap];
      }
      st_pair<T>(static_cast<T*>(e.w_ohwi), static_cast<T*>(e.w_ohwi_lo), (size_t)r, v, as_lo);
    } else {
      const long long j = r - n1;
      const int ci = (int)(j / e.Kp2), kk = (int)(j - (long long)ci * e.Kp2);
      float v = 0.f;
      if (ci < e.Cin && kk < taps * e.Cout_pad) {
        const int tap = kk / e.Cout_pad, co = kk - tap * e.Cout_pad;
        if (co < e.Cout) v = w[((size_t)co * e.Cin_total + ci) * taps + tap];
      }
      DT<T>::st(static_cast<T*>(e.w_ihwo) + j, v);
    }
  }
}

}  // namespace uegan

using namespace uegan;

extern "C" int64_t uegan_packed_k(int64_t k) { return (k + 7) / 8 * 8; }

extern "C" int uegan_pack_weights(int dtype, const float* w_oihw, int Cout, int Cin, int KH, int KW, int Cout_pad, int Cin_pad, void* w_ohwi,
                                  void* w_ihwo, uegan_stream_t stream) {
  return uegan_pack_weights_slice(dtype, w_oihw, Cout, Cin, Cin, KH, KW, Cout_pad, Cin_pad, w_ohwi, w_ihwo, stream);
}

extern "C" int uegan_pack_weights_slice(int dtype, const float* w_oihw, int Cout, int Cin, int Cin_total, int KH, int KW, int Cout_pad,
                                        int Cin_pad, void* w_ohwi, void* w_ihwo, uegan_stream_t stream) {
  return uegan_pack_weights_pair(dtype, w_oihw, Cout, Cin, Cin_total, KH, KW, Cout_pad, Cin_pad, w_ohwi, w_ihwo, nullptr, 0, stream);
}

extern "C" int uegan_pack_weights_pair(int dtype, const float* w_oihw, int Cout, int Cin, int Cin_total, int KH, int KW, int Cout_pad, int Cin_pad,
                                       void* w_ohwi, void* w_ihwo, void* w_ohwi_lo, int dup_cin, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(w_oihw && w_ohwi && Cout_pad >= Cout && Cin_pad >= Cin && Cin_total >= Cin, "bad pack_weights args");
  UEGAN_CHECK_ARG(!w_ohwi_lo || dtype == UEGAN_BF16, "hi + lo pairs exist for the 16-bit storage format");
  UEGAN_CHECK_ARG(dup_cin >= 0 && dup_cin <= 2 && (!dup_cin || 2 * Cin <= Cin_pad), "dup_cin: 0, 1 or 2; the repeated channels must fit the padding (2 Cin <= Cin_pad)");
  UEGAN_CHECK_ARG(dup_cin != 2 || dtype == UEGAN_BF16, "hi + lo pairs exist for the 16-bit storage format");
  const int Kp = (int)uegan_packed_k((int64_t)KH * KW * Cin_pad), Kp2 = (int)uegan_packed_k((int64_t)KH * KW * Cout_pad);
  const size_t total = (size_t)Cout_pad * Kp + (w_ihwo ? (size_t)Cin_pad * Kp2 : 0);
  // (w_ohwi_lo is null unless the storage type is the 16-bit one: checked above)
  UEGAN_DISPATCH_T(dtype, hipLaunchKernelGGL((pack_weights_kernel<T>), dim3(grid_for(total, 2048)), dim3(256), 0, (hipStream_t)stream, w_oihw, (T*)w_ohwi, (T*)w_ihwo,
                                              Cout, Cin, KH, KW, Cout_pad, Cin_pad, Kp, Kp2, Cin_total, (T*)w_ohwi_lo, dup_cin));
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_pack_weights_multi(int dtype, const uegan_pack_entry* table_dev, int n_entries, int64_t total, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(table_dev && n_entries > 0 && total > 0, "bad pack_weights_multi args");
  UEGAN_DISPATCH_T(dtype, hipLaunchKernelGGL((pack_weights_multi_kernel<T>), dim3(grid_for((size_t)total, 4096)), dim3(256), 0, (hipStream_t)stream, table_dev,
                                              n_entries, (long long)total));
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}
