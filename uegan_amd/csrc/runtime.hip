// Process-wide state of the library behind the C ABI: error text, version, launch-variant thresholds, implementation switches, the HIP-event
// profiler and the MFMA layout self-test.
#include "conv_core.h"

#include <stdarg.h>

namespace uegan {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

ConvImpl g_impl = {UEGAN_IMPL_AUTO, true, true, true, true, true};
// launch-variant thresholds (uegan_set_tuning): process-wide, set explicitly through the C ABI -- the library never reads the environment
int g_tuning[UEGAN_TUNE_COUNT] = {256, -1, 0, 192, 192, 0, 1, 1, 1, 1, 1, 1, 1, 1};
int g_abl_stream = 0, g_abl_wide = 0;
#ifdef UEGAN_TOOLS_BUILD
extern "C" int uegan_tools_set_ablation(int stream_wgrad_bits, int wide_variant) {
  g_abl_stream = stream_wgrad_bits;
  g_abl_wide = wide_variant;
  return UEGAN_OK;
}
#endif

bool g_prof_on = false;
std::vector<ProfRecord> g_prof_records;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;
size_t g_prof_used = 0;

// MFMA layout self-test: D = A*B with A = I (16x16 padded in K) and an asymmetric B.
__global__ void selftest_mfma_kernel(float* out) {
  const int lane = threadIdx.x & 63;
  // f32: A[i][k] (k<4): identity block k==i for i<4; B[k][j] = 100*k + j  -> D[i][j] = 100*i + j for i<4
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int ai = lane & 15, ak = lane >> 4;
  acc = mfma_f32(ai == ak ? 1.f : 0.f, 100.f * (lane >> 4) + (lane & 15), acc);
  for (int r = 0; r < 4; ++r) out[lane * 4 + r] = acc[r];
  // bf16: A[i][k] = (k == i) (K = 32), B[k][j] = (8k + j)/2: exactly representable for the rows that matter
  __attribute__((aligned(16))) unsigned short av[8];
  __attribute__((aligned(16))) unsigned short bv[8];
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * (lane >> 4) + e;
    av[e] = f32_to_bf16((lane & 15) == k ? 1.f : 0.f);
    bv[e] = f32_to_bf16((float)(k * 8 + (lane & 15)) * 0.5f);
  }
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
  acc2 = mfma_bf16(*reinterpret_cast<u32x4*>(av), *reinterpret_cast<u32x4*>(bv), acc2);
  for (int r = 0; r < 4; ++r) out[256 + lane * 4 + r] = acc2[r];
  // bf16 32x32x16 (conv_wide.hip): A[i][k] = (k == i) (K = 16); B[k][j] = k + 1, then j + 1  ->  D[i][j] = i + 1 / j + 1 for i < 16
  typedef float f32x16_t __attribute__((ext_vector_type(16)));
  __attribute__((aligned(16))) unsigned short bk[8];
  for (int e = 0; e < 8; ++e) {
    const int k = 8 * (lane >> 5) + e;
    av[e] = f32_to_bf16((lane & 31) == k ? 1.f : 0.f);
    bk[e] = f32_to_bf16((float)(k + 1));
    bv[e] = f32_to_bf16((float)((lane & 31) + 1));
  }
  f32x16_t z16;
  for (int r = 0; r < 16; ++r) z16[r] = 0.f;
  const bf16x8_t a8 = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<u32x4*>(av));
#ifdef UEGAN_HALF_FP16
  const f32x16_t d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, __builtin_bit_cast(bf16x8_t, *reinterpret_cast<u32x4*>(bk)), z16, 0, 0, 0);
  const f32x16_t d2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, __builtin_bit_cast(bf16x8_t, *reinterpret_cast<u32x4*>(bv)), z16, 0, 0, 0);
#else
  const f32x16_t d1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, __builtin_bit_cast(bf16x8_t, *reinterpret_cast<u32x4*>(bk)), z16, 0, 0, 0);
  const f32x16_t d2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, __builtin_bit_cast(bf16x8_t, *reinterpret_cast<u32x4*>(bv)), z16, 0, 0, 0);
#endif
  for (int r = 0; r < 16; ++r) {
    out[512 + lane * 16 + r] = d1[r];
    out[1536 + lane * 16 + r] = d2[r];
  }
}

}  // namespace uegan

using namespace uegan;

extern "C" int uegan_version(void) { return UEGAN_VERSION; }
extern "C" const char* uegan_last_error(void) { return g_err; }

extern "C" int uegan_set_tuning(int knob, int value, int* previous) {
  UEGAN_CHECK_ARG(knob >= 0 && knob < UEGAN_TUNE_COUNT, "unknown tuning knob %d", knob);
  if (previous) *previous = g_tuning[knob];
  g_tuning[knob] = value;
  return UEGAN_OK;
}

extern "C" int uegan_set_conv_impl(int impl) {
  const int old = g_impl.impl;
  g_impl = {impl, true, true, true, true, true};
  if (impl == UEGAN_IMPL_MFMA_REGSTAGE) { g_impl.impl = UEGAN_IMPL_MFMA; g_impl.glds = false; g_impl.heads = false; g_impl.wgtr = false; }
  else if (impl == UEGAN_IMPL_MFMA_GENERIC) { g_impl.impl = UEGAN_IMPL_MFMA; g_impl.patch = false; g_impl.heads = false; g_impl.wgtr = false; g_impl.stream = false; }
  return old;
}

extern "C" int uegan_selftest_mfma(void* scratch, uegan_stream_t stream) {
  UEGAN_CHECK_ARG(scratch, "null scratch");
  hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (float*)scratch);
  UEGAN_CHECK_LAUNCH();
  return UEGAN_OK;
}

extern "C" int uegan_profile_begin(int max_records) {
  UEGAN_CHECK_ARG(max_records > 0, "max_records must be positive");
  while ((int)g_prof_pool.size() < max_records) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
      set_error("hipEventCreate failed");
      return UEGAN_E_HIP;
    }
    g_prof_pool.push_back(std::make_pair(a, b));
  }
  g_prof_records.clear();
  g_prof_used = 0;
  g_prof_on = true;
  return UEGAN_OK;
}

extern "C" int uegan_profile_end(uegan_profile_entry* out, int max_entries, int* n_entries) {
  UEGAN_CHECK_ARG(out && n_entries && max_entries > 0, "bad profile_end args");
  g_prof_on = false;
  std::vector<int> keys;
  std::vector<double> ms, fl, by;
  std::vector<long long> cnt;
  for (const ProfRecord& r : g_prof_records) {
    if (hipEventSynchronize(r.stop) != hipSuccess) { set_error("hipEventSynchronize failed"); return UEGAN_E_HIP; }
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.start, r.stop) != hipSuccess) { set_error("hipEventElapsedTime failed"); return UEGAN_E_HIP; }
    size_t i = 0;
    while (i < keys.size() && keys[i] != r.kernel_id) ++i;
    if (i == keys.size()) { keys.push_back(r.kernel_id); ms.push_back(0); fl.push_back(0); by.push_back(0); cnt.push_back(0); }
    ms[i] += t; fl[i] += r.flops; by[i] += r.bytes; cnt[i] += 1;
  }
  int n = 0;
  for (size_t i = 0; i < keys.size() && n < max_entries; ++i, ++n) {
    prof_kernel_name(keys[i], out[n].name, sizeof(out[n].name));
    out[n].launches = cnt[i];
    out[n].total_ms = ms[i];
    out[n].total_flops = fl[i];
    out[n].total_bytes = by[i];
  }
  *n_entries = n;
  g_prof_records.clear();
  g_prof_used = 0;
  return UEGAN_OK;
}
