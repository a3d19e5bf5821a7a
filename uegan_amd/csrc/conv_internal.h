// Internal (non-ABI) entry points shared between the convolution translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/uegan_hip.h"

namespace uegan {
// narrow-head VALU kernels (heads.hip): stride-1 KxK reflect-padded convs with <= 4 real output channels
bool heads_applicable(const uegan_conv_desc* d);
int heads_fwd(const uegan_conv_desc* d, const void* x, const void* w_ohwi, const float* bias, const float* scale, void* y, hipStream_t s);
bool heads_dgrad_applicable(const uegan_conv_desc* d);
int heads_dgrad(const uegan_conv_desc* d, const void* dz, const void* w_ihwo, const float* scale, void* dx, hipStream_t s);
int heads_wgrad_blocks(const uegan_conv_desc* d);
int heads_wgrad(const uegan_conv_desc* d, const void* x, const void* dz, float* ws, hipStream_t s);
// norm.hip: the per-(image, channel) constants of a fidelity-loss tap's backward inside its scratch (uegan_percep_tap_fwd's tmp)
void percep_tap_consts(int dtype, const float* tmp, int B, int HW, int C, const float** st, const float** tot);
// norm.hip: the first two launches of uegan_instnorm_bwd -- {sum dy, sum dy*y} per (image, channel) at tot[(b*C + c)*2 + {0,1}], inside tmp
// (fp32 [uegan_reduce_workspace_floats])
int instnorm_bwd_sums(int dtype, const void* dy, const void* y, float* tmp, int B, int HW, int C, hipStream_t s, const float** tot);
// wgrad.hip: wgrad_reduce_kernel over nsplit partials [N][ktot] (pstride floats apart) of a 1x1 layer's weight gradient, no bias, no scale
int wgrad_reduce_1x1(const float* ws, float* dw, int nsplit, int N, int C, int Cin_w, int Cin_row, size_t pstride, int acc, hipStream_t s);
}  // namespace uegan
