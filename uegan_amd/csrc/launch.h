// Host-side launch vocabulary of the HBM-bound kernels (norm.hip, loss.hip, elementwise.hip, act_bwd.hip, optim_sn.hip, pack_weights.hip):
// storage-type dispatch and block counts.  Include after common.h; nothing here is device code.
#pragma once
#include "common.h"

namespace uegan {

// elements per 16-byte chunk of the storage type (DT<T>::EPC, for a run-time dtype)
static inline int epc_of(int dtype) { return dtype == UEGAN_BF16 ? 8 : 4; }

// clamp(ceil(work / per_block), 1, cap): the block count of a grid-stride launch.  The fixed-order reductions make results a function of
// this count, and the workspaces are sized by the caps, so the boundaries below are what tests/test_loss_optim_kernels.py aims at.
constexpr int blocks_for(size_t work, int per_block, int cap) {
  const size_t b = (work + (size_t)per_block - 1) / (size_t)per_block;
  return b < 1 ? 1 : (b < (size_t)cap ? (int)b : cap);
}
static_assert(blocks_for(0, 1024, 64) == 1 && blocks_for(1, 1024, 64) == 1, "an empty or tiny launch is one block");
static_assert(blocks_for(65536, 1024, 64) == 64 && blocks_for(65537, 1024, 64) == 64, "cap 64 is reached exactly at 64 * 1024 and holds past it");
static_assert(blocks_for(131072, 1024, 128) == 128 && blocks_for(131073, 1024, 128) == 128, "cap 128 is reached exactly at 128 * 1024 and holds past it");
static_assert(blocks_for((size_t)8192 * 256 + 1, 256, 8192) == 8192, "cap 8192 holds past 8192 * 256");
static_assert(blocks_for(1025, 1024, 64) == 2 && blocks_for(64512, 1024, 64) == 63, "ceil below the cap");

// one thread per work item, 256 per block
static inline int grid_for(size_t n, int cap = 8192) { return blocks_for(n, 256, cap); }
// threads of a block that owns one row of n work items: whole waves, at most 256
static inline int row_threads(size_t n) { return n >= 256 ? 256 : (int)((n + 63) / 64) * 64; }

}  // namespace uegan

// Run the statement(s) with T bound to the storage type of `dtype`; any other dtype is refused before anything is launched.
#define UEGAN_DISPATCH_T(dtype, ...)                                                       \
  do {                                                                                     \
    if ((dtype) == UEGAN_F32) { using T = float; __VA_ARGS__; }                            \
    else if ((dtype) == UEGAN_BF16) { using T = uegan::bf16_t; __VA_ARGS__; }              \
    else { uegan::set_error("bad dtype %d", (int)(dtype)); return UEGAN_E_INVALID; }       \
  } while (0)
// ... with T and V bound: V = one 16-byte chunk per thread when `vec_ok`, else 1
#define UEGAN_DISPATCH_TV(dtype, vec_ok, ...)                                                                                                      \
  do {                                                                                                                                             \
    if ((dtype) == UEGAN_F32) { using T = float; if (vec_ok) { constexpr int V = 4; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } }    \
    else if ((dtype) == UEGAN_BF16) { using T = uegan::bf16_t; if (vec_ok) { constexpr int V = 8; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } \
    else { uegan::set_error("bad dtype %d", (int)(dtype)); return UEGAN_E_INVALID; }                                                               \
  } while (0)
// ... with a run-time flag bound as the compile-time constant NAME
#define UEGAN_DISPATCH_BOOL(flag, NAME, ...)                                                                           \
  do { if (flag) { constexpr bool NAME = true; __VA_ARGS__; } else { constexpr bool NAME = false; __VA_ARGS__; } } while (0)
