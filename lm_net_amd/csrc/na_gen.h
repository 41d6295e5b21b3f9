// Neighborhood attention for any head_dim 1..32 (na_gen.hip): the launchers lmn_na_fwd / lmn_na_bwd (na.hip) call for the head
// dims the channel-quad kernels of na.hip do not take (every hd outside {1, 2, 4, 8, 16}, or every hd with LMN_NA_GENERAL=1).
// Arguments as lmn_na_fwd / lmn_na_bwd, K > 0.  Not exported (library-internal linkage).
#pragma once
#include "common.h"

#define LMN_NA_ANY_MAX_HD 32
__attribute__((visibility("hidden"))) int lmn_na_any_fwd(const void* qkv, const float* rpb, void* out, int B, int H, int W, int heads,
                                                         int hd, int K, float scale, int act_dtype, hipStream_t st);
__attribute__((visibility("hidden"))) int lmn_na_any_bwd(const void* qkv, const float* rpb, const void* dout, void* dqkv, float* drpb,
                                                         float* stat, int B, int H, int W, int heads, int hd, int K, float scale,
                                                         int act_dtype, hipStream_t st);
// LMN_NA_GENERAL=1: the kernels of na_gen.hip for every head_dim (A/B runs against the channel-quad kernels)
__attribute__((visibility("hidden"))) bool lmn_na_force_general();
