// The first step of every entry that scores or post-processes a prediction (metrics.hip, surface.hip, postprocess.hip): one class
// id per pixel, from fp32 logits [B, C, H, W] (arg-max over C) or from an integer label map, and the same range test for the target.
// A value outside [0, C) is no class; what stands for "no class" (-1, 255, 0) is the caller's choice and part of its behaviour.
// Device helpers only, no kernels.
#pragma once
#include "common.h"

namespace {

// arg-max of one pixel's C logits lg[c * hw]: first maximum wins, as torch.argmax
__device__ __forceinline__ int pred_argmax(const float* lg, int C, int64_t hw) {
  int best = 0;
  float bv = lg[0];
#pragma unroll 8
  for (int c = 1; c < C; ++c) {
    const float v = lg[c * hw];
    if (v > bv) { bv = v; best = c; }
  }
  return best;
}

// the same with the class count known at compile time, fully unrolled
template <int C>
__device__ __forceinline__ int pred_argmax(const float* lg, int64_t hw) {
  int best = 0;
  float bv = lg[0];
#pragma unroll
  for (int c = 1; c < C; ++c) {
    const float v = lg[c * hw];
    if (v > bv) { bv = v; best = c; }
  }
  return best;
}

// does a label of any integer width (a uint8 prediction, an int64 target) name a class, 0 <= v < C?  (compared in v's own promoted
// type: a uint8 costs one 32-bit compare)
template <typename T>
__device__ __forceinline__ bool pred_in_range(T v, int C) {
  return v >= 0 && v < C;
}
// ... and its class id: (int)v, or `none` outside [0, C)
template <typename T>
__device__ __forceinline__ int pred_class(T v, int C, int none) {
  return pred_in_range(v, C) ? (int)v : none;
}

}  // namespace
