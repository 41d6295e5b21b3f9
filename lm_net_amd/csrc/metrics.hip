// The counting entries of the evaluation side (lm_net_amd.metrics.ConfusionMeter, ImageStatsMeter): a prediction -- fp32 logits
// (arg-max, pred_common.h) or a uint8 label map -- against int64 labels, counted with integer or exactly representable float sums.
//   lmn_confusion         counts[t*C + p] of argmax(logits): confusion_kernel<C> for C in {2, 3, 4}, confusion_gen_kernel above
//   lmn_confusion_labels  the same for a label-map prediction: confusion_labels_kernel
//   lmn_image_stats       tp / fp / fn / tn per image and class (include/lmnet_loss.h): image_stats_kernel
// A label outside [0, C) is counted nowhere.  The zero fill and the capped grid are those of the losses (loss_common.h).
#include "loss_common.h"
#include "pred_common.h"
#include "../../include/lmnet_loss.h"

namespace {

constexpr int MT_MAXC = 64;

// Confusion matrix of argmax(logits) against the labels: counts[t*C + p] += 1.  The float cells are exact while
// they stay below 2^24: the entries refuse B * HW >= 2^24 pixels per call, and the host (ConfusionMeter) splits larger inputs, hands
// every call zeroed cells and accumulates in double.
template <int C>
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        int B, int64_t hw, float* __restrict__ counts) {
  __shared__ float sc[C * C];
  for (int i = threadIdx.x; i < C * C; i += 256) sc[i] = 0.f;
  __syncthreads();
  int cnt[C * C];
#pragma unroll
  for (int k = 0; k < C * C; ++k) cnt[k] = 0;
  const int64_t total = (int64_t)B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const float* lg = logits + b * C * hw;
    const int best = pred_argmax<C>(lg + i, hw);
    const int y = pred_class(target[idx], C, -1);      // (tested as int64: a label such as -2^40 has the low word of class 0; no cell
                                                       //  k equals -C + best, so a label outside [0, C) is counted nowhere)
#pragma unroll
    for (int k = 0; k < C * C; ++k) cnt[k] += (k == y * C + best) ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < C * C; ++k) {
    int v = cnt[k];
#pragma unroll
    for (int m = 1; m <= 32; m <<= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sc[k], (float)v);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += 256)
    if (sc[i] != 0.f) atomicAdd(counts + i, sc[i]);
}

// General class count (5 <= C <= 64): the block's C x C histogram lives in LDS as int32 (16 KB at C = 64) instead of C^2 registers per
// thread; labels outside [0, C) are dropped (Evaluator._generate_matrix).
__global__ __launch_bounds__(256) void confusion_gen_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                            int B, int C, int64_t hw, float* __restrict__ counts) {
  extern __shared__ int s_hist[];                     // [C * C]
  for (int i = threadIdx.x; i < C * C; i += 256) s_hist[i] = 0;
  __syncthreads();
  const int64_t total = (int64_t)B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const float* lg = logits + b * C * hw + i;
    const int best = pred_argmax(lg, C, hw);
    const int64_t y = target[idx];
    if (pred_in_range(y, C)) atomicAdd(&s_hist[(int)y * C + best], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += 256)
    if (s_hist[i]) atomicAdd(counts + i, (float)s_hist[i]);
}

// Confusion matrix of a label-map prediction (lmn_confusion with the arg-max already taken): int32 histogram per block in LDS.
__global__ __launch_bounds__(256) void confusion_labels_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ target, int C,
                                                               int64_t total, float* __restrict__ counts) {
  extern __shared__ int s_hist[];                     // [C * C]
  for (int i = threadIdx.x; i < C * C; i += 256) s_hist[i] = 0;
  __syncthreads();
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int p = pred[idx];
    const int64_t y = target[idx];
    const bool pok = pred_in_range(p, C), yok = pred_in_range(y, C);   // (both loads are issued before either test)
    if (pok && yok) atomicAdd(&s_hist[(int)y * C + p], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += 256)
    if (s_hist[i]) atomicAdd(counts + i, (float)s_hist[i]);
}

// tp / fp / fn / tn per image and class.  blockIdx.y is the image, blockIdx.x strides over ITS pixels only, so a block's LDS
// counters (predicted, labelled and correct pixels per class, and the valid pixels) belong to one image whatever HW is.  Small C
// counts by wave ballots (a handful of lanes would otherwise serialise on two or three LDS words); larger C by LDS atomics.
__global__ __launch_bounds__(256) void image_stats_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ pred_labels,
                                                          const int64_t* __restrict__ target, int C, int64_t hw,
                                                          unsigned long long* __restrict__ stats) {
  __shared__ int s_cnt[3 * MT_MAXC + 1];              // [0..C) tp, [C..2C) predicted, [2C..3C) labelled, [3C] valid
  for (int i = threadIdx.x; i <= 3 * C; i += 256) s_cnt[i] = 0;
  __syncthreads();
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t* tg = target + (int64_t)b * hw;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < hw; base += (int64_t)gridDim.x * 256) {   // (uniform trip count per wave)
    const int64_t i = base + threadIdx.x;
    int y = -1, best = -1;
    if (i < hw) {
      const int64_t yl = tg[i];
      if (pred_in_range(yl, C)) {                     // (a void pixel's prediction is never read)
        y = (int)yl;
        if (logits) best = pred_argmax(logits + (int64_t)b * C * hw + i, C, hw);
        else best = pred_class(pred_labels[(int64_t)b * hw + i], C, -1);
      }
    }
    if (C <= 8) {
      const int nv = __popcll(__ballot(y >= 0));
      if (nv == 0) continue;
      if (lane == 0) atomicAdd(&s_cnt[3 * C], nv);
      for (int c = 0; c < C; ++c) {
        const int np = __popcll(__ballot(y >= 0 && best == c)), nl = __popcll(__ballot(y == c)), nt = __popcll(__ballot(y == c && best == c));
        if (lane == 0) {
          if (nt) atomicAdd(&s_cnt[c], nt);
          if (np) atomicAdd(&s_cnt[C + c], np);
          if (nl) atomicAdd(&s_cnt[2 * C + c], nl);
        }
      }
    } else if (y >= 0) {
      atomicAdd(&s_cnt[3 * C], 1);
      atomicAdd(&s_cnt[2 * C + y], 1);
      if (best >= 0) atomicAdd(&s_cnt[C + best], 1);
      if (best == y) atomicAdd(&s_cnt[y], 1);
    }
  }
  __syncthreads();
  const int nvalid = s_cnt[3 * C];
  if (nvalid == 0) return;
  for (int c = threadIdx.x; c < C; c += 256) {
    const int tp = s_cnt[c], np = s_cnt[C + c], nl = s_cnt[2 * C + c];
    unsigned long long* o = stats + ((int64_t)b * C + c) * 4;
    if (tp) atomicAdd(o + 0, (unsigned long long)tp);
    if (np - tp) atomicAdd(o + 1, (unsigned long long)(np - tp));
    if (nl - tp) atomicAdd(o + 2, (unsigned long long)(nl - tp));
    atomicAdd(o + 3, (unsigned long long)(nvalid - np - nl + tp));   // >= 0: pixels predicted or labelled c are among the valid
  }
}

}  // namespace

extern "C" {

int lmn_confusion(const float* logits, const int64_t* target, int B, int C, int64_t HW, float* counts, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && counts, "confusion: null pointer");
  LMN_REQUIRE(B > 0 && HW > 0 && C >= 2 && C <= MT_MAXC, "confusion: C=%d not in [2, 64]", C);
  LMN_REQUIRE((int64_t)B * HW < (1LL << 24), "confusion: B*HW=%lld pixels, float counts are exact below 2^24 = 16777216 pixels per call (split the call)",
              (long long)((int64_t)B * HW));
  hipStream_t st = (hipStream_t)stream;
  const int grid = loss_grid((int64_t)B * HW, 512);
  switch (C) {
    case 2: LMN_LAUNCH((confusion_kernel<2>), dim3(grid), dim3(256), 0, st, logits, target, B, HW, counts); break;
    case 3: LMN_LAUNCH((confusion_kernel<3>), dim3(grid), dim3(256), 0, st, logits, target, B, HW, counts); break;
    case 4: LMN_LAUNCH((confusion_kernel<4>), dim3(grid), dim3(256), 0, st, logits, target, B, HW, counts); break;
    default: LMN_LAUNCH(confusion_gen_kernel, dim3(grid), dim3(256), (size_t)C * C * sizeof(int), st, logits, target, B, C, HW, counts); break;
  }
  return lmn_launch_status("confusion");
}

int lmn_confusion_labels(const uint8_t* pred_labels, const int64_t* target, int B, int C, int64_t HW, float* counts, lmn_stream_t stream) {
  LMN_REQUIRE(pred_labels && target && counts, "confusion_labels: null pointer");
  LMN_REQUIRE(B > 0 && HW > 0 && C >= 2 && C <= MT_MAXC, "confusion_labels: C=%d not in [2, 64]", C);
  LMN_REQUIRE((int64_t)B * HW < (1LL << 24), "confusion_labels: B*HW=%lld pixels, float counts are exact below 2^24 = 16777216 pixels per call (split the call)",
              (long long)((int64_t)B * HW));
  const int64_t total = (int64_t)B * HW;
  LMN_LAUNCH(confusion_labels_kernel, dim3(loss_grid(total, 1024)), dim3(256), (size_t)C * C * sizeof(int), (hipStream_t)stream, pred_labels,
             target, C, total, counts);
  return lmn_launch_status("confusion_labels");
}

int lmn_image_stats(const float* logits, const uint8_t* pred_labels, const int64_t* target, int B, int C, int64_t HW, int has_ignore,
                    int64_t ignore_index, int64_t* stats, lmn_stream_t stream) {
  LMN_REQUIRE(target && stats, "image_stats: null pointer");
  LMN_REQUIRE((logits != nullptr) != (pred_labels != nullptr), "image_stats: exactly one of logits and pred_labels must be given");
  LMN_REQUIRE(C >= 2 && C <= MT_MAXC, "image_stats: C=%d not in [2, %d]", C, MT_MAXC);
  LMN_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW < (1LL << 31), "image_stats: B=%d, HW=%lld (need B <= 65535, HW < 2^31)", B, (long long)HW);
  LMN_REQUIRE(!has_ignore || ignore_index < 0 || ignore_index >= C, "image_stats: ignore_index=%lld inside [0, %d)", (long long)ignore_index, C);
  hipStream_t st = (hipStream_t)stream;
  const int64_t words = (int64_t)B * C * 8;
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(words, 64)), dim3(256), 0, st, (uint32_t*)stats, words);
  const int per_image = 512 / B > 0 ? 512 / B : 1;          // (few blocks per image: every block ends in 4C same-address atomics)
  LMN_LAUNCH(image_stats_kernel, dim3(loss_grid(HW, per_image), B), dim3(256), 0, st, logits, pred_labels, target, C, HW,
             (unsigned long long*)stats);
  return lmn_launch_status("image_stats");
}

}  // extern "C"
