// lmn_augment_u8: the training augmentations on the device.  The kernels, their arithmetic and the argument
// checks live in augment_common.h, shared with the OneOf entry (oneof.hip).
#include "augment_common.h"

int lmn_sizeof_aug_param(void) { return (int)sizeof(lmn_aug_param_t); }

int lmn_augment_u8(const uint8_t* images, const uint8_t* masks, const lmn_aug_param_t* params, const int32_t* src_hw,
                   lmn_aug_param_t* params_dev, int B, int Hs, int Ws, int H, int W, int channels, int mask_mode, const double* mean,
                   const double* std, uint8_t* scratch, uint64_t* gray_sum, float* out, int64_t* labels, lmn_stream_t stream) {
  AugGeom g;
  int rc = aug_check_args("augment_u8", images, masks, params, src_hw, params_dev, B, Hs, Ws, H, W, channels, mask_mode, mean, std,
                          scratch, gray_sum, out, labels, g);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = aug_launch_geom("augment_u8 (geometry)", images, masks, params, params_dev, B, channels, scratch, gray_sum, labels, g, st);
  if (rc || !images) return rc;
  const dim3 grid = aug_grid(H * W, B);
  unsigned long long* gs = (unsigned long long*)gray_sum;
  if (channels == 1)
    LMN_LAUNCH((augment_color_kernel<1, false>), grid, dim3(256), 0, st, scratch, params_dev, gs, out, (uint8_t*)nullptr, g);
  else
    LMN_LAUNCH((augment_color_kernel<3, false>), grid, dim3(256), 0, st, scratch, params_dev, gs, out, (uint8_t*)nullptr, g);
  return lmn_launch_status("augment_u8 (colour)");
}
