// roi_kernels.h -- RoI pooling / RoI Align / RoI max pooling launchers shared by the stand-alone entry and the model handle (roi_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rpn {

// how the feature map is stored: float32 NHWC, or SPLIT16 (hi / lo 16-bit halves, split_format.hip) in bfloat16 / float16
enum RoiSource { ROI_SRC_F32 = 0, ROI_SRC_SPLIT_BF16 = 1, ROI_SRC_SPLIT_F16 = 2 };

// validates the geometry (RPN_ERR_INVALID, message prefixed with `who`), then launches; x is (B,H,W,C) in the form `src` names
int roi_pool_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                     int pw, const int *d_valid, float *d_out, hipStream_t s);

// the same for RoI Align; also validates sampling_ratio (1..4) and the extent (finite, > 0)
int roi_align_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                      int pw, int sampling_ratio, float extent_y, float extent_x, const int *d_valid, float *d_out, hipStream_t s);

// the same for RoI max pooling; validates the extent (finite, > 0); d_argmax (B,R,ph,pw,C) int32 may be null (not written then)
int roi_max_pool_forward(const char *who, const void *d_x, int src, int B, int H, int W, int C, const float *d_rois, int R, int ph,
                         int pw, float extent_y, float extent_x, const int *d_valid, float *d_out, int32_t *d_argmax, hipStream_t s);

}  // namespace rpn
