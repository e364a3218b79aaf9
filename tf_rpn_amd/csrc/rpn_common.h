// rpn_common.h -- shared host-side helpers of librpn_hip.so (error state, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../../include/rpn_hip.h"
#include "rpn_knobs.h"

namespace rpn {

// thread-local message returned by rpn_last_error()
char *error_buffer();
constexpr int kErrorBufferLen = 512;

inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), kErrorBufferLen, fmt, ap);
    va_end(ap);
    return code;
}

// true when a HIP device is usable; fills the error buffer otherwise (no CPU fallback exists)
bool have_device();

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// workspace sections start on 256-byte boundaries
inline size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace rpn

#define RPN_REQUIRE(cond, ...)                                         \
    do {                                                               \
        if (!(cond)) return rpn::fail(RPN_ERR_INVALID, __VA_ARGS__);   \
    } while (0)

#define RPN_REQUIRE_DEVICE()                                           \
    do {                                                               \
        if (!rpn::have_device()) return RPN_ERR_NO_DEVICE;             \
    } while (0)

#define RPN_HIP_CHECK(expr)                                                                      \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return rpn::fail(RPN_ERR_NO_DEVICE, "%s failed: %s (%s:%d)", #expr,                  \
                             hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

#define RPN_CHECK_LAUNCH() RPN_HIP_CHECK(hipGetLastError())

// ---- the model handle as the head trainer sees it (model.hip) ----------------------------------------------------------------
namespace rpn {
// channels of the backbone features, feature-map side F, anchors per position K, the handle's largest batch
void model_train_dims(const rpn_model *m, int *cin, int *F, int *K, int *max_batch);
// the handle's backbone (RPN_BACKBONE_*) and input side
void model_train_backbone(const rpn_model *m, int *backbone, int *img_size);
// the ops up to the backbone features on stream s, then the features as NHWC float32 (B, F, F, cin) into d_feat
int model_features(rpn_model *m, const float *d_imgs, int B, float *d_feat, hipStream_t s);
// the same up to the tensor `name` (an op's output, e.g. "block_6_project"), and that tensor's shape per image
int model_features_at(rpn_model *m, const char *name, const float *d_imgs, int B, float *d_out, hipStream_t s);
int model_tensor_shape(const rpn_model *m, const char *name, int *H, int *W, int *C);
bool model_has_layer(const rpn_model *m, const char *name);
}  // namespace rpn
