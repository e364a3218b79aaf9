// train_head.h -- host-side interface of the RPN losses, the head's backward kernels, the 3x3 weight gradient at the head's shape and
// Adam (train_kernels.hip; internal to librpn_hip.so); the helpers the training kernel files share are in train_common.h (a256 in
// rpn_common.h).  Every kernel is float32 (float64 sums inside the losses), writes each output
// once and uses no floating-point atomics: every sum has a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rpn {

// ---- rpn_reg_loss / rpn_cls_loss over the n = B A anchors: reg (n, 4), cls (n) -----------------------------------------------------
// out: [reg, cls] or, with_total, [reg + cls, reg, cls]; graw_reg / graw_cls (or null): the UNSCALED gradients with respect to the
// predictions.  ws: losses_ws_bytes(n) bytes of device scratch; the two gradient scales {1 / max(1, n_pos), 1 / n_valid or 0} land
// at its end, where losses_scale(ws, n) points.
size_t losses_ws_bytes(long long n);
float *losses_scale(void *ws, long long n);
hipError_t launch_losses(const float *reg_true, const float *reg_pred, const float *cls_true, const float *cls_pred, long long n,
                         float *graw_reg, float *graw_cls, float *out, int with_total, void *ws, hipStream_t s);

// ---- out (C) = the column sums of x (rows, C): chunks of 64 rows in order, then the chunks in order --------------------------------
// part: colsum_ws_floats(rows, C) floats of device scratch
size_t colsum_ws_floats(long long rows, int C);
hipError_t launch_colsum(const float *x, long long rows, int C, float *part, float *out, hipStream_t s);

// ---- the 3x3 stride-1 'same' weight-gradient GEMM on the float32 MFMA (conv3x3_wgrad_f32_kernel: the one kernel behind launch_wgrad
// and train_backbone.h's launch_wgrad_wide), x (B,H,W,Cin), dy (B,H,W,Cout), Cin % 4 == 0, Cout % 4 == 0 --------------------------------
// writes `leaves` slabs of (9 Cin + ones) x Cout floats to part and nothing else: slab l = the gradient over the pixels
// [l P / leaves, (l + 1) P / leaves), row (3 r + s) Cin + ci; with `ones`, row 9 Cin = the sum of dy over the same pixels (db).
// The caller adds the slabs in its own fixed order.  No error is read here: the caller's hipGetLastError covers the launch.
void launch_wgrad_slabs(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, int leaves, bool ones, float *part,
                        hipStream_t s);

// ---- dw (3,3,Cin,Cout) HWIO = the weight gradient of a 3x3 stride-1 'same' conv, x (B,H,W,Cin), dy (B,H,W,Cout) -----------------------
// four fixed ranges of pixels added as (l0 + l1) + (l2 + l3).  Cin % 4 == 0, Cout % 4 == 0.  part: wgrad_ws_floats(Cin, Cout) floats.
size_t wgrad_ws_floats(int Cin, int Cout);
hipError_t launch_wgrad(const float *x, const float *dy, int B, int H, int W, int Cin, int Cout, float *part, float *dw, hipStream_t s);

// ---- the fused 1x1 head (512 -> nc = 5 K columns: rpn_reg, then rpn_cls) backward over P pixels ------------------------------------
// dz (P, nc) = [graw_reg * scale[0] | graw_cls * scale[1] * cls (1 - cls)]; dw_head (513, nc) = S^T dz (rows 0 .. 511: the kernel's
// gradient) and sum dz (row 512: the bias's); dS (P, 512) = (dz w_head^T) * [S > 0].  part: head_backward_ws_floats(P, nc) floats.
// *supported = false and nothing after dz launched when nc is no instantiated width (5, 10 .. 60).
size_t head_backward_ws_floats(long long P, int nc);
hipError_t launch_head_backward(const float *graw_reg, const float *graw_cls, const float *cls, const float *scale, const float *S,
                                const float *w_head, long long P, int K, float *dz, float *part, float *dw_head, float *dS,
                                bool *supported, hipStream_t s);

// ---- Adam (ApplyAdam) over one flat buffer of n floats; t: the number of this step, from 1 ---------------------------------------
hipError_t launch_adam(float *w, const float *g, float *m, float *v, long long n, long long t, float lr, float b1, float b2, float eps,
                       hipStream_t s);

// ---- the configurable update (optim_kernels.hip): SGD momentum, L2 weight decay, clipping by the global norm ---------------------
// Per element, float32, every operation rounded on its own (c: the clip scale, 1 without a clip norm; wd: the decay):
//   g1 = g c;  g2 = g1 + wd w on a decayed element, g1 elsewhere
//   SGD (Keras / TF 2.0 ApplyKerasMomentum, restated as recalled): a = mu a - lr g2;  w += a  (nesterov: w += mu a - lr g2, the new a);
//     a lives in m, v is not touched
//   Adam: launch_adam's arithmetic on g2
// So the clip acts on the loss gradient alone (what get_gradient returns) and the decay joins after it: Caffe's order and
// py-faster-rcnn's.  A non-finite squared norm gives c = NaN and the step propagates it into every weight, as tf.clip_by_global_norm does.
struct OptimConfig {
    int kind = 0;                                // RPN_OPT_ADAM / RPN_OPT_SGD
    float momentum = 0.0f, weight_decay = 0.0f, clipnorm = 0.0f;
    int nesterov = 0;
    // what both handles launch today: launch_adam, no norm pass
    bool is_default() const { return kind == 0 && weight_decay == 0.0f && clipnorm == 0.0f; }
};
// RPN_ERR_INVALID with a message for a bad value, before any device work
int optim_check_config(const char *who, int kind, float momentum, int nesterov, float weight_decay, float clipnorm);

// the update's own device memory: S (double) | c (float) | the norm's partials | the decayed ranges; allocated at the first step that
// needs it.  ranges: sorted, disjoint [begin, end) pairs of element indices into the flat buffer.
struct OptimDevice {
    char *buf = nullptr;
    int n_ranges = 0;
    bool stepped = false;                        // a step has written S and c under the current configuration
};
void optim_free(OptimDevice *d);

// S = sum g[i]^2 in float64 (a float32 square is exact there): per-workgroup partials in a fixed order, then one finishing workgroup;
// the grid, and so the order, depends on n alone.  Writes S and c = clipnorm > 0 && sqrt(S) > clipnorm ? (float)(clipnorm / sqrt(S)) : 1
// (NaN when S is not finite).  g 16-byte aligned; part: grad_norm_ws_bytes(n) bytes.
size_t grad_norm_ws_bytes(long long n);
hipError_t launch_grad_sq_norm(const float *g, long long n, float clipnorm, double *part, double *S, float *scale, hipStream_t s);

// one update of the flat buffer under cfg: the norm pass when a clip norm is set, then one launch.  t: the number of this step, from 1.
// Never called with cfg.is_default(): that step is launch_adam.
int optim_step(const char *who, const OptimConfig &cfg, OptimDevice *d, const long long *ranges, int n_ranges, float *w, const float *g,
               float *m, float *v, long long n, long long t, float lr, float b1, float b2, float eps, hipStream_t s);
// the pre-clip global norm and the scale of the last step (synchronises s)
int optim_grad_norm(const char *who, const OptimConfig &cfg, const OptimDevice &d, double *norm, float *scale, hipStream_t s);

}  // namespace rpn
