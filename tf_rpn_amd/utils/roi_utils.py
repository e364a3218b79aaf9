"""RoI pooling of a feature map under proposals on MI355X.

This module has NO counterpart in the reference, which stops at the proposals (its README: an RPN that "can be used for
Faster-RCNN").  It is the operator a second stage needs between the two values the reference does return -- the feature
extractor's output and the proposals -- as TensorFlow Faster R-CNN implementations write it:

    tf.image.crop_and_resize(feature_map, rois, box_indices, pooling_size)      method "bilinear", extrapolation_value 0

with ``box_indices`` fixed to "RoI r of image b samples image b" (the shape ``Proposer.propose`` returns).

    roi_pooling(feature_map, rois, pooling_size=(7, 7), valid=None)   -> rpn_roi_pool (+ rpn_roi_pool_backward under autograd)

Arguments may be torch tensors (any device; results come back as CUDA tensors) or numpy arrays (results come back as numpy).
Everything runs on the current torch HIP stream.  There is no CPU path: without a GPU ``roi_pooling`` raises ``RuntimeError``.
The arithmetic contract (float32, each operation rounded on its own, bit-exact) is stated in ``include/rpn_hip.h``.
"""
import torch

from .. import _lib as L


def _pool_size(pooling_size):
    ph, pw = (int(v) for v in pooling_size)
    if ph < 1 or pw < 1:
        raise ValueError("pooling_size must be two positive integers, got %r" % (pooling_size,))
    return ph, pw


def _check(x, rois, valid):
    if x.dim() != 4:
        raise ValueError("feature_map must be (B, H, W, C) NHWC, got %s" % (tuple(x.shape),))
    B = int(x.shape[0])
    if rois.dim() != 3 or int(rois.shape[0]) != B or int(rois.shape[2]) != 4:
        raise ValueError("rois must be (%d, R, 4) normalised [y1, x1, y2, x2], got %s" % (B, tuple(rois.shape)))
    if valid is not None and tuple(valid.shape) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, tuple(valid.shape)))


def _forward(x, rois, valid, ph, pw):
    B, H, W, C = (int(v) for v in x.shape)
    R = int(rois.shape[1])
    out = torch.empty((B, R, ph, pw, C), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_roi_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, ph, pw, L.ptr(valid), L.ptr(out), L.stream_ptr())
    L.check(st, "roi_pooling")
    return out


def roi_pooling_backward(grad_out, rois, feature_shape, valid=None):
    """Gradient of ``roi_pooling`` with respect to the feature map: ``grad_out`` (B, R, ph, pw, C) -> (B, H, W, C), the exact
    adjoint of the forward.  A gather without floating-point atomics: the same bits on every run, and image b's gradient depends on
    image b's RoIs alone.  There is no gradient with respect to the boxes (Faster R-CNN stops it there)."""
    g, was_np = L.to_device(grad_out)
    r, _ = L.to_device(rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    B, H, W, C = (int(s) for s in feature_shape)
    if g.dim() != 5 or int(g.shape[0]) != B or int(g.shape[4]) != C:
        raise ValueError("grad_out must be (%d, R, ph, pw, %d), got %s" % (B, C, tuple(g.shape)))
    if tuple(r.shape) != (B, int(g.shape[1]), 4):
        raise ValueError("rois must be (%d, %d, 4), got %s" % (B, int(g.shape[1]), tuple(r.shape)))
    if v is not None and tuple(v.shape) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, tuple(v.shape)))
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_roi_pool_backward(L.ptr(g), L.ptr(r), L.ptr(v), B, H, W, C, int(g.shape[1]), int(g.shape[2]), int(g.shape[3]),
                                       L.ptr(dx), L.stream_ptr())
    L.check(st, "roi_pooling_backward")
    return L.from_device(dx, was_np)


class _RoIPooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, valid, ph, pw):
        ctx.save_for_backward(rois, valid if valid is not None else torch.empty(0))
        ctx.has_valid = valid is not None
        ctx.feature_shape = tuple(x.shape)
        return _forward(x, rois, valid, ph, pw)

    @staticmethod
    def backward(ctx, grad_out):
        rois, valid = ctx.saved_tensors
        dx = roi_pooling_backward(grad_out.contiguous(), rois, ctx.feature_shape, valid if ctx.has_valid else None)
        return dx, None, None, None, None


def roi_pooling(feature_map, rois, pooling_size=(7, 7), valid=None):
    """feature_map (B, H, W, C) NHWC, rois (B, R, [y1, x1, y2, x2]) normalised -> (B, R, ph, pw, C).

    ``valid`` (B,) int32, optional: rows ``r >= valid[b]`` come back as zeros -- pass the count ``Proposer.propose`` /
    ``non_max_suppression`` returns, whose padding boxes are all-zero and would otherwise all sample pixel (0, 0).

    A CUDA ``feature_map`` that requires grad gets its gradient through ``rpn_roi_pool_backward`` (``torch.autograd``); ``rois``
    and ``valid`` get none."""
    ph, pw = _pool_size(pooling_size)
    needs_grad = isinstance(feature_map, torch.Tensor) and feature_map.requires_grad and torch.is_grad_enabled()
    x, was_np = L.to_device(feature_map)
    r, _ = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    _check(x, r, v)
    if needs_grad:
        return _RoIPooling.apply(x, r, v, ph, pw)
    return L.from_device(_forward(x.detach(), r, v, ph, pw), was_np)
