"""RoI pooling of a feature map under proposals on MI355X.

This module has NO counterpart in the reference, which stops at the proposals (its README: an RPN that "can be used for
Faster-RCNN").  It is the operator a second stage needs between the two values the reference does return -- the feature
extractor's output and the proposals -- as TensorFlow Faster R-CNN implementations write it:

    tf.image.crop_and_resize(feature_map, rois, box_indices, pooling_size)      method "bilinear", extrapolation_value 0

with ``box_indices`` fixed to "RoI r of image b samples image b" (the shape ``Proposer.propose`` returns).

    roi_pooling(feature_map, rois, pooling_size=(7, 7), valid=None)   -> rpn_roi_pool (+ rpn_roi_pool_backward under autograd)

beside it RoI Align, the pooling of Mask R-CNN and later Faster R-CNNs (each bin the average of s x s bilinear samples, pixel-centre
coordinates: every feature pixel under a box is read, whatever the size of the box):

    roi_align(feature_map, rois, pooling_size=(7, 7), sampling_ratio=2, extent=None, valid=None)
                                                                      -> rpn_roi_align (+ rpn_roi_align_backward under autograd)

and RoI max pooling, Fast R-CNN's RoIPool and the pooling of the VGG16 Faster R-CNN recipe (each bin the maximum over a quantised
block of feature pixels; what ImageNet's ``fc1`` / ``fc2`` were trained behind):

    roi_max_pooling(feature_map, rois, pooling_size=(7, 7), extent=None, valid=None, return_argmax=False)
                                                                      -> rpn_roi_max_pool (+ rpn_roi_max_pool_backward under autograd)

and, around them, what a second stage trains on and how its outputs become detections (the counterparts of the RPN's
``calculate_rpn_actual_outputs`` / ``reg_loss`` + ``cls_loss`` / ``decode_and_nms``; thresholds and sampling rule are this project's
choice):

    calculate_roi_targets(rois, gt_boxes, gt_labels, hyper_params, ...)   -> rpn_roi_targets
    sample_roi_targets(rois, gt_boxes, gt_labels, hyper_params, ...)      -> rpn_roi_sample_targets (the proposal-target layer:
                                                                             the gt boxes are candidates, only the sampled RoIs go on)
    roi_losses(cls_logits, reg_pred, roi_labels, roi_deltas)              -> rpn_roi_losses (gradients under autograd)
    roi_detections(rois, reg_pred, cls_logits, variances, ...)            -> rpn_roi_decode_scores + rpn_combined_nms (nms="hard") or
                                                                             rpn_soft_nms (nms="linear" / "gaussian")

Arguments may be torch tensors (any device; results come back as CUDA tensors) or numpy arrays (results come back as numpy).
Everything runs on the current torch HIP stream.  There is no CPU path: without a GPU ``roi_pooling`` raises ``RuntimeError``.
The arithmetic contract (float32, each operation rounded on its own, bit-exact) is stated in ``include/rpn_hip.h``.
"""
import numpy as np
import torch

from .. import _lib as L
from . import bbox_utils


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


# ---- RoI Align ------------------------------------------------------------------------------------------------------------------
def _sampling_ratio(sampling_ratio):
    s = int(sampling_ratio)
    if s != sampling_ratio or not 1 <= s <= 4:
        raise ValueError("sampling_ratio must be an integer in 1..4 (the adaptive form, <= 0, is not implemented), got %r"
                         % (sampling_ratio,))
    return s


def _extent(extent, H, W):
    """(Sy, Sx): the image's size in feature pixels; None -> (H, W)"""
    sy, sx = (float(H), float(W)) if extent is None else (float(v) for v in extent)
    if not (np.isfinite(sy) and np.isfinite(sx) and sy > 0.0 and sx > 0.0):
        raise ValueError("extent must be two finite positive numbers, got %r" % (extent,))
    return sy, sx


def _align_forward(x, rois, valid, ph, pw, s, sy, sx):
    B, H, W, C = (int(v) for v in x.shape)
    R = int(rois.shape[1])
    out = torch.empty((B, R, ph, pw, C), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_roi_align(L.ptr(x), B, H, W, C, L.ptr(rois), R, ph, pw, s, sy, sx, L.ptr(valid), L.ptr(out), L.stream_ptr())
    L.check(st, "roi_align")
    return out


def roi_align_backward(grad_out, rois, feature_shape, sampling_ratio=2, extent=None, valid=None):
    """Gradient of ``roi_align`` with respect to the feature map: ``grad_out`` (B, R, ph, pw, C) -> (B, H, W, C), the exact adjoint
    of the forward (``rpn_roi_align_backward``).  A gather without floating-point atomics: the same bits on every run, and image b's
    gradient depends on image b's RoIs alone.  There is no gradient with respect to the boxes."""
    s = _sampling_ratio(sampling_ratio)
    B, H, W, C = (int(v) for v in feature_shape)
    sy, sx = _extent(extent, H, W)
    g, was_np = L.to_device(grad_out)
    r, _ = L.to_device(rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    if g.dim() != 5 or int(g.shape[0]) != B or int(g.shape[4]) != C:
        raise ValueError("grad_out must be (%d, R, ph, pw, %d), got %s" % (B, C, tuple(g.shape)))
    if tuple(r.shape) != (B, int(g.shape[1]), 4):
        raise ValueError("rois must be (%d, %d, 4), got %s" % (B, int(g.shape[1]), tuple(r.shape)))
    if v is not None and tuple(v.shape) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, tuple(v.shape)))
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_roi_align_backward(L.ptr(g), L.ptr(r), L.ptr(v), B, H, W, C, int(g.shape[1]), int(g.shape[2]), int(g.shape[3]),
                                        s, sy, sx, L.ptr(dx), L.stream_ptr())
    L.check(st, "roi_align_backward")
    return L.from_device(dx, was_np)


class _RoIAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, valid, ph, pw, s, sy, sx):
        ctx.save_for_backward(rois, valid if valid is not None else torch.empty(0))
        ctx.has_valid = valid is not None
        ctx.feature_shape = tuple(x.shape)
        ctx.sampling = (s, (sy, sx))
        return _align_forward(x, rois, valid, ph, pw, s, sy, sx)

    @staticmethod
    def backward(ctx, grad_out):
        rois, valid = ctx.saved_tensors
        s, extent = ctx.sampling
        dx = roi_align_backward(grad_out.contiguous(), rois, ctx.feature_shape, s, extent, valid if ctx.has_valid else None)
        return dx, None, None, None, None, None, None, None


def roi_align(feature_map, rois, pooling_size=(7, 7), sampling_ratio=2, extent=None, valid=None):
    """RoI Align: feature_map (B, H, W, C) NHWC, rois (B, R, [y1, x1, y2, x2]) normalised -> (B, R, ph, pw, C), every bin the
    average of ``sampling_ratio`` x ``sampling_ratio`` bilinear samples spread over the bin, in pixel-centre coordinates
    (``rpn_roi_align``; Detectron2's ``aligned=True`` arithmetic, stated in ``include/rpn_hip.h``).

    ``sampling_ratio``: 1..4.  ``extent`` (Sy, Sx): the image's height and width in feature pixels, default (H, W); the
    stride-exact value of a stride-16 backbone on 500 pixels is (500 / 16, 500 / 16).  ``valid`` (B,) int32, optional: rows
    ``r >= valid[b]`` come back as zeros.

    A CUDA ``feature_map`` that requires grad gets its gradient through ``rpn_roi_align_backward``; ``rois`` and ``valid`` get none."""
    ph, pw = _pool_size(pooling_size)
    s = _sampling_ratio(sampling_ratio)
    shape = tuple(int(v) for v in (feature_map.shape if hasattr(feature_map, "shape") else np.shape(feature_map)))
    if len(shape) != 4:
        raise ValueError("feature_map must be (B, H, W, C) NHWC, got %s" % (shape,))
    sy, sx = _extent(extent, shape[1], shape[2])
    needs_grad = isinstance(feature_map, torch.Tensor) and feature_map.requires_grad and torch.is_grad_enabled()
    x, was_np = L.to_device(feature_map)
    r, _ = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    _check(x, r, v)
    if needs_grad:
        return _RoIAlign.apply(x, r, v, ph, pw, s, sy, sx)
    return L.from_device(_align_forward(x.detach(), r, v, ph, pw, s, sy, sx), was_np)


# ---- RoI max pooling ----------------------------------------------------------------------------------------------------------
def _max_extent(extent, H, W):
    """(Sy, Sx): the box scale in feature pixels; None -> (H - 1, W - 1), the box [0, 1] is exactly the pixels 0 .. H - 1 (an axis
    of one pixel takes 1: the scale must be > 0, and every box that reaches the axis then pools that pixel)"""
    return _extent((max(int(H) - 1, 1), max(int(W) - 1, 1)) if extent is None else extent, H, W)


def _max_forward(x, rois, valid, ph, pw, sy, sx, want_argmax):
    B, H, W, C = (int(v) for v in x.shape)
    R = int(rois.shape[1])
    out = torch.empty((B, R, ph, pw, C), dtype=torch.float32, device="cuda")
    argmax = torch.empty((B, R, ph, pw, C), dtype=torch.int32, device="cuda") if want_argmax else None
    st = L.lib().rpn_roi_max_pool(L.ptr(x), B, H, W, C, L.ptr(rois), R, ph, pw, sy, sx, L.ptr(valid), L.ptr(out), L.ptr(argmax),
                                  L.stream_ptr())
    L.check(st, "roi_max_pooling")
    return out, argmax


def roi_max_pooling_backward(grad_out, argmax, rois, feature_shape, extent=None, valid=None):
    """Gradient of ``roi_max_pooling`` with respect to the feature map: ``grad_out`` (B, R, ph, pw, C) and the forward's ``argmax``
    (same shape, int32) -> (B, H, W, C): every pixel gets the sum of the ``grad_out`` of the bins that chose it, added in float32
    in (r, i, j) order (``rpn_roi_max_pool_backward``).  A gather without floating-point atomics: the same bits on every run, and
    image b's gradient depends on image b alone.  ``rois``, ``extent`` and ``valid`` must be the forward's.  There is no gradient
    with respect to the boxes."""
    B, H, W, C = (int(v) for v in feature_shape)
    sy, sx = _max_extent(extent, H, W)
    gs, as_ = _shape(grad_out), _shape(argmax)
    if len(gs) != 5 or gs[0] != B or gs[4] != C:
        raise ValueError("grad_out must be (%d, R, ph, pw, %d), got %s" % (B, C, gs))
    if str(getattr(argmax, "dtype", None)).split(".")[-1] != "int32":
        raise ValueError("argmax must be int32, got %s" % (getattr(argmax, "dtype", type(argmax)),))
    if as_ != gs:
        raise ValueError("argmax must be %s int32 like grad_out, got %s" % (gs, as_))
    if _shape(rois) != (B, gs[1], 4):
        raise ValueError("rois must be (%d, %d, 4), got %s" % (B, gs[1], _shape(rois)))
    if valid is not None and _shape(valid) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, _shape(valid)))
    if C < 4 or C % 4:
        raise ValueError("the channel count must be a positive multiple of 4, got %d" % C)
    g, was_np = L.to_device(grad_out)
    a = L.to_device(argmax, dtype=torch.int32)[0]
    r, _ = L.to_device(rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    dx = torch.empty((B, H, W, C), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_roi_max_pool_backward(L.ptr(g), L.ptr(a), L.ptr(r), L.ptr(v), B, H, W, C, int(g.shape[1]), int(g.shape[2]),
                                           int(g.shape[3]), sy, sx, L.ptr(dx), L.stream_ptr())
    L.check(st, "roi_max_pooling_backward")
    return L.from_device(dx, was_np)


class _RoIMaxPooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rois, valid, ph, pw, sy, sx):
        out, argmax = _max_forward(x, rois, valid, ph, pw, sy, sx, True)
        ctx.save_for_backward(rois, valid if valid is not None else torch.empty(0), argmax)
        ctx.has_valid = valid is not None
        ctx.feature_shape = tuple(x.shape)
        ctx.extent = (sy, sx)
        ctx.mark_non_differentiable(argmax)
        return out, argmax

    @staticmethod
    def backward(ctx, grad_out, _grad_argmax):
        rois, valid, argmax = ctx.saved_tensors
        dx = roi_max_pooling_backward(grad_out.contiguous(), argmax, rois, ctx.feature_shape, ctx.extent,
                                      valid if ctx.has_valid else None)
        return dx, None, None, None, None, None, None


def roi_max_pooling(feature_map, rois, pooling_size=(7, 7), extent=None, valid=None, return_argmax=False):
    """RoI max pooling (Fast R-CNN's RoIPool): feature_map (B, H, W, C) NHWC, rois (B, R, [y1, x1, y2, x2]) normalised ->
    (B, R, ph, pw, C), every bin the maximum over a quantised block of feature pixels (``rpn_roi_max_pool``; Caffe's
    ``ROIPooling`` arithmetic, stated in ``include/rpn_hip.h``).  The first maximum of a bin wins a tie, a NaN in a bin reaches the
    output, an empty bin is 0.

    ``extent`` (Sy, Sx): the box scale in feature pixels, default (H - 1, W - 1) -- the box [0, 0, 1, 1] is exactly the whole map,
    as in ``roi_pooling``; the stride-exact value of a stride-16 backbone on 500 pixels is (500 / 16, 500 / 16).  ``valid`` (B,)
    int32, optional: rows ``r >= valid[b]`` come back as zeros.  ``return_argmax``: also return the int32 tensor of the pixel
    ``y * W + x`` every output was taken from (-1 for empty bins and dead rows), which ``roi_max_pooling_backward`` takes.

    A CUDA ``feature_map`` that requires grad gets its gradient through ``rpn_roi_max_pool_backward`` (the forward then keeps the
    argmax); otherwise no argmax is allocated unless asked for.  ``rois`` and ``valid`` get no gradient."""
    ph, pw = _pool_size(pooling_size)
    shape = tuple(int(v) for v in (feature_map.shape if hasattr(feature_map, "shape") else np.shape(feature_map)))
    if len(shape) != 4:
        raise ValueError("feature_map must be (B, H, W, C) NHWC, got %s" % (shape,))
    if shape[3] < 4 or shape[3] % 4:
        raise ValueError("the channel count must be a positive multiple of 4, got %d" % shape[3])
    sy, sx = _max_extent(extent, shape[1], shape[2])
    needs_grad = isinstance(feature_map, torch.Tensor) and feature_map.requires_grad and torch.is_grad_enabled()
    x, was_np = L.to_device(feature_map)
    r, _ = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    _check(x, r, v)
    if needs_grad:
        out, argmax = _RoIMaxPooling.apply(x, r, v, ph, pw, sy, sx)
    else:
        out, argmax = _max_forward(x.detach(), r, v, ph, pw, sy, sx, bool(return_argmax))
        out = L.from_device(out, was_np)
        argmax = L.from_device(argmax, was_np) if argmax is not None else None
    return (out, argmax) if return_argmax else out


# ---- second stage: targets, losses, detections ------------------------------------------------------------------------------
def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def calculate_roi_targets(rois, gt_boxes, gt_labels, hyper_params, valid=None, total_pos=None, total_neg=None, pos_iou=0.5,
                          neg_iou=(0.1, 0.5), random_pos=None, random_neg=None):
    """Training targets of the detection head, one launch on the device (``rpn_roi_targets``; contract in ``include/rpn_hip.h``).

    rois (B,R,4) normalised [y1,x1,y2,x2]; gt_boxes (B,G,4); gt_labels (B,G) int: a row is a gt box iff its label is >= 1 (0 is
    background, padding is -1); ``valid`` (B,) int32, optional: rows ``r >= valid[b]`` are padding (the count ``decode_and_nms``
    returns).  Returns (roi_deltas (B,R,4) float32, roi_labels (B,R) int32).

    A live row's gt is the valid one of highest IoU (the first on ties; none when every IoU is 0 or NaN).  Rows with IoU above
    ``pos_iou`` are positive candidates; ``total_pos`` of them are kept, by the priorities ``random_pos`` ((B,R) int32 >= 1, highest
    first, ties to the lower index).  Rows not kept as positives with ``neg_iou[0] <= IoU < neg_iou[1]`` are negative candidates;
    ``total_pos + total_neg`` minus the kept positives of them are kept by ``random_neg``.  Labels: the gt's label, 0 for a kept
    negative, -1 otherwise; deltas: ``get_deltas_from_bboxes(roi, gt) / variances`` for kept positives, +0.0 elsewhere.  The counts
    default to ``hyper_params["total_pos_bboxes"]`` / ``["total_neg_bboxes"]``; priorities that are not given come from torch's
    generator on the device (no readback).  The (B,R,G) IoU map is never materialised."""
    rs, gs, ls = _shape(rois), _shape(gt_boxes), _shape(gt_labels)
    if len(rs) != 3 or rs[2] != 4 or len(gs) != 3 or gs[2] != 4 or gs[0] != rs[0] or ls != gs[:2]:
        raise ValueError("expected rois (B,R,4), gt_boxes (B,G,4), gt_labels (B,G); got %s %s %s" % (rs, gs, ls))
    B, R, G = rs[0], rs[1], gs[1]
    if B < 1 or R < 1 or G < 1:
        raise ValueError("B, R and G must be >= 1 (gt_boxes needs at least one, possibly padded, row per image); got %d, %d, %d" % (B, R, G))
    if valid is not None and _shape(valid) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, _shape(valid)))
    for name, r in (("random_pos", random_pos), ("random_neg", random_neg)):
        if r is not None and _shape(r) != (B, R):
            raise ValueError("%s must be (%d, %d) int32, got %s" % (name, B, R, _shape(r)))
    total_pos = int(hyper_params["total_pos_bboxes"] if total_pos is None else total_pos)
    total_neg = int(hyper_params["total_neg_bboxes"] if total_neg is None else total_neg)
    neg_lo, neg_hi = (float(v) for v in neg_iou)
    if total_pos < 0 or total_neg < 0:
        raise ValueError("total_pos and total_neg must be >= 0, got %d and %d" % (total_pos, total_neg))
    if not (0.0 <= neg_lo <= neg_hi) or not float(pos_iou) >= 0.0:
        raise ValueError("thresholds need 0 <= neg_iou[0] <= neg_iou[1] and pos_iou >= 0, got %r and %r" % (neg_iou, pos_iou))

    def given(r, what):
        if not isinstance(r, torch.Tensor):
            r = torch.from_numpy(np.ascontiguousarray(np.asarray(r)))
        if r.numel() and int(r.min()) < 1:          # key 0 marks a non-candidate: a priority <= 0 would silently drop the row
            raise ValueError("%s: priorities must be >= 1" % what)
        return r.to(device="cuda", dtype=torch.int32).contiguous()

    r, was_np = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    g, _ = L.to_device(gt_boxes)
    lab, _ = L.to_device(gt_labels, dtype=torch.int32)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None

    def draw():
        return torch.randint(1, 2 ** 31 - 1, (B, R), dtype=torch.int32, device="cuda")

    rp = given(random_pos, "random_pos") if random_pos is not None else draw()
    rn = given(random_neg, "random_neg") if random_neg is not None else draw()
    deltas = torch.empty((B, R, 4), dtype=torch.float32, device="cuda")
    labels = torch.empty((B, R), dtype=torch.int32, device="cuda")
    lib = L.lib()
    ws_bytes = int(lib.rpn_roi_targets_workspace_bytes(B, R, G))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    _keep, vptr = L.host_floats(hyper_params["variances"])
    st = lib.rpn_roi_targets(L.ptr(r), L.ptr(v), L.ptr(g), L.ptr(lab), B, R, G, total_pos, total_neg, float(pos_iou), neg_lo, neg_hi,
                             vptr, L.ptr(rp), L.ptr(rn), L.ptr(deltas), L.ptr(labels), L.ptr(ws), ws_bytes, L.stream_ptr())
    L.check(st, "calculate_roi_targets")
    return L.from_device(deltas, was_np), L.from_device(labels, was_np)


def sample_roi_targets(rois, gt_boxes, gt_labels, hyper_params, valid=None, add_gt=True, total_pos=None, total_neg=None, pos_iou=0.5,
                       neg_iou=(0.1, 0.5), random_pos=None, random_neg=None, return_index=False):
    """The proposal-target layer, one launch on the device (``rpn_roi_sample_targets``; contract in ``include/rpn_hip.h``): the
    assignment of ``calculate_roi_targets`` over the proposals plus, with ``add_gt``, the gt boxes themselves, and only the sampled
    RoIs handed on, as a dense batch of ``S = total_pos + total_neg`` rows per image.

    Arguments as ``calculate_roi_targets``; the candidates of an image are its ``R`` RoIs followed by its ``G`` gt rows (``N = R + G``
    with ``add_gt``, else ``R``), and ``random_pos`` / ``random_neg`` are (B,N) int32 >= 1.  A gt row is a candidate iff its label is
    >= 1; it matches itself at IoU 1, so an image with a gt always has a positive.  Returns

        rois_s (B,S,4) float32, roi_deltas (B,S,4) float32, roi_labels (B,S) int32, counts (B,2) int32 [n_sampled, n_pos]

    and, with ``return_index=True``, the candidate index (B,S) int32 of every row (``>= R``: gt box ``index - R``).  Rows of an
    image: the kept positives in ascending candidate index, then the kept negatives in ascending candidate index, then padding (box
    and deltas +0.0, label -1, index -1).  ``counts[:, 0]`` is what the pools and ``roi_decode_scores`` take as ``valid``; the
    labels are what ``roi_losses`` takes.  An image without a gt box has counts [0, 0] under the default thresholds: the pools write
    zeros for it and it adds nothing to either loss.  No gradient flows to anything."""
    rs, gs, ls = _shape(rois), _shape(gt_boxes), _shape(gt_labels)
    if len(rs) != 3 or rs[2] != 4 or len(gs) != 3 or gs[2] != 4 or gs[0] != rs[0] or ls != gs[:2]:
        raise ValueError("expected rois (B,R,4), gt_boxes (B,G,4), gt_labels (B,G); got %s %s %s" % (rs, gs, ls))
    B, R, G = rs[0], rs[1], gs[1]
    if B < 1 or R < 1 or G < 1:
        raise ValueError("B, R and G must be >= 1 (gt_boxes needs at least one, possibly padded, row per image); got %d, %d, %d" % (B, R, G))
    if valid is not None and _shape(valid) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, _shape(valid)))
    add_gt = bool(add_gt)
    N = R + G if add_gt else R
    for name, r in (("random_pos", random_pos), ("random_neg", random_neg)):
        if r is not None and _shape(r) != (B, N):
            raise ValueError("%s must be (%d, %d) int32, one priority per candidate (%d RoIs%s), got %s"
                             % (name, B, N, R, " + %d gt rows" % G if add_gt else "", _shape(r)))
    total_pos = int(hyper_params["total_pos_bboxes"] if total_pos is None else total_pos)
    total_neg = int(hyper_params["total_neg_bboxes"] if total_neg is None else total_neg)
    neg_lo, neg_hi = (float(v) for v in neg_iou)
    if total_pos < 0 or total_neg < 0:
        raise ValueError("total_pos and total_neg must be >= 0, got %d and %d" % (total_pos, total_neg))
    S = total_pos + total_neg
    if S < 1:
        raise ValueError("total_pos + total_neg must be >= 1: the batch has that many rows per image")
    if not (0.0 <= neg_lo <= neg_hi) or not float(pos_iou) >= 0.0:
        raise ValueError("thresholds need 0 <= neg_iou[0] <= neg_iou[1] and pos_iou >= 0, got %r and %r" % (neg_iou, pos_iou))

    def given(r, what):
        if not isinstance(r, torch.Tensor):
            r = torch.from_numpy(np.ascontiguousarray(np.asarray(r)))
        if r.numel() and int(r.min()) < 1:          # key 0 marks a non-candidate: a priority <= 0 would silently drop the row
            raise ValueError("%s: priorities must be >= 1" % what)
        return r.to(device="cuda", dtype=torch.int32).contiguous()

    r, was_np = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    g, _ = L.to_device(gt_boxes.detach() if isinstance(gt_boxes, torch.Tensor) else gt_boxes)
    lab, _ = L.to_device(gt_labels, dtype=torch.int32)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None

    def draw():
        return torch.randint(1, 2 ** 31 - 1, (B, N), dtype=torch.int32, device="cuda")

    rp = given(random_pos, "random_pos") if random_pos is not None else draw()
    rn = given(random_neg, "random_neg") if random_neg is not None else draw()
    rois_s = torch.empty((B, S, 4), dtype=torch.float32, device="cuda")
    deltas = torch.empty((B, S, 4), dtype=torch.float32, device="cuda")
    labels = torch.empty((B, S), dtype=torch.int32, device="cuda")
    index = torch.empty((B, S), dtype=torch.int32, device="cuda")
    counts = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    lib = L.lib()
    ws_bytes = int(lib.rpn_roi_sample_targets_workspace_bytes(B, R, G, int(add_gt)))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    _keep, vptr = L.host_floats(hyper_params["variances"])
    st = lib.rpn_roi_sample_targets(L.ptr(r), L.ptr(v), L.ptr(g), L.ptr(lab), B, R, G, int(add_gt), total_pos, total_neg, float(pos_iou),
                                    neg_lo, neg_hi, vptr, L.ptr(rp), L.ptr(rn), S, L.ptr(rois_s), L.ptr(labels), L.ptr(deltas),
                                    L.ptr(index), L.ptr(counts), L.ptr(ws), ws_bytes, L.stream_ptr())
    L.check(st, "sample_roi_targets")
    out = (rois_s, deltas, labels, counts) + ((index,) if return_index else ())
    return tuple(L.from_device(t, was_np) for t in out)


def _check_losses(cs, ps, ls, ds):
    if len(cs) != 3 or len(ps) != 3 or cs[:2] != ps[:2] or ps[2] != 4 * cs[2] or ls != cs[:2] or ds != cs[:2] + (4,):
        raise ValueError("expected cls_logits (B,R,C), reg_pred (B,R,4C), roi_labels (B,R), roi_deltas (B,R,4); got %s %s %s %s"
                         % (cs, ps, ls, ds))
    if min(cs) < 1:
        raise ValueError("B, R and C must be >= 1, got %s" % (cs,))


def _losses(logits, reg, labels, deltas, with_grads):
    """-> (losses (2,) [reg, cls], grad_logits or None, grad_reg or None), all on the device"""
    B, R, C = (int(v) for v in logits.shape)
    losses = torch.empty((2,), dtype=torch.float32, device="cuda")
    g_logits = torch.empty_like(logits) if with_grads else None
    g_reg = torch.empty_like(reg) if with_grads else None
    lib = L.lib()
    ws_bytes = int(lib.rpn_roi_losses_workspace_bytes(B, R, C))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    st = lib.rpn_roi_losses(L.ptr(logits), L.ptr(reg), L.ptr(labels), L.ptr(deltas), B, R, C, L.ptr(losses), L.ptr(g_logits),
                            L.ptr(g_reg), L.ptr(ws), ws_bytes, L.stream_ptr())
    L.check(st, "roi_losses")
    return losses, g_logits, g_reg


class _RoILosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, reg, labels, deltas):
        losses, g_logits, g_reg = _losses(logits, reg, labels, deltas, True)
        ctx.save_for_backward(g_logits, g_reg)
        reg_loss, cls_loss = losses.clone().unbind()
        return reg_loss, cls_loss

    @staticmethod
    def backward(ctx, d_reg_loss, d_cls_loss):
        g_logits, g_reg = ctx.saved_tensors
        return (g_logits * d_cls_loss if ctx.needs_input_grad[0] else None,
                g_reg * d_reg_loss if ctx.needs_input_grad[1] else None, None, None)


def roi_losses(cls_logits, reg_pred, roi_labels, roi_deltas):
    """The detection head's losses on the device (``rpn_roi_losses``) -> (reg_loss, cls_loss), 0-d CUDA tensors for torch input, numpy
    float32 scalars for numpy input.

    cls_logits (B,R,C) logits; reg_pred (B,R,4C) class-specific boxes; roi_labels (B,R) int and roi_deltas (B,R,4) as
    ``calculate_roi_targets`` returns them.  Rows with a label outside [0, C) are ignored.  cls_loss is the softmax cross-entropy
    averaged over the kept rows, reg_loss the Huber (delta 1) sum of the labelled class's four coordinates over the positive rows
    divided by their count; either is 0, never NaN, when it has no row.  When a prediction requires grad the result is part of the
    torch graph: the forward pass computes both gradients, the backward pass scales them; labels and deltas get none."""
    _check_losses(_shape(cls_logits), _shape(reg_pred), _shape(roi_labels), _shape(roi_deltas))
    needs_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (cls_logits, reg_pred))
    logits, was_np = L.to_device(cls_logits)
    reg, _ = L.to_device(reg_pred)
    labels, _ = L.to_device(roi_labels.detach() if isinstance(roi_labels, torch.Tensor) else roi_labels, dtype=torch.int32)
    deltas, _ = L.to_device(roi_deltas.detach() if isinstance(roi_deltas, torch.Tensor) else roi_deltas)
    if needs_grad:
        return _RoILosses.apply(logits, reg, labels, deltas)
    losses = _losses(logits.detach(), reg.detach(), labels, deltas, False)[0]
    if was_np:
        host = losses.cpu().numpy()
        return host[0], host[1]
    return losses[0], losses[1]


def roi_decode_scores(rois, reg_pred, cls_logits, variances, valid=None):
    """Head outputs -> (boxes (B,R,C,4), scores (B,R,C)) in one launch (``rpn_roi_decode_scores``): boxes[b,r,c] =
    ``get_bboxes_from_deltas(rois, reg_pred[..., c, :], variances)``, not clipped; scores = softmax(cls_logits) with background
    (class 0) and rows ``r >= valid[b]`` exactly 0."""
    rs, ps, cs = _shape(rois), _shape(reg_pred), _shape(cls_logits)
    if len(rs) != 3 or rs[2] != 4 or len(cs) != 3 or cs[:2] != rs[:2] or ps != rs[:2] + (4 * cs[2],):
        raise ValueError("expected rois (B,R,4), reg_pred (B,R,4C), cls_logits (B,R,C); got %s %s %s" % (rs, ps, cs))
    B, R, C = cs
    if min(cs) < 1:
        raise ValueError("B, R and C must be >= 1, got %s" % (cs,))
    if valid is not None and _shape(valid) != (B,):
        raise ValueError("valid must be (%d,) int32, got %s" % (B, _shape(valid)))
    r, was_np = L.to_device(rois.detach() if isinstance(rois, torch.Tensor) else rois)
    reg, _ = L.to_device(reg_pred.detach() if isinstance(reg_pred, torch.Tensor) else reg_pred)
    logits, _ = L.to_device(cls_logits.detach() if isinstance(cls_logits, torch.Tensor) else cls_logits)
    v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
    boxes = torch.empty((B, R, C, 4), dtype=torch.float32, device="cuda")
    scores = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    _keep, vptr = L.host_floats(variances)
    st = L.lib().rpn_roi_decode_scores(L.ptr(r), L.ptr(v), L.ptr(reg), L.ptr(logits), vptr, B, R, C, L.ptr(boxes), L.ptr(scores),
                                       L.stream_ptr())
    L.check(st, "roi_decode_scores")
    return L.from_device(boxes, was_np), L.from_device(scores, was_np)


def roi_detections(rois, reg_pred, cls_logits, variances, valid=None, max_output_size_per_class=100, max_total_size=300,
                   iou_threshold=0.5, score_threshold=0.5, return_indices=False, nms="hard", sigma=0.5):
    """A trained head's outputs -> detections: ``roi_decode_scores`` then ``bbox_utils.non_max_suppression`` with class-specific
    boxes.  Returns (boxes (B,M,4) clipped to [0, 1], scores (B,M), classes (B,M), valid_detections (B,) int32), M =
    ``max_total_size`` (+ the selected RoI indices (B,M) int32 with ``return_indices=True``).  ``score_threshold`` must be above 0:
    background and padding rows carry a score of exactly 0 and must never be selected.

    ``nms``: ``"hard"`` (the default) deletes every box whose IoU with a selected one is above ``iou_threshold``; ``"linear"`` and
    ``"gaussian"`` run ``bbox_utils.soft_non_max_suppression`` with that method, ``iou_threshold`` and ``sigma`` (> 0; used by
    ``"gaussian"`` only) instead: overlapping boxes keep a decayed score, and the scores returned are the decayed ones."""
    if nms not in ("hard",) + tuple(bbox_utils.SOFT_NMS_METHODS):
        raise ValueError("nms must be 'hard', 'linear' or 'gaussian', got %r" % (nms,))
    if not float(score_threshold) > 0.0:
        raise ValueError("score_threshold must be > 0 (background and padding rows have score 0), got %r" % (score_threshold,))
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be > 0, got %r" % (sigma,))
    was_np = not isinstance(rois, torch.Tensor)
    if was_np:
        rois = torch.from_numpy(np.ascontiguousarray(np.asarray(rois, dtype=np.float32)))
    boxes, scores = roi_decode_scores(rois, reg_pred, cls_logits, variances, valid=valid)          # stay on the device
    if nms == "hard":
        res = bbox_utils.non_max_suppression(boxes, scores, max_output_size_per_class=int(max_output_size_per_class),
                                             max_total_size=int(max_total_size), iou_threshold=float(iou_threshold),
                                             score_threshold=float(score_threshold), return_indices=bool(return_indices))
    else:
        res = bbox_utils.soft_non_max_suppression(boxes, scores, int(max_output_size_per_class), int(max_total_size), method=nms,
                                                  sigma=float(sigma), iou_threshold=float(iou_threshold),
                                                  score_threshold=float(score_threshold), return_indices=bool(return_indices))
    return tuple(L.from_device(t, was_np) for t in res)
