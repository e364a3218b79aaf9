"""Box math of the RPN proposal path on MI355X -- same call signatures as the reference's
``utils/bbox_utils.py``, each bound to one C-ABI entry point of ``librpn_hip.so``:

    generate_anchors(hyper_params)                  -> rpn_generate_anchors   (bbox_utils.py:23-46)
    get_bboxes_from_deltas(anchors, deltas)         -> rpn_decode             (bbox_utils.py:72-96)
    get_deltas_from_bboxes(bboxes, gt_boxes)        -> rpn_encode             (bbox_utils.py:98-124)
    generate_iou_map(bboxes, gt_boxes)              -> rpn_iou_map            (bbox_utils.py:126-150)
    normalize_bboxes / denormalize_bboxes(...)      -> rpn_scale_boxes        (bbox_utils.py:152-182)
    non_max_suppression(pred_bboxes, pred_labels, **kwargs) -> rpn_combined_nms (bbox_utils.py:48-70)

and, without a counterpart in the reference, Soft-NMS (Bodla et al. 2017) with the same input and output shapes:

    soft_non_max_suppression(pred_bboxes, pred_labels, max_output_size_per_class, max_total_size, ...) -> rpn_soft_nms

Arguments may be torch tensors (any device; results come back as CUDA tensors) or numpy
arrays (results come back as numpy).  Everything runs on the current torch HIP stream.
There is no CPU path: without a GPU these functions raise ``RuntimeError``.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L


def generate_anchors(hyper_params, as_numpy=False):
    """All anchors for the feature map, (F*F*K, [y1, x1, y2, x2]) normalised to [0, 1]."""
    ratios = np.ascontiguousarray(hyper_params["anchor_ratios"], dtype=np.float64)
    scales = np.ascontiguousarray(hyper_params["anchor_scales"], dtype=np.float64)
    fm = int(hyper_params["feature_map_shape"])
    L.require_gpu()
    out = torch.empty((fm * fm * len(ratios) * len(scales), 4), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_generate_anchors(float(hyper_params["img_size"]), fm,
                                      ratios.ctypes.data_as(L.c_double_p), len(ratios),
                                      scales.ctypes.data_as(L.c_double_p), len(scales), L.ptr(out), L.stream_ptr())
    L.check(st, "generate_anchors")
    return L.from_device(out, as_numpy)


def get_bboxes_from_deltas(anchors, deltas, variances=None):
    """Decode (B, A, [dy, dx, dh, dw]) against anchors (A,4) or (B,A,4) -> (B, A, [y1, x1, y2, x2]).

    ``variances`` (4 floats) optionally fuses the caller's ``deltas *= variances``
    (predictor.py:55) into the same kernel; the default keeps the reference's two-step contract.
    """
    d, was_np = L.to_device(deltas)
    a, _ = L.to_device(anchors)
    if d.dim() != 3 or d.shape[-1] != 4:
        raise ValueError("deltas must be (batch, total_bboxes, 4), got %s" % (tuple(d.shape),))
    B, A = int(d.shape[0]), int(d.shape[1])
    if a.dim() == 2:
        batched = 0
        ok = tuple(a.shape) == (A, 4)
    else:
        batched = 1
        ok = tuple(a.shape) == (B, A, 4)
    if not ok:
        raise ValueError("anchors %s do not match deltas %s" % (tuple(a.shape), tuple(d.shape)))
    out = torch.empty_like(d)
    vptr = None
    if variances is not None:
        _keep, vptr = L.host_floats(variances)
    st = L.lib().rpn_decode(L.ptr(a), batched, L.ptr(d), vptr, B, A, L.ptr(out), L.stream_ptr())
    L.check(st, "get_bboxes_from_deltas")
    return L.from_device(out, was_np)


def get_deltas_from_bboxes(bboxes, gt_boxes):
    """Encode gt_boxes (B,A,4) against bboxes (A,4) or (B,A,4) -> (B, A, [dy, dx, dh, dw])."""
    g, was_np = L.to_device(gt_boxes)
    b, _ = L.to_device(bboxes)
    if g.dim() != 3 or g.shape[-1] != 4:
        raise ValueError("gt_boxes must be (batch, total_bboxes, 4), got %s" % (tuple(g.shape),))
    B, A = int(g.shape[0]), int(g.shape[1])
    batched = 0 if b.dim() == 2 else 1
    if tuple(b.shape) != ((A, 4) if batched == 0 else (B, A, 4)):
        raise ValueError("bboxes %s do not match gt_boxes %s" % (tuple(b.shape), tuple(g.shape)))
    out = torch.empty_like(g)
    st = L.lib().rpn_encode(L.ptr(b), batched, L.ptr(g), B, A, L.ptr(out), L.stream_ptr())
    L.check(st, "get_deltas_from_bboxes")
    return L.from_device(out, was_np)


def generate_iou_map(bboxes, gt_boxes):
    """Pairwise IoU of bboxes (A,4) or (B,A,4) with gt_boxes (B,G,4) -> (B, A, G)."""
    g, was_np = L.to_device(gt_boxes)
    b, _ = L.to_device(bboxes)
    if g.dim() != 3 or g.shape[-1] != 4:
        raise ValueError("gt_boxes must be (batch, total_gt_boxes, 4), got %s" % (tuple(g.shape),))
    B, G = int(g.shape[0]), int(g.shape[1])
    batched = 0 if b.dim() == 2 else 1
    A = int(b.shape[-2])
    if b.shape[-1] != 4 or (batched and int(b.shape[0]) != B):
        raise ValueError("bboxes %s do not match gt_boxes %s" % (tuple(b.shape), tuple(g.shape)))
    out = torch.empty((B, A, G), dtype=torch.float32, device="cuda")
    st = L.lib().rpn_iou_map(L.ptr(b), batched, A, L.ptr(g), B, G, L.ptr(out), L.stream_ptr())
    L.check(st, "generate_iou_map")
    return L.from_device(out, was_np)


def _scale_boxes(bboxes, height, width, denormalize):
    b, was_np = L.to_device(bboxes)
    if b.shape[-1] != 4:
        raise ValueError("bboxes must end in 4 coordinates, got %s" % (tuple(b.shape),))
    out = torch.empty_like(b)
    st = L.lib().rpn_scale_boxes(L.ptr(b), b.numel() // 4, float(height), float(width), int(denormalize), L.ptr(out),
                                 L.stream_ptr())
    L.check(st, "denormalize_bboxes" if denormalize else "normalize_bboxes")
    return L.from_device(out, was_np)


def normalize_bboxes(bboxes, height, width):
    """(…, [y1, x1, y2, x2]) in pixels -> normalised [0, 1] (utils/bbox_utils.py:152-166)."""
    return _scale_boxes(bboxes, height, width, False)


def denormalize_bboxes(bboxes, height, width):
    """Normalised boxes -> pixels, rounded half-to-even like tf.round (utils/bbox_utils.py:168-182)."""
    return _scale_boxes(bboxes, height, width, True)


_NMS_KWARGS = ("max_output_size_per_class", "max_total_size", "iou_threshold", "score_threshold",
               "pad_per_class", "clip_boxes", "name")


def non_max_suppression(pred_bboxes, pred_labels, **kwargs):
    """Per-image, per-class greedy NMS with the keyword arguments of
    ``tf.image.combined_non_max_suppression`` (the reference passes **kwargs straight through).

    pred_bboxes (B, N, q, 4) with q == 1 or q == total_labels; pred_labels (B, N, total_labels).
    Returns (nmsed_boxes (B,M,4), nmsed_scores (B,M), nmsed_classes (B,M), valid_detections (B,) int32);
    entries past valid_detections[i] are zero padding.  ``return_indices=True`` (extension, not in
    TF) appends the selected box indices (B,M) int32, -1 padded.
    """
    return_indices = bool(kwargs.pop("return_indices", False))
    unknown = [k for k in kwargs if k not in _NMS_KWARGS]
    if unknown:
        raise TypeError("non_max_suppression() got unexpected keyword argument(s) %s" % unknown)
    if "max_output_size_per_class" not in kwargs or "max_total_size" not in kwargs:
        raise TypeError("non_max_suppression() needs max_output_size_per_class and max_total_size")
    max_per_class = int(kwargs["max_output_size_per_class"])
    max_total = int(kwargs["max_total_size"])
    iou_thr = float(kwargs.get("iou_threshold", 0.5))
    score_thr = float(kwargs.get("score_threshold", float("-inf")))
    pad_per_class = bool(kwargs.get("pad_per_class", False))
    clip_boxes = bool(kwargs.get("clip_boxes", True))

    boxes, was_np = L.to_device(pred_bboxes)
    scores, _ = L.to_device(pred_labels)
    if boxes.dim() != 4 or boxes.shape[-1] != 4 or scores.dim() != 3:
        raise ValueError("expected pred_bboxes (B,N,q,4) and pred_labels (B,N,C), got %s and %s"
                         % (tuple(boxes.shape), tuple(scores.shape)))
    B, N, q = int(boxes.shape[0]), int(boxes.shape[1]), int(boxes.shape[2])
    C = int(scores.shape[2])
    if tuple(scores.shape[:2]) != (B, N) or q not in (1, C):
        raise ValueError("pred_bboxes %s and pred_labels %s are inconsistent" % (tuple(boxes.shape), tuple(scores.shape)))
    if max_per_class < 0 or max_total < 0:
        raise ValueError("max_output_size_per_class and max_total_size must be >= 0")
    M = min(max_total, max_per_class * C) if pad_per_class else max_total

    out_boxes = torch.zeros((B, M, 4), dtype=torch.float32, device="cuda")
    out_scores = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    out_classes = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    out_idx = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    out_valid = torch.zeros((B,), dtype=torch.int32, device="cuda")
    if B > 0 and M > 0:
        lib = L.lib()
        ws_bytes = int(lib.rpn_nms_workspace_bytes(B, N, C, max_per_class, M))
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device="cuda")
        st = lib.rpn_combined_nms(L.ptr(boxes), L.ptr(scores), B, N, q, C, max_per_class, M, iou_thr, score_thr,
                                  int(clip_boxes), L.ptr(out_boxes), L.ptr(out_scores), L.ptr(out_classes),
                                  L.ptr(out_idx), L.ptr(out_valid), L.ptr(ws), ws_bytes, L.stream_ptr())
        L.check(st, "non_max_suppression")
    res = (out_boxes, out_scores, out_classes, out_valid)
    if return_indices:
        res = res + (out_idx,)
    return tuple(L.from_device(t, was_np) for t in res)


SOFT_NMS_METHODS = {"linear": 0, "gaussian": 1}


def soft_non_max_suppression(pred_bboxes, pred_labels, max_output_size_per_class, max_total_size, method="gaussian", sigma=0.5,
                             iou_threshold=0.5, score_threshold=0.001, clip_boxes=True, return_indices=False):
    """Per-image, per-class Soft-NMS (``rpn_soft_nms``; contract in ``include/rpn_hip.h``): the box of highest score is taken, the
    scores of the boxes that overlap it are decayed, and so on until ``max_output_size_per_class`` boxes are taken or no score is
    above ``score_threshold``.

    ``method="linear"``: a score is multiplied by ``1 - iou`` when ``iou > iou_threshold``.  ``method="gaussian"``: a box with
    ``iou > iou_threshold`` is removed (TensorFlow's hard cut; ``iou_threshold=1.0`` is the paper's pure Gaussian), any other
    overlapping box has its score multiplied by ``exp(-iou^2 / sigma)``.  TensorFlow's ``soft_nms_sigma = s`` is ``sigma = 2 s``
    here; ``sigma=float("inf")`` is hard NMS at ``iou_threshold``, bit for bit.

    pred_bboxes (B, N, q, 4) with q == 1 or q == total_labels; pred_labels (B, N, total_labels); N <= 4096 and
    ``total_labels * min(max_output_size_per_class, N) <= 16384``.  ``score_threshold`` must be >= 0.  Returns what
    ``non_max_suppression`` returns -- (boxes (B,M,4), scores (B,M), classes (B,M), valid_detections (B,) int32), M =
    ``max_total_size``, zero padded, + the selected rows (B,M) int32, -1 padded, with ``return_indices=True`` -- with the DECAYED
    scores, ordered by them.  Runs on the current stream and does not synchronise."""
    if method not in SOFT_NMS_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(SOFT_NMS_METHODS), method))
    max_per_class, M = int(max_output_size_per_class), int(max_total_size)
    sigma, iou_thr, score_thr = float(sigma), float(iou_threshold), float(score_threshold)
    if not sigma > 0.0:
        raise ValueError("sigma must be > 0, got %r" % (sigma,))
    if not iou_thr >= 0.0:
        raise ValueError("iou_threshold must be >= 0, got %r" % (iou_thr,))
    if not score_thr >= 0.0:
        raise ValueError("score_threshold must be >= 0 (a decay would raise a negative score), got %r" % (score_thr,))
    if max_per_class < 0 or M < 0:
        raise ValueError("max_output_size_per_class and max_total_size must be >= 0")
    bs = tuple(int(v) for v in (pred_bboxes.shape if hasattr(pred_bboxes, "shape") else np.shape(pred_bboxes)))
    ss = tuple(int(v) for v in (pred_labels.shape if hasattr(pred_labels, "shape") else np.shape(pred_labels)))
    if len(bs) != 4 or bs[-1] != 4 or len(ss) != 3:
        raise ValueError("expected pred_bboxes (B,N,q,4) and pred_labels (B,N,C), got %s and %s" % (bs, ss))
    B, N, q = bs[:3]
    C = ss[2]
    if ss[:2] != (B, N) or q not in (1, C) or C < 1:
        raise ValueError("pred_bboxes %s and pred_labels %s are inconsistent" % (bs, ss))
    lib = L.lib()
    if B > 0 and M > 0:       # the library's limits, before anything is copied or launched
        st = lib.rpn_soft_nms(None, None, 0, N, q, C, max_per_class, M, SOFT_NMS_METHODS[method], iou_thr, sigma, score_thr,
                              int(bool(clip_boxes)), None, None, None, None, None, None, 0, None)
        L.check(st, "soft_non_max_suppression")
    boxes, was_np = L.to_device(pred_bboxes)
    scores, _ = L.to_device(pred_labels)

    out_boxes = torch.zeros((B, M, 4), dtype=torch.float32, device="cuda")
    out_scores = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    out_classes = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    out_idx = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    out_valid = torch.zeros((B,), dtype=torch.int32, device="cuda")
    if B > 0 and M > 0:
        ws_bytes = int(lib.rpn_soft_nms_workspace_bytes(B, N, C, max_per_class, M))
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device="cuda")
        st = lib.rpn_soft_nms(L.ptr(boxes), L.ptr(scores), B, N, q, C, max_per_class, M, SOFT_NMS_METHODS[method], iou_thr, sigma,
                              score_thr, int(bool(clip_boxes)), L.ptr(out_boxes), L.ptr(out_scores), L.ptr(out_classes),
                              L.ptr(out_idx), L.ptr(out_valid), L.ptr(ws), ws_bytes, L.stream_ptr())
        L.check(st, "soft_non_max_suppression")
    res = (out_boxes, out_scores, out_classes, out_valid)
    if return_indices:
        res = res + (out_idx,)
    return tuple(L.from_device(t, was_np) for t in res)


def check_proposal_filter(pre_nms_topn, min_size):
    """Validate the proposal layer's two filter arguments (no device involved) -> (topn int, 0 = no cut; use_min_size 0 / 1;
    min_h; min_w).  ``pre_nms_topn``: None or a positive integer.  ``min_size``: None, a float or (min_h, min_w), >= 0, in the
    normalised units of the boxes."""
    topn = 0
    if pre_nms_topn is not None:
        if isinstance(pre_nms_topn, bool) or not isinstance(pre_nms_topn, (int, np.integer)) or int(pre_nms_topn) < 1:
            raise ValueError("pre_nms_topn must be None or a positive integer, got %r" % (pre_nms_topn,))
        topn = min(int(pre_nms_topn), 2 ** 31 - 1)
    if min_size is None:
        return topn, 0, 0.0, 0.0
    try:
        hw = [float(v) for v in min_size] if isinstance(min_size, (tuple, list, np.ndarray)) else [float(min_size)] * 2
    except (TypeError, ValueError):
        raise ValueError("min_size must be None, a number or (min_h, min_w), got %r" % (min_size,))
    if len(hw) != 2 or not all(v >= 0.0 for v in hw):                  # (NaN >= 0 is False)
        raise ValueError("min_size must be None, a number >= 0 or (min_h, min_w) >= 0, got %r" % (min_size,))
    return topn, 1, hw[0], hw[1]


def _shape_of(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _check_proposal_shapes(anchors, deltas, scores):
    a, d, s = _shape_of(anchors), _shape_of(deltas), _shape_of(scores)
    if len(d) != 3 or d[-1] != 4 or a != (d[1], 4) or s != d[:2]:
        raise ValueError("inconsistent shapes: anchors %s deltas %s scores %s" % (a, d, s))
    return d[0], d[1]


def _launch_proposal_filter(a, d, s, vptr, B, A, filt, score_threshold, clip_boxes, masked, kept):
    topn, use_min, min_h, min_w = filt
    ws_bytes = int(L.lib().rpn_proposal_filter_workspace_bytes(B, A))          # 0 today: NULL is passed and nothing is allocated
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda") if ws_bytes else None
    st = L.lib().rpn_proposal_filter(L.ptr(a) if use_min else None, L.ptr(d) if use_min else None, vptr, L.ptr(s), B, A, topn,
                                     use_min, min_h, min_w, float(score_threshold), int(bool(clip_boxes)), L.ptr(masked),
                                     L.ptr(kept), L.ptr(ws), ws_bytes, L.stream_ptr())
    L.check(st, "filter_proposals")


def filter_proposals(anchors, deltas, scores, variances, pre_nms_topn=None, min_size=None, score_threshold=float("-inf"),
                     clip_boxes=True):
    """The proposal layer's filters in front of the NMS (``rpn_proposal_filter``; contract in ``include/rpn_hip.h``): raw head
    deltas (B,A,4) and objectness (B,A) -> (masked_scores (B,A), kept (B,) int32).

    An anchor is a candidate iff its score is > ``score_threshold`` and, with ``min_size``, its decoded box (clipped to [0, 1] iff
    ``clip_boxes``) is at least ``min_h`` high and ``min_w`` wide.  ``min_size`` is a float or ``(min_h, min_w)`` in the NORMALISED
    units of the boxes (16 px at 500 x 500 is ``16 / 500``); ``None`` switches the size test off.  With ``pre_nms_topn`` only that
    many best-scored candidates are kept (ties to the lower index, exactly); ``None`` keeps them all.  ``masked_scores`` holds the
    score where kept and -inf elsewhere, so ``decode_and_nms`` on it with the same threshold is the whole proposal layer
    (``decode_and_nms(..., pre_nms_topn=, min_size=)`` does both).  Runs on the current stream and does not synchronise."""
    filt = check_proposal_filter(pre_nms_topn, min_size)
    B, A = _check_proposal_shapes(anchors, deltas, scores)
    d, was_np = L.to_device(deltas)
    s, _ = L.to_device(scores)
    a, _ = L.to_device(anchors)
    masked = torch.empty((B, A), dtype=torch.float32, device="cuda")
    kept = torch.zeros((B,), dtype=torch.int32, device="cuda")
    vptr = None
    if variances is not None:
        _keep, vptr = L.host_floats(variances)
    if B > 0:
        _launch_proposal_filter(a, d, s, vptr, B, A, filt, score_threshold, clip_boxes, masked, kept)
    return L.from_device(masked, was_np), L.from_device(kept, was_np)


def decode_and_nms(anchors, deltas, scores, variances, max_total_size, iou_threshold=0.5,
                   score_threshold=float("-inf"), clip_boxes=True, pre_nms_topn=None, min_size=None):
    """predictor.py:52-56 followed by NMS, in one kernel: raw head deltas (B,A,4) and objectness
    (B,A) -> (boxes (B,M,4), scores (B,M), indices (B,M) int32, valid (B,) int32).  Decoded boxes
    are never written to HBM (-> rpn_decode_nms).

    ``pre_nms_topn`` / ``min_size`` (see ``filter_proposals``; both ``None`` by default: the calls above and nothing else) put the
    proposal layer's filters in front: ``rpn_proposal_filter`` masks the scores, then the same ``rpn_decode_nms`` runs on the masked
    scores, both on the current stream without a synchronisation or a host copy."""
    filt = None
    if pre_nms_topn is not None or min_size is not None:
        filt = check_proposal_filter(pre_nms_topn, min_size)
        _check_proposal_shapes(anchors, deltas, scores)
    d, was_np = L.to_device(deltas)
    s, _ = L.to_device(scores)
    a, _ = L.to_device(anchors)
    B, A = int(d.shape[0]), int(d.shape[1])
    if tuple(a.shape) != (A, 4) or tuple(s.shape) != (B, A) or d.shape[-1] != 4:
        raise ValueError("inconsistent shapes: anchors %s deltas %s scores %s"
                         % (tuple(a.shape), tuple(d.shape), tuple(s.shape)))
    M = int(max_total_size)
    out_boxes = torch.zeros((B, M, 4), dtype=torch.float32, device="cuda")
    out_scores = torch.zeros((B, M), dtype=torch.float32, device="cuda")
    out_idx = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    out_valid = torch.zeros((B,), dtype=torch.int32, device="cuda")
    vptr = None
    if variances is not None:
        _keep, vptr = L.host_floats(variances)
    if B > 0 and M > 0:
        if filt is not None:
            masked = torch.empty((B, A), dtype=torch.float32, device="cuda")
            _launch_proposal_filter(a, d, s, vptr, B, A, filt, score_threshold, clip_boxes, masked, None)
            s = masked
        ws_bytes = int(L.lib().rpn_nms_workspace_bytes(B, A, 1, M, M))
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device="cuda")
        st = L.lib().rpn_decode_nms(L.ptr(a), L.ptr(d), vptr, L.ptr(s), B, A, M, float(iou_threshold),
                                    float(score_threshold), int(bool(clip_boxes)), L.ptr(out_boxes),
                                    L.ptr(out_scores), L.ptr(out_idx), L.ptr(out_valid), L.ptr(ws), ws_bytes,
                                    L.stream_ptr())
        L.check(st, "decode_and_nms")
    return tuple(L.from_device(t, was_np) for t in (out_boxes, out_scores, out_idx, out_valid))
