"""Scoring the detector on MI355X: PASCAL VOC average precision of the detections and the recall of the proposals, accumulated on
the device (``rpn_evaluator_*``; the contract is written out in ``include/rpn_hip.h``).

This module has NO counterpart in the reference, whose training script is wired for the VOC protocol (``voc/2007``, difficult
objects dropped under ``evaluate=True``) but stops at ``val_loss``.  The rules are VOCdevkit's ``VOCevaldet``:

    ev = DetectionEvaluator(total_labels=21, max_images=4952, max_detections=300, iou_threshold=0.5,
                            top_k=(10, 100, 300), recall_iou=(0.5, 0.7))
    for imgs, gt_boxes, gt_labels, gt_difficult in val_feed:
        rois, _, valid, pooled = prop.propose_features(imgs)
        ev.update_proposals(rois, valid, gt_boxes, gt_labels, gt_difficult)
        boxes, scores, classes, n = head.detect(rois, pooled, hp["variances"], valid=valid)
        flags = ev.update(boxes, scores, classes, n, gt_boxes, gt_labels, gt_difficult)
    r = ev.result()                                  # the one synchronisation

Where the devkit is loose the choice is this project's: a detection matches with ``IoU >= iou_threshold`` (``>=``, as the devkit);
of two gts with the same IoU the first is the match; of two detections with the same score the lower row (then the lower slot, in
the ranking) comes first; the 11-point AP compares ``10 * tp >= k * npos`` in integers.

``CocoEvaluator`` is a second evaluator beside it with COCO's rules (AP over ten IoU thresholds and four object sizes, AR at 1 / 10
/ 100 detections; ``rpn_coco_evaluator_*``); ``evaluate`` feeds either, or several at once.

``update`` and ``update_proposals`` enqueue on the current torch stream and return: nothing is copied to the host and nothing
synchronises.  Arguments may be torch tensors (any device) or numpy arrays.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from .. import _lib as L

MAX_CUTOFFS = 8
MAX_GT = 2048
MAX_DETECTIONS = 4096


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


class DetectionEvaluator(object):
    """A device-resident accumulator of detection records and proposal hits; it owns all its device memory from its creation
    (``memory_bytes()``: 24 bytes per detection row of ``max_images * max_detections``, plus the counters)."""

    def __init__(self, total_labels, max_images, max_detections=300, iou_threshold=0.5, top_k=(10, 100, 300), recall_iou=(0.5, 0.7)):
        self.total_labels, self.max_images, self.max_detections = int(total_labels), int(max_images), int(max_detections)
        self.iou_threshold = float(iou_threshold)
        self.top_k = tuple(int(k) for k in top_k)
        self.recall_iou = tuple(float(t) for t in recall_iou)
        if len(self.top_k) > MAX_CUTOFFS or len(self.recall_iou) > MAX_CUTOFFS:
            raise ValueError("at most %d cut-offs and %d thresholds, got %d and %d" % (MAX_CUTOFFS, MAX_CUTOFFS, len(self.top_k),
                                                                                     len(self.recall_iou)))
        ks = np.ascontiguousarray(self.top_k, dtype=np.int32)
        ts = np.ascontiguousarray(self.recall_iou, dtype=np.float32)
        h = L.vp(0)
        L.check(L.lib().rpn_evaluator_create(self.total_labels, self.max_images, self.max_detections, self.iou_threshold,
                                             ks.ctypes.data_as(L.c_int_p), len(self.top_k), ts.ctypes.data_as(L.c_float_p),
                                             len(self.recall_iou), ctypes.byref(h)), "rpn_evaluator_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().rpn_evaluator_destroy(h)
            except Exception:
                pass

    def memory_bytes(self):
        n = ctypes.c_size_t(0)
        L.check(L.lib().rpn_evaluator_memory_bytes(self._h, ctypes.byref(n)), "rpn_evaluator_memory_bytes")
        return int(n.value)

    @property
    def images(self):
        """detection images counted so far (a host counter: ``update`` knows its batch size)"""
        return int(L.lib().rpn_evaluator_images(self._h))

    def reset(self):
        L.check(L.lib().rpn_evaluator_reset(self._h, L.stream_ptr()), "rpn_evaluator_reset")

    # ---- accumulation -------------------------------------------------------------------
    @staticmethod
    def _check_gt(B, gt_boxes, gt_labels, gt_difficult):
        gs, ls = _shape(gt_boxes), _shape(gt_labels)
        if len(gs) != 3 or gs[0] != B or gs[2] != 4 or ls != gs[:2]:
            raise ValueError("expected gt_boxes (%d,G,4) and gt_labels (%d,G), got %s and %s" % (B, B, gs, ls))
        G = gs[1]
        if G < 1 or G > MAX_GT:
            raise ValueError("G = %d, must be in [1, %d] (pad an image without objects with a row of label -1)" % (G, MAX_GT))
        if gt_difficult is not None and _shape(gt_difficult) != (B, G):
            raise ValueError("gt_difficult must be (%d, %d) uint8, got %s" % (B, G, _shape(gt_difficult)))
        return G

    @staticmethod
    def _gt_to_device(gt_boxes, gt_labels, gt_difficult):
        g = L.to_device(gt_boxes)[0]
        lab = L.to_device(gt_labels, dtype=torch.int32)[0]
        diff = L.to_device(gt_difficult, dtype=torch.uint8)[0] if gt_difficult is not None else None
        return g, lab, diff

    def update(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_difficult=None, return_flags=True):
        """One batch of detections -- (boxes (B,M,4), scores (B,M), classes (B,M), valid (B,)) as ``non_max_suppression`` /
        ``DetectionHead.detect`` return them, M == ``max_detections`` -- against gt_boxes (B,G,4), gt_labels (B,G) (a gt iff >= 1)
        and gt_difficult (B,G) uint8 or None.  Returns the (B,M) int32 flags, 1 TP / 0 FP / -1 not counted (numpy for numpy
        boxes), or None with ``return_flags=False``.  Raises ``ValueError`` before anything is launched."""
        bs, ss, cs, vs = _shape(boxes), _shape(scores), _shape(classes), _shape(valid)
        if len(bs) != 3 or bs[2] != 4 or ss != bs[:2] or cs != bs[:2] or vs != bs[:1] or bs[0] < 1:
            raise ValueError("expected boxes (B,M,4), scores (B,M), classes (B,M), valid (B,); got %s %s %s %s" % (bs, ss, cs, vs))
        B, M = bs[:2]
        if M != self.max_detections:
            raise ValueError("M = %d detections per image, the evaluator was made for max_detections = %d" % (M, self.max_detections))
        G = self._check_gt(B, gt_boxes, gt_labels, gt_difficult)
        if self.images + B > self.max_images:
            raise ValueError("%d images seen + %d > max_images = %d" % (self.images, B, self.max_images))
        b, was_np = L.to_device(boxes)
        s, c = L.to_device(scores)[0], L.to_device(classes)[0]
        v = L.to_device(valid, dtype=torch.int32)[0]
        g, lab, diff = self._gt_to_device(gt_boxes, gt_labels, gt_difficult)
        flags = torch.empty((B, M), dtype=torch.int32, device="cuda") if return_flags else None
        st = L.lib().rpn_evaluator_update(self._h, L.ptr(b), L.ptr(s), L.ptr(c), L.ptr(v), L.ptr(g), L.ptr(lab), L.ptr(diff), B, G,
                                          L.ptr(flags), L.stream_ptr())
        L.check(st, "DetectionEvaluator.update")
        return L.from_device(flags, was_np) if return_flags else None

    def update_proposals(self, rois, valid, gt_boxes, gt_labels, gt_difficult=None):
        """One batch of proposals -- rois (B,R,4) in score order and valid (B,) or None, as ``Proposer.propose`` returns them --
        for the recall of the RPN alone at the ``top_k`` cut-offs and ``recall_iou`` thresholds."""
        rs = _shape(rois)
        if len(rs) != 3 or rs[2] != 4 or rs[0] < 1 or rs[1] < 1:
            raise ValueError("expected rois (B,R,4), got %s" % (rs,))
        B, R = rs[:2]
        if valid is not None and _shape(valid) != (B,):
            raise ValueError("valid must be (%d,) int32, got %s" % (B, _shape(valid)))
        G = self._check_gt(B, gt_boxes, gt_labels, gt_difficult)
        r = L.to_device(rois)[0]
        v = L.to_device(valid, dtype=torch.int32)[0] if valid is not None else None
        g, lab, diff = self._gt_to_device(gt_boxes, gt_labels, gt_difficult)
        st = L.lib().rpn_evaluator_update_proposals(self._h, L.ptr(r), L.ptr(v), R, L.ptr(g), L.ptr(lab), L.ptr(diff), B, G,
                                                    L.stream_ptr())
        L.check(st, "DetectionEvaluator.update_proposals")

    # ---- results ------------------------------------------------------------------------
    def result(self):
        """Everything seen so far -> {"ap", "ap_11pt": (C,) float64 (NaN where a class has no gt, index 0 always), "mAP",
        "mAP_11pt": their means over the classes with gts (NaN if there is none), "npos", "ndet": (C,) int32, "recall": (K,T)
        float64 (NaN without gts), "n_gt", "images"}.  The one synchronisation: the results are copied to the host."""
        C, K, T = self.total_labels, len(self.top_k), len(self.recall_iou)
        ap = torch.empty((2, C), dtype=torch.float64, device="cuda")
        counts = torch.empty((2, C), dtype=torch.int32, device="cuda")
        recall = torch.empty((max(K * T, 1),), dtype=torch.float64, device="cuda")
        n_gt = torch.empty((1,), dtype=torch.int64, device="cuda")
        st = L.lib().rpn_evaluator_result(self._h, L.ptr(ap[0]), L.ptr(ap[1]), L.ptr(counts[0]), L.ptr(counts[1]), L.ptr(recall),
                                          L.ptr(n_gt), L.stream_ptr())
        L.check(st, "DetectionEvaluator.result")
        ap_h, counts_h = ap.cpu().numpy(), counts.cpu().numpy()
        has_gt = counts_h[0] > 0
        mean = lambda a: float(np.mean(a[has_gt])) if has_gt.any() else float("nan")
        return {"ap": ap_h[0], "ap_11pt": ap_h[1], "mAP": mean(ap_h[0]), "mAP_11pt": mean(ap_h[1]), "npos": counts_h[0],
                "ndet": counts_h[1], "recall": recall.cpu().numpy()[:K * T].reshape(K, T), "n_gt": int(n_gt.cpu()[0]),
                "images": self.images}

    def pr_curve(self, c):
        """Class ``c``'s records in rank order -> (scores float32, tp int32, slots int32), numpy; slot = image * M + row.
        precision = cumsum(tp) / arange(1, n + 1), recall = cumsum(tp) / npos[c]."""
        c = int(c)
        if not 1 <= c < self.total_labels:
            raise ValueError("class %d outside [1, %d)" % (c, self.total_labels))
        cap = max(self.images * self.max_detections, 1)
        scores = torch.empty((cap,), dtype=torch.float32, device="cuda")
        out = torch.empty((2, cap), dtype=torch.int32, device="cuda")
        n = torch.empty((1,), dtype=torch.int32, device="cuda")
        st = L.lib().rpn_evaluator_pr_curve(self._h, c, L.ptr(scores), L.ptr(out[0]), L.ptr(out[1]), cap, L.ptr(n), L.stream_ptr())
        L.check(st, "DetectionEvaluator.pr_curve")
        k = int(n.cpu()[0])
        return scores[:k].cpu().numpy(), out[0, :k].cpu().numpy(), out[1, :k].cpu().numpy()


MAX_IOU_THRESHOLDS = 10
MAX_AREA_RANGES = 4
MAX_CUTS = 4
COCO_IOU_THRESHOLDS = tuple(np.float32(0.5 + 0.05 * i) for i in range(10))
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
COCO_MAX_DETS = (1, 10, 100)


class CocoEvaluator(object):
    """COCO-style scoring beside ``DetectionEvaluator`` (``rpn_coco_evaluator_*``; the rules are written out in
    ``include/rpn_hip.h``): AP over ``iou_thresholds`` and ``area_ranges`` (pixels^2 of the ``image_size`` (height, width), or of the
    per-image ``image_sizes`` given to ``update``), AR at the ``max_dets`` cut-offs.  The greedy rule of pycocotools' ``COCOeval``
    in bbox mode, without crowd boxes; of two gts with the same IoU the LAST is the match.  It owns all its device memory from its
    creation (``memory_bytes()``: 36 bytes per detection row of ``max_images * max_detections``, plus the counters)."""

    def __init__(self, total_labels, max_images, max_detections=300, iou_thresholds=None, area_ranges=None, max_dets=COCO_MAX_DETS,
                 image_size=(500, 500)):
        self.total_labels, self.max_images, self.max_detections = int(total_labels), int(max_images), int(max_detections)
        thr = np.ascontiguousarray(COCO_IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds, dtype=np.float32).reshape(-1)
        areas = np.ascontiguousarray(COCO_AREA_RANGES if area_ranges is None else area_ranges, dtype=np.float32)
        cuts = np.ascontiguousarray(COCO_MAX_DETS if max_dets is None else max_dets, dtype=np.int32).reshape(-1)
        if not 1 <= thr.size <= MAX_IOU_THRESHOLDS:
            raise ValueError("%d IoU thresholds, must be in [1, %d]" % (thr.size, MAX_IOU_THRESHOLDS))
        if areas.ndim != 2 or areas.shape[1] != 2 or not 1 <= areas.shape[0] <= MAX_AREA_RANGES:
            raise ValueError("area_ranges must be (A, 2) with 1 <= A <= %d, got %s" % (MAX_AREA_RANGES, areas.shape))
        if not 1 <= cuts.size <= MAX_CUTS:
            raise ValueError("%d cut-offs in max_dets, must be in [1, %d]" % (cuts.size, MAX_CUTS))
        if len(tuple(image_size)) != 2:
            raise ValueError("image_size must be (height, width), got %r" % (image_size,))
        self.iou_thresholds, self.area_ranges, self.max_dets = thr, areas, tuple(int(k) for k in cuts)
        self.image_size = (float(image_size[0]), float(image_size[1]))
        h = L.vp(0)
        L.check(L.lib().rpn_coco_evaluator_create(self.total_labels, self.max_images, self.max_detections,
                                                  thr.ctypes.data_as(L.c_float_p), thr.size, areas.ctypes.data_as(L.c_float_p),
                                                  areas.shape[0], cuts.ctypes.data_as(L.c_int_p), cuts.size, self.image_size[0],
                                                  self.image_size[1], ctypes.byref(h)), "rpn_coco_evaluator_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().rpn_coco_evaluator_destroy(h)
            except Exception:
                pass

    def memory_bytes(self):
        n = ctypes.c_size_t(0)
        L.check(L.lib().rpn_coco_evaluator_memory_bytes(self._h, ctypes.byref(n)), "rpn_coco_evaluator_memory_bytes")
        return int(n.value)

    @property
    def images(self):
        """images counted so far (a host counter: ``update`` knows its batch size)"""
        return int(L.lib().rpn_coco_evaluator_images(self._h))

    def reset(self):
        L.check(L.lib().rpn_coco_evaluator_reset(self._h, L.stream_ptr()), "rpn_coco_evaluator_reset")

    def update(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_difficult=None, image_sizes=None, return_flags=False):
        """One batch, the arguments of ``DetectionEvaluator.update`` and image_sizes (B,2) float32 [height, width] or None (the
        evaluator's ``image_size``).  Returns the (B,M,A,T) int8 flags -- 1 TP / 0 FP / -1 ignored / -2 not counted; numpy for numpy
        boxes -- with ``return_flags=True``, else None.  Raises ``ValueError`` before anything is launched."""
        bs, ss, cs, vs = _shape(boxes), _shape(scores), _shape(classes), _shape(valid)
        if len(bs) != 3 or bs[2] != 4 or ss != bs[:2] or cs != bs[:2] or vs != bs[:1] or bs[0] < 1:
            raise ValueError("expected boxes (B,M,4), scores (B,M), classes (B,M), valid (B,); got %s %s %s %s" % (bs, ss, cs, vs))
        B, M = bs[:2]
        if M != self.max_detections:
            raise ValueError("M = %d detections per image, the evaluator was made for max_detections = %d" % (M, self.max_detections))
        G = DetectionEvaluator._check_gt(B, gt_boxes, gt_labels, gt_difficult)
        if image_sizes is not None and _shape(image_sizes) != (B, 2):
            raise ValueError("image_sizes must be (%d, 2) float32 [height, width], got %s" % (B, _shape(image_sizes)))
        if self.images + B > self.max_images:
            raise ValueError("%d images seen + %d > max_images = %d" % (self.images, B, self.max_images))
        b, was_np = L.to_device(boxes)
        s, c = L.to_device(scores)[0], L.to_device(classes)[0]
        v = L.to_device(valid, dtype=torch.int32)[0]
        g, lab, diff = DetectionEvaluator._gt_to_device(gt_boxes, gt_labels, gt_difficult)
        sizes = L.to_device(image_sizes)[0] if image_sizes is not None else None
        A, T = self.area_ranges.shape[0], self.iou_thresholds.size
        flags = torch.empty((B, M, A, T), dtype=torch.int8, device="cuda") if return_flags else None
        st = L.lib().rpn_coco_evaluator_update(self._h, L.ptr(b), L.ptr(s), L.ptr(c), L.ptr(v), L.ptr(g), L.ptr(lab), L.ptr(diff),
                                               L.ptr(sizes), B, G, L.ptr(flags), L.stream_ptr())
        L.check(st, "CocoEvaluator.update")
        return L.from_device(flags, was_np) if return_flags else None

    def result(self):
        """Everything seen so far -> {"ap" (C,A,T), "ar" (C,A,T,K) float64 (NaN where a class has no counted gt in the area range,
        class 0 always), "npig" (C,A), "ndet" (C,) int32, "images", and the summaries -- means over the non-NaN entries, NaN if
        there is none: "AP", "AP50", "AP75" (NaN unless that threshold is configured), "AP_area" (A,), "AR_max_dets" (K,) at area 0,
        "AR_area" (A,) at the last cut-off, "stats": pycocotools' twelve numbers in ``summarize`` order under the default
        configuration, else None}.  The one synchronisation: the results are copied to the host."""
        C, A, T, K = self.total_labels, self.area_ranges.shape[0], self.iou_thresholds.size, len(self.max_dets)
        ap = torch.empty((C, A, T), dtype=torch.float64, device="cuda")
        ar = torch.empty((C, A, T, K), dtype=torch.float64, device="cuda")
        npig = torch.empty((C, A), dtype=torch.int32, device="cuda")
        ndet = torch.empty((C,), dtype=torch.int32, device="cuda")
        st = L.lib().rpn_coco_evaluator_result(self._h, L.ptr(ap), L.ptr(ar), L.ptr(npig), L.ptr(ndet), L.stream_ptr())
        L.check(st, "CocoEvaluator.result")
        r = {"ap": ap.cpu().numpy(), "ar": ar.cpu().numpy(), "npig": npig.cpu().numpy(), "ndet": ndet.cpu().numpy(),
             "images": self.images}
        r.update(coco_summaries(r["ap"], r["ar"], self.iou_thresholds, self.area_ranges, self.max_dets))
        return r


def _nanmean(a):
    a = np.asarray(a, np.float64).reshape(-1)
    a = a[~np.isnan(a)]
    return float(np.mean(a)) if a.size else float("nan")


def coco_summaries(ap, ar, iou_thresholds, area_ranges, max_dets):
    """The summary numbers of ``CocoEvaluator.result`` from ap (C,A,T) and ar (C,A,T,K), on the host in float64."""
    thr = np.asarray(iou_thresholds, np.float32).reshape(-1)
    areas = np.asarray(area_ranges, np.float32)
    A, K = ap.shape[1], ar.shape[3]

    def at(value):
        hit = np.nonzero(thr == np.float32(value))[0]
        return _nanmean(ap[:, 0, hit[0]]) if hit.size else float("nan")

    out = {"AP": _nanmean(ap[:, 0, :]), "AP50": at(0.5), "AP75": at(0.75),
           "AP_area": np.array([_nanmean(ap[:, a, :]) for a in range(A)], np.float64),
           "AR_max_dets": np.array([_nanmean(ar[:, 0, :, k]) for k in range(K)], np.float64),
           "AR_area": np.array([_nanmean(ar[:, a, :, K - 1]) for a in range(A)], np.float64), "stats": None}
    default = (thr.size == len(COCO_IOU_THRESHOLDS) and np.array_equal(thr, np.asarray(COCO_IOU_THRESHOLDS, np.float32))
               and areas.shape == (4, 2) and np.array_equal(areas, np.asarray(COCO_AREA_RANGES, np.float32))
               and tuple(int(k) for k in max_dets) == COCO_MAX_DETS)
    if default:
        out["stats"] = np.array([out["AP"], out["AP50"], out["AP75"], out["AP_area"][1], out["AP_area"][2], out["AP_area"][3],
                                 out["AR_max_dets"][0], out["AR_max_dets"][1], out["AR_max_dets"][2], out["AR_area"][1],
                                 out["AR_area"][2], out["AR_area"][3]], np.float64)
    return out


def evaluate(proposer, head, feed, steps, evaluator, **nms_kwargs):
    """``steps`` batches of ``feed`` -- an iterator of (imgs, gt_boxes, gt_labels[, gt_difficult]) -- through ``proposer`` and
    ``head`` into ``evaluator`` (proposals and detections), then ``evaluator.result()``.  ``evaluator`` is a ``DetectionEvaluator``,
    a ``CocoEvaluator`` or a tuple / list of them: every batch goes to each (``update_proposals`` only to those that have it) and a
    list of results comes back.  ``nms_kwargs`` go to ``head.detect`` and on to ``roi_utils.roi_detections`` (``nms="gaussian", sigma=0.5,
    score_threshold=0.001`` scores Soft-NMS detections); ``max_total_size`` defaults to the (first) evaluator's
    ``max_detections``.  One synchronisation, at the end."""
    several = isinstance(evaluator, (tuple, list))
    evaluators = list(evaluator) if several else [evaluator]
    if not evaluators:
        raise ValueError("evaluate needs at least one evaluator")
    nms_kwargs.setdefault("max_total_size", evaluators[0].max_detections)
    feed = iter(feed)
    for _ in range(int(steps)):
        batch = next(feed)
        imgs, gt_boxes, gt_labels = batch[:3]
        gt_difficult = batch[3] if len(batch) > 3 else None
        x = L.to_device(imgs)[0]
        rois, _scores, valid, pooled = proposer.propose_features(x, pooling_size=head.pooling_size)
        for ev in evaluators:
            if hasattr(ev, "update_proposals"):
                ev.update_proposals(rois, valid, gt_boxes, gt_labels, gt_difficult)
        boxes, scores, classes, n = head.detect(rois, pooled, proposer.hyper_params["variances"], valid=valid, **nms_kwargs)
        for ev in evaluators:
            ev.update(boxes, scores, classes, n, gt_boxes, gt_labels, gt_difficult, return_flags=False)
    results = [ev.result() for ev in evaluators]
    return results if several else results[0]
