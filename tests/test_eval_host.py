"""CPU suite: the detection metric (VOC AP, proposal recall) restated in numpy as plainly as possible, pinned by hand-made cases, and
the C-ABI boundary of rpn_evaluator_* (no compute calls without a GPU).

``RefEvaluator`` is what tests/test_gpu_eval.py holds the device evaluator against: a Python loop over the detections of an image in
(score descending, row ascending) order with a ``taken`` array -- VOCdevkit's VOCevaldet, not the parallel formulation of the
kernels -- on the IoU of ``oracle.bbox_oracle.generate_iou_map``."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import bbox_oracle as bo
from tf_rpn_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rpn_evaluator_create", "rpn_evaluator_destroy", "rpn_evaluator_memory_bytes", "rpn_evaluator_reset",
               "rpn_evaluator_images", "rpn_evaluator_update", "rpn_evaluator_update_proposals", "rpn_evaluator_result",
               "rpn_evaluator_pr_curve"]


class RefEvaluator(object):
    def __init__(self, C, M, iou_threshold=0.5, top_k=(), recall_iou=()):
        self.C, self.M, self.thr = int(C), int(M), np.float32(iou_threshold)
        self.top_k, self.recall_iou = tuple(int(k) for k in top_k), tuple(np.float32(t) for t in recall_iou)
        self.reset()

    def reset(self):
        self.images = 0
        self.records = []                                   # (class, score, slot, tp) of every TP / FP record
        self.npos = np.zeros((self.C,), np.int64)
        self.hits = np.zeros((len(self.top_k), len(self.recall_iou)), np.int64)
        self.n_gt = 0
        self.reasons = {"tp": 0, "duplicate": 0, "ignored": 0, "miss": 0}    # why each live detection got its flag

    def update(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_difficult=None):
        boxes, scores, classes = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(classes, np.float32)
        gt_boxes, gt_labels = np.asarray(gt_boxes, np.float32), np.asarray(gt_labels)
        B, M = scores.shape
        G = gt_labels.shape[1]
        assert M == self.M
        diff = np.zeros((B, G), bool) if gt_difficult is None else np.asarray(gt_difficult) != 0
        flags = np.full((B, M), -1, np.int32)
        for b in range(B):
            iou = bo.generate_iou_map(boxes[b][None], gt_boxes[b][None])[0]              # (M, G) float32
            for g in range(G):
                if 1 <= gt_labels[b, g] < self.C and not diff[b, g]:
                    self.npos[gt_labels[b, g]] += 1
            live = []
            for m in range(min(max(int(valid[b]), 0), M)):
                c, s = classes[b, m], scores[b, m]
                if np.isfinite(c) and c == np.floor(c) and 1 <= c < self.C and np.isfinite(s) and s > 0:
                    live.append(m)
            live.sort(key=lambda m: (-float(scores[b, m]), m))
            taken = np.zeros((G,), bool)
            for m in live:
                c = int(classes[b, m])
                best, jmax = -np.inf, -1
                for g in range(G):
                    if gt_labels[b, g] == c and iou[m, g] > best:                        # strict: the first gt wins a tie
                        best, jmax = iou[m, g], g
                if jmax < 0 or not best >= self.thr:
                    flags[b, m], why = 0, "miss"
                elif diff[b, jmax]:
                    flags[b, m], why = -1, "ignored"                                     # does not take the gt
                elif not taken[jmax]:
                    taken[jmax] = True
                    flags[b, m], why = 1, "tp"
                else:
                    flags[b, m], why = 0, "duplicate"
                self.reasons[why] += 1
                if flags[b, m] >= 0:
                    self.records.append((c, float(scores[b, m]), (self.images + b) * M + m, int(flags[b, m])))
        self.images += B
        return flags

    def update_proposals(self, rois, valid, gt_boxes, gt_labels, gt_difficult=None):
        rois, gt_boxes, gt_labels = np.asarray(rois, np.float32), np.asarray(gt_boxes, np.float32), np.asarray(gt_labels)
        B, R = rois.shape[:2]
        G = gt_labels.shape[1]
        diff = np.zeros((B, G), bool) if gt_difficult is None else np.asarray(gt_difficult) != 0
        for b in range(B):
            iou = bo.generate_iou_map(rois[b][None], gt_boxes[b][None])[0]               # (R, G)
            nv = R if valid is None else min(max(int(valid[b]), 0), R)
            for g in range(G):
                if gt_labels[b, g] < 1 or diff[b, g]:
                    continue
                self.n_gt += 1
                for ki, k in enumerate(self.top_k):
                    best = -np.inf
                    for r in range(min(k, nv)):
                        if iou[r, g] > best:
                            best = iou[r, g]
                    for ti, t in enumerate(self.recall_iou):
                        if best >= t:
                            self.hits[ki, ti] += 1

    def pr_curve(self, c):
        rec = sorted((r for r in self.records if r[0] == c), key=lambda r: (-r[1], r[2]))
        return (np.array([r[1] for r in rec], np.float32), np.array([r[3] for r in rec], np.int32),
                np.array([r[2] for r in rec], np.int32))

    def curve(self, c):
        """(precision, recall) at every rank of class c, float64"""
        _s, tp, _slots = self.pr_curve(c)
        cum = np.cumsum(tp)
        prec = np.array([cum[i] / float(i + 1) for i in range(len(tp))], np.float64)
        return prec, cum / float(self.npos[c]) if self.npos[c] else np.full(len(tp), np.nan)

    def result(self):
        C = self.C
        ap, ap11 = np.full((C,), np.nan), np.full((C,), np.nan)
        ndet = np.zeros((C,), np.int64)
        for c in range(1, C):
            _s, tp, _slots = self.pr_curve(c)
            n, npos = len(tp), int(self.npos[c])
            ndet[c] = n
            if npos == 0:
                continue
            cum, prec, t = [], [], 0
            for i in range(n):
                t += int(tp[i])
                cum.append(t)
                prec.append(t / float(i + 1))
            pmax, run = [0.0] * n, 0.0
            for i in range(n - 1, -1, -1):
                run = max(run, prec[i])
                pmax[i] = run
            total = 0.0
            for i in range(n):
                if tp[i]:
                    total += pmax[i]
            ap[c] = total / npos
            s11 = 0.0
            for k in range(11):
                vals = [prec[i] for i in range(n) if 10 * cum[i] >= k * npos]              # integers, on purpose
                s11 += max(vals) if vals else 0.0
            ap11[c] = s11 / 11.0
        has = self.npos > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            recall = self.hits / float(self.n_gt) if self.n_gt else np.full(self.hits.shape, np.nan)
        return {"ap": ap, "ap_11pt": ap11, "mAP": float(np.mean(ap[has])) if has.any() else float("nan"),
                "mAP_11pt": float(np.mean(ap11[has])) if has.any() else float("nan"), "npos": self.npos.copy(), "ndet": ndet,
                "recall": recall, "n_gt": self.n_gt, "images": self.images, "hits": self.hits.copy()}


# ---- hand-made cases: (boxes, scores, classes, valid, gt_boxes, gt_labels, gt_difficult), one image each --------------------
def _img(dets, gts, M=None):
    """dets: [(box, score, class)], gts: [(box, label, difficult)] -> batch-of-one arrays"""
    M = M or len(dets)
    boxes, scores, classes = np.zeros((1, M, 4), np.float32), np.zeros((1, M), np.float32), np.zeros((1, M), np.float32)
    for m, (box, s, c) in enumerate(dets):
        boxes[0, m], scores[0, m], classes[0, m] = box, s, c
    G = max(len(gts), 1)
    gt_boxes, gt_labels, gt_diff = np.zeros((1, G, 4), np.float32), np.full((1, G), -1, np.int32), np.zeros((1, G), np.uint8)
    for g, (box, lab, d) in enumerate(gts):
        gt_boxes[0, g], gt_labels[0, g], gt_diff[0, g] = box, lab, d
    return boxes, scores, classes, np.array([len(dets)], np.int32), gt_boxes, gt_labels, gt_diff


A_BOX, B_BOX, D_BOX = [0.0, 0.0, 0.4, 0.4], [0.5, 0.5, 0.9, 0.9], [0.0, 0.5, 0.4, 0.9]


def case_required():
    """gts A, B (class 1) and D (class 1, difficult).  d0 = A; d1 = A shifted (IoU 0.95 with A: a duplicate); d2 = D; d3 touches
    nothing; d4 = B."""
    dets = [(A_BOX, 0.9, 1), ([0.02, 0.0, 0.4, 0.4], 0.8, 1), (D_BOX, 0.7, 1), ([0.6, 0.0, 0.62, 0.02], 0.6, 1), (B_BOX, 0.5, 1)]
    return _img(dets, [(A_BOX, 1, 0), (B_BOX, 1, 0), (D_BOX, 1, 1)])


def case_iou_equal_to_threshold():
    """detection [0,0,1,1] (area 1) on gt [0,0,1,0.5] (area 0.5): inter 0.5, union 1 + 0.5 - 0.5 = 1, IoU exactly 0.5 in float32"""
    return _img([([0.0, 0.0, 1.0, 1.0], 0.9, 1)], [([0.0, 0.0, 1.0, 0.5], 1, 0)])


def case_equal_iou_two_gts():
    """two identical gts: the detection's IoU with both is 1; the FIRST is its match, so a second detection finds it taken (the
    second gt is never matched by anyone: it is nobody's jmax)"""
    return _img([(A_BOX, 0.9, 1), (A_BOX, 0.8, 1)], [(A_BOX, 1, 0), (A_BOX, 1, 0)])


def case_equal_scores():
    """two detections of the same score on one gt: the lower row is the true positive"""
    return _img([([0.01, 0.0, 0.4, 0.4], 0.5, 1), (A_BOX, 0.5, 1)], [(A_BOX, 1, 0)])


def case_recall_three_tenths():
    """class 1: ten gts, three detected (1.0 precision each), then a false positive.  class 2: a gt and no detection.  class 3:
    a detection and no gt."""
    cells = [[0.1 * i, 0.0, 0.1 * i + 0.08, 0.08] for i in range(10)]
    dets = [(cells[0], 0.9, 1), (cells[1], 0.8, 1), (cells[2], 0.7, 1), ([0.5, 0.5, 0.6, 0.6], 0.6, 1), ([0.5, 0.5, 0.6, 0.6], 0.9, 3)]
    return _img(dets, [(c, 1, 0) for c in cells] + [([0.7, 0.7, 0.9, 0.9], 2, 0)])


def test_required_case_flags_curve_and_aps():
    ref = RefEvaluator(2, 5)
    flags = ref.update(*case_required())
    assert flags.tolist() == [[1, 0, -1, 0, 1]]
    prec, rec = ref.curve(1)
    # ranking: d0 TP, d1 FP, d3 FP, d4 TP (d2 is ignored: in neither count)
    assert prec.tolist() == [1.0, 1.0 / 2, 1.0 / 3, 2.0 / 4] and rec.tolist() == [0.5, 0.5, 0.5, 1.0]
    r = ref.result()
    assert r["npos"].tolist() == [0, 2] and r["ndet"].tolist() == [0, 4]
    # all-point: pmax(d0) = 1, pmax(d4) = 2/4 -> (1 + 0.5) / 2;  11-point: 10 tp >= 2 k holds from rank 0 (tp = 1) for k <= 5, from rank
    # 3 (tp = 2) for k = 6..10 -> (6 * 1 + 5 * 0.5) / 11
    assert r["ap"][1] == 0.75 and r["ap_11pt"][1] == 8.5 / 11 and math.isnan(r["ap"][0]) and math.isnan(r["ap_11pt"][0])
    assert r["mAP"] == 0.75 and r["mAP_11pt"] == 8.5 / 11


def test_iou_exactly_at_the_threshold_is_a_match():
    case = case_iou_equal_to_threshold()
    iou = bo.generate_iou_map(case[0][0][None], case[4][0][None])[0]
    assert iou.dtype == np.float32 and iou[0, 0] == np.float32(0.5)
    ref = RefEvaluator(2, 1, iou_threshold=0.5)
    assert ref.update(*case).tolist() == [[1]]              # >=, as the devkit
    assert RefEvaluator(2, 1, iou_threshold=np.nextafter(np.float32(0.5), np.float32(1))).update(*case).tolist() == [[0]]


def test_ties_first_gt_and_lower_row():
    ref = RefEvaluator(2, 2)
    assert ref.update(*case_equal_iou_two_gts()).tolist() == [[1, 0]]
    assert ref.result()["npos"][1] == 2
    ref = RefEvaluator(2, 2)
    assert ref.update(*case_equal_scores()).tolist() == [[1, 0]]
    scores, tp, slots = ref.pr_curve(1)
    assert tp.tolist() == [1, 0] and slots.tolist() == [0, 1]                            # equal scores: the lower slot ranks first


def test_recall_of_three_tenths_counts_for_k_3_and_the_empty_classes():
    ref = RefEvaluator(5, 5)
    flags = ref.update(*case_recall_three_tenths())
    assert flags.tolist() == [[1, 1, 1, 0, 0]]
    r = ref.result()
    # class 1: precision 1, 1, 1, 3/4; recall reaches 3/10 at rank 2.  10 * 3 >= 3 * 10: k = 0..3 see precision 1, k >= 4 nothing.
    # (in float64, 3 / 10 < np.arange(0, 1.1, 0.1)[3] = 0.30000000000000004: the common port gives 3 / 11 here)
    assert 3 / 10.0 < np.arange(0, 1.1, 0.1)[3]
    assert r["ap_11pt"][1] == 4.0 / 11 and r["ap"][1] == 3.0 / 10
    assert r["npos"].tolist() == [0, 10, 1, 0, 0] and r["ndet"].tolist() == [0, 4, 0, 1, 0]
    assert r["ap"][2] == 0.0 and r["ap_11pt"][2] == 0.0                                  # gts, no detections
    assert math.isnan(r["ap"][3]) and math.isnan(r["ap_11pt"][3]) and math.isnan(r["ap"][4])   # no gts
    assert r["mAP"] == (3.0 / 10 + 0.0) / 2


def test_dropped_rows_and_difficult_only_class():
    boxes, scores, classes, valid, gtb, gtl, gtd = case_required()
    classes[0, 0], scores[0, 1], classes[0, 3], scores[0, 4] = 1.5, np.nan, 2.0, np.inf   # fractional, NaN, class == C, inf
    ref = RefEvaluator(2, 5)
    assert ref.update(boxes, scores, classes, valid, gtb, gtl, gtd).tolist() == [[-1, -1, -1, -1, -1]]
    assert ref.result()["ndet"].tolist() == [0, 0] and ref.result()["ap"][1] == 0.0


def test_proposal_recall_restatement():
    rois = np.array([[[0.6, 0.0, 0.62, 0.02], A_BOX, B_BOX]], np.float32)
    gtb = np.array([[A_BOX, B_BOX, D_BOX, A_BOX]], np.float32)
    gtl, gtd = np.array([[1, 2, 1, 0]], np.int32), np.array([[0, 0, 1, 0]], np.uint8)
    ref = RefEvaluator(3, 1, top_k=(1, 2, 5), recall_iou=(0.5, 1.0))
    ref.update_proposals(rois, np.array([3], np.int32), gtb, gtl, gtd)
    assert ref.n_gt == 2 and ref.hits.tolist() == [[0, 0], [1, 1], [2, 2]]               # the difficult and the background row do not count
    ref.update_proposals(rois, np.array([0], np.int32), gtb, gtl, None)                  # no live RoI: no hit; D counts now
    assert ref.n_gt == 5 and ref.hits.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert ref.result()["recall"].tolist() == [[0.0, 0.0], [0.2, 0.2], [0.4, 0.4]]
    assert np.isnan(RefEvaluator(3, 1, top_k=(1,), recall_iou=(0.5,)).result()["recall"]).all()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rpn_[a-z0-9_]+)\s*\(", code))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name), "librpn_hip.so does not export %s" % name
        assert name in L.exported_symbols(), "%s is not bound in tf_rpn_amd/_lib.py" % name
    assert "typedef struct rpn_evaluator rpn_evaluator;" in code
    for phrase in ("VOCevaldet", ">=, as the devkit", "IN INTEGERS", "FIRST on ties"):   # the contract is written out in the header
        assert phrase in header, phrase


def _create(lib, C=21, max_images=16, M=300, thr=0.5, top_k=(10, 100, 300), recall_iou=(0.5, 0.7)):
    ks, ts = (ctypes.c_int * max(len(top_k), 1))(*top_k), (ctypes.c_float * max(len(recall_iou), 1))(*recall_iou)
    h = L.vp(0)
    return lib.rpn_evaluator_create(C, max_images, M, thr, ks, len(top_k), ts, len(recall_iou), ctypes.byref(h)), h


def test_argument_validation_precedes_device_use(lib):
    for bad in (dict(C=1), dict(C=70000), dict(max_images=0), dict(M=0), dict(M=4097), dict(max_images=1 << 20, M=4096), dict(thr=0.0),
                dict(thr=1.5), dict(top_k=(0,)), dict(top_k=tuple(range(1, 10))), dict(recall_iou=(0.5,) * 9), dict(recall_iou=(0.0,))):
        st, h = _create(lib, **bad)
        assert st == L.RPN_ERR_INVALID and not h.value, bad
        assert b"rpn_evaluator_create" in lib.rpn_last_error()
    st, h = _create(lib, max_images=4952)
    assert st == L.RPN_OK and h.value
    try:
        n = ctypes.c_size_t(0)
        assert lib.rpn_evaluator_memory_bytes(h, ctypes.byref(n)) == L.RPN_OK
        assert 24 * 4952 * 300 <= n.value <= 24 * 4952 * 300 + (1 << 16)                # records + the sort's ping-pong pair + counters
        assert lib.rpn_evaluator_images(h) == 0
        buf = np.zeros((64,), np.float32)
        p = L.vp(buf.ctypes.data + (-buf.ctypes.data) % 16)
        args = (h, p, p, p, p, p, p, None)
        assert lib.rpn_evaluator_update(*(args + (1, 0, None, None))) == L.RPN_ERR_INVALID          # G = 0
        assert lib.rpn_evaluator_update(*(args + (1, 2049, None, None))) == L.RPN_ERR_INVALID and b"2048" in lib.rpn_last_error()
        assert lib.rpn_evaluator_update(*(args + (4953, 4, None, None))) == L.RPN_ERR_INVALID and b"max_images" in lib.rpn_last_error()
        assert lib.rpn_evaluator_update(h, None, p, p, p, p, p, None, 1, 4, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_evaluator_update_proposals(h, p, None, 0, p, p, None, 1, 4, None) == L.RPN_ERR_INVALID
        assert lib.rpn_evaluator_update_proposals(h, p, None, 300, p, p, None, 1, 2049, None) == L.RPN_ERR_INVALID
        assert lib.rpn_evaluator_pr_curve(h, 0, p, p, p, 4, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_evaluator_pr_curve(h, 21, p, p, p, 4, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_evaluator_images(h) == 0
    finally:
        lib.rpn_evaluator_destroy(h)


def test_python_checks_raise_before_anything_is_launched():
    from tf_rpn_amd.utils import eval_utils
    with pytest.raises(ValueError):
        eval_utils.DetectionEvaluator(21, 8, 300, top_k=tuple(range(1, 10)))
    with pytest.raises(ValueError):
        eval_utils.DetectionEvaluator(21, 8, 300, recall_iou=(0.5,) * 9)
    ev = eval_utils.DetectionEvaluator(total_labels=4, max_images=2, max_detections=5)
    assert ev.images == 0 and ev.memory_bytes() >= 24 * 10
    boxes, scores, classes, valid, gtb, gtl, gtd = case_required()
    with pytest.raises(ValueError):
        ev.update(boxes[:, :4], scores[:, :4], classes[:, :4], valid, gtb, gtl, gtd)                # M != max_detections
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes[:, :4], valid, gtb, gtl, gtd)                              # wrong shape
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes, valid, gtb, gtl, gtd[:, :2])
    rep = lambda a, n: np.repeat(a, n, axis=0)
    with pytest.raises(ValueError):                                                                  # 3 images > max_images
        ev.update(rep(boxes, 3), rep(scores, 3), rep(classes, 3), rep(valid, 3), rep(gtb, 3), rep(gtl, 3), rep(gtd, 3))
    with pytest.raises(ValueError):                                                                  # G > 2048
        ev.update(boxes, scores, classes, valid, np.zeros((1, 2049, 4), np.float32), np.zeros((1, 2049), np.int32))
    with pytest.raises(ValueError):
        ev.update_proposals(np.zeros((1, 7, 3), np.float32), None, gtb, gtl)
    with pytest.raises(ValueError):
        ev.pr_curve(0)
    assert ev.images == 0
