"""The COCO-style detection metric (rpn_coco_evaluator_*, include/rpn_hip.h) restated in numpy as plainly as possible: Python loops,
``oracle.bbox_oracle.generate_iou_map`` for the IoUs, float32 pixel areas rounded after every operation, sequential float64 sums.
Written from the rules, not from the kernels: one greedy loop per (image, class, area range, threshold) with its own ``taken`` array.

``RefCocoEvaluator.reasons`` counts why each (detection, area range, threshold) got its flag, so that a random case can prove that
it exercised every branch."""
import numpy as np

from oracle import bbox_oracle as bo

DEFAULT_IOU = tuple(np.float32(0.5 + 0.05 * i) for i in range(10))
DEFAULT_AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
DEFAULT_MAX_DETS = (1, 10, 100)
REASONS = ("tp_best", "tp_second_choice", "tie_last", "ignored_gt", "ignored_area", "fp", "fp_gt_taken", "beyond_max_dets")
SPACING = 2.0 ** -52                                         # np.spacing(1)


def pixel_area(box, height, width):
    box = np.asarray(box, np.float32)
    h = np.float32(np.float32(box[2] - box[0]) * np.float32(height))
    w = np.float32(np.float32(box[3] - box[1]) * np.float32(width))
    return np.float32(h * w)


class RefCocoEvaluator(object):
    def __init__(self, C, M, iou_thresholds=None, area_ranges=None, max_dets=DEFAULT_MAX_DETS, image_size=(500, 500)):
        self.C, self.M = int(C), int(M)
        self.thr = [np.float32(t) for t in (DEFAULT_IOU if iou_thresholds is None else iou_thresholds)]
        self.areas = [(np.float32(lo), np.float32(hi)) for lo, hi in (DEFAULT_AREAS if area_ranges is None else area_ranges)]
        self.max_dets = tuple(int(k) for k in max_dets)
        self.image_size = (np.float32(image_size[0]), np.float32(image_size[1]))
        self.reset()

    def reset(self):
        self.images = 0
        self.records = []                                   # (class, score, slot, rank, flags (A,T)) of every ranked row
        self.npig = np.zeros((self.C, len(self.areas)), np.int64)
        self.reasons = dict((k, 0) for k in REASONS)

    def update(self, boxes, scores, classes, valid, gt_boxes, gt_labels, gt_difficult=None, image_sizes=None):
        boxes, scores, classes = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(classes, np.float32)
        gt_boxes, gt_labels = np.asarray(gt_boxes, np.float32), np.asarray(gt_labels)
        B, M = scores.shape
        G = gt_labels.shape[1]
        A, T = len(self.areas), len(self.thr)
        assert M == self.M
        diff = np.zeros((B, G), bool) if gt_difficult is None else np.asarray(gt_difficult) != 0
        flags = np.full((B, M, A, T), -2, np.int8)
        cut = self.max_dets[-1]
        for b in range(B):
            height, width = self.image_size if image_sizes is None else (np.float32(image_sizes[b][0]), np.float32(image_sizes[b][1]))
            iou = bo.generate_iou_map(boxes[b][None], gt_boxes[b][None])[0]              # (M, G) float32
            garea = [pixel_area(gt_boxes[b, g], height, width) for g in range(G)]
            for g in range(G):
                if 1 <= gt_labels[b, g] < self.C:
                    for a, (lo, hi) in enumerate(self.areas):
                        if not (diff[b, g] or garea[g] < lo or garea[g] > hi):
                            self.npig[gt_labels[b, g], a] += 1
            live = []
            for m in range(min(max(int(valid[b]), 0), M)):
                c, s = classes[b, m], scores[b, m]
                if np.isfinite(c) and c == np.floor(c) and 1 <= c < self.C and np.isfinite(s) and s > 0:
                    live.append(m)
            for c in sorted(set(int(classes[b, m]) for m in live)):
                D = sorted((m for m in live if int(classes[b, m]) == c), key=lambda m: (-float(scores[b, m]), m))
                self.reasons["beyond_max_dets"] += max(len(D) - cut, 0)
                D = D[:cut]
                gts = [g for g in range(G) if gt_labels[b, g] == c]
                for a, (lo, hi) in enumerate(self.areas):
                    ignored = dict((g, bool(diff[b, g] or garea[g] < lo or garea[g] > hi)) for g in gts)
                    for t, thr in enumerate(self.thr):
                        taken = set()
                        for m in D:
                            flags[b, m, a, t] = self._match(iou[m], gts, ignored, taken, thr, pixel_area(boxes[b, m], height, width), lo, hi)
                for rank, m in enumerate(D):
                    self.records.append((c, float(scores[b, m]), (self.images + b) * M + m, rank, flags[b, m].copy()))
        self.images += B
        return flags

    def _match(self, iou, gts, ignored, taken, thr, darea, lo, hi):
        match = -1
        for want_ignored in (False, True):
            best, cands = None, []
            for g in gts:
                if g in taken or ignored[g] != want_ignored or not iou[g] >= thr:        # a NaN never matches
                    continue
                if best is None or iou[g] >= best:                                       # >=: the LAST of equal IoUs wins
                    cands = cands + [g] if (best is not None and iou[g] == best) else [g]
                    best, match = iou[g], g
            if match >= 0:
                if len(cands) >= 2:
                    self.reasons["tie_last"] += 1
                break
        if match >= 0:
            taken.add(match)
            if ignored[match]:
                self.reasons["ignored_gt"] += 1
                return -1
            # the gt this detection would have had with nothing taken
            first = -1
            for g in gts:
                if not ignored[g] and iou[g] >= thr and (first < 0 or iou[g] >= iou[first]):
                    first = g
            self.reasons["tp_best" if first == match else "tp_second_choice"] += 1
            return 1
        if darea < lo or darea > hi:
            self.reasons["ignored_area"] += 1
            return -1
        self.reasons["fp_gt_taken" if any(iou[g] >= thr for g in gts) else "fp"] += 1
        return 0

    def ranking(self, c):
        return sorted((r for r in self.records if r[0] == c), key=lambda r: (-r[1], r[2]))

    def result(self):
        C, A, T, K = self.C, len(self.areas), len(self.thr), len(self.max_dets)
        ap, ar = np.full((C, A, T), np.nan), np.full((C, A, T, K), np.nan)
        ndet = np.zeros((C,), np.int64)
        for c in range(1, C):
            rows = self.ranking(c)
            ndet[c] = len(rows)
            for a in range(A):
                npig = int(self.npig[c, a])
                if npig == 0:
                    continue
                for t in range(T):
                    for k, cutoff in enumerate(self.max_dets):
                        tps, fps, tp, fp = [], [], 0, 0
                        for r in rows:
                            f = int(r[4][a, t])
                            if r[3] >= cutoff or f == -1:
                                continue
                            tp += f == 1
                            fp += f == 0
                            tps.append(tp)
                            fps.append(fp)
                        ar[c, a, t, k] = tp / float(npig)
                    # (the lists are the last cut-off's)
                    n = len(tps)
                    prec = [tps[i] / (float(tps[i] + fps[i]) + SPACING) for i in range(n)]
                    for i in range(n - 2, -1, -1):
                        prec[i] = max(prec[i], prec[i + 1])
                    total, i = 0.0, 0
                    for q in range(101):
                        while i < n and 100 * tps[i] < q * npig:                         # the first rank with 100 tp >= q npig: integers,
                            i += 1                                                       # on purpose (tp never falls, so i never goes back)
                        total += prec[i] if i < n else 0.0
                    ap[c, a, t] = total / 101.0
        return {"ap": ap, "ar": ar, "npig": self.npig.copy(), "ndet": ndet, "images": self.images}
