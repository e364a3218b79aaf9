"""Soft-NMS on the GPU (rpn_soft_nms, bbox_utils.soft_non_max_suppression, roi_detections(nms=...)) against the numpy restatement
of tests/test_soft_nms_host.py and against the hard NMS kernel.

Tolerances (none of them comes from what the kernel gives):
  * linear: all five outputs bit for bit -- the IoU is the hard NMS's float32 arithmetic and the decay rounds once per operation.
  * gaussian with sigma = +inf: bit for bit what bbox_utils.non_max_suppression returns (every weight is expf(-0.0) = 1).
  * gaussian: the device's expf is not numpy's.  One decay cur * expf(t), t = fl(fl(iou^2) k), carries at most
    (2 |t| + e + 1) 2^-24 relative error against the float64 restatement: the two roundings of t reach the result as 2 |t| 2^-24,
    e = 2 is the expf allowance of tests/test_gpu_roi_head.py's header, 1 the product's rounding; |t| <= 1 / sigma.  A score after k
    decays carries k times that (test_soft_nms_host.decay_bound).  A pair (image, class) is DECIDED when the smallest decision
    margin of its float64 run exceeds twice its own bound (its most-decayed score's k); decided pairs must match in rows, classes
    and count exactly and in scores within the bound.  Undecided pairs are skipped and counted: more than 10 % of a case's pairs
    skipped fails the test (test_soft_nms_host.py checks on the CPU that the generated cases stay inside that).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_det_head_host as dh  # noqa: E402
import test_roi_head_host as rh  # noqa: E402
import test_soft_nms_host as sn  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from test_soft_nms_host import lib  # noqa: E402,F401  (fixture)
from tf_rpn_amd.utils import bbox_utils, roi_utils  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def run(boxes, scores, **kw):
    return bbox_utils.soft_non_max_suppression(boxes, scores, return_indices=True, **kw)


def describe(got, ref):
    return ["%s differs at %d places" % (name, int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum()))
            for name, a, b in zip(("boxes", "scores", "classes", "valid", "indices"), got, ref) if a.tobytes() != b.tobytes()]


# ---- linear: bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(sn.LINEAR_SHAPES)))
def test_linear_bit_for_bit(lib, index):
    boxes, scores, kw, ref = sn.linear_case(index)
    got = run(boxes, scores, **kw)
    assert all(isinstance(a, np.ndarray) for a in got) and got[3].dtype == np.int32 and got[4].dtype == np.int32
    print(sn.LINEAR_SHAPES[index], "valid", got[3].tolist(), describe(got, ref))
    assert sn.same(got, ref)
    assert sn.same(run(boxes, scores, **kw), got)                                    # the same bits on a second run
    dev = run(torch.from_numpy(boxes.copy()).cuda(), torch.from_numpy(scores.copy()), **kw)
    assert all(t.is_cuda for t in dev) and sn.same([t.cpu().numpy() for t in dev], got)
    four = bbox_utils.soft_non_max_suppression(boxes, scores, **kw)
    assert len(four) == 4 and sn.same(four, got[:4])


def test_linear_image_without_a_candidate_and_batch_independence(lib):
    boxes, scores, kw, _ref = sn.linear_case(0)
    scores = scores.copy()
    scores[1] = F32(kw["score_threshold"])                                           # not above the threshold: no candidate
    ref = sn.soft_nms_ref(boxes, scores, **kw)
    got = run(boxes, scores, **kw)
    print("valid", got[3].tolist(), describe(got, ref))
    assert sn.same(got, ref) and got[3][1] == 0 and got[3][0] > 0 and (got[4][1] == -1).all()
    alone = run(boxes[:1], scores[:1], **kw)                                         # image 0 without the other image
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(alone, got))


def test_linear_at_the_size_limit_and_one_past_it(lib):
    N, C = sn.N_LIMIT, 2
    rng = np.random.RandomState(3)
    boxes, _ = sn.cluster_case(7, 1, N, C, 1, n_clusters=3)
    scores = np.zeros((1, N, C), F32)
    rows = np.unique(np.concatenate([[0, 63, 64, 255, 256, N - 257, N - 1], rng.randint(0, N, size=40)]))
    scores[0, rows] = rng.uniform(0.1, 0.9, size=(len(rows), C)).astype(F32)
    scores[0, [0, N - 1]] = F32([[0.99, 0.98], [1.0, 0.97]])                        # the first and the last row are taken
    kw = dict(max_output_size_per_class=30, max_total_size=50, method="linear", iou_threshold=0.3, score_threshold=0.05)
    ref = sn.soft_nms_ref(boxes, scores, **kw)
    got = run(boxes, scores, **kw)
    print("valid", got[3].tolist(), describe(got, ref))
    assert sn.same(got, ref) and got[3][0] >= 20 and got[4].max() == N - 1
    with pytest.raises(ValueError):
        run(np.zeros((1, N + 1, 1, 4), F32), np.zeros((1, N + 1, C), F32), **kw)


# ---- sigma = inf is the hard NMS ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0.5, 0.7])
@pytest.mark.parametrize("s", [0.05, 0.5])
def test_infinite_sigma_equals_the_hard_kernel(lib, t, s):
    boxes, scores = sn.tie_case()
    for m, total, clip in ((7, 12, True), (96, 300, False)):
        got = run(boxes, scores, max_output_size_per_class=m, max_total_size=total, method="gaussian", sigma=float("inf"),
                  iou_threshold=t, score_threshold=s, clip_boxes=clip)
        want = bbox_utils.non_max_suppression(boxes, scores, max_output_size_per_class=m, max_total_size=total, iou_threshold=t,
                                              score_threshold=s, clip_boxes=clip, return_indices=True)
        print("t", t, "s", s, "valid", got[3].tolist(), describe(got, want))
        assert sn.same(got, want) and got[3].min() > 0
    one = (boxes[:, :, 0, :][:, :, None, :].copy(), scores[:, :, 1:2].copy())          # C == 1: the hard kernel's one-launch form
    got = run(*one, max_output_size_per_class=50, max_total_size=40, method="gaussian", sigma=float("inf"), iou_threshold=t,
              score_threshold=s)
    want = bbox_utils.non_max_suppression(*one, max_output_size_per_class=50, max_total_size=40, iou_threshold=t, score_threshold=s,
                                          return_indices=True)
    assert sn.same(got, want)


# ---- gaussian against the float64 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(sn.GAUSS_CASES)))
def test_gaussian_against_float64(lib, index):
    sigma = sn.GAUSS_CASES[index][0]
    boxes, scores, kw, _ref, details = sn.gauss_case(index)
    ok = sn.decided(details, sigma)
    gb, gs, gc, gv, gi = run(boxes, scores, **kw)
    assert sn.same(run(boxes, scores, **kw), (gb, gs, gc, gv, gi))                   # the same bits on a second run
    B, N, C, _q = sn.GAUSS_SHAPE
    skipped, worst = 0, 0.0
    for b in range(B):
        n = int(gv[b])
        assert (gi[b, n:] == -1).all() and not gs[b, n:].any() and not gb[b, n:].any()
        key = list(zip((-gs[b, :n]).tolist(), gc[b, :n].tolist()))
        assert key == sorted(key)                                                    # the device's own merge order
        assert np.array_equal(gb[b, :n], np.clip(boxes[b, gi[b, :n], gc[b, :n].astype(int)], 0, 1))
        for c in range(C):
            sel, _margin, _kmax = details[(b, c)]
            if (b, c) not in ok:
                skipped += 1
                continue
            mine = gc[b, :n] == c
            rows, sc = gi[b, :n][mine], gs[b, :n][mine].astype(np.float64)
            assert rows.tolist() == [i for i, _s in sel], (b, c)
            want = np.array([s for _i, s in sel], np.float64)
            err = np.abs(sc - want) / want
            if ok[(b, c)] > 0:
                worst = max(worst, float(err.max()) / ok[(b, c)])
            assert (err <= ok[(b, c)]).all(), (b, c, float(err.max()), ok[(b, c)])
        if all((b, c) in ok for c in range(C)):
            assert n == sum(len(details[(b, c)][0]) for c in range(C))
    print("case", index, "pairs", B * C, "skipped", skipped, "largest err / bound", worst)
    assert skipped <= 0.1 * B * C


def test_gaussian_batch_independence(lib):
    boxes, scores, kw, _ref, _details = sn.gauss_case(0)
    full = run(boxes, scores, **kw)
    alone = run(boxes[:1], scores[:1], **kw)
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(alone, full))


# ---- roi_detections -----------------------------------------------------------------------------------------------------------------------
def head_outputs(C=5, seed=0):
    t = rh.target_case(0)                                                            # (B, R) = (2, 64); valid = [64, 43]
    rng = np.random.RandomState(seed)
    B, R = t["rois"].shape[:2]
    reg = rng.normal(0, 0.5, size=(B, R, 4 * C)).astype(F32)
    logits = rng.normal(0, 2.0, size=(B, R, C)).astype(F32)
    return t["rois"], reg, logits, t["valid"]


def test_roi_detections_hard_is_unchanged(lib):
    rois, reg, logits, valid = head_outputs()
    kw = dict(max_output_size_per_class=20, max_total_size=60, iou_threshold=0.5, score_threshold=0.05)
    boxes, scores = roi_utils.roi_decode_scores(rois, reg, logits, rh.VARIANCES, valid=valid)
    want = bbox_utils.non_max_suppression(boxes, scores, return_indices=True, **kw)
    got = roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, return_indices=True, nms="hard", **kw)
    default = roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, return_indices=True, **kw)
    assert sn.same(got, want) and sn.same(default, want) and want[3].min() > 0


@pytest.mark.parametrize("nms", ["linear", "gaussian"])
def test_roi_detections_soft(lib, nms):
    rois, reg, logits, valid = head_outputs()
    kw = dict(max_output_size_per_class=20, max_total_size=60, iou_threshold=0.5, score_threshold=0.05)
    boxes, scores = roi_utils.roi_decode_scores(rois, reg, logits, rh.VARIANCES, valid=valid)
    got = roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, return_indices=True, nms=nms, sigma=0.4, **kw)
    direct = run(boxes, scores, method=nms, sigma=0.4, **kw)
    assert sn.same(got, direct)                                                      # decode, then the new entry
    b, s, c, n, i = got
    hard = roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, **kw)
    assert n.min() > 0 and s.tobytes() != hard[1].tobytes()                           # decayed scores
    for img in range(len(n)):
        assert (c[img, :n[img]] >= 1).all()                                          # never the background
        assert (i[img, :n[img]] < valid[img]).all() and (i[img, :n[img]] >= 0).all()     # never a padding row
    if nms == "linear":
        ref = sn.soft_nms_ref(boxes, scores, method="linear", **kw)
        print("valid", n.tolist(), "hard", hard[3].tolist(), describe(got, ref))
        assert sn.same(got, ref)
    three = roi_utils.roi_detections(torch.from_numpy(rois.copy()).cuda(), reg, logits, rh.VARIANCES, valid=valid, nms=nms, sigma=0.4, **kw)
    assert len(three) == 4 and all(t.is_cuda for t in three) and sn.same([t.cpu().numpy() for t in three], got[:4])


def test_roi_detections_refuses_bad_options(lib):
    rois, reg, logits, valid = head_outputs()
    for kw in (dict(nms="soft"), dict(nms=None), dict(nms="gaussian", sigma=0.0), dict(nms="gaussian", sigma=-0.5),
               dict(nms="linear", score_threshold=-0.1), dict(nms="linear", score_threshold=0.0), dict(nms="hard", score_threshold=-0.1)):
        with pytest.raises(ValueError):
            roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, **kw)


def test_head_detect_passes_the_options_on(lib):
    import test_gpu_det_head as gd
    c = dh.head_case(1)
    head = gd.make_head(c)
    pooled = torch.from_numpy(np.array(c["pooled"])).cuda()
    t = rh.target_case(3)
    rois, valid = torch.from_numpy(np.array(t["rois"])).cuda(), torch.from_numpy(np.array(t["valid"])).cuda()
    kw = dict(valid=valid, score_threshold=0.02, max_total_size=50, max_output_size_per_class=10, nms="gaussian", sigma=0.5)
    got = head.detect(rois, pooled, rh.VARIANCES, **kw)
    with torch.no_grad():
        ref = roi_utils.roi_detections(rois, *reversed(head(pooled)), rh.VARIANCES, **kw)
        hard = roi_utils.roi_detections(rois, *reversed(head(pooled)), rh.VARIANCES, **dict(kw, nms="hard"))
    assert len(got) == len(ref) == 4 and int(got[3].sum()) > 0
    assert all(gd.same_bits(a, b) for a, b in zip(got, ref))
    assert not gd.same_bits(got[1], hard[1])                                         # and it is not the hard path


def test_proposer_detect_passes_the_options_on(lib):
    from tf_rpn_amd.models import DetectionHead
    from tf_rpn_amd.models._rpn_model import synthetic_weights
    from tf_rpn_amd.predictor import Proposer
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    prop = Proposer("vgg16", hyper_params=dict(hp), weights=synthetic_weights("vgg16", hp, seed=1), precision="f32", max_batch=2)
    head = DetectionHead(5, pooling_size=(3, 3), channels=prop.feature_extractor.output_shape[3], hidden=(16, 16),
                         max_rois=2 * prop.topn, trainable=False, seed=2)
    imgs = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, size=(2, 96, 96, 3)).astype(F32)).cuda()
    kw = dict(score_threshold=0.01, max_total_size=50, nms="linear")
    got = [t.clone() for t in prop.detect(imgs, head, **kw)]
    rois, _s, valid, pooled = prop.propose_features(imgs, pooling_size=(3, 3))
    want = head.detect(rois, pooled, prop.hyper_params["variances"], valid=valid, **kw)
    assert len(got) == 4 and int(got[3].sum()) > 0 and all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        prop.detect(imgs, head, nms="soft")
