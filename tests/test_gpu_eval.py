"""GPU suite: the device evaluator (rpn_evaluator_*, utils/eval_utils.py) against the numpy restatement of tests/test_eval_host.py.

Flags, counts, ranking order and the 11-point sum's inputs are integers or exactly rounded float64 quotients on both sides and are
compared exactly.  ``ap`` and ``ap_11pt`` differ from the restatement only in the order of one float64 sum of at most npos terms in
[0, 1] (and 11 terms for the 11-point form, added in the same order on both sides): the bar is npos * 2^-52 absolute -- a bound,
not a measurement -- and NaN positions must match exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_eval_host as th                                                             # noqa: E402
from oracle import bbox_oracle as bo                                                    # noqa: E402
from tf_rpn_amd.utils import eval_utils                                                 # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def jittered_batch(rng, B, M, G, C, valid, noise=0.03, far=0.15):
    """Detections made by jittering gt rows, so that several claim the same gt; a share of them is thrown far away."""
    gt_boxes = np.zeros((B, G, 4), np.float32)
    y1, x1 = rng.uniform(0.0, 0.6, size=(B, G)), rng.uniform(0.0, 0.6, size=(B, G))
    gt_boxes[..., 0], gt_boxes[..., 1] = y1, x1
    gt_boxes[..., 2], gt_boxes[..., 3] = y1 + rng.uniform(0.15, 0.4, size=(B, G)), x1 + rng.uniform(0.15, 0.4, size=(B, G))
    gt_labels = rng.randint(1, C, size=(B, G)).astype(np.int32)
    gt_diff = (rng.uniform(size=(B, G)) < 0.25).astype(np.uint8)
    pick = rng.randint(0, G, size=(B, M))
    boxes = np.take_along_axis(gt_boxes, pick[..., None].repeat(4, axis=2), axis=1) + rng.normal(0, noise, size=(B, M, 4)).astype(np.float32)
    lost = rng.uniform(size=(B, M)) < far
    boxes[lost] = boxes[lost] * np.float32(0.2) + np.float32(0.8)
    classes = np.take_along_axis(gt_labels, pick, axis=1).astype(np.float32)
    wrong = rng.uniform(size=(B, M)) < 0.1
    classes[wrong] = rng.randint(1, C, size=int(wrong.sum()))
    scores = rng.uniform(0.05, 1.0, size=(B, M)).astype(np.float32)
    return (np.ascontiguousarray(boxes, np.float32), scores, classes, np.asarray(valid, np.int32), gt_boxes, gt_labels, gt_diff)


def flags_case(seed=0):
    """B = 3, M = 37, G = 5, C = 4: valid {0, 37, 12}; gt padding (-1) and background (0) rows; difficult gts; dropped rows of every
    kind (class 0, class C, fractional class, score 0 / NaN / inf) among the live rows of image 1."""
    rng = np.random.RandomState(seed)
    boxes, scores, classes, valid, gtb, gtl, gtd = jittered_batch(rng, 3, 37, 5, 4, [0, 37, 12])
    gtl[:, 3], gtl[:, 4] = -1, 0
    gtl[0, 0] = -1
    classes[1, 0], classes[1, 1], classes[1, 2] = 0.0, 4.0, 1.5
    scores[1, 3], scores[1, 4], scores[1, 5] = 0.0, np.nan, np.inf
    classes[2, 1], scores[2, 2] = -1.0, -0.5
    return boxes, scores, classes, valid, gtb, gtl, gtd


def evaluator(C, max_images, M, **kw):
    kw.setdefault("top_k", (1, 8))
    kw.setdefault("recall_iou", (0.5,))
    return eval_utils.DetectionEvaluator(total_labels=C, max_images=max_images, max_detections=M, **kw)


def check_result(got, ref, what=""):
    assert np.array_equal(got["npos"], ref["npos"]) and np.array_equal(got["ndet"], ref["ndet"]), what
    assert got["images"] == ref["images"]
    for key in ("ap", "ap_11pt"):
        g, r = got[key], ref[key]
        assert g.dtype == np.float64 and g.shape == r.shape
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, key, g, r)
        assert np.isnan(g[0])
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        bound = ref["npos"][ok] * EPS
        print("%s %-8s max err %.3e  (bound: npos * 2^-52, smallest %.3e)  classes %d" % (what, key, err.max() if err.size else 0.0,
                                                                                       bound.min() if bound.size else 0.0, int(ok.sum())))
        assert (err <= bound).all(), (what, key, g, r)
    for key in ("mAP", "mAP_11pt"):
        assert (np.isnan(got[key]) and np.isnan(ref[key])) or abs(got[key] - ref[key]) <= max(ref["npos"].max(), 1) * EPS, (what, key)


def check_curves(ev, ref, C):
    for c in range(1, C):
        gs, gtp, gslot = ev.pr_curve(c)
        rs, rtp, rslot = ref.pr_curve(c)
        assert np.array_equal(gslot, rslot), c
        assert np.array_equal(gtp, rtp) and np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), c


# ---- flags --------------------------------------------------------------------------------------------------------------------
def test_flags_are_bit_equal_to_the_restatement():
    case = flags_case()
    ref = th.RefEvaluator(4, 37)
    want = ref.update(*case)
    # conditions on the INPUT (the seed was picked on the CPU so that they hold): one of each outcome at least
    assert all(ref.reasons[k] >= 1 for k in ("tp", "duplicate", "ignored", "miss")), ref.reasons
    assert (want[0] == -1).all() and (want[2, 12:] == -1).all() and (want[1, :6] == -1).all() and (want[2, 1:3] == -1).all()
    ev = evaluator(4, 3, 37)
    got = ev.update(*case)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    ev2 = evaluator(4, 6, 37)
    tens = [torch.from_numpy(a).cuda() for a in case]
    got2 = ev2.update(*tens)
    assert isinstance(got2, torch.Tensor) and got2.is_cuda and np.array_equal(got2.cpu().numpy(), want)
    assert np.array_equal(ev2.update(*case), want)                                       # a second batch: the same flags
    check_result(ev.result(), ref.result(), "flags")
    check_curves(ev, ref, 4)


@pytest.mark.parametrize("name", ["required", "iou_equal_to_threshold", "equal_iou_two_gts", "equal_scores", "recall_three_tenths"])
def test_hand_made_cases_on_the_device(name):
    case = getattr(th, "case_" + name)()
    M = case[1].shape[1]
    ref = th.RefEvaluator(5, M)
    want = ref.update(*case)
    ev = evaluator(5, 1, M)
    assert np.array_equal(ev.update(*case), want)
    got, exp = ev.result(), ref.result()
    check_result(got, exp, name)
    if name == "required":
        assert want.tolist() == [[1, 0, -1, 0, 1]] and got["ap"][1] == 0.75 and got["ap_11pt"][1] == 8.5 / 11
    if name == "recall_three_tenths":
        assert got["ap_11pt"][1] == 4.0 / 11 and got["ap"][2] == 0.0 and np.isnan(got["ap"][3])
    check_curves(ev, ref, 5)


# ---- accumulation -------------------------------------------------------------------------------------------------------------
def accumulation_batches():
    rng = np.random.RandomState(5)
    out = []
    for B, G in ((1, 5), (3, 3), (2, 7)):
        out.append(jittered_batch(rng, B, 37, G, 4, rng.randint(0, 38, size=B)))
    out[1][5][1, :] = -1                                                                 # an image without gts
    return out


def test_accumulation_over_updates_and_reset():
    batches = accumulation_batches()
    ref = th.RefEvaluator(4, 37)
    ev = evaluator(4, 6, 37)
    for case in batches:
        want = ref.update(*case)
        assert np.array_equal(ev.update(*case), want)
    assert ev.images == 6
    exp, got = ref.result(), ev.result()
    assert sum(exp["ndet"]) >= 40 and (exp["npos"][1:] > 0).all()
    check_result(got, exp, "accumulate")
    check_curves(ev, ref, 4)
    again = ev.result()                                                                  # result() changes nothing
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got)
    curves = [ev.pr_curve(c) for c in range(1, 4)]
    ev.reset()
    assert ev.images == 0 and ev.result()["ndet"].sum() == 0 and np.isnan(ev.result()["mAP"])
    for case in batches:
        ev.update(*case, return_flags=False)
    after = ev.result()
    assert all(np.asarray(got[k]).tobytes() == np.asarray(after[k]).tobytes() for k in got)
    for c in range(1, 4):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(curves[c - 1], ev.pr_curve(c)))


# ---- the sort -----------------------------------------------------------------------------------------------------------------
def sort_scores(kind, rng, shape):
    if kind == "eight_values":
        return rng.choice(np.linspace(0.1, 0.9, 8).astype(np.float32), size=shape)
    n = int(np.prod(shape))
    low = np.uint32(0x3F000000) | rng.randint(0, 256, size=n).astype(np.uint32)          # differ in the lowest byte only
    high = (rng.randint(0, 0x7F, size=n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00400000)   # in the highest only (0: a denormal)
    den = rng.randint(1, 0x00800000, size=n).astype(np.uint32)                           # denormals
    mid = rng.randint(0x3E000000, 0x3F800000, size=n).astype(np.uint32)                  # every byte varies
    which = rng.randint(0, 4, size=n)
    bits = np.choose(which, [low, high, den, mid]).astype(np.uint32)
    s = bits.view(np.float32).reshape(shape)
    assert np.isfinite(s).all() and (s > 0).all()
    return s


def sort_case(kind, B=40):
    """one class, 40 images x M = 64 = 2560 records: more than one pass of the workgroup's 1024 threads over the keys; "bytes_long"
    is 88 images = 5632 records, about 4500 of them live: they do not fit one 4096-key tile of a sort pass either"""
    rng = np.random.RandomState(11)
    M = 64
    if kind == "bytes_long":
        kind, B = "bytes", 88
    if kind == "all_tp":                                                                 # every detection sits on a gt of its own
        cells = np.array([[0.125 * i, 0.125 * j, 0.125 * i + 0.1, 0.125 * j + 0.1] for i in range(8) for j in range(8)], np.float32)
        gtb = np.broadcast_to(cells, (B, 64, 4)).copy()
        case = (gtb.copy(), sort_scores("bytes", rng, (B, M)), np.ones((B, M), np.float32), np.full((B,), M, np.int32), gtb,
                np.ones((B, 64), np.int32), None)
        return case
    boxes, scores, classes, valid, gtb, gtl, gtd = jittered_batch(rng, B, M, 8, 2, [M] * B)
    scores = sort_scores("eight_values" if kind == "eight_values" else "bytes", rng, (B, M))
    if kind == "all_fp":
        gtb = gtb * np.float32(0.01)                                                     # the gts are somewhere else
        gtd[:] = 0
    return boxes, scores, classes, valid, gtb, gtl, gtd


@pytest.mark.parametrize("kind", ["eight_values", "bytes", "all_fp", "all_tp", "bytes_long"])
def test_ranking_is_a_stable_sort_by_score(kind):
    case = sort_case(kind)
    B = case[1].shape[0]
    ref = th.RefEvaluator(2, 64)
    ev = evaluator(2, B, 64)
    # in updates of eight images, as a loop over a feed would
    flags = np.concatenate([ref.update(*[a[i:i + 8] if a is not None else None for a in case]) for i in range(0, B, 8)])
    got_flags = np.concatenate([ev.update(*[a[i:i + 8] if a is not None else None for a in case]) for i in range(0, B, 8)])
    assert np.array_equal(got_flags, flags)
    if kind == "all_fp":
        assert (flags == 0).all()
    elif kind == "all_tp":
        assert (flags == 1).all()
    else:
        assert (flags == 1).sum() > 100 and (flags == 0).sum() > 100
    scores, tp, slots = ev.pr_curve(1)
    live = np.flatnonzero(flags.reshape(-1) >= 0)
    s = case[1].reshape(-1)[live]
    order = live[np.lexsort((live, -s.astype(np.float64)))]
    assert len(slots) == len(live) >= (4200 if kind == "bytes_long" else 1900)
    assert np.array_equal(slots, order)
    assert np.array_equal(scores.view(np.uint32), case[1].reshape(-1)[order].view(np.uint32))
    assert np.array_equal(tp, flags.reshape(-1)[order])
    if kind == "eight_values":
        assert len(np.unique(scores)) == 8
    got, exp = ev.result(), ref.result()
    check_result(got, exp, kind)
    if kind == "all_fp":
        assert got["ap"][1] == 0.0 and got["ap_11pt"][1] == 0.0
    if kind == "all_tp":
        assert got["ap"][1] == 1.0 and got["ap_11pt"][1] == 1.0 and got["npos"][1] == 2560


# ---- proposal recall --------------------------------------------------------------------------------------------------------
def recall_case(seed, valid, no_gt_image=None):
    rng = np.random.RandomState(seed)
    B, R, G = 2, 70, 6
    _b, _s, _c, _v, gtb, gtl, gtd = jittered_batch(rng, B, 1, G, 4, [1] * B)
    pick = rng.randint(0, G, size=(B, R))
    noise = rng.choice([0.01, 0.04, 0.08], size=(B, R, 1)).astype(np.float32)
    rois = np.take_along_axis(gtb, pick[..., None].repeat(4, axis=2), axis=1) + rng.normal(0, 1, size=(B, R, 4)).astype(np.float32) * noise
    gtl[:, 4], gtl[:, 5] = 0, -1
    if no_gt_image is not None:
        gtl[no_gt_image] = np.where(gtd[no_gt_image] != 0, gtl[no_gt_image], -1)         # only difficult ones are left
    return np.ascontiguousarray(rois, np.float32), np.asarray(valid, np.int32), gtb, gtl, gtd


def test_proposal_recall_hits_are_integer_equal():
    top_k, thr = (1, 8, 64, 300), (0.5, 0.7)
    ref = th.RefEvaluator(4, 1, top_k=top_k, recall_iou=thr)
    ev = evaluator(4, 1, 1, top_k=top_k, recall_iou=thr)
    first = recall_case(3, [70, 9])                                                     # k = 300 > valid = 70 = R, k = 64 > valid = 9
    ref.update_proposals(*first)
    ev.update_proposals(*first)
    r1 = ev.result()
    assert r1["n_gt"] == ref.n_gt >= 4 and r1["recall"].tobytes() == ref.result()["recall"].tobytes()
    assert np.array_equal(np.rint(r1["recall"] * r1["n_gt"]).astype(np.int64), ref.hits)
    # the cut-offs and the thresholds all matter in this case
    assert ref.hits[0, 0] < ref.hits[1, 0] < ref.hits[2, 0] and ref.hits[2, 0] == ref.hits[3, 0] and ref.hits[2, 1] < ref.hits[2, 0]
    second = recall_case(2, [70, 33], no_gt_image=1)
    before = ref.n_gt
    ref.update_proposals(*[a[1:] for a in second])
    assert ref.n_gt == before                                                            # (the image has no counted gt)
    ref.update_proposals(*[a[:1] for a in second])
    ev.update_proposals(*[torch.from_numpy(a).cuda() for a in second])
    r2, exp = ev.result(), ref.result()
    assert r2["n_gt"] == exp["n_gt"] > before and r2["recall"].tobytes() == exp["recall"].tobytes()
    ev3 = evaluator(4, 1, 1, top_k=(300, 1, 64, 8), recall_iou=(0.7, 0.5))               # the caller's order of rows and columns
    ev3.update_proposals(*first)
    assert np.array_equal(ev3.result()["recall"], r1["recall"][[3, 0, 2, 1]][:, ::-1])
    assert np.isnan(evaluator(4, 1, 1).result()["recall"]).all()
    ev4 = evaluator(4, 1, 1, top_k=top_k, recall_iou=thr)
    ev4.update_proposals(first[0], None, *first[2:])                                     # no valid: every row is live
    ref4 = th.RefEvaluator(4, 1, top_k=top_k, recall_iou=thr)
    ref4.update_proposals(first[0], None, *first[2:])
    assert ev4.result()["recall"].tobytes() == ref4.result()["recall"].tobytes()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_evaluator_unchanged():
    batches = accumulation_batches()
    ev = evaluator(4, 4, 37)
    ev.update(*batches[0])
    ev.update(*batches[1])
    before = ev.result()
    with pytest.raises(ValueError):
        ev.update(*batches[2])                                                           # 4 + 2 > max_images
    with pytest.raises(ValueError):
        ev.update(*[a[:, :36] if a.ndim > 1 and a.shape[1] == 37 else a for a in batches[0]])     # M mismatch
    with pytest.raises(ValueError):
        ev.update(*(batches[0][:4] + (np.zeros((1, 2049, 4), np.float32), np.zeros((1, 2049), np.int32))))
    with pytest.raises(ValueError):
        evaluator(4, 4, 37, recall_iou=(0.5,) * 9)
    after = ev.result()
    assert ev.images == 4 and all(np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes() for k in before)
    # the C entry point itself refuses as well, before anything is enqueued
    from tf_rpn_amd import _lib as L
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batches[2]]
    st = L.lib().rpn_evaluator_update(ev._h, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), L.ptr(t[5]), L.ptr(t[6]), 2,
                                      7, None, L.stream_ptr())
    assert st == L.RPN_ERR_INVALID and ev.images == 4
    final = ev.result()
    assert all(np.asarray(before[k]).tobytes() == np.asarray(final[k]).tobytes() for k in before)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_evaluate_end_to_end_against_the_restatement():
    from tf_rpn_amd.models import DetectionHead
    from tf_rpn_amd.models._rpn_model import synthetic_weights
    from tf_rpn_amd.predictor import Proposer
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    prop = Proposer("vgg16", hyper_params=dict(hp), weights=synthetic_weights("vgg16", hp, seed=1), precision="f32", max_batch=2)
    head = DetectionHead(4, pooling_size=(7, 7), channels=512, hidden=(64, 64), max_rois=2 * prop.topn, trainable=False, seed=2)
    rng = np.random.RandomState(0)
    M, top_k, thr = 60, (1, 10, 300), (0.3, 0.5)
    feed = []
    for _ in range(2):
        imgs = rng.uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)
        gtb = np.array([[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.5, 0.5], [0.4, 0.4, 1.0, 1.0], [0.2, 0.1, 0.7, 0.9], [0, 0, 0, 0]]] * 2, np.float32)
        gtb[:, :4] += rng.uniform(-0.03, 0.03, size=(2, 4, 4)).astype(np.float32)
        gtl = np.array([[1, 2, 3, 1, -1], [2, 3, 1, 2, -1]], np.int32)
        gtd = np.array([[0, 0, 0, 1, 0], [0, 1, 0, 0, 0]], np.uint8)
        feed.append((imgs, gtb, gtl, gtd))
    kw = dict(score_threshold=0.05, max_output_size_per_class=30)
    ref = th.RefEvaluator(4, M, top_k=top_k, recall_iou=thr)
    for imgs, gtb, gtl, gtd in feed:                                                     # the detect outputs, copied to the host
        rois, _s, valid, pooled = prop.propose_features(torch.from_numpy(imgs).cuda(), pooling_size=head.pooling_size)
        ref.update_proposals(rois.cpu().numpy(), valid.cpu().numpy(), gtb, gtl, gtd)
        boxes, scores, classes, n = head.detect(rois, pooled, hp["variances"], valid=valid, max_total_size=M, **kw)
        ref.update(boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), n.cpu().numpy(), gtb, gtl, gtd)
    exp = ref.result()
    assert int(exp["ndet"].sum()) >= 10, exp["ndet"]                                     # live records: the threshold is low enough
    ev = evaluator(4, 4, M, top_k=top_k, recall_iou=thr)
    got = eval_utils.evaluate(prop, head, feed, 2, ev, **kw)
    check_result(got, exp, "end to end")
    assert got["images"] == 4 and got["n_gt"] == exp["n_gt"] == 12
    assert got["recall"].tobytes() == exp["recall"].tobytes()
    check_curves(ev, ref, 4)
