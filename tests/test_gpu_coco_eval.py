"""GPU suite: the COCO-style device evaluator (rpn_coco_evaluator_*, utils/eval_utils.CocoEvaluator) against the numpy restatement of
tests/coco_eval_ref.py and the hand-made cases of tests/test_coco_eval_host.py.

Flags, npig, ndet and ar (one float64 division of two integers) are compared exactly.  ``ap`` differs from the restatement only in how
the 101 recall points are added -- the device adds pmax * (number of points) per TP in a tree, the restatement the 101 terms in
order: 101 non-negative terms <= 1 in float64 in any order, one multiply per TP group and one division, <= 100 * 2^-53 * 101 / 101
plus the products' roundings.  The bar is 2.5e-14 absolute -- a bound, not a measurement -- and NaN positions must match exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_eval_ref as cr                                                              # noqa: E402
import test_coco_eval_host as ch                                                        # noqa: E402
import test_eval_host as th                                                             # noqa: E402
import test_gpu_eval as tg                                                              # noqa: E402
from oracle import bbox_oracle as bo                                                    # noqa: E402
from tf_rpn_amd import _lib as L                                                        # noqa: E402
from tf_rpn_amd.utils import eval_utils                                                 # noqa: E402

pytestmark = pytest.mark.gpu

AP_TOL = 2.5e-14


def coco(C, max_images, M, **kw):
    return eval_utils.CocoEvaluator(total_labels=C, max_images=max_images, max_detections=M, **kw)


def check_result(got, ref, what=""):
    assert np.array_equal(got["npig"], ref["npig"]) and np.array_equal(got["ndet"], ref["ndet"]), what
    assert got["images"] == ref["images"]
    assert got["ar"].dtype == np.float64 and got["ar"].shape == ref["ar"].shape
    assert np.array_equal(got["ar"], ref["ar"], equal_nan=True), (what, got["ar"], ref["ar"])
    g, r = got["ap"], ref["ap"]
    assert g.dtype == np.float64 and g.shape == r.shape
    assert np.array_equal(np.isnan(g), np.isnan(r)), (what, g, r)
    assert np.isnan(g[0]).all() and np.isnan(got["ar"][0]).all()
    ok = ~np.isnan(r)
    err = np.abs(g[ok] - r[ok])
    print("%s ap max err %.3e over %d entries (bound %.1e)" % (what, err.max() if err.size else 0.0, int(ok.sum()), AP_TOL))
    assert (err <= AP_TOL).all(), (what, g, r)
    s = eval_utils.coco_summaries(r, ref["ar"], got_thresholds(got), got_areas(got), got_cuts(got))
    for key in ("AP", "AP50", "AP75"):
        assert (np.isnan(got[key]) and np.isnan(s[key])) or abs(got[key] - s[key]) <= AP_TOL, (what, key)
    assert np.allclose(got["AR_max_dets"], s["AR_max_dets"], rtol=0, atol=0, equal_nan=True)
    assert np.allclose(got["AR_area"], s["AR_area"], rtol=0, atol=0, equal_nan=True)
    assert np.allclose(got["AP_area"], s["AP_area"], rtol=0, atol=AP_TOL, equal_nan=True)


# the configuration travels with the result in these tests (set by run())
def got_thresholds(got): return got["_cfg"][0]
def got_areas(got): return got["_cfg"][1]
def got_cuts(got): return got["_cfg"][2]


def result_of(ev):
    r = ev.result()
    r["_cfg"] = (ev.iou_thresholds, ev.area_ranges, ev.max_dets)
    return r


def same_bytes(a, b, keys=("ap", "ar", "npig", "ndet")):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


# ---- 1. the hand-made cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ch.HAND_CASES))
def test_hand_made_cases_on_the_device(name):
    make, kw = ch.HAND_CASES[name]
    case = make()
    ref, want, exp = ch.run_ref(name)
    ev = coco(3, case[1].shape[0], ch.M_HAND, image_size=ch.SIZE, **kw)
    got = ev.update(*case, return_flags=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.int8 and got.shape == want.shape
    assert np.array_equal(got, want), (got[..., 0, :], want[..., 0, :])
    r = result_of(ev)
    check_result(r, exp, name)
    if name == "a":
        assert ch.close(r["ap"][1, 0], [51 / 101.0] * 3 + [25.5 / 101.0] * 7)
        assert r["ar"][1, 0].tolist() == [[0.5, 0.5, 0.5]] * 3 + [[0.0, 0.5, 0.5]] * 7
        assert r["stats"] is not None and r["stats"].shape == (12,)
    if name == "b":
        assert got[0, 1, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0] and ch.close(r["ap"][1, 0], [1.0] * 6 + [51 / 101.0] * 4)
    if name == "c":
        assert got[0, 0, 0].tolist() == [1] * 6 + [-1] * 4 and r["npig"][1].tolist() == [1, 0, 0, 1]
    if name == "d":
        assert got[0, 2, :, 0].tolist() == [0, 0, -1, -1] and r["ar"][1, :, 0, :].tolist() == [[0.5, 1, 1], [1, 1, 1], [0.5, 1, 1], [0, 1, 1]]
    if name == "five_detections":
        assert r["stats"] is None and r["ar"][1, 0, 0].tolist() == [1 / 5.0, 2 / 5.0, 2 / 5.0]


# ---- 2. random, tie-rich flags ------------------------------------------------------------------------------------------------
def tie_rich_case(seed, B=8, M=64, G=24, C=5):
    """Every coordinate is a multiple of 1/32: gts with sides of 2, 4, 6, 12 or 9 thirty-seconds (32 and 96 pixels exactly at image
    sizes 512 and 256), some of them copies of another gt; detections are gts shifted by -1, 0 or 1 thirty-seconds per coordinate, so
    that equal IoUs are common; an eighth of them is thrown to a corner where no gt is.  Scores from eight values."""
    rng = np.random.RandomState(seed)
    side = rng.choice([2, 4, 6, 12, 9], size=(B, G, 2))
    org = rng.randint(0, 12, size=(B, G, 2))
    gtb = np.concatenate([org, org + side], axis=2).astype(np.float32) / np.float32(32)
    gtl = rng.choice(np.arange(1, C), p=[0.55, 0.15, 0.15, 0.15], size=(B, G)).astype(np.int32)
    for b in range(B):                                                                   # copies: ties between different gts
        for g in rng.choice(G, size=4, replace=False):
            src = rng.randint(0, G)
            gtb[b, g], gtl[b, g] = gtb[b, src], gtl[b, src]
    gtl[:, -2], gtl[:, -1] = 0, -1
    gtd = (rng.uniform(size=(B, G)) < 1 / 3.0).astype(np.uint8)
    pick = rng.randint(0, G - 2, size=(B, M))
    boxes = np.take_along_axis(gtb, pick[..., None].repeat(4, axis=2), axis=1) + rng.randint(-1, 2, size=(B, M, 4)).astype(np.float32) / np.float32(32)
    far = rng.uniform(size=(B, M)) < 0.125
    boxes[far] = np.array([30, 30, 31, 31], np.float32) / np.float32(32)
    classes = np.take_along_axis(gtl, pick, axis=1).astype(np.float32)
    scores = rng.choice(np.linspace(0.1, 0.9, 8).astype(np.float32), size=(B, M))
    valid = np.resize(np.array([M, 0, 40, M, 17, M, M, 33], np.int32), B)
    gtl[3] = -1                                                                          # an image with label -1 rows only
    classes[0, 5], classes[0, 6], scores[0, 7], scores[0, 8] = 2.5, float(C), np.nan, 0.0
    sizes = rng.choice([256.0, 512.0], size=(B, 2)).astype(np.float32)
    return (np.ascontiguousarray(boxes, np.float32), scores, classes, valid, gtb, gtl, gtd), sizes


TIE_SEED = 1      # chosen on the CPU so that every reason counter of the restatement is >= 1 on this input


def test_tie_rich_flags_are_bit_equal_to_the_restatement():
    case, sizes = tie_rich_case(TIE_SEED)
    kw = dict(max_dets=(1, 5, 20))
    ref = cr.RefCocoEvaluator(5, 64, **kw)
    want = ref.update(*case, image_sizes=sizes)
    assert all(ref.reasons[k] >= 1 for k in cr.REASONS), ref.reasons                    # a condition on the INPUT
    assert (want[1] == -2).all() and (want[2, 40:] == -2).all() and (want[0, 5:9] == -2).all()
    ev = coco(5, 8, 64, **kw)
    got = ev.update(*case, image_sizes=sizes, return_flags=True)
    assert got.shape == (8, 64, 4, 10) and got.dtype == np.int8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])
    ev2 = coco(5, 8, 64, **kw)
    tens = [torch.from_numpy(a).cuda() for a in case]
    got2 = ev2.update(*tens, image_sizes=torch.from_numpy(sizes).cuda(), return_flags=True)
    assert isinstance(got2, torch.Tensor) and got2.is_cuda and got2.dtype == torch.int8 and np.array_equal(got2.cpu().numpy(), want)
    check_result(result_of(ev), ref.result(), "tie rich")


# ---- 3. accumulation ----------------------------------------------------------------------------------------------------------
def accumulation_feed():
    (case, sizes) = tie_rich_case(3, B=12)
    cuts = [(0, 1), (1, 4), (4, 12)]
    return [(tuple(a[i:j] for a in case), sizes[i:j]) for i, j in cuts]


def test_accumulation_over_updates_reset_and_determinism():
    feed = accumulation_feed()
    kw = dict(max_dets=(1, 5, 20))
    ref = cr.RefCocoEvaluator(5, 64, **kw)
    ev, twin = coco(5, 12, 64, **kw), coco(5, 12, 64, **kw)
    for case, sizes in feed:
        want = ref.update(*case, image_sizes=sizes)
        assert np.array_equal(ev.update(*case, image_sizes=sizes, return_flags=True), want)
        twin.update(*case, image_sizes=sizes)
        check_result(result_of(ev), ref.result(), "after %d images" % ref.images)       # result() between updates
    assert ev.images == 12
    got = result_of(ev)
    assert same_bytes(got, ev.result()) and same_bytes(got, twin.result())               # result() changes nothing; two evaluators agree
    ev.reset()
    empty = ev.result()
    assert ev.images == 0 and empty["ndet"].sum() == 0 and empty["npig"].sum() == 0 and np.isnan(empty["AP"])
    for case, sizes in feed:
        assert ev.update(*case, image_sizes=sizes) is None
    assert same_bytes(got, ev.result())


# ---- 4. ranking across images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["eight_values", "bytes", "all_fp", "all_tp"])
def test_ranking_is_the_stable_score_slot_order(kind):
    case = tg.sort_case(kind)
    B = case[1].shape[0]
    kw = dict(iou_thresholds=(0.5, 0.75), area_ranges=((0, 1e10), (0, 150.0 ** 2)), max_dets=(1, 10, 64))
    ref = cr.RefCocoEvaluator(2, 64, **kw)
    ev = coco(2, B, 64, **kw)
    for i in range(0, B, 8):
        part = [a[i:i + 8] if a is not None else None for a in case]
        assert np.array_equal(ev.update(*part, return_flags=True), ref.update(*part))
    got, exp = result_of(ev), ref.result()
    assert exp["ndet"][1] == B * 64
    check_result(got, exp, kind)
    if kind == "all_fp":
        assert (got["ap"][1, 0] == 0.0).all() and (got["ar"][1, 0] == 0.0).all()
    if kind == "all_tp":
        assert ch.close(got["ap"][1, 0], [1.0, 1.0]) and (got["ar"][1, 0, :, 2] == 1.0).all() and got["npig"][1, 0] == 2560
    if kind in ("eight_values", "bytes"):
        assert 0.0 < got["ap"][1, 0, 1] < got["ap"][1, 0, 0] < 1.0


# ---- 5. the wide paths --------------------------------------------------------------------------------------------------------
def test_more_gts_than_lanes_and_a_long_chain():
    rng = np.random.RandomState(7)
    G, M = 136, 1100
    org = rng.randint(0, 24, size=(G, 2))
    side = rng.choice([2, 3, 4, 6], size=(G, 2))
    gtb = (np.concatenate([org, org + side], axis=1).astype(np.float32) / np.float32(32))[None]
    gtl = np.ones((1, G), np.int32)
    gtl[0, 130:] = [2, 2, 0, -1, 2, 2]                                                   # 130 gts of class 1: three strides of the lanes
    gtd = (rng.uniform(size=(1, G)) < 0.2).astype(np.uint8)
    pick = rng.randint(0, G, size=(1, M))
    boxes = gtb[0][pick[0]][None] + rng.randint(-1, 2, size=(1, M, 4)).astype(np.float32) / np.float32(64)
    classes = np.where(rng.uniform(size=(1, M)) < 0.95, 1.0, 2.0).astype(np.float32)
    scores = rng.choice(np.linspace(0.05, 0.95, 64).astype(np.float32), size=(1, M))
    case = (np.ascontiguousarray(boxes, np.float32), scores, classes, np.array([M], np.int32), gtb, gtl, gtd)
    kw = dict(iou_thresholds=(0.5, 0.75), area_ranges=((0, 1e10), (0, 40.0 ** 2)), max_dets=(100, 1100), image_size=(512, 512))
    ref = cr.RefCocoEvaluator(3, M, **kw)
    want = ref.update(*case)
    assert (want[0, :, 0, 0] != -2).all() and (classes == 1.0).sum() > 1024 and ref.reasons["fp_gt_taken"] > 100
    ev = coco(3, 1, M, **kw)
    got = ev.update(*case, return_flags=True)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8])
    check_result(result_of(ev), ref.result(), "wide")


def test_the_limits_g_2048_and_m_4096():
    rng = np.random.RandomState(9)
    G, M = 2048, 4096
    org = rng.randint(0, 28, size=(G, 2))
    gtb = (np.concatenate([org, org + rng.randint(1, 5, size=(G, 2))], axis=1).astype(np.float32) / np.float32(32))[None]
    gtl = np.ones((1, G), np.int32)
    pick = rng.randint(0, G, size=(M,))
    boxes = np.ascontiguousarray(gtb[0][pick][None], np.float32)
    scores = rng.uniform(0.05, 1.0, size=(1, M)).astype(np.float32)
    ev = coco(2, 1, M, iou_thresholds=(0.5,), area_ranges=((0, 1e10),), max_dets=(M,))
    flags = ev.update(boxes, scores, np.ones((1, M), np.float32), np.array([3000], np.int32), gtb, gtl, None, return_flags=True)
    r = ev.result()
    assert (flags[0, 3000:] == -2).all() and (flags[0, :3000] >= 0).all()
    assert r["ndet"].tolist() == [0, 3000] and r["npig"][1, 0] == G
    # the detections are copies of gts: a detection is a TP unless every gt at its place (at IoU 1; a few lie elsewhere) is taken
    assert (flags[0, :3000] == 1).sum() == int(round(r["ar"][1, 0, 0, 0] * G)) > 1000


# ---- 6. image sizes -----------------------------------------------------------------------------------------------------------
def test_default_image_size_and_per_image_sizes():
    case, _sizes = tie_rich_case(5)
    kw = dict(max_dets=(1, 5, 20))
    a, b, c = coco(5, 8, 64, image_size=(256, 512), **kw), coco(5, 8, 64, **kw), coco(5, 8, 64, image_size=(512, 512), **kw)
    fa = a.update(*case, return_flags=True)
    # (this input has a class of 17 to 32 gts in one image: a chain 32 lanes wide, which the other inputs do not have)
    assert any(17 <= int((case[5][b] == c).sum()) <= 32 and (case[2][b, :case[3][b]] == c).any() for b in range(8) for c in range(1, 5))
    assert np.array_equal(fa, cr.RefCocoEvaluator(5, 64, image_size=(256, 512), **kw).update(*case))
    fb = b.update(*case, image_sizes=np.tile(np.array([[256, 512]], np.float32), (8, 1)), return_flags=True)
    fc = c.update(*case, return_flags=True)
    assert fa.tobytes() == fb.tobytes() and same_bytes(a.result(), b.result())
    assert np.array_equal(fa[:, :, 0], fc[:, :, 0])                                      # [0, 1e10] holds every box at either size
    assert not np.array_equal(fa[:, :, 1:], fc[:, :, 1:])
    ra, rc = a.result(), c.result()
    assert np.array_equal(ra["npig"][:, 0], rc["npig"][:, 0]) and not np.array_equal(ra["npig"][:, 1:], rc["npig"][:, 1:])
    assert ra["ap"][:, 0].tobytes() == rc["ap"][:, 0].tobytes()


# ---- 7. against the VOC evaluator ---------------------------------------------------------------------------------------------
def test_agrees_with_the_voc_evaluator_where_the_rules_coincide():
    """Gts on a grid of cells that do not touch; every detection is a shrunken copy of one cell (its own shrink, so no two IoUs are
    equal) or lies in an empty cell: it overlaps at most one gt.  Then the best gt and the best untaken gt differ only when the best
    is taken, where both rules say FP."""
    rng = np.random.RandomState(21)
    B, M, G, C = 4, 48, 12, 4
    cells = np.array([[0.25 * i, 0.25 * j, 0.25 * i + 0.2, 0.25 * j + 0.2] for i in range(4) for j in range(4)], np.float32)
    where = np.stack([rng.permutation(16)[:G] for _ in range(B)])                        # the cell of every gt
    gtb = cells[where]
    gtl = rng.randint(1, C, size=(B, G)).astype(np.int32)
    gtl[:, -1] = -1
    pick = rng.randint(0, 16, size=(B, M))
    shrink = (1 + np.arange(B * M).reshape(B, M, 1)) * np.float32(0.0002) * np.array([1, 1, -1, -1], np.float32)
    boxes = np.ascontiguousarray(cells[pick] + shrink, np.float32)
    classes = rng.randint(1, C, size=(B, M)).astype(np.float32)
    for b in range(B):                                                                   # three in four take the class of the gt in their cell
        for m in range(M):
            g = np.flatnonzero(where[b] == pick[b, m])
            if g.size and gtl[b, g[0]] >= 1 and rng.uniform() < 0.75:
                classes[b, m] = gtl[b, g[0]]
    scores = rng.choice(np.linspace(0.1, 0.9, 8).astype(np.float32), size=(B, M))
    valid = np.array([M, 30, M, 0], np.int32)
    for b in range(B):
        iou = bo.generate_iou_map(boxes[b][None], gtb[b][None])[0]
        assert ((iou > 0).sum(axis=1) <= 1).all() and len(np.unique(iou[iou > 0])) == (iou > 0).sum()
    voc = eval_utils.DetectionEvaluator(total_labels=C, max_images=B, max_detections=M, iou_threshold=0.5, top_k=(), recall_iou=())
    want = voc.update(boxes, scores, classes, valid, gtb, gtl, None)
    ev = coco(C, B, M, iou_thresholds=(0.5,), area_ranges=((0, 1e10),), max_dets=(M,))
    got = ev.update(boxes, scores, classes, valid, gtb, gtl, None, return_flags=True)[:, :, 0, 0]
    live = want >= 0
    assert live.sum() > 100 and (want[live] == 1).sum() > 20 and (want[live] == 0).sum() > 20
    assert np.array_equal(got[live], want[live]) and (got[~live] == -2).all()
    rv, rc = voc.result(), ev.result()
    assert np.array_equal(rv["npos"], rc["npig"][:, 0]) and np.array_equal(rv["ndet"], rc["ndet"])


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_evaluator_unchanged():
    feed = accumulation_feed()
    kw = dict(max_dets=(1, 5, 20))
    ev = coco(5, 5, 64, **kw)
    ev.update(*feed[0][0], image_sizes=feed[0][1])
    ev.update(*feed[1][0], image_sizes=feed[1][1])
    before = ev.result()
    with pytest.raises(ValueError):
        ev.update(*feed[2][0])                                                           # 4 + 8 > max_images
    with pytest.raises(ValueError):
        ev.update(*[a[:, :63] if a.ndim > 1 and a.shape[1] == 64 else a for a in feed[0][0]])      # M mismatch
    with pytest.raises(ValueError):
        ev.update(*feed[0][0], image_sizes=np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        ev.update(*feed[0][0], image_sizes=np.zeros((2, 2), np.float32))
    after = ev.result()
    assert ev.images == 4 and same_bytes(before, after)
    # the C entry point itself refuses as well, before anything is enqueued
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in feed[2][0]]
    st = L.lib().rpn_coco_evaluator_update(ev._h, L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(t[3]), L.ptr(t[4]), L.ptr(t[5]),
                                           L.ptr(t[6]), None, 8, 24, None, L.stream_ptr())
    assert st == L.RPN_ERR_INVALID and ev.images == 4
    assert same_bytes(before, ev.result())


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------
def test_evaluate_feeds_a_tuple_of_evaluators():
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
    ckw = dict(iou_thresholds=(0.1, 0.3, 0.5), max_dets=(1, 10, 60), image_size=(96, 96))
    ref, cref = th.RefEvaluator(4, M, top_k=top_k, recall_iou=thr), cr.RefCocoEvaluator(4, M, **ckw)
    for imgs, gtb, gtl, gtd in feed:                                                     # the detect outputs, copied to the host
        rois, _s, valid, pooled = prop.propose_features(torch.from_numpy(imgs).cuda(), pooling_size=head.pooling_size)
        ref.update_proposals(rois.cpu().numpy(), valid.cpu().numpy(), gtb, gtl, gtd)
        boxes, scores, classes, n = head.detect(rois, pooled, hp["variances"], valid=valid, max_total_size=M, **kw)
        args = (boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy(), n.cpu().numpy(), gtb, gtl, gtd)
        ref.update(*args)
        cref.update(*args)
    assert int(cref.result()["ndet"].sum()) >= 10
    voc_ev = tg.evaluator(4, 4, M, top_k=top_k, recall_iou=thr)
    coco_ev = coco(4, 4, M, **ckw)
    out = eval_utils.evaluate(prop, head, feed, 2, (voc_ev, coco_ev), **kw)
    assert isinstance(out, list) and len(out) == 2
    tg.check_result(out[0], ref.result(), "end to end, voc")
    assert out[0]["recall"].tobytes() == ref.result()["recall"].tobytes()
    out[1]["_cfg"] = (coco_ev.iou_thresholds, coco_ev.area_ranges, coco_ev.max_dets)
    check_result(out[1], cref.result(), "end to end, coco")
    assert out[1]["images"] == 4
    # a CocoEvaluator alone (it has no update_proposals), and a list
    coco_ev.reset()
    alone = eval_utils.evaluate(prop, head, feed, 2, coco_ev, **kw)
    assert isinstance(alone, dict) and same_bytes(alone, out[1])
