"""CPU suite: the COCO-style metric's numpy restatement (tests/coco_eval_ref.py) pinned by hand-made cases IN NUMBERS, and the C-ABI
boundary of rpn_coco_evaluator_* (no compute calls without a GPU).  tests/test_gpu_coco_eval.py runs the same cases on the device.

The pinned APs are sums of 101 precisions tp / (tp + fp + 2^-52): a precision of "1" is 1 / (1 + 2^-52), so the APs are compared
with 1e-14 absolute (101 terms, each within 2.3e-16 of the stated fraction), everything else exactly."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_eval_ref as cr                                                              # noqa: E402
import test_eval_host as th                                                             # noqa: E402
import __graft_entry__ as entry                                                         # noqa: E402
from tf_rpn_amd import _lib as L                                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COCO_SYMBOLS = ["rpn_coco_evaluator_create", "rpn_coco_evaluator_destroy", "rpn_coco_evaluator_memory_bytes",
                "rpn_coco_evaluator_reset", "rpn_coco_evaluator_images", "rpn_coco_evaluator_update", "rpn_coco_evaluator_result"]
SIZE = (512, 512)
M_HAND = 100               # the smallest M that the default max_dets = (1, 10, 100) admits
G1 = [0.0, 0.25, 0.5, 0.75]
TOL = 1e-14


# ---- hand-made cases: name -> (batch of one image, M = M_HAND) ------------------------------------------------------------------
def case_a():
    """a tie to the last gt"""
    return th._img([([0.0, 0.125, 0.5, 0.625], 0.9, 1), (G1, 0.8, 1)], [([0.0, 0.0, 0.5, 0.5], 1, 0), (G1, 1, 0)], M=M_HAND)


def case_b():
    """the best gt is taken, the second best still matches"""
    return th._img([(G1, 0.9, 1), ([0.0, 0.1875, 0.5, 0.6875], 0.8, 1)], [([0.0, 0.125, 0.5, 0.625], 1, 0), (G1, 1, 0)], M=M_HAND)


def case_c():
    """difficult gts"""
    return th._img([(G1, 0.9, 1), (G1, 0.8, 1), (G1, 0.7, 1)], [([0.0, 0.1875, 0.5, 0.6875], 1, 0), (G1, 1, 1)], M=M_HAND)


S32, S96 = [0.0, 0.0, 0.0625, 0.0625], [0.5, 0.5, 0.6875, 0.6875]


def case_d():
    """areas: a gt of exactly 32^2 and one of exactly 96^2 pixels"""
    return th._img([(S32, 0.9, 1), (S96, 0.8, 1), ([0.9, 0.9, 0.92, 0.92], 0.7, 1)], [(S32, 1, 0), (S96, 1, 0)], M=M_HAND)


def case_no_detections():
    """class 1: a gt and no detection; class 2: a detection and a gt"""
    return th._img([(G1, 0.9, 2)], [(G1, 1, 0), (G1, 2, 0)], M=M_HAND)


def case_dropped_rows():
    """row 0 is live; the others are dropped: class 2.5, score 0 / NaN / inf, class 0, class C; row 7 and the rows after it are beyond valid"""
    dets = [(G1, 0.9, 1), (G1, 0.8, 2.5), (G1, 0.0, 1), (G1, np.nan, 1), (G1, np.inf, 1), (G1, 0.5, 0), (G1, 0.5, 3), (G1, 0.5, 1)]
    case = list(th._img(dets, [(G1, 1, 0)], M=M_HAND))
    case[3] = np.array([7], np.int32)
    return tuple(case)


def case_five_detections():
    """five detections on five gts in a row; the scores fall; the third is off its gt.  max_dets = (1, 2, 3) sees ranks 0, 1, 2 only"""
    cells = [[0.0, 0.2 * i, 0.5, 0.2 * i + 0.15] for i in range(5)]
    dets = [(cells[i], 0.9 - 0.1 * i, 1) for i in range(5)]
    dets[2] = ([0.6, 0.0, 0.9, 0.1], 0.7, 1)
    return th._img(dets, [(c, 1, 0) for c in cells], M=M_HAND)


def case_quarter_recalls():
    """npig = 4; ranking TP, FP, TP, FP: recall is exactly .25 at rank 0 and exactly .5 at rank 2"""
    cells = [[0.0, 0.25 * i, 0.5, 0.25 * i + 0.2] for i in range(4)]
    miss = [0.6, 0.0, 0.9, 0.1]
    return th._img([(cells[0], 0.9, 1), (miss, 0.8, 1), (cells[1], 0.7, 1), (miss, 0.6, 1)], [(c, 1, 0) for c in cells], M=M_HAND)


def case_equal_scores_two_images():
    """two images, one detection each at the same score: image 0's misses, image 1's hits.  The lower slot ranks first."""
    one = th._img([([0.6, 0.0, 0.9, 0.1], 0.5, 1)], [(G1, 1, 0)], M=M_HAND)
    two = th._img([(G1, 0.5, 1)], [(G1, 1, 0)], M=M_HAND)
    return tuple(np.concatenate([x, y]) for x, y in zip(one, two))


HAND_CASES = {"a": (case_a, {}), "b": (case_b, {}), "c": (case_c, {}), "d": (case_d, {}), "no_detections": (case_no_detections, {}),
              "dropped_rows": (case_dropped_rows, {}), "five_detections": (case_five_detections, {"max_dets": (1, 2, 3)}),
              "quarter_recalls": (case_quarter_recalls, {}), "equal_scores_two_images": (case_equal_scores_two_images, {})}


def run_ref(name, C=3):
    make, kw = HAND_CASES[name]
    ref = cr.RefCocoEvaluator(C, M_HAND, image_size=SIZE, **kw)
    flags = ref.update(*make())
    return ref, flags, ref.result()


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and bool((np.abs(got - want)[~np.isnan(want)] <= TOL).all())


def test_case_a_a_tie_goes_to_the_last_gt():
    case = case_a()
    iou = cr.bo.generate_iou_map(case[0][0][None], case[4][0][None])[0]
    assert iou[0, 0] == iou[0, 1] >= np.float32(0.6)
    ref, flags, r = run_ref("a")
    assert flags[0, 0, 0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0] and flags[0, 1, 0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert (flags[0, 2:] == -2).all() and ref.reasons["tie_last"] >= 1
    assert close(r["ap"][1, 0], [51 / 101.0] * 3 + [25.5 / 101.0] * 7)
    assert r["ar"][1, 0].tolist() == [[0.5, 0.5, 0.5]] * 3 + [[0.0, 0.5, 0.5]] * 7
    assert r["npig"][1].tolist() == [2, 0, 0, 2] and r["ndet"].tolist() == [0, 2, 0]
    assert np.isnan(r["ap"][1, 1]).all() and np.isnan(r["ap"][0]).all() and np.isnan(r["ap"][2]).all()    # no small gt; class 0; no gt


def test_case_b_the_second_best_gt_still_matches():
    ref, flags, r = run_ref("b")
    assert (flags[0, 0, 0] == 1).all() and flags[0, 1, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert ref.reasons["tp_second_choice"] >= 1
    assert close(r["ap"][1, 0], [1.0] * 6 + [51 / 101.0] * 4)


def test_case_c_difficult_gts():
    ref, flags, r = run_ref("c")
    assert flags[0, 0, 0].tolist() == [1] * 6 + [-1] * 4          # the non-ignored gt at IoU 7/9 before the difficult one at 1.0
    assert flags[0, 1, 0].tolist() == [-1] * 6 + [0] * 4          # the difficult gt matches once only
    assert (flags[0, 2, 0] == 0).all()
    assert r["npig"][1].tolist() == [1, 0, 0, 1]
    assert close(r["ap"][1, 0], [1.0] * 6 + [0.0] * 4)
    assert ref.reasons["ignored_gt"] >= 1 and ref.reasons["fp_gt_taken"] >= 1


def test_case_d_area_ranges_are_inclusive_at_both_ends():
    case = case_d()
    assert cr.pixel_area(case[4][0, 0], 512, 512) == 1024.0 and cr.pixel_area(case[4][0, 1], 512, 512) == 9216.0
    ref, flags, r = run_ref("d")
    assert flags[0, 0, :, 0].tolist() == [1, 1, 1, -1] and flags[0, 1, :, 0].tolist() == [1, -1, 1, 1]
    assert flags[0, 2, :, 0].tolist() == [0, 0, -1, -1]
    assert r["npig"][1].tolist() == [2, 1, 2, 1]
    assert r["ar"][1, :, 0, :].tolist() == [[0.5, 1, 1], [1, 1, 1], [0.5, 1, 1], [0, 1, 1]]
    assert close(r["ap"][1, :, 0], [1.0] * 4)
    assert ref.reasons["ignored_area"] >= 1


def test_equal_scores_in_two_images_rank_by_slot():
    ref, flags, r = run_ref("equal_scores_two_images")
    assert flags[0, 0, 0, 0] == 0 and flags[1, 0, 0, 0] == 1
    assert [row[2] for row in ref.ranking(1)] == [0, M_HAND]
    # FP then TP: precision 0, 1/2 -> 1/2 at the recall points up to 1/2 (the other order would give 51 points of 1); both rows have
    # rank 0 in their image
    assert close(r["ap"][1, 0, 0], 25.5 / 101.0) and r["ar"][1, 0, 0].tolist() == [0.5, 0.5, 0.5] and r["npig"][1, 0] == 2


def test_no_detections_is_zero_and_no_gts_in_an_area_is_nan():
    _ref, _flags, r = run_ref("no_detections")
    assert (r["ap"][1, 0] == 0.0).all() and (r["ar"][1, 0] == 0.0).all() and (r["ap"][1, 3] == 0.0).all()
    assert np.isnan(r["ap"][1, 1]).all() and np.isnan(r["ar"][1, 2]).all()             # every gt is outside small and medium
    assert close(r["ap"][2, 0], [1.0] * 10) and r["ndet"].tolist() == [0, 0, 1]


def test_dropped_rows_get_minus_two_and_no_record():
    ref, flags, r = run_ref("dropped_rows")
    assert (flags[0, 0, 0] == 1).all() and (flags[0, 1:] == -2).all()
    assert len(ref.records) == 1 and r["ndet"].tolist() == [0, 1, 0]


def test_max_dets_cuts_before_the_chain():
    ref, flags, r = run_ref("five_detections")
    assert flags[0, :5, 0, 0].tolist() == [1, 1, 0, -2, -2]                            # ranks 3 and 4 are counted nowhere
    assert r["ndet"][1] == 3 and r["npig"][1, 0] == 5 and ref.reasons["beyond_max_dets"] == 2
    assert r["ar"][1, 0, 0].tolist() == [1 / 5.0, 2 / 5.0, 2 / 5.0]
    # TP, TP, FP: precision 1 up to recall 2/5 -> the points q = 0..40
    assert close(r["ap"][1, 0, 0], 41 / 101.0)


def test_recall_points_exactly_at_a_quarter_and_a_half():
    _ref, flags, r = run_ref("quarter_recalls")
    assert flags[0, :4, 0, 0].tolist() == [1, 0, 1, 0]
    # precision 1, 1/2, 2/3, 1/2 -> from the right 1, 2/3, 2/3, 1/2.  100 tp >= 4 q: q <= 25 at rank 0 (26 points of 1), q <= 50 at rank
    # 2 (25 points of 2/3), nothing beyond: q = 25 and q = 50 belong to the ranks where the recall is reached exactly
    want = 0.0
    for q in range(101):
        want += (1.0 / (1.0 + 2.0 ** -52)) if q <= 25 else (2.0 / (3.0 + 2.0 ** -52) if q <= 50 else 0.0)
    assert r["ap"][1, 0, 0] == want / 101.0 and close(r["ap"][1, 0, 0], (26 + 25 * 2 / 3.0) / 101.0)
    assert r["ar"][1, 0, 0].tolist() == [0.25, 0.5, 0.5]


def test_summaries_on_the_host():
    from tf_rpn_amd.utils import eval_utils
    _ref, _flags, r = run_ref("b")
    s = eval_utils.coco_summaries(r["ap"], r["ar"], cr.DEFAULT_IOU, cr.DEFAULT_AREAS, cr.DEFAULT_MAX_DETS)
    assert abs(s["AP"] - (6 + 4 * 51 / 101.0) / 10) <= TOL and abs(s["AP50"] - 1.0) <= TOL and abs(s["AP75"] - 1.0) <= TOL
    assert np.isnan(s["AP_area"][1]) and np.isnan(s["AP_area"][2]) and abs(s["AP_area"][3] - s["AP"]) <= TOL
    assert s["AR_max_dets"].shape == (3,) and s["AR_area"].shape == (4,) and s["stats"].shape == (12,)
    assert s["stats"][0] == s["AP"] and s["stats"][1] == s["AP50"] and s["stats"][8] == s["AR_max_dets"][2]
    other = eval_utils.coco_summaries(r["ap"][:, :, :1], r["ar"][:, :, :1], (0.5,), cr.DEFAULT_AREAS, cr.DEFAULT_MAX_DETS)
    assert other["stats"] is None and np.isnan(other["AP75"]) and abs(other["AP50"] - 1.0) <= TOL


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def test_coco_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rpn_[a-z0-9_]+)\s*\(", code))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in COCO_SYMBOLS:
        assert name in declared, "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name), "librpn_hip.so does not export %s" % name
        assert name in L.exported_symbols(), "%s is not bound in tf_rpn_amd/_lib.py" % name
    assert "typedef struct rpn_coco_evaluator rpn_coco_evaluator;" in code
    assert lib.rpn_abi_version() == 1
    for phrase in ("RECALLED", "LAST in input order on ties", "IN INTEGERS", "36 bytes per detection row", "2^-52"):
        assert phrase in header, phrase


def _create(lib, C=21, max_images=16, M=300, thr=cr.DEFAULT_IOU, areas=cr.DEFAULT_AREAS, max_dets=(1, 10, 100), size=(500.0, 500.0),
            T=None, A=None, K=None):
    ts = (ctypes.c_float * max(len(thr), 1))(*thr)
    flat = [v for pair in areas for v in pair]
    ar = (ctypes.c_float * max(len(flat), 2))(*flat)
    ks = (ctypes.c_int * max(len(max_dets), 1))(*max_dets)
    h = L.vp(0)
    st = lib.rpn_coco_evaluator_create(C, max_images, M, ts, len(thr) if T is None else T, ar, len(areas) if A is None else A, ks,
                                       len(max_dets) if K is None else K, size[0], size[1], ctypes.byref(h))
    return st, h


def test_coco_argument_validation_precedes_device_use(lib):
    for bad in (dict(T=0), dict(thr=(0.5,) * 11), dict(thr=(0.0,)), dict(thr=(1.5,)), dict(areas=((0.0, 1.0),) * 5), dict(A=0),
                dict(areas=((2.0, 1.0),)), dict(areas=((-1.0, 1.0),)), dict(areas=((0.0, float("inf")),)), dict(max_dets=(10, 10)),
                dict(max_dets=(10, 5)), dict(max_dets=(0, 5)), dict(max_dets=(1, 10, 301)), dict(max_dets=(1, 2, 3, 4, 5)), dict(K=0),
                dict(C=1), dict(C=70000), dict(max_images=0), dict(M=0), dict(M=4097), dict(max_images=1 << 20, M=4096),
                dict(size=(0.0, 500.0)), dict(size=(500.0, float("nan")))):
        st, h = _create(lib, **bad)
        assert st == L.RPN_ERR_INVALID and not h.value, bad
        assert b"rpn_coco_evaluator_create" in lib.rpn_last_error()
    st, h = _create(lib, max_images=4952)
    assert st == L.RPN_OK and h.value
    try:
        n = ctypes.c_size_t(0)
        assert lib.rpn_coco_evaluator_memory_bytes(h, ctypes.byref(n)) == L.RPN_OK
        assert 36 * 4952 * 300 <= n.value <= 36 * 4952 * 300 + (1 << 16)                # records, flags, the sort's pair, counters
        assert lib.rpn_coco_evaluator_images(h) == 0
        buf = np.zeros((64,), np.float32)
        p = L.vp(buf.ctypes.data + (-buf.ctypes.data) % 16)
        off = L.vp(p.value + 4)
        args = (h, p, p, p, p, p, p, None, None)
        assert lib.rpn_coco_evaluator_update(*(args + (1, 0, None, None))) == L.RPN_ERR_INVALID         # G = 0
        assert lib.rpn_coco_evaluator_update(*(args + (1, 2049, None, None))) == L.RPN_ERR_INVALID and b"2048" in lib.rpn_last_error()
        assert lib.rpn_coco_evaluator_update(*(args + (0, 4, None, None))) == L.RPN_ERR_INVALID
        assert lib.rpn_coco_evaluator_update(*(args + (4953, 4, None, None))) == L.RPN_ERR_INVALID and b"max_images" in lib.rpn_last_error()
        assert lib.rpn_coco_evaluator_update(h, None, p, p, p, p, p, None, None, 1, 4, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_coco_evaluator_update(h, off, p, p, p, p, p, None, None, 1, 4, None, None) == L.RPN_ERR_INVALID   # misaligned
        assert b"aligned" in lib.rpn_last_error()
        assert lib.rpn_coco_evaluator_update(h, p, p, p, p, off, p, None, None, 1, 4, None, None) == L.RPN_ERR_INVALID
        assert lib.rpn_coco_evaluator_images(h) == 0
    finally:
        lib.rpn_coco_evaluator_destroy(h)
    # NULL arrays stand for the defaults
    h = L.vp(0)
    assert lib.rpn_coco_evaluator_create(21, 4, 300, None, 0, None, 0, None, 0, 500.0, 500.0, ctypes.byref(h)) == L.RPN_OK
    lib.rpn_coco_evaluator_destroy(h)
    h = L.vp(0)
    assert lib.rpn_coco_evaluator_create(21, 4, 50, None, 0, None, 0, None, 0, 500.0, 500.0, ctypes.byref(h)) == L.RPN_ERR_INVALID   # 100 > M


def test_coco_python_checks_raise_before_anything_is_launched():
    from tf_rpn_amd.utils import eval_utils
    for bad in (dict(iou_thresholds=(0.5,) * 11), dict(iou_thresholds=()), dict(iou_thresholds=(1.5,)), dict(area_ranges=((0, 1),) * 5),
                dict(area_ranges=((2, 1),)), dict(area_ranges=(0, 1, 2)), dict(max_dets=(5, 5)), dict(max_dets=(1, 10, 301)),
                dict(max_dets=(1, 2, 3, 4, 5)), dict(image_size=(500,)), dict(image_size=(0, 500))):
        with pytest.raises(ValueError):
            eval_utils.CocoEvaluator(21, 8, 300, **bad)
    ev = eval_utils.CocoEvaluator(total_labels=3, max_images=2, max_detections=M_HAND, image_size=SIZE)
    assert ev.images == 0 and ev.memory_bytes() >= 36 * 2 * M_HAND
    boxes, scores, classes, valid, gtb, gtl, gtd = case_a()
    with pytest.raises(ValueError):
        ev.update(boxes[:, :4], scores[:, :4], classes[:, :4], valid, gtb, gtl, gtd)                # M != max_detections
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes[:, :4], valid, gtb, gtl, gtd)                              # wrong shape
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes, valid, gtb, gtl, gtd[:, :1])
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes, valid, gtb, gtl, gtd, image_sizes=np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        ev.update(boxes, scores, classes, valid, gtb, gtl, gtd, image_sizes=np.zeros((2, 2), np.float32))
    rep = lambda a, n: np.repeat(a, n, axis=0)
    with pytest.raises(ValueError):                                                                  # 3 images > max_images
        ev.update(rep(boxes, 3), rep(scores, 3), rep(classes, 3), rep(valid, 3), rep(gtb, 3), rep(gtl, 3), rep(gtd, 3))
    with pytest.raises(ValueError):                                                                  # G > 2048
        ev.update(boxes, scores, classes, valid, np.zeros((1, 2049, 4), np.float32), np.zeros((1, 2049), np.int32))
    assert ev.images == 0
