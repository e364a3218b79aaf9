"""CPU suite of the proposal filter (rpn_proposal_filter, bbox_utils.filter_proposals, the pre_nms_topn / min_size keywords):
the numpy oracle checked on hand-written cases, the exported symbols, and every argument check -- all without a device."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import proposal_filter_ref as ref
from tf_rpn_amd import _lib as L
from tf_rpn_amd.predictor import Proposer
from tf_rpn_amd.utils import bbox_utils

NINF = -np.inf


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


def _f32(*v):
    return np.array([v], np.float32)


# ---- the oracle on hand-written cases -------------------------------------------------------------
def test_oracle_tie_across_the_cut_goes_to_the_lower_index():
    s = _f32(0.5, 0.9, 0.5, 0.5, 0.1)
    m, k = ref.filter_ref(None, s, pre_nms_topn=3)
    assert k.tolist() == [3]
    assert np.array_equal(ref.bits(m), ref.bits(_f32(0.5, 0.9, 0.5, NINF, NINF)))
    m, k = ref.filter_ref(None, s, pre_nms_topn=2)
    assert np.array_equal(ref.bits(m), ref.bits(_f32(0.5, 0.9, NINF, NINF, NINF))) and k.tolist() == [2]
    # -0.0 and +0.0 tie: index decides, and the kept bits are the input's
    z = _f32(0.0, -0.0, 0.0, -0.0)
    m, k = ref.filter_ref(None, z, pre_nms_topn=2)
    assert np.array_equal(ref.bits(m), ref.bits(_f32(0.0, -0.0, NINF, NINF))) and k.tolist() == [2]
    m, _ = ref.filter_ref(None, _f32(-0.0, 0.0, -0.0), pre_nms_topn=1)
    assert np.array_equal(ref.bits(m), ref.bits(_f32(-0.0, NINF, NINF)))


def test_oracle_nan_minus_inf_and_the_threshold_are_never_kept():
    s = _f32(np.nan, NINF, 0.5, 0.25, np.inf, 0.75)
    m, k = ref.filter_ref(None, s, score_threshold=0.5)
    assert np.array_equal(ref.bits(m), ref.bits(_f32(NINF, NINF, NINF, NINF, np.inf, 0.75))) and k.tolist() == [2]
    m, k = ref.filter_ref(None, s)                                   # threshold -inf: -inf itself is not > -inf
    assert np.array_equal(ref.bits(m), ref.bits(_f32(NINF, NINF, 0.5, 0.25, np.inf, 0.75))) and k.tolist() == [4]
    m, k = ref.filter_ref(None, s, pre_nms_topn=1)                   # +inf ranks first
    assert np.array_equal(ref.bits(m), ref.bits(_f32(NINF, NINF, NINF, NINF, np.inf, NINF))) and k.tolist() == [1]
    m, k = ref.filter_ref(None, s, score_threshold=np.nan)           # nothing is > NaN
    assert k.tolist() == [0] and np.isneginf(m).all()


def test_oracle_kept_is_min_of_n_and_candidates():
    rng = np.random.RandomState(0)
    s = rng.uniform(0, 1, size=(3, 50)).astype(np.float32)
    cands = (s > np.float32(0.5)).sum(axis=1)
    for n in (1, 10, 49, 50, 55):
        m, k = ref.filter_ref(None, s, pre_nms_topn=n, score_threshold=0.5)
        assert k.tolist() == np.minimum(n, cands).tolist()
        assert ((~np.isneginf(m)).sum(axis=1) == k).all()
        for b in range(3):                                            # the kept are the n best
            kept = ~np.isneginf(m[b])
            if k[b] < cands[b]:
                assert s[b][kept].min() > s[b][(s[b] > 0.5) & ~kept].max()
    m, k = ref.filter_ref(None, s, pre_nms_topn=None, score_threshold=0.5)
    assert k.tolist() == cands.tolist()


def test_oracle_min_size_boundary():
    side = np.float32(0.125)
    above = np.nextafter(side, np.float32(np.inf))
    boxes = np.array([[[0.25, 0.25, 0.375, 0.5]]], np.float32)        # h = 0.125, w = 0.25 exactly
    s = _f32(0.5)
    assert ref.filter_ref(boxes, s, min_size=(side, 0.0))[1].tolist() == [1]          # equal passes
    assert ref.filter_ref(boxes, s, min_size=(above, 0.0))[1].tolist() == [0]         # the next float32 rejects
    assert ref.filter_ref(boxes, s, min_size=(0.0, 0.25))[1].tolist() == [1]
    assert ref.filter_ref(boxes, s, min_size=(0.0, np.nextafter(np.float32(0.25), np.float32(1))))[1].tolist() == [0]
    assert ref.filter_ref(boxes, s, min_size=side)[1].tolist() == [1]                 # a scalar is both
    assert ref.filter_ref(boxes, s, min_size=0.25)[1].tolist() == [0]
    # clipping comes first: 0.1875 high unclipped, 0.125 inside the image
    out = np.array([[[-0.0625, 0.0, 0.125, 0.5]]], np.float32)
    assert ref.filter_ref(out, s, min_size=(0.1875, 0.0), clip=False)[1].tolist() == [1]
    assert ref.filter_ref(out, s, min_size=(0.1875, 0.0), clip=True)[1].tolist() == [0]
    nan = np.array([[[-np.inf, 0.0, np.nan, 0.5]]], np.float32)       # a NaN side fails, clipped or not
    assert ref.filter_ref(nan, s, min_size=0.0, clip=True)[1].tolist() == [0]
    assert ref.filter_ref(nan, s, min_size=0.0, clip=False)[1].tolist() == [0]
    assert ref.filter_ref(None, s, min_size=None)[1].tolist() == [1]
    # the size test comes first: the cut counts the survivors only
    boxes = np.array([[[0, 0, 0.5, 0.5], [0, 0, 0.01, 0.5], [0, 0, 0.5, 0.5], [0, 0, 0.5, 0.5]]], np.float32)
    m, k = ref.filter_ref(boxes, _f32(0.1, 0.9, 0.2, 0.3), pre_nms_topn=2, min_size=0.1)
    assert np.array_equal(ref.bits(m), ref.bits(_f32(NINF, NINF, 0.2, 0.3))) and k.tolist() == [2]


# ---- the library and the wrappers -----------------------------------------------------------------
def test_symbols_are_exported_and_in_the_ctypes_table(lib):
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ("rpn_proposal_filter", "rpn_proposal_filter_workspace_bytes"):
        assert hasattr(raw, name) and name in L.exported_symbols()
    header = open(os.path.join(entry.ROOT, "include", "rpn_hip.h")).read()
    assert "int rpn_proposal_filter(" in header and "size_t rpn_proposal_filter_workspace_bytes(int B, int A);" in header
    assert int(lib.rpn_proposal_filter_workspace_bytes(8, 61440)) >= 0


def test_library_argument_validation_precedes_device_use(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, L.vp)
    q = L.vp(ctypes.addressof(buf) + 32 * 4)

    def call(anchors=p, deltas=p, scores=p, B=1, A=8, topn=0, use_min=0, mh=0.0, mw=0.0, masked=q):
        return lib.rpn_proposal_filter(anchors, deltas, None, scores, B, A, topn, use_min, mh, mw, 0.0, 1, masked, None, None, 0, None)

    for kwargs, text in (({"B": -1}, b"negative size"), ({"A": -1}, b"negative size"),
                         ({"use_min": 1, "mh": -1.0}, b"min_size"), ({"use_min": 1, "mw": float("nan")}, b"min_size"),
                         ({"scores": None}, b"null score pointer"), ({"masked": None}, b"null score pointer"),
                         ({"use_min": 1, "anchors": None}, b"needs anchors and deltas"),
                         ({"use_min": 1, "deltas": None}, b"needs anchors and deltas"),
                         ({"masked": p}, b"must not alias"), ({"masked": L.vp(ctypes.addressof(buf) + 4)}, b"must not alias")):
        assert call(**kwargs) == L.RPN_ERR_INVALID, kwargs
        assert text in lib.rpn_last_error(), (kwargs, lib.rpn_last_error())
    # a negative or NaN minimum is only looked at when the size test is on (B = 0: accepted, and returns before any device use)
    assert call(B=0, mh=-1.0) == L.RPN_OK
    assert call(B=0, mw=float("nan")) == L.RPN_OK
    assert call(B=0, use_min=1, mh=-1.0) == L.RPN_ERR_INVALID


@pytest.mark.parametrize("bad", [0, -3, 2.5, "7", True, float("nan")])
def test_pre_nms_topn_must_be_a_positive_integer(bad):
    a, d, s = np.zeros((5, 4), np.float32), np.zeros((2, 5, 4), np.float32), np.zeros((2, 5), np.float32)
    with pytest.raises(ValueError, match="pre_nms_topn"):
        bbox_utils.filter_proposals(a, d, s, None, pre_nms_topn=bad)
    with pytest.raises(ValueError, match="pre_nms_topn"):
        bbox_utils.decode_and_nms(a, d, s, None, 3, pre_nms_topn=bad)
    with pytest.raises(ValueError, match="pre_nms_topn"):
        Proposer("vgg16", pre_nms_topn=bad)


@pytest.mark.parametrize("bad", [-0.5, float("nan"), (0.1, -1e-9), (float("nan"), 0.1), (0.1, 0.2, 0.3), (0.1,), "x"])
def test_min_size_must_be_non_negative(bad):
    a, d, s = np.zeros((5, 4), np.float32), np.zeros((2, 5, 4), np.float32), np.zeros((2, 5), np.float32)
    with pytest.raises(ValueError, match="min_size"):
        bbox_utils.filter_proposals(a, d, s, None, min_size=bad)
    with pytest.raises(ValueError, match="min_size"):
        bbox_utils.decode_and_nms(a, d, s, None, 3, min_size=bad)
    with pytest.raises(ValueError, match="min_size"):
        Proposer("vgg16", min_size=bad)


def test_wrong_shapes_are_refused_before_any_launch():
    good = (np.zeros((5, 4), np.float32), np.zeros((2, 5, 4), np.float32), np.zeros((2, 5), np.float32))
    for i, wrong in ((0, np.zeros((6, 4), np.float32)), (0, np.zeros((5, 3), np.float32)), (1, np.zeros((2, 5, 3), np.float32)),
                     (1, np.zeros((10, 4), np.float32)), (2, np.zeros((2, 6), np.float32)), (2, np.zeros((3, 5), np.float32)),
                     (2, np.zeros((2, 5, 1), np.float32))):
        args = list(good)
        args[i] = wrong
        with pytest.raises(ValueError, match="inconsistent shapes"):
            bbox_utils.filter_proposals(*args, None, pre_nms_topn=3)
        with pytest.raises(ValueError, match="inconsistent shapes"):
            bbox_utils.decode_and_nms(*args, None, 3, pre_nms_topn=3, min_size=0.1)


def test_check_proposal_filter_accepts_the_documented_forms():
    assert bbox_utils.check_proposal_filter(None, None) == (0, 0, 0.0, 0.0)
    assert bbox_utils.check_proposal_filter(12000, 16 / 500) == (12000, 1, 16 / 500, 16 / 500)
    assert bbox_utils.check_proposal_filter(np.int64(7), (0.0, 0.5)) == (7, 1, 0.0, 0.5)
    assert bbox_utils.check_proposal_filter(None, [0.25, 0.125]) == (0, 1, 0.25, 0.125)
    assert bbox_utils.check_proposal_filter(None, np.float32(0.5)) == (0, 1, 0.5, 0.5)


def test_new_keywords_default_to_none():
    for fn in (bbox_utils.decode_and_nms, Proposer.__init__):
        params = inspect.signature(fn).parameters
        assert params["pre_nms_topn"].default is None and params["min_size"].default is None
    params = inspect.signature(bbox_utils.decode_and_nms).parameters
    assert list(params)[:8] == ["anchors", "deltas", "scores", "variances", "max_total_size", "iou_threshold", "score_threshold",
                                "clip_boxes"]                       # the new keywords come after the existing arguments
    params = inspect.signature(bbox_utils.filter_proposals).parameters
    assert list(params) == ["anchors", "deltas", "scores", "variances", "pre_nms_topn", "min_size", "score_threshold", "clip_boxes"]
    assert params["pre_nms_topn"].default is None and params["min_size"].default is None
    assert params["score_threshold"].default == float("-inf") and params["clip_boxes"].default is True
