"""Soft-NMS: the numpy restatement of the contract in include/rpn_hip.h (rpn_soft_nms), its self-checks, and the case generator of
tests/test_gpu_soft_nms.py.  Nothing here needs a GPU.

The restatement runs the scores in float32 for ``linear`` (the device must match it bit for bit: one rounding per operation) and
in float64 for ``gaussian`` (the device's expf is not numpy's; test_gpu_soft_nms.py derives the bound).  The IoU is
``oracle.bbox_oracle.nms_iou`` (float32, the arithmetic of the hard NMS) in both, and the merge of the classes' lists is the
oracle's ``combined_non_max_suppression`` rule: (score descending, class ascending, selection rank ascending).

Besides the five outputs the restatement reports, per (image, class) pair,
  * the smallest DECISION MARGIN of its run: the relative gap between the two best live scores at every arg-max, and every updated
    score's relative distance from the score threshold -- the places where a last-bit difference in a score changes WHICH box is
    taken or whether one survives (the IoU tests compare identical float32 numbers on both sides and need no margin);
  * the largest number of decays (multiplications) any score of the pair received.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as entry  # noqa: E402
import cases  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

F32 = np.float32
N_LIMIT = 4096                   # include/rpn_hip.h: boxes per image
ENTRY_LIMIT = 16384              # C * min(max_per_class, N)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _soft_one_class(boxes, scores, max_out, method, k, iou_threshold, thr, ft):
    """-> ([(row, emitted score as ft)], smallest decision margin, most decays of one score)"""
    thr_t = ft(thr)
    cur = {n: ft(scores[n]) for n in range(len(scores)) if scores[n] > thr}          # strict: a NaN score never qualifies
    decays = dict.fromkeys(cur, 0)
    out, margin, kmax = [], np.inf, 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        while cur and len(out) < max_out:
            order = sorted(cur, key=lambda n: (-float(cur[n]), n))                   # highest score, ties to the lower row
            m = order[0]
            if len(order) > 1:
                margin = min(margin, (float(cur[m]) - float(cur[order[1]])) / float(cur[m]))
            out.append((m, cur.pop(m)))
            for n in sorted(cur):
                iou = bo.nms_iou(boxes[m], boxes[n])
                if method == "linear":
                    if not iou > iou_threshold:
                        continue
                    new = ft(cur[n] * ft(ft(1) - ft(iou)))
                else:
                    if iou > iou_threshold:                                          # TensorFlow's hard cut: a removal
                        del cur[n]
                        continue
                    if not iou > 0:
                        continue
                    new = ft(cur[n] * ft(np.exp(ft(ft(ft(iou) * ft(iou)) * ft(k)))))
                decays[n] += 1
                kmax = max(kmax, decays[n])
                if new > thr_t:
                    cur[n] = new
                    margin = min(margin, abs(float(new) - float(thr_t)) / max(float(new), float(thr_t)))
                else:
                    if new == new and max(abs(float(new)), float(thr_t)) > 0:
                        margin = min(margin, abs(float(new) - float(thr_t)) / max(abs(float(new)), float(thr_t)))
                    del cur[n]
    return out, margin, kmax


def soft_nms_ref(boxes, scores, max_output_size_per_class, max_total_size, method="gaussian", sigma=0.5, iou_threshold=0.5,
                 score_threshold=0.001, clip_boxes=True, details=None):
    """boxes (B,N,q,4) with q in {1,C}; scores (B,N,C) -> (boxes (B,M,4), scores (B,M), classes (B,M), valid (B,) int32,
    indices (B,M) int32, -1 padded), float32.  ``details`` (a dict) receives {(b, c): (list of (row, score), margin, decays)}."""
    assert method in ("linear", "gaussian") and float(sigma) > 0 and float(iou_threshold) >= 0 and float(score_threshold) >= 0
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    B, N, q, _ = boxes.shape
    C = scores.shape[2]
    assert q in (1, C)
    ft = F32 if method == "linear" else np.float64
    k = F32(-1.0 / float(sigma))                     # -0.0 for sigma = inf: every weight is exactly 1
    iou_threshold = F32(iou_threshold)
    thr = F32(score_threshold)
    M = int(max_total_size)
    out_boxes = np.zeros((B, M, 4), F32)
    out_scores = np.zeros((B, M), F32)
    out_classes = np.zeros((B, M), F32)
    out_idx = np.full((B, M), -1, np.int32)
    valid = np.zeros((B,), np.int32)
    for b in range(B):
        entries = []
        for c in range(C):
            sel, margin, kmax = _soft_one_class(boxes[b, :, 0 if q == 1 else c, :], scores[b, :, c], int(max_output_size_per_class),
                                                method, k, iou_threshold, thr, ft)
            if details is not None:
                details[(b, c)] = (sel, margin, kmax)
            for rank, (i, s) in enumerate(sel):
                entries.append((-float(s), c, rank, i))
        entries.sort()
        entries = entries[:M]
        valid[b] = len(entries)
        for r, (neg, c, _, i) in enumerate(entries):
            bx = boxes[b, i, 0 if q == 1 else c, :]
            if clip_boxes:
                bx = np.minimum(np.maximum(bx, F32(0)), F32(1))
            out_boxes[b, r] = bx
            out_scores[b, r] = F32(-neg)
            out_classes[b, r] = F32(c)
            out_idx[b, r] = i
    return out_boxes, out_scores, out_classes, valid, out_idx


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- case generators (shared with the GPU tests) ----------------------------------------------------------------------------------
def cluster_case(seed, B, N, C, q, n_clusters=4, centre_jitter=0.03, size_jitter=0.15):
    """Per (image, box set): ``n_clusters`` clusters of N / n_clusters boxes jittered off one box each (centres by
    ``centre_jitter``, log-sizes by ``size_jitter``), uniform scores in [0, 1)."""
    rng = np.random.RandomState(seed)
    boxes = np.zeros((B, N, q, 4), F32)
    for b in range(B):
        for j in range(q):
            cy, cx = rng.uniform(0.2, 0.8, size=(2, n_clusters))
            h, w = rng.uniform(0.1, 0.35, size=(2, n_clusters))
            pick = np.arange(N) % n_clusters
            yy = cy[pick] + rng.normal(0, centre_jitter, N)
            xx = cx[pick] + rng.normal(0, centre_jitter, N)
            hh = h[pick] * np.exp(rng.normal(0, size_jitter, N))
            ww = w[pick] * np.exp(rng.normal(0, size_jitter, N))
            boxes[b, :, j] = np.stack([yy - hh / 2, xx - ww / 2, yy + hh / 2, xx + ww / 2], axis=-1)
    scores = rng.uniform(0, 1, size=(B, N, C)).astype(F32)
    return boxes, scores


# (B, N, C, q) of the bit-for-bit linear tests: one past a wave, one past a 256-thread sweep, a single row
LINEAR_SHAPES = [(2, 64, 5, 5), (1, 65, 3, 1), (1, 257, 2, 1), (3, 1, 2, 1)]


@functools.lru_cache(maxsize=None)
def linear_case(index):
    B, N, C, q = LINEAR_SHAPES[index]
    boxes, scores = cluster_case(100 + index, B, N, C, q, n_clusters=max(1, min(4, N // 8)))
    scores[:, ::7] = np.round(scores[:, ::7] * 4) / 4                # some exact ties: the row order decides
    if N > 8:
        boxes[:, 5] = boxes[:, 4]                                    # an exact duplicate (IoU 1: a linear decay to 0)
    kw = dict(max_output_size_per_class=min(N, 40), max_total_size=min(N * C, 70), method="linear", iou_threshold=0.3,
              score_threshold=0.05)
    return boxes, scores, kw, soft_nms_ref(boxes, scores, **kw)


@functools.lru_cache(maxsize=None)
def tie_case(seed=5, B=2, N=96, C=3):
    """Tied and duplicate scores, duplicate / flipped / degenerate / NaN boxes: what the hard-equivalence tests run"""
    rng = np.random.RandomState(seed)
    boxes = cases.clustered_boxes(rng, B, N, n_clusters=6)
    boxes[:, 10] = boxes[:, 3]                                       # duplicates
    boxes[:, 11] = boxes[:, 3]
    boxes[:, 20] = boxes[:, 21][..., [2, 3, 0, 1]]                   # flipped corners: the same canonical box
    boxes[:, 30, 2] = boxes[:, 30, 0]                                # zero height
    boxes[0, 40] = [np.nan, 0.1, 0.5, 0.5]                           # NaN area: its IoUs are NaN and never suppress
    boxes[1, 41] = [0.2, 0.2, np.nan, 0.6]                           # a NaN that canonical() drops: area 0
    scores = (rng.randint(0, 9, size=(B, N, C)) / 8.0).astype(F32)   # heavy ties
    scores[0, 50, 1] = np.nan                                        # never a candidate
    return boxes[:, :, None, :].copy(), scores


# sigma / iou_threshold / score_threshold of the Gaussian tests; (B, N, C, q) = (4, 64, 5, 5): 20 independent pairs each
GAUSS_SHAPE = (4, 64, 5, 5)
GAUSS_CASES = [(0.5, 1.0, 0.05), (0.5, 1.0, 0.001), (0.25, 0.5, 0.05), (0.25, 0.5, 0.001)]
EXPF_ULPS = 2.0                  # the expf allowance of tests/test_gpu_roi_head.py's header (its softmax bound's second term)


def decay_bound(sigma):
    """Relative error of ONE device decay against the float64 restatement: the argument t = fl(fl(iou^2) k) carries two roundings,
    |t| 2^-24 each, which expf turns into 2 |t| 2^-24 relative; expf's own allowance; the product's rounding.  |t| <= 1 / sigma."""
    return (2.0 / sigma + EXPF_ULPS + 1.0) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def gauss_case(index):
    sigma, iou_thr, score_thr = GAUSS_CASES[index]
    B, N, C, q = GAUSS_SHAPE
    boxes, scores = cluster_case(200 + index, B, N, C, q)
    kw = dict(max_output_size_per_class=N, max_total_size=N * C, method="gaussian", sigma=sigma, iou_threshold=iou_thr,
              score_threshold=score_thr)
    details = {}
    ref = soft_nms_ref(boxes, scores, details=details, **kw)
    return boxes, scores, kw, ref, details


def decided(details, sigma):
    """{pair: bound} of the pairs whose smallest margin exceeds twice their own bound (decays x one decay's bound)"""
    out = {}
    for pair, (_sel, margin, kmax) in details.items():
        bound = kmax * decay_bound(sigma)
        if margin > 2.0 * bound:
            out[pair] = bound
    return out


# ---- self-checks ------------------------------------------------------------------------------------------------------------------
def _hard(boxes, scores, **kw):
    return bo.combined_non_max_suppression(boxes, scores, return_indices=True, **kw)


@pytest.mark.parametrize("t", [0.5, 0.7])
@pytest.mark.parametrize("s", [0.0, 0.05, 0.5])
def test_infinite_sigma_is_hard_nms_on_ties_duplicates_and_nans(t, s):
    boxes, scores = tie_case()
    for m, total in ((7, 12), (96, 300)):
        got = soft_nms_ref(boxes, scores, m, total, method="gaussian", sigma=float("inf"), iou_threshold=t, score_threshold=s)
        want = _hard(boxes, scores, max_output_size_per_class=m, max_total_size=total, iou_threshold=t, score_threshold=s)
        assert same(got, want)
        assert got[3].min() > 0


def test_infinite_sigma_is_hard_nms_on_random_cases():
    rng = np.random.RandomState(11)
    for it in range(12):
        B, N, C = int(rng.randint(1, 3)), int(rng.randint(1, 50)), int(rng.randint(1, 4))
        q = C if it & 1 else 1
        boxes = np.stack([cases.clustered_boxes(rng, B, N, n_clusters=4) for _ in range(q)], axis=2)
        scores = (cases.permutation_scores(rng, B, N * C).reshape(B, N, C) if it % 3 else
                  (rng.randint(0, 5, size=(B, N, C)) / 4.0).astype(F32))
        t = float(rng.choice([0.3, 0.5, 0.75]))
        kw = dict(max_output_size_per_class=int(rng.choice([1, 5, 50])), max_total_size=int(rng.choice([3, 20, 200])))
        s = float(rng.choice([0.0, 0.2]))
        for clip in (True, False):
            got = soft_nms_ref(boxes - (0.0 if clip else 0.3), scores, method="gaussian", sigma=float("inf"), iou_threshold=t,
                               score_threshold=s, clip_boxes=clip, **kw)
            want = _hard(boxes - (0.0 if clip else 0.3), scores, iou_threshold=t, score_threshold=s, clip_boxes=clip, **kw)
            assert same(got, want), it


A = [0.0, 0.0, 0.5, 1.0]                   # area 1/2
HALF = [0.0, 0.0, 0.5, 0.5]                # inside A: IoU exactly 1/2
FAR = [0.6, 0.0, 0.9, 1.0]                 # IoU 0 with both


def _one(boxes, scores):
    return np.asarray(boxes, F32)[None, :, None, :], np.asarray(scores, F32)[None, :, None]


def test_two_identical_boxes():
    boxes, scores = _one([A, A], [0.9, 0.8])
    b, s, c, v, i = soft_nms_ref(boxes, scores, 10, 10, method="linear", iou_threshold=0.3, score_threshold=0.0)
    assert v.tolist() == [1] and i[0, :2].tolist() == [0, -1]        # 0.8 * (1 - 1) = 0 is not > 0: it dies
    b, s, c, v, i = soft_nms_ref(boxes, scores, 10, 10, method="gaussian", sigma=0.5, iou_threshold=1.0, score_threshold=0.001)
    assert v.tolist() == [2] and i[0, :2].tolist() == [0, 1]
    assert s[0, 0] == F32(0.9) and s[0, 1] == F32(np.float64(F32(0.8)) * np.exp(-1.0 / 0.5))
    b, s, c, v, i = soft_nms_ref(boxes, scores, 10, 10, method="gaussian", sigma=0.5, iou_threshold=0.5, score_threshold=0.001)
    assert v.tolist() == [1]                                         # the hard cut removes it


def test_a_decay_lets_a_lower_box_overtake():
    boxes, scores = _one([A, HALF, FAR], [0.9, 0.8, 0.7])
    b, s, c, v, i = soft_nms_ref(boxes, scores, 10, 10, method="linear", iou_threshold=0.3, score_threshold=0.05)
    assert v.tolist() == [3] and i[0, :3].tolist() == [0, 2, 1]
    assert s[0, :3].tolist() == [F32(0.9), F32(0.7), F32(F32(0.8) * F32(0.5))]
    assert (np.diff(s[0, :3]) <= 0).all()
    hard = _hard(boxes, scores, max_output_size_per_class=10, max_total_size=10, iou_threshold=0.3, score_threshold=0.05)
    assert hard[3].tolist() == [2]                                   # hard NMS deletes the middle box


def test_a_score_decayed_to_exactly_the_threshold_dies():
    boxes, scores = _one([A, HALF], [0.9, 0.5])
    for thr, n in ((0.25, 1), (0.2, 2)):                             # 0.5 * (1 - 0.5) = 0.25 exactly
        v = soft_nms_ref(boxes, scores, 10, 10, method="linear", iou_threshold=0.3, score_threshold=thr)[3]
        assert v.tolist() == [n], thr
    details = {}
    soft_nms_ref(boxes, scores, 10, 10, method="linear", iou_threshold=0.3, score_threshold=0.25, details=details)
    assert details[(0, 0)][1] == 0.0 and details[(0, 0)][2] == 1     # the margin sees it; one decay


def test_output_sizes():
    boxes, scores = _one([A, FAR, HALF], [0.9, 0.7, 0.8])
    b, s, c, v, i = soft_nms_ref(boxes, scores, 1, 10, method="linear", iou_threshold=0.3, score_threshold=0.05)
    assert v.tolist() == [1] and i[0].tolist() == [0] + [-1] * 9 and b.shape == (1, 10, 4)
    # two classes of three each, four places
    boxes2 = np.repeat(boxes, 2, axis=2)
    scores2 = np.concatenate([scores, scores - F32(0.05)], axis=2)
    b, s, c, v, i = soft_nms_ref(boxes2, scores2, 10, 4, method="linear", iou_threshold=0.3, score_threshold=0.05)
    assert v.tolist() == [4] and c[0].tolist() == [0, 1, 0, 1] and i[0].tolist() == [0, 0, 1, 1]
    assert soft_nms_ref(boxes2, scores2, 0, 4, method="linear")[3].tolist() == [0]


def test_class_zero_is_a_class_like_any_other():
    boxes, scores = _one([A, FAR], [0.9, 0.7])
    scores3 = np.concatenate([scores, np.zeros_like(scores), scores * F32(0.5)], axis=2)
    b, s, c, v, i = soft_nms_ref(boxes, scores3, 10, 10, method="gaussian", sigma=0.5, iou_threshold=0.5, score_threshold=0.001)
    assert v.tolist() == [4] and c[0, :4].tolist() == [0, 0, 2, 2]


def test_merge_ties_go_to_the_lower_class_then_the_earlier_selection():
    boxes, scores = _one([A, FAR], [0.5, 0.5])
    scores2 = np.repeat(scores, 2, axis=2)
    b, s, c, v, i = soft_nms_ref(boxes, scores2, 10, 3, method="linear", iou_threshold=0.3, score_threshold=0.0)
    assert c[0].tolist() == [0, 0, 1] and i[0].tolist() == [0, 1, 0]


def test_linear_cases_hold_the_contracts_properties():
    for index in range(len(LINEAR_SHAPES)):
        boxes, scores, kw, (b, s, c, v, i) = linear_case(index)
        for img in range(boxes.shape[0]):
            n = int(v[img])
            assert (np.diff(s[img, :n]) <= 0).all() and (s[img, :n] > kw["score_threshold"]).all()
            assert (i[img, n:] == -1).all() and (s[img, n:] == 0).all() and (b[img, n:] == 0).all()
            for cls in range(scores.shape[2]):
                rows = i[img, :n][c[img, :n] == cls]
                assert len(set(rows.tolist())) == len(rows)                      # a row is selected once per class
    assert any(int(linear_case(k)[3][3].max()) == linear_case(k)[2]["max_total_size"] for k in range(2))    # the cut is reached


@pytest.mark.parametrize("index", range(len(GAUSS_CASES)))
def test_gaussian_cases_stay_inside_the_skip_condition(index):
    """What tests/test_gpu_soft_nms.py requires of its inputs, checked under the restatement alone: at most 10 % of a case's pairs
    have a decision margin within twice their bound."""
    sigma = GAUSS_CASES[index][0]
    boxes, scores, kw, ref, details = gauss_case(index)
    ok = decided(details, sigma)
    margins = sorted(m for _s, m, _k in details.values())
    print("case", index, "pairs", len(details), "undecided", len(details) - len(ok), "smallest margins", margins[:3],
          "most decays", max(k for _s, _m, k in details.values()), "largest bound", max(ok.values()))
    assert len(details) == GAUSS_SHAPE[0] * GAUSS_SHAPE[2]
    assert len(details) - len(ok) <= 0.1 * len(details)
    assert max(k for _s, _m, k in details.values()) >= 10                        # the scores really are decayed many times


# ---- the Python entry without a device: everything is refused before anything is copied or launched ----------------------------------
def test_bad_arguments_raise_value_error(lib):
    from tf_rpn_amd.utils import bbox_utils, roi_utils
    boxes = np.zeros((1, 4, 1, 4), F32)
    scores = np.zeros((1, 4, 2), F32)
    for kw in (dict(method="hard"), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(iou_threshold=-0.1),
               dict(score_threshold=-0.001), dict(score_threshold=float("nan"))):
        with pytest.raises(ValueError):
            bbox_utils.soft_non_max_suppression(boxes, scores, 10, 10, **kw)
    with pytest.raises(ValueError):
        bbox_utils.soft_non_max_suppression(np.zeros((1, N_LIMIT + 1, 1, 4), F32), np.zeros((1, N_LIMIT + 1, 2), F32), 10, 10)
    with pytest.raises(ValueError):
        bbox_utils.soft_non_max_suppression(np.zeros((1, 4096, 1, 4), F32), np.zeros((1, 4096, 5), F32), 4000, 10)    # 5 * 4000 entries
    rois, reg, logits = np.zeros((1, 4, 4), F32), np.zeros((1, 4, 8), F32), np.zeros((1, 4, 2), F32)
    for kw in (dict(nms="soft"), dict(nms="gaussian", sigma=0.0), dict(nms="linear", score_threshold=-1.0),
               dict(nms="linear", score_threshold=0.0)):
        with pytest.raises(ValueError):
            roi_utils.roi_detections(rois, reg, logits, [0.1, 0.1, 0.2, 0.2], **kw)


def test_library_refuses_over_limit_calls_before_device_use(lib):
    def call(N=64, C=2, m=10, method=1, iou=0.5, sigma=0.5, thr=0.001, B=0):
        return lib.rpn_soft_nms(None, None, B, N, 1, C, m, 10, method, iou, sigma, thr, 1, None, None, None, None, None, None, 0, None)
    assert call() == L.RPN_OK                                        # B == 0: nothing to do
    assert call(N=N_LIMIT) == L.RPN_OK
    for kw in (dict(N=N_LIMIT + 1), dict(C=5, N=4096, m=4000), dict(method=2), dict(method=-1), dict(iou=-1.0), dict(sigma=0.0),
               dict(sigma=float("nan")), dict(thr=-0.5), dict(C=0)):
        assert call(**kw) == L.RPN_ERR_INVALID, kw
        assert b"rpn_soft_nms" in lib.rpn_last_error()
    assert call(sigma=float("inf")) == L.RPN_OK
    assert lib.rpn_soft_nms_workspace_bytes(2, 300, 21, 100, 300) >= 2 * 21 * 100 * 8 + 2 * 21 * 4
    assert lib.rpn_soft_nms_workspace_bytes(2, 30, 21, 100, 300) < lib.rpn_soft_nms_workspace_bytes(2, 300, 21, 100, 300)
