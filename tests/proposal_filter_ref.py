"""numpy restatement of rpn_proposal_filter (include/rpn_hip.h), shared by the host and the GPU tests of the proposal filter.

It takes ALREADY DECODED boxes: the device's expf is not numpy's, so the oracle never decodes -- a GPU test feeds it the device's
own get_bboxes_from_deltas, a hand-written case feeds it boxes whose decode is exact."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def _clip01(v):
    """bbox_core.h's clip01: v < 0 ? 0 : (v > 1 ? 1 : v) -- a NaN stays a NaN."""
    v = np.asarray(v, np.float32)
    return np.where(v < 0, np.float32(0), np.where(v > 1, np.float32(1), v)).astype(np.float32)


def min_size_pair(min_size):
    if min_size is None:
        return None
    if isinstance(min_size, (tuple, list, np.ndarray)):
        mh, mw = min_size
    else:
        mh = mw = min_size
    return np.float32(mh), np.float32(mw)


def size_ok(boxes, min_size, clip=True):
    """(..., 4) float32 boxes [y1, x1, y2, x2] -> bool: both sides reach the minimum (one float32 subtraction each; NaN fails)."""
    mh, mw = min_size_pair(min_size)
    bx = np.asarray(boxes, np.float32)
    if clip:
        bx = _clip01(bx)
    with np.errstate(invalid="ignore"):
        h = (bx[..., 2] - bx[..., 0]).astype(np.float32)
        w = (bx[..., 3] - bx[..., 1]).astype(np.float32)
        return (h >= mh) & (w >= mw)


def filter_ref(boxes, scores, pre_nms_topn=None, min_size=None, score_threshold=float("-inf"), clip=True):
    """boxes (B,A,4) float32 decoded (unclipped) or None when min_size is None; scores (B,A) float32
    -> (masked (B,A) float32: the score's bits where kept, -inf elsewhere; kept (B,) int32)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    B, A = s.shape
    thr = np.float32(score_threshold)
    masked = np.full((B, A), NEG_INF, np.float32)
    kept = np.zeros((B,), np.int32)
    with np.errstate(invalid="ignore"):
        cand = s > thr                                           # strict; False for NaN
    if min_size is not None:
        cand = cand & size_ok(boxes, min_size, clip)
    for b in range(B):
        idx = np.nonzero(cand[b])[0]                             # ascending index
        # score descending as floats compare, ties (-0.0 and +0.0 among them) to the lower index: a stable sort of -score
        order = idx[np.argsort(-s[b, idx], kind="stable")]
        if pre_nms_topn is not None:
            order = order[:int(pre_nms_topn)]
        masked[b, order] = s[b, order]
        kept[b] = len(order)
    return masked, kept


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
