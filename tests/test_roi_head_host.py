"""Second-stage targets, losses and detections (tf_rpn_amd/csrc/roi_head_kernels.hip): what can be checked without a GPU.

The numpy restatements the GPU suite (tests/test_gpu_roi_head.py) compares against live here.  They are compositions of
``oracle.bbox_oracle`` functions -- ``generate_iou_map`` on (B,R,4) boxes, ``randomly_select_xyz_mask``,
``get_deltas_from_bboxes`` -- so the arithmetic and the sampling rule are the ones the RPN targets are already held to.  This file
checks the restatements against themselves (counts, padding, float32 against float64, gradients against central differences), the
five C-ABI entries (declared, exported, bound; arguments validated before any device use; loud failure without a device) and the new
kernels' register budgets.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from oracle import bbox_oracle as bo
from tf_rpn_amd import _lib as L
from tf_rpn_amd.utils import roi_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
VARIANCES = [0.1, 0.1, 0.2, 0.2]
NEW_SYMBOLS = ["rpn_roi_decode_scores", "rpn_roi_losses", "rpn_roi_losses_workspace_bytes", "rpn_roi_targets",
               "rpn_roi_targets_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry.build()
    return L.lib()


# ---- restatements -------------------------------------------------------------------------------------------------------------
def roi_targets_ref(rois, valid, gt_boxes, gt_labels, total_pos, total_neg, random_pos, random_neg, pos_iou=0.5, neg_iou=(0.1, 0.5),
                    variances=VARIANCES):
    """-> (roi_deltas (B,R,4) f32, roi_labels (B,R) i32, raw positive candidates per image)"""
    rois, gt_boxes = np.asarray(rois, F32), np.asarray(gt_boxes, F32)
    gt_labels = np.asarray(gt_labels, np.int32)
    B, R, _ = rois.shape
    live = np.arange(R)[None, :] < (np.full((B,), R) if valid is None else np.clip(np.asarray(valid), 0, R))[:, None]
    iou = bo.generate_iou_map(rois, gt_boxes)                                            # (B,R,G)
    # "for valid gt g in index order: if (iou > best) { best = iou; arg = g; }" from best = 0: a NaN or an invalid gt never wins
    usable = np.logical_and((gt_labels >= 1)[:, None, :], np.logical_not(np.isnan(iou)))
    masked = np.where(usable, iou, F32(-1.0)).astype(F32)
    top, first = masked.max(axis=2), masked.argmax(axis=2)                               # argmax: the first maximum
    has = top > 0
    best = np.where(has, top, F32(0.0)).astype(F32)
    arg = np.where(has, first, 0)
    pos_cand = np.logical_and(live, best > F32(pos_iou))
    pos = bo.randomly_select_xyz_mask(pos_cand, np.array([total_pos]), random_pos)
    neg_want = (total_pos + total_neg) - pos.sum(axis=-1)
    neg_cand = live & np.logical_not(pos) & (best >= F32(neg_iou[0])) & (best < F32(neg_iou[1]))
    neg = bo.randomly_select_xyz_mask(neg_cand, neg_want, random_neg)
    labels = np.where(pos, np.take_along_axis(gt_labels, arg, axis=1), np.where(neg, 0, -1)).astype(np.int32)
    matched = np.take_along_axis(gt_boxes, arg[..., None].repeat(4, -1), axis=1)
    deltas = (bo.get_deltas_from_bboxes(rois, matched) / np.asarray(variances, F32)).astype(F32)
    deltas = np.where(pos[..., None], deltas, F32(0.0)).astype(F32)
    return deltas, labels, pos_cand.sum(axis=-1)


def tree_sum(v):
    """per-thread partials, then a tree: the fixed-order sum a float32 kernel would make"""
    v = np.asarray(v).reshape(-1)
    n = 1
    while n < v.size:
        n *= 2
    buf = np.zeros((n,), v.dtype)
    buf[:v.size] = v
    while n > 1:
        n //= 2
        buf = (buf[:n] + buf[n:2 * n]).astype(v.dtype)
    return buf[0]


def roi_losses_ref(logits, reg, labels, deltas, dtype=np.float64, total=None):
    """-> (reg_loss, cls_loss, grad_logits, grad_reg) in `dtype`; `total`: how the per-row terms are summed (default np.sum in float64,
    tree_sum in float32)"""
    total = total or (tree_sum if dtype == np.float32 else np.sum)
    l, p, t = np.asarray(logits, dtype), np.asarray(reg, dtype), np.asarray(deltas, dtype)
    labels = np.asarray(labels, np.int64)
    B, R, C = l.shape
    one = dtype(1.0)
    kept = (labels >= 0) & (labels < C)
    posm = kept & (labels >= 1)
    safe = np.where(kept, labels, 0)
    m = l.max(axis=-1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=-1, keepdims=True)
    lse = (m + np.log(s))[..., 0]
    ce = lse - np.take_along_axis(l, safe[..., None], axis=-1)[..., 0]
    n_kept, n_pos = max(1, int(kept.sum())), max(1, int(posm.sum()))
    cls_loss = total(np.where(kept, ce, dtype(0.0)).astype(dtype)) / dtype(n_kept)
    pred = np.take_along_axis(p.reshape(B, R, C, 4), safe[..., None, None].repeat(4, -1), axis=2)[:, :, 0, :]
    err = pred - t
    a = np.abs(err)
    q = np.minimum(a, one)
    hub = (dtype(0.5) * q * q + (a - q)).sum(axis=-1)
    reg_loss = total(np.where(posm, hub, dtype(0.0)).astype(dtype)) / dtype(n_pos)
    onehot = (np.arange(C)[None, None, :] == safe[..., None]).astype(dtype)
    g_logits = np.where(kept[..., None], (e / s - onehot) / dtype(n_kept), dtype(0.0)).astype(dtype)
    g_reg = np.zeros((B, R, C, 4), dtype)
    g_pos = np.clip(err, -one, one) / dtype(n_pos)
    bi, ri = np.nonzero(posm)
    g_reg[bi, ri, labels[bi, ri]] = g_pos[bi, ri]
    return reg_loss, cls_loss, g_logits, g_reg.reshape(B, R, 4 * C)


def softmax64(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# (B, R, G, valid gts per image, total_pos, total_neg)
TARGET_CASES = [
    (2, 64, 4, [3, 1], 8, 8),
    (3, 300, 42, [40, 5, 0], 32, 96),            # an image without a gt
    (1, 2000, 8, [8], 128, 128),                 # R above the workgroup size; hundreds of raw positives subsampled to 128
    (2, 37, 1, [1, 1], 4, 4),                    # odd R
]
_CASE_CACHE = {}


def target_case(index):
    """Inputs and restated outputs of TARGET_CASES[index], computed once.  RoIs cycle through a jittered gt, a shifted gt and a random
    box; valid = R on even images, R - R // 3 on odd ones; priorities from [1, 40), so ties are common."""
    if index in _CASE_CACHE:
        return _CASE_CACHE[index]
    B, R, G, ngt, total_pos, total_neg = TARGET_CASES[index]
    rng = np.random.RandomState(100 + index)
    y1x1 = rng.uniform(0.0, 0.6, size=(B, G, 2))
    hw = rng.uniform(0.15, 0.4, size=(B, G, 2))
    gt = np.concatenate([y1x1, y1x1 + hw], axis=-1).astype(F32)
    gt_labels = rng.randint(1, 21, size=(B, G)).astype(np.int32)
    for b in range(B):
        gt[b, ngt[b]:] = 0.0
        gt_labels[b, ngt[b]:] = -1
    rois = np.zeros((B, R, 4), F32)
    for b in range(B):
        for r in range(R):
            kind = r % 3
            if kind == 2 or ngt[b] == 0:
                a = rng.uniform(0.0, 0.7, size=2)
                rois[b, r] = np.concatenate([a, a + rng.uniform(0.05, 0.3, size=2)])
            else:
                g = gt[b, rng.randint(ngt[b])].astype(np.float64)
                h, w = g[2] - g[0], g[3] - g[1]
                if kind == 0:
                    rois[b, r] = g + rng.uniform(-0.08, 0.08, size=4) * np.array([h, w, h, w])
                else:
                    rois[b, r] = g + np.array([h, w, h, w]) * rng.uniform(0.2, 0.9) * rng.choice([-1.0, 1.0])
    valid = np.array([R if b % 2 == 0 else R - R // 3 for b in range(B)], np.int32)
    rpos = rng.randint(1, 40, size=(B, R)).astype(np.int32)
    rneg = rng.randint(1, 40, size=(B, R)).astype(np.int32)
    deltas, labels, raw_pos = roi_targets_ref(rois, valid, gt, gt_labels, total_pos, total_neg, rpos, rneg)
    for a in (rois, valid, gt, gt_labels, rpos, rneg, deltas, labels, raw_pos):
        a.setflags(write=False)
    case = dict(B=B, R=R, G=G, ngt=ngt, total_pos=total_pos, total_neg=total_neg, rois=rois, valid=valid, gt=gt, gt_labels=gt_labels,
                rpos=rpos, rneg=rneg, deltas=deltas, labels=labels, raw_pos=raw_pos)
    _CASE_CACHE[index] = case
    return case


def hand_case():
    """One image of hand-made rows with neg_iou = (0.0, 0.5), and a second image with valid = 0.  Rows of image 0: a RoI equal to a gt,
    two identical RoIs of equal priority, a zero-area RoI, a RoI with a NaN coordinate, a RoI that overlaps nothing, then padding."""
    gt = np.zeros((2, 3, 4), F32)
    gt[0, 0] = [0.1, 0.1, 0.5, 0.5]
    gt[0, 1] = [0.5, 0.5, 0.9, 0.9]                      # label -1: never matched, although row 6 equals it
    gt[0, 2] = [0.1, 0.1, 0.5, 0.5]                      # a copy of gt 0: the first maximum must win
    gt[1, 0] = [0.2, 0.2, 0.6, 0.6]
    gt_labels = np.array([[7, -1, 9], [3, -1, -1]], np.int32)
    rois = np.zeros((2, 9, 4), F32)
    rois[0, 0] = gt[0, 0]
    rois[0, 1] = rois[0, 2] = [0.12, 0.1, 0.5, 0.52]
    rois[0, 3] = [0.3, 0.3, 0.3, 0.3]
    rois[0, 4] = [np.nan, 0.1, 0.5, 0.5]
    rois[0, 5] = [0.6, 0.6, 0.7, 0.7]
    rois[0, 6] = gt[0, 1]
    rois[0, 7] = rois[0, 8] = gt[0, 0]                   # padding rows that would be perfect positives
    rois[1, :] = gt[1, 0]
    valid = np.array([7, 0], np.int32)
    rpos = np.full((2, 9), 5, np.int32)
    rneg = np.full((2, 9), 5, np.int32)
    return dict(rois=rois, valid=valid, gt=gt, gt_labels=gt_labels, rpos=rpos, rneg=rneg, total_pos=2, total_neg=8, neg_iou=(0.0, 0.5))


LOSS_SHAPES = [(2, 64, 21), (8, 300, 21), (2, 2000, 5), (1, 5, 3)]


def loss_case(shape, seed=0):
    """logits ~ 3 N(0,1), labels uniform in [-1, C); then the rows every case must hold: logits [100, -100, ...] with the label on the
    -100, a row of equal logits, labels -1, 0, C - 1 and one label equal to C; residuals on both sides of |e| = 1."""
    B, R, C = shape
    rng = np.random.RandomState(seed + 7 * R + C)
    logits = (3.0 * rng.standard_normal((B, R, C))).astype(F32)
    labels = rng.randint(-1, C, size=(B, R)).astype(np.int32)
    deltas = rng.standard_normal((B, R, 4)).astype(F32)
    reg = (np.tile(deltas, (1, 1, C)) + rng.uniform(-2.0, 2.0, size=(B, R, 4 * C))).astype(F32)
    logits[0, 0, :] = 0.0
    logits[0, 0, 0], logits[0, 0, 1] = 100.0, -100.0
    labels[0, 0] = 1
    logits[0, 1, :] = 1.25
    labels[0, 1] = C - 1
    labels[0, 2], labels[0, 3], labels[0, 4] = -1, 0, C
    reg[0, 1, 4 * (C - 1):4 * C] = deltas[0, 1] + np.array([0.5, -0.5, 1.5, -1.5], F32)
    return logits, reg, labels, deltas


# ---- restatement self-checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(TARGET_CASES)))
def test_target_restatement_counts_and_padding(index):
    c = target_case(index)
    B, R = c["B"], c["R"]
    want = c["total_pos"] + c["total_neg"]
    live = np.arange(R)[None, :] < c["valid"][:, None]
    iou = bo.generate_iou_map(c["rois"], c["gt"])
    best = np.where((c["gt_labels"] >= 1)[:, None, :], iou, 0.0).max(axis=2)
    for b in range(B):
        lab = c["labels"][b]
        n_pos, n_neg = int((lab >= 1).sum()), int((lab == 0).sum())
        neg_cand = int((live[b] & (lab < 1) & (best[b] >= F32(0.1)) & (best[b] < F32(0.5))).sum())
        print("case", index, "image", b, "raw positives", int(c["raw_pos"][b]), "kept", n_pos, "/", n_neg, "negative candidates", neg_cand)
        assert n_pos == min(c["total_pos"], int(c["raw_pos"][b]))
        assert n_pos + n_neg <= want
        assert n_neg == min(want - n_pos, neg_cand)                 # equal to the batch when enough candidates exist
        assert (lab[~live[b]] == -1).all()
        if c["ngt"][b] == 0:
            assert (best[b] == 0).all() and (lab == -1).all()       # IoU 0 everywhere is below neg_iou[0] = 0.1
        assert (c["deltas"][b][lab < 1] == 0).all() and not np.signbit(c["deltas"][b][lab < 1]).any()
    assert np.isfinite(c["deltas"]).all()
    assert (c["deltas"][c["labels"] >= 1] != 0).any(axis=-1).all()
    if index == 0:
        # one image subsamples its positives and fills the batch, the other runs out of negatives: both paths stay covered
        totals = [(c["labels"][b] >= 0).sum() for b in range(B)]
        assert max(totals) == want and min(totals) < want and (c["raw_pos"] > c["total_pos"]).all()
    if index == 2:
        assert c["raw_pos"][0] > 4 * c["total_pos"] and (c["labels"][0] >= 1).sum() == 128 and (c["labels"][0] == 0).sum() == 128


def test_hand_made_rows_restatement():
    h = hand_case()
    deltas, labels, raw = roi_targets_ref(h["rois"], h["valid"], h["gt"], h["gt_labels"], h["total_pos"], h["total_neg"], h["rpos"],
                                          h["rneg"], neg_iou=h["neg_iou"])
    # rows 0, 1, 2 are positive candidates of equal priority: the two of lowest index are kept, with gt 0's label (not its copy's);
    # row 2 then has IoU >= 0.5 and is nothing; the zero-area, NaN, disjoint and invalid-gt rows have IoU 0: negatives under
    # neg_iou[0] = 0; padding rows and the image with valid = 0 stay -1
    assert labels[0].tolist() == [7, 7, -1, 0, 0, 0, 0, -1, -1] and raw.tolist() == [3, 0]
    assert (labels[1] == -1).all() and (deltas[1] == 0).all()
    assert (deltas[0, 0] == 0).all() and (deltas[0, 1] != 0).any() and (deltas[0, 2:] == 0).all()


@pytest.mark.parametrize("shape", [(2, 64, 21), (8, 300, 21), (2, 2000, 5)])
def test_loss_restatement_float32_tree_against_float64(shape):
    logits, reg, labels, deltas = loss_case(shape)
    r64, c64, _, _ = roi_losses_ref(logits, reg, labels, deltas, np.float64)
    r32, c32, _, _ = roi_losses_ref(logits, reg, labels, deltas, np.float32)
    seq = lambda v: np.cumsum(np.asarray(v, np.float32).reshape(-1), dtype=np.float32)[-1]
    rs, cs, _, _ = roi_losses_ref(logits, reg, labels, deltas, np.float32, total=seq)
    print(shape, "tree", abs(r32 - r64) / r64, abs(c32 - c64) / c64, "sequential", abs(rs - r64) / r64, abs(cs - c64) / c64)
    assert r32.dtype == np.float32 and c32.dtype == np.float32
    assert abs(r32 - r64) <= 1e-6 * r64 and abs(c32 - c64) <= 1e-6 * c64


def test_loss_restatement_empty_is_zero():
    logits, reg, labels, deltas = loss_case((1, 5, 3))
    r, c, gl, gr = roi_losses_ref(logits, reg, np.full_like(labels, -1), deltas)
    assert r == 0 and c == 0 and not gl.any() and not gr.any()


def test_loss_restatement_gradients_against_central_differences():
    rng = np.random.RandomState(3)
    B, R, C = 2, 8, 5
    logits = 3.0 * rng.standard_normal((B, R, C))
    labels = rng.randint(-1, C + 1, size=(B, R))
    labels[0, :4] = [-1, 0, C - 1, C]
    deltas = rng.standard_normal((B, R, 4))
    err = rng.uniform(-2.0, 2.0, size=(B, R, 4 * C))
    err = np.where(np.abs(np.abs(err) - 1.0) < 1e-2, 1.1 * err, err)                     # away from the Huber kink at |e| = 1
    reg = np.tile(deltas, (1, 1, C)) + err
    assert (np.abs(err) > 1).any() and (np.abs(err) < 1).any()
    _, _, g_logits, g_reg = roi_losses_ref(logits, reg, labels, deltas)
    h = 1e-6
    for x, g, which in ((logits, g_logits, 1), (reg, g_reg, 0)):
        num = np.zeros_like(x)
        for i in np.ndindex(*x.shape):
            keep = x[i]
            x[i] = keep + h
            up = roi_losses_ref(logits, reg, labels, deltas)[which]
            x[i] = keep - h
            dn = roi_losses_ref(logits, reg, labels, deltas)[which]
            x[i] = keep
            num[i] = (up - dn) / (2 * h)
        assert np.abs(num - g).max() <= 1e-8 + 1e-6 * np.abs(g).max(), which
    assert g_reg.any() and g_logits.any()


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "rpn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rpn_[a-z0-9_]+)\s*\(", code))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in include/rpn_hip.h" % name
        assert hasattr(raw, name), "librpn_hip.so does not export %s" % name
        assert name in L.exported_symbols(), "%s is not bound in tf_rpn_amd/_lib.py" % name
    assert "NO NaN" in header                                 # the header states where rpn_roi_losses departs from rpn_rpn_losses
    assert lib.rpn_abi_version() == 1
    assert lib.rpn_roi_targets_workspace_bytes(0, 5, 5) == 0 and lib.rpn_roi_losses_workspace_bytes(2, 0, 5) == 0
    assert lib.rpn_roi_targets_workspace_bytes(3, 300, 42) >= 2 * 3 * 300 * 4


def _buf(nbytes):
    """host memory, 16-byte aligned: validation precedes device use, so nothing reads it"""
    raw = np.zeros((nbytes + 16,), np.uint8)
    off = (-raw.ctypes.data) % 16
    view = raw[off:off + nbytes]
    return view, L.vp(view.ctypes.data)


def _targets_call(lib, p, B=2, R=8, G=3, total_pos=2, total_neg=2, pos_iou=0.5, neg_lo=0.1, neg_hi=0.5, ws_bytes=None, null=()):
    _keep, var = L.host_floats(VARIANCES)
    a = {k: (None if k in null else p) for k in ("rois", "gt", "lab", "rp", "rn", "deltas", "labels", "ws")}
    need = int(lib.rpn_roi_targets_workspace_bytes(B, R, G))
    return lib.rpn_roi_targets(a["rois"], None, a["gt"], a["lab"], B, R, G, total_pos, total_neg, pos_iou, neg_lo, neg_hi,
                               None if "var" in null else var, a["rp"], a["rn"], a["deltas"], a["labels"], a["ws"],
                               need if ws_bytes is None else ws_bytes, None)


def test_argument_validation_precedes_device_use(lib):
    _keep, p = _buf(1 << 16)
    _keepv, var = L.host_floats(VARIANCES)
    for null in ("rois", "gt", "lab", "var", "rp", "rn", "deltas", "labels"):
        assert _targets_call(lib, p, null=(null,)) == L.RPN_ERR_INVALID, null
        assert b"rpn_roi_targets: null pointer" in lib.rpn_last_error()
    for kw in (dict(B=0), dict(R=0), dict(G=0)):
        assert _targets_call(lib, p, **kw) == L.RPN_ERR_INVALID and b"rpn_roi_targets" in lib.rpn_last_error(), kw
    assert _targets_call(lib, p, G=2049) == L.RPN_ERR_INVALID and b"rpn_roi_targets: G = 2049 > 2048" in lib.rpn_last_error()
    assert _targets_call(lib, p, neg_lo=0.6, neg_hi=0.5) == L.RPN_ERR_INVALID and b"rpn_roi_targets" in lib.rpn_last_error()
    assert _targets_call(lib, p, neg_lo=-0.1) == L.RPN_ERR_INVALID
    assert _targets_call(lib, p, pos_iou=-1.0) == L.RPN_ERR_INVALID
    assert _targets_call(lib, p, total_pos=-1) == L.RPN_ERR_INVALID
    assert _targets_call(lib, p, ws_bytes=16) == L.RPN_ERR_WORKSPACE and b"rpn_roi_targets: workspace" in lib.rpn_last_error()
    assert _targets_call(lib, p, null=("ws",)) == L.RPN_ERR_WORKSPACE

    need = int(lib.rpn_roi_losses_workspace_bytes(2, 8, 5))
    assert need > 0
    assert lib.rpn_roi_losses(None, p, p, p, 2, 8, 5, p, None, None, p, need, None) == L.RPN_ERR_INVALID
    assert b"rpn_roi_losses: null pointer" in lib.rpn_last_error()
    assert lib.rpn_roi_losses(p, p, p, p, 2, 8, 5, None, None, None, p, need, None) == L.RPN_ERR_INVALID
    for dims in ((0, 8, 5), (2, 0, 5), (2, 8, 0)):
        assert lib.rpn_roi_losses(p, p, p, p, dims[0], dims[1], dims[2], p, None, None, p, need, None) == L.RPN_ERR_INVALID
        assert b"rpn_roi_losses" in lib.rpn_last_error()
    assert lib.rpn_roi_losses(p, p, p, p, 2, 8, 5, p, None, None, p, need - 1, None) == L.RPN_ERR_WORKSPACE
    assert b"rpn_roi_losses: workspace" in lib.rpn_last_error()
    assert lib.rpn_roi_losses(p, p, p, p, 2, 8, 5, p, None, None, None, need, None) == L.RPN_ERR_WORKSPACE

    assert lib.rpn_roi_decode_scores(p, None, p, None, var, 2, 8, 5, p, p, None) == L.RPN_ERR_INVALID
    assert b"rpn_roi_decode_scores: null pointer" in lib.rpn_last_error()
    assert lib.rpn_roi_decode_scores(p, None, p, p, None, 2, 8, 5, p, p, None) == L.RPN_ERR_INVALID
    for dims in ((0, 8, 5), (2, 0, 5), (2, 8, 0)):
        assert lib.rpn_roi_decode_scores(p, None, p, p, var, dims[0], dims[1], dims[2], p, p, None) == L.RPN_ERR_INVALID
        assert b"rpn_roi_decode_scores" in lib.rpn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_compute_calls_fail_loudly_without_a_device(lib):
    _keep, p = _buf(1 << 16)
    _keepv, var = L.host_floats(VARIANCES)
    assert _targets_call(lib, p) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    need = int(lib.rpn_roi_losses_workspace_bytes(2, 8, 5))
    assert lib.rpn_roi_losses(p, p, p, p, 2, 8, 5, p, p, p, p, need, None) == L.RPN_ERR_NO_DEVICE
    assert lib.rpn_roi_decode_scores(p, None, p, p, var, 2, 8, 5, p, p, None) == L.RPN_ERR_NO_DEVICE
    c = target_case(3)
    hp = bo.get_hyper_params("vgg16")
    with pytest.raises(RuntimeError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], hp, valid=c["valid"])
    logits, reg, labels, deltas = loss_case((1, 5, 3))
    with pytest.raises(RuntimeError):
        roi_utils.roi_losses(logits, reg, labels, deltas)
    with pytest.raises(RuntimeError):
        roi_utils.roi_detections(c["rois"][:1, :5], reg, logits, VARIANCES)


def test_python_shape_and_argument_errors_come_first():
    """ValueError before the library (or a device) is touched"""
    c = target_case(3)
    hp = bo.get_hyper_params("vgg16")
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"][..., :3], c["gt"], c["gt_labels"], hp)
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"][:1], c["gt_labels"], hp)
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"][:, :0], hp)
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], hp, valid=np.zeros((3,), np.int32))
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], hp, random_pos=c["rpos"][:, :5])
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], hp, neg_iou=(0.6, 0.5))
    logits, reg, labels, deltas = loss_case((1, 5, 3))
    with pytest.raises(ValueError):
        roi_utils.roi_losses(logits, reg[..., :8], labels, deltas)
    with pytest.raises(ValueError):
        roi_utils.roi_losses(logits, reg, labels[:, :4], deltas)
    with pytest.raises(ValueError):
        roi_utils.roi_detections(c["rois"][:1, :5], reg, logits, VARIANCES, score_threshold=0)
    with pytest.raises(ValueError):
        roi_utils.roi_detections(c["rois"][:1, :5], reg, logits[..., :2], VARIANCES)


# ---- kernel budgets ---------------------------------------------------------------------------------------------------------------
def test_roi_head_kernel_budgets(lib):
    """No scratch and no spills in any new kernel (tests/test_host.py holds the whole library to no scratch); the target kernel's
    1024-thread workgroup needs 128 VGPRs or fewer (four waves per SIMD) and its LDS -- the radix histogram plus 1024 staged gt
    boxes -- stays under the 64 KB a workgroup gets without asking."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    names = ["roi_target_kernel", "roi_loss_kernel", "roi_loss_finish_kernel", "roi_loss_grad_kernel", "roi_decode_scores_kernel"]
    for name in names:
        assert name in tab, "librpn_hip.so has no kernel %s" % name
        vgpr, sspill, vspill, scratch, lds, wg = tab[name]
        print(name, "vgpr", vgpr, "sgpr spills", sspill, "lds", lds, "workgroup", wg)
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, sspill, vspill, scratch)
        assert vgpr <= 128
    vgpr, _, _, _, lds, wg = tab["roi_target_kernel"]
    assert wg == 1024 and vgpr <= 128 and lds <= 65536
