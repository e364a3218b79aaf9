"""The proposal-target layer (rpn_roi_sample_targets, roi_utils.sample_roi_targets): what can be checked without a GPU.

``roi_sample_ref`` is the numpy restatement the GPU suite (tests/test_gpu_roi_sample.py) compares against.  It adds nothing to the
arithmetic or the sampling rule: per image it packs the live candidates (live RoIs, then -- with add_gt -- the gt rows that are gt
boxes) into a prefix, calls ``test_roi_head_host.roi_targets_ref`` on that prefix with ``valid`` = the live count, maps the rows
back to candidate indices and writes the kept positives, then the kept negatives, each in ascending candidate index.  Packing keeps
the order, so ties still go to the lower candidate index.  This file checks the restatement against itself, the two C-ABI entries
(declared, exported, bound; arguments validated before any device use; loud failure without a device) and the new kernel's code
object.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_roi_head_host as rh  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402
from test_roi_head_host import lib  # noqa: E402,F401  (fixture)

ROOT = rh.ROOT
F32 = np.float32
NEW_SYMBOLS = ["rpn_roi_sample_targets", "rpn_roi_sample_targets_workspace_bytes"]
SAMPLE = roi_utils.sample_roi_targets            # what the restatement below restates: without it this file has nothing to check


# ---- restatement ----------------------------------------------------------------------------------------------------------------
def candidates(rois, valid, gt_boxes, gt_labels, add_gt):
    """-> (boxes (B,N,4) f32, live (B,N) bool): the RoIs, then (add_gt) the gt rows"""
    rois, gt_boxes = np.asarray(rois, F32), np.asarray(gt_boxes, F32)
    B, R, _ = rois.shape
    live = np.arange(R)[None, :] < (np.full((B,), R) if valid is None else np.clip(np.asarray(valid), 0, R))[:, None]
    if not add_gt:
        return rois, live
    return np.concatenate([rois, gt_boxes], axis=1), np.concatenate([live, np.asarray(gt_labels) >= 1], axis=1)


def roi_sample_ref(rois, valid, gt_boxes, gt_labels, total_pos, total_neg, random_pos, random_neg, add_gt=True, pos_iou=0.5,
                   neg_iou=(0.1, 0.5), variances=rh.VARIANCES):
    """-> dict(rois (B,S,4) f32, deltas (B,S,4) f32, labels (B,S) i32, index (B,S) i32, counts (B,2) i32 [n_sampled, n_pos])"""
    gt_boxes, gt_labels = np.asarray(gt_boxes, F32), np.asarray(gt_labels, np.int32)
    boxes, live = candidates(rois, valid, gt_boxes, gt_labels, add_gt)
    B, N, _ = boxes.shape
    S = total_pos + total_neg
    random_pos, random_neg = np.asarray(random_pos), np.asarray(random_neg)
    assert random_pos.shape == (B, N) and random_neg.shape == (B, N)
    out = dict(rois=np.zeros((B, S, 4), F32), deltas=np.zeros((B, S, 4), F32), labels=np.full((B, S), -1, np.int32),
               index=np.full((B, S), -1, np.int32), counts=np.zeros((B, 2), np.int32))
    for b in range(B):
        idx = np.nonzero(live[b])[0]
        n = idx.size
        packed = np.zeros((1, N, 4), F32)
        rp, rn = np.ones((1, N), np.int32), np.ones((1, N), np.int32)
        packed[0, :n], rp[0, :n], rn[0, :n] = boxes[b, idx], random_pos[b, idx], random_neg[b, idx]
        with np.errstate(all="ignore"):
            d, l, _ = rh.roi_targets_ref(packed, np.array([n]), gt_boxes[b:b + 1], gt_labels[b:b + 1], total_pos, total_neg, rp, rn,
                                         pos_iou=pos_iou, neg_iou=neg_iou, variances=variances)
        assert (l[0, n:] == -1).all()
        order = np.concatenate([np.nonzero(l[0] >= 1)[0], np.nonzero(l[0] == 0)[0]])
        k = order.size
        out["index"][b, :k] = idx[order]
        out["rois"][b, :k] = boxes[b, idx[order]]
        out["deltas"][b, :k] = d[0, order]
        out["labels"][b, :k] = l[0, order]
        out["counts"][b] = [k, int((l[0] >= 1).sum())]
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# (B, R, G, valid gts per image, total_pos, total_neg); the first four are test_roi_head_host.TARGET_CASES
SAMPLE_CASES = list(rh.TARGET_CASES) + [
    (1, 40, 1030, [1030], 16, 16),               # the gts cross the 1024-box LDS chunk and outnumber total_pos
]
HAND = len(SAMPLE_CASES)                         # case number of rh.hand_case()
_CACHE = {}


def _many_gt_case():
    B, R, G, ngt, total_pos, total_neg = SAMPLE_CASES[4]
    rng = np.random.RandomState(104)
    y1x1 = rng.uniform(0.0, 0.8, size=(B, G, 2))
    gt = np.concatenate([y1x1, y1x1 + rng.uniform(0.05, 0.2, size=(B, G, 2))], axis=-1).astype(F32)
    gt_labels = rng.randint(1, 21, size=(B, G)).astype(np.int32)
    rois = np.zeros((B, R, 4), F32)
    for r in range(R):
        # the jittered rows sit on the last gt boxes, 1022 .. 1029: their maximum is found in the second LDS chunk
        g = gt[0, G - 1 - (r // 3) % 8 if r % 3 == 0 else rng.randint(G)].astype(np.float64)
        h, w = g[2] - g[0], g[3] - g[1]
        if r % 3 == 0:
            rois[0, r] = g + rng.uniform(-0.08, 0.08, size=4) * np.array([h, w, h, w])
        elif r % 3 == 1:
            rois[0, r] = g + np.array([h, w, h, w]) * rng.uniform(0.2, 0.9) * rng.choice([-1.0, 1.0])
        else:
            a = rng.uniform(0.0, 0.7, size=2)
            rois[0, r] = np.concatenate([a, a + rng.uniform(0.05, 0.3, size=2)])
    return dict(B=B, R=R, G=G, ngt=ngt, total_pos=total_pos, total_neg=total_neg, rois=rois, valid=np.array([R - 3], np.int32), gt=gt,
                gt_labels=gt_labels, rpos=rng.randint(1, 40, size=(B, R)).astype(np.int32),
                rneg=rng.randint(1, 40, size=(B, R)).astype(np.int32), neg_iou=(0.1, 0.5))


def sample_case(index, add_gt):
    """Inputs and restated outputs of case `index` (HAND = rh.hand_case()), computed once and read-only.  The RoI columns of the
    priorities are the case's own; the gt columns are drawn from the same [1, 40) (the hand case: the same constant), so ties between
    RoIs and gt boxes are common."""
    key = (index, bool(add_gt))
    if key in _CACHE:
        return _CACHE[key]
    if index == HAND:
        c = dict(rh.hand_case())
        c.update(B=c["rois"].shape[0], R=c["rois"].shape[1], G=c["gt"].shape[1])
        gp = gn = np.full((c["B"], c["G"]), 5, np.int32)
    else:
        c = dict(rh.target_case(index)) if index < len(rh.TARGET_CASES) else _many_gt_case()
        c.setdefault("neg_iou", (0.1, 0.5))
        rng = np.random.RandomState(500 + index)
        gp = rng.randint(1, 40, size=(c["B"], c["G"])).astype(np.int32)
        gn = rng.randint(1, 40, size=(c["B"], c["G"])).astype(np.int32)
    c["add_gt"] = bool(add_gt)
    c["rp"] = np.concatenate([c["rpos"], gp], axis=1) if add_gt else np.array(c["rpos"])
    c["rn"] = np.concatenate([c["rneg"], gn], axis=1) if add_gt else np.array(c["rneg"])
    c["N"] = c["R"] + (c["G"] if add_gt else 0)
    c["S"] = c["total_pos"] + c["total_neg"]
    c["ref"] = roi_sample_ref(c["rois"], c["valid"], c["gt"], c["gt_labels"], c["total_pos"], c["total_neg"], c["rp"], c["rn"],
                              add_gt=add_gt, neg_iou=c["neg_iou"])
    for a in list(c["ref"].values()) + [c["rp"], c["rn"]]:
        a.setflags(write=False)
    _CACHE[key] = c
    return c


ALL_CASES = [(i, g) for i in range(HAND + 1) for g in (True, False)]


# ---- restatement self-checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,add_gt", ALL_CASES)
def test_restatement_counts_order_and_padding(index, add_gt):
    c = sample_case(index, add_gt)
    ref, S, R = c["ref"], c["S"], c["R"]
    boxes, live = candidates(c["rois"], c["valid"], c["gt"], c["gt_labels"], add_gt)
    for b in range(c["B"]):
        n, n_pos = (int(v) for v in ref["counts"][b])
        print("case", index, "add_gt", add_gt, "image", b, "sampled", n, "positives", n_pos, "of them gt boxes",
              int((ref["index"][b, :n_pos] >= R).sum()))
        assert 0 <= n_pos <= c["total_pos"] and n_pos <= n <= S
        lab, idx = ref["labels"][b], ref["index"][b]
        assert (lab[:n_pos] >= 1).all() and (lab[n_pos:n] == 0).all()
        assert (np.diff(idx[:n_pos]) > 0).all() and (np.diff(idx[n_pos:n]) > 0).all()          # ascending within each group
        assert (idx[:n] >= 0).all() and (idx[:n] < c["N"]).all() and live[b, idx[:n]].all() and len(set(idx[:n].tolist())) == n
        assert ref["rois"][b, :n].tobytes() == boxes[b, idx[:n]].tobytes()
        assert (lab[n:] == -1).all() and (idx[n:] == -1).all()                                 # padding rows
        for name in ("rois", "deltas"):
            assert not ref[name][b, n:].view(np.uint32).any()
        assert not ref["deltas"][b, n_pos:].view(np.uint32).any()                               # negatives: +0.0
        assert np.isfinite(ref["deltas"][b]).all() and (ref["deltas"][b, :n_pos] != 0).any(axis=-1).sum() >= n_pos - c["G"]
    if index == 1:
        assert ref["counts"][2].tolist() == [0, 0]                                              # the image without a gt
    if index == 2:
        assert ref["counts"][0].tolist() == [256, 128] and (ref["index"][0] >= 1024).any()      # the scan crosses chunks
    if index == 3:
        assert (ref["counts"][:, 0] < S).any()                                                  # fewer candidates than rows
    if index == 4 and add_gt:
        assert ref["counts"][0, 1] == 16 and (ref["index"][0, :16] >= R).sum() >= 8            # the gt candidates are subsampled
    if index == 4 and not add_gt:
        kept = ref["index"][0, :ref["counts"][0, 1]]
        arg = bo.generate_iou_map(c["rois"], c["gt"])[0, kept].argmax(axis=-1)
        assert (arg >= 1024).any() and (arg < 1024).any()                                       # matched in both LDS chunks


@pytest.mark.parametrize("index", range(HAND + 1))
def test_restatement_without_gt_candidates_is_the_scattered_target_restatement(index):
    """add_gt=False: scattering the compact rows back by index gives roi_targets_ref's labels and deltas, bit for bit"""
    c = sample_case(index, False)
    d_full, l_full, _ = rh.roi_targets_ref(c["rois"], c["valid"], c["gt"], c["gt_labels"], c["total_pos"], c["total_neg"], c["rp"], c["rn"],
                                           neg_iou=c["neg_iou"])
    ref = c["ref"]
    labels, deltas = np.full_like(l_full, -1), np.zeros_like(d_full)
    for b in range(c["B"]):
        n = ref["counts"][b, 0]
        labels[b, ref["index"][b, :n]] = ref["labels"][b, :n]
        deltas[b, ref["index"][b, :n]] = ref["deltas"][b, :n]
    assert np.array_equal(labels, l_full) and deltas.tobytes() == d_full.tobytes()


@pytest.mark.parametrize("index", range(HAND + 1))
def test_every_proper_gt_box_is_a_positive_candidate(index):
    """add_gt=True with room for every positive: each valid gt box of non-zero area is kept as a positive with a gt's label -- its own,
    or that of an identical box of lower index"""
    c = sample_case(index, True)
    N, R = c["N"], c["R"]
    ref = roi_sample_ref(c["rois"], c["valid"], c["gt"], c["gt_labels"], N, 0, c["rp"], c["rn"], add_gt=True, neg_iou=c["neg_iou"])
    area = (c["gt"][..., 2] - c["gt"][..., 0]) * (c["gt"][..., 3] - c["gt"][..., 1])
    proper = (c["gt_labels"] >= 1) & (area > 0)
    for b in range(c["B"]):
        n_pos = ref["counts"][b, 1]
        kept = set(ref["index"][b, :n_pos].tolist())
        want = set((R + np.nonzero(proper[b])[0]).tolist())
        assert want <= kept, (b, sorted(want - kept))
        assert n_pos >= int(proper[b].sum())
    if index == HAND:
        # image 0: gt 0 and its copy gt 2 both match gt 0 (the first maximum); gt 1 has label -1 and is no candidate.  Image 1 has
        # valid = 0, so its one gt box is its only candidate
        b0 = ref["index"][0, :ref["counts"][0, 1]].tolist()
        assert R + 0 in b0 and R + 2 in b0 and R + 1 not in ref["index"][0].tolist()
        assert ref["labels"][0, b0.index(R + 2)] == 7
        assert ref["counts"][1].tolist() == [1, 1] and ref["index"][1, 0] == R and ref["labels"][1, 0] == 3
        assert not ref["deltas"][1, 0].any()                                                   # a box encoded against itself


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
    assert "rpn_roi_sample_targets:" in header                # the contract is written out beside rpn_roi_targets'
    assert lib.rpn_abi_version() == 1
    assert lib.rpn_roi_sample_targets_workspace_bytes(0, 5, 5, 1) == 0 and lib.rpn_roi_sample_targets_workspace_bytes(2, 5, 0, 0) == 0
    assert lib.rpn_roi_sample_targets_workspace_bytes(3, 300, 42, 1) >= 2 * 3 * 342 * 4
    assert lib.rpn_roi_sample_targets_workspace_bytes(3, 300, 42, 0) == lib.rpn_roi_targets_workspace_bytes(3, 300, 42)


def _sample_call(lib, p, B=2, R=8, G=3, add_gt=1, total_pos=2, total_neg=2, S=None, pos_iou=0.5, neg_lo=0.1, neg_hi=0.5, ws_bytes=None,
                 null=()):
    _keep, var = L.host_floats(rh.VARIANCES)
    names = ("rois", "gt", "lab", "rp", "rn", "out_rois", "out_labels", "out_deltas", "out_index", "out_counts", "ws")
    a = {k: (None if k in null else p) for k in names}
    need = int(lib.rpn_roi_sample_targets_workspace_bytes(B, R, G, add_gt))
    return lib.rpn_roi_sample_targets(a["rois"], None, a["gt"], a["lab"], B, R, G, add_gt, total_pos, total_neg, pos_iou, neg_lo, neg_hi,
                                      None if "var" in null else var, a["rp"], a["rn"], total_pos + total_neg if S is None else S,
                                      a["out_rois"], a["out_labels"], a["out_deltas"], a["out_index"], a["out_counts"], a["ws"],
                                      need if ws_bytes is None else ws_bytes, None)


def test_argument_validation_precedes_device_use(lib):
    _keep, p = rh._buf(1 << 16)
    for null in ("rois", "gt", "lab", "var", "rp", "rn", "out_rois", "out_labels", "out_deltas", "out_index", "out_counts"):
        assert _sample_call(lib, p, null=(null,)) == L.RPN_ERR_INVALID, null
        assert b"rpn_roi_sample_targets: null pointer" in lib.rpn_last_error()
    for kw in (dict(B=0), dict(R=0), dict(G=0)):
        assert _sample_call(lib, p, **kw) == L.RPN_ERR_INVALID and b"rpn_roi_sample_targets" in lib.rpn_last_error(), kw
    assert _sample_call(lib, p, G=2049) == L.RPN_ERR_INVALID and b"rpn_roi_sample_targets: G = 2049 > 2048" in lib.rpn_last_error()
    for kw in (dict(S=5), dict(S=3), dict(total_pos=0, total_neg=0)):
        assert _sample_call(lib, p, **kw) == L.RPN_ERR_INVALID, kw
        assert b"rpn_roi_sample_targets: S = " in lib.rpn_last_error()
    assert _sample_call(lib, p, neg_lo=0.6, neg_hi=0.5) == L.RPN_ERR_INVALID and b"rpn_roi_sample_targets" in lib.rpn_last_error()
    assert _sample_call(lib, p, neg_lo=-0.1) == L.RPN_ERR_INVALID
    assert _sample_call(lib, p, pos_iou=-1.0) == L.RPN_ERR_INVALID
    assert _sample_call(lib, p, total_pos=-1, S=1) == L.RPN_ERR_INVALID
    assert _sample_call(lib, p, ws_bytes=16) == L.RPN_ERR_WORKSPACE and b"rpn_roi_sample_targets: workspace" in lib.rpn_last_error()
    assert _sample_call(lib, p, null=("ws",)) == L.RPN_ERR_WORKSPACE
    # the workspace of add_gt = 0 is too small for add_gt = 1
    small = int(lib.rpn_roi_sample_targets_workspace_bytes(2, 300, 42, 0))
    assert _sample_call(lib, p, R=300, G=42, add_gt=1, ws_bytes=small) == L.RPN_ERR_WORKSPACE


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_the_call_fails_loudly_without_a_device(lib):
    _keep, p = rh._buf(1 << 16)
    assert _sample_call(lib, p) == L.RPN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.rpn_last_error()
    c = sample_case(3, True)
    with pytest.raises(RuntimeError):
        SAMPLE(c["rois"], c["gt"], c["gt_labels"], bo.get_hyper_params("vgg16"), valid=c["valid"])


def test_python_shape_and_argument_errors_come_first():
    """ValueError before the library (or a device) is touched"""
    c = sample_case(3, True)
    hp = bo.get_hyper_params("vgg16")
    call = SAMPLE
    with pytest.raises(ValueError):
        call(c["rois"][..., :3], c["gt"], c["gt_labels"], hp)
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"][:1], c["gt_labels"], hp)
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"], c["gt_labels"][:, :0], hp)
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"], c["gt_labels"], hp, valid=np.zeros((3,), np.int32))
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"], c["gt_labels"], hp, neg_iou=(0.6, 0.5))
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"], c["gt_labels"], hp, total_pos=-1)
    with pytest.raises(ValueError):
        call(c["rois"], c["gt"], c["gt_labels"], hp, total_pos=0, total_neg=0)
    # a priority tensor must be (B, N): (B, R) priorities belong to add_gt=False, (B, R + G) ones to add_gt=True
    with pytest.raises(ValueError, match="random_pos"):
        call(c["rois"], c["gt"], c["gt_labels"], hp, random_pos=c["rpos"])
    with pytest.raises(ValueError, match="random_neg"):
        call(c["rois"], c["gt"], c["gt_labels"], hp, add_gt=False, random_neg=c["rn"])


# ---- kernel budget ----------------------------------------------------------------------------------------------------------------
def test_roi_sample_kernel_code_object(lib):
    """No scratch, no spills; the 1024-thread workgroup needs 128 VGPRs or fewer, and the LDS -- the radix histogram, 1024 staged gt
    boxes and the scan's wave totals -- stays under the 64 KB a workgroup gets without asking.  The neighbouring kernel is still there
    with its workgroup size."""
    import codeobj
    tab = codeobj.table(L.LIB_PATH)
    assert "roi_sample_kernel" in tab, "librpn_hip.so has no kernel roi_sample_kernel"
    vgpr, sspill, vspill, scratch, lds, wg = tab["roi_sample_kernel"]
    print("roi_sample_kernel vgpr", vgpr, "spills", sspill, vspill, "scratch", scratch, "lds", lds, "workgroup", wg)
    assert sspill == 0 and vspill == 0 and scratch == 0
    assert wg == 1024 and vgpr <= 128 and lds <= 65536
    assert tab["roi_target_kernel"][5] == 1024
