"""Second-stage targets, losses and detections on the GPU against the numpy restatements of tests/test_roi_head_host.py.

Tolerances (none of them comes from what the kernels give):
  * roi_labels: bit-equal.  roi_deltas: 2e-6 * max(1, max|ref|), the bar tests/test_gpu_bbox.py holds the RPN targets to (the device's
    logf is not numpy's); rows that are zero in the restatement are +0.0 bit for bit.
  * losses: 1e-6 relative to the float64 restatement (the bar of tests/test_train.py for the RPN losses).
  * gradients: 2e-6 * max|g|: a softmax entry of C <= 21 terms carries at most about (2 + 2 + 10 + 1) * 2^-24 relative error (the
    subtraction, expf, the sum, the divide), just under 1e-6, and the scale adds one more rounding.
  * scores: 2e-6 absolute against a float64 softmax, by the same bound (p <= 1).  Boxes: bit-equal to get_bboxes_from_deltas.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_roi_head_host as rh  # noqa: E402
import test_train_backbone as vb  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd.utils import bbox_utils, roi_utils  # noqa: E402
from test_roi_head_host import lib  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu
HP = bo.get_hyper_params("vgg16")


def run_targets(c, **kw):
    args = dict(valid=c["valid"], total_pos=c["total_pos"], total_neg=c["total_neg"], random_pos=c["rpos"], random_neg=c["rneg"])
    args.update(kw)
    return roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], HP, **args)


# ---- targets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(rh.TARGET_CASES)))
def test_targets_match_the_restatement(lib, index):
    c = rh.target_case(index)
    deltas, labels = run_targets(c)
    assert isinstance(deltas, np.ndarray) and deltas.dtype == np.float32 and labels.dtype == np.int32
    assert deltas.shape == c["deltas"].shape and labels.shape == c["labels"].shape
    err = np.abs(deltas - c["deltas"]).max()
    bar = 2e-6 * max(1.0, np.abs(c["deltas"]).max())
    print("case", index, "labels differ at", int((labels != c["labels"]).sum()), "deltas err", err, "bar", bar)
    assert np.array_equal(labels, c["labels"])
    assert err <= bar
    zero = (c["deltas"] == 0).all(axis=-1)
    assert deltas[zero].view(np.uint32).max() == 0                     # +0.0, bit for bit
    # the same call again, and through torch tensors: the same bits
    d2, l2 = run_targets(c)
    assert d2.tobytes() == deltas.tobytes() and l2.tobytes() == labels.tobytes()
    d3, l3 = roi_utils.calculate_roi_targets(torch.from_numpy(c["rois"].copy()).cuda(), torch.from_numpy(c["gt"].copy()), c["gt_labels"], HP,
                                             valid=torch.from_numpy(c["valid"].copy()).cuda(), total_pos=c["total_pos"],
                                             total_neg=c["total_neg"], random_pos=c["rpos"], random_neg=c["rneg"])
    assert d3.is_cuda and l3.is_cuda and l3.dtype == torch.int32
    assert d3.cpu().numpy().tobytes() == deltas.tobytes() and l3.cpu().numpy().tobytes() == labels.tobytes()


def test_targets_without_valid_treat_every_row_as_live(lib):
    c = rh.target_case(3)
    ref_d, ref_l, _ = rh.roi_targets_ref(c["rois"], None, c["gt"], c["gt_labels"], c["total_pos"], c["total_neg"], c["rpos"], c["rneg"])
    deltas, labels = run_targets(c, valid=None)
    assert np.array_equal(labels, ref_l) and not np.array_equal(labels, c["labels"])
    assert np.abs(deltas - ref_d).max() <= 2e-6 * max(1.0, np.abs(ref_d).max())


def test_targets_hand_made_rows(lib):
    h = rh.hand_case()
    ref_d, ref_l, _ = rh.roi_targets_ref(h["rois"], h["valid"], h["gt"], h["gt_labels"], h["total_pos"], h["total_neg"], h["rpos"],
                                         h["rneg"], neg_iou=h["neg_iou"])
    deltas, labels = roi_utils.calculate_roi_targets(h["rois"], h["gt"], h["gt_labels"], HP, valid=h["valid"], total_pos=h["total_pos"],
                                                     total_neg=h["total_neg"], neg_iou=h["neg_iou"], random_pos=h["rpos"],
                                                     random_neg=h["rneg"])
    print(labels.tolist())
    assert labels[0].tolist() == [7, 7, -1, 0, 0, 0, 0, -1, -1] and (labels[1] == -1).all()
    assert np.array_equal(labels, ref_l)
    assert np.abs(deltas - ref_d).max() <= 2e-6 * max(1.0, np.abs(ref_d).max())
    assert deltas[labels < 1].view(np.uint32).max() == 0
    with pytest.raises(ValueError):
        roi_utils.calculate_roi_targets(h["rois"], h["gt"], h["gt_labels"], HP, random_pos=np.zeros((2, 9), np.int32))


def test_targets_default_priorities_counts(lib):
    c = rh.target_case(1)
    B, R = c["B"], c["R"]
    torch.manual_seed(0)
    deltas, labels = roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], HP, valid=c["valid"], total_pos=c["total_pos"],
                                                     total_neg=c["total_neg"])
    live = np.arange(R)[None, :] < c["valid"][:, None]
    iou = bo.generate_iou_map(c["rois"], c["gt"])
    best = np.where((c["gt_labels"] >= 1)[:, None, :], iou, 0.0).max(axis=2)
    want = c["total_pos"] + c["total_neg"]
    for b in range(B):
        n_pos, n_neg = int((labels[b] >= 1).sum()), int((labels[b] == 0).sum())
        neg_cand = int((live[b] & (best[b] >= np.float32(0.1)) & (best[b] < np.float32(0.5))).sum())
        assert n_pos == min(c["total_pos"], int(c["raw_pos"][b])) and n_neg == min(want - n_pos, neg_cand), (b, n_pos, n_neg)
        assert (best[b][labels[b] >= 1] > 0.5).all() and (labels[b][~live[b]] == -1).all()
    assert (deltas[labels < 1] == 0).all() and np.isfinite(deltas).all()
    assert not np.array_equal(labels, c["labels"])                      # (another draw than the case's priorities)


# ---- losses -----------------------------------------------------------------------------------------------------------------------
def gpu_losses_and_grads(logits, reg, labels, deltas):
    lt = torch.from_numpy(logits).cuda().requires_grad_()
    rt = torch.from_numpy(reg).cuda().requires_grad_()
    r, c = roi_utils.roi_losses(lt, rt, torch.from_numpy(labels).cuda(), torch.from_numpy(deltas).cuda())
    assert r.dim() == 0 and c.dim() == 0 and r.is_cuda and c.is_cuda
    r.backward(retain_graph=True)
    c.backward()
    return r.item(), c.item(), lt.grad.cpu().numpy(), rt.grad.cpu().numpy()


@pytest.mark.parametrize("shape", rh.LOSS_SHAPES)
def test_losses_and_gradients_match_float64(lib, shape):
    logits, reg, labels, deltas = rh.loss_case(shape)
    C = shape[2]
    assert {-1, 0, C - 1, C} <= set(labels.reshape(-1).tolist())
    r64, c64, gl64, gr64 = rh.roi_losses_ref(logits, reg, labels, deltas)
    r, c, gl, gr = gpu_losses_and_grads(logits, reg, labels, deltas)
    e_gl, e_gr = np.abs(gl - gl64).max(), np.abs(gr - gr64).max()
    print(shape, "reg", r, "rel", abs(r - r64) / r64, "cls", c, "rel", abs(c - c64) / c64, "grad_logits", e_gl / np.abs(gl64).max(),
          "grad_reg", e_gr / np.abs(gr64).max())
    assert abs(r - r64) <= 1e-6 * r64 and abs(c - c64) <= 1e-6 * c64
    assert e_gl <= 2e-6 * np.abs(gl64).max() and e_gr <= 2e-6 * np.abs(gr64).max()
    assert (gl[gl64 == 0] == 0).all() and (gr[gr64 == 0] == 0).all()    # ignored rows and the other classes: written, and zero
    # without autograd: the same losses, bit for bit, as numpy scalars for numpy input; and twice the same bits
    r_np, c_np = roi_utils.roi_losses(logits, reg, labels, deltas)
    assert isinstance(r_np, np.float32) and isinstance(c_np, np.float32)
    assert r_np == np.float32(r) and c_np == np.float32(c)
    r2, c2, gl2, gr2 = gpu_losses_and_grads(logits, reg, labels, deltas)
    assert (r2, c2) == (r, c) and gl2.tobytes() == gl.tobytes() and gr2.tobytes() == gr.tobytes()


def test_losses_with_nothing_kept_are_zero(lib):
    logits, reg, labels, deltas = rh.loss_case((2, 64, 21))
    r, c, gl, gr = gpu_losses_and_grads(logits, reg, np.full_like(labels, -1), deltas)
    assert r == 0.0 and c == 0.0 and not gl.any() and not gr.any()
    only_background = np.zeros_like(labels)
    r, c, gl, gr = gpu_losses_and_grads(logits, reg, only_background, deltas)
    assert r == 0.0 and c > 0.0 and gl.any() and not gr.any()


def test_losses_under_autograd_scale_the_library_gradients(lib):
    logits, reg, labels, deltas = rh.loss_case((2, 64, 21))
    _, _, gl, gr = gpu_losses_and_grads(logits, reg, labels, deltas)
    lt = torch.from_numpy(logits).cuda().requires_grad_()
    rt = torch.from_numpy(reg).cuda().requires_grad_()
    lab, dt = torch.from_numpy(labels).cuda(), torch.from_numpy(deltas).cuda().requires_grad_()
    r, c = roi_utils.roi_losses(lt, rt, lab, dt)
    (r + 2 * c).backward()
    assert np.array_equal(lt.grad.cpu().numpy(), 2 * gl) and np.array_equal(rt.grad.cpu().numpy(), gr)
    assert dt.grad is None                                               # labels and deltas get no gradient
    lt.grad = None
    r, c = roi_utils.roi_losses(lt, rt.detach(), lab, dt.detach())      # one prediction alone
    (3 * c + r).backward()
    assert np.array_equal(lt.grad.cpu().numpy(), 3 * gl)
    with torch.no_grad():
        r, c = roi_utils.roi_losses(lt, rt, lab, dt)
    assert not r.requires_grad and not c.requires_grad


# ---- decode and scores --------------------------------------------------------------------------------------------------------------
def detection_case(B, R, C, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.0, 0.7, size=(B, R, 2))
    rois = np.concatenate([a, a + rng.uniform(0.05, 0.3, size=(B, R, 2))], axis=-1).astype(np.float32)
    reg = rng.standard_normal((B, R, 4 * C)).astype(np.float32)
    logits = (3.0 * rng.standard_normal((B, R, C))).astype(np.float32)
    valid = np.array([R if b % 2 == 0 else R - R // 3 for b in range(B)], np.int32)
    return rois, reg, logits, valid


@pytest.mark.parametrize("shape", [(2, 64, 5), (1, 37, 21)])
def test_decode_scores(lib, shape):
    B, R, C = shape
    rois, reg, logits, valid = detection_case(B, R, C, seed=11)
    if B == 1:
        valid = np.array([R - 5], np.int32)
    boxes, scores = roi_utils.roi_decode_scores(rois, reg, logits, rh.VARIANCES, valid=valid)
    assert boxes.shape == (B, R, C, 4) and scores.shape == (B, R, C)
    ref_boxes = bbox_utils.get_bboxes_from_deltas(np.repeat(rois, C, axis=1), reg.reshape(B, R * C, 4), variances=rh.VARIANCES)
    assert boxes.tobytes() == np.asarray(ref_boxes).tobytes()
    live = np.arange(R)[None, :] < valid[:, None]
    p = rh.softmax64(logits)
    err = np.abs(scores - p)[live][:, 1:].max()
    print(shape, "score err", err)
    assert err <= 2e-6
    assert scores[..., 0].view(np.uint32).max() == 0 and scores[~live].view(np.uint32).max() == 0
    assert (scores[live][:, 1:] > 0).all()
    b2, s2 = roi_utils.roi_decode_scores(rois, reg, logits, rh.VARIANCES)      # every row live
    assert b2.tobytes() == boxes.tobytes() and np.abs(s2 - p)[..., 1:].max() <= 2e-6 and not s2[..., 0].any()


def test_roi_detections_match_the_nms_restatement(lib):
    B, R, C = 2, 64, 5
    rois, reg, logits, valid = detection_case(B, R, C, seed=12)
    reg *= 0.5
    kw = dict(max_output_size_per_class=10, max_total_size=20, iou_threshold=0.5, score_threshold=0.3)
    got = roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, valid=valid, return_indices=True, **kw)
    boxes, scores = roi_utils.roi_decode_scores(rois, reg, logits, rh.VARIANCES, valid=valid)
    ref = bo.non_max_suppression(boxes, scores, return_indices=True, **kw)
    print("valid detections", got[3].tolist())
    assert got[3].min() > 0 and np.array_equal(got[3], ref[3])
    assert np.array_equal(got[4], ref[4]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    live_idx = got[4][got[4] >= 0]
    assert (got[2][got[4] >= 0] >= 1).all() and len(live_idx)             # never background
    for b in range(B):
        assert (got[4][b] < valid[b]).all()                               # never a padding row
    four = roi_utils.roi_detections(torch.from_numpy(rois).cuda(), torch.from_numpy(reg).cuda(), torch.from_numpy(logits).cuda(),
                                    rh.VARIANCES, valid=torch.from_numpy(valid).cuda(), **kw)
    assert len(four) == 4 and four[0].is_cuda and np.array_equal(four[0].cpu().numpy(), got[0])
    with pytest.raises(ValueError):
        roi_utils.roi_detections(rois, reg, logits, rh.VARIANCES, score_threshold=0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_joint_step_with_targets_pool_head_and_losses(lib):
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    B, C, M = 2, 21, 32
    imgs, deltas, labels = vb.batch(hp, B, seed=5)
    model = vb.make_model(hp, B)
    model.compile(learning_rate=1e-5, train_backbone=True)
    anchors = bbox_utils.generate_anchors(hp)
    rng = np.random.RandomState(2)
    a = rng.uniform(0.0, 0.5, size=(B, 6, 2))
    gt_host = np.concatenate([a, a + rng.uniform(0.3, 0.5, size=(B, 6, 2))], axis=-1).astype(np.float32)
    gt_host[:, 0] = [0.05, 0.05, 0.95, 0.95]                    # at img_size 96 every anchor is a large part of the image: positives exist
    gt = torch.from_numpy(gt_host).cuda()
    gt_labels = torch.from_numpy(rng.randint(1, C, size=(B, 6)).astype(np.int32)).cuda()
    gt_labels[:, 5] = -1
    rp = torch.from_numpy(rng.randint(1, 1000, size=(B, M)).astype(np.int32)).cuda()
    rn = torch.from_numpy(rng.randint(1, 1000, size=(B, M)).astype(np.int32)).cuda()
    torch.manual_seed(0)
    head = torch.nn.Linear(2 * 2 * 512, 5 * C).cuda()
    seen = {}

    def second_stage(feat, reg, cls):
        boxes, _, _, valid = bbox_utils.decode_and_nms(anchors, reg.reshape(B, -1, 4), cls.reshape(B, -1), hp["variances"], M,
                                                       iou_threshold=0.7)
        roi_deltas, roi_labels = roi_utils.calculate_roi_targets(boxes, gt, gt_labels, hp, valid=valid, total_pos=8, total_neg=8,
                                                                 pos_iou=0.2, neg_iou=(0.0, 0.2), random_pos=rp, random_neg=rn)
        pooled = roi_utils.roi_pooling(feat, boxes, (2, 2), valid=valid)
        out = head(pooled.flatten(2))
        reg_loss, cls_loss = roi_utils.roi_losses(out[..., :C], out[..., C:], roi_labels, roi_deltas)
        seen.update(feat=feat, pooled=pooled.detach(), labels=roi_labels, deltas=roi_deltas, reg=reg_loss.detach(), cls=cls_loss.detach(),
                    valid=valid)
        return reg_loss + cls_loss

    out = model.train_on_batch(imgs, (deltas, labels), second_stage=second_stage)
    lab = seen["labels"].cpu().numpy()
    print("losses", out, "valid", seen["valid"].tolist(), "positives", int((lab >= 1).sum()), "negatives", int((lab == 0).sum()))
    assert len(out) == 4 and np.isfinite(out).all()
    assert out[3] == float((seen["reg"] + seen["cls"]).item())
    assert (lab >= 1).any() and float(seen["reg"]) > 0 and float(seen["cls"]) > 0
    assert seen["feat"].grad is not None and seen["feat"].grad.abs().max().item() > 0
    # the head's gradients against a float64 torch replay of the loss part
    W = head.weight.detach().double().requires_grad_()
    bias = head.bias.detach().double().requires_grad_()
    o = seen["pooled"].double().flatten(2) @ W.t() + bias
    lab_t, d_t = seen["labels"].long(), seen["deltas"].double()
    kept, posm = lab_t >= 0, lab_t >= 1
    ce = torch.nn.functional.cross_entropy(o[..., :C][kept], lab_t[kept], reduction="sum") / max(1, int(kept.sum()))
    pred = o[..., C:].reshape(B, M, C, 4)[posm][torch.arange(int(posm.sum())), lab_t[posm]]
    hub = torch.nn.functional.smooth_l1_loss(pred, d_t[posm], reduction="sum", beta=1.0) / max(1, int(posm.sum()))
    (ce + hub).backward()
    assert abs((ce + hub).item() - out[3]) <= 1e-5 * abs(out[3])
    for got, ref in ((head.weight.grad, W.grad), (head.bias.grad, bias.grad)):
        err = (got.double() - ref).abs().max().item()
        print("head gradient err", err, "of", ref.abs().max().item())
        assert err <= 1e-5 * ref.abs().max().item()
