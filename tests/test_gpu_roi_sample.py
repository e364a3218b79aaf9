"""The proposal-target layer on the GPU (roi_utils.sample_roi_targets -> rpn_roi_sample_targets) against the numpy restatement of
tests/test_roi_sample_host.py, against the existing entry, and in front of the pool, the head and the losses.

Tolerances (none of them comes from what the kernel gives):
  * labels, index, counts: bit-equal.  rois_s: bit-equal to the gathered candidates (a NaN coordinate included).
  * deltas: 2e-6 * max(1, max|ref|), the bar tests/test_gpu_roi_head.py holds the targets to (the device's logf is not numpy's); the
    deltas of negatives and padding rows are +0.0 bit for bit.
  * against calculate_roi_targets (add_gt=False, same priorities): byte for byte, the two kernels run the same arithmetic.
  * downstream: logits and box deltas of a sampled row are bit-equal to the same RoI's in a run over every candidate (the head's
    contract: a row's outputs do not depend on M); the two losses agree to 1e-6 relative (the same rows in another float64 sum
    order; the loss bar of tests/test_gpu_roi_head.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_roi_sample_host as sh  # noqa: E402
from oracle import bbox_oracle as bo  # noqa: E402
from tf_rpn_amd.models.detection_head import DetectionHead  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402
from test_roi_head_host import lib  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu
HP = bo.get_hyper_params("vgg16")


def run_sample(c, **kw):
    args = dict(valid=c["valid"], add_gt=c["add_gt"], total_pos=c["total_pos"], total_neg=c["total_neg"], neg_iou=c["neg_iou"],
                random_pos=c["rp"], random_neg=c["rn"], return_index=True)
    args.update(kw)
    return roi_utils.sample_roi_targets(c["rois"], c["gt"], c["gt_labels"], HP, **args)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("index,add_gt", sh.ALL_CASES)
def test_sample_matches_the_restatement(lib, index, add_gt):
    c = sh.sample_case(index, add_gt)
    ref, B, S = c["ref"], c["B"], c["S"]
    got = run_sample(c)
    assert len(got) == 5 and all(isinstance(a, np.ndarray) for a in got)
    rois_s, deltas, labels, counts, idx = got
    assert rois_s.shape == (B, S, 4) and deltas.shape == (B, S, 4) and labels.shape == (B, S) and idx.shape == (B, S)
    assert counts.shape == (B, 2)
    assert rois_s.dtype == np.float32 and deltas.dtype == np.float32
    assert labels.dtype == np.int32 and idx.dtype == np.int32 and counts.dtype == np.int32
    err = np.abs(deltas - ref["deltas"]).max()
    bar = 2e-6 * max(1.0, np.abs(ref["deltas"]).max())
    print("case", index, "add_gt", add_gt, "counts", counts.tolist(), "labels differ at", int((labels != ref["labels"]).sum()),
          "index differs at", int((idx != ref["index"]).sum()), "deltas err", err, "bar", bar)
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(idx, ref["index"])
    assert np.array_equal(labels, ref["labels"])
    assert bits(rois_s) == bits(ref["rois"])                                   # the gathered candidates, padding rows +0.0
    assert err <= bar
    zero = labels < 1                                                          # negatives and padding
    assert not deltas[zero].view(np.uint32).any()
    assert len(run_sample(c, return_index=False)) == 4
    # the same call again, and through torch tensors: the same bits
    again = run_sample(c)
    assert all(bits(a) == bits(g) for a, g in zip(again, got))
    t = run_sample(dict(c, rois=torch.from_numpy(c["rois"].copy()).cuda().requires_grad_(), gt=torch.from_numpy(c["gt"].copy()),
                        gt_labels=torch.from_numpy(c["gt_labels"].copy()).cuda()),
                   valid=torch.from_numpy(c["valid"].copy()).cuda(), random_pos=torch.from_numpy(c["rp"].copy()).cuda())
    assert all(a.is_cuda and not a.requires_grad for a in t) and t[2].dtype == torch.int32 and t[3].dtype == torch.int32
    assert all(bits(a.cpu().numpy()) == bits(g) for a, g in zip(t, got))


@pytest.mark.parametrize("index", range(sh.HAND + 1))
def test_scattered_sample_is_calculate_roi_targets(lib, index):
    """add_gt=False, the same priorities: the compact rows scattered back by index are the existing entry's output byte for byte, and
    the rows absent from the sample are exactly its -1 rows"""
    c = sh.sample_case(index, False)
    full_d, full_l = roi_utils.calculate_roi_targets(c["rois"], c["gt"], c["gt_labels"], HP, valid=c["valid"], total_pos=c["total_pos"],
                                                     total_neg=c["total_neg"], neg_iou=c["neg_iou"], random_pos=c["rp"],
                                                     random_neg=c["rn"])
    _rois_s, deltas, labels, counts, idx = run_sample(c)
    lab, dl = np.full_like(full_l, -1), np.zeros_like(full_d)
    sampled = np.zeros(full_l.shape, bool)
    for b in range(c["B"]):
        n = counts[b, 0]
        assert (idx[b, :n] >= 0).all() and (idx[b, n:] == -1).all()
        lab[b, idx[b, :n]] = labels[b, :n]
        dl[b, idx[b, :n]] = deltas[b, :n]
        sampled[b, idx[b, :n]] = True
        assert counts[b, 1] == (full_l[b] >= 1).sum() and n == (full_l[b] >= 0).sum()
    assert bits(lab) == bits(full_l) and bits(dl) == bits(full_d)
    assert np.array_equal(~sampled, full_l == -1)


def test_default_priorities_counts_and_no_duplicate(lib):
    c = sh.sample_case(1, True)
    torch.manual_seed(0)
    rois_s, deltas, labels, counts, idx = run_sample(c, random_pos=None, random_neg=None)
    # under the default thresholds the two candidate sets are disjoint, so the counts do not depend on the draw
    assert np.array_equal(counts, c["ref"]["counts"]) and counts[2].tolist() == [0, 0]
    boxes, live = sh.candidates(c["rois"], c["valid"], c["gt"], c["gt_labels"], True)
    for b in range(c["B"]):
        n, n_pos = counts[b]
        row = idx[b, :n]
        assert len(set(row.tolist())) == n and live[b, row].all()
        assert (np.diff(row[:n_pos]) > 0).all() and (np.diff(row[n_pos:]) > 0).all()
        assert (labels[b, :n_pos] >= 1).all() and (labels[b, n_pos:n] == 0).all() and (labels[b, n:] == -1).all()
        assert bits(rois_s[b, :n]) == bits(boxes[b, row]) and not rois_s[b, n:].view(np.uint32).any()
    assert not deltas[labels < 1].view(np.uint32).any() and np.isfinite(deltas).all()
    assert not np.array_equal(idx, c["ref"]["index"])                          # (another draw than the case's priorities)
    with pytest.raises(ValueError):
        run_sample(c, random_pos=np.zeros((c["B"], c["N"]), np.int32))         # priorities must be >= 1


def test_sampled_batch_through_pool_head_and_losses(lib):
    """Path A: sample, pool the S sampled rows with valid = counts[:, 0], run the head.  Path B: pool every candidate (RoIs ++ gts),
    run the head, gather the sampled rows by index."""
    c = sh.sample_case(0, True)
    B, R, G, C = c["B"], c["R"], c["G"], 5
    gt_labels = np.where(c["gt_labels"] >= 1, (c["gt_labels"] - 1) % (C - 1) + 1, c["gt_labels"]).astype(np.int32)      # classes 1 .. 4
    rng = np.random.RandomState(9)
    feat = torch.from_numpy(rng.standard_normal((B, 9, 9, 8)).astype(np.float32)).cuda()
    head = DetectionHead(C, (2, 2), 8, (16, 16), seed=3)
    rois_s, deltas_s, labels_s, counts, idx = (torch.from_numpy(a).cuda() for a in run_sample(dict(c, gt_labels=gt_labels)))
    cand = torch.from_numpy(np.concatenate([c["rois"], c["gt"]], axis=1)).cuda()
    with torch.no_grad():
        logits_a, reg_a = head(roi_utils.roi_pooling(feat, rois_s, (2, 2), valid=counts[:, 0]))
        logits_b, reg_b = head(roi_utils.roi_pooling(feat, cand, (2, 2)))
    full_labels = torch.full((B, R + G), -1, dtype=torch.int32, device="cuda")
    full_deltas = torch.zeros((B, R + G, 4), dtype=torch.float32, device="cuda")
    n_pos = 0
    for b in range(B):
        n = int(counts[b, 0])
        assert 0 < int(counts[b, 1]) < n
        n_pos += int((labels_s[b, :n] >= 1).sum())
        row = idx[b, :n].long()
        assert bits(logits_a[b, :n].cpu().numpy()) == bits(logits_b[b, row].cpu().numpy())
        assert bits(reg_a[b, :n].cpu().numpy()) == bits(reg_b[b, row].cpu().numpy())
        full_labels[b, row] = labels_s[b, :n]
        full_deltas[b, row] = deltas_s[b, :n]
    reg_loss_a, cls_loss_a = (float(v) for v in roi_utils.roi_losses(logits_a, reg_a, labels_s, deltas_s))
    reg_loss_b, cls_loss_b = (float(v) for v in roi_utils.roi_losses(logits_b, reg_b, full_labels, full_deltas))
    print("positives", n_pos, "reg", reg_loss_a, reg_loss_b, "cls", cls_loss_a, cls_loss_b)
    assert n_pos > 0 and reg_loss_b > 0 and cls_loss_b > 0
    assert abs(reg_loss_a - reg_loss_b) <= 1e-6 * reg_loss_b and abs(cls_loss_a - cls_loss_b) <= 1e-6 * cls_loss_b
