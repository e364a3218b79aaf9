"""Times the second-stage entries (B = 8, G = 42, C = 21, R in {300, 2000}) in ONE process with HIP events, the variants
interleaved round by round (median and minimum over the rounds):

    targets          rpn_roi_targets (one launch; the (B,R,G) IoU map is never written)
    torch targets    the same assignment written with torch ops: IoU map, argmax, two double argsorts, gather, encode
    losses           rpn_roi_losses, losses only
    losses + grads   rpn_roi_losses with both gradient tensors
    torch losses     torch.nn.functional.cross_entropy + smooth_l1_loss, forward only
    torch loss+grad  the same with .backward() to the logits and the box predictions
    decode + scores  rpn_roi_decode_scores

Prints one table and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/second_stage_bench.py [--rounds 20] [--iters 20] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import roi_utils  # noqa: E402

B, G, C = 8, 42, 21
TOTAL_POS, TOTAL_NEG = 128, 128
VARIANCES = [0.1, 0.1, 0.2, 0.2]


def torch_targets(rois, valid, gt, gt_labels, rpos, rneg, var):
    """The plain restatement a user would write (pos_iou 0.5, neg_iou [0.1, 0.5))."""
    Bn, R, _ = rois.shape
    y1 = torch.maximum(rois[:, :, None, 0], gt[:, None, :, 0])
    x1 = torch.maximum(rois[:, :, None, 1], gt[:, None, :, 1])
    y2 = torch.minimum(rois[:, :, None, 2], gt[:, None, :, 2])
    x2 = torch.minimum(rois[:, :, None, 3], gt[:, None, :, 3])
    inter = (x2 - x1).clamp(min=0) * (y2 - y1).clamp(min=0)
    area = lambda b: (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    iou = inter / (area(rois)[:, :, None] + area(gt)[:, None, :] - inter)                      # (B,R,G)
    iou = torch.where((gt_labels >= 1)[:, None, :], iou, torch.full_like(iou, -1.0))
    best, arg = iou.max(dim=2)
    live = torch.arange(R, device=rois.device)[None, :] < valid[:, None]

    def select(mask, count, prio):
        order = torch.argsort(-(mask.long() * prio.long()), dim=1, stable=True)
        ranks = torch.argsort(order, dim=1, stable=True)
        return mask & (ranks < count[:, None])

    pos = select(live & (best > 0.5), torch.full((Bn,), TOTAL_POS, device=rois.device), rpos)
    neg = select(live & ~pos & (best >= 0.1) & (best < 0.5), TOTAL_POS + TOTAL_NEG - pos.sum(dim=1), rneg)
    labels = torch.where(pos, torch.gather(gt_labels, 1, arg), torch.where(neg, 0, -1)).to(torch.int32)
    m = torch.gather(gt, 1, arg[..., None].expand(-1, -1, 4))
    bw, bh = rois[..., 3] - rois[..., 1], rois[..., 2] - rois[..., 0]
    gw, gh = m[..., 3] - m[..., 1], m[..., 2] - m[..., 0]
    d = torch.stack([((m[..., 0] + 0.5 * gh) - (rois[..., 0] + 0.5 * bh)) / bh, ((m[..., 1] + 0.5 * gw) - (rois[..., 1] + 0.5 * bw)) / bw,
                     torch.log(gh / bh), torch.log(gw / bw)], dim=-1) / var
    return torch.where(pos[..., None], d, torch.zeros_like(d)), labels


def torch_losses(logits, reg, labels, deltas):
    lab = labels.long()
    kept, posm = lab >= 0, lab >= 1
    ce = torch.nn.functional.cross_entropy(logits.flatten(0, 1), torch.where(kept, lab, -100).flatten(), ignore_index=-100,
                                           reduction="sum") / kept.sum().clamp(min=1)
    pred = torch.gather(reg.reshape(*lab.shape, C, 4), 2, lab.clamp(min=0)[..., None, None].expand(-1, -1, 1, 4))[:, :, 0]
    hub = (torch.nn.functional.smooth_l1_loss(pred, deltas, reduction="none", beta=1.0).sum(-1) * posm).sum() / posm.sum().clamp(min=1)
    return hub, ce


def time_variants(variants, rounds, iters):
    """{name: callable} -> {name: (median_us, min_us)}; each round times every variant once (iters calls between two events)."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {n: (float(np.median(v)), float(np.min(v))) for n, v in samples.items()}


def make_inputs(rng, R):
    a = rng.uniform(0.0, 0.6, size=(B, G, 2))
    gt = np.concatenate([a, a + rng.uniform(0.15, 0.4, size=(B, G, 2))], axis=-1).astype(np.float32)
    gt_labels = rng.randint(1, C, size=(B, G)).astype(np.int32)
    gt[:, 30:] = 0.0
    gt_labels[:, 30:] = -1
    pick = gt[np.arange(B)[:, None], rng.randint(0, 30, size=(B, R))]
    hw = np.concatenate([pick[..., 2:] - pick[..., :2]] * 2, axis=-1)
    jitter = np.where((np.arange(R) % 2 == 0)[None, :, None], rng.uniform(-0.08, 0.08, size=(B, R, 4)),
                      rng.uniform(0.2, 0.9, size=(B, R, 1)) * rng.choice([-1.0, 1.0], size=(B, R, 1)))
    rois = (pick + jitter * hw).astype(np.float32)
    cuda = lambda x: torch.from_numpy(x).cuda()
    return dict(rois=cuda(rois), gt=cuda(gt), gt_labels=cuda(gt_labels), valid=torch.full((B,), R - R // 10, dtype=torch.int32, device="cuda"),
                rpos=cuda(rng.randint(1, 2 ** 31 - 1, size=(B, R)).astype(np.int32)),
                rneg=cuda(rng.randint(1, 2 ** 31 - 1, size=(B, R)).astype(np.int32)),
                logits=cuda((3.0 * rng.standard_normal((B, R, C))).astype(np.float32)),
                reg=cuda(rng.standard_normal((B, R, 4 * C)).astype(np.float32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.lib()
    rng = np.random.RandomState(0)
    hp = {"variances": VARIANCES, "total_pos_bboxes": TOTAL_POS, "total_neg_bboxes": TOTAL_NEG}
    _keep, vptr = L.host_floats(VARIANCES)
    var_t = torch.tensor(VARIANCES, device="cuda")
    results = {}
    for R in (300, 2000):
        x = make_inputs(rng, R)
        deltas, labels = roi_utils.calculate_roi_targets(x["rois"], x["gt"], x["gt_labels"], hp, valid=x["valid"], random_pos=x["rpos"],
                                                         random_neg=x["rneg"])
        t_deltas, t_labels = torch_targets(x["rois"], x["valid"], x["gt"], x["gt_labels"], x["rpos"], x["rneg"], var_t)
        # the same assignment (torch may contract or reorder the IoU arithmetic: a candidate on a threshold can move the selection)
        same = labels == t_labels
        assert same.float().mean().item() >= 0.99 and ((deltas - t_deltas).abs().amax(dim=-1) * same).max().item() <= 1e-3
        reg_loss, cls_loss = roi_utils.roi_losses(x["logits"], x["reg"], labels, deltas)
        t_reg, t_cls = torch_losses(x["logits"], x["reg"], labels, deltas)
        assert abs(reg_loss.item() - t_reg.item()) <= 1e-4 * t_reg.item() and abs(cls_loss.item() - t_cls.item()) <= 1e-4 * t_cls.item()
        stream = L.stream_ptr()
        tws_bytes = int(lib.rpn_roi_targets_workspace_bytes(B, R, G))
        lws_bytes = int(lib.rpn_roi_losses_workspace_bytes(B, R, C))
        tws = torch.empty((tws_bytes,), dtype=torch.uint8, device="cuda")
        lws = torch.empty((lws_bytes,), dtype=torch.uint8, device="cuda")
        losses = torch.empty((2,), device="cuda")
        g_logits, g_reg = torch.empty_like(x["logits"]), torch.empty_like(x["reg"])
        boxes = torch.empty((B, R, C, 4), device="cuda")
        scores = torch.empty((B, R, C), device="cuda")
        tl = x["logits"].clone().requires_grad_()
        tr = x["reg"].clone().requires_grad_()

        def torch_loss_and_grad():
            tl.grad = tr.grad = None
            hub, ce = torch_losses(tl, tr, labels, deltas)
            (hub + ce).backward()

        variants = {
            "targets": lambda: lib.rpn_roi_targets(L.ptr(x["rois"]), L.ptr(x["valid"]), L.ptr(x["gt"]), L.ptr(x["gt_labels"]), B, R, G,
                                                   TOTAL_POS, TOTAL_NEG, 0.5, 0.1, 0.5, vptr, L.ptr(x["rpos"]), L.ptr(x["rneg"]),
                                                   L.ptr(deltas), L.ptr(labels), L.ptr(tws), tws_bytes, stream),
            "torch targets": lambda: torch_targets(x["rois"], x["valid"], x["gt"], x["gt_labels"], x["rpos"], x["rneg"], var_t),
            "losses": lambda: lib.rpn_roi_losses(L.ptr(x["logits"]), L.ptr(x["reg"]), L.ptr(labels), L.ptr(deltas), B, R, C, L.ptr(losses),
                                                 None, None, L.ptr(lws), lws_bytes, stream),
            "losses + grads": lambda: lib.rpn_roi_losses(L.ptr(x["logits"]), L.ptr(x["reg"]), L.ptr(labels), L.ptr(deltas), B, R, C,
                                                         L.ptr(losses), L.ptr(g_logits), L.ptr(g_reg), L.ptr(lws), lws_bytes, stream),
            "torch losses": lambda: torch_losses(x["logits"], x["reg"], labels, deltas),
            "torch loss+grad": torch_loss_and_grad,
            "decode + scores": lambda: lib.rpn_roi_decode_scores(L.ptr(x["rois"]), L.ptr(x["valid"]), L.ptr(x["reg"]), L.ptr(x["logits"]),
                                                                 vptr, B, R, C, L.ptr(boxes), L.ptr(scores), stream),
        }
        results["R=%d" % R] = time_variants(variants, args.rounds, args.iters)
    print("%-8s %-16s %10s %10s" % ("shape", "variant", "median us", "min us"))
    for label, row in results.items():
        for name, v in row.items():
            print("%-8s %-16s %10.1f %10.1f" % (label, name, v[0], v[1]))
    line = json.dumps({"B": B, "G": G, "C": C, "rounds": args.rounds, "iters": args.iters, "us_median_min": results})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
