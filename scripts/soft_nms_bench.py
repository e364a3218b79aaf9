"""Times roi_utils.roi_detections with nms = "hard", "linear" and "gaussian" in ONE process, HIP events around the device work, the
variants interleaved inside every round, median of the rounds:

    B = 8, C = 21, R in {300, 2000}, score_threshold in {0.05, 0.001}, max_output_size_per_class 100, max_total_size 300

The head outputs are synthetic: RoIs jittered off 2 gt boxes per class (as scripts/eval_bench.py makes its detections), the gt's class
with a logit from U(-1, 6) against a background logit of 0 and the other classes around -5, small regression deltas -- so that a
class has tens of candidates at 0.05 and several times that at 0.001, as a trained head gives.  `decode` is roi_decode_scores alone
(the part the three share).  The script checks that sigma = inf reproduces the hard path before it prints.  Prints one table (the
README's, between the `soft nms bench` markers) and, last, one JSON line.  Needs a GPU (there is no CPU path).
    python scripts/soft_nms_bench.py [--rounds 5] [--iters 20] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf_rpn_amd import _lib as L  # noqa: E402
from tf_rpn_amd.utils import bbox_utils, roi_utils  # noqa: E402

B, C = 8, 21
VARIANCES = [0.1, 0.1, 0.2, 0.2]
KW = dict(max_output_size_per_class=100, max_total_size=300, iou_threshold=0.5)


def make_inputs(rng, R):
    G = 2 * (C - 1)
    y1, x1 = rng.uniform(0, 0.7, size=(B, G)), rng.uniform(0, 0.7, size=(B, G))
    gt = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.3, size=(B, G)), x1 + rng.uniform(0.1, 0.3, size=(B, G))], axis=-1)
    label = 1 + np.arange(G) % (C - 1)
    pick = rng.randint(0, G, size=(B, R))
    rois = np.take_along_axis(gt, pick[..., None].repeat(4, axis=2), axis=1) + rng.normal(0, 0.03, size=(B, R, 4))
    logits = rng.normal(-5.0, 1.5, size=(B, R, C))
    logits[..., 0] = 0.0
    np.put_along_axis(logits, label[pick][..., None], rng.uniform(-1.0, 6.0, size=(B, R, 1)), axis=2)
    reg = rng.normal(0, 0.3, size=(B, R, 4 * C))
    valid = rng.randint(R - R // 10, R + 1, size=(B,)).astype(np.int32)
    return [torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda() for a in (rois, reg, logits)] + [torch.from_numpy(valid).cuda()]


def interleaved_us(fns, rounds, iters):
    """{name: (median, min)} in microseconds per call; every round times each variant once, in turn"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {name: (float(np.median(v)), float(np.min(v))) for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    L.require_gpu()
    rng = np.random.RandomState(0)
    rows, same = [], True
    for R in (300, 2000):
        rois, reg, logits, valid = make_inputs(rng, R)
        boxes, scores = roi_utils.roi_decode_scores(rois, reg, logits, VARIANCES, valid=valid)
        for thr in (0.05, 0.001):
            cand = (scores > thr).sum(dim=1)[:, 1:].float()                                    # per (image, class >= 1)

            def detect(nms, thr=thr):
                return roi_utils.roi_detections(rois, reg, logits, VARIANCES, valid=valid, score_threshold=thr, nms=nms, sigma=0.5, **KW)

            hard = bbox_utils.non_max_suppression(boxes, scores, score_threshold=thr, return_indices=True, **KW)
            soft = bbox_utils.soft_non_max_suppression(boxes, scores, KW["max_output_size_per_class"], KW["max_total_size"],
                                                       method="gaussian", sigma=float("inf"), iou_threshold=KW["iou_threshold"],
                                                       score_threshold=thr, return_indices=True)
            same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(hard, soft))
            fns = {"decode": lambda: roi_utils.roi_decode_scores(rois, reg, logits, VARIANCES, valid=valid)}
            fns.update({nms: (lambda nms=nms: detect(nms)) for nms in ("hard", "linear", "gaussian")})
            us = interleaved_us(fns, args.rounds, args.iters)
            kept = {nms: float(detect(nms)[3].float().mean()) for nms in ("hard", "linear", "gaussian")}
            rows.append({"R": R, "score_threshold": thr, "candidates_mean": float(cand.mean()), "candidates_max": int(cand.max()),
                         "us_median_min": us, "valid_mean": kept})
    print("roi_detections at B = %d, C = %d, max per class %d, max total %d, IoU threshold %.1f, sigma 0.5; median (min) us of %d rounds x %d calls"
          % (B, C, KW["max_output_size_per_class"], KW["max_total_size"], KW["iou_threshold"], args.rounds, args.iters))
    print("| R | score threshold | candidates per class, mean (max) | decode | hard | linear | gaussian |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %g | %.0f (%d) | %s |" % (r["R"], r["score_threshold"], r["candidates_mean"], r["candidates_max"],
                                               " | ".join("%.1f (%.1f)" % r["us_median_min"][k] for k in ("decode", "hard", "linear", "gaussian"))))
    print("sigma = inf equal to the hard path, bit for bit: %s" % same)
    line = json.dumps({"B": B, "C": C, "rounds": args.rounds, "iters": args.iters, "rows": rows, "inf_sigma_equals_hard": bool(same)})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    print(line)
    assert same


if __name__ == "__main__":
    main()
